"""The linear probe on the MI355X: keep_probe_forward / keep_probe_loss_grad, KEEPModel.probe_predict /
probe_loss_grad / probe_fit / probe_fit_batches, wsi.probe_map and tile_eval.linear_probe.

The yardsticks are the restatements of keep_amd.probe, which tests/test_probe.py holds to per-row Python loops.  A logit is an fp32 fma
chain of length D plus the bias, within (D + 1) 2^-24 (sum |x w| + |b|) of float64; the bound of a probability follows from that through
the softmax (prob_bound below) and is computed from float64 values only.  The accumulators are integers and are
compared exactly with loss_grad_numpy on the probabilities the device wrote; the loss word is held to the float64 loss."""
import ctypes as C_
import math

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel, _lib, tile_eval, wsi
from keep_amd.classmap import ClassRaster, class_raster_numpy, one_hot_numpy
from keep_amd.config import small_shape
from keep_amd.model import _ptr, _stream
from keep_amd.probe import (GRAD_ONE, LOSS_ONE, LinearProbe, ProbeSums, check_class_weight, forward_numpy, kept_numpy, loss_grad_numpy,
                            objective_numpy)
from keep_amd.synth import synth_state_dict
from test_cluster import unit_rows
from test_probe import fit_problem, scipy_optimum

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


@pytest.fixture(scope="module")
def model():
    m = KEEPModel(precision="strict")
    m.load_state_dict(synth_state_dict(small_shape(2, 2), seed=5), strict=True)
    return m.to(DEV).eval()


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                         # a copy: the shared cases are read-only


def prob_bound(x, w, b, p64, z64):
    """The bound of |device probability - float64 probability| per element [N, C], from float64 values:
    L = (D + 1) u max_c(sum |x w_c| + |b_c|) bounds a logit's error, u (max z - min z) the rounding of z - max, 2^-23 the documented 1 ulp
    of expf; numerator and denominator of the softmax each carry 2 L + u R + 2^-23, the sum 7 more roundings and the division one."""
    d = x.shape[1]
    L = (d + 1) * U * (np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)).T + np.abs(b.astype(np.float64))).max(axis=1)
    R = z64.max(axis=1) - z64.min(axis=1)
    rel = 2.0 * (2.0 * L + U * R + 2.0 ** -23) + 8.0 * U
    return p64 * rel[:, None] * 1.01 + 2.0 ** -126


def weights(c, d, seed):
    g = np.random.default_rng(seed)
    return (g.standard_normal((c, d)) * 0.5 / math.sqrt(d)).astype(np.float32), (g.standard_normal(c) * 0.25).astype(np.float32)


# (D, C, N, seed): the seed is one for which the float64 margins leave at most 1 % of the rows under twice the bound (asserted below)
CASES = [(768, 16, 4099, 0), (768, 64, 257, 0), (768, 17, 65, 0), (768, 3, 64, 0), (768, 2, 1, 0), (16, 2, 63, 0), (272, 17, 257, 0),
         (1024, 64, 63, 0), (1024, 2, 64, 0)]
_cases = {}


def case(D, C, N, seed):
    """Unit rows, weights and the float64 forward, computed once and shared (never written to)."""
    key = (D, C, N, seed)
    if key not in _cases:
        x = unit_rows(N, D, 300 + seed)
        w, b = weights(C, D, 400 + seed)
        p, labels, best, margin, z = forward_numpy(x, w, b)
        out = (x, w, b, p, labels, best, margin, z, prob_bound(x, w, b, p, z))
        for a in out:
            a.setflags(write=False)
        _cases[key] = out
    return _cases[key]


@pytest.mark.parametrize("D,C,N,seed", CASES)
def test_forward_matches_float64(model, D, C, N, seed):
    x, w, b, wp, wl, wb, wm, z, bound = case(D, C, N, seed)
    row_bound = bound.max(axis=1)
    sure = wm > 2 * row_bound
    assert (~sure).sum() <= N // 100, f"{(~sure).sum()} of {N} rows under the margin bound: choose another seed"
    labels, probs, margin, skipped = model.probe_predict((dev(w), dev(b)), dev(x), normalize=False)
    assert labels.dtype == torch.int32 and probs.dtype == margin.dtype == torch.float32 and probs.shape == (N, C) and int(skipped) == 0
    gl, gp, gm = labels.cpu().numpy(), probs.cpu().numpy().astype(np.float64), margin.cpu().numpy().astype(np.float64)
    print(f"D={D} C={C} N={N}: left out {(~sure).sum()}, label mismatches {(gl != wl)[sure].sum()}, "
          f"worst prob err / bound {(np.abs(gp - wp) / bound).max():.3g}, margin err / bound {(np.abs(gm - wm) / (2 * row_bound)).max():.3g}")
    assert (gl[sure] == wl[sure]).all() and (gl >= 0).all() and (gl < C).all()
    assert (np.abs(gp - wp) <= bound).all()
    assert (np.abs(gm - wm) <= 2 * row_bound).all()
    assert np.abs(gp.sum(axis=1) - 1).max() <= (C + 8) * U
    # the winner's probability is the row's largest and the margin its lead, in the device's own fp32 values
    srt = np.sort(probs.cpu().numpy(), axis=1)
    assert (probs.cpu().numpy()[np.arange(N), gl] == srt[:, -1]).all() and (margin.cpu().numpy() == srt[:, -1] - srt[:, -2]).all()


def planted(D, C, N, seed):
    """The case's rows with a NaN and a 1.5 planted, labels with a -1 planted, class weights."""
    x, w, b = case(D, C, N, seed)[:3]
    x = x.copy()
    g = np.random.default_rng(seed + 7)
    y = g.integers(0, C, N).astype(np.int32)
    if N >= 8:
        x[1, 3 % D] = np.nan
        x[N - 2, D - 1] = 1.5
        y[4] = -1
        y[N - 1] = -1
    cw = check_class_weight(g.uniform(0.25, 1.0, C), C)
    return x, y, w, b, cw


def run_grad(model, x, y, w, b, cw, sums, groups=0):
    return model.probe_loss_grad(x, y, w, b, sums, class_weight=cw, normalize=False, forward=True, groups=groups)


@pytest.mark.parametrize("D,C,N,seed", CASES)
def test_gradient_words_match_the_restatement_bit_for_bit(model, D, C, N, seed):
    x, y, w, b, cw = planted(D, C, N, seed)
    xd, yd, wd, bd, cwd = dev(x), dev(y), dev(w), dev(b), dev(cw)
    for labels in (y, np.full(N, 1, np.int32)):                          # the planted labels, then all rows of one class
        sums = ProbeSums(C, D, DEV)
        gl, gp, gb, gm = run_grad(model, xd, dev(labels), wd, bd, cwd, sums)
        got, probs = sums.host(), gp.cpu().numpy()
        want = loss_grad_numpy(x, labels, probs, cw)
        assert np.array_equal(got["grad"], want["grad"]) and np.array_equal(got["gbias"], want["gbias"])
        assert np.array_equal(got["counts"], want["counts"]) and got["skipped"] == want["skipped"] == (2 if N >= 8 else 0)
        # the forward outputs of the gradient launch are the forward launch's; an unlabelled row is still predicted
        fl, fp, fm, _ = model.probe_predict((wd, bd), xd, normalize=False)
        assert torch.equal(fl, gl) and torch.equal(fp, gp) and torch.equal(fm, gm)
        if N >= 8:
            assert gl[1] == -1 and gl[N - 2] == -1 and float(gp[1].abs().sum()) == 0 and gl[4] >= 0 and gl[N - 1] >= 0
        kept = kept_numpy(x, labels)
        if kept.any():
            xs = np.where(kept[:, None], x, 0).astype(np.float32)
            z = forward_numpy(xs, w, b)[4][kept]
            yk = labels[kept]
            rows = (np.log(np.exp(z - z.max(1, keepdims=True)).sum(1)) + z.max(1) - z[np.arange(len(yk)), yk])
            loss64 = float((cw[yk].astype(np.float64) * rows).sum())
            tol = kept.sum() * U * (2 * np.abs(z).max() + math.log(C) + 1)
            print(f"D={D} C={C} N={N}: loss word {got['loss'] / LOSS_ONE:.9g} against float64 {loss64:.9g}: off {abs(got['loss'] / LOSS_ONE - loss64):.3g}, "
                  f"allowed {tol:.3g}")
            assert abs(got["loss"] / LOSS_ONE - loss64) <= tol
        else:
            assert got["loss"] == 0


@pytest.mark.parametrize("D,C,N,seed", CASES)
def test_gradient_words_do_not_depend_on_grouping_or_split(model, D, C, N, seed):
    x, y, w, b, cw = planted(D, C, N, seed)
    xd, yd, wd, bd, cwd = dev(x), dev(y), dev(w), dev(b), dev(cw)
    whole = ProbeSums(C, D, DEV)
    first = run_grad(model, xd, yd, wd, bd, cwd, whole)
    assert whole.tiles == N
    again = ProbeSums(C, D, DEV)
    second = run_grad(model, xd, yd, wd, bd, cwd, again)
    assert torch.equal(again.buf, whole.buf) and all(torch.equal(a, c) for a, c in zip(first, second))
    for groups in (1, 2, 4):
        if groups * ((C + 15) // 16) > 8:
            with pytest.raises(ValueError):
                run_grad(model, xd, yd, wd, bd, cwd, ProbeSums(C, D, DEV), groups)
            continue
        s = ProbeSums(C, D, DEV)
        out = run_grad(model, xd, yd, wd, bd, cwd, s, groups)
        assert torch.equal(s.buf, whole.buf), f"groups = {groups}"
        assert all(torch.equal(a, c) for a, c in zip(first, out)), f"groups = {groups}"
    for at in sorted({1, 64, (N // 3) | 1}):
        if at >= N:
            continue
        s = ProbeSums(C, D, DEV)
        a = run_grad(model, xd[:at], yd[:at], wd, bd, cwd, s)
        c = run_grad(model, xd[at:], yd[at:], wd, bd, cwd, s)
        assert s.tiles == N and torch.equal(s.buf, whole.buf), f"split at {at}"
        assert all(torch.equal(torch.cat([u, v]), t) for u, v, t in zip(a, c, first)), f"split at {at}"


FITS = [(300, 48, 3, 0.6), (257, 272, 17, 0.3), (65, 16, 2, 1.0)]
_fits = {}


def fit_case(N, D, C, sep):
    if (N, D, C, sep) not in _fits:
        x, y = fit_problem(N, D, C, sep, 0)
        ws, bs = scipy_optimum(x, y, C, 1e-3)
        for a in (x, y, ws, bs):
            a.setflags(write=False)
        _fits[(N, D, C, sep)] = (x, y, ws, bs)
    return _fits[(N, D, C, sep)]


@pytest.mark.parametrize("N,D,C,sep", FITS)
def test_fit_reaches_the_float64_optimum(model, N, D, C, sep):
    x, y, ws, bs = fit_case(N, D, C, sep)
    l2, gtol = 1e-3, 1e-4
    probe = model.probe_fit(dev(x), dev(y), C, l2=l2, gtol=gtol)
    assert isinstance(probe, LinearProbe) and probe.weight.shape == (C, D) and probe.bias.shape == (C,) and probe.weight.dtype == torch.float32
    w, b = probe.weight.cpu().numpy(), probe.bias.cpu().numpy()
    dw, db = w.astype(np.float64) - ws, (b.astype(np.float64) - b.astype(np.float64).mean()) - bs
    delta = float((np.sqrt((dw * dw).sum(axis=1)) + np.abs(db)).max())
    zs = x.astype(np.float64) @ ws.T + bs
    srt = np.sort(zs, axis=1)
    sure = srt[:, -1] - srt[:, -2] > 4 * delta
    labels, _, _, _ = model.probe_predict(probe, dev(x))
    gl = labels.cpu().numpy()
    f, gw, gb = objective_numpy(x, y, w, b, l2)
    gnorm = max(np.abs(gw).max(), np.abs(gb).max())
    # the evaluation error of the gradient: the probabilities' bound averaged over the rows (|x| <= 1), one
    # rounding of each term (2^-24 + 2^-31), and the penalty taken at the float64 parameters the fp32 ones were rounded from
    p64, _, _, _, z64 = forward_numpy(x, w, b)
    e_grad = float(prob_bound(x, w, b, p64, z64).mean(axis=0).max()) + 2.0 ** -24 + 2.0 ** -31 + l2 * U * float(np.abs(w).max())
    print(f"N={N} D={D} C={C}: {probe.n_iter} iterations, {probe.n_eval} evaluations, {probe.stop_reason}; delta {delta:.3g}, under the margin "
          f"{(~sure).sum()}, label mismatches {(gl != zs.argmax(1))[sure].sum()}; |grad|inf device {probe.grad_norm:.3g}, float64 {gnorm:.3g} "
          f"(evaluation error allowed {e_grad:.3g}); objective {probe.loss:.9g} against float64 {f:.9g}")
    assert (~sure).sum() <= N * 5 // 100
    assert (gl[sure] == zs.argmax(axis=1)[sure]).all()
    assert gnorm <= gtol + e_grad
    assert probe.converged and probe.stop_reason == "converged" and probe.grad_norm <= gtol
    assert probe.counts.cpu().tolist() == np.bincount(y, minlength=C).tolist() and probe.skipped == 0
    again = model.probe_fit(dev(x), dev(y), C, l2=l2, gtol=gtol)
    assert torch.equal(again.weight, probe.weight) and torch.equal(again.bias, probe.bias) and again.n_eval == probe.n_eval
    cuts = [0, N // 5, N // 5 + N // 2 + 1, N]
    parts = model.probe_fit_batches(lambda: [(dev(x[a:c]), y[a:c]) for a, c in zip(cuts, cuts[1:])], C, D, l2=l2, gtol=gtol)
    assert torch.equal(parts.weight, probe.weight) and torch.equal(parts.bias, probe.bias) and parts.loss == probe.loss
    assert parts.n_iter == probe.n_iter and parts.n_eval == probe.n_eval


def test_fit_with_balanced_weights_and_left_out_rows(model):
    x, y = fit_problem(240, 48, 3, 0.6, 1)
    x, y = x.copy(), y.copy()
    y[:100] = 0
    y[[3, 200]] = -1
    x[7, 0] = np.nan
    probe = model.probe_fit(dev(x), y.astype(np.int64), 3, class_weight="balanced", classes=("a", "b", "c"))
    counts = np.bincount(y[y >= 0], minlength=3)
    assert np.array_equal(probe.class_weight, check_class_weight("balanced", 3, counts)) and probe.classes == ("a", "b", "c")
    kept = kept_numpy(x, y)
    assert probe.skipped == 1 and probe.counts.cpu().tolist() == np.bincount(y[kept], minlength=3).tolist() and probe.converged
    xs = np.where(kept[:, None], x, 0).astype(np.float32)
    ys = np.where(kept, y, -1).astype(np.int32)
    f, gw, gb = objective_numpy(xs, ys, probe.weight.cpu().numpy(), probe.bias.cpu().numpy(), probe.l2, probe.class_weight)
    assert abs(f - probe.loss) < 1e-5 and max(np.abs(gw).max(), np.abs(gb).max()) < 2e-4
    stalled = model.probe_fit(dev(x), y.astype(np.int64), 3, gtol=1e-12, max_iter=300)
    print(f"gtol 1e-12: {stalled.stop_reason} after {stalled.n_iter} iterations, |grad|inf {stalled.grad_norm:.3g}")
    assert not stalled.converged and stalled.stop_reason in ("stalled", "max_iter")


def test_probe_map_rasterises_the_probabilities(model):
    gw, gh, P, d, C = 12, 9, 256, 16, 3
    shape = (gh * P // d, gw * P // d)
    x, y = fit_problem(gw * gh, 768, C, 0.3, 3)
    x = x.copy()
    coords = np.stack([np.arange(gw * gh) % gw * P, np.arange(gw * gh) // gw * P], axis=1).astype(np.int64)
    probe = model.probe_fit(dev(x), y, C, classes=("n", "t", "s"))
    nan_tile = 50
    x[nan_tile, 3] = np.nan
    labels, probs, margin, skipped = model.probe_predict(probe, dev(x))
    gl = labels.cpu().numpy()
    keep = gl >= 0
    assert int(skipped) == 1 and not keep[nan_tile] and keep.sum() == gw * gh - 1
    raster = wsi.probe_map(probe, dev(x), torch.from_numpy(coords), d, shape, patch_size=P, model=model)
    assert isinstance(raster, ClassRaster) and raster.n_classes == C and raster.shape == shape and raster.classes == ("n", "t", "s")
    want = class_raster_numpy(coords[keep], probs.cpu().numpy()[keep], P, d, shape)
    assert torch.equal(raster.acc.cpu(), torch.from_numpy(want))
    votes = wsi.probe_map((probe.weight, probe.bias), dev(x), coords, d, shape, patch_size=P, vote=True, model=model)
    assert torch.equal(votes.acc.cpu(), torch.from_numpy(class_raster_numpy(coords[keep], one_hot_numpy(gl[keep], C), P, d, shape)))
    cm = model.class_map(raster)
    y0, x0 = coords[nan_tile, 1] // d, coords[nan_tile, 0] // d
    assert (cm.labels[y0:y0 + P // d, x0:x0 + P // d] == 255).all()
    assert sorted(wsi.subtype_regions(cm, model=model)) == list(range(C))


def test_linear_probe_protocol_matches_sklearns_metrics(model):
    from sklearn.metrics import balanced_accuracy_score, confusion_matrix, f1_score
    C = 4
    x, y = fit_problem(400, 48, C, 0.35, 5)
    res = tile_eval.linear_probe(model, dev(x[:250]), y[:250], dev(x[250:]), y[250:], C, n_boot=50, seed=3)
    pred = res["labels"].cpu().numpy()
    truth = y[250:]
    assert (pred >= 0).all() and res["skipped"] == 0 and 0.3 < res["balanced_accuracy"] < 1.0
    assert np.array_equal(res["confusion"], confusion_matrix(truth, pred, labels=list(range(C))))
    assert abs(res["balanced_accuracy"] - balanced_accuracy_score(truth, pred)) < 1e-12
    assert abs(res["weighted_f1"] - f1_score(truth, pred, average="weighted")) < 1e-12
    assert res["balanced_accuracy_ci"].estimate == pytest.approx(res["balanced_accuracy"], abs=1e-12)
    assert res["weighted_f1_ci"].estimate == pytest.approx(res["weighted_f1"], abs=1e-12)
    per_class, macro = res["ovr_roc"]
    assert len(per_class) == C and 0.5 < macro.estimate <= 1.0


def test_abi_errors_launch_nothing(model):
    lib, h, st = _lib.load(), model._handle, _stream(torch.device(DEV))
    N, D, C = 8, 32, 3
    x = dev(unit_rows(N, D, 0))
    w, b = (dev(a) for a in weights(C, D, 1))
    y = torch.zeros(N, dtype=torch.int32, device=DEV)
    probs = torch.full((N, C), 7.0, dtype=torch.float32, device=DEV)
    labels = torch.full((N,), 77, dtype=torch.int32, device=DEV)
    sums = ProbeSums(C, D, DEV)
    sums.buf.fill_(5)
    null = C_.c_void_p(0)
    off = lambda t, n: C_.c_void_p(t.data_ptr() + n)

    def forward(h_=h, x_=_ptr(x), n=N, d=D, w_=_ptr(w), b_=_ptr(b), c=C, p=_ptr(probs), l=_ptr(labels), groups=0):
        return lib.keep_probe_forward(h_, x_, n, d, w_, b_, c, p, l, null, null, null, groups, st)

    def grad(h_=h, x_=_ptr(x), n=N, d=D, y_=_ptr(y), w_=_ptr(w), c=C, cw=null, g=_ptr(sums.grad), loss=_ptr(sums.loss), groups=0):
        return lib.keep_probe_loss_grad(h_, x_, n, d, y_, w_, _ptr(b), c, cw, g, _ptr(sums.gbias), loss, _ptr(sums.counts), _ptr(sums.skipped),
                                        _ptr(probs), _ptr(labels), null, null, groups, st)

    y_bad = y.clone()
    y_bad[5] = C                                                         # a label equal to C
    y_low = y.clone()
    y_low[2] = -2
    cw_bad = torch.tensor([1.0, 0.0, 0.5], dtype=torch.float32, device=DEV)
    bad = [lambda: forward(c=1), lambda: forward(c=65), lambda: forward(d=24), lambda: forward(d=1040), lambda: forward(n=0),
           lambda: forward(n=(1 << 22) + 1), lambda: forward(x_=null), lambda: forward(w_=null), lambda: forward(b_=null),
           lambda: forward(x_=off(x, 4)), lambda: forward(w_=off(w, 8)), lambda: forward(p=off(probs, 2)), lambda: forward(p=null, l=null),
           lambda: forward(groups=3), lambda: grad(c=1), lambda: grad(d=24), lambda: grad(y_=null), lambda: grad(y_=off(y, 2)),
           lambda: grad(x_=off(x, 4)), lambda: grad(g=null), lambda: grad(loss=off(sums.loss, 4)), lambda: grad(groups=8),
           lambda: grad(y_=_ptr(y_bad)), lambda: grad(y_=_ptr(y_low)), lambda: grad(cw=_ptr(cw_bad))]
    for i, call in enumerate(bad):
        assert call() == _lib.KEEP_EINVAL, f"bad call {i}"
        assert len(lib.keep_last_error(h)) > 10, f"bad call {i}"
    assert forward(h_=None) == _lib.KEEP_EINVAL and grad(h_=None) == _lib.KEEP_EINVAL
    torch.cuda.synchronize()
    assert (probs == 7.0).all() and (labels == 77).all() and (sums.buf == 5).all()
    # and the same arguments, sound, go through
    assert forward() == _lib.KEEP_OK and grad() == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert (labels >= 0).all() and (labels < C).all() and not (sums.buf == 5).all()
    with pytest.raises(ValueError):
        model.probe_loss_grad(x, y_bad, w, b, ProbeSums(C, D, DEV), normalize=False)
