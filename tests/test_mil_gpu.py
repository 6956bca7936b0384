"""Attention MIL on the MI355X: keep_mil_forward / keep_mil_backward, KEEPModel.mil_forward / mil_loss_grad /
mil_predict / mil_fit / mil_fit_batches, wsi.mil_attention_map and tile_eval.attention_mil.

The yardsticks are the float64 restatements of keep_amd.mil, which tests/test_mil.py holds to central differences.  Every bound is
computed from float64 values (forward) or from the operands the device itself read (backward), never from the output under test; the
derivations are DESIGN.md section 29 and the docstrings of forward_bounds / ds_bound below.  u = 2^-24; expf is taken at its documented
1 ulp, as in section 27, and tanhf at 2 ulp (the HIP math API documents no more)."""
import ctypes as C_

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel, _lib, mil, probe, tile_eval, wsi
from keep_amd.cluster import skipped_numpy
from keep_amd.config import small_shape
from keep_amd.mil import CHUNK, GRAD_ONE, MilSums, chunk_table, forward_numpy, key_share, synthetic_cohort
from keep_amd.model import _ptr, _stream
from keep_amd.synth import synth_state_dict
from test_mil import (BAD_BAG, BAG_SIZES, EMPTY_BAG, FIT, FIT_SHARE_FLOAT64, NAN_BAG, UNLABELLED_BAG, cohort, params32)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
TANH_ULP, EXP_ULP = 2.0, 1.0
CHAIN = 1.5e-7                       # the fp32 MFMA chain against float64, per unit of sum |a b|, at K <= 1024
# the share of positive bags whose most-attended tile is a key tile: the float64 fit reaches FIT_SHARE_FLOAT64 = 1.0 (test_mil.py); the
# device fit reached 1.0 on its first run; the margin is one bag of the 32, for the fp32 evaluation
FIT_SHARE_MARGIN = 1.0 / 32
SHAPES = [(48, 16, 2), (272, 48, 3), (768, 128, 4)]


@pytest.fixture(scope="module")
def model():
    m = KEEPModel(precision="strict")
    m.load_state_dict(synth_state_dict(small_shape(2, 2), seed=5), strict=True)
    return m.to(DEV).eval()


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                         # a copy: the shared cases are read-only


def class_weights(C):
    return (1.0 / (1.0 + np.arange(C))).astype(np.float32)              # 1, 1/2, 1/3, ...: in (0, 1], the largest 1


def forward_bounds(x, o, params, f):
    """Bounds of |device - float64| for h [N, L], s [N], a [N], z [S, D], the logits [S] and the probabilities [S, C], from the float64
    forward ``f``.  t = V x + bv is an fma chain of D terms plus one addition: (D + 1) u (sum |x V| + |bv|); tanh has slope <= 1, tanhf 2
    ulp: Eh = Et + 2 x 2^-23 |h|; s adds L / 16 fma and 4 tree additions: Es = |w| . Eh + (L / 16 + 5) u |w| . |h|.  The attention is a ratio,
    so a shift of every score of a bag cancels: with Eb the largest Es of the bag and R its score range, e_i carries exp's 1 ulp and the
    rounding u R of s - m, Z the n 2^-41 of its fixed point, fp32(Z) and the division one rounding each:
    rel_a = 2 Eb + 2 (2^-23 + u (R + 2 Eb)) + n 2^-41 + 3 u.  z: every term e x is rounded once (u) and once to 2^-40, the quotient once:
    Ez = (rel_a + 2 u) sum a |x| + n 2^-41 + u |z|.  The logits: the probe's chain bound plus |Wc| . Ez; the probabilities as in section 27."""
    V, bv, w, Wc, bc = (np.asarray(a, np.float64) for a in params)
    D, L = x.shape[1], V.shape[0]
    skip = skipped_numpy(x)
    ax = np.where(skip[:, None], 0.0, np.abs(x.astype(np.float64)))
    ah = np.abs(f["h"])
    Eh = (D + 1) * U * (ax @ np.abs(V).T + np.abs(bv)) + TANH_ULP * 2.0 ** -23 * ah
    Es = Eh @ np.abs(w) + (L // 16 + 5) * U * (ah @ np.abs(w))
    S = len(o) - 1
    rel_a, Ez = np.zeros(S), np.zeros((S, D))
    Ea = np.zeros(x.shape[0])
    for b in range(S):
        rows = np.arange(o[b], o[b + 1])[~skip[o[b]:o[b + 1]]]
        if rows.size == 0:
            continue
        Eb = Es[rows].max()
        R = f["s"][rows].max() - f["s"][rows].min() + 2.0 * Eb
        rel_a[b] = 1.01 * (2.0 * Eb + 2.0 * (EXP_ULP * 2.0 ** -23 + U * R) + rows.size * 2.0 ** -41 + 3.0 * U)
        Ea[rows] = f["a"][rows] * rel_a[b] + 2.0 ** -120
        Ez[b] = 1.01 * ((rel_a[b] + 2.0 * U) * (f["a"][rows, None] * ax[rows]).sum(axis=0) + rows.size * 2.0 ** -41 + U * np.abs(f["z"][b]))
    Elog = (D + 1) * U * (np.abs(f["z"]) @ np.abs(Wc).T + np.abs(bc)).max(axis=1) + (Ez @ np.abs(Wc).T).max(axis=1)
    Rl = f["logits"].max(axis=1) - f["logits"].min(axis=1)
    Ep = f["probs"] * (2.0 * (2.0 * Elog + U * Rl + 2.0 ** -23) + 8.0 * U)[:, None] * 1.01 + 2.0 ** -126
    return dict(h=Eh * 1.01 + 2.0 ** -126, s=Es * 1.01, a=Ea, z=Ez, logits=Elog, probs=Ep)


_cases = {}


def case(D, L, C):
    """The cohort, parameters, float64 forward and its bounds, computed once and shared (never written to)."""
    if (D, L, C) not in _cases:
        x, o, y = cohort(D, C)
        p = params32(D, L, C, 0)
        mil.check_params(p, D)
        f = forward_numpy(x, o, p)
        _cases[(D, L, C)] = (x, o, y, p, f, forward_bounds(x, o, p, f))
    return _cases[(D, L, C)]


def evaluate(model, x, o, y, p, C, sums=None, **kw):
    L, D = p[0].shape
    sums = MilSums(L, C, D, DEV) if sums is None else sums
    out = model.mil_loss_grad(dev(x), o, dev(y), tuple(dev(a) for a in p), sums, dev(class_weights(C)), normalize=False, **kw)
    return sums, out


@pytest.mark.parametrize("D,L,C", SHAPES)
def test_forward_matches_float64(model, D, L, C):
    x, o, y, p, f, E = case(D, L, C)
    out = model.mil_forward(dev(x), o, tuple(dev(a) for a in p), normalize=False, hidden=True)
    skip = skipped_numpy(x)
    s, a, z, h = (out[k].cpu().numpy().astype(np.float64) for k in ("scores", "attention", "pooled", "hidden"))
    assert np.array_equal(np.isneginf(s), skip) and not a[skip].any()
    err_h = np.abs(h - f["h"])[~skip]
    err_s, err_a, err_z = np.abs(s[~skip] - f["s"][~skip]), np.abs(a - f["a"]), np.abs(z - f["z"])
    print(f"h {err_h.max():.3e} of {E['h'][~skip].max():.3e}; s {err_s.max():.3e} of {E['s'][~skip].max():.3e}; a/bound "
          f"{(err_a / E['a'].clip(1e-300)).max():.3f}; z/bound {(err_z / E['z'].clip(1e-300)).max():.3f}")
    assert (err_h <= E["h"][~skip]).all()
    assert (err_s <= E["s"][~skip]).all()
    assert (err_a <= E["a"]).all()
    assert (err_z <= E["z"]).all()
    assert out["kept_rows"].cpu().numpy().tolist() == f["kept_rows"].tolist()
    assert out["skipped"].cpu().tolist() == [f["skipped_rows"], f["skipped_bags"]]
    labels, probs, attention, skipped = model.mil_predict(tuple(dev(a_) for a_ in p), dev(x), o, normalize=False)
    assert torch.equal(attention, out["attention"]) and skipped.cpu().tolist() == [f["skipped_rows"], f["skipped_bags"]]
    err_p = np.abs(probs.cpu().numpy().astype(np.float64) - f["probs"])
    print(f"p/bound {(err_p / E['probs']).max():.3f}")
    assert (err_p <= E["probs"]).all()
    top2 = np.sort(f["logits"], axis=1)[:, -2:]
    kept = f["labels"] >= 0
    assert ((top2[:, 1] - top2[:, 0])[kept] > 2.0 * E["logits"][kept]).all()           # no bag is left out of the label comparison
    assert labels.cpu().numpy().tolist() == f["labels"].tolist()


def ds_bound(x, o, hl, cw, Wc, a, z, probs):
    """float64 ds from the operands the device read (its own attention a, pooled rows z and head probabilities, all fp32) and the bound
    of the device's ds against it -> (ds64 [N], bound [N]).  r is formed as the probe forms it, exactly.  dz is an fma chain over C
    terms: Edz = C u |r| . |Wc|; u_b is at most 4 fma per thread, 6 tree additions and 3 more: Eu = Edz . |z| + 13 u |dz| . |z|; da is D / 64
    fma per lane and 6 tree additions: Eda = Edz . |x| + (D / 64 + 6) u |dz| . |x|; ds = a (da - u) rounds twice."""
    D, C = x.shape[1], Wc.shape[0]
    kept = hl >= 0
    yk = np.where(kept, hl, 0)
    onehot = np.zeros_like(probs)
    onehot[np.arange(len(hl)), yk] = 1.0
    r = (cw[yk][:, None] * (probs - onehot)).astype(np.float32)         # fp32: the subtraction, then the product
    r[~kept] = 0.0
    r64, Wc64, z64 = r.astype(np.float64), Wc.astype(np.float64), z.astype(np.float64)
    skip = skipped_numpy(x)
    x64 = np.where(skip[:, None], 0.0, x.astype(np.float64))
    bag = np.repeat(np.arange(len(o) - 1), np.diff(o))
    dz = r64 @ Wc64
    Edz = C * U * (np.abs(r64) @ np.abs(Wc64))
    u = (dz * z64).sum(axis=1)
    Eu = (Edz * np.abs(z64)).sum(axis=1) + 13 * U * (np.abs(dz) * np.abs(z64)).sum(axis=1)
    da = (dz[bag] * x64).sum(axis=1)
    Eda = (Edz[bag] * np.abs(x64)).sum(axis=1) + (D // 64 + 6) * U * (np.abs(dz[bag]) * np.abs(x64)).sum(axis=1)
    a64 = a.astype(np.float64)
    ds = a64 * (da - u[bag])
    return ds, 1.01 * (a64 * (Eda + Eu[bag]) + 2.0 * U * a64 * (np.abs(da) + np.abs(u[bag]))) + 2.0 ** -140


@pytest.mark.parametrize("D,L,C", SHAPES)
def test_gradient_words_match_float64(model, D, L, C):
    x, o, y, p, f, E = case(D, L, C)
    cw = class_weights(C)
    sums, out = evaluate(model, x, o, y, p, C, detail=True)
    words = sums.host()
    hl = out["head_labels"].cpu().numpy()
    assert hl.tolist() == [(-1 if f["kept_rows"][b] == 0 else int(y[b])) for b in range(len(y))]
    a, z, probs, h, ds = (out[k].cpu().numpy() for k in ("attention", "pooled", "probs", "hidden", "ds"))
    # the head: the probe's own words, exactly, from the pooled rows and probabilities the device wrote
    want = probe.loss_grad_numpy(z, hl, probs, cw)
    assert np.array_equal(words["head"]["grad"], want["grad"]) and np.array_equal(words["head"]["gbias"], want["gbias"])
    assert np.array_equal(words["head"]["counts"], want["counts"]) and words["head"]["skipped"] == 0
    assert words["skipped_rows"] == f["skipped_rows"] and words["skipped_bags"] == f["skipped_bags"]
    kept = hl >= 0
    lg = f["logits"]
    lse = np.log(np.exp(lg - lg.max(axis=1, keepdims=True)).sum(axis=1)) + lg.max(axis=1)
    zy = lg[np.arange(len(y)), np.where(kept, hl, 0)]
    loss64 = (cw.astype(np.float64)[np.where(kept, hl, 0)] * (lse - zy))[kept].sum()
    loss_bound = (2.0 * E["logits"] + 8.0 * U * (np.abs(lse) + np.abs(zy)) + 2.0 ** -25)[kept].sum()
    print(f"loss {abs(words['head']['loss'] / probe.LOSS_ONE - loss64):.3e} of {loss_bound:.3e}")
    assert abs(words["head"]["loss"] / probe.LOSS_ONE - loss64) <= loss_bound
    # ds against float64 from the same operands
    ds64, Eds = ds_bound(x, o, hl, cw, p[3], a, z, probs)
    err = np.abs(ds.astype(np.float64) - ds64)
    print(f"ds/bound {(err / Eds).max():.3f}; max |ds| {np.abs(ds64).max():.3e}")
    assert (err <= Eds).all()
    bag = np.repeat(np.arange(len(o) - 1), np.diff(o))
    assert not ds[~kept[bag]].any() and not ds[skipped_numpy(x)].any()
    # the words against the float64 sums of the residuals the device formed: R in fp32 as the kernel stages it
    on = kept[bag] & ~skipped_numpy(x)
    w32 = p[2]
    R = ((ds[:, None] * w32[None, :]).astype(np.float32) * (np.float32(1.0) - (h * h).astype(np.float32)).astype(np.float32)).astype(np.float32)
    R[~on] = 0.0
    R64 = R.astype(np.float64)
    x64 = np.where(on[:, None], x.astype(np.float64), 0.0)
    table = chunk_table(o)
    n_chunks = int(kept[table[:, 0]].sum())
    gV = words["gV"].astype(np.float64) / GRAD_ONE
    bound_V = CHAIN * (np.abs(R64).T @ np.abs(x64)) + n_chunks * 2.0 ** -37      # the chain of every chunk, and one rounding per chunk
    err_V = np.abs(gV - R64.T @ x64)
    print(f"gV/bound {(err_V / bound_V).max():.3f}; max |gV| {np.abs(gV).max():.3e}")
    assert (err_V <= bound_V).all()
    n_terms = int(on.sum())
    gbv = words["gbv"].astype(np.float64) / GRAD_ONE
    assert (np.abs(gbv - R64.sum(axis=0)) <= n_terms * (U * np.abs(R64).max() + 2.0 ** -37)).all()
    G64 = np.where(on[:, None], ds.astype(np.float64)[:, None] * h.astype(np.float64), 0.0)
    gw = words["gw"].astype(np.float64) / GRAD_ONE
    assert (np.abs(gw - G64.sum(axis=0)) <= n_terms * (U * np.abs(G64).max() + 2.0 ** -37)).all()
    assert np.abs(gV).max() > 1e-4 and np.abs(gbv).max() > 1e-5 and np.abs(gw).max() > 1e-5        # a gradient, not zeros


def take_bags(x, o, y, bags):
    """The cohort of the listed bags, in that order."""
    xs = [x[o[b]:o[b + 1]] for b in bags]
    sizes = [len(a) for a in xs]
    return np.concatenate(xs) if sum(sizes) else x[:0], np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), y[list(bags)]


@pytest.mark.parametrize("D,L,C", SHAPES)
def test_words_do_not_depend_on_the_split_or_the_order(model, D, L, C):
    x, o, y, p, f, E = case(D, L, C)
    whole, _ = evaluate(model, x, o, y, p, C)
    again, _ = evaluate(model, x, o, y, p, C)
    assert torch.equal(whole.buf, again.buf)
    S = len(y)
    split = MilSums(L, C, D, DEV)
    for part in (range(0, 2), range(2, 7), range(7, S)):                   # three uneven calls; the last starts with the empty bag
        evaluate(model, *take_bags(x, o, y, list(part)), p, C, sums=split)
    assert split.bags == S and torch.equal(whole.buf, split.buf)
    perm = np.random.default_rng(5).permutation(S)
    assert not np.array_equal(perm, np.arange(S))
    mixed, _ = evaluate(model, *take_bags(x, o, y, list(perm)), p, C)
    assert torch.equal(whole.buf, mixed.buf)
    shuffled = MilSums(L, C, D, DEV)
    for part in (perm[7:], perm[:3], perm[3:7]):
        evaluate(model, *take_bags(x, o, y, list(part)), p, C, sums=shuffled)
    assert torch.equal(whole.buf, shuffled.buf)


def test_skip_and_leave_out_rules(model):
    D, L, C = SHAPES[1]
    x, o, y, p, f, E = case(D, L, C)
    whole, (labels, probs, attention) = evaluate(model, x, o, y, p, C, forward=True)
    words = whole.host()
    assert words["skipped_rows"] == 1 + BAG_SIZES[BAD_BAG] and words["skipped_bags"] == 2
    assert int(words["head"]["counts"].sum()) == len(y) - 3                # the empty bag, the out-of-range bag and the one labelled -1
    assert labels.cpu().numpy().tolist() == f["labels"].tolist() and labels[UNLABELLED_BAG] >= 0
    for b in (EMPTY_BAG, BAD_BAG):
        assert labels[b] == -1 and not probs[b].any() and not attention[o[b]:o[b + 1]].any()
    assert attention[o[NAN_BAG] + 3] == 0 and abs(float(attention[o[NAN_BAG]:o[NAN_BAG + 1]].sum()) - 1.0) < 1e-5
    # a skipped bag's label, the contents of a skipped row and everything about the bag labelled -1 change no word
    x2, y2 = x.copy(), y.copy()
    y2[EMPTY_BAG], y2[BAD_BAG] = (y[EMPTY_BAG] + 1) % C, (y[BAD_BAG] + 1) % C
    x2[o[NAN_BAG] + 3, :4] = 0.25
    x2[o[BAD_BAG]:o[BAD_BAG + 1], 2:] = -7.0
    x2[o[UNLABELLED_BAG]:o[UNLABELLED_BAG + 1]] = x[o[1]:o[1] + BAG_SIZES[UNLABELLED_BAG]]
    other, _ = evaluate(model, x2, o, y2, p, C)
    assert torch.equal(whole.buf, other.buf)
    y3 = y.copy()
    y3[UNLABELLED_BAG] = 0                                                 # labelled after all: now it is in the sums
    third, _ = evaluate(model, x, o, y3, p, C)
    assert not torch.equal(whole.gV, third.gV) and int(third.head.counts.sum()) == len(y) - 2


def fit_cohort():
    return synthetic_cohort(0)


def test_fit(model):
    x, o, y, key = fit_cohort()
    fitted = model.mil_fit(dev(x), o, y, 2, **FIT)
    assert fitted.n_steps == FIT["n_steps"] and len(fitted.loss_history) == FIT["n_steps"] + 1 and np.isfinite(fitted.grad_norm)
    assert fitted.loss_history[-1] < fitted.loss_history[0] and fitted.loss == fitted.loss_history[-1]
    labels, probs, attention, skipped = model.mil_predict(fitted, dev(x), o)
    assert labels.cpu().numpy().tolist() == y.tolist() and skipped.cpu().tolist() == [0, 0]
    share = key_share(attention.cpu().numpy(), o, y, key)
    print(f"loss {fitted.loss_history[0]:.4f} -> {fitted.loss:.4f}; |grad|inf {fitted.grad_norm:.2e}; key share {share:.4f}")
    assert share >= FIT_SHARE_FLOAT64 - FIT_SHARE_MARGIN


def test_fit_batches_gives_the_bits_of_the_resident_fit(model):
    x, o, y, key = fit_cohort()
    args = dict(FIT, n_steps=12)
    whole = model.mil_fit(dev(x), o, y, 2, class_weight="balanced", **args)
    again = model.mil_fit(dev(x), o, y, 2, class_weight="balanced", **args)
    S = len(y)
    order = [list(range(40, S)), list(range(0, 9)), list(range(9, 40))]

    def batches():
        for part in order:
            xs, os_, ys = take_bags(x, o, y, part)
            yield torch.from_numpy(xs), os_, ys
    streamed = model.mil_fit_batches(batches, 2, x.shape[1], class_weight="balanced", **args)
    for a, b, c in zip(whole.params, again.params, streamed.params):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert whole.loss_history == again.loss_history == streamed.loss_history and whole.grad_norm == streamed.grad_norm
    assert torch.equal(whole.counts, streamed.counts)


def test_attention_map_is_tile_raster_of_the_attention(model):
    D, L, C = SHAPES[0]
    x, o, y, p, f, E = case(D, L, C)
    rows = slice(int(o[NAN_BAG]), int(o[NAN_BAG + 1]))                      # one slide of 7 tiles, one of them skipped
    feats = dev(x[rows])
    n = feats.shape[0]
    coords = torch.stack([torch.arange(n) % 4 * 256, torch.arange(n) // 4 * 256], dim=1)
    pd = tuple(dev(a) for a in p)
    raster = wsi.mil_attention_map(pd, feats, coords, 16, (32, 64), patch_size=256, model=model)
    out = model.mil_forward(feats, np.array([0, n]), pd)
    keep = out["scores"] > float("-inf")
    assert int(keep.sum()) == n - 1
    a = out["attention"][keep]
    want = model.tile_raster(coords.to(DEV)[keep], a / a.max(), 256, 16, (32, 64), (0, 0))
    assert torch.equal(raster.acc, want.acc) and raster.tiles == want.tiles == n - 1
    assert float((a / a.max()).max()) == 1.0


def test_attention_mil_protocol(model):
    x, o, y, key = fit_cohort()
    xt, ot, yt, _ = synthetic_cohort(1, n_bags=24)
    res = tile_eval.attention_mil(model, (dev(x), o), y, (dev(xt), ot), yt, 2, hidden=FIT["hidden"], l2=FIT["l2"], lr=FIT["lr"], n_steps=40,
                                  n_boot=50)
    labels, probs, attention, _ = model.mil_predict(res["mil"], dev(xt), ot)
    assert torch.equal(labels, res["labels"]) and torch.equal(probs, res["probs"]) and torch.equal(attention, res["attention"])
    conf = np.zeros((2, 2), np.int64)
    np.add.at(conf, (yt, labels.cpu().numpy()), 1)
    assert np.array_equal(res["confusion"], conf) and conf.sum() == 24
    assert res["skipped"] == 0 and res["balanced_accuracy_ci"] is not None and res["ovr_roc"] is not None
    assert 0.0 <= res["balanced_accuracy"] <= 1.0


def test_abi_errors_launch_nothing(model):
    D, L, C = SHAPES[0]
    x, o, y, p, f, E = case(D, L, C)
    lib, h, st = _lib.load(), model._handle, _stream(torch.device(DEV))
    N, S = x.shape[0], len(y)
    xd, (V, bv, w, Wc, bc) = dev(x), tuple(dev(a) for a in p)
    good = chunk_table(o)
    need = C_.c_int64(0)
    assert lib.keep_mil_workspace_bytes(h, N, D, S, C_.byref(need)) == 0 and need.value > N * 4
    assert lib.keep_mil_workspace_bytes(h, N, D, S, None) == _lib.KEEP_EINVAL
    assert lib.keep_mil_workspace_bytes(h, N, D, 0, C_.byref(need)) == _lib.KEEP_EINVAL
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    s_out, a_out = torch.full((N,), 7.0, device=DEV), torch.full((N,), 7.0, device=DEV)
    z_out, kept = torch.full((S, D), 7.0, device=DEV), torch.full((S,), 7, dtype=torch.int32, device=DEV)
    hid = torch.full((N, L), 7.0, device=DEV)
    skipped = torch.zeros(2, dtype=torch.int64, device=DEV)

    def forward(table=good, L_=L, ws_=ws, nbytes=None, s_=s_out, S_=S):
        t = dev(np.ascontiguousarray(table))
        return lib.keep_mil_forward(h, _ptr(xd), N, D, _ptr(t), t.shape[0], S_, None, _ptr(V), _ptr(bv), _ptr(w), L_, _ptr(s_), _ptr(a_out), _ptr(z_out),
                                    _ptr(kept), _ptr(hid), None, _ptr(skipped[0:1]), _ptr(skipped[1:2]), _ptr(ws_), need.value if nbytes is None else nbytes,
                                    st)

    def untouched():
        torch.cuda.synchronize()
        return bool((s_out == 7).all() and (a_out == 7).all() and (z_out == 7).all() and (kept == 7).all() and (hid == 7).all() and not skipped.any())

    for row, bad in ((0, (S, 0, 1)), (0, (-1, 0, 1)), (3, (3, N - 1, 2)), (3, (3, -1, 2)), (2, (2, 64, 0)), (2, (2, 64, CHUNK + 1))):
        t = good.copy()
        t[row] = bad
        assert forward(table=t) == _lib.KEEP_EINVAL and untouched(), bad
    assert forward(L_=24) == _lib.KEEP_EINVAL and forward(L_=144) == _lib.KEEP_EINVAL and untouched()
    assert forward(nbytes=need.value - 1) == _lib.KEEP_EINVAL and forward(s_=None) == _lib.KEEP_EINVAL and untouched()
    assert forward(S_=0) == _lib.KEEP_EINVAL and untouched()
    assert forward() == 0
    torch.cuda.synchronize()
    assert not (s_out == 7).any() and skipped.cpu().tolist() == [f["skipped_rows"], f["skipped_bags"]]
    # the backward: C = 1, a null accumulator and a bad table add nothing
    hl = torch.zeros(S, dtype=torch.int32, device=DEV)
    probs = torch.full((S, C), 0.5, device=DEV)
    acc = torch.zeros(L * D + 2 * L, dtype=torch.int64, device=DEV)

    def backward(table=good, C__=C, gV=acc[:L * D], gw=acc[L * D + L:]):
        t = dev(np.ascontiguousarray(table))
        return lib.keep_mil_backward(h, _ptr(xd), N, D, _ptr(t), t.shape[0], S, _ptr(hl), _ptr(probs), _ptr(Wc), C__, None, _ptr(w), L, _ptr(s_out),
                                     _ptr(a_out), _ptr(z_out), _ptr(hid), _ptr(gV), _ptr(acc[L * D:L * D + L]), _ptr(gw), None, _ptr(ws), need.value, st)

    bad = good.copy()
    bad[1] = (1, N, 1)
    for rc in (backward(C__=1), backward(C__=65), backward(gV=None), backward(gw=None), backward(table=bad)):
        assert rc == _lib.KEEP_EINVAL
    torch.cuda.synchronize()
    assert not acc.any()
    assert backward() == 0
    torch.cuda.synchronize()
    assert acc.any()
