"""Bootstrap resampling on the MI355X: keep_boot_roc / keep_boot_confusion, KEEPModel.bootstrap_roc /
bootstrap_confusion / bootstrap_metric / bootstrap_ovr_roc and cohort.bootstrap_subtyping / bootstrap_detection.

The device counts are integers of a counter-based resampling, so every comparison is exact equality with the numpy restatements of
keep_amd.bootstrap, which tests/test_bootstrap.py holds to roc_numpy / np.bincount on the resampled arrays."""
import ctypes as C

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel, _lib, bootstrap, cohort
from keep_amd.bootstrap import LDS_GROUPS, boot_confusion_numpy, boot_roc_numpy
from keep_amd.config import small_shape
from keep_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 11


@pytest.fixture(scope="module")
def model():
    m = KEEPModel(precision="strict")
    m.load_state_dict(synth_state_dict(small_shape(2, 2), seed=5), strict=True)
    return m.to(DEV).eval()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def raw_roc(model, s, y, seed, first, B):
    """keep_boot_roc as the C ABI has it -> int64 [B,4] on the host."""
    sd, yd = torch.from_numpy(s).to(DEV), torch.from_numpy(y).to(DEV)
    out = torch.full((B, 4), -7, dtype=torch.int64, device=DEV)
    _lib.check(model._handle, _lib.load().keep_boot_roc(model._handle, _ptr(sd), _ptr(yd), len(s), seed, first, B, _ptr(out), _stream()), "boot_roc")
    return out.cpu().numpy()


def raw_confusion(model, t, p, n_classes, seed, first, B):
    td, pd = torch.from_numpy(t).to(DEV), torch.from_numpy(p).to(DEV)
    out = torch.full((B, n_classes, n_classes), -7, dtype=torch.int64, device=DEV)
    rc = _lib.load().keep_boot_confusion(model._handle, _ptr(td), _ptr(pd), len(t), n_classes, seed, first, B, _ptr(out), _stream())
    _lib.check(model._handle, rc, "boot_confusion")
    return out.cpu().numpy()


def same_values(a, b) -> bool:
    """float64 arrays equal bit for bit, NaNs in the same places."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


BIG = 2 * LDS_GROUPS + 17
ROC_CASES = {
    "one_item": (1, 64), "one_of_each": (2, 64), "below_a_wave": (63, 64), "wave_tail": (257, 64), "block_tail": (4097, 64),
    "global_slabs": (BIG, 8), "large_n_in_lds": (BIG, 8), "all_equal": (5000, 64),
}


def roc_case(name):
    n, B = ROC_CASES[name]
    g = np.random.default_rng(n)
    y = (g.random(n) < {"below_a_wave": 0.3, "wave_tail": 0.1, "block_tail": 0.02}.get(name, 0.25)).astype(np.uint8)
    y[:2] = [1, 0][:n]
    if name in ("one_item", "one_of_each"):
        s = np.array([0.5, 0.25][:n], np.float32)
    elif name in ("below_a_wave", "wave_tail"):
        s = (np.round(g.random(n) * 16) / 4 - 2).astype(np.float32)                      # a grid of 0.25: ties
        if name == "wave_tail":
            s[[7, 70, 130, 200, 256]] = np.nan
            s[20], s[21] = -0.0, 0.0
    elif name in ("block_tail", "global_slabs"):
        s = (g.permutation(n) / n).astype(np.float32)                                    # distinct: K = n
        assert len(np.unique(s)) == n
    elif name == "large_n_in_lds":
        s = (np.round(g.random(n) * 4000) / 4000).astype(np.float32)
        assert len(np.unique(s)) < LDS_GROUPS
    else:
        s = np.full(n, 0.25, np.float32)
    return s, y, B


@pytest.fixture(scope="module")
def roc_wants():
    """The restatement of every case, rows -1 .. B - 1, computed once."""
    return {name: boot_roc_numpy(*roc_case(name)[:2], ROC_CASES[name][1] + 1, SEED, first_replicate=-1) for name in ROC_CASES}


@pytest.mark.parametrize("name", list(ROC_CASES))
def test_boot_roc_equals_the_restatement(model, roc_wants, name):
    s, y, B = roc_case(name)
    want = roc_wants[name]
    counts, res = model.bootstrap_roc(s, y, n_boot=B, seed=SEED)
    assert counts.device == torch.device(DEV) and counts.dtype == torch.int64 and tuple(counts.shape) == (B, 4)
    assert np.array_equal(counts.cpu().numpy(), want[1:])
    auc = bootstrap.auc_from_counts(want[:, 1], want[:, 2], want[:, 3])
    undefined = int(((want[1:, 1] == 0) | (want[1:, 2] == 0)).sum())
    assert res.n_undefined == undefined == {"one_item": 64, "one_of_each": 35}.get(name, 0)
    assert same_values(res.values, auc[1:]) and same_values([res.estimate], auc[:1])
    assert res.n == int((~np.isnan(s)).sum()) and res.seed == SEED
    if name == "all_equal":
        assert (counts[:, 3] == counts[:, 1] * counts[:, 2]).all()
    # the sample's own row is keep_eval_roc's
    row = raw_roc(model, s, y, SEED, -1, 1)[0]
    assert np.array_equal(row, want[0])
    if row[1] and row[2]:
        roc = model.tile_roc(s, y, curve=False)
        assert tuple(row) == (roc.n, roc.n_pos, roc.n_neg, roc.u2) and res.estimate == roc.auc
    lo, hi = res.ci()
    assert undefined == B or lo <= hi


@pytest.mark.parametrize("name", ["wave_tail", "block_tail"])
def test_boot_roc_does_not_depend_on_the_split_or_the_run(model, roc_wants, name):
    s, y, B = roc_case(name)
    whole = raw_roc(model, s, y, SEED, 0, B)
    assert np.array_equal(whole, roc_wants[name][1:])
    assert np.array_equal(whole, raw_roc(model, s, y, SEED, 0, B))
    parts = [raw_roc(model, s, y, SEED, first, 16) for first in (0, 16, 32, 48)]
    assert np.array_equal(whole, np.concatenate(parts))
    counts, _ = model.bootstrap_roc(s, y, n_boot=16, seed=SEED, first_replicate=32)
    assert np.array_equal(counts.cpu().numpy(), whole[32:48])


def test_boot_roc_global_slabs_split_and_rerun(model, roc_wants):
    s, y, B = roc_case("global_slabs")
    whole = raw_roc(model, s, y, SEED, 0, B)
    assert np.array_equal(whole, roc_wants["global_slabs"][1:]) and np.array_equal(whole, raw_roc(model, s, y, SEED, 0, B))
    assert np.array_equal(whole[5:8], raw_roc(model, s, y, SEED, 5, 3))


@pytest.mark.parametrize("seed", [0, 7, 2 ** 64 - 1])
def test_boot_roc_seeds(model, seed):
    s, y, _ = roc_case("wave_tail")
    counts, res = model.bootstrap_roc(torch.from_numpy(s).to(DEV), torch.from_numpy(y).to(DEV) != 0, n_boot=16, seed=seed)
    want = boot_roc_numpy(s, y, 16, seed)
    assert np.array_equal(counts.cpu().numpy(), want) and res.seed == seed
    assert same_values(res.values, bootstrap.auc_from_counts(want[:, 1], want[:, 2], want[:, 3]))


def test_boot_roc_pairs_two_score_vectors(model):
    s, y, _ = roc_case("wave_tail")
    other = np.where(np.isnan(s), np.nan, np.random.default_rng(3).random(len(s))).astype(np.float32)
    (a, ra), (b, rb) = model.bootstrap_roc(s, y, 64, SEED), model.bootstrap_roc(other, y, 64, SEED)
    assert torch.equal(a[:, :3], b[:, :3]) and not torch.equal(a[:, 3], b[:, 3])
    assert np.array_equal(b.cpu().numpy(), boot_roc_numpy(other, y, 64, SEED))
    d = ra.minus(rb)
    assert same_values(d.values, ra.values - rb.values) and d.estimate == ra.estimate - rb.estimate
    with pytest.raises(ValueError):
        ra.minus(model.bootstrap_roc(other, y, 64, SEED + 1)[1])


def test_boot_roc_python_errors(model):
    s, y, _ = roc_case("below_a_wave")
    for kw in (dict(seed=-1), dict(seed=2 ** 64), dict(seed=0.5), dict(n_boot=-1), dict(n_boot=2 ** 20 + 1), dict(first_replicate=-1)):
        with pytest.raises(ValueError):
            model.bootstrap_roc(s, y, **kw)
    with pytest.raises(ValueError):
        model.bootstrap_roc(s, y[:5])
    with pytest.raises(ValueError):
        model.bootstrap_roc(np.zeros(0, np.float32), np.zeros(0, np.uint8))
    counts, res = model.bootstrap_roc(s, y, n_boot=0)
    assert tuple(counts.shape) == (0, 4) and res.values.shape == (0,) and res.estimate == model.tile_roc(s, y, curve=False).auc


# ------------------------------------------------------------------------------------------------ confusion
def confusion_case(n, n_classes):
    g = np.random.default_rng(100 * n + n_classes)
    t = g.integers(0, n_classes - (n_classes == 3), n).astype(np.uint8)                  # C = 3: class 2 never occurs in the truth
    p = np.where(g.random(n) < 0.7, t, g.integers(0, n_classes, n)).astype(np.uint8)
    return t, p


@pytest.mark.parametrize("n_classes", [2, 3, 16])
@pytest.mark.parametrize("n", [1, 63, 4097])
def test_boot_confusion_equals_the_restatement(model, n, n_classes):
    t, p = confusion_case(n, n_classes)
    B = 64
    want = boot_confusion_numpy(t, p, n_classes, B + 1, SEED, first_replicate=-1)
    got = model.bootstrap_confusion(t, p, n_classes, n_boot=B, seed=SEED)
    assert got.device == torch.device(DEV) and got.dtype == torch.int64 and tuple(got.shape) == (B, n_classes, n_classes)
    assert np.array_equal(got.cpu().numpy(), want[1:])
    assert (got.sum((1, 2)) == n).all()
    if n_classes == 3:
        assert (got[:, 2, :] == 0).all()
    own = raw_confusion(model, t, p, n_classes, SEED, -1, 1)[0]
    assert np.array_equal(own.ravel(), np.bincount(t.astype(np.int64) * n_classes + p, minlength=n_classes ** 2))
    whole = raw_confusion(model, t, p, n_classes, SEED, 0, B)
    assert np.array_equal(whole, want[1:]) and np.array_equal(whole, raw_confusion(model, t, p, n_classes, SEED, 0, B))
    assert np.array_equal(whole, np.concatenate([raw_confusion(model, t, p, n_classes, SEED, first, 16) for first in (0, 16, 32, 48)]))
    for metric in ("accuracy", "balanced_accuracy", "weighted_f1") + (("sensitivity", "specificity") if n_classes == 2 else ()):
        res = model.bootstrap_metric(torch.from_numpy(t).to(DEV), torch.from_numpy(p.astype(np.int64)).to(DEV), n_classes, metric, B, SEED)
        v = bootstrap.METRICS[metric](want)
        assert same_values(res.values, v[1:]) and same_values([res.estimate], v[:1]) and res.n == n
    res = model.bootstrap_metric(t, p, n_classes, lambda m: bootstrap.precision(m, 1), B, SEED)
    assert same_values(res.values, bootstrap.precision(want[1:], 1))


def test_boot_confusion_python_errors(model):
    t, p = confusion_case(63, 3)
    for bad in (dict(truth=t, pred=p, n_classes=2), dict(truth=t, pred=p, n_classes=17), dict(truth=t, pred=p[:5], n_classes=3),
                dict(truth=t.astype(np.float32), pred=p, n_classes=3), dict(truth=t.astype(np.int64) - 1, pred=p, n_classes=3),
                dict(truth=t, pred=p, n_classes=3, seed=-1), dict(truth=t, pred=p, n_classes=3, n_boot=-1),
                dict(truth=t, pred=p, n_classes=3, first_replicate=-1)):
        with pytest.raises(ValueError):
            model.bootstrap_confusion(**bad)
    with pytest.raises(ValueError):
        model.bootstrap_metric(t, p, 3, "sensitivity")
    with pytest.raises(ValueError):
        model.bootstrap_metric(t, p, 3, "f2")


def test_boot_ovr_roc(model):
    g = np.random.default_rng(5)
    n, n_classes = 257, 3
    y = g.integers(0, n_classes, n)
    probs = g.random((n, n_classes)).astype(np.float32) + 0.5 * np.eye(n_classes, dtype=np.float32)[y]
    probs[[9, 200], [0, 2]] = np.nan
    per_class, macro = model.bootstrap_ovr_roc(probs, y, n_boot=64, seed=SEED)
    keep = ~np.isnan(probs).any(1)
    assert keep.sum() == n - 2 and len(per_class) == n_classes
    wants = []
    for c in range(n_classes):
        rows = boot_roc_numpy(probs[keep, c], (y[keep] == c).astype(np.uint8), 65, SEED, first_replicate=-1)
        wants.append(bootstrap.result_from_roc_counts(rows, SEED))
        assert same_values(per_class[c].values, wants[c].values) and per_class[c].estimate == wants[c].estimate and per_class[c].n == n - 2
    want = bootstrap.macro_mean(wants)
    assert same_values(macro.values, want.values) and macro.estimate == want.estimate and macro.n_undefined == 0
    with pytest.raises(ValueError):
        model.bootstrap_ovr_roc(probs, y[:5])
    with pytest.raises(ValueError):
        model.bootstrap_ovr_roc(probs, y + 1)
    with pytest.raises(ValueError):
        model.bootstrap_ovr_roc(probs[:, 0], y)


# ------------------------------------------------------------------------------------------------ the C entry points' refusals
def test_c_entry_errors_write_nothing(model):
    lib, h, st = _lib.load(), model._handle, _stream()
    s = torch.rand(64, device=DEV)
    y = (torch.rand(64, device=DEV) < 0.5).to(torch.uint8)
    out = torch.full((4 * 16 * 16,), -7, dtype=torch.int64, device=DEV)
    null = C.c_void_p(0)
    roc = lambda sp=_ptr(s), yp=_ptr(y), n=64, first=0, B=4, o=_ptr(out): lib.keep_boot_roc(h, sp, yp, n, 1, first, B, o, st)      # noqa: E731
    conf = lambda tp=_ptr(y), pp=_ptr(y), n=64, c=2, first=0, B=4, o=_ptr(out): lib.keep_boot_confusion(h, tp, pp, n, c, 1, first, B, o, st)   # noqa: E731
    for fn in (roc, conf):
        for kw in (dict(n=-1), dict(n=2 ** 24), dict(B=-1), dict(B=2 ** 20 + 1), dict(first=-2), dict(o=null)):
            assert fn(**kw) == _lib.KEEP_EINVAL, kw
            assert lib.keep_last_error(h)
    assert roc(sp=null) == roc(yp=null) == conf(tp=null) == conf(pp=null) == _lib.KEEP_EINVAL
    assert conf(c=1) == conf(c=17) == conf(c=0) == _lib.KEEP_EINVAL
    assert b"classes" in lib.keep_last_error(h)
    assert lib.keep_boot_roc(None, _ptr(s), _ptr(y), 64, 1, 0, 4, _ptr(out), st) == _lib.KEEP_EINVAL
    assert lib.keep_boot_confusion(None, _ptr(y), _ptr(y), 64, 2, 1, 0, 4, _ptr(out), st) == _lib.KEEP_EINVAL
    # B = 0 succeeds and writes nothing; N = 0 succeeds and writes zeros
    assert roc(B=0) == conf(B=0) == roc(B=0, o=null) == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert (out == -7).all()
    assert roc(n=0, sp=null, yp=null) == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert (out[:16] == 0).all() and (out[16:] == -7).all()
    assert conf(n=0, tp=null, pp=null, c=3) == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert (out[:36] == 0).all() and (out[36:] == -7).all()


# ------------------------------------------------------------------------------------------------ where users meet it
def test_cohort_bootstrap_on_a_synthetic_cohort(model):
    g = np.random.default_rng(40)
    ids = [f"slide_{i:02d}" for i in range(40)]
    truth = g.integers(0, 3, 40)
    called = np.where(g.random(40) < 0.75, truth, g.integers(0, 3, 40))
    targets = {i: int(t) for i, t in zip(ids, truth)}
    preds = {i: torch.tensor(int(c)) for i, c in reversed(list(zip(ids, called)))}        # a mapping is aligned by slide id
    got = cohort.bootstrap_subtyping(preds, targets, 3, n_boot=64, seed=SEED, model=model)
    want = boot_confusion_numpy(truth, called, 3, 65, SEED, first_replicate=-1)
    for name, fn in (("balanced_accuracy", bootstrap.balanced_accuracy), ("weighted_f1", bootstrap.weighted_f1)):
        assert same_values(got[name].values, fn(want[1:])) and got[name].estimate == float(fn(want[0])) and got[name].n == 40
        lo, hi = got[name].ci()
        assert 0.0 <= lo <= hi <= 1.0
    assert got["balanced_accuracy"].minus(got["weighted_f1"]).n_undefined == 0
    binary = {i: int(t > 0) for i, t in targets.items()}
    scores = [float(s) for s in (truth > 0) * 0.3 + g.random(40)]
    det = cohort.bootstrap_detection(scores, binary, n_boot=64, seed=SEED, model=model)
    rows = boot_roc_numpy(np.asarray(scores, np.float32), (truth > 0).astype(np.uint8), 65, SEED, first_replicate=-1)
    want_det = bootstrap.result_from_roc_counts(rows, SEED)
    assert same_values(det.values, want_det.values) and det.estimate == want_det.estimate and det.ci() == want_det.ci()
    with pytest.raises(ValueError):
        cohort.bootstrap_subtyping({i: 0 for i in ids[:-1]}, targets, 3, model=model)
    with pytest.raises(ValueError):
        cohort.bootstrap_subtyping({i: torch.zeros(4, 3) for i in ids}, targets, 3, model=model)
    with pytest.raises(ValueError):
        cohort.bootstrap_detection(scores[:-1], binary, model=model)
