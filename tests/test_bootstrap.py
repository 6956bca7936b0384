"""The bootstrap's host side: the generator against its definition in Python integers and against literal
values, the numpy restatements against keep_amd.evaluation.roc_numpy / np.bincount on the resampled arrays, the metrics against
scikit-learn (hand-written loops where it does not import), the result class and every ValueError.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

from keep_amd import _lib, bootstrap
from keep_amd.bootstrap import (BootstrapResult, boot_confusion_numpy, boot_roc_numpy, draw, draws_numpy, key, mix64)
from keep_amd.evaluation import roc_numpy
from keep_amd.tile_eval import weighted_f1_from_confusion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the generator
def test_the_generator_is_pinned_by_literals():
    assert mix64(bootstrap.G) == 0xE220A8397B1DCDAF
    assert [draw(7, 0, j, 1000) for j in range(6)] == [732, 481, 664, 576, 90, 731]
    assert [draw(0, 0, j, 5) for j in range(5)] == [1, 1, 1, 1, 2]
    assert [draw(2 ** 63 + 5, 999, j, 2 ** 24 - 1) for j in range(4)] == [14752765, 5561210, 10939927, 8995573]
    assert draws_numpy(7, 0, 1000)[:6].tolist() == [732, 481, 664, 576, 90, 731]
    assert draws_numpy(0, 0, 5).tolist() == [1, 1, 1, 1, 2]
    assert draws_numpy(2 ** 63 + 5, 999, 2 ** 24 - 1)[:4].tolist() == [14752765, 5561210, 10939927, 8995573]


def spelled_out(seed, b, j, n):
    """The contract once more, written from the issue's text and not from the module."""
    M = (1 << 64) - 1
    G = 0x9E3779B97F4A7C15

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    k = mix(seed ^ mix(((b + 1) * G) & M))
    return (mix((k + j * G) & M) * n) >> 64


@pytest.mark.parametrize("n", [1, 2, 3, 97, 4097, 2 ** 24 - 1])
def test_draws_numpy_equals_python_integers(n):
    for seed, b in ((0, 0), (7, 3), (2 ** 64 - 1, 999), (2 ** 63 + 5, 2 ** 20)):
        got = draws_numpy(seed, b, n)
        assert got.dtype == np.int64 and got.shape == (n,) and got.min() >= 0 and got.max() < n
        js = sorted(set(range(min(n, 64))) | {n - 1, n // 2, n // 3})
        assert [int(got[j]) for j in js] == [spelled_out(seed, b, j, n) for j in js] == [draw(seed, b, j, n) for j in js]
    assert draws_numpy(5, -1, n).tolist() == list(range(n)) if n < 5000 else draws_numpy(5, -1, n)[-1] == n - 1
    assert key(7, 0) != key(7, 1) != key(8, 1)


def test_a_replicate_depends_on_seed_replicate_and_size_alone():
    assert np.array_equal(draws_numpy(3, 17, 500), draws_numpy(3, 17, 500))
    assert not np.array_equal(draws_numpy(3, 17, 500), draws_numpy(3, 18, 500))
    assert not np.array_equal(draws_numpy(3, 17, 500), draws_numpy(4, 17, 500))
    # a fair resample: every position about once, about 1 - 1/e of the items drawn
    d = draws_numpy(11, 0, 100000)
    assert abs(len(np.unique(d)) / 100000 - (1 - math.exp(-1))) < 0.01


def test_draws_errors():
    for seed in (-1, 2 ** 64, 1.5, "7", None, True):
        with pytest.raises(ValueError):
            draws_numpy(seed, 0, 10)
    with pytest.raises(ValueError):
        draws_numpy(0, -2, 10)
    with pytest.raises(ValueError):
        draws_numpy(0, 0, 2 ** 24)
    with pytest.raises(ValueError):
        draws_numpy(0, 0, -1)
    assert draws_numpy(np.int64(7), np.int32(0), np.int64(1000))[:2].tolist() == [732, 481]
    assert draws_numpy(0, 0, 0).shape == (0,)


def test_the_exported_cap_is_the_headers():
    hdr = open(os.path.join(ROOT, "include", "keep_hip.h")).read()
    assert int(re.search(r"KEEP_BOOT_LDS_GROUPS\s*=\s*(\d+)", hdr).group(1)) == bootstrap.LDS_GROUPS
    assert {"keep_boot_roc", "keep_boot_confusion"} <= set(_lib.SIGNATURES)


# ------------------------------------------------------------------------------------------------ the restatements
def roc_case(n, seed, ties=True, frac=0.3, nans=0):
    g = np.random.default_rng(seed)
    s = (np.round(g.random(n) * 8) / 4 - 1).astype(np.float32) if ties else g.random(n).astype(np.float32)
    y = (g.random(n) < frac).astype(np.uint8)
    if n >= 2:
        y[:2] = [1, 0]
    if nans:
        s[g.choice(np.arange(2, n), nans, replace=False)] = np.nan
    if n > 20:
        s[10], s[11] = -0.0, 0.0
    return s, y


@pytest.mark.parametrize("n, ties, nans", [(1, True, 0), (2, True, 0), (63, True, 0), (257, True, 5), (300, False, 0), (1000, False, 7)])
def test_boot_roc_numpy_is_roc_numpy_of_the_resampled_arrays(n, ties, nans):
    s, y = roc_case(n, n, ties, nans=nans)
    B, seed = 24, 11
    got = boot_roc_numpy(s, y, B, seed, first_replicate=-1)
    ok = ~np.isnan(s)
    ss, yy = s[ok], y[ok]
    assert got.dtype == np.int64 and got.shape == (B, 4) and (got[:, 0] == ok.sum()).all()
    assert (got[:, 1] + got[:, 2] == ok.sum()).all()
    one_class = 0
    for r in range(B):
        idx = draws_numpy(seed, r - 1, len(ss))
        try:
            want = roc_numpy(ss[idx], yy[idx], curve=False)
        except ValueError:
            assert got[r, 1] == 0 or got[r, 2] == 0
            one_class += 1
            continue
        assert tuple(got[r]) == (want.n, want.n_pos, want.n_neg, want.u2), r
    assert (one_class == B) if n == 1 else (one_class > 0) if n == 2 else (one_class == 0)
    # the replicates do not depend on how they are split over calls
    assert np.array_equal(got[1:], boot_roc_numpy(s, y, B - 1, seed))
    assert np.array_equal(got[9:14], boot_roc_numpy(s, y, 5, seed, first_replicate=8))


def test_boot_roc_numpy_one_class_counts_the_issue_states():
    """Labels l[0] = 1, l[1] = 0 forced, seed 11, B = 64: no one-class replicate at N = 63, 257, 4097, 5000; 35 at N = 2; 64 at N = 1."""
    for n, want in ((1, 64), (2, 35), (63, 0), (257, 0)):
        s, y = roc_case(n, 1)
        c = boot_roc_numpy(s, y, 64, 11)
        assert int(((c[:, 1] == 0) | (c[:, 2] == 0)).sum()) == want


def test_equal_scores_give_u2_p_times_n():
    s, y = np.full(500, 0.25, np.float32), roc_case(500, 3)[1]
    c = boot_roc_numpy(s, y, 16, 5)
    assert (c[:, 3] == c[:, 1] * c[:, 2]).all()


def test_paired_replicates_share_their_class_counts():
    s, y = roc_case(400, 8, nans=6)
    t = np.where(np.isnan(s), np.nan, np.random.default_rng(1).random(400).astype(np.float32))
    a, b = boot_roc_numpy(s, y, 12, 9), boot_roc_numpy(t, y, 12, 9)
    assert np.array_equal(a[:, :3], b[:, :3]) and not np.array_equal(a[:, 3], b[:, 3])


@pytest.mark.parametrize("n, C", [(1, 2), (63, 3), (500, 16)])
def test_boot_confusion_numpy_is_bincount_of_the_resampled_arrays(n, C):
    g = np.random.default_rng(n)
    t, p = g.integers(0, C - (C == 3), n).astype(np.uint8), g.integers(0, C, n).astype(np.int64)
    got = boot_confusion_numpy(t, p, C, 10, 4, first_replicate=-1)
    assert got.shape == (10, C, C) and (got.sum((1, 2)) == n).all()
    for r in range(10):
        idx = draws_numpy(4, r - 1, n)
        assert np.array_equal(got[r].ravel(), np.bincount(t[idx].astype(np.int64) * C + p[idx], minlength=C * C))
    assert np.array_equal(got[0].ravel(), np.bincount(t.astype(np.int64) * C + p, minlength=C * C))
    assert np.array_equal(got[4:7], boot_confusion_numpy(t, p, C, 3, 4, first_replicate=3))


def test_restatement_errors():
    s, y = roc_case(10, 0)
    for kw in (dict(n_boot=-1), dict(n_boot=2 ** 20 + 1), dict(first_replicate=-2), dict(seed=-1), dict(seed=2 ** 64), dict(n_boot=1.5)):
        args = dict(n_boot=4, seed=0, first_replicate=0)
        args.update(kw)
        with pytest.raises(ValueError):
            boot_roc_numpy(s, y, **args)
        with pytest.raises(ValueError):
            boot_confusion_numpy(y, y, 2, **args)
    with pytest.raises(ValueError):
        boot_roc_numpy(s, y[:5], 4, 0)
    with pytest.raises(ValueError):
        boot_roc_numpy(y, y, 4, 0)                                # integer scores
    t = np.array([0, 1, 2], np.uint8)
    for bad in (dict(truth=t, pred=t, n_classes=2), dict(truth=t, pred=t, n_classes=1), dict(truth=t, pred=t, n_classes=17),
                dict(truth=t, pred=t[:2], n_classes=3), dict(truth=t.astype(np.float32), pred=t, n_classes=3),
                dict(truth=t.astype(np.int64) - 1, pred=t, n_classes=3), dict(truth=t.reshape(1, 3), pred=t.reshape(1, 3), n_classes=3),
                dict(truth=t, pred=t, n_classes=3.0)):
        with pytest.raises(ValueError):
            boot_confusion_numpy(n_boot=2, seed=0, **bad)
    assert boot_confusion_numpy(t, t, 3, 0, 0).shape == (0, 3, 3)
    assert boot_roc_numpy(s, y, 0, 0).shape == (0, 4)


# ------------------------------------------------------------------------------------------------ the metrics
def loops(conf):
    """accuracy, balanced accuracy, weighted F1 and the per-class recall / precision of one confusion, by hand."""
    C = conf.shape[0]
    n = int(conf.sum())
    rec, pre, f1, weight = [], [], [], []
    for c in range(C):
        tp, row, col = int(conf[c, c]), int(conf[c].sum()), int(conf[:, c].sum())
        rec.append(tp / row if row else math.nan)
        pre.append(tp / col if col else math.nan)
        f1.append(2 * tp / (row + col) if row + col else 0.0)
        weight.append(row)
    present = [r for r in rec if not math.isnan(r)]
    return (sum(int(conf[c, c]) for c in range(C)) / n, sum(present) / len(present), sum(f * w for f, w in zip(f1, weight)) / n, rec, pre)


def confusions():
    g = np.random.default_rng(0)
    out = [g.integers(0, 50, (C, C)) for C in (2, 3, 5, 16)]
    out.append(np.array([[5, 2, 0], [0, 0, 0], [1, 0, 7]]))          # a class that never occurs in the truth
    out.append(np.array([[5, 0, 2], [3, 0, 4], [1, 0, 7]]))          # a class that is never predicted
    return [c.astype(np.int64) for c in out]


# Each metric is a handful of float64 operations on integers below 2^24, so two correct orders of evaluation differ by a few units in the
# last place: 1e-12 relative leaves three orders of magnitude of room and is six below any difference a wrong formula would make.
TOL = 1e-12


@pytest.mark.parametrize("conf", confusions())
def test_metrics_against_loops_and_scikit_learn(conf):
    C = conf.shape[0]
    acc, bal, wf1, rec, pre = loops(conf)
    assert bootstrap.accuracy(conf) == pytest.approx(acc, rel=TOL)
    assert bootstrap.balanced_accuracy(conf) == pytest.approx(bal, rel=TOL)
    assert bootstrap.weighted_f1(conf) == pytest.approx(wf1, rel=TOL)
    assert float(bootstrap.weighted_f1(conf)) == pytest.approx(weighted_f1_from_confusion(conf), rel=TOL)
    for c in range(C):
        assert float(bootstrap.recall(conf, c)) == pytest.approx(rec[c], rel=TOL, nan_ok=True)
        assert float(bootstrap.precision(conf, c)) == pytest.approx(pre[c], rel=TOL, nan_ok=True)
    if C == 2:
        assert bootstrap.sensitivity(conf) == bootstrap.recall(conf, 1) and bootstrap.specificity(conf) == bootstrap.recall(conf, 0)
    else:
        with pytest.raises(ValueError):
            bootstrap.sensitivity(conf)
        with pytest.raises(ValueError):
            bootstrap.specificity(conf)
    try:
        import warnings
        from sklearn.metrics import accuracy_score, balanced_accuracy_score, f1_score
    except ImportError:
        return
    t, p = np.repeat(np.arange(C), conf.sum(1)), np.concatenate([np.repeat(np.arange(C), row) for row in conf])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert bootstrap.accuracy(conf) == pytest.approx(accuracy_score(t, p), rel=TOL)
        assert bootstrap.balanced_accuracy(conf) == pytest.approx(balanced_accuracy_score(t, p), rel=TOL)
        assert bootstrap.weighted_f1(conf) == pytest.approx(f1_score(t, p, average="weighted"), rel=TOL)


def test_metrics_take_a_stack_and_say_nan_for_nothing():
    stack = np.stack([c for c in confusions() if c.shape[0] == 3] + [np.zeros((3, 3), np.int64)])
    for fn in (bootstrap.accuracy, bootstrap.balanced_accuracy, bootstrap.weighted_f1):
        v = fn(stack)
        assert v.dtype == np.float64 and v.shape == (4,) and math.isnan(v[3]) and not np.isnan(v[:3]).any()
        assert [float(fn(stack[k])) for k in range(3)] == v[:3].tolist()
    with pytest.raises(ValueError):
        bootstrap.accuracy(np.zeros((3, 2), np.int64))
    with pytest.raises(ValueError):
        bootstrap.accuracy(np.zeros((3, 3)))
    with pytest.raises(ValueError):
        bootstrap.resolve_metric("f2")
    assert bootstrap.resolve_metric(len) is len


def test_auc_from_counts():
    v = bootstrap.auc_from_counts(np.array([3, 0, 2]), np.array([4, 5, 0]), np.array([12, 0, 0]))
    assert v[0] == 12.0 / (2.0 * 3 * 4) and math.isnan(v[1]) and math.isnan(v[2])
    s, y = roc_case(300, 2)
    c = boot_roc_numpy(s, y, 1, 0, first_replicate=-1)[0]
    assert float(bootstrap.auc_from_counts(c[1], c[2], c[3])) == roc_numpy(s, y, curve=False).auc


# ------------------------------------------------------------------------------------------------ the result
def test_result_ci_se_minus():
    v = np.array([0.5, np.nan, 0.7, 0.6, 0.9, np.nan, 0.8])
    r = BootstrapResult(0.65, v, seed=3, n=40)
    good = v[~np.isnan(v)]
    assert r.estimate == 0.65 and r.n_undefined == 2 and np.array_equal(r.defined, good)
    assert r.ci() == tuple(np.percentile(good, [2.5, 97.5])) and r.ci(0.5) == tuple(np.percentile(good, [25.0, 75.0]))
    assert r.se == np.std(good, ddof=1)
    for level in (0, 1, 1.5, -0.1):
        with pytest.raises(ValueError):
            r.ci(level)
    empty = BootstrapResult(math.nan, np.full(3, np.nan), 3, 40)
    assert all(math.isnan(x) for x in empty.ci()) and math.isnan(empty.se) and empty.n_undefined == 3
    assert math.isnan(BootstrapResult(0.5, [0.5], 0, 1).se)
    other = BootstrapResult(0.6, v[::-1].copy(), seed=3, n=40)
    d = r.minus(other)
    assert d.estimate == 0.65 - 0.6 and d.n_undefined == 2 and np.array_equal(d.defined, (v - v[::-1])[~np.isnan(v - v[::-1])])
    for bad in (BootstrapResult(0.6, v, 4, 40), BootstrapResult(0.6, v, 3, 41), BootstrapResult(0.6, v[:-1], 3, 40),
                BootstrapResult(0.6, v, 3, 40, first_replicate=7), 0.6):
        with pytest.raises(ValueError):
            r.minus(bad)
    assert "BootstrapResult" in repr(r)


def test_results_from_counts_and_the_macro_mean():
    s, y = roc_case(300, 5)
    rows = boot_roc_numpy(s, y, 9, 2, first_replicate=-1)
    r = bootstrap.result_from_roc_counts(rows, 2)
    assert r.estimate == roc_numpy(s, y, curve=False).auc and r.values.shape == (8,) and r.n == 300 and r.seed == 2
    t, p = np.random.default_rng(0).integers(0, 3, (2, 200))
    confs = boot_confusion_numpy(t, p, 3, 9, 2, first_replicate=-1)
    m = bootstrap.result_from_confusions(confs, "balanced_accuracy", 2)
    assert m.estimate == float(bootstrap.balanced_accuracy(confs[0])) and np.array_equal(m.values, bootstrap.balanced_accuracy(confs[1:]))
    assert bootstrap.result_from_confusions(confs, lambda c: bootstrap.recall(c, 2), 2).estimate == float(bootstrap.recall(confs[0], 2))
    with pytest.raises(ValueError):
        bootstrap.result_from_confusions(confs, lambda c: np.zeros(3), 2)
    a, b = BootstrapResult(0.5, [0.25, np.nan, 0.75], 1, 10), BootstrapResult(1.0, [0.75, 0.5, np.nan], 1, 10)
    mm = bootstrap.macro_mean([a, b])
    assert mm.estimate == 0.75 and mm.values[0] == 0.5 and mm.n_undefined == 2
    with pytest.raises(ValueError):
        bootstrap.macro_mean([a, BootstrapResult(1.0, [0.75, 0.5, np.nan], 2, 10)])
    with pytest.raises(ValueError):
        bootstrap.macro_mean([])
