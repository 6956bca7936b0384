"""Bootstrap confidence intervals: the resampling contract, its restatements in numpy, the metrics of a
resampled confusion matrix and the result class.  No device code lives here: ``KEEPModel.bootstrap_roc`` / ``bootstrap_confusion`` /
``bootstrap_metric`` / ``bootstrap_ovr_roc`` (``slide.py``, kernels in ``csrc/bootstrap.hip``) produce the integer counts of every
replicate on the device, and :func:`boot_roc_numpy` / :func:`boot_confusion_numpy` are what those counts equal exactly.

The resampling.  All arithmetic modulo 2^64, ``G = 0x9E3779B97F4A7C15``::

    mix64(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
               z = (z ^ (z >> 27)) * 0x94D049BB133111EB
               return z ^ (z >> 31)                               # the splitmix64 finaliser
    key(seed, b)        = mix64(seed ^ mix64((b + 1) * G))        # b >= 0: the replicate
    draw(seed, b, j, n) = (mix64(key(seed, b) + j * G) * n) >> 64 # the high half of the 128-bit product; j = 0..n-1

Replicate ``b >= 0`` of a sample of ``n`` items is the multiset ``{item[draw(seed, b, j, n)] : j = 0..n-1}``; replicate ``-1`` is the
sample itself.  A replicate depends on ``(seed, b, n)`` alone -- not on how many replicates a call asks for or how they are split
over calls -- and two samples of equal ``n`` resampled with equal ``seed`` draw the same positions: their replicates are paired,
which is what :meth:`BootstrapResult.minus` needs.  For the ROC the sample is the items whose score is not NaN, in their original
order, so two score vectors are paired exactly when their NaN positions coincide.  The index bias of the multiply-shift is below
``n / 2^64``.  Every class is resampled together (no stratification); the interval is the percentile interval."""
from __future__ import annotations

import math
import operator
from typing import Callable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

LDS_GROUPS = 8192                      # KEEP_BOOT_LDS_GROUPS: distinct scores up to which the device keeps a replicate's counters in LDS
MAX_ITEMS = (1 << 24) - 1
MAX_REPLICATES = 1 << 20
MAX_CLASSES = 16
G = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1
_C1, _C2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


# ------------------------------------------------------------------------------------------------ the generator
def mix64(z: int) -> int:
    """The splitmix64 finaliser in Python integers; ``mix64(G) == 0xE220A8397B1DCDAF``."""
    z &= _M64
    z = ((z ^ (z >> 30)) * _C1) & _M64
    z = ((z ^ (z >> 27)) * _C2) & _M64
    return z ^ (z >> 31)


def key(seed: int, b: int) -> int:
    return mix64(seed ^ mix64((b + 1) * G))


def draw(seed: int, b: int, j: int, n: int) -> int:
    """Position ``j`` of replicate ``b >= 0`` of a sample of ``n`` items, in Python integers."""
    return (mix64(key(seed, b) + j * G) * n) >> 64


def check_seed(seed) -> int:
    try:
        s = operator.index(seed)
    except TypeError:
        raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}") from None
    if isinstance(seed, bool) or s < 0 or s > _M64:
        raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
    return s


def check_replicates(n_boot, first_replicate) -> Tuple[int, int]:
    try:
        B, first = operator.index(n_boot), operator.index(first_replicate)
    except TypeError:
        raise ValueError(f"n_boot and first_replicate must be integers, got {n_boot!r} and {first_replicate!r}") from None
    if B < 0 or B > MAX_REPLICATES:
        raise ValueError(f"n_boot must be in 0 .. 2^20, got {B}")
    if first < -1:
        raise ValueError(f"first_replicate must be >= -1 (-1 = the sample itself), got {first}")
    return B, first


def _mix64_np(z: np.ndarray) -> np.ndarray:
    z = (z ^ (z >> np.uint64(30))) * np.uint64(_C1)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(_C2)
    return z ^ (z >> np.uint64(31))


def draws_numpy(seed, b, n) -> np.ndarray:
    """int64 ``[n]``: the positions replicate ``b`` draws from a sample of ``n`` items (``b = -1``: ``0..n-1``), in numpy ``uint64``; the high
    half of the 128-bit product from two 32-bit halves (``n < 2^24``, so neither partial product overflows)."""
    seed = check_seed(seed)
    b, n = operator.index(b), operator.index(n)
    if b < -1:
        raise ValueError(f"replicate {b} < -1")
    if n < 0 or n > MAX_ITEMS:
        raise ValueError(f"n must be in 0 .. 2^24 - 1, got {n}")
    if b < 0:
        return np.arange(n, dtype=np.int64)
    with np.errstate(over="ignore"):
        x = _mix64_np(np.uint64(key(seed, b)) + np.arange(n, dtype=np.uint64) * np.uint64(G))
        hi, lo, nn = x >> np.uint64(32), x & np.uint64(0xFFFFFFFF), np.uint64(n)
        return ((hi * nn + ((lo * nn) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)


# ------------------------------------------------------------------------------------------------ argument checks
def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _is_integer(dtype) -> bool:
    if isinstance(dtype, torch.dtype):
        return not (dtype.is_floating_point or dtype.is_complex)
    return dtype.kind in "iub"


def check_classes(n_classes) -> int:
    try:
        C = operator.index(n_classes)
    except TypeError:
        raise ValueError(f"n_classes must be an integer, got {n_classes!r}") from None
    if C < 2 or C > MAX_CLASSES:
        raise ValueError(f"n_classes must be in 2 .. 16, got {C}")
    return C


def check_confusion_args(truth, pred, n_classes) -> Tuple[int, int]:
    """truth, pred: bool / integer ``[N]`` (numpy or torch) with every value in ``[0, n_classes)`` -> ``(N, C)``.  The range check reads
    the arrays (one synchronisation for device tensors)."""
    C = check_classes(n_classes)
    ts, ps = tuple(truth.shape), tuple(pred.shape)
    if len(ts) != 1 or ps != ts:
        raise ValueError(f"truth and pred must both be [N], got {ts} and {ps}")
    if not _is_integer(truth.dtype) or not _is_integer(pred.dtype):
        raise ValueError(f"truth and pred must be bool or integers, got {truth.dtype} and {pred.dtype}")
    N = int(ts[0])
    if N > MAX_ITEMS:
        raise ValueError(f"at most 2^24 - 1 items, got {N}")
    for name, a in (("truth", truth), ("pred", pred)):
        if N and a.dtype not in (torch.bool, np.dtype(bool)):
            lo, hi = int(a.min()), int(a.max())
            if lo < 0 or hi >= C:
                raise ValueError(f"{name} holds labels in [{lo}, {hi}], outside [0, {C})")
    return N, C


# ------------------------------------------------------------------------------------------------ the restatements
def boot_roc_numpy(scores, labels, n_boot, seed, first_replicate=0) -> np.ndarray:
    """keep_boot_roc restated on the host -> int64 ``[n_boot, 4]``: ``n, P_b, Nn_b, U2_b`` of replicates ``first_replicate ..``.  A NaN score
    removes its item, -0.0 counts as +0.0, the scores are rounded to float32 first (as :func:`keep_amd.evaluation.roc_numpy`).  With
    ``wp[g]`` / ``wn[g]`` the drawn positives / negatives at the ``g``-th distinct score, ``U2_b = sum_g wp[g] (2 sum_{g' < g} wn[g'] +
    wn[g])``: what ``roc_numpy`` computes from the resampled arrays (``tests/test_bootstrap.py`` holds it to that)."""
    from .evaluation import check_roc_args
    s, l = _host(scores), _host(labels)
    check_roc_args(s, l)
    seed = check_seed(seed)
    B, first = check_replicates(n_boot, first_replicate)
    s = s.astype(np.float32)
    ok = ~np.isnan(s)
    s, pos = s[ok] + np.float32(0), l[ok] != 0
    n = len(s)
    uniq, g = np.unique(s, return_inverse=True)
    g = g.reshape(-1)
    K = len(uniq)
    out = np.zeros((B, 4), np.int64)
    out[:, 0] = n
    for r in range(B):
        idx = draws_numpy(seed, first + r, n)
        gi, pi = g[idx], pos[idx]
        wp = np.bincount(gi[pi], minlength=K).astype(np.int64)
        wn = np.bincount(gi[~pi], minlength=K).astype(np.int64)
        below = np.cumsum(wn) - wn
        out[r, 1:] = wp.sum(), wn.sum(), int((wp * (2 * below + wn)).sum())
    return out


def boot_confusion_numpy(truth, pred, n_classes, n_boot, seed, first_replicate=0) -> np.ndarray:
    """keep_boot_confusion restated on the host -> int64 ``[n_boot, C, C]``, ``out[r, t, p]`` = the draws of replicate ``first_replicate + r``
    that landed on an item with truth ``t`` and prediction ``p``."""
    t, p = _host(truth), _host(pred)
    N, C = check_confusion_args(t, p, n_classes)
    seed = check_seed(seed)
    B, first = check_replicates(n_boot, first_replicate)
    code = t.astype(np.int64) * C + p.astype(np.int64)
    out = np.zeros((B, C, C), np.int64)
    for r in range(B):
        out[r] = np.bincount(code[draws_numpy(seed, first + r, N)], minlength=C * C).reshape(C, C)
    return out


# ------------------------------------------------------------------------------------------------ metrics of [..., C, C] confusions
def _conf(conf) -> np.ndarray:
    m = _host(conf)
    if m.ndim < 2 or m.shape[-1] != m.shape[-2] or m.dtype.kind not in "iu":
        raise ValueError(f"a confusion is an integer array [..., C, C], got {m.dtype} {m.shape}")
    return m.astype(np.float64)


def _ratio(num: np.ndarray, den: np.ndarray) -> np.ndarray:
    """num / den in float64, NaN where den is 0."""
    return np.divide(num, den, out=np.full(np.broadcast(num, den).shape, np.nan), where=den > 0)


def _tp(m: np.ndarray) -> np.ndarray:
    return np.diagonal(m, axis1=-2, axis2=-1)


def accuracy(conf):
    m = _conf(conf)
    return _ratio(_tp(m).sum(-1), m.sum((-2, -1)))


def balanced_accuracy(conf):
    """The mean recall over the classes that occur in the truth, as ``sklearn.metrics.balanced_accuracy_score``; NaN with no item."""
    m = _conf(conf)
    rows = m.sum(-1)
    rec = np.divide(_tp(m), rows, out=np.zeros_like(rows), where=rows > 0)
    return _ratio(rec.sum(-1), (rows > 0).sum(-1).astype(np.float64))


def weighted_f1(conf):
    """``keep_amd.tile_eval.weighted_f1_from_confusion``'s definition over the leading axes: per-class F1 (0 where undefined)
    weighted by the class's true count; NaN with no item."""
    m = _conf(conf)
    tp = _tp(m)
    fp, fn = m.sum(-2) - tp, m.sum(-1) - tp
    den = 2 * tp + fp + fn
    f = np.divide(2 * tp, den, out=np.zeros_like(den), where=den > 0)
    w = tp + fn
    return _ratio((f * w).sum(-1), w.sum(-1))


def recall(conf, c: int):
    m = _conf(conf)
    return _ratio(m[..., c, c], m[..., c, :].sum(-1))


def precision(conf, c: int):
    m = _conf(conf)
    return _ratio(m[..., c, c], m[..., :, c].sum(-1))


def _binary(conf) -> None:
    if _host(conf).shape[-1] != 2:
        raise ValueError(f"sensitivity and specificity are defined for two classes, got {_host(conf).shape[-1]}")


def sensitivity(conf):
    _binary(conf)
    return recall(conf, 1)


def specificity(conf):
    _binary(conf)
    return recall(conf, 0)


def auc_from_counts(P, Nn, U2):
    """``float(U2) / (2.0 P Nn)`` in float64, NaN where a class is missing."""
    P, Nn, U2 = (np.asarray(_host(x)).astype(np.float64) for x in (P, Nn, U2))
    return _ratio(U2, 2.0 * P * Nn)


METRICS = {"accuracy": accuracy, "balanced_accuracy": balanced_accuracy, "weighted_f1": weighted_f1, "sensitivity": sensitivity,
           "specificity": specificity}


def resolve_metric(metric) -> Callable:
    if callable(metric):
        return metric
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)} or a callable on the confusion array, got {metric!r}")
    return METRICS[metric]


# ------------------------------------------------------------------------------------------------ the result
class BootstrapResult:
    """``estimate``: the value of the sample itself (replicate -1); ``values``: float64 ``[B]``, one per replicate, NaN where the
    replicate leaves the value undefined (one class only); ``n_undefined`` counts those.  ``seed``, ``n`` (the sample's size) and
    ``first_replicate`` say which resamples these are."""

    def __init__(self, estimate, values, seed: int, n: int, first_replicate: int = 0):
        self.estimate = float(estimate)
        self.values = np.asarray(values, dtype=np.float64).reshape(-1)
        self.seed, self.n, self.first_replicate = int(seed), int(n), int(first_replicate)

    def __repr__(self):
        lo, hi = self.ci()
        return (f"BootstrapResult(estimate={self.estimate:.6f}, ci95=({lo:.6f}, {hi:.6f}), replicates={len(self.values)}, "
                f"undefined={self.n_undefined})")

    @property
    def n_undefined(self) -> int:
        return int(np.isnan(self.values).sum())

    @property
    def defined(self) -> np.ndarray:
        return self.values[~np.isnan(self.values)]

    def ci(self, level: float = 0.95) -> Tuple[float, float]:
        """The percentile interval: ``np.percentile`` of the defined values at ``50 (1 - level)`` and ``100 - 50 (1 - level)``, numpy's
        default linear rule; ``(nan, nan)`` when no replicate is defined."""
        if not 0.0 < level < 1.0:
            raise ValueError(f"level must lie in (0, 1), got {level!r}")
        v = self.defined
        if len(v) == 0:
            return math.nan, math.nan
        lo, hi = np.percentile(v, [50.0 * (1.0 - level), 100.0 - 50.0 * (1.0 - level)])
        return float(lo), float(hi)

    @property
    def se(self) -> float:
        """The standard deviation of the defined values (ddof 1); NaN with fewer than two."""
        v = self.defined
        return float(np.std(v, ddof=1)) if len(v) > 1 else math.nan

    def minus(self, other: "BootstrapResult") -> "BootstrapResult":
        """The paired difference ``self - other``, replicate by replicate: both must come from the same resamples (equal ``seed``,
        ``n``, ``first_replicate`` and number of replicates).  A replicate undefined in either is undefined in the difference."""
        if not isinstance(other, BootstrapResult):
            raise ValueError(f"other must be a BootstrapResult, got {type(other).__name__}")
        mine, theirs = (self.seed, self.n, self.first_replicate, len(self.values)), (other.seed, other.n, other.first_replicate, len(other.values))
        if mine != theirs:
            raise ValueError(f"the replicates are not paired: (seed, n, first_replicate, B) = {mine} against {theirs}")
        return BootstrapResult(self.estimate - other.estimate, self.values - other.values, self.seed, self.n, self.first_replicate)


def result_from_roc_counts(counts, seed: int, first_replicate: int = 0) -> BootstrapResult:
    """counts: int64 ``[1 + B, 4]``, the sample's row first -> the AUROC's :class:`BootstrapResult`."""
    c = _host(counts)
    auc = auc_from_counts(c[:, 1], c[:, 2], c[:, 3])
    return BootstrapResult(auc[0], auc[1:], seed, int(c[0, 0]), first_replicate)


def result_from_confusions(confs, metric, seed: int, first_replicate: int = 0) -> BootstrapResult:
    """confs: int64 ``[1 + B, C, C]``, the sample's confusion first -> the metric's :class:`BootstrapResult`."""
    c = _host(confs)
    v = np.asarray(resolve_metric(metric)(c), dtype=np.float64).reshape(-1)
    if v.shape[0] != c.shape[0]:
        raise ValueError(f"the metric returned {v.shape[0]} values for {c.shape[0]} confusions")
    return BootstrapResult(v[0], v[1:], seed, int(c[0].sum()), first_replicate)


def macro_mean(results: Sequence[BootstrapResult]) -> BootstrapResult:
    """The mean over per-class results of the same resamples; a replicate undefined for any class is undefined for the mean."""
    if not results:
        raise ValueError("no results")
    first = results[0]
    for r in results[1:]:
        first.minus(r)                                            # the pairing check
    est = np.stack([np.float64(r.estimate) for r in results]).sum(0) / len(results)
    vals = np.stack([r.values for r in results]).sum(0) / len(results)
    return BootstrapResult(est, vals, first.seed, first.n, first.first_replicate)
