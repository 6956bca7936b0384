"""Segmentation evaluation: how good is a heatmap against a pathologist's annotation.

The reference ends its segmentation flow with two functions (``WSI_evaluation/segment_utils.py:91-152``): ``eval_seg_auc`` labels every
tile from the ground-truth mask, takes the tile-level AUROC with scikit-learn and the threshold of the best ``tpr - fpr``;
``eval_seg_coarse`` takes the Dice of the predicted mask against the truth at level 16.  ``KEEPModel.tile_roc`` / ``mask_overlap`` /
``raster_sweep`` / ``annotation_tile_labels`` do that arithmetic on the device (``csrc/eval.hip``); this module holds the host side:
the result classes, the band planner of the tile labels, and the restatements in numpy -- :func:`roc_numpy`,
:func:`mask_counts_numpy`, :func:`raster_hist_numpy`, :func:`sweep_from_hist_numpy` -- which the device results equal exactly.

The ROC, in integers.  A NaN score removes its tile and -0.0 counts as +0.0.  With P positives and Nn negatives left,
``U2 = sum over the positives of (2 less + eq)`` (the negatives below / equal to the positive's score) and
``AUC = float(U2) / (2.0 * P * Nn)``: the exact area under the curve, ties as the trapezoid takes them, rounded once.  The curve has
one point per distinct score in descending order (``fps`` / ``tps``: the negatives / positives at or above it); ``kept`` marks what
``roc_curve(drop_intermediate=True)`` keeps (first, last, and every point where the second difference of ``fps`` or ``tps`` is not
zero).  The best threshold is the reference's ``thresholds[np.argmax(tpr - fpr)]``: over the kept points the first maximum of
``J = tps / P - fps / Nn`` in float64, and ``inf`` -- the point ``(0, 0)`` scikit-learn prepends -- when no kept point has ``J > 0``.

The sweep.  A raster pixel's score is its mean in 16-bit fixed point, ``m = (2 S + c) // (2 c)`` (``peak16``'s rule); the histogram
counts the pixels by truth and by ``m``, the uncovered ones in bin 65536.  "Predicted at threshold t" is ``m > t`` for ``t`` in
0..65535 (an uncovered pixel is never predicted), which is what ``wsi.segment_regions`` thresholds."""
import math
from typing import List, Optional, Tuple

import numpy as np
import torch

from .heatmap import COUNT_SHIFT, Q_ONE, SUM_MASK, _integer, quantize

HIST_BINS = Q_ONE + 2                                            # the means 0..65535, then the uncovered pixels
MAX_TILES = (1 << 24) - 1
MAX_PIXELS = 1 << 30
ONE_CLASS = "Only one class present in y_true. ROC AUC score is not defined in that case."       # scikit-learn's words


def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


# ------------------------------------------------------------------------------------------------ results
class RocResult:
    """``auc``, ``best_threshold`` (Python floats), ``n`` / ``n_pos`` / ``n_neg`` / ``u2`` (Python ints) and, unless the call asked for
    the scalars alone, the curve: ``thresholds`` fp32, ``fps`` / ``tps`` int32, ``kept`` bool, each ``[K]``, rows in descending
    threshold order -- device tensors from ``KEEPModel.tile_roc``, numpy arrays from :func:`roc_numpy`."""

    def __init__(self, n: int, n_pos: int, n_neg: int, u2: int, best_threshold: float, thresholds=None, fps=None, tps=None, kept=None):
        self.n, self.n_pos, self.n_neg, self.u2 = int(n), int(n_pos), int(n_neg), int(u2)
        if self.n_pos == 0 or self.n_neg == 0:
            raise ValueError(ONE_CLASS)
        self.auc = float(self.u2) / (2.0 * self.n_pos * self.n_neg)
        self.best_threshold = float(best_threshold)
        self.thresholds, self.fps, self.tps, self.kept = thresholds, fps, tps, kept

    def __repr__(self):
        return (f"RocResult(auc={self.auc:.6f}, best_threshold={self.best_threshold!r}, n={self.n}, n_pos={self.n_pos}, n_neg={self.n_neg}, "
                f"points={'none' if self.thresholds is None else len(self.thresholds)})")

    def _curve(self):
        if self.thresholds is None:
            raise ValueError("this result holds the scalars only: ask for curve=True")

    @property
    def fpr(self):
        """float64 [K]: ``fps / n_neg``."""
        self._curve()
        return self.fps.to(torch.float64) / self.n_neg if isinstance(self.fps, torch.Tensor) else self.fps.astype(np.float64) / self.n_neg

    @property
    def tpr(self):
        """float64 [K]: ``tps / n_pos``."""
        self._curve()
        return self.tps.to(torch.float64) / self.n_pos if isinstance(self.tps, torch.Tensor) else self.tps.astype(np.float64) / self.n_pos

    def sklearn_curve(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``(fpr, tpr, thresholds)`` as ``sklearn.metrics.roc_curve`` returns them (host arrays): the kept points behind the
        prepended ``(0, 0)`` with threshold ``inf``."""
        self._curve()
        kept = _host(self.kept).astype(bool)
        fps = np.r_[0, _host(self.fps)[kept]].astype(np.float64)
        tps = np.r_[0, _host(self.tps)[kept]].astype(np.float64)
        return fps / fps[-1], tps / tps[-1], np.r_[np.float32(np.inf), _host(self.thresholds)[kept]].astype(np.float32)


class MaskOverlap:
    """The four counts of two masks ``a`` and ``b`` (over ``within``, or all pixels): ``a``, ``b``, ``both`` set, ``considered``."""

    def __init__(self, a: int, b: int, both: int, considered: int):
        self.a, self.b, self.both, self.considered = int(a), int(b), int(both), int(considered)

    def __repr__(self):
        return f"MaskOverlap(a={self.a}, b={self.b}, both={self.both}, considered={self.considered}, dice={self.dice:.6f})"

    def __eq__(self, other):
        return isinstance(other, MaskOverlap) and self.counts == other.counts

    @property
    def counts(self) -> Tuple[int, int, int, int]:
        return self.a, self.b, self.both, self.considered

    @property
    def dice(self):
        """``2 both / (a + b)`` in Python integers, ``1`` when neither mask has a pixel (segment_utils.py:147-151)."""
        return 1 if self.a + self.b == 0 else 2 * self.both / (self.a + self.b)

    @property
    def iou(self):
        union = self.a + self.b - self.both
        return 1 if union == 0 else self.both / union

    @property
    def confusion(self) -> Tuple[Tuple[int, int], Tuple[int, int]]:
        """``((tn, fp), (fn, tp))`` with ``a`` as the truth and ``b`` as the prediction: ``sklearn.metrics.confusion_matrix``'s layout."""
        return ((self.considered - self.a - self.b + self.both, self.b - self.both), (self.a - self.both, self.both))


class RasterSweep:
    """Every threshold of a raster against a truth mask at once.  ``hist`` int64 ``[2, 65537]`` by truth; ``tp`` / ``fp`` / ``fn`` int64
    ``[65536]`` and ``dice`` float64 ``[65536]`` of "mean16 > t" for t = 0..65535 (device tensors from ``KEEPModel.raster_sweep``, numpy
    arrays from :func:`sweep_from_hist_numpy`); ``best_t16`` the threshold of the best Dice, the lowest on ties, ``best_threshold =
    best_t16 / 65535``, ``best_dice``; ``n_pos`` / ``n_neg`` the truth's pixels; ``u2`` and ``auc``: the pixel-level AUROC of the mean
    (an uncovered pixel scores below every covered one), exact as in :class:`RocResult`, NaN with one class only."""

    def __init__(self, hist, tp, fp, fn, dice, best_t16: int, n_pos: int, n_neg: int, u2: int):
        self.hist, self.tp, self.fp, self.fn, self.dice = hist, tp, fp, fn, dice
        self.best_t16, self.n_pos, self.n_neg, self.u2 = int(best_t16), int(n_pos), int(n_neg), int(u2)
        self.best_threshold = self.best_t16 / Q_ONE
        self.best_dice = float(dice[self.best_t16])
        self.auc = self.u2 / (2 * self.n_pos * self.n_neg) if self.n_pos and self.n_neg else math.nan

    def __repr__(self):
        return (f"RasterSweep(best_threshold={self.best_threshold:.6f}, best_dice={self.best_dice:.6f}, auc={self.auc:.6f}, n_pos={self.n_pos}, "
                f"n_neg={self.n_neg})")

    def overlap_at(self, thd) -> MaskOverlap:
        """The counts of the truth against "mean16 > quantize(thd)"."""
        t = quantize(thd)
        tp, fp, fn = int(self.tp[t]), int(self.fp[t]), int(self.fn[t])
        return MaskOverlap(tp + fn, tp + fp, tp, self.n_pos + self.n_neg)

    def dice_at(self, thd):
        return self.overlap_at(thd).dice


# ------------------------------------------------------------------------------------------------ argument checks
def check_roc_args(scores, labels) -> int:
    """scores: floating [N]; labels: uint8 / bool / integer [N] -> N."""
    ss, ls = tuple(scores.shape), tuple(labels.shape)
    if len(ss) != 1 or ls != ss:
        raise ValueError(f"scores and labels must both be [N], got {ss} and {ls}")
    sd, ld = scores.dtype, labels.dtype
    if not (sd.is_floating_point if isinstance(sd, torch.dtype) else sd.kind == "f"):
        raise ValueError(f"scores must be floating point, got {sd}")
    if ld.is_floating_point or ld.is_complex if isinstance(ld, torch.dtype) else ld.kind not in "iub":
        raise ValueError(f"labels must be bool or integers (non-zero = positive), got {ld}")
    if ss[0] > MAX_TILES:
        raise ValueError(f"at most 2^24 - 1 tiles, got {ss[0]}")
    if ss[0] == 0:
        raise ValueError("no tiles: the ROC of nothing is not defined")
    return int(ss[0])


def check_mask(m, name: str, shape=None):
    """A uint8 / bool ``[h,w]`` numpy array or torch tensor, or a ``TissueMask`` (its mask) -> the array as given."""
    from .region import TissueMask
    if isinstance(m, TissueMask):
        m = m.mask
    ok = (isinstance(m, np.ndarray) and m.dtype in (np.uint8, np.bool_)) or (isinstance(m, torch.Tensor) and m.dtype in (torch.uint8, torch.bool))
    if not ok or m.ndim != 2:
        raise ValueError(f"{name} must be a [h, w] bool or uint8 array or a TissueMask, got {getattr(m, 'dtype', type(m))} "
                         f"{tuple(getattr(m, 'shape', ()))}")
    h, w = int(m.shape[0]), int(m.shape[1])
    if h < 1 or w < 1 or h * w > MAX_PIXELS:
        raise ValueError(f"{name} of {h}x{w} pixels: need 1 <= h * w <= 2^30")
    if shape is not None and (h, w) != tuple(shape):
        raise ValueError(f"{name} has shape {(h, w)}, expected {tuple(shape)}")
    return m


def check_same_geometry(raster, mask, name: str) -> None:
    """A ``TissueMask`` beside a raster must have its downsample and shape, as ``wsi.segment_regions`` asks of ``tissue``."""
    from .region import TissueMask
    if isinstance(mask, TissueMask) and (mask.downsample != raster.downsample or tuple(mask.mask.shape) != raster.shape):
        raise ValueError(f"{name} mask has downsample {mask.downsample} and shape {tuple(mask.mask.shape)}, the raster "
                         f"{raster.downsample} and {raster.shape}")


# ------------------------------------------------------------------------------------------------ the restatements
def roc_numpy(scores, labels, curve: bool = True) -> RocResult:
    """The tile ROC restated on the host in numpy -> :class:`RocResult` with numpy arrays.  ``scores`` are rounded to float32 first."""
    s, l = _host(scores), _host(labels)
    check_roc_args(s, l)
    s = s.astype(np.float32)
    ok = ~np.isnan(s)
    s, pos = s[ok] + np.float32(0), l[ok] != 0                  # -0.0 + 0.0 = +0.0
    sp, sn = np.sort(s[pos]), np.sort(s[~pos])
    P, Nn = len(sp), len(sn)
    if P == 0 or Nn == 0:
        raise ValueError(ONE_CLASS)
    less, upto = np.searchsorted(sn, sp, "left").astype(np.int64), np.searchsorted(sn, sp, "right").astype(np.int64)
    u2 = int((less + upto).sum())                                # 2 less + eq = less + (less + eq)
    thr = np.unique(s)[::-1].copy()
    tps = (P - np.searchsorted(sp, thr, "left")).astype(np.int32)
    fps = (Nn - np.searchsorted(sn, thr, "left")).astype(np.int32)
    kept = np.ones(len(thr), bool)
    if len(thr) > 2:
        kept[1:-1] = (np.diff(fps.astype(np.int64), 2) != 0) | (np.diff(tps.astype(np.int64), 2) != 0)
    rows = np.flatnonzero(kept)
    j = tps[rows].astype(np.float64) / np.float64(P) - fps[rows].astype(np.float64) / np.float64(Nn)
    a = int(np.argmax(j))                                        # the first maximum
    best = float(thr[rows[a]]) if j[a] > 0 else math.inf
    return RocResult(P + Nn, P, Nn, u2, best, *((thr, fps, tps, kept) if curve else ()))


def mask_counts_numpy(a, b, within=None) -> np.ndarray:
    """int64 [4]: over the pixels where ``within`` is set (all without it), those set in ``a``, in ``b``, in both, and their number."""
    a = _host(check_mask(a, "a")) != 0
    b = _host(check_mask(b, "b", a.shape)) != 0
    w = np.ones(a.shape, bool) if within is None else _host(check_mask(within, "within", a.shape)) != 0
    return np.array([(a & w).sum(), (b & w).sum(), (a & b & w).sum(), w.sum()], np.int64)


def mean16_numpy(acc) -> np.ndarray:
    """int64 [h,w]: a raster pixel's mean in 16-bit fixed point, ``(2 S + c) // (2 c)``, and 65536 where no tile covers it."""
    a = _host(acc).view(np.uint64)
    S, c = (a & np.uint64(SUM_MASK)).astype(np.int64), (a >> np.uint64(COUNT_SHIFT)).astype(np.int64)
    return np.where(c > 0, np.minimum((2 * S + c) // np.maximum(2 * c, 1), Q_ONE), Q_ONE + 1)


def raster_hist_numpy(acc, truth, within=None) -> np.ndarray:
    """int64 [2, 65537]: the pixels (inside ``within``) by truth and by :func:`mean16_numpy`.  ``acc``: a raster's accumulator."""
    m = mean16_numpy(acc)
    t = _host(check_mask(truth, "truth", m.shape)) != 0
    w = np.ones(m.shape, bool) if within is None else _host(check_mask(within, "within", m.shape)) != 0
    return np.stack([np.bincount(m[w & (t == k)], minlength=HIST_BINS) for k in (False, True)]).astype(np.int64)


def _sweep(hist, xp) -> RasterSweep:
    """The sweep from a histogram: ``xp`` is numpy or torch, and both run the same integer and float64 operations."""
    cat = np.concatenate if xp is np else torch.cat
    f64 = (lambda v: v.astype(np.float64)) if xp is np else (lambda v: v.to(torch.float64))
    pos, neg = hist[1], hist[0]
    n_pos, n_neg = int(pos.sum()), int(neg.sum())
    cov_pos, cov_neg = pos[:Q_ONE + 1], neg[:Q_ONE + 1]
    tp = int(cov_pos.sum()) - xp.cumsum(cov_pos, 0)              # the covered pixels with m > t
    fp = int(cov_neg.sum()) - xp.cumsum(cov_neg, 0)
    fn = n_pos - tp
    den = 2 * tp + fp + fn
    dice = f64(2 * tp) / f64(den + (den == 0))                   # IEEE float64 on both sides
    dice[den == 0] = 1.0
    best = int(xp.nonzero(dice == dice.max())[0][0])             # the lowest threshold among equals
    # scores in ascending order: the uncovered pixels first, then the means 0..65535
    p, eq = cat([pos[Q_ONE + 1:], pos[:Q_ONE + 1]]), cat([neg[Q_ONE + 1:], neg[:Q_ONE + 1]])
    term, on = 2 * (xp.cumsum(eq, 0) - eq) + eq, p > 0           # a product fits an int64 (< 2^61); their sum may not: Python adds them
    u2 = sum(a * b for a, b in zip(p[on].tolist(), term[on].tolist()))
    return RasterSweep(hist, tp, fp, fn, dice, best, n_pos, n_neg, u2)


def sweep_from_hist_numpy(hist) -> RasterSweep:
    """The threshold sweep of a ``[2, 65537]`` histogram restated on the host -> :class:`RasterSweep` with numpy arrays."""
    h = _host(hist)
    if h.shape != (2, HIST_BINS) or h.dtype != np.int64:
        raise ValueError(f"hist must be int64 [2, {HIST_BINS}], got {h.dtype} {h.shape}")
    return _sweep(h, np)


def sweep_from_hist(hist: torch.Tensor) -> RasterSweep:
    """The same with torch operations on the histogram's device (cumulative sums; a few scalars are read back)."""
    if tuple(hist.shape) != (2, HIST_BINS) or hist.dtype != torch.int64:
        raise ValueError(f"hist must be int64 [2, {HIST_BINS}], got {hist.dtype} {tuple(hist.shape)}")
    return _sweep(hist, torch)


# ------------------------------------------------------------------------------------------------ tile labels from an annotation
def plan_label_bands(ys, x0: int, x1: int, patch: int, max_band_bytes: int = 1 << 28) -> List[Tuple[int, int]]:
    """The horizontal bands in which a level-0 annotation mask is filled to label tiles -> ``[(y_first, y_last), ...]``: band k
    holds the tiles whose top edge ``y`` lies in ``[y_first, y_last]`` (both are tile rows of ``ys``), its mask covers the level-0
    rows ``[y_first, y_last + patch)`` and the columns ``[x0, x1)`` -- whole tiles, so no tile is clipped and the labels do not depend
    on the banding -- and takes at most ``max_band_bytes`` bytes (and at most the 2^28 cells a fill accepts).  Every tile row
    belongs to exactly one band.  One tile row that does not fit is a ValueError that names the cap."""
    patch, cap, width = _integer(patch, "patch_size"), _integer(max_band_bytes, "max_band_bytes"), int(x1) - int(x0)
    if patch < 1 or width < patch or cap < 1:
        raise ValueError(f"need patch_size >= 1, x1 - x0 >= patch_size and max_band_bytes >= 1, got {patch}, {width}, {cap}")
    rows = np.unique(np.asarray(ys, dtype=np.int64))
    max_h = min(cap // width, (1 << 28) // (width + 1))
    if len(rows) and patch > max_h:
        raise ValueError(f"one tile row of {patch} x {width} level-0 pixels does not fit max_band_bytes = {cap} "
                         f"(or the 2^28 cells of one fill): raise the cap or label fewer columns at once")
    bands, k = [], 0
    while k < len(rows):
        e = int(np.searchsorted(rows, rows[k] + max_h - patch, "right")) - 1      # the last row with y + patch - y_first <= max_h
        bands.append((int(rows[k]), int(rows[e])))
        k = e + 1
    return bands


def default_eval_shape(coords, polys, patch: int, downsample: int = 16) -> Tuple[int, int]:
    """The smallest ``(h, w)`` at ``downsample`` (origin 0) whose pixels cover every tile ``[x, x + patch) x [y, y + patch)`` and every
    vertex of ``polys`` (a ``PolygonSet`` or None); at least ``(1, 1)``."""
    d = int(downsample)
    c = np.asarray(_host(coords), dtype=np.int64).reshape(-1, 2)
    far = [1, 1]                                                 # exclusive level-0 extents (x, y)
    if len(c):
        far = [max(far[k], int(c[:, k].max()) + int(patch)) for k in (0, 1)]
    if polys is not None and len(polys.vertices):
        far = [max(far[k], int(polys.vertices[:, k].max()) + 1) for k in (0, 1)]
    return -(-far[1] // d), -(-far[0] // d)


def resolve_annotation(mask_path):
    """What ``eval_seg_auc`` / ``eval_seg_coarse`` / ``zero_shot_segment`` take as ``mask_path`` -> ``(PolygonSet | TissueMask, order)``,
    or None for anything else (a slide file needs openslide): a ``PolygonSet``; a pair ``(PolygonSet, order)`` (``CAMELYON16_ORDER``);
    a ``TissueMask``; a path ending in ``.xml`` (ASAP) or ``.geojson`` / ``.json``."""
    import os
    from .annotation import PolygonSet
    from .region import TissueMask
    if isinstance(mask_path, (PolygonSet, TissueMask)):
        return mask_path, None
    if isinstance(mask_path, (tuple, list)) and len(mask_path) == 2 and isinstance(mask_path[0], PolygonSet):
        return mask_path[0], mask_path[1]
    if isinstance(mask_path, (str, os.PathLike)):
        name = os.fspath(mask_path).lower()
        if name.endswith(".xml"):
            return PolygonSet.from_asap_xml(os.fspath(mask_path)), None
        if name.endswith((".geojson", ".json")):
            return PolygonSet.from_geojson(os.fspath(mask_path)), None
    return None
