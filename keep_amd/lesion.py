"""Lesion-level scoring: which points does a heatmap propose, which annotated lesion does each one hit, and
what is the sensitivity at 1/4 ... 8 false positives per slide (FROC) -- the score a CAMELYON16-style challenge is judged by.

``KEEPModel.mask_distance`` / ``dilate_mask`` / ``erode_mask`` / ``evaluation_mask`` / ``raster_peaks`` / ``lesion_hits`` do the pixel and
candidate work on the device (``csrc/lesion.hip``); this module holds the host side: the result classes, the argument checks, the
:class:`FrocAccumulator` and the restatements in numpy -- :func:`dist2_numpy`, :func:`peaks_numpy`, :func:`lesion_hits_numpy`,
:func:`froc_numpy` -- which the device results equal exactly.

The rules, all in integers.  ``d2`` is the squared Euclidean distance in pixels to the nearest set (or zero) pixel, exact up to
``R^2`` and ``R^2 + 1`` beyond; pixels outside the image do not exist.  "Within ``T`` pixels" is ``sqrt(d2) < T`` in float64, which is the
integer test ``d2 <= k`` with ``k = max{v <= R^2 : sqrt(v) < T}``, ``R = ceil(T)`` (:func:`distance_threshold`).  The evaluation mask is
the truth dilated by the margin, its holes (4-connected background that touches no border) filled, labelled 8-connected.  A raster
pixel's value is its mean in 16-bit fixed point, ``m = (2 S + c) // (2 c)``; a pixel is a peak iff it is eligible (covered and inside
the tissue mask), ``m >= min16`` and no other eligible pixel of its ``(2 r + 1)^2`` window has a larger ``m``, or the same ``m`` and a lower
row-major index.  A candidate hits the label under it; a lesion's score is the largest ``max(score, 0)`` of its hits.  The FROC
curve is the published rule of the CAMELYON16 evaluation restated (:func:`froc_numpy`), and its isolated-tumour-cell rule (a major
axis length below 275 um) is ``evaluation_mask(ignore_major_axis=)`` on the device's integer moments (``keep_amd.morphometry``,
DESIGN.md section 21).  Parity with that script itself and with scikit-image's ``major_axis_length`` is unpinned: neither is
available here."""
import math
from typing import Iterable, Optional, Tuple

import numpy as np
import torch

from .heatmap import COUNT_SHIFT, Q_ONE, SUM_MASK, _integer

MAX_RADIUS = 1024                                             # of the distance transform
MAX_PEAK_RADIUS = 127
MAX_PIXELS = 1 << 30
MAX_CANDIDATES = (1 << 24) - 1
MAX_LABELS = 1 << 20
FROC_POINTS = (0.25, 0.5, 1.0, 2.0, 4.0, 8.0)                 # average false positives per slide at which the sensitivity is read
DIRECTIONS = ("foreground", "background")


def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


# ------------------------------------------------------------------------------------------------ results
class EvaluationMask:
    """The lesions a detection may hit.  ``labels`` int32 ``[h,w]`` (0 = background, lesions 1..n in the row-major order of their first
    pixels), ``n``, ``table`` (the ``RegionTable`` of the labelling, or None from the restatement), ``ignore`` uint8 ``[n]`` (1: hits on
    this lesion are neither true nor false positives and it does not count as a lesion; callers may overwrite it), ``downsample``
    and ``origin``: the level-0 geometry of pixel (0, 0)."""

    def __init__(self, labels, n: int, table, ignore, downsample: int, origin=(0, 0)):
        self.labels, self.n, self.table, self.ignore = labels, int(n), table, ignore
        self.downsample, self.origin = int(downsample), (int(origin[0]), int(origin[1]))

    def __repr__(self):
        return f"EvaluationMask({tuple(self.labels.shape)}, n={self.n}, downsample={self.downsample}, origin={self.origin})"


class LesionCandidates:
    """The peaks of one raster: ``xy`` int64 ``[n,2]``, level-0 ``(x, y)`` of the centre of the raster pixel (``origin + px * d + d // 2``),
    ``scores`` float32 ``[n]`` (``float32(float64(m) / 65535)``) and ``m16`` int64 ``[n]``, rows in ascending row-major order of the pixels."""

    def __init__(self, xy, scores, m16=None):
        self.xy, self.scores, self.m16 = xy, scores, m16

    def __len__(self) -> int:
        return int(self.xy.shape[0])

    def __repr__(self):
        return f"LesionCandidates(n={len(self)})"


class LesionHits:
    """One slide's detections against its lesions: ``hit`` int32 ``[N]`` (the label, 0 = a false positive, -1 = a NaN score),
    ``lesion_max`` float32 ``[n]`` (the best score on every lesion; 0 for one never hit, or ignored), ``n_lesions = n - ignored`` and
    ``fp_scores``: the scores whose hit is 0."""

    def __init__(self, hit, lesion_max, n_lesions: int, fp_scores):
        self.hit, self.lesion_max, self.n_lesions, self.fp_scores = hit, lesion_max, int(n_lesions), fp_scores

    def __repr__(self):
        return f"LesionHits(candidates={int(self.hit.shape[0])}, lesions={self.n_lesions}, false_positives={int(self.fp_scores.shape[0])})"


class FrocCurve:
    """``thresholds`` float32 ``[K]`` ascending, ``fps`` / ``tps`` int64 ``[K + 1]`` (the false positives / lesions scoring at or above every
    threshold, then the closing row ``(0, 0)``), ``avg_fps`` / ``sensitivity`` float64 ``[K + 1]``, ``score`` (the mean sensitivity at
    :data:`FROC_POINTS`), ``n_slides`` and ``n_lesions``: numpy arrays on the host."""

    def __init__(self, thresholds, fps, tps, n_slides: int, n_lesions: int):
        self.thresholds = np.asarray(thresholds, np.float32)
        self.fps, self.tps = np.asarray(fps, np.int64), np.asarray(tps, np.int64)
        self.n_slides, self.n_lesions = int(n_slides), int(n_lesions)
        self.avg_fps = self.fps.astype(np.float64) / np.float64(self.n_slides)
        self.sensitivity = self.tps.astype(np.float64) / np.float64(self.n_lesions)
        self.sensitivity_at = np.interp(FROC_POINTS, self.avg_fps[::-1], self.sensitivity[::-1])
        self.score = float(np.mean(self.sensitivity_at))

    def __repr__(self):
        return f"FrocCurve(score={self.score:.6f}, points={len(self.fps)}, n_slides={self.n_slides}, n_lesions={self.n_lesions})"

    def __eq__(self, other):
        return (isinstance(other, FrocCurve) and (self.n_slides, self.n_lesions, self.score) == (other.n_slides, other.n_lesions, other.score)
                and np.array_equal(self.thresholds.view(np.int32), other.thresholds.view(np.int32)) and np.array_equal(self.fps, other.fps)
                and np.array_equal(self.tps, other.tps))


# ------------------------------------------------------------------------------------------------ argument checks
def check_radius(radius, limit: int = MAX_RADIUS, name: str = "radius") -> int:
    r = _integer(radius, name)
    if r < 1 or r > limit:
        raise ValueError(f"{name} must lie in [1, {limit}], got {r}")
    return r


def check_direction(to: str) -> int:
    """-> the kernel's ``invert``: 0 for the distance to the foreground, 1 to the background."""
    if to not in DIRECTIONS:
        raise ValueError(f"to must be one of {DIRECTIONS}, got {to!r}")
    return DIRECTIONS.index(to)


def distance_threshold(distance) -> Tuple[int, int]:
    """-> ``(R, k)``: ``R = ceil(distance)`` and ``k = max{v <= R^2 : math.sqrt(v) < distance}``, so that for every squared distance ``d2``
    capped at ``R^2 + 1``, ``d2 <= k`` iff ``sqrt(d2) < distance`` in float64 (the square root of an integer is rounded once)."""
    t = float(distance)
    if not 0 < t <= MAX_RADIUS:
        raise ValueError(f"distance must lie in (0, {MAX_RADIUS}] pixels, got {distance!r}")
    R = math.ceil(t)
    k = min(int(t * t), R * R)
    while math.sqrt(k) >= t:
        k -= 1
    while k < R * R and math.sqrt(k + 1) < t:
        k += 1
    return R, k


def camelyon16_margin(mpp: float = 0.243, downsample: int = 32) -> float:
    """The margin of the CAMELYON16 evaluation mask in mask pixels: 75 um on either side of the annotation,
    ``75 / (mpp * downsample * 2)`` as the published evaluation writes it (4.82 pixels at level 5 of a 0.243 um slide)."""
    return 75 / (float(mpp) * downsample * 2)


def check_peak_args(radius, min_score, max_peaks) -> Tuple[int, int, int]:
    """-> (radius, min16, max_peaks)."""
    from .heatmap import quantize
    r = check_radius(radius, MAX_PEAK_RADIUS)
    cap = _integer(max_peaks, "max_peaks")
    if cap < 0:
        raise ValueError(f"max_peaks must be >= 0, got {cap}")
    return r, quantize(min_score), cap


def check_peak_count(n: int, max_peaks: int) -> int:
    if n > max_peaks:
        raise ValueError(f"the raster has {n} peaks, max_peaks is {max_peaks}: raise min_score, radius or max_peaks")
    return n


def check_candidates(xy, scores) -> int:
    """xy: integers [N,2]; scores: floating [N] -> N."""
    from .heatmap import check_tiles
    n = check_tiles(xy, scores)
    if n > MAX_CANDIDATES:
        raise ValueError(f"at most 2^24 - 1 candidates, got {n}")
    return n


# ------------------------------------------------------------------------------------------------ the restatements
def dist2_numpy(mask, radius, to: str = "foreground") -> np.ndarray:
    """The capped squared distance restated on the host -> uint32 ``[h,w]``: the two passes of the kernel in numpy."""
    R, invert = check_radius(radius), check_direction(to)
    b = (_host(mask) != 0) != bool(invert)
    if b.ndim != 2 or b.size < 1:
        raise ValueError(f"mask must be [h, w] with h, w >= 1, got {b.shape}")
    h, w = b.shape
    rows = np.arange(h, dtype=np.int64)[:, None]
    above = np.maximum.accumulate(np.where(b, rows, -(R + 1) - h), axis=0)                     # the last such row at or above
    below = np.minimum.accumulate(np.where(b, rows, 2 * h + R + 1)[::-1], axis=0)[::-1]        # the first at or below
    g = np.minimum(np.minimum(rows - above, below - rows), R + 1)
    cap = R * R + 1
    best = np.minimum(g * g, cap)
    for dx in range(1, min(R, w - 1) + 1 if int(g.min()) <= R else 0):      # no column within R rows of a pixel: all sentinel
        if dx * dx >= int(best.max()):                                      # as the kernel's threads stop
            break
        best[:, dx:] = np.minimum(best[:, dx:], g[:, :-dx] ** 2 + dx * dx)
        best[:, :-dx] = np.minimum(best[:, :-dx], g[:, dx:] ** 2 + dx * dx)
    return best.astype(np.uint32)


def mean16_keys_numpy(acc, mask=None) -> np.ndarray:
    """uint64 ``[h,w]``: ``(m + 1) << 32 | (0xFFFFFFFF - index)`` for the eligible pixels, 0 elsewhere."""
    a = _host(acc)
    if a.dtype != np.int64 or a.ndim != 2:
        raise ValueError(f"acc must be int64 [h, w], got {a.dtype} {a.shape}")
    a = a.view(np.uint64)
    S, c = (a & np.uint64(SUM_MASK)).astype(np.int64), (a >> np.uint64(COUNT_SHIFT)).astype(np.int64)
    on = c > 0
    if mask is not None:
        on &= _host(mask) != 0
    m = np.minimum((2 * S + c) // np.maximum(2 * c, 1), Q_ONE)
    index = np.arange(a.size, dtype=np.int64).reshape(a.shape)
    return np.where(on, ((m + 1) << 32) | (0xFFFFFFFF - index), 0).astype(np.uint64)


def _window_max(a: np.ndarray, r: int, axis: int) -> np.ndarray:
    """The maximum over ``|d| <= r`` along ``axis`` (zero beyond the ends), by doubling: O(log r) passes."""
    a = np.moveaxis(a, axis, -1)
    n, width = a.shape[-1], 2 * r + 1
    cur = np.concatenate([np.zeros(a.shape[:-1] + (r,), a.dtype), a, np.zeros(a.shape[:-1] + (r,), a.dtype)], axis=-1)    # cur[i]: window 1 at i - r
    span = 1
    while 2 * span <= width:
        cur = np.maximum(cur[..., :cur.shape[-1] - span], cur[..., span:])
        span *= 2
    out = np.maximum(cur[..., :n], cur[..., width - span:width - span + n])                  # [i, i + span) and [i + width - span, i + width)
    return np.moveaxis(out, -1, axis)


def peaks_numpy(acc, radius, min16: int = 0, mask=None) -> np.ndarray:
    """The peaks restated on the host -> int64 ``[n,3]``, rows ``(x, y, m)`` in ascending row-major order."""
    r = check_radius(radius, MAX_PEAK_RADIUS)
    key = mean16_keys_numpy(acc, mask)
    best = _window_max(_window_max(key, r, 1), r, 0)
    m = (key >> np.uint64(32)).astype(np.int64) - 1
    ys, xs = np.nonzero((key != 0) & (key == best) & (m >= int(min16)))
    return np.stack([xs, ys, m[ys, xs]], axis=1).astype(np.int64).reshape(-1, 3)


def candidates_numpy(peaks: np.ndarray, downsample: int, origin=(0, 0)) -> LesionCandidates:
    """Peak rows ``(x, y, m)`` -> :class:`LesionCandidates` with numpy arrays."""
    p = np.asarray(peaks, np.int64).reshape(-1, 3)
    d = int(downsample)
    xy = p[:, :2] * d + np.asarray(origin, np.int64) + d // 2
    return LesionCandidates(xy, (p[:, 2].astype(np.float64) / np.float64(Q_ONE)).astype(np.float32), p[:, 2].copy())


def lesion_hits_numpy(xy, scores, labels, downsample: int, origin=(0, 0), n_labels: Optional[int] = None, ignore=None) -> LesionHits:
    """The look-up and the per-lesion maxima restated on the host -> :class:`LesionHits` with numpy arrays."""
    xy, s, lab = _host(xy).astype(np.int64).reshape(-1, 2), _host(scores).astype(np.float32).reshape(-1), _host(labels)
    n = int(lab.max(initial=0)) if n_labels is None else int(n_labels)
    ig = np.zeros(n, bool) if ignore is None else _host(ignore).astype(bool)
    d, (hm, wm) = int(downsample), lab.shape
    px, py = (xy[:, 0] - int(origin[0])) // d, (xy[:, 1] - int(origin[1])) // d             # numpy floors
    inside = (px >= 0) & (px < wm) & (py >= 0) & (py < hm)
    v = np.zeros(len(s), np.int64)
    v[inside] = lab[py[inside], px[inside]]
    hit = np.where((v >= 1) & (v <= n), v, 0)
    nan = np.isnan(s)
    hit[nan] = -1
    pos = np.where(s > 0, s, np.float32(0)).astype(np.float32)                              # max(s, +0.0)
    best = np.zeros(n, np.float32)
    for l, p in zip(hit.tolist(), pos.tolist()):
        if l > 0 and not ig[l - 1] and p > best[l - 1]:
            best[l - 1] = p
    return LesionHits(hit.astype(np.int32), best, n - int(ig.sum()), s[hit == 0] + np.float32(0))


def _populations(slides) -> Tuple[list, list, int, int]:
    fps, tps, n_slides, n_lesions = [], [], 0, 0
    for s in slides:
        if not isinstance(s, LesionHits):
            raise ValueError(f"a slide must be a LesionHits, got {type(s).__name__}")
        fps.append(s.fp_scores)
        tps.append(s.lesion_max)
        n_slides += 1
        n_lesions += s.n_lesions
    if n_lesions == 0:
        raise ValueError(f"{n_slides} slides with no lesion at all: the sensitivity is not defined")
    return fps, tps, n_slides, n_lesions


def froc_numpy(slides: Iterable[LesionHits]) -> FrocCurve:
    """The FROC curve of the CAMELYON16 evaluation, restated on the host.  ``FP``: every slide's ``fp_scores``; ``TP``: every slide's
    ``lesion_max``, the zeros of the missed and the ignored lesions included; ``T``: the ascending distinct values of both, the
    thresholds are ``T[1:]``; per threshold ``fps = #{FP >= t}`` and ``tps = #{TP >= t}``, then one closing row ``(0, 0)``."""
    fps, tps, n_slides, n_lesions = _populations(slides)
    fp = np.concatenate([_host(v).astype(np.float32).reshape(-1) for v in fps])
    tp = np.concatenate([_host(v).astype(np.float32).reshape(-1) for v in tps])
    t = np.unique(np.concatenate([fp, tp]) + np.float32(0))[1:]
    fp, tp = np.sort(fp), np.sort(tp)
    f = len(fp) - np.searchsorted(fp, t, "left")
    s = len(tp) - np.searchsorted(tp, t, "left")
    return FrocCurve(t, np.r_[f, 0], np.r_[s, 0], n_slides, n_lesions)


class FrocAccumulator:
    """``.add(LesionHits)`` once per slide, ``.curve()`` -> :class:`FrocCurve`.  With device tensors the counts come from the device:
    ``keep_sort_f32`` on each population and ``keep_rank_f32`` (``n - less``) at the distinct values; ``torch.unique`` / ``cat`` are
    plumbing.  With numpy arrays it is :func:`froc_numpy`.  The two are equal exactly."""

    def __init__(self, model=None):
        self.slides, self._model = [], model

    def add(self, hits: LesionHits) -> "FrocAccumulator":
        if not isinstance(hits, LesionHits):
            raise ValueError(f"add takes a LesionHits, got {type(hits).__name__}")
        self.slides.append(hits)
        return self

    def curve(self) -> FrocCurve:
        fps, tps, n_slides, n_lesions = _populations(self.slides)
        dev = next((v.device for v in fps + tps if isinstance(v, torch.Tensor) and v.device.type == "cuda"), None)
        if dev is None:
            return froc_numpy(self.slides)
        from .model import engine_for
        m = engine_for(device=dev, model=self._model)
        fp, tp = (torch.cat([torch.as_tensor(v).to(m._device, torch.float32).reshape(-1) for v in pop]) for pop in (fps, tps))
        t = torch.unique(torch.cat([fp, tp]) + 0.0)[1:].contiguous()

        def at_or_above(pop):
            if pop.shape[0] == 0 or t.shape[0] == 0:
                return np.zeros(int(t.shape[0]), np.int64)
            less = m._rank(m.score_reference(pop), t, False, False, True)[1]
            return int(pop.shape[0]) - less.cpu().numpy().astype(np.int64)
        return FrocCurve(t.cpu().numpy(), np.r_[at_or_above(fp), 0], np.r_[at_or_above(tp), 0], n_slides, n_lesions)
