"""Tile scores rasterised onto the slide thumbnail: the last stage of the slide flow.

``KEEPModel.tile_raster`` scatters per-tile values (the tumour probabilities of ``keep_amd.wsi.refine``) into a raster whose pixel
covers ``downsample`` x ``downsample`` level-0 pixels -- the geometry of ``KEEPModel.tissue_mask`` and of the thumbnail it was given --
and ``KEEPModel.render_heatmap`` blends the coloured mean over that thumbnail.  It replaces the pred-mask painting inside the
reference's ``eval_seg_coarse`` (``WSI_evaluation/segment_utils.py:134-140``) and the heatmap that closes CLAM's step of the
reference's ``README.md:74``.

Everything is integer arithmetic.  A value becomes ``q = rint(clip(float32(v), 0, 1) * 65535)`` (round half to even; NaN skips the
tile) and one uint64 per raster pixel holds the sum of q over the covering tiles in bits 0..39 and their number in bits 40..63.
The device kernels (``csrc/heatmap.hip``) equal the numpy restatements below exactly, and integer sums do not depend on the order, so
a raster is the same however its tiles are split over calls.

This module holds the host side: argument checks (ValueError before any device call), :class:`TileRaster`, the colour tables and
the restatements ``raster_numpy`` / ``mean_numpy`` / ``pred_numpy`` / ``render_numpy``; ``cell_raster_numpy`` restates the token-cell
raster of ``KEEPModel.cell_raster``.

The two display steps of CLAM's heatmaps follow below: rank percentiles of the tile values
(``KEEPModel.score_reference`` / ``percentiles``, :class:`ScoreReference`; ``sort_numpy`` / ``rank_numpy`` / ``percentiles_numpy``) and a
Gaussian smoothing of the raster under its support (``KEEPModel.smooth_raster``; ``gaussian_taps`` / ``clam_blur`` / ``smooth_numpy``),
integer-exact like the rest."""
from typing import Optional, Tuple

import numpy as np
import torch

COUNT_SHIFT = 40
SUM_MASK = (1 << COUNT_SHIFT) - 1
Q_ONE = 65535
MAX_TILES = (1 << 24) - 1                      # the count field; (2^24 - 1) * 65535 < 2^40, so neither field can overflow
MAX_PIXELS = 1 << 30
MAX_PATCH = 1 << 30
MAX_ORIGIN = 1 << 40
COLORMAPS = ("jet", "gray")


def _integer(v, name: str) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer, float)) or int(v) != v:
        raise ValueError(f"{name} must be an integer, got {v!r}")
    return int(v)


def check_raster_args(patch, downsample, shape, origin=(0, 0)) -> Tuple[int, int, Tuple[int, int], Tuple[int, int]]:
    """Validate the raster geometry on the host -> (patch, downsample, (h, w), (ox, oy))."""
    patch, d = _integer(patch, "patch_size"), _integer(downsample, "downsample")
    if patch < 1 or patch > MAX_PATCH:
        raise ValueError(f"patch_size must lie in [1, 2^30], got {patch}")
    if d < 1 or d > patch:
        raise ValueError(f"downsample must lie in [1, patch_size = {patch}], got {d}")
    if len(shape) != 2:
        raise ValueError(f"shape must be (h, w), got {shape!r}")
    h, w = _integer(shape[0], "shape[0]"), _integer(shape[1], "shape[1]")
    if h < 1 or w < 1 or h * w > MAX_PIXELS:
        raise ValueError(f"raster of {h}x{w} pixels: need 1 <= h * w <= 2^30")
    if len(origin) != 2:
        raise ValueError(f"origin must be two integers (x, y), got {origin!r}")
    ox, oy = _integer(origin[0], "origin[0]"), _integer(origin[1], "origin[1]")
    if ox % d or oy % d:
        raise ValueError(f"origin {(ox, oy)} must be a multiple of downsample {d}: raster pixel (0, 0) starts on the pixel lattice")
    if abs(ox) > MAX_ORIGIN or abs(oy) > MAX_ORIGIN:
        raise ValueError(f"origin {(ox, oy)} outside +-2^40")
    return patch, d, (h, w), (ox, oy)


def check_tiles(coords, values) -> int:
    """Shapes of one call's tiles: coords [N,2] of an integer type, values [N] of a floating type -> N."""
    cs, vs = tuple(coords.shape), tuple(values.shape)
    if len(cs) != 2 or cs[1] != 2 or len(vs) != 1 or vs[0] != cs[0]:
        raise ValueError(f"coords must be [N,2] and values [N], got {cs} and {vs}")
    cd = coords.dtype
    if cd in (torch.bool, np.dtype(bool)) or (cd.is_floating_point if isinstance(cd, torch.dtype) else cd.kind not in "iu"):
        raise ValueError(f"coords must hold integers, got {cd}")
    vd = values.dtype
    if not (vd.is_floating_point if isinstance(vd, torch.dtype) else vd.kind == "f"):
        raise ValueError(f"values must be floating point, got {vd}")
    return int(cs[0])


MAX_CELLS = 1 << 24                            # cells per tile of a cell raster


def check_cell_args(grid, patch, downsample, shape, origin=(0, 0)):
    """The geometry of a cell raster (``KEEPModel.cell_raster``) on the host -> ((gh, gw), patch, downsample, (h, w), (ox, oy)):
    :func:`check_raster_args`, a grid whose sides divide the patch, and a raster pixel no larger than a cell."""
    if len(grid) != 2:
        raise ValueError(f"grid must be (gh, gw), got {grid!r}")
    gh, gw = _integer(grid[0], "grid[0]"), _integer(grid[1], "grid[1]")
    patch = _integer(patch, "patch_size")
    if gh < 1 or gw < 1 or gh * gw > MAX_CELLS:
        raise ValueError(f"grid {(gh, gw)}: need gh, gw >= 1 and gh * gw <= 2^24")
    if patch < 1 or patch % gw or patch % gh:
        raise ValueError(f"patch_size {patch} must be a multiple of both sides of the grid {(gh, gw)}: cells are whole level-0 pixels")
    cmin = min(patch // gw, patch // gh)
    d = _integer(downsample, "downsample")
    if d < 1 or d > cmin:
        raise ValueError(f"downsample must lie in [1, cell side = {cmin}] (patch_size {patch}, grid {(gh, gw)}), got {d}")
    patch, d, shape, origin = check_raster_args(patch, d, shape, origin)
    return (gh, gw), patch, d, shape, origin


def check_cells(coords, values, grid) -> int:
    """Shapes of one call's tiles with cell values: coords [N,2] of an integer type, values [N, gh gw] of a floating type -> N."""
    cs, vs = tuple(coords.shape), tuple(values.shape)
    if len(vs) != 2 or vs[1] != grid[0] * grid[1]:
        raise ValueError(f"cell values must be [N, gh gw = {grid[0] * grid[1]}], got {vs}")
    return check_tiles(coords, values[:, 0])


def quantize(value) -> int:
    """One value in the raster's fixed point: rint(clip(float32(v), 0, 1) * 65535); NaN is an error here."""
    v = np.float32(value)
    if np.isnan(v):
        raise ValueError("a window / threshold value must not be NaN")
    return int(np.rint(np.clip(v, np.float32(0), np.float32(1)) * np.float32(Q_ONE)))


def render_args(alpha, window, min_value, background) -> Tuple[int, int, int, int, Tuple[int, int, int]]:
    """The display arguments as the integers the kernel takes -> (a, lo16, hi16, min16, (R, G, B))."""
    if isinstance(alpha, bool) or not (0.0 <= float(alpha) <= 1.0):
        raise ValueError(f"alpha must lie in [0, 1], got {alpha!r}")
    a = int(round(256 * float(alpha)))
    if len(window) != 2:
        raise ValueError(f"window must be (low, high), got {window!r}")
    lo16, hi16 = quantize(window[0]), quantize(window[1])
    if lo16 >= hi16:
        raise ValueError(f"window {tuple(window)!r} is empty in 16-bit fixed point ({lo16} >= {hi16})")
    bg = tuple(_integer(c, "background") for c in background)
    if len(bg) != 3 or any(c < 0 or c > 255 for c in bg):
        raise ValueError(f"background must be three integers in 0..255, got {background!r}")
    return a, lo16, hi16, quantize(min_value), bg


def colormap(name) -> np.ndarray:
    """A colour table, uint8 [256,3], built in integer arithmetic from the formulas below; a caller's own [256,3] uint8 array is
    checked and passed through.  No parity with matplotlib's tables of the same names is claimed: "jet" is the piecewise-linear
    blue -> cyan -> yellow -> red ramp ``channel(i) = clamp((765 - 2 |4 i - 255 k| + 1) // 2, 0, 255)`` with k = 3 / 2 / 1 for
    R / G / B (1.5 - |4 t - k| at t = i / 255, scaled to 0..255 and rounded half up), "gray" is ``(i, i, i)``."""
    if isinstance(name, str):
        i = np.arange(256, dtype=np.int64)
        if name == "jet":
            return np.stack([np.clip((765 - 2 * np.abs(4 * i - 255 * k) + 1) // 2, 0, 255) for k in (3, 2, 1)], axis=1).astype(np.uint8)
        if name == "gray":
            return np.stack([i, i, i], axis=1).astype(np.uint8)
        raise ValueError(f"colormap must be one of {COLORMAPS} or a uint8 [256,3] array, got {name!r}")
    lut = name.cpu().numpy() if isinstance(name, torch.Tensor) else np.asarray(name)
    if lut.dtype != np.uint8 or lut.shape != (256, 3):
        raise ValueError(f"a colour table must be uint8 [256,3], got {lut.dtype} {lut.shape}")
    return np.ascontiguousarray(lut)


_table = colormap                              # the name `colormap` is also the keyword of the render functions


class TileRaster:
    """An accumulator and its geometry: ``acc`` int64 ``[h,w]`` (bits 0..39 the sum of the fixed-point values of the tiles covering
    the pixel, bits 40..63 their number), ``downsample`` (level-0 pixels per raster pixel), ``patch`` (a tile's footprint in level-0
    units), ``origin`` (the level-0 position of raster pixel (0, 0)) and ``tiles``, the number of tiles added so far (NaN tiles
    included: the cap of 2^24 - 1 is enforced by counting on the host).  ``KEEPModel.tile_raster`` makes and extends one."""

    def __init__(self, acc: torch.Tensor, downsample: int, patch: int, origin=(0, 0), tiles: int = 0, model=None):
        if not isinstance(acc, torch.Tensor) or acc.dtype != torch.int64 or acc.dim() != 2 or not acc.is_contiguous():
            raise ValueError("acc must be a contiguous int64 [h,w] tensor")
        self.patch, self.downsample, _, self.origin = check_raster_args(patch, downsample, acc.shape, origin)
        self.acc = acc
        self.tiles = 0
        self._model = model
        self.claim(tiles)

    @property
    def shape(self) -> Tuple[int, int]:
        return int(self.acc.shape[0]), int(self.acc.shape[1])

    def __repr__(self):
        return (f"TileRaster({self.shape} on {self.acc.device}, downsample={self.downsample}, patch={self.patch}, origin={self.origin}, "
                f"tiles={self.tiles})")

    def claim(self, n: int) -> None:
        """Count ``n`` more tiles against the cap, before they are added; ValueError beyond 2^24 - 1."""
        n = _integer(n, "the number of tiles")
        if n < 0 or self.tiles + n > MAX_TILES:
            raise ValueError(f"a raster takes at most 2^24 - 1 = {MAX_TILES} tiles in all (its count field is 24 bits): {self.tiles} added, "
                             f"{n} more asked for")
        self.tiles += n

    def check_geometry(self, patch: int, downsample: int, shape, origin) -> None:
        if (self.patch, self.downsample, self.shape, self.origin) != (patch, downsample, tuple(shape), tuple(origin)):
            raise ValueError(f"into= raster has patch {self.patch}, downsample {self.downsample}, shape {self.shape}, origin {self.origin}; "
                             f"the call has {patch}, {downsample}, {tuple(shape)}, {tuple(origin)}")

    def _engine(self):
        from .model import engine_for
        if self.acc.device.type != "cuda":
            raise ValueError("this raster lives on the host: use the numpy restatements (mean_numpy, pred_numpy, render_numpy)")
        return engine_for(device=self.acc.device, model=self._model)

    def _read(self, uncovered: float, mean: bool, count: bool, pred: bool):
        return self._engine()._heat_read(self, float(uncovered), mean, count, pred)

    @property
    def sum(self) -> torch.Tensor:
        """int64 [h,w]: the sum of the 16-bit fixed-point values of the covering tiles."""
        return self.acc & SUM_MASK

    @property
    def count(self) -> torch.Tensor:
        """int32 [h,w]: the number of covering tiles."""
        return self._read(0.0, False, True, False)[1]

    def mean(self, uncovered: float = 0.0) -> torch.Tensor:
        """fp32 [h,w]: ``float32(float64(sum) / float64(65535 * count))`` where a tile covers the pixel, ``uncovered`` elsewhere."""
        return self._read(uncovered, True, False, False)[0]

    def pred(self) -> torch.Tensor:
        """uint8 {0,255} [h,w]: 255 where sum > 0.  With values ``p > thd`` this is "any covering tile above the threshold", the
        pred_mask of ``segment_utils.py:134-140``."""
        return self._read(0.0, False, False, True)[2]


# ------------------------------------------------------------------------------------------------ the restatements
def footprints_numpy(coords: np.ndarray, patch: int, d: int, shape, origin) -> np.ndarray:
    """int64 [N,4]: (c0, c1, r0, r1) of every tile, floor division (also below zero), clipped to the raster; empty when c1 <= c0 or
    r1 <= r0."""
    c = np.asarray(coords).astype(np.int64).reshape(-1, 2)
    x, y = c[:, 0] - origin[0], c[:, 1] - origin[1]
    h, w = shape
    return np.stack([np.clip(x // d, 0, None), np.clip((x + patch) // d, None, w), np.clip(y // d, 0, None), np.clip((y + patch) // d, None, h)],
                    axis=1)


def quantize_numpy(values: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """-> (q int64 [N], skip bool [N]): q = rint(clip(float32(v), 0, 1) * float32(65535)), skip where v is NaN."""
    v = np.asarray(values).astype(np.float32).reshape(-1)
    skip = np.isnan(v)
    q = np.rint(np.clip(np.where(skip, np.float32(0), v), np.float32(0), np.float32(1)) * np.float32(Q_ONE)).astype(np.int64)
    return q, skip


def raster_numpy(coords, values, patch: int, downsample: int, shape, origin=(0, 0), into: Optional[np.ndarray] = None) -> np.ndarray:
    """The accumulate step restated on the host -> the accumulator, int64 [h,w]; ``into`` adds to an earlier one (in place)."""
    patch, d, (h, w), origin = check_raster_args(patch, downsample, shape, origin)
    coords, values = np.asarray(coords), np.asarray(values)
    check_tiles(coords, values)
    if into is None:
        into = np.zeros((h, w), np.int64)
    elif into.dtype != np.int64 or into.shape != (h, w):
        raise ValueError(f"into must be int64 {(h, w)}, got {into.dtype} {into.shape}")
    acc = into.view(np.uint64)
    q, skip = quantize_numpy(values)
    fp = footprints_numpy(coords, patch, d, (h, w), origin)
    for n in np.nonzero(~skip & (fp[:, 1] > fp[:, 0]) & (fp[:, 3] > fp[:, 2]))[0]:
        c0, c1, r0, r1 = fp[n]
        acc[r0:r1, c0:c1] += np.uint64((1 << COUNT_SHIFT) | int(q[n]))
    return into


def cell_raster_numpy(coords, values, grid, patch: int, downsample: int, shape, origin=(0, 0), into: Optional[np.ndarray] = None) -> np.ndarray:
    """``KEEPModel.cell_raster`` restated on the host -> the accumulator, int64 [h,w]; ``into`` adds to an earlier one (in place).  A tile's
    footprint is :func:`footprints_numpy`'s; pixel (X, Y) of it takes cell ``(clip((Y d - y) // ch, 0, gh - 1), clip((X d - x) // cw, 0, gw - 1))``
    with (x, y) the tile's corner relative to the origin, and adds ``(1 << 40) | q`` of that cell unless the cell is NaN."""
    (gh, gw), patch, d, (h, w), origin = check_cell_args(grid, patch, downsample, shape, origin)
    coords, values = np.asarray(coords), np.asarray(values)
    check_cells(coords, values, (gh, gw))
    if into is None:
        into = np.zeros((h, w), np.int64)
    elif into.dtype != np.int64 or into.shape != (h, w):
        raise ValueError(f"into must be int64 {(h, w)}, got {into.dtype} {into.shape}")
    acc = into.view(np.uint64)
    q, skip = quantize_numpy(values)
    add = np.where(skip, 0, (1 << COUNT_SHIFT) | q).astype(np.uint64).reshape(-1, gh, gw)
    fp = footprints_numpy(coords, patch, d, (h, w), origin)
    c = coords.astype(np.int64).reshape(-1, 2)
    cw, ch = patch // gw, patch // gh
    for n in np.nonzero((fp[:, 1] > fp[:, 0]) & (fp[:, 3] > fp[:, 2]))[0]:
        c0, c1, r0, r1 = fp[n]
        cx = np.clip((np.arange(c0, c1) * d - (c[n, 0] - origin[0])) // cw, 0, gw - 1)
        cy = np.clip((np.arange(r0, r1) * d - (c[n, 1] - origin[1])) // ch, 0, gh - 1)
        acc[r0:r1, c0:c1] += add[n][cy[:, None], cx[None, :]]
    return into


def unpack_numpy(acc: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """-> (sum int64 [h,w], count int32 [h,w])."""
    a = np.asarray(acc).view(np.uint64)
    return (a & np.uint64(SUM_MASK)).astype(np.int64), (a >> np.uint64(COUNT_SHIFT)).astype(np.int32)


def mean_numpy(acc: np.ndarray, uncovered: float = 0.0) -> Tuple[np.ndarray, np.ndarray]:
    """-> (mean fp32 [h,w], count int32 [h,w]); the division is done in float64 and rounded to float32 once."""
    s, c = unpack_numpy(acc)
    out = np.full(s.shape, np.float32(uncovered), np.float32)
    on = c > 0
    out[on] = (s[on].astype(np.float64) / (Q_ONE * c[on].astype(np.int64)).astype(np.float64)).astype(np.float32)
    return out, c


def pred_numpy(acc: np.ndarray) -> np.ndarray:
    """uint8 {0,255} [h,w]: 255 where sum > 0."""
    return np.where(unpack_numpy(acc)[0] > 0, 255, 0).astype(np.uint8)


def render_numpy(acc: np.ndarray, thumbnail: Optional[np.ndarray] = None, alpha: float = 0.4, colormap="jet", mask: Optional[np.ndarray] = None,
                 window=(0.0, 1.0), min_value: float = 0.0, background=(255, 255, 255)) -> np.ndarray:
    """The render step restated on the host -> uint8 [h,w,3].  ``thumbnail``: uint8 [h,w,3|4] (any strides; alpha ignored);
    ``mask``: [h,w], non-zero = show."""
    a, lo16, hi16, min16, bg = render_args(alpha, window, min_value, background)
    lut = _table(colormap).astype(np.int64)
    S, c = unpack_numpy(acc)
    c = c.astype(np.int64)
    h, w = S.shape
    if thumbnail is None:
        under = np.empty((h, w, 3), np.int64)
        under[:] = bg
    else:
        if thumbnail.dtype != np.uint8 or thumbnail.ndim != 3 or thumbnail.shape[:2] != (h, w) or thumbnail.shape[2] not in (3, 4):
            raise ValueError(f"thumbnail must be uint8 {(h, w)} x 3|4, got {thumbnail.dtype} {thumbnail.shape}")
        under = thumbnail[..., :3].astype(np.int64)
    shown = (c > 0) & (S >= min16 * c)
    if mask is not None:
        if mask.shape != (h, w):
            raise ValueError(f"mask must be {(h, w)}, got {mask.shape}")
        shown &= np.asarray(mask) != 0
    span, cs = hi16 - lo16, np.maximum(c, 1)
    idx = np.clip((2 * 255 * (S - lo16 * c) + span * c) // (2 * span * cs), 0, 255)
    blend = (a * lut[idx] + (256 - a) * under + 128) >> 8
    return np.where(shown[..., None], blend, under).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ percentiles
CANONICAL_NAN = 0x7FC00000
MAX_VALUES = MAX_TILES                         # a population or a set of queries: at most the raster's tile cap
MAX_RADIUS = 127
TAP_SUM = 32768


def check_values(values, name: str = "values", least: int = 1) -> int:
    """A population or a set of queries: [N] of a floating type, ``least <= N <= 2^24 - 1`` -> N."""
    vs, vd = tuple(values.shape), values.dtype
    if not (vd.is_floating_point if isinstance(vd, torch.dtype) else vd.kind == "f"):
        raise ValueError(f"{name} must be floating point, got {vd}")
    if len(vs) != 1 or not least <= vs[0] <= MAX_VALUES:
        raise ValueError(f"{name} must be [N] with {least} <= N <= 2^24 - 1, got {vs}")
    return int(vs[0])


def _float32(values, name: str = "values", least: int = 1) -> np.ndarray:
    v = values.detach().cpu().numpy() if isinstance(values, torch.Tensor) else np.asarray(values)
    check_values(v, name, least)
    return v.astype(np.float32)


def sort_numpy(values) -> Tuple[np.ndarray, int]:
    """keep_sort_f32 restated -> (sorted fp32 [M], n): the n values that are not NaN in ascending order with -0 stored as +0, then
    M - n NaNs with the bits 0x7FC00000."""
    v = _float32(values)
    kept = v[~np.isnan(v)]
    kept = np.sort(np.where(kept == 0, np.float32(0), kept))
    out = np.full(v.shape, CANONICAL_NAN, np.uint32).view(np.float32)
    out[:kept.size] = kept
    return out, int(kept.size)


def rank_numpy(sorted_values: np.ndarray, n: int, queries, self_rank: bool) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """keep_rank_f32 restated -> (pct fp32 [N], less int32 [N], eq int32 [N]).  ``sorted_values`` / ``n``: what :func:`sort_numpy`
    returns.  ``less`` / ``eq``: how many of the n values are smaller than / equal to the query; ``r2 = 2 less + eq + self_rank`` and
    ``pct = float32(float64(r2) / float64(2 n))``; a NaN query gives NaN, -1, -1 and n = 0 gives NaN for every query."""
    q = _float32(queries, "queries", 0)
    pop = np.asarray(sorted_values, np.float32)[:n]
    nan = np.isnan(q)
    qc = np.where(nan | (q == 0), np.float32(0), q)
    less = np.searchsorted(pop, qc, "left").astype(np.int64)
    eq = np.searchsorted(pop, qc, "right").astype(np.int64) - less
    pct = np.full(q.shape, CANONICAL_NAN, np.uint32).view(np.float32)
    if n > 0:
        pct[~nan] = ((2 * less + eq + int(bool(self_rank)))[~nan].astype(np.float64) / np.float64(2 * n)).astype(np.float32)
    return pct, np.where(nan, -1, less).astype(np.int32), np.where(nan, -1, eq).astype(np.int32)


def percentiles_numpy(values, reference=None) -> np.ndarray:
    """``KEEPModel.percentiles`` restated -> fp32 [N]: the values ranked among themselves (twice the average rank over 2 n, the
    rule of ``scipy.stats.rankdata(v, 'average') / n``), or against the population ``reference``
    (``scipy.stats.percentileofscore(reference, v, kind='mean') / 100``)."""
    s, n = sort_numpy(values if reference is None else reference)
    return rank_numpy(s, n, values, reference is None)[0]


class ScoreReference:
    """A sorted score population on the device: ``sorted`` fp32 [M] (the n values that are not NaN in ascending order, then NaNs),
    ``n`` int64 [1] on the device, and ``M``.  ``KEEPModel.score_reference`` makes one; it is what a slide's scores are ranked
    against when an ROI is shown beside the population it came from."""

    def __init__(self, sorted_values: torch.Tensor, n: torch.Tensor, model=None):
        if not isinstance(sorted_values, torch.Tensor) or sorted_values.dtype != torch.float32 or sorted_values.dim() != 1 or not sorted_values.is_contiguous():
            raise ValueError("sorted must be a contiguous fp32 [M] tensor")
        if not isinstance(n, torch.Tensor) or n.dtype != torch.int64 or n.numel() != 1 or n.device != sorted_values.device:
            raise ValueError("n must be one int64 on sorted's device")
        self.sorted, self.n, self.M = sorted_values, n, check_values(sorted_values, "sorted")
        self._model = model

    def __repr__(self):
        return f"ScoreReference(M={self.M} on {self.sorted.device})"

    def _engine(self):
        from .model import engine_for
        if self.sorted.device.type != "cuda":
            raise ValueError("this population lives on the host: use the numpy restatements (rank_numpy, percentiles_numpy)")
        return engine_for(device=self.sorted.device, model=self._model)

    def rank(self, values) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (less int32 [N], eq int32 [N]): how many of the population are smaller than / equal to each value; -1 for a NaN."""
        return self._engine()._rank(self, values, False, False, True)[1:]

    def percentiles(self, values) -> torch.Tensor:
        """-> fp32 [N]: ``(2 less + eq) / (2 n)``, the values as outsiders to the population."""
        return self._engine()._rank(self, values, False, True, False)[0]


# ------------------------------------------------------------------------------------------------ smoothing
def gaussian_taps(sigma, radius=None) -> np.ndarray:
    """Integer Gaussian taps, int32 [2 r + 1]: ``w_k = exp(-k^2 / (2 sigma^2))`` in float64, ``t_k = floor(32768 w_k / sum w)``;
    r defaults to ``ceil(3 sigma)``.  The floor keeps the table symmetric, non-increasing from the centre and its sum <= 32768."""
    sigma = float(sigma)
    if not (sigma > 0.0 and np.isfinite(sigma)):
        raise ValueError(f"sigma must be a positive number, got {sigma!r}")
    r = int(np.ceil(3.0 * sigma)) if radius is None else _integer(radius, "radius")
    if r < 1 or r > MAX_RADIUS:
        raise ValueError(f"radius must lie in [1, {MAX_RADIUS}], got {r}")
    k = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return check_taps(np.floor(TAP_SUM * w / w.sum()).astype(np.int32))


def clam_blur(patch, downsample, factor=2) -> Tuple[float, int]:
    """The size of CLAM's overlay blur -> (sigma, radius): ``ksize = (factor patch // downsample) | 1`` and the sigma an image
    library derives from a kernel size, ``0.3 ((ksize - 1) / 2 - 1) + 0.8``.  A convenience: feed it to :func:`gaussian_taps`;
    no parity with such a library's blur is claimed."""
    patch, d, factor = _integer(patch, "patch"), _integer(downsample, "downsample"), _integer(factor, "factor")
    if patch < 1 or d < 1 or factor < 1:
        raise ValueError(f"patch, downsample and factor must be >= 1, got {patch}, {d}, {factor}")
    ksize = (factor * patch // d) | 1
    r = (ksize - 1) // 2
    if r < 1 or r > MAX_RADIUS:
        raise ValueError(f"kernel size {ksize} gives radius {r} outside [1, {MAX_RADIUS}]")
    return 0.3 * ((ksize - 1) / 2 - 1) + 0.8, r


def check_taps(taps) -> np.ndarray:
    """A table of taps -> int32 [2 r + 1], 1 <= r <= 127: every tap >= 0, the centre tap >= 1, the sum <= 32768."""
    t = taps.detach().cpu().numpy() if isinstance(taps, torch.Tensor) else np.asarray(taps)
    if t.dtype.kind not in "iu" or t.ndim != 1 or t.size % 2 == 0:
        raise ValueError(f"taps must be an odd number of integers, got {t.dtype} {t.shape}")
    r = t.size // 2
    if r < 1 or r > MAX_RADIUS:
        raise ValueError(f"radius must lie in [1, {MAX_RADIUS}], got {r}")
    t = t.astype(np.int64)
    if t.min() < 0 or t[r] < 1 or t.sum() > TAP_SUM:
        raise ValueError(f"taps must be >= 0 with a centre tap >= 1 and a sum <= {TAP_SUM}: min {t.min()}, centre {t[r]}, sum {t.sum()}")
    return t.astype(np.int32)


def smooth_taps(sigma=None, radius=None, taps=None) -> np.ndarray:
    """The taps of a smoothing call: ``taps`` as given (checked; ``radius`` must agree with it), or :func:`gaussian_taps`."""
    if taps is None:
        if sigma is None:
            raise ValueError("give sigma (with radius, optionally) or taps")
        return gaussian_taps(sigma, radius)
    if sigma is not None:
        raise ValueError("give sigma or taps, not both")
    t = check_taps(taps)
    if radius is not None and _integer(radius, "radius") != t.size // 2:
        raise ValueError(f"radius {radius} does not match {t.size} taps")
    return t


def smooth_numpy(acc: np.ndarray, taps, mask: Optional[np.ndarray] = None) -> np.ndarray:
    """keep_heat_smooth restated on the host -> the smoothed accumulator, int64 [h,w] (count 1 on the support, 0 elsewhere)."""
    t = check_taps(taps).astype(np.int64)
    r = t.size // 2
    acc = np.asarray(acc)
    if acc.dtype != np.int64 or acc.ndim != 2:
        raise ValueError(f"acc must be int64 [h,w], got {acc.dtype} {acc.shape}")
    S, c = unpack_numpy(acc)
    c = c.astype(np.int64)
    h, w = S.shape
    s = c > 0
    if mask is not None:
        if np.asarray(mask).shape != (h, w):
            raise ValueError(f"mask must be {(h, w)}, got {np.asarray(mask).shape}")
        s &= np.asarray(mask) != 0
    m = np.where(s, (2 * S + c) // (2 * np.maximum(c, 1)), 0)

    def conv(plane, axis):
        pad = [(0, 0), (0, 0)]
        pad[axis] = (r, r)
        p = np.pad(plane, pad)
        out = np.zeros_like(plane)
        for k in range(2 * r + 1):
            if t[k]:
                out += t[k] * (p[:, k:k + w] if axis == 1 else p[k:k + h])
        return out

    Nn, D = conv(conv(m, 1), 0), conv(conv(s.astype(np.int64), 1), 0)
    return np.where(s, (1 << COUNT_SHIFT) | ((2 * Nn + D) // (2 * np.maximum(D, 1))), 0).astype(np.int64)
