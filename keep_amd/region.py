"""Slide regions -> patch grid, tissue rule, coords: the host side of ``KEEPModel.region_grid`` /
``region_patches_uint8`` / ``encode_region`` and of ``cohort.extract_slide_features``.

  * argument checks that run before any device call (``check_grid_args``, ``tissue_params``);
  * the Resize(224, BICUBIC) tables of a patch size, built once per (size, device) (``resize_tables``);
  * the band planner that walks a slide in horizontal bands of whole grid rows (``plan_bands``);
  * a numpy restatement of the grid and the tissue rule, the yardstick of the device kernels (``region_grid_numpy``);
  * the thumbnail segmentation of DESIGN.md section 11: its parameters (``TissueSegmentation``), a mask and how to read it
    (``TissueMask``), Otsu's threshold in exact integers (``otsu_threshold``), the numpy restatements of the segmentation and
    of the grid on a mask (``tissue_mask_numpy``, ``mask_grid_numpy``) and what a masked extraction reads (``plan_mask_reads``).

``TissueRule`` is a per-pixel integer test, NOT CLAM's contour segmentation (median blur + Otsu on saturation + contour
filtering, README.md:74 of the reference): a pixel is tissue iff ``max(r,g,b) > 0`` and ``255 (max - min) >= sat_min max``
(HSV saturation >= sat_min / 255, exact in integers); a cell is kept iff it holds at least ``ceil(min_fraction p^2)`` of them.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch

TILE = 224


@dataclass(frozen=True)
class TissueRule:
    """Keep a grid cell iff at least ``min_fraction`` of its pixels have HSV saturation >= ``sat_min`` (0..255 scale).
    Glass (near-white, grey, black) has saturation near 0; H & E stain well above 20."""
    sat_min: int = 20
    min_fraction: float = 0.25


TissueArg = Union[None, bool, TissueRule, Tuple[int, float], Dict[str, float]]


def tissue_params(tissue: TissueArg, patch: int) -> Tuple[int, int]:
    """-> (sat_min, min_pixels) for the kernel; the rule off is (0, 0): every cell is kept, no pixel is read."""
    if tissue is None or tissue is False:
        return 0, 0
    if tissue is True:
        rule = TissueRule()
    elif isinstance(tissue, TissueRule):
        rule = tissue
    elif isinstance(tissue, dict):
        rule = TissueRule(**tissue)
    elif isinstance(tissue, (tuple, list)) and len(tissue) == 2:
        rule = TissueRule(*tissue)
    else:
        raise ValueError(f"tissue: None, True, a TissueRule, (sat_min, min_fraction) or a dict, got {tissue!r}")
    if int(rule.sat_min) != rule.sat_min or not 0 <= rule.sat_min <= 255:
        raise ValueError(f"tissue sat_min must be an integer in [0, 255], got {rule.sat_min!r}")
    if not 0.0 <= float(rule.min_fraction) <= 1.0:
        raise ValueError(f"tissue min_fraction must lie in [0, 1], got {rule.min_fraction!r}")
    return int(rule.sat_min), int(math.ceil(float(rule.min_fraction) * patch * patch))


MASK_MODES = ("four_pt", "four_pt_hard", "center")           # index = KEEP_MASK_* of keep_hip.h
TISSUE_MAX_PIXELS = 1 << 30


@dataclass(frozen=True)
class TissueSegmentation:
    """Parameters of the thumbnail segmentation, named after CLAM's ``segmentTissue``:

    ``mthresh``   side k of the k x k median of the saturation, odd in 3..15, 1 = off;
    ``sthresh``   foreground iff median > sthresh (0..255), unless ``use_otsu`` picks the threshold from the histogram;
    ``close``     side of the closing box, 0 = off, <= 31;
    ``min_area``  CLAM's ``a_t``: 8-connected components of <= min_area pixels are dropped;
    ``min_hole``  CLAM's ``a_h``: holes (4-connected background that touches no border) of <= min_hole pixels are filled;
    ``mode``      how a grid cell is tested against the mask: ``"four_pt"`` (any of the four points ``centre +- patch // 4``),
                  ``"four_pt_hard"`` (all four) or ``"center"``.

    Areas are THUMBNAIL pixels.  CLAM scales its presets by the reference patch seen at the segmentation level, so its
    ``a_t`` / ``a_h`` map to ``a * (ref_patch_size // downsample) ** 2`` here (:meth:`from_clam`); the defaults are the raw numbers
    of CLAM's ``create_patches`` presets, remembered as defaults, not as a parity claim."""
    mthresh: int = 7
    sthresh: int = 8
    use_otsu: bool = False
    close: int = 4
    min_area: int = 100
    min_hole: int = 16
    mode: str = "four_pt"

    def __post_init__(self):
        def integer(name, lo, hi=None):
            v = getattr(self, name)
            if isinstance(v, bool) or int(v) != v or v < lo or (hi is not None and v > hi):
                raise ValueError(f"{name} must be an integer in [{lo}, {'inf' if hi is None else hi}], got {v!r}")
        integer("mthresh", 1, 15)
        if self.mthresh % 2 == 0:
            raise ValueError(f"mthresh (the median's side) must be odd, got {self.mthresh}")
        integer("sthresh", 0, 255)
        integer("close", 0, 31)
        integer("min_area", 0)
        integer("min_hole", 0)
        if self.mode not in MASK_MODES:
            raise ValueError(f"mode must be one of {MASK_MODES}, got {self.mode!r}")

    @classmethod
    def from_clam(cls, downsample: int, a_t: int = 100, a_h: int = 16, ref_patch_size: int = 512, **kw) -> "TissueSegmentation":
        """CLAM's area presets at a thumbnail ``downsample`` times smaller than level 0: ``a * (ref_patch_size // downsample)^2``."""
        scale = (int(ref_patch_size) // check_downsample(downsample)) ** 2
        return cls(min_area=int(a_t) * scale, min_hole=int(a_h) * scale, **kw)


def check_downsample(downsample) -> int:
    if isinstance(downsample, bool) or int(downsample) != downsample or downsample < 1:
        raise ValueError(f"downsample must be an integer >= 1, got {downsample!r}")
    return int(downsample)


class TissueMask:
    """A tissue mask and how to read it: ``mask`` uint8 {0,1} ``[h, w]`` (torch, any device), one pixel of it covering
    ``downsample`` x ``downsample`` pixels of the level being tiled; ``mode`` as in :class:`TissueSegmentation`; ``threshold`` the
    saturation threshold that made it (``None`` for a caller's own mask).  ``KEEPModel.tissue_mask`` returns one; a caller's own
    ``[h, w]`` bool / uint8 array (an annotation, a mask CLAM made) is wrapped the same way: non-zero = tissue."""

    def __init__(self, mask, downsample: int, mode: str = "four_pt", threshold: Optional[int] = None):
        m = torch.from_numpy(np.ascontiguousarray(mask)) if isinstance(mask, np.ndarray) else mask
        if not isinstance(m, torch.Tensor) or m.dim() != 2 or m.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"mask must be a [h, w] bool or uint8 array, got {getattr(m, 'dtype', type(m))} "
                             f"{tuple(getattr(m, 'shape', ()))}")
        if m.shape[0] < 1 or m.shape[1] < 1:
            raise ValueError(f"mask is empty: {tuple(m.shape)}")
        if mode not in MASK_MODES:
            raise ValueError(f"mode must be one of {MASK_MODES}, got {mode!r}")
        self.mask = (m != 0).to(torch.uint8).contiguous()
        self.downsample = check_downsample(downsample)
        self.mode = mode
        self.threshold = None if threshold is None else int(threshold)

    def __repr__(self):
        return (f"TissueMask({tuple(self.mask.shape)} on {self.mask.device}, downsample={self.downsample}, mode={self.mode!r}, "
                f"threshold={self.threshold})")


def thumbnail_layout(thumbnail: torch.Tensor) -> Tuple[int, int, int, int]:
    """:func:`region_layout` plus the segmentation's size limit (int32 pixel indices)."""
    h, w, C, row = region_layout(thumbnail)
    if h * w > TISSUE_MAX_PIXELS:
        raise ValueError(f"thumbnail of {h}x{w} pixels: the segmentation takes h * w <= 2^30")
    return h, w, C, row


def otsu_threshold(hist) -> int:
    """Otsu's threshold of a 256-bin histogram in Python integers: the smallest t that maximises the between-class variance
    ``(m0 N - w0 M)^2 / (w0 w1)`` (w0, m0: count and sum of the values <= t; N, M: the totals), fractions compared by
    cross-multiplication; a t that leaves one class empty is skipped, so an image of one level gives 0."""
    hist = [int(v) for v in hist]
    if len(hist) != 256 or any(v < 0 for v in hist):
        raise ValueError("otsu_threshold takes 256 non-negative counts")
    N, M = sum(hist), sum(i * v for i, v in enumerate(hist))
    best_num, best_den, best_t, w0, m0 = 0, 1, 0, 0, 0
    for t in range(256):
        w0 += hist[t]
        m0 += t * hist[t]
        w1 = N - w0
        if w0 == 0 or w1 == 0:
            continue
        num, den = (m0 * N - w0 * M) ** 2, w0 * w1
        if num * best_den > best_num * den:
            best_num, best_den, best_t = num, den, t
    return best_t


def saturation_numpy(rgb: np.ndarray) -> np.ndarray:
    """uint8 [h,w,3|4] -> HSV saturation on the 0..255 scale, rounded half up: ``(2 * 255 (max - min) + max) // (2 max)``, 0 at max = 0."""
    c = rgb[..., :3].astype(np.int64)
    mx, mn = c.max(axis=2), c.min(axis=2)
    return np.where(mx > 0, (510 * (mx - mn) + mx) // (2 * np.maximum(mx, 1)), 0).astype(np.uint8)


def median_numpy(img: np.ndarray, k: int) -> np.ndarray:
    """k x k median of a uint8 image, border replicated (``cv2.medianBlur`` / ``median_filter(mode="nearest")``), numpy only:
    the k^2 shifted views of a block of rows are stacked and partitioned."""
    if k == 1:
        return img.copy()
    r, (h, w) = k // 2, img.shape
    pad = np.pad(img, r, mode="edge")
    out = np.empty_like(img)
    rows = max(1, (1 << 25) // (k * k * w))
    for y0 in range(0, h, rows):
        y1 = min(h, y0 + rows)
        stack = np.stack([pad[y0 + dy:y1 + dy, dx:dx + w] for dy in range(k) for dx in range(k)])
        out[y0:y1] = np.partition(stack, (k * k) // 2, axis=0)[(k * k) // 2]
    return out


def close_numpy(b: np.ndarray, c: int) -> np.ndarray:
    """Closing of a {0,1} image by a c x c box, anchor c // 2: window [x - a, x + c - 1 - a] on both axes, outside = 0 for the
    dilation and 1 for the erosion (OpenCV's constant borders)."""
    if c <= 0:
        return b.copy()
    a, (h, w) = c // 2, b.shape

    def box(src, fill, op):
        p = np.full((h + c, w + c), fill, src.dtype)
        p[a:a + h, a:a + w] = src
        rows = p[:, 0:w].copy()
        for d in range(1, c):
            rows = op(rows, p[:, d:d + w])
        out = rows[0:h].copy()
        for d in range(1, c):
            out = op(out, rows[d:d + h])
        return out
    return box(box(b, 0, np.maximum), 1, np.minimum)


def label_numpy(b: np.ndarray, conn8: bool) -> Tuple[np.ndarray, np.ndarray]:
    """Connected components of the non-zero pixels of ``b`` -> (labels int64 [h,w], 0 = background, components 1..n; pixel counts
    int64 [n + 1]).  numpy + a plain union-find over the horizontal runs (no scipy): two runs of neighbouring rows are joined iff
    their columns overlap (4-connectivity) or come within one column of each other (8-connectivity)."""
    b = np.asarray(b) != 0
    h, w = b.shape
    pad = np.zeros((h, w + 2), np.int8)
    pad[:, 1:-1] = b
    d = np.diff(pad, axis=1)
    ys, xs = np.nonzero(d == 1)                                # run starts, row-major
    xe = np.nonzero(d == -1)[1]                                # run ends (exclusive), same order
    first = np.searchsorted(ys, np.arange(h + 1))             # runs of row y: [first[y], first[y + 1])
    parent = list(range(len(xs)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    reach = 1 if conn8 else 0
    S, E = xs.tolist(), xe.tolist()
    for y in range(1, h):
        i, i1, j, j1 = int(first[y - 1]), int(first[y]), int(first[y]), int(first[y + 1])
        while i < i1 and j < j1:
            if S[j] < E[i] + reach and E[j] + reach > S[i]:
                ri, rj = find(i), find(j)
                if ri != rj:
                    parent[max(ri, rj)] = min(ri, rj)
            if E[i] < E[j]:
                i += 1
            else:
                j += 1
    roots = np.array([find(i) for i in range(len(parent))], np.int64)
    _, comp = np.unique(roots, return_inverse=True)
    lab = np.zeros((h, w), np.int64)
    lab[b] = np.repeat(comp.reshape(-1) + 1, xe - xs)         # np.nonzero order = run order
    return lab, np.bincount(lab.ravel(), minlength=1)


def tissue_mask_numpy(thumbnail: np.ndarray, params: TissueSegmentation = TissueSegmentation(), stages: Optional[dict] = None):
    """The segmentation restated on the host, numpy only: the yardstick of the device kernels -> (mask uint8 {0,1} [h,w],
    threshold).  ``stages``: a dict that receives every intermediate (``saturation``, ``median``, ``hist``, ``thresholded``,
    ``closed``, ``holes_filled`` / ``holes_kept`` (counts), ``filled``, ``components`` / ``components_kept`` (counts))."""
    thumbnail = np.asarray(thumbnail)
    if thumbnail.dtype != np.uint8 or thumbnail.ndim != 3 or thumbnail.shape[2] not in (3, 4):
        raise ValueError(f"thumbnail must be uint8 [h,w,3|4], got {thumbnail.dtype} {thumbnail.shape}")
    sat = saturation_numpy(thumbnail)
    med = median_numpy(sat, params.mthresh)
    hist = np.bincount(med.ravel(), minlength=256)
    t = otsu_threshold(hist) if params.use_otsu else int(params.sthresh)
    thresholded = (med > t).astype(np.uint8)
    closed = close_numpy(thresholded, params.close)
    # step 5: background components (4-connected) that touch no border and hold <= min_hole pixels
    lab, area = label_numpy(closed == 0, conn8=False)
    border = np.zeros(len(area), bool)
    for edge in (lab[0], lab[-1], lab[:, 0], lab[:, -1]):
        border[edge] = True
    border[0] = True                                           # label 0 = foreground: never "filled"
    fill = ~border & (area <= params.min_hole)
    filled = closed | fill[lab].astype(np.uint8)
    # step 6: foreground components (8-connected) of > min_area pixels
    lab2, area2 = label_numpy(filled, conn8=True)
    keep = area2 > params.min_area
    keep[0] = False
    mask = keep[lab2].astype(np.uint8)
    if stages is not None:
        stages.update(saturation=sat, median=med, hist=hist, thresholded=thresholded, closed=closed, filled=filled,
                      holes_filled=int(fill.sum()), holes_kept=int((~border & ~fill).sum()), components=len(area2) - 1,
                      components_kept=int(keep.sum()))
    return mask, t


def mask_grid_numpy(mask: np.ndarray, downsample: int, H: int, W: int, patch: int, step: Optional[int] = None, origin=(0, 0),
                    mode: str = "four_pt") -> np.ndarray:
    """The grid on a mask restated on the host -> kept cells' (x, y) offsets in the H x W region, int64 [N,2], row-major.  A cell at
    (x, y) is tested at ``c = origin + (x, y) + patch // 2`` (``center``) or at the four points ``c +- patch // 4``
    (``four_pt``: any, ``four_pt_hard``: all); a point is tissue iff ``mask[py // downsample, px // downsample]`` is set, outside
    the mask it is not."""
    step = patch if step is None else step
    mask = np.asarray(mask) != 0
    gy, gx = grid_shape(H, W, patch, step)
    cx = int(origin[0]) + np.arange(gx, dtype=np.int64) * step + patch // 2
    cy = int(origin[1]) + np.arange(gy, dtype=np.int64) * step + patch // 2

    def tissue(px, py):                                        # px [gx], py [gy] -> [gy, gx]
        mx, my = px // downsample, py // downsample
        okx, oky = (px >= 0) & (mx < mask.shape[1]), (py >= 0) & (my < mask.shape[0])
        v = mask[np.clip(my, 0, mask.shape[0] - 1)[:, None], np.clip(mx, 0, mask.shape[1] - 1)[None, :]]
        return v & oky[:, None] & okx[None, :]
    s = patch // 4
    if mode == "center":
        keep = tissue(cx, cy)
    elif mode in ("four_pt", "four_pt_hard"):
        pts = [tissue(cx + sx, cy + sy) for sy in (-s, s) for sx in (-s, s)]
        keep = np.logical_and.reduce(pts) if mode == "four_pt_hard" else np.logical_or.reduce(pts)
    else:
        raise ValueError(f"mode must be one of {MASK_MODES}, got {mode!r}")
    yy, xx = np.nonzero(keep.reshape(gy, gx))
    return np.stack([xx * step, yy * step], axis=1).astype(np.int64).reshape(-1, 2)


def plan_mask_reads(cells, bands: List[Tuple[int, int, int, int]], patch: int, step: int) -> List[Tuple[int, int, int, int]]:
    """What ``extract_slide_features`` reads when a mask decides the grid: ``cells`` are the kept cells' (x, y) offsets in the
    slide level (int [N,2]), ``bands`` those of :func:`plan_bands`.  -> one ``(x0, y0, w, h)`` per band that holds a kept cell, in
    band order: the band's rows and only the columns ``[min kept x, max kept x + patch)``.  A band with no kept cell is absent."""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 2)
    reads = []
    for r0, r1, y0, h in bands:
        x = cells[(cells[:, 1] >= r0 * step) & (cells[:, 1] < r1 * step), 0]
        if x.size:
            reads.append((int(x.min()), y0, int(x.max()) + patch - int(x.min()), h))
    return reads


def check_grid_args(patch: int, step: Optional[int], origin=(0, 0), coord_scale: int = 1) -> Tuple[int, int, Tuple[int, int], int]:
    """Validate the grid arguments on the host -> (patch, step, origin, coord_scale); ``step=None`` means ``step = patch``."""
    if isinstance(patch, bool) or int(patch) != patch or patch < 16:
        raise ValueError(f"patch_size must be an integer >= 16, got {patch!r}")
    patch = int(patch)
    step = patch if step is None else step
    if isinstance(step, bool) or int(step) != step or step < 1:
        raise ValueError(f"step must be an integer >= 1, got {step!r}")
    if isinstance(coord_scale, bool) or int(coord_scale) != coord_scale or coord_scale < 1:
        raise ValueError(f"coord_scale must be an integer >= 1, got {coord_scale!r}")
    if len(origin) != 2 or any(int(o) != o for o in origin):
        raise ValueError(f"origin must be two integers (x, y), got {origin!r}")
    return patch, int(step), (int(origin[0]), int(origin[1])), int(coord_scale)


def region_layout(region: torch.Tensor) -> Tuple[int, int, int, int]:
    """uint8 [H,W,C], C in (3, 4), channels contiguous and pixels C bytes apart -> (H, W, C, row_stride_bytes)."""
    if region.dtype != torch.uint8 or region.dim() != 3 or region.shape[2] not in (3, 4):
        raise ValueError(f"region must be uint8 [H,W,3] (RGB) or [H,W,4] (RGBA), got {region.dtype} {tuple(region.shape)}")
    H, W, C = (int(v) for v in region.shape)
    if H < 1 or W < 1:
        raise ValueError(f"region is empty: {tuple(region.shape)}")
    s0, s1, s2 = region.stride()
    if (C > 1 and s2 != 1) or (W > 1 and s1 != C):
        raise ValueError(f"region pixels must be {C} contiguous bytes (strides (*, {C}, 1)), got strides {region.stride()}")
    row = s0 if H > 1 else W * C
    if row < W * C:
        raise ValueError(f"region row stride {row} < W * C = {W * C}")
    return H, W, C, row


def grid_shape(H: int, W: int, patch: int, step: int) -> Tuple[int, int]:
    """(rows, columns) of the grid: every cell wholly inside the region."""
    return ((H - patch) // step + 1 if H >= patch else 0), ((W - patch) // step + 1 if W >= patch else 0)


def region_grid_numpy(region: np.ndarray, patch: int, step: Optional[int] = None, sat_min: int = 0, min_pixels: int = 0) -> np.ndarray:
    """The grid + tissue rule restated on the host: uint8 [H,W,3|4] -> kept cells' (x, y) pixel offsets, int64 [N,2], row-major."""
    step = patch if step is None else step
    H, W = region.shape[:2]
    gy, gx = grid_shape(H, W, patch, step)
    if min_pixels > 0 and gy and gx:
        rgb = region[..., :3].astype(np.int64)
        mx, mn = rgb.max(axis=2), rgb.min(axis=2)
        tissue = ((mx > 0) & (255 * (mx - mn) >= sat_min * mx)).astype(np.int64)
        ii = np.zeros((H + 1, W + 1), np.int64)                # summed-area table: exact window counts
        ii[1:, 1:] = tissue.cumsum(0).cumsum(1)
        ys, xs = np.arange(gy) * step, np.arange(gx) * step
        cnt = ii[ys[:, None] + patch, xs[None, :] + patch] - ii[ys[:, None], xs[None, :] + patch] - ii[ys[:, None] + patch, xs[None, :]] \
            + ii[ys[:, None], xs[None, :]]
        keep = cnt >= min_pixels
    else:
        keep = np.ones((gy, gx), bool)
    yy, xx = np.nonzero(keep)                                  # row-major: y outer, x inner
    return np.stack([xx * step, yy * step], axis=1).astype(np.int64).reshape(-1, 2)


def plan_bands(width: int, height: int, patch: int, step: Optional[int] = None, band_rows: int = 8) -> List[Tuple[int, int, int, int]]:
    """Horizontal bands of ``band_rows`` grid rows -> [(r0, r1, y0, h)]: band k holds grid rows [r0, r1) and covers pixel rows
    [y0, y0 + h) = [r0 step, (r1 - 1) step + patch), so every grid cell of the whole slide falls in exactly one band."""
    patch, step, _, _ = check_grid_args(patch, step)
    if isinstance(band_rows, bool) or int(band_rows) != band_rows or band_rows < 1:
        raise ValueError(f"band_rows must be an integer >= 1, got {band_rows!r}")
    if width < 1 or height < 1:
        raise ValueError(f"slide size must be positive, got {width}x{height}")
    gy, _ = grid_shape(height, width, patch, step)
    return [(r0, min(r0 + band_rows, gy), r0 * step, (min(r0 + band_rows, gy) - 1 - r0) * step + patch) for r0 in range(0, gy, band_rows)]


_TABLES: Dict[Tuple[int, str], tuple] = {}


def resize_tables(patch: int, device: torch.device) -> tuple:
    """Pillow's Resize(224, BICUBIC) tables of a square ``patch`` (the same for both axes; CenterCrop(224) is then the
    identity) on ``device`` -> (bounds, weights, ksize); built in float64 by ``pil_bicubic_coeffs`` once per (patch, device)."""
    from .preprocess import pil_bicubic_coeffs
    key = (int(patch), str(device))
    if key not in _TABLES:
        b, k, ks = pil_bicubic_coeffs(int(patch), TILE)
        _TABLES[key] = (torch.from_numpy(b).to(device).contiguous(), torch.from_numpy(k).to(device).contiguous(), ks)
    return _TABLES[key]
