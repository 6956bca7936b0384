"""The region table: the connected regions of a mask, numbered, with their geometry and their scores.

``KEEPModel.mask_regions`` labels the non-zero pixels of a mask on the device (a tissue mask of ``KEEPModel.tissue_mask``, or a
thresholded ``TileRaster`` through ``keep_amd.wsi.segment_regions``) and returns a :class:`RegionTable`: how many regions there are,
where each one is, how large it is and, with a raster, how sure the model is about it.  It stands where CLAM hands back a list of
tissue contours with areas and boxes, restated on the pixel mask.

Everything the device computes is an integer.  A component is KEPT iff it holds ``>= min_area`` pixels (the tissue filter of
``TissueSegmentation`` is the other way round: a fragment is DROPPED iff it holds ``<= min_area``).  The kept components are numbered
1..n in the row-major order of their first pixels: ``scipy.ndimage.label``'s numbering with the dropped ones removed.  The device
kernels (``csrc/components.hip``) equal :func:`regions_numpy` exactly.

This module holds the host side: argument checks (ValueError before any device call), :class:`RegionTable` (whose float64
conversions are not part of the integer contract) and the restatement :func:`regions_numpy`."""
from typing import Optional, Tuple

import numpy as np
import torch

from .heatmap import COUNT_SHIFT, Q_ONE, SUM_MASK, TileRaster, _integer
from .region import TISSUE_MAX_PIXELS, TissueMask, label_numpy

COLUMNS = ("first_x", "first_y", "area", "x0", "y0", "x1", "y1", "sum_x", "sum_y", "border", "covered", "sum_c", "sum_s", "peak16")
NCOLS = len(COLUMNS)
MAX_REGIONS = 1 << 20


# ------------------------------------------------------------------------------------------------ argument checks
def check_regions_args(connectivity, min_area, max_regions=MAX_REGIONS) -> Tuple[int, int, int]:
    """-> (connectivity, min_area, max_regions) as integers."""
    connectivity, min_area = _integer(connectivity, "connectivity"), _integer(min_area, "min_area")
    max_regions = _integer(max_regions, "max_regions")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity}")
    if min_area < 1:
        raise ValueError(f"min_area must be >= 1 (a component is kept iff it holds >= min_area pixels), got {min_area}")
    if max_regions < 0:
        raise ValueError(f"max_regions must be >= 0, got {max_regions}")
    return connectivity, min_area, max_regions


def mask_tensor(mask) -> Tuple[torch.Tensor, Optional[int]]:
    """A mask argument -> (bool / uint8 [h,w] tensor on its own device, the downsample a ``TissueMask`` brings or None)."""
    if isinstance(mask, TissueMask):
        m, d = mask.mask, mask.downsample
    else:
        m, d = (torch.from_numpy(np.ascontiguousarray(mask)) if isinstance(mask, np.ndarray) else mask), None
    if not isinstance(m, torch.Tensor) or m.dim() != 2 or m.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"mask must be a [h, w] bool or uint8 array or a TissueMask, got {getattr(m, 'dtype', type(m))} "
                         f"{tuple(getattr(m, 'shape', ()))}")
    h, w = int(m.shape[0]), int(m.shape[1])
    if h < 1 or w < 1 or h * w > TISSUE_MAX_PIXELS:
        raise ValueError(f"mask of {h}x{w} pixels: need 1 <= h * w <= 2^30")
    return m, d


def check_raster(raster, shape, downsample: Optional[int]) -> Optional[int]:
    """The raster against the mask it scores -> the table's downsample.  ValueError for a raster of another shape, for two
    downsamples that differ, and for a raster whose region sums could leave int64: every pixel's sum is at most 65535 times its
    count, a tile covers at most ``(patch // downsample + 1)^2`` pixels, so ``sum_s <= 65535 tiles (patch // downsample + 1)^2``."""
    if raster is None:
        return downsample
    if not isinstance(raster, TileRaster):
        raise ValueError(f"raster must be a TileRaster, got {type(raster).__name__}")
    if raster.shape != tuple(shape):
        raise ValueError(f"the raster is {raster.shape}, the mask {tuple(shape)}")
    if downsample is not None and downsample != raster.downsample:
        raise ValueError(f"the mask has downsample {downsample}, the raster {raster.downsample}")
    bound = raster.tiles * (raster.patch // raster.downsample + 1) ** 2 * Q_ONE
    if bound >= 1 << 63:
        raise ValueError(f"a region's sum of scores could leave int64: {raster.tiles} tiles x (patch {raster.patch} // downsample "
                         f"{raster.downsample} + 1)^2 x 65535 = {bound} >= 2^63")
    return raster.downsample


def check_region_count(n: int, max_regions: int) -> int:
    """The cap on the table's rows, checked before the table is allocated (a one-pixel checkerboard at 2^30 pixels would otherwise ask
    for tens of GB)."""
    if n > max_regions:
        raise ValueError(f"the mask has {n} regions, max_regions is {max_regions}: raise min_area or max_regions")
    return n


# ------------------------------------------------------------------------------------------------ the result
class RegionTable:
    """The regions of one mask.  ``table``: int64 ``[n,14]`` (torch, on the device that made it; columns :data:`COLUMNS`), row i - 1
    for label i; ``labels``: int32 ``[h,w]``, 0 = background or dropped (None if not asked for); ``downsample``: level-0 pixels per
    mask pixel (None if neither the mask nor the raster said); ``origin``: the level-0 position of pixel (0, 0); ``ids``: the label of
    every row (1..n until :meth:`sort` permutes a copy).  Every column is an attribute (``.area``, ``.x0`` ...: int64 ``[n]`` views of
    the table); ``connectivity``: the connectivity ``mask_regions`` labelled with (None if unknown), which ``region_outlines`` takes as
    its default; ``label_order``: row i - 1 belongs to label i (False for the copy :meth:`sort` returns, and for any table built with its
    own ``ids``).  The methods below convert on the host in float64 and are not part of the integer contract."""

    def __init__(self, table: torch.Tensor, labels: Optional[torch.Tensor] = None, downsample: Optional[int] = None, origin=(0, 0),
                 ids: Optional[torch.Tensor] = None, connectivity: Optional[int] = None):
        if not isinstance(table, torch.Tensor) or table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != NCOLS:
            raise ValueError(f"table must be an int64 [n,{NCOLS}] tensor")
        self.table, self.labels, self.downsample = table, labels, downsample
        self.origin = (int(origin[0]), int(origin[1]))
        self.connectivity = connectivity
        self.ids = torch.arange(1, table.shape[0] + 1, dtype=torch.int64, device=table.device) if ids is None else ids
        self.label_order = ids is None
        self._host = None

    @property
    def n(self) -> int:
        return int(self.table.shape[0])

    def __len__(self) -> int:
        return self.n

    def __repr__(self):
        return f"RegionTable(n={self.n} on {self.table.device}, downsample={self.downsample}, origin={self.origin})"

    def __getattr__(self, name):
        if name in COLUMNS:
            return self.table[:, COLUMNS.index(name)]
        raise AttributeError(name)

    def numpy(self) -> np.ndarray:
        """The table on the host, int64 [n,14] (read once)."""
        if self._host is None:
            self._host = self.table.cpu().numpy()
        return self._host

    def _col(self, name: str) -> np.ndarray:
        return self.numpy()[:, COLUMNS.index(name)].astype(np.float64)

    def centroid(self) -> np.ndarray:
        """float64 [n,2]: ``(sum_x / area + 0.5, sum_y / area + 0.5)`` in mask pixels (a pixel's centre lies at its index + 0.5)."""
        a = self._col("area")
        return np.stack([self._col("sum_x") / a + 0.5, self._col("sum_y") / a + 0.5], axis=1)

    def to_level0(self) -> dict:
        """Box ``[n,4]`` (x0, y0, x1, y1), centroid ``[n,2]`` and area ``[n]`` in level-0 units: ``origin + downsample * ...`` and
        ``area * downsample^2`` (float64)."""
        if self.downsample is None:
            raise ValueError("this table has no downsample: pass a TissueMask or a raster to mask_regions")
        d, o = float(self.downsample), np.asarray(self.origin, np.float64)
        box = self.numpy()[:, 3:7].astype(np.float64) * d + np.concatenate([o, o])
        return {"box": box, "centroid": self.centroid() * d + o, "area": self._col("area") * d * d}

    def area_mm2(self, mpp: float) -> np.ndarray:
        """float64 [n]: the areas in mm^2 at ``mpp`` microns per level-0 pixel."""
        return self.to_level0()["area"] * float(mpp) ** 2 * 1e-6

    def mean_score(self) -> np.ndarray:
        """float64 [n]: ``sum_s / (65535 sum_c)``, the mean over the region's pixels weighted by their tile counts; NaN where no
        pixel is covered."""
        c = self._col("sum_c")
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(c > 0, self._col("sum_s") / (Q_ONE * c), np.nan)

    def peak_score(self) -> np.ndarray:
        """float64 [n]: ``peak16 / 65535``, the largest pixel mean of the region."""
        return self._col("peak16") / Q_ONE

    def sort(self, by: str = "area", descending: bool = True) -> "RegionTable":
        """A copy with the rows permuted by a column, ``"mean_score"`` or ``"peak_score"`` (stable; ``ids`` follows).  This table and
        the labels stay in label order."""
        if by in COLUMNS:
            key = self.numpy()[:, COLUMNS.index(by)]              # int64 itself: float64 would tie keys above 2^53 (sum_x, sum_y, sum_s)
        elif by in ("mean_score", "peak_score"):
            key = np.nan_to_num(getattr(self, by)(), nan=-1.0)
        else:
            raise ValueError(f"by must be one of {COLUMNS + ('mean_score', 'peak_score')}, got {by!r}")
        order = torch.from_numpy(np.argsort(-key if descending else key, kind="stable")).to(self.table.device)
        return RegionTable(self.table[order], self.labels, self.downsample, self.origin, self.ids[order], self.connectivity)


# ------------------------------------------------------------------------------------------------ the restatement
def regions_numpy(mask, connectivity: int = 8, min_area: int = 1, acc: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The labelling and the table restated on the host -> (labels int32 [h,w], table int64 [n,14]); ``acc``: the int64 [h,w]
    accumulator of a raster (``heatmap.raster_numpy``) or None.  ``region.label_numpy`` numbers the components by first pixel; the cut
    at ``min_area`` renumbers the kept ones in the same order; the columns are sums, minima and maxima over every label's pixels, taken
    in int64 after a stable sort of the foreground by label."""
    connectivity, min_area, _ = check_regions_args(connectivity, min_area)
    b = np.asarray(mask) != 0
    if b.ndim != 2:
        raise ValueError(f"mask must be [h, w], got {b.shape}")
    h, w = b.shape
    lab, area = label_numpy(b, connectivity == 8)
    keep = area >= min_area
    keep[0] = False
    new = np.where(keep, np.cumsum(keep), 0)
    labels = new[lab].astype(np.int32)
    n = int(keep.sum())
    table = np.zeros((n, NCOLS), np.int64)
    if n == 0:
        return labels, table
    flat = labels.ravel()
    p = np.flatnonzero(flat)                                      # row-major: a label's first entry is its first pixel
    p = p[np.argsort(flat[p], kind="stable")]
    start = np.searchsorted(flat[p], np.arange(1, n + 1))
    y, x = p // w, p % w
    add, lo, hi = (lambda v: np.add.reduceat(v.astype(np.int64), start)), (lambda v: np.minimum.reduceat(v, start)), \
        (lambda v: np.maximum.reduceat(v, start))
    table[:, 0], table[:, 1] = x[start], y[start]
    table[:, 2] = add(np.ones_like(p))
    table[:, 3], table[:, 4], table[:, 5], table[:, 6] = lo(x), lo(y), hi(x) + 1, hi(y) + 1
    table[:, 7], table[:, 8] = add(x), add(y)
    table[:, 9] = hi(((x == 0) | (y == 0) | (x == w - 1) | (y == h - 1)).astype(np.int64))
    if acc is not None:
        a = np.asarray(acc)
        if a.dtype != np.int64 or a.shape != (h, w):
            raise ValueError(f"acc must be int64 {(h, w)}, got {a.dtype} {a.shape}")
        a = a.view(np.uint64).ravel()[p]
        S, c = (a & np.uint64(SUM_MASK)).astype(np.int64), (a >> np.uint64(COUNT_SHIFT)).astype(np.int64)
        table[:, 10], table[:, 11], table[:, 12] = add(c > 0), add(c), add(S)
        table[:, 13] = hi(np.where(c > 0, (2 * S + c) // (2 * np.maximum(c, 1)), 0))
    return labels, table
