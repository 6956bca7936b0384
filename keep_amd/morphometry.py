"""Region shape: the second moments and the exact largest diameter of every region of a ``RegionTable``.

``KEEPModel.region_shape`` computes both on the device (``csrc/shape.hip``) and returns a :class:`RegionShape`.  It answers what the
table's area and box cannot: how long a lesion is along its own axis (the rule by which the CAMELYON16 evaluation sets isolated
tumour cells aside: ``regionprops(evaluation_mask)[i].major_axis_length < 275 / (resolution * 2^level)``) and what its largest
dimension is (isolated tumour cells below 0.2 mm, a micro-metastasis up to 2 mm, a macro-metastasis above).

Everything the device computes is an integer.

Moments.  ``sum_uu``, ``sum_vv``, ``sum_uv`` are the sums of ``u^2``, ``v^2`` and ``u v`` over a region's pixels with ``u = x - x0``,
``v = y - y0`` taken from the region's box origin, so that the sums stay small.  The central sums follow on the host in exact Python
integers: ``A sum_uu - sum_u^2`` with ``sum_u = sum_x - A x0``, and likewise for ``vv`` and ``uv``.

Feret diameter.  Region i is the union of the closed unit squares ``[x, x + 1] x [y, y + 1]`` of its pixels.  Its squared Feret
diameter ``d2`` is the largest squared Euclidean distance between two of its corner-lattice points; distance is convex, so that is
the largest distance between any two points of the region, an integer ``<= W^2 + H^2``.  The pair ``(ax, ay), (bx, by)`` is a maximal
pair with ``a < b`` in lattice row-major order ``y (W + 1) + x``: among the maximal pairs the one with the smallest ``a``, then the
smallest ``b``.  A label no pixel carries gives zero rows.

This module holds the host side: argument checks (ValueError before any device call), :class:`RegionShape` (whose float64
conversions are not part of the integer contract) and the restatement :func:`shape_numpy`, which the device kernels equal exactly."""
from typing import Optional, Tuple

import numpy as np
import torch

from .components import COLUMNS as TABLE_COLUMNS, RegionTable
from .heatmap import _integer

MOMENT_COLUMNS = ("sum_uu", "sum_vv", "sum_uv")
FERET_COLUMNS = ("d2", "ax", "ay", "bx", "by")
MAX_PIXELS = 1 << 30                                           # of a label image, as keep_regions_label's
MAX_LATTICE = 1 << 31                                          # a lattice index y (W + 1) + x fits 32 bits
MAX_PAIRS_LIMIT = 1 << 50
# The default cap on a call's candidate pairs: about one second of the pair walk at the rate tools/shape_bench.py measured
# 
DEFAULT_MAX_PAIRS = 1 << 39
_COL = {name: i for i, name in enumerate(TABLE_COLUMNS)}


# ------------------------------------------------------------------------------------------------ argument checks
def check_shape_args(h, w, feret: bool = True, max_pairs=DEFAULT_MAX_PAIRS) -> int:
    """The label image's shape against what the integer sums and the lattice index can hold -> max_pairs as an integer.  The sum of
    ``x^2`` over a region that fills the image is ``< h w^3 / 3``, so ``h w max(h, w)^2 < 3 * 2^63`` keeps every moment in int64 (a
    32768 x 32768 mask passes); ``h w <= 2^30`` is the entry points' own limit on a label image; with ``feret`` a lattice index must fit 32 bits: ``(h + 1) (w + 1) <= 2^31``."""
    h, w, max_pairs = _integer(h, "h"), _integer(w, "w"), _integer(max_pairs, "max_pairs")
    if h < 1 or w < 1:
        raise ValueError(f"labels of {h}x{w} pixels: need h, w >= 1")
    if h * w > MAX_PIXELS:
        raise ValueError(f"labels of {h}x{w} pixels: need h * w <= 2^30")
    if not h * w * max(h, w) ** 2 < 3 << 63:
        raise ValueError(f"labels of {h}x{w} pixels: a region's second moments could leave int64 (need h w max(h, w)^2 < 3 * 2^63)")
    if feret and (h + 1) * (w + 1) > MAX_LATTICE:
        raise ValueError(f"labels of {h}x{w} pixels: a lattice index must fit 32 bits (need (h + 1) (w + 1) <= 2^31)")
    if max_pairs < 0 or max_pairs > MAX_PAIRS_LIMIT:
        raise ValueError(f"max_pairs must lie in [0, 2^50], got {max_pairs}")
    return max_pairs


def camelyon16_itc_axis(mpp: float = 0.243, downsample: int = 32) -> float:
    """The major axis length in mask pixels below which the CAMELYON16 evaluation sets a lesion aside as isolated tumour cells:
    275 um, ``275 / (mpp * downsample)`` as the published evaluation writes it (35.4 pixels at level 5 of a 0.243 um slide)."""
    return 275 / (float(mpp) * downsample)


# ------------------------------------------------------------------------------------------------ the result
class RegionShape:
    """The shape of the regions of one ``RegionTable``.  ``moments``: int64 ``[n,3]`` (columns :data:`MOMENT_COLUMNS`) and ``feret``:
    int64 ``[n,5]`` (columns :data:`FERET_COLUMNS`; None if not asked for), torch, on the device that made them, row i - 1 for label
    i; ``table``: the ``RegionTable`` they belong to, in label order, which brings ``downsample`` and ``origin``.  Every column is an
    attribute (``.sum_uu``, ``.d2`` ...: int64 ``[n]`` views).  The methods below convert on the host in float64 and are not part of
    the integer contract."""

    def __init__(self, moments: torch.Tensor, feret: Optional[torch.Tensor], table: RegionTable):
        if not isinstance(table, RegionTable):
            raise ValueError(f"table must be a RegionTable, got {type(table).__name__}")
        if not isinstance(moments, torch.Tensor) or moments.dtype != torch.int64 or tuple(moments.shape) != (table.n, 3):
            raise ValueError(f"moments must be an int64 [{table.n},3] tensor")
        if feret is not None and (not isinstance(feret, torch.Tensor) or feret.dtype != torch.int64 or tuple(feret.shape) != (table.n, 5)):
            raise ValueError(f"feret must be an int64 [{table.n},5] tensor or None")
        self.moments, self.feret, self.table = moments, feret, table
        self._host = None

    @property
    def n(self) -> int:
        return int(self.moments.shape[0])

    @property
    def downsample(self):
        return self.table.downsample

    @property
    def origin(self):
        return self.table.origin

    def __len__(self) -> int:
        return self.n

    def __repr__(self):
        return f"RegionShape(n={self.n} on {self.moments.device}, feret={self.feret is not None}, downsample={self.downsample}, origin={self.origin})"

    def __getattr__(self, name):
        if name in MOMENT_COLUMNS:
            return self.moments[:, MOMENT_COLUMNS.index(name)]
        if name in FERET_COLUMNS:
            if self.feret is None:
                raise AttributeError(f"{name}: this RegionShape was made with feret=False")
            return self.feret[:, FERET_COLUMNS.index(name)]
        raise AttributeError(name)

    def numpy(self) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """(moments int64 [n,3], feret int64 [n,5] or None) on the host (read once)."""
        if self._host is None:
            self._host = (self.moments.cpu().numpy(), None if self.feret is None else self.feret.cpu().numpy())
        return self._host

    def _feret_host(self) -> np.ndarray:
        f = self.numpy()[1]
        if f is None:
            raise ValueError("this RegionShape was made with feret=False")
        return f

    def central_sums(self) -> list:
        """Per region ``(A, A sum_uu - sum_u^2, A sum_vv - sum_v^2, A sum_uv - sum_u sum_v)`` in exact Python integers: ``A^2`` times
        the central moments."""
        t, m = self.table.numpy(), self.numpy()[0]
        out = []
        for r, (suu, svv, suv) in zip(t.tolist(), m.tolist()):
            A = r[_COL["area"]]
            su, sv = r[_COL["sum_x"]] - A * r[_COL["x0"]], r[_COL["sum_y"]] - A * r[_COL["y0"]]
            out.append((A, A * suu - su * su, A * svv - sv * sv, A * suv - su * sv))
        return out

    def central_moments(self) -> np.ndarray:
        """float64 ``[n,3]``: ``mu20, mu02, mu11`` divided by the area, the covariance of the pixel coordinates
        (``np.cov(coords, bias=True)``): each an exact integer quotient rounded once.  NaN for a label no pixel carries."""
        out = np.full((self.n, 3), np.nan)
        for i, (A, cuu, cvv, cuv) in enumerate(self.central_sums()):
            if A > 0:
                out[i] = cuu / (A * A), cvv / (A * A), cuv / (A * A)         # true division of Python integers is rounded once
        return out

    def _eigen(self) -> Tuple[np.ndarray, np.ndarray]:
        """(l1, l2), ``l1 >= l2 >= 0``: the eigenvalues of ``[[mu20, mu11], [mu11, mu02]] / A``."""
        a, c, b = self.central_moments().T
        half = np.sqrt(((a - c) / 2) ** 2 + b * b)
        l1, l2 = (a + c) / 2 + half, (a + c) / 2 - half
        diag = b == 0                                                   # axis-parallel: the eigenvalues are the two variances themselves
        l1, l2 = np.where(diag, np.maximum(a, c), l1), np.where(diag, np.minimum(a, c), l2)
        return l1, np.maximum(l2, 0.0)

    def axis_lengths(self) -> np.ndarray:
        """float64 ``[n,2]``: ``4 sqrt(l1), 4 sqrt(l2)``, the major and minor axis lengths in mask pixels of the ellipse with the
        region's second central moments.  This is the formula of scikit-image's ``major_axis_length`` / ``minor_axis_length`` (which
        has no 1/12 pixel term) restated; scikit-image is not installed where this is built and tested, so parity with it is
        unpinned."""
        l1, l2 = self._eigen()
        return np.stack([4 * np.sqrt(l1), 4 * np.sqrt(l2)], axis=1)

    def eccentricity(self) -> np.ndarray:
        """float64 ``[n]``: ``sqrt(1 - l2 / l1)``; 0 for a one-pixel region."""
        l1, l2 = self._eigen()
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(l1 > 0, np.sqrt(np.maximum(1 - l2 / np.where(l1 > 0, l1, 1.0), 0.0)), np.where(np.isnan(l1), np.nan, 0.0))

    def orientation(self) -> np.ndarray:
        """float64 ``[n]``: ``0.5 atan2(2 mu11, mu20 - mu02)``, the angle of the major axis from +x with y pointing down, in
        ``(-pi / 2, pi / 2]``.  This is NOT scikit-image's convention (which measures from the row axis, counter-clockwise)."""
        a, c, b = self.central_moments().T
        return 0.5 * np.arctan2(2 * b, a - c)

    def feret_diameter(self) -> np.ndarray:
        """float64 ``[n]``: ``sqrt(d2)``, the largest diameter in mask pixels (0 for a label no pixel carries)."""
        return np.sqrt(self._feret_host()[:, 0].astype(np.float64))

    def feret_points(self) -> np.ndarray:
        """int64 ``[n,2,2]``: the two end points ``(x, y)`` of the largest diameter on the corner lattice."""
        return self._feret_host()[:, 1:5].reshape(-1, 2, 2).copy()

    def to_level0(self) -> dict:
        """``axis_lengths`` ``[n,2]`` and ``feret`` ``[n]`` times the downsample, ``feret_points`` ``[n,2,2]`` as ``origin + downsample * p``
        (float64; the last two only with the Feret columns)."""
        if self.downsample is None:
            raise ValueError("this shape's table has no downsample: pass a TissueMask or a raster to mask_regions")
        d, o = float(self.downsample), np.asarray(self.origin, np.float64)
        out = {"axis_lengths": self.axis_lengths() * d}
        if self.feret is not None:
            out["feret"] = self.feret_diameter() * d
            out["feret_points"] = self.feret_points().astype(np.float64) * d + o
        return out

    def to_um(self, mpp: float) -> dict:
        """:meth:`to_level0` in microns at ``mpp`` microns per level-0 pixel."""
        return {k: v * float(mpp) for k, v in self.to_level0().items()}

    def size_class(self, mpp: float, itc_um: float = 200.0, macro_um: float = 2000.0) -> np.ndarray:
        """int8 ``[n]`` by the Feret diameter in microns: 0 below ``itc_um`` (isolated tumour cells), 2 above ``macro_um`` (a
        macro-metastasis), 1 in between, both ends included (a micro-metastasis)."""
        if not 0 <= itc_um <= macro_um:
            raise ValueError(f"need 0 <= itc_um <= macro_um, got {itc_um!r} and {macro_um!r}")
        um = self.to_um(mpp).get("feret")
        if um is None:
            raise ValueError("this RegionShape was made with feret=False")
        return np.where(um < itc_um, 0, np.where(um > macro_um, 2, 1)).astype(np.int8)


# ------------------------------------------------------------------------------------------------ the restatement
def _feret_lines(xs, ys, x0, y0, bw, bh) -> Tuple[np.ndarray, np.ndarray]:
    """The candidates of one region -> (X, Y) int64: along the shorter box side (rows iff ``bh <= bw``) the four corners of the first
    and of the last pixel of every line that has pixels."""
    rows = bh <= bw
    L = min(bw, bh)
    line, pos, base = (ys - y0, xs, y0) if rows else (xs - x0, ys, x0)
    ok = (line >= 0) & (line < L)
    lo, hi = np.full(max(L, 0), np.iinfo(np.int64).max), np.full(max(L, 0), -1, np.int64)
    np.minimum.at(lo, line[ok], pos[ok])
    np.maximum.at(hi, line[ok], pos[ok])
    k = np.flatnonzero(hi >= lo)
    along = np.stack([lo[k], hi[k] + 1, lo[k], hi[k] + 1], axis=1).ravel()
    across = np.stack([base + k, base + k, base + k + 1, base + k + 1], axis=1).ravel()
    return (along, across) if rows else (across, along)


def _feret_best(X, Y, w: int, chunk: int = 2048) -> Tuple[int, int]:
    """The largest squared distance over all pairs and the smallest packed ``(a << 32) | b`` among the pairs that reach it."""
    index = Y * (w + 1) + X
    best, key = 0, None
    for i0 in range(0, len(X), chunk):
        d2 = (X[i0:i0 + chunk, None] - X[None, :]) ** 2 + (Y[i0:i0 + chunk, None] - Y[None, :]) ** 2
        m = int(d2.max())
        if m < best:
            continue
        ii, jj = np.nonzero(d2 == m)
        a, b = np.minimum(index[i0 + ii], index[jj]), np.maximum(index[i0 + ii], index[jj])
        k = int(((a << 32) | b).min())
        best, key = (m, k) if m > best or key is None else (m, min(key, k))
    return best, key


def shape_numpy(labels, table, feret: bool = True) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """The moments and the Feret diameter restated on the host -> (moments int64 ``[n,3]``, feret int64 ``[n,5]`` or None).
    ``labels``: integers ``[h,w]`` (values outside 1..n count as background); ``table``: the int64 ``[n,14]`` region table, of which the
    box is read.  Moments: sums over every label's pixels taken in int64 after a stable sort of the foreground by label
    (``regions_numpy``'s idiom).  Feret: per region the candidates of the module's rule and a numpy maximum over all their pairs,
    with the tie rule."""
    lab, t = np.asarray(labels), np.asarray(table)
    if lab.ndim != 2 or lab.size < 1:
        raise ValueError(f"labels must be [h, w] with h, w >= 1, got {lab.shape}")
    if t.ndim != 2 or t.shape[1] != len(TABLE_COLUMNS) or t.dtype != np.int64:
        raise ValueError(f"table must be int64 [n,{len(TABLE_COLUMNS)}], got {t.dtype} {t.shape}")
    h, w = lab.shape
    n = len(t)
    check_shape_args(h, w, feret)
    moments = np.zeros((n, 3), np.int64)
    out = np.zeros((n, 5), np.int64) if feret else None
    flat = np.where((lab >= 1) & (lab <= n), lab, 0).astype(np.int64).ravel()
    p = np.flatnonzero(flat)
    if n == 0 or len(p) == 0:
        return moments, out
    p = p[np.argsort(flat[p], kind="stable")]
    l = flat[p]
    start = np.searchsorted(l, np.arange(1, n + 1))
    count = np.bincount(l, minlength=n + 1)[1:]
    x0, y0 = t[:, _COL["x0"]], t[:, _COL["y0"]]
    y, x = p // w, p % w
    u, v = x - x0[l - 1], y - y0[l - 1]
    present = np.flatnonzero(count > 0)                            # a label no pixel carries has no segment: its row stays zero
    add = lambda a: np.add.reduceat(a.astype(np.int64), start[present])
    moments[present, 0], moments[present, 1], moments[present, 2] = add(u * u), add(v * v), add(u * v)
    if not feret:
        return moments, out
    for i in present.tolist():
        sl = slice(start[i], start[i] + count[i])
        X, Y = _feret_lines(x[sl], y[sl], int(x0[i]), int(y0[i]), int(t[i, _COL["x1"]] - x0[i]), int(t[i, _COL["y1"]] - y0[i]))
        if len(X) == 0:
            continue
        d2, key = _feret_best(X, Y, w)
        a, b = key >> 32, key & 0xFFFFFFFF
        out[i] = d2, a % (w + 1), a // (w + 1), b % (w + 1), b // (w + 1)
    return moments, out
