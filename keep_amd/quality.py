"""Tile quality control: the host side of ``KEEPModel.tile_quality`` / ``region_quality`` / ``pen_mask`` and of
the ``quality=`` keyword of ``region_grid`` / ``encode_region`` / ``cohort.extract_slide_features``.

  * the per-pixel rules (``QualityRules``) and the words the kernels read them from (``QualityRules.blob``);
  * a tile table on its device and how to read it (``TileQuality``), and the decision on it (``QualityGate``);
  * numpy restatements, the yardsticks of the device kernels (``classify_numpy``, ``pen_mask_numpy``, ``tile_quality_numpy``);
  * ``exclude``: the pixels of chosen classes taken out of a ``TissueMask``.

Every pixel gets exactly ONE class, the first that applies of

  1. pen ink, of the lowest class id with a box that holds the pixel (``PEN_CLASSES``);
  2. dark:   ``max(r, g, b) <= dark_max``;
  3. glass:  ``min(r, g, b) >= white_min``;
  4. tissue: ``max > 0`` and ``255 (max - min) >= sat_min max``, the rule of ``keep_amd.region.TissueRule`` (HSV saturation
     ``>= sat_min / 255``, exact in integers; ``region.saturation_numpy`` is the same quantity rounded to a byte);
  5. other.

so a tile's class counts and "other" sum to its pixels.  Focus is the variance of an integer Laplacian: with the grey level
``g = (77 r + 150 g + 29 b + 128) >> 8``, ``L = 4 g(x,y) - g(x-1,y) - g(x+1,y) - g(x,y-1) - g(x,y+1)`` over the ``(P - 2)^2`` interior
pixels of the tile itself; no pixel outside the tile is read, so a tile's numbers do not depend on where it lies.

The default pen table is a handful of RGB boxes chosen by eye for saturated marker strokes on bright-field H & E scans.  It claims
parity with no library's pen filter (HistoQC's among them); slides marked with other inks want boxes of their own.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np
import torch

from .region import TissueMask

PEN_CLASSES = ("blue", "green", "red", "black")
CLASS_NAMES = ("none", "pen_blue", "pen_green", "pen_red", "pen_black", "dark", "glass", "tissue")   # the bytes of a class mask
DARK, GLASS, TISSUE = 5, 6, 7
MAX_BOXES = 32
MAX_PATCH = 1024
MAX_CELLS = (1 << 24) - 1
NCOLS = 12              # pen 0..3, dark, glass, tissue, S L, S L^2, n_t, S L over tissue, S L^2 over tissue
BLOB_HEAD = 8
BLOB_WORDS = BLOB_HEAD + 3 * 256

# (class, r_lo, r_hi, g_lo, g_hi, b_lo, b_hi), bounds inclusive.  Haematoxylin (r 60-130, g 30-90, b 120-180) and eosin (r > 200) stay
# outside every box; so does the black of a scanner edge (every channel <= 40), which is "dark".
DEFAULT_PEN = (
    (0, 0, 60, 0, 140, 150, 255),        # blue marker, full strength
    (0, 0, 90, 90, 170, 190, 255),       # blue marker, thin stroke
    (1, 0, 110, 120, 255, 0, 120),       # green marker
    (2, 170, 255, 0, 70, 0, 70),         # red marker
    (3, 41, 85, 41, 85, 41, 95),         # black marker: a neutral dark grey
)


def _integer(v, name: str, lo: int, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or v > hi:
        raise ValueError(f"{name} must be an integer in [{lo}, {hi}], got {v!r}")
    return int(v)


@dataclass(frozen=True)
class QualityRules:
    """The per-pixel rules (module docstring).  ``pen``: up to 32 boxes ``(cls, r_lo, r_hi, g_lo, g_hi, b_lo, b_hi)``, bounds inclusive
    in 0..255, ``cls`` in 0..3 (``PEN_CLASSES``); an empty tuple switches ink off."""
    sat_min: int = 20
    white_min: int = 220
    dark_max: int = 40
    pen: Tuple[Tuple[int, int, int, int, int, int, int], ...] = DEFAULT_PEN

    def __post_init__(self):
        for name in ("sat_min", "white_min", "dark_max"):
            object.__setattr__(self, name, _integer(getattr(self, name), name, 0, 255))
        if not isinstance(self.pen, (tuple, list)):
            raise ValueError(f"pen must be a tuple of boxes (cls, r_lo, r_hi, g_lo, g_hi, b_lo, b_hi), got {self.pen!r}")
        if len(self.pen) > MAX_BOXES:
            raise ValueError(f"pen takes at most {MAX_BOXES} boxes, got {len(self.pen)}")
        boxes = []
        for i, box in enumerate(self.pen):
            if not isinstance(box, (tuple, list)) or len(box) != 7:
                raise ValueError(f"pen box {i} must be (cls, r_lo, r_hi, g_lo, g_hi, b_lo, b_hi), got {box!r}")
            cls = _integer(box[0], f"pen box {i}: cls", 0, len(PEN_CLASSES) - 1)
            b = [_integer(v, f"pen box {i}: bound", 0, 255) for v in box[1:]]
            if b[0] > b[1] or b[2] > b[3] or b[4] > b[5]:
                raise ValueError(f"pen box {i}: a lower bound exceeds its upper bound: {tuple(box)!r}")
            boxes.append((cls, *b))
        object.__setattr__(self, "pen", tuple(boxes))

    def blob(self) -> np.ndarray:
        """The int32 ``[776]`` words ``keep_region_quality`` / ``keep_pen_mask`` read (include/keep_hip.h): the three limits, the number of
        boxes, the first box of class 1, 2 and 3 after a stable sort by class, 0, then per channel 256 words whose bit i says that box i
        holds that value.  Built once per set of rules; a copy is returned."""
        return _blob(self).copy()


@functools.lru_cache(maxsize=64)
def _blob(rules: "QualityRules") -> np.ndarray:
    boxes = sorted(rules.pen, key=lambda b: b[0])
    out = np.zeros(BLOB_WORDS, np.int64)
    out[:4] = rules.sat_min, rules.white_min, rules.dark_max, len(boxes)
    for k in (1, 2, 3):
        out[3 + k] = sum(1 for b in boxes if b[0] < k)
    v = np.arange(256)
    for i, b in enumerate(boxes):
        for c in range(3):
            out[BLOB_HEAD + 256 * c:BLOB_HEAD + 256 * (c + 1)] |= ((v >= b[1 + 2 * c]) & (v <= b[2 + 2 * c])).astype(np.int64) << i
    return out.astype(np.uint32).view(np.int32)


def check_rules(rules) -> QualityRules:
    rules = QualityRules() if rules is None else rules
    if not isinstance(rules, QualityRules):
        raise ValueError(f"rules must be a QualityRules, got {type(rules).__name__}")
    return rules


def check_patch(patch) -> int:
    return _integer(patch, "patch_size", 1, MAX_PATCH)


def check_pen_class(cls) -> Optional[int]:
    if cls is None:
        return None
    if isinstance(cls, str):
        if cls not in PEN_CLASSES:
            raise ValueError(f"pen class must be one of {PEN_CLASSES} or 0..3, got {cls!r}")
        return PEN_CLASSES.index(cls)
    return _integer(cls, "pen class", 0, len(PEN_CLASSES) - 1)


# ------------------------------------------------------------------------------------------------ the table and the gate
class TileQuality:
    """The table of ``keep_region_quality`` on its device: ``table`` int64 ``[N, 12]`` (torch) and the tiles' side ``patch``.
    Columns: 0-3 the pixels of pen class 0..3, 4 dark, 5 glass, 6 tissue; 7, 8 the sum of L and of L^2 over the ``(patch - 2)^2``
    interior pixels; 9 the interior pixels whose own class is tissue, 10, 11 the two sums over those."""

    def __init__(self, table: torch.Tensor, patch: int):
        if not isinstance(table, torch.Tensor) or table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != NCOLS:
            raise ValueError(f"table must be an int64 [N, {NCOLS}] tensor, got {getattr(table, 'dtype', type(table))} "
                             f"{tuple(getattr(table, 'shape', ()))}")
        self.table = table
        self.patch = check_patch(patch)

    @property
    def n(self) -> int:
        return int(self.table.shape[0])

    @property
    def pixels(self) -> int:
        return self.patch * self.patch

    @property
    def interior(self) -> int:
        return max(self.patch - 2, 0) ** 2

    def __repr__(self):
        return f"TileQuality({self.n} tiles of {self.patch} on {self.table.device})"

    def pen_count(self, cls=None) -> torch.Tensor:
        c = check_pen_class(cls)
        return self.table[:, :4].sum(dim=1) if c is None else self.table[:, c]

    def _share(self, count: torch.Tensor) -> torch.Tensor:
        # tensor by tensor: a true division (by a Python number torch multiplies with its reciprocal on the device, one ulp off)
        return count.to(torch.float64) / torch.full_like(count, self.pixels, dtype=torch.float64)

    def pen_fraction(self, cls=None) -> torch.Tensor:
        """The share of ink pixels, of all classes or of one (an id or a name of ``PEN_CLASSES``) -> float64 ``[N]``."""
        return self._share(self.pen_count(cls))

    def dark_fraction(self) -> torch.Tensor:
        return self._share(self.table[:, 4])

    def glass_fraction(self) -> torch.Tensor:
        return self._share(self.table[:, 5])

    def tissue_fraction(self) -> torch.Tensor:
        return self._share(self.table[:, 6])

    def other_count(self) -> torch.Tensor:
        return self.pixels - self.table[:, :7].sum(dim=1)

    def focus(self, tissue: bool = False) -> torch.Tensor:
        """The variance of the Laplacian over the interior pixels (``tissue=True``: over those whose own class is tissue) -> float64
        ``[N]``: ``(n S2 - S1^2) / n^2`` with the numerator taken in exact integers (it stays below 2^61), NaN where n = 0."""
        t = self.table
        if tissue:
            n, s1, s2 = t[:, 9], t[:, 10], t[:, 11]
        else:
            n, s1, s2 = torch.full_like(t[:, 7], self.interior), t[:, 7], t[:, 8]
        num = (n * s2 - s1 * s1).to(torch.float64)
        den = (n * n).to(torch.float64)
        return torch.where(n > 0, num / den.clamp(min=1.0), torch.full_like(num, float("nan")))

    def to_numpy(self) -> np.ndarray:
        return self.table.cpu().numpy()


def _fraction(v, name: str) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) <= 1.0:
        raise ValueError(f"{name} must lie in [0, 1], got {v!r}")
    return float(v)


@dataclass(frozen=True)
class QualityGate:
    """Which tiles are worth encoding.  A tile is kept iff it holds at least ``ceil(min_tissue P^2)`` tissue pixels, at most
    ``floor(max_pen P^2)`` ink pixels of all classes and ``floor(max_dark P^2)`` dark pixels (integer comparisons, as
    ``keep_amd.region.tissue_params`` makes its pixel count) and its focus (over the tissue pixels when ``focus_on_tissue``) is
    ``>= min_focus``; a NaN focus (no such pixel) fails every positive ``min_focus``.  The defaults keep every tile."""
    rules: QualityRules = field(default_factory=QualityRules)
    min_tissue: float = 0.0
    max_pen: float = 1.0
    max_dark: float = 1.0
    min_focus: float = 0.0
    focus_on_tissue: bool = True

    def __post_init__(self):
        object.__setattr__(self, "rules", check_rules(self.rules))          # None: the default rules
        for name in ("min_tissue", "max_pen", "max_dark"):
            object.__setattr__(self, name, _fraction(getattr(self, name), name))
        f = self.min_focus
        if isinstance(f, bool) or not isinstance(f, (int, float, np.integer, np.floating)) or not 0.0 <= float(f) < math.inf:
            raise ValueError(f"min_focus must be a finite number >= 0, got {f!r}")
        object.__setattr__(self, "min_focus", float(f))
        if not isinstance(self.focus_on_tissue, (bool, np.bool_)):
            raise ValueError(f"focus_on_tissue must be a bool, got {self.focus_on_tissue!r}")

    def limits(self, patch: int) -> Tuple[int, int, int]:
        """-> (least tissue pixels, most ink pixels, most dark pixels) of a tile of side ``patch``."""
        p2 = patch * patch
        return int(math.ceil(self.min_tissue * p2)), int(math.floor(self.max_pen * p2)), int(math.floor(self.max_dark * p2))

    def keep(self, q: TileQuality) -> torch.Tensor:
        """-> bool ``[N]`` on the table's device."""
        if not isinstance(q, TileQuality):
            raise ValueError(f"q must be a TileQuality, got {type(q).__name__}")
        lo_t, hi_p, hi_d = self.limits(q.patch)
        t = q.table
        keep = (t[:, 6] >= lo_t) & (t[:, :4].sum(dim=1) <= hi_p) & (t[:, 4] <= hi_d)
        if self.min_focus > 0:
            keep = keep & (q.focus(tissue=bool(self.focus_on_tissue)) >= self.min_focus)          # NaN >= x is False
        return keep


def check_gate(quality) -> Optional[QualityGate]:
    """The ``quality=`` keyword: ``None`` or a ``QualityGate``."""
    if quality is not None and not isinstance(quality, QualityGate):
        raise ValueError(f"quality must be None or a QualityGate, got {type(quality).__name__}")
    return quality


# ------------------------------------------------------------------------------------------------ the restatements
def _rgb(image, name: str) -> np.ndarray:
    a = image.cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4):
        raise ValueError(f"{name} must be uint8 [h,w,3|4], got {a.dtype} {a.shape}")
    return a[..., :3].astype(np.int64)


def classify_numpy(image, rules: Optional[QualityRules] = None) -> np.ndarray:
    """uint8 ``[h,w,3|4]`` -> the class byte of every pixel, uint8 ``[h,w]``: 0 none, 1-4 pen class + 1, 5 dark, 6 glass, 7 tissue.
    Straight from the boxes and the priority list, without the kernels' tables."""
    rules = check_rules(rules)
    c = _rgb(image, "image")
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    mx, mn = c.max(axis=2), c.min(axis=2)
    out = np.zeros(mx.shape, np.uint8)
    out[(mx > 0) & (255 * (mx - mn) >= rules.sat_min * mx)] = TISSUE
    out[mn >= rules.white_min] = GLASS
    out[mx <= rules.dark_max] = DARK
    for cls in reversed(range(len(PEN_CLASSES))):              # the lowest class is written last
        for k, r0, r1, g0, g1, b0, b1 in rules.pen:
            if k == cls:
                out[(r >= r0) & (r <= r1) & (g >= g0) & (g <= g1) & (b >= b0) & (b <= b1)] = cls + 1
    return out


def pen_mask_numpy(thumbnail, rules: Optional[QualityRules] = None) -> np.ndarray:
    """``KEEPModel.pen_mask`` restated on the host."""
    return classify_numpy(thumbnail, rules)


def grey_numpy(image) -> np.ndarray:
    c = _rgb(image, "image")
    return (77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8


def laplacian_numpy(grey: np.ndarray) -> np.ndarray:
    """int64 ``[h,w]`` grey levels -> L on the ``(h - 2) x (w - 2)`` interior pixels (empty below 3 a side)."""
    g = np.asarray(grey, np.int64)
    if g.shape[0] < 3 or g.shape[1] < 3:
        return np.zeros((max(g.shape[0] - 2, 0), max(g.shape[1] - 2, 0)), np.int64)
    return 4 * g[1:-1, 1:-1] - g[1:-1, :-2] - g[1:-1, 2:] - g[:-2, 1:-1] - g[2:, 1:-1]


def check_cells_host(cells, H: int, W: int, patch: int) -> np.ndarray:
    c = cells.cpu().numpy() if isinstance(cells, torch.Tensor) else np.asarray(cells)
    c = c.reshape(-1, 2) if c.size == 0 else c
    if c.ndim != 2 or c.shape[1] != 2 or not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f"cells must be integers [N,2] (x, y), got {c.dtype} {c.shape}")
    c = c.astype(np.int64)
    if c.size and (c.min() < 0 or (c[:, 0] + patch > W).any() or (c[:, 1] + patch > H).any()):
        raise ValueError(f"a cell (x, y) has x < 0, y < 0, x + {patch} > {W} or y + {patch} > {H}")
    return c


def tile_quality_numpy(region, cells, patch: int, rules: Optional[QualityRules] = None) -> np.ndarray:
    """``keep_region_quality`` restated on the host: uint8 region ``[H,W,3|4]``, cells ``(x, y)`` integers ``[N,2]`` -> int64 ``[N, 12]``."""
    rules, patch = check_rules(rules), check_patch(patch)
    a = region.cpu().numpy() if isinstance(region, torch.Tensor) else np.asarray(region)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4):
        raise ValueError(f"region must be uint8 [H,W,3|4], got {a.dtype} {a.shape}")
    H, W = a.shape[:2]
    c = check_cells_host(cells, H, W, patch)
    out = np.zeros((c.shape[0], NCOLS), np.int64)
    for i, (x, y) in enumerate(c):
        t = a[y:y + patch, x:x + patch]
        cls = classify_numpy(t, rules)
        out[i, :7] = np.bincount(cls.ravel(), minlength=8)[1:8]
        L = laplacian_numpy(grey_numpy(t))
        tis = cls[1:-1, 1:-1] == TISSUE if patch >= 3 else np.zeros(L.shape, bool)
        out[i, 7], out[i, 8] = L.sum(), (L * L).sum()
        out[i, 9], out[i, 10], out[i, 11] = tis.sum(), L[tis].sum(), (L[tis] ** 2).sum()
    return out


# ------------------------------------------------------------------------------------------------ classes out of a tissue mask
def exclude(mask: TissueMask, classes_u8, drop=(1, 2, 3, 4, 5), radius: int = 0, model=None) -> TissueMask:
    """A ``TissueMask`` without the pixels whose class (a class mask of ``KEEPModel.pen_mask`` / ``pen_mask_numpy``, of the tissue
    mask's shape) is in ``drop`` (default: every ink and dark) -> a new ``TissueMask`` of the same geometry.  ``radius > 0`` first
    grows the dropped set by a true disc: every pixel within ``radius`` pixels (Euclidean, ``<=``) of a dropped one goes too, so the
    halo of a pen stroke leaves with it.  ``model``: a ``KEEPModel`` runs the dilation on its device (``dilate_mask``); without one it is
    the numpy restatement of the same distance transform (``keep_amd.lesion.dist2_numpy``)."""
    if not isinstance(mask, TissueMask):
        raise ValueError(f"mask must be a TissueMask, got {type(mask).__name__}")
    c = torch.from_numpy(np.ascontiguousarray(classes_u8)) if isinstance(classes_u8, np.ndarray) else classes_u8
    if not isinstance(c, torch.Tensor) or c.dtype != torch.uint8 or tuple(c.shape) != tuple(mask.mask.shape):
        raise ValueError(f"classes_u8 must be uint8 of the tissue mask's shape {tuple(mask.mask.shape)}, got "
                         f"{getattr(c, 'dtype', type(c))} {tuple(getattr(c, 'shape', ()))}")
    drop = tuple(_integer(d, "drop", 0, 255) for d in (drop if isinstance(drop, (tuple, list)) else (drop,)))
    radius = _integer(radius, "radius", 0, 1023)
    c = c.to(mask.mask.device)
    dropped = torch.zeros_like(c, dtype=torch.bool)
    for d in drop:
        dropped |= c == d
    if radius > 0 and bool(dropped.any()):
        reach = math.nextafter(float(radius), math.inf)         # dilate_mask takes "< distance": <= radius in float64
        if model is not None:
            grown = model.dilate_mask(dropped.to(torch.uint8), reach).mask
            dropped = grown.to(dropped.device) != 0
        else:
            from .lesion import dist2_numpy, distance_threshold
            R, k = distance_threshold(reach)
            dropped = torch.from_numpy(dist2_numpy(dropped.cpu().numpy(), R).astype(np.int64) <= k).to(dropped.device)
    out = mask.mask & (~dropped).to(torch.uint8)
    return TissueMask(out, mask.downsample, mask.mode, mask.threshold)
