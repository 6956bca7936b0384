"""The subtype map: the spatial output of the subtyping flow.

``wsi.zero_shot_subtyping`` (``WSI_evaluation/subtyping_utils.py:67-83``) reduces the refined per-tile class probabilities ``[U, C]`` to
one slide label.  Here they are kept in slide geometry: ``KEEPModel.class_raster`` scatters them into C planes of the heatmap's
accumulator word (:class:`ClassRaster`), ``KEEPModel.class_map`` takes the per-pixel argmax with its confidence (:class:`ClassMap`),
``KEEPModel.label_confusion`` compares two label maps and ``KEEPModel.render_class_map`` paints one with a palette.

Everything is integer arithmetic on the 16-bit fixed point of ``keep_amd.heatmap``; the device kernels (``csrc/classmap.hip``) equal
the numpy restatements below exactly (``class_raster_numpy`` / ``class_argmax_numpy`` / ``confusion_numpy`` / ``class_render_numpy``).
Only ``fractions`` and :func:`overlap_from_confusion` are floating point, float64 on the host.

Label values: ``0 .. C - 1`` a class, ``254`` undecided (covered, but below ``min_value`` or ``min_margin``), ``255`` nothing to say
(no tile covers the pixel, or it lies outside the tissue mask)."""
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from .heatmap import (COUNT_SHIFT, MAX_PIXELS, MAX_TILES, SUM_MASK, TileRaster, _integer, check_raster_args, check_tiles, footprints_numpy,
                      quantize, quantize_numpy, render_args, unpack_numpy)

MAX_CLASSES = 64
UNDECIDED = 254
NO_LABEL = 255


# ------------------------------------------------------------------------------------------------ argument checks
def check_classes(n_classes, shape=None) -> int:
    """The number of planes: an integer in 1..64, and with ``shape`` = (h, w) also ``C h w <= 2^30``."""
    C = _integer(n_classes, "the number of classes")
    if C < 1 or C > MAX_CLASSES:
        raise ValueError(f"the number of classes must lie in [1, {MAX_CLASSES}], got {C}")
    if shape is not None and C * int(shape[0]) * int(shape[1]) > MAX_PIXELS:
        raise ValueError(f"a class raster of {C} planes of {shape[0]}x{shape[1]} pixels: need C * h * w <= 2^30")
    return C


def check_class_tiles(coords, values) -> Tuple[int, int]:
    """Shapes of one call's tiles: coords [N,2] of an integer type, values [N,C] of a floating type, 1 <= C <= 64 -> (N, C)."""
    vs = tuple(values.shape)
    if len(vs) != 2:
        raise ValueError(f"class values must be [N, C], got {vs}")
    C = check_classes(vs[1])
    return check_tiles(coords, values[:, 0]), C


def check_labels(coords, labels, n_classes: int) -> int:
    """``labels=``: integers [N] beside coords [N,2], every one in ``0 .. C - 1`` (read on the host) -> N."""
    ls, ld = tuple(labels.shape), labels.dtype
    integer = (not ld.is_floating_point and ld != torch.bool) if isinstance(ld, torch.dtype) else ld.kind in "iu"
    if not integer or len(ls) != 1:
        raise ValueError(f"labels must be integers [N], got {ld} {ls}")
    N = check_tiles(coords, np.zeros(ls, np.float32))
    if N and (int(labels.min()) < 0 or int(labels.max()) >= n_classes):
        raise ValueError(f"labels must lie in 0..{n_classes - 1}, got {int(labels.min())}..{int(labels.max())}")
    return N


def check_class_names(classes, n_classes: Optional[int] = None):
    if classes is None:
        return None
    names = tuple(str(c) for c in classes)
    if n_classes is not None and len(names) != n_classes:
        raise ValueError(f"{len(names)} class names for {n_classes} classes")
    return names


def class_map_args(min_value=0.0, min_margin=0.0) -> Tuple[int, int]:
    """The two thresholds of the label map in the raster's fixed point -> (min16, margin16)."""
    return quantize(min_value), quantize(min_margin)


def palette(n_classes) -> np.ndarray:
    """The default colours of C classes, uint8 [C,3], from an integer formula; a caller's own uint8 [C,3] array passes through
    :func:`check_palette`.  Class c takes the hue ``H = (1530 c) // C`` on a wheel of 6 x 255 steps at full saturation and value:
    with ``s = H // 255`` and ``f = H % 255`` the colour is ``(255, f, 0)``, ``(255 - f, 255, 0)``, ``(0, 255, f)``, ``(0, 255 - f, 255)``,
    ``(f, 0, 255)``, ``(255, 0, 255 - f)`` for s = 0..5: red, then round the wheel through yellow, green, cyan, blue and magenta.  No
    parity with any library's palette is claimed; the colours of up to 64 classes are distinct."""
    C = check_classes(n_classes)
    out = np.zeros((C, 3), np.uint8)
    for c in range(C):
        H = (1530 * c) // C
        s, f = H // 255, H % 255
        out[c] = [(255, f, 0), (255 - f, 255, 0), (0, 255, f), (0, 255 - f, 255), (f, 0, 255), (255, 0, 255 - f)][s]
    return out


def check_palette(pal, n_classes: int) -> np.ndarray:
    """``palette=``: None for :func:`palette`, or a uint8 [C,3] array -> uint8 [C,3], contiguous, on the host."""
    if pal is None:
        return palette(n_classes)
    p = pal.detach().cpu().numpy() if isinstance(pal, torch.Tensor) else np.asarray(pal)
    if p.dtype != np.uint8 or p.shape != (n_classes, 3):
        raise ValueError(f"a palette must be uint8 [{n_classes},3], got {p.dtype} {p.shape}")
    return np.ascontiguousarray(p)


def check_label_map(m, name: str, shape=None):
    """A uint8 ``[h,w]`` numpy array or torch tensor, or a :class:`ClassMap` (its labels) -> the array."""
    if isinstance(m, ClassMap):
        m = m.labels
    ok = (isinstance(m, np.ndarray) and m.dtype == np.uint8) or (isinstance(m, torch.Tensor) and m.dtype == torch.uint8)
    if not ok or m.ndim != 2:
        raise ValueError(f"{name} must be a uint8 [h, w] label map or a ClassMap, got {getattr(m, 'dtype', type(m))} {tuple(getattr(m, 'shape', ()))}")
    h, w = int(m.shape[0]), int(m.shape[1])
    if h < 1 or w < 1 or h * w > MAX_PIXELS:
        raise ValueError(f"{name} of {h}x{w} pixels: need 1 <= h * w <= 2^30")
    if shape is not None and (h, w) != tuple(shape):
        raise ValueError(f"{name} has shape {(h, w)}, expected {tuple(shape)}")
    return m


# ------------------------------------------------------------------------------------------------ the classes
class ClassRaster:
    """C accumulators and their geometry: ``acc`` int64 ``[C,h,w]``, plane c a :class:`keep_amd.heatmap.TileRaster` accumulator of
    class c's values (bits 0..39 the sum of the fixed-point values of the covering tiles, bits 40..63 their number: the same in every
    plane), ``downsample``, ``patch``, ``origin`` and ``tiles`` as a ``TileRaster`` has them (the cap of 2^24 - 1 tiles included) and
    ``classes``, optional names.  ``KEEPModel.class_raster`` makes and extends one."""

    def __init__(self, acc: torch.Tensor, downsample: int, patch: int, origin=(0, 0), tiles: int = 0, classes=None, model=None):
        if not isinstance(acc, torch.Tensor) or acc.dtype != torch.int64 or acc.dim() != 3 or not acc.is_contiguous():
            raise ValueError("acc must be a contiguous int64 [C,h,w] tensor")
        check_classes(acc.shape[0])
        self.patch, self.downsample, _, self.origin = check_raster_args(patch, downsample, acc.shape[1:], origin)
        check_classes(acc.shape[0], acc.shape[1:])
        self.classes = check_class_names(classes, int(acc.shape[0]))
        self.acc = acc
        self.tiles = 0
        self._model = model
        self.claim(tiles)

    @property
    def n_classes(self) -> int:
        return int(self.acc.shape[0])

    @property
    def shape(self) -> Tuple[int, int]:
        return int(self.acc.shape[1]), int(self.acc.shape[2])

    def __repr__(self):
        return (f"ClassRaster({self.n_classes} x {self.shape} on {self.acc.device}, downsample={self.downsample}, patch={self.patch}, "
                f"origin={self.origin}, tiles={self.tiles})")

    def claim(self, n: int) -> None:
        """Count ``n`` more tiles against the cap, before they are added; ValueError beyond 2^24 - 1."""
        n = _integer(n, "the number of tiles")
        if n < 0 or self.tiles + n > MAX_TILES:
            raise ValueError(f"a raster takes at most 2^24 - 1 = {MAX_TILES} tiles in all (its count field is 24 bits): {self.tiles} added, "
                             f"{n} more asked for")
        self.tiles += n

    def check_geometry(self, n_classes: int, patch: int, downsample: int, shape, origin) -> None:
        if (self.n_classes, self.patch, self.downsample, self.shape, self.origin) != (n_classes, patch, downsample, tuple(shape), tuple(origin)):
            raise ValueError(f"into= raster has {self.n_classes} classes, patch {self.patch}, downsample {self.downsample}, shape {self.shape}, "
                             f"origin {self.origin}; the call has {n_classes}, {patch}, {downsample}, {tuple(shape)}, {tuple(origin)}")

    def plane(self, c: int) -> TileRaster:
        """Class c's accumulator as a ``TileRaster``: a view, no copy, so everything that takes a ``TileRaster`` takes it."""
        c = _integer(c, "the class")
        if not 0 <= c < self.n_classes:
            raise ValueError(f"class {c} outside 0..{self.n_classes - 1}")
        return TileRaster(self.acc[c], self.downsample, self.patch, self.origin, self.tiles, self._model)

    def _engine(self):
        from .model import engine_for
        if self.acc.device.type != "cuda":
            raise ValueError("this raster lives on the host: use the numpy restatements (class_argmax_numpy, smooth_numpy)")
        return engine_for(device=self.acc.device, model=self._model)

    def smooth(self, sigma=None, radius=None, taps=None, tissue=None) -> "ClassRaster":
        """``KEEPModel.smooth_raster`` plane by plane -> a new ``ClassRaster`` of the same geometry, names and ``tiles``.  The support
        is the same in every plane, so the counts (1 on it) still agree across the planes."""
        m = self._engine()
        planes = [m.smooth_raster(self.plane(c), sigma, radius, taps, tissue).acc for c in range(self.n_classes)]
        return ClassRaster(torch.stack(planes), self.downsample, self.patch, self.origin, self.tiles, self.classes, self._model)


class ClassMap:
    """The per-pixel call of a :class:`ClassRaster`: ``labels`` uint8 ``[h,w]`` (0..C-1, 254 undecided, 255 none), ``top`` and ``margin``,
    two ``TileRaster``s whose pixels hold ``(n << 40) | S_top`` and ``(n << 40) | (S_top - S_second)`` (zero where the label is 255):
    the winning class's mean and its lead over the runner-up, which ``render_heatmap`` / ``smooth_raster`` / ``mask_regions`` read
    like any raster.  ``raster`` is the ``ClassRaster`` it came from.  ``KEEPModel.class_map`` makes one."""

    def __init__(self, labels: torch.Tensor, top: TileRaster, margin: TileRaster, raster: ClassRaster, model=None):
        self.labels, self.top, self.margin, self.raster = labels, top, margin, raster
        self.n_classes, self.classes = raster.n_classes, raster.classes
        self.downsample, self.origin = raster.downsample, raster.origin
        self._model = model

    @property
    def shape(self) -> Tuple[int, int]:
        return int(self.labels.shape[0]), int(self.labels.shape[1])

    def __repr__(self):
        return f"ClassMap({self.n_classes} classes, {self.shape} on {self.labels.device}, downsample={self.downsample}, origin={self.origin})"

    def _engine(self):
        from .model import engine_for
        if self.labels.device.type != "cuda":
            raise ValueError("this label map lives on the host: use the numpy restatements (confusion_numpy)")
        return engine_for(device=self.labels.device, model=self._model)

    def mask(self, c: int) -> torch.Tensor:
        """uint8 {0,255} [h,w]: 255 where the label is class c; what ``mask_regions`` takes."""
        c = _integer(c, "the class")
        if not 0 <= c < self.n_classes:
            raise ValueError(f"class {c} outside 0..{self.n_classes - 1}")
        return (self.labels == c).to(torch.uint8) * 255

    def counts(self, within=None) -> torch.Tensor:
        """int64 [C + 1] on the device: the pixels of every class (inside ``within``), then those with no class (254 and 255): the
        diagonal of ``label_confusion`` of the map with itself."""
        return self._engine().label_confusion(self.labels, self.labels, self.n_classes, within).diagonal().contiguous()

    def fractions(self, within=None, drop_last: bool = False) -> np.ndarray:
        """float64 [C] (or [C - 1] with ``drop_last``) on the host: every class's share of the classified area, the pixels whose
        label is one of the classes counted; NaN when there are none."""
        n = np.array(self.counts(within).tolist()[:self.n_classes - int(bool(drop_last))], np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return n / n.sum()

    def slide_label(self, drop_last: bool = True, within=None) -> int:
        """The class with the largest area; ``drop_last`` leaves the last class out, as ``subtyping_utils.py:81`` drops ``Normal``
        (``frac[0:-1]``).  Ties go to the lowest index."""
        C = self.n_classes - int(bool(drop_last))
        if C < 1:
            raise ValueError("drop_last=True leaves no class of a one-class map")
        n = self.counts(within).tolist()[:C]
        return int(max(range(C), key=lambda c: (n[c], -c)))


def overlap_from_confusion(m) -> Dict[str, np.ndarray]:
    """Per-class overlap from ``label_confusion(a, b, C)`` (int64 [C+1, C+1], a along the rows) -> float64 [C] arrays ``dice``, ``iou``,
    ``precision`` and ``recall`` with a as the prediction and b as the truth: ``tp = m[c, c]``, ``A = sum_j m[c, j]``, ``B = sum_i m[i, c]``;
    dice = 2 tp / (A + B), iou = tp / (A + B - tp), precision = tp / A, recall = tp / B, NaN where a denominator is 0."""
    m = np.asarray(m.cpu() if isinstance(m, torch.Tensor) else m)
    if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 2 or m.dtype.kind not in "iu":
        raise ValueError(f"a confusion matrix must be integers [C+1, C+1], got {m.dtype} {m.shape}")
    C = m.shape[0] - 1
    tp = np.diagonal(m)[:C].astype(np.float64)
    A, B = m.sum(axis=1)[:C].astype(np.float64), m.sum(axis=0)[:C].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return {"dice": 2 * tp / (A + B), "iou": tp / (A + B - tp), "precision": tp / A, "recall": tp / B}


# ------------------------------------------------------------------------------------------------ the restatements
def one_hot_numpy(labels, n_classes: int) -> np.ndarray:
    """``labels=`` as the values they stand for: fp32 [N,C], 1 at the label."""
    l = np.asarray(labels).astype(np.int64).reshape(-1)
    out = np.zeros((l.size, n_classes), np.float32)
    out[np.arange(l.size), l] = 1
    return out


def class_raster_numpy(coords, values, patch: int, downsample: int, shape, origin=(0, 0), into: Optional[np.ndarray] = None) -> np.ndarray:
    """The class accumulate restated on the host -> int64 [C,h,w]; ``into`` adds to an earlier one (in place).  A row with a NaN is
    skipped in every plane."""
    patch, d, (h, w), origin = check_raster_args(patch, downsample, shape, origin)
    coords, values = np.asarray(coords), np.asarray(values)
    N, C = check_class_tiles(coords, values)
    check_classes(C, (h, w))
    if into is None:
        into = np.zeros((C, h, w), np.int64)
    elif into.dtype != np.int64 or into.shape != (C, h, w):
        raise ValueError(f"into must be int64 {(C, h, w)}, got {into.dtype} {into.shape}")
    acc = into.view(np.uint64)
    q, skip = quantize_numpy(values)
    q, skip = q.reshape(N, C), skip.reshape(N, C).any(axis=1)
    fp = footprints_numpy(coords, patch, d, (h, w), origin)
    for n in np.nonzero(~skip & (fp[:, 1] > fp[:, 0]) & (fp[:, 3] > fp[:, 2]))[0]:
        c0, c1, r0, r1 = fp[n]
        acc[:, r0:r1, c0:c1] += ((1 << COUNT_SHIFT) | q[n]).astype(np.uint64)[:, None, None]
    return into


def class_argmax_numpy(acc: np.ndarray, mask: Optional[np.ndarray] = None, min_value=0.0, min_margin=0.0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """keep_class_argmax restated on the host -> (label uint8 [h,w], top int64 [h,w], margin int64 [h,w])."""
    min16, margin16 = class_map_args(min_value, min_margin)
    acc = np.asarray(acc)
    if acc.dtype != np.int64 or acc.ndim != 3:
        raise ValueError(f"acc must be int64 [C,h,w], got {acc.dtype} {acc.shape}")
    C = check_classes(acc.shape[0], acc.shape[1:])
    S, n = unpack_numpy(acc)
    n = n[0].astype(np.int64)
    on = n > 0
    if mask is not None:
        if np.asarray(mask).shape != acc.shape[1:]:
            raise ValueError(f"mask must be {acc.shape[1:]}, got {np.asarray(mask).shape}")
        on &= np.asarray(mask) != 0
    best = np.argmax(S, axis=0)                                                  # the first of equal maxima: the smallest c
    top = np.take_along_axis(S, best[None], 0)[0]
    rest = S.copy()
    np.put_along_axis(rest, best[None], -1, 0)
    second = np.maximum(rest.max(axis=0), 0)                                     # 0 when C = 1
    gap = top - second
    label = np.where((top < min16 * n) | (gap < margin16 * n), UNDECIDED, best)
    label = np.where(on, label, NO_LABEL).astype(np.uint8)
    return label, np.where(on, (n << COUNT_SHIFT) | top, 0).astype(np.int64), np.where(on, (n << COUNT_SHIFT) | gap, 0).astype(np.int64)


def confusion_numpy(a, b, n_classes: int, within=None) -> np.ndarray:
    """keep_class_confusion restated on the host -> int64 [C+1, C+1]: ``m[i, j]`` the pixels inside ``within`` with a = i and b = j,
    every label >= C at index C."""
    C = check_classes(n_classes)
    a, b = np.asarray(a), np.asarray(b)
    check_label_map(a, "a")
    check_label_map(b, "b", a.shape)
    ia, ib = np.minimum(a.astype(np.int64), C).reshape(-1), np.minimum(b.astype(np.int64), C).reshape(-1)
    if within is not None:
        if np.asarray(within).shape != a.shape:
            raise ValueError(f"within must be {a.shape}, got {np.asarray(within).shape}")
        keep = np.asarray(within).reshape(-1) != 0
        ia, ib = ia[keep], ib[keep]
    return np.bincount(ia * (C + 1) + ib, minlength=(C + 1) ** 2).astype(np.int64).reshape(C + 1, C + 1)


def class_render_numpy(labels: np.ndarray, palette=None, n_classes: Optional[int] = None, thumbnail: Optional[np.ndarray] = None, alpha: float = 0.5,
                       strength: Optional[np.ndarray] = None, window=(0.0, 1.0), background=(255, 255, 255)) -> np.ndarray:
    """keep_class_render restated on the host -> uint8 [h,w,3].  ``palette``: uint8 [C,3] (default :func:`palette` of ``n_classes``);
    ``strength``: an int64 [h,w] accumulator (``ClassMap.margin`` / ``.top``) whose windowed mean scales alpha."""
    a, lo16, hi16, _, bg = render_args(alpha, window, 0.0, background)
    labels = np.asarray(labels)
    check_label_map(labels, "labels")
    if palette is None and n_classes is None:
        raise ValueError("give palette= or n_classes=")
    C = check_classes(n_classes if n_classes is not None else len(palette))
    pal = check_palette(palette, C).astype(np.int64)
    h, w = labels.shape
    if thumbnail is None:
        under = np.empty((h, w, 3), np.int64)
        under[:] = bg
    else:
        if thumbnail.dtype != np.uint8 or thumbnail.ndim != 3 or thumbnail.shape[:2] != (h, w) or thumbnail.shape[2] not in (3, 4):
            raise ValueError(f"thumbnail must be uint8 {(h, w)} x 3|4, got {thumbnail.dtype} {thumbnail.shape}")
        under = thumbnail[..., :3].astype(np.int64)
    a_eff = np.full((h, w), a, np.int64)
    if strength is not None:
        strength = np.asarray(strength)
        if strength.dtype != np.int64 or strength.shape != (h, w):
            raise ValueError(f"strength must be int64 {(h, w)}, got {strength.dtype} {strength.shape}")
        S, c = unpack_numpy(strength)
        c = c.astype(np.int64)
        span = hi16 - lo16
        idx = np.clip((2 * 255 * (S - lo16 * c) + span * c) // (2 * span * np.maximum(c, 1)), 0, 255)
        a_eff = (a * np.where(c > 0, idx, 0) + 127) // 255
    shown = labels < C
    colour = pal[np.where(shown, labels, 0)]
    blend = (a_eff[..., None] * colour + (256 - a_eff[..., None]) * under + 128) >> 8
    return np.where(shown[..., None], blend, under).astype(np.uint8)
