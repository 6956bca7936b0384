"""Region outlines: the boundary rings of a label image on the corner lattice, with holes, as polygons a viewer
opens, and an outline drawn into an image.

``KEEPModel.region_outlines`` traces the regions of a ``RegionTable`` (``KEEPModel.mask_regions`` / ``keep_amd.wsi.segment_regions``)
on the device and returns a :class:`RegionOutlines`; ``KEEPModel.draw_outlines`` paints them.  It stands where CLAM's ``segmentTissue``
hands back contour polygons with a hole list per contour and where a lesion goes into a viewer (QuPath, ASAP) as a polygon annotation.
It is NOT ``cv2.findContours``: OpenCV joins pixel centres, this joins pixel corners.

The specification.  Pixel ``p = y W + x`` with label ``l`` in 1..n has a directed crack edge on side ``s`` iff the pixel across that
side lies outside the image or carries another label: side 0 top, direction +x, start vertex ``(x, y)``; 1 right, +y, ``(x + 1, y)``;
2 bottom, -x, ``(x + 1, y + 1)``; 3 left, -y, ``(x, y + 1)`` (x to the right, y down: the region is on the walker's right).
``slot = 4 p + s``.  At the end vertex of an edge, with AR = ``p`` moved one step along the direction and AL = AR moved one step
across side ``s`` ("in" = inside the image with label ``l``): AR and AL in: turn left, side ``(s + 3) % 4`` of AL; AR in, AL out:
straight, side ``s`` of AR; both out: turn right, side ``(s + 1) % 4`` of ``p``; AR out and AL in (the saddle): right with
connectivity 4, left with connectivity 8, where the ring passes through the diagonal contact and touches itself at that vertex.
The successor map is a permutation of the edges and its cycles are the rings.  An edge is a corner iff its predecessor lies on
another side; a ring's leader is its corner edge with the smallest slot; its vertices are the start vertices of its corner edges in
walking order from the leader; rings are numbered in ascending leader slot.  With labels of ``mask_regions`` and the same
connectivity a region's first ring is its one outer ring (``lead = (first_x, first_y)``) and every other ring of it is a hole.

This module holds the host side: argument checks (ValueError before any device call), :class:`RegionOutlines` and the restatements
:func:`outlines_numpy` (sequential tracing, straight from the specification) and :func:`draw_numpy`.  The device kernels
(``csrc/outline.hip``) equal them exactly."""
from typing import List, Optional, Tuple

import numpy as np
import torch

from .components import COLUMNS as TABLE_COLUMNS, RegionTable
from .heatmap import _integer

COLUMNS = ("label", "start", "nvert", "nedge", "area2", "lead_x", "lead_y", "hole")
NCOLS = len(COLUMNS)
MAX_PIXELS = 1 << 28                                             # an edge slot 4 p + side fits an int32
MAX_RINGS = 1 << 20
MAX_WIDTH = 16
_DX, _DY = (1, 0, -1, 0), (0, 1, 0, -1)                          # an edge's direction by side; side s's outward normal is (s + 3) % 4's


# ------------------------------------------------------------------------------------------------ argument checks
def check_outline_args(connectivity, max_rings=MAX_RINGS) -> Tuple[int, int]:
    """-> (connectivity, max_rings) as integers."""
    connectivity, max_rings = _integer(connectivity, "connectivity"), _integer(max_rings, "max_rings")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity}")
    if max_rings < 0:
        raise ValueError(f"max_rings must be >= 0, got {max_rings}")
    return connectivity, max_rings


def labels_tensor(labels) -> torch.Tensor:
    """A label image (numpy or torch, host or device) -> an int32 [h,w] tensor on its own device."""
    t = torch.from_numpy(np.ascontiguousarray(labels)) if isinstance(labels, np.ndarray) else labels
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.int32:
        raise ValueError(f"labels must be an int32 [h, w] array, got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    h, w = int(t.shape[0]), int(t.shape[1])
    if h < 1 or w < 1 or h * w > MAX_PIXELS:
        raise ValueError(f"labels of {h}x{w} pixels: need 1 <= h * w <= 2^28")
    return t


def regions_labels(regions, n=None, connectivity=None):
    """What ``region_outlines`` / ``draw_outlines`` take -> (labels tensor, n, connectivity or None, downsample, origin).
    ``regions``: a ``RegionTable`` that kept its labels (it brings n, the downsample, the origin and the connectivity
    ``mask_regions`` used), or an int32 [h,w] label image with ``n=`` (None where the caller does not need one)."""
    if isinstance(regions, RegionTable):
        if regions.labels is None:
            raise ValueError("this RegionTable has no labels: call mask_regions with labels=True")
        if n is not None and _integer(n, "n") != regions.n:
            raise ValueError(f"n = {n}, the table has {regions.n} regions")
        return labels_tensor(regions.labels), regions.n, getattr(regions, "connectivity", None), regions.downsample, regions.origin
    t = labels_tensor(regions)
    if n is not None:
        n = _integer(n, "n")
        if n < 0 or n > t.numel():
            raise ValueError(f"n must lie in [0, h * w = {t.numel()}], got {n}")
    return t, n, connectivity, None, (0, 0)


def check_draw_args(color, width) -> Tuple[int, int]:
    """-> (R | G << 8 | B << 16, width)."""
    width = _integer(width, "width")
    if width < 1 or width > MAX_WIDTH:
        raise ValueError(f"width must lie in [1, {MAX_WIDTH}], got {width}")
    try:
        c = [_integer(v, "color") for v in color]
    except TypeError:
        raise ValueError(f"color must be three integers in [0, 255], got {color!r}") from None
    if len(c) != 3 or min(c) < 0 or max(c) > 255:
        raise ValueError(f"color must be three integers in [0, 255], got {color!r}")
    return c[0] | c[1] << 8 | c[2] << 16, width


def rgb_tensor(rgb, shape) -> torch.Tensor:
    """An image (numpy or torch, host or device) -> a uint8 [h,w,3] tensor of the labels' shape."""
    t = torch.from_numpy(np.ascontiguousarray(rgb)) if isinstance(rgb, np.ndarray) else rgb
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f"rgb must be a uint8 [h, w, 3] array, got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    if tuple(t.shape[:2]) != tuple(shape):
        raise ValueError(f"rgb is {tuple(t.shape[:2])}, the labels {tuple(shape)}")
    return t


def check_ring_count(r: int, max_rings: int) -> int:
    if r > max_rings:
        raise ValueError(f"the labels have {r} rings, max_rings is {max_rings}: raise min_area or max_rings")
    return r


# ------------------------------------------------------------------------------------------------ the result
class RegionOutlines:
    """The rings of one label image.  ``rings``: int64 ``[R,8]`` (torch, on the device that made it; columns :data:`COLUMNS`), in
    ascending leader slot; ``vertices``: int32 ``[V,2]`` ``(x, y)`` on the corner lattice (0..w, 0..h), ring after ring: ring r owns
    rows ``start[r] : start[r] + nvert[r]``; ``downsample``: level-0 pixels per mask pixel (None if unknown); ``origin``: the level-0
    position of pixel (0, 0); ``n``: the number of regions.  Every column is an attribute (``.label``, ``.area2`` ...: int64 ``[R]``
    views).  ``nedge`` is the perimeter in pixel sides; ``area2`` twice the enclosed area, > 0 for an outer ring and < 0 for a hole;
    a region's ``area2`` add up to twice its pixel count.  Rings are open (the first point is not repeated) except in GeoJSON."""

    def __init__(self, rings: torch.Tensor, vertices: torch.Tensor, downsample: Optional[int] = None, origin=(0, 0), n: Optional[int] = None):
        if not isinstance(rings, torch.Tensor) or rings.dtype != torch.int64 or rings.dim() != 2 or rings.shape[1] != NCOLS:
            raise ValueError(f"rings must be an int64 [R,{NCOLS}] tensor")
        if not isinstance(vertices, torch.Tensor) or vertices.dtype != torch.int32 or vertices.dim() != 2 or vertices.shape[1] != 2:
            raise ValueError("vertices must be an int32 [V,2] tensor")
        self.rings, self.vertices, self.downsample = rings, vertices, downsample
        self.origin = (int(origin[0]), int(origin[1]))
        self._host = None
        self.n = int(n) if n is not None else (int(self.numpy()[0][:, 0].max()) if rings.shape[0] else 0)

    @property
    def n_rings(self) -> int:
        return int(self.rings.shape[0])

    def __len__(self) -> int:
        return self.n_rings

    def __repr__(self):
        return (f"RegionOutlines({self.n_rings} rings, {int(self.vertices.shape[0])} vertices, n={self.n} on {self.rings.device}, "
                f"downsample={self.downsample}, origin={self.origin})")

    def __getattr__(self, name):
        if name in COLUMNS:
            return self.rings[:, COLUMNS.index(name)]
        raise AttributeError(name)

    def numpy(self) -> Tuple[np.ndarray, np.ndarray]:
        """(rings int64 [R,8], vertices int32 [V,2]) on the host (read once)."""
        if self._host is None:
            self._host = (self.rings.cpu().numpy(), self.vertices.cpu().numpy())
        return self._host

    def rings_of(self, label: int) -> np.ndarray:
        """The row indices of a region's rings, the outer ring first, then its holes in ring order."""
        r = self.numpy()[0]
        idx = np.flatnonzero(r[:, 0] == label)
        return idx[np.argsort(r[idx, 7], kind="stable")]

    def ring(self, i: int) -> np.ndarray:
        """int32 [nvert,2]: the vertices of ring i."""
        r, v = self.numpy()
        return v[r[i, 1]:r[i, 1] + r[i, 2]]

    def _select(self, label: int, max_n_holes, min_hole_area) -> np.ndarray:
        r = self.numpy()[0]
        idx = self.rings_of(label)
        outer, holes = idx[r[idx, 7] == 0], idx[r[idx, 7] == 1]
        holes = holes[-r[holes, 4] >= 2 * min_hole_area]
        if max_n_holes is not None:
            if _integer(max_n_holes, "max_n_holes") < 0:
                raise ValueError(f"max_n_holes must be >= 0, got {max_n_holes}")
            holes = np.sort(holes[np.argsort(r[holes, 4], kind="stable")[:max_n_holes]])      # area2 < 0: ascending = the largest first
        return np.concatenate([outer, holes])

    def polygons(self, label: int, max_n_holes: Optional[int] = None, min_hole_area=0) -> List[np.ndarray]:
        """The region as a list of int32 ``[k,2]`` arrays: the outer ring, then the holes (in ring order).  ``min_hole_area`` keeps a
        hole iff ``|area2| >= 2 min_hole_area``; of those ``max_n_holes`` keeps the largest by ``|area2|`` (CLAM's cut; ties go to the
        earlier ring)."""
        return [self.ring(i) for i in self._select(label, max_n_holes, min_hole_area)]

    def n_holes(self) -> np.ndarray:
        """int64 [n]: the number of hole rings of every region."""
        r = self.numpy()[0]
        lab = r[r[:, 7] == 1, 0]
        return np.bincount(lab, minlength=self.n + 1)[1:self.n + 1].astype(np.int64)

    def perimeter(self) -> np.ndarray:
        """int64 [n]: ``nedge`` of every region's outer ring, the outer perimeter in pixel sides (0 for a label without pixels)."""
        r = self.numpy()[0]
        out = np.zeros(self.n + 1, np.int64)
        o = r[r[:, 7] == 0]
        out[o[:, 0]] = o[:, 3]
        return out[1:]

    def area(self) -> np.ndarray:
        """int64 [n]: every region's pixel count, half the sum of its rings' ``area2``."""
        r = self.numpy()[0]
        out = np.zeros(self.n + 1, np.int64)
        np.add.at(out, r[:, 0], r[:, 4])
        return out[1:] // 2

    def to_level0(self) -> np.ndarray:
        """int64 [V,2]: the vertices as ``origin + downsample * v``.  Exact in integers: a lattice corner has no half-pixel offset."""
        if self.downsample is None:
            raise ValueError("these outlines have no downsample: trace a RegionTable made from a TissueMask or a raster")
        return self.numpy()[1].astype(np.int64) * int(self.downsample) + np.asarray(self.origin, np.int64)

    def to_geojson(self, table: Optional[RegionTable] = None, level0: bool = True, max_n_holes: Optional[int] = None, min_hole_area=0,
                   shape=None) -> dict:
        """A GeoJSON ``FeatureCollection`` (a dict that ``json.dumps`` takes): one ``Polygon`` feature per region that has pixels, in
        label order; its exterior ring first, then the holes that ``max_n_holes`` / ``min_hole_area`` keep (see :meth:`polygons`),
        every ring closed by repeating its first point.  Coordinates are level-0 pixels (``level0=True``, needs a downsample) or mask
        pixels.  ``properties``: ``label``, ``area`` (mask pixels), ``n_holes`` (all of the region's holes, cut or not), ``perimeter``
        (the outer ring's, in pixel sides); with the region's ``RegionTable`` also ``mean_score``, ``peak_score`` (None where no pixel
        is covered) and ``border``; with the regions' ``keep_amd.morphometry.RegionShape`` (``shape=``, made with its Feret columns)
        also ``major_axis``, ``minor_axis``, ``feret`` and ``feret_line`` (the two end points of the largest diameter), in the units of
        the coordinates.  Rings keep the orientation of the trace (region on the right with y down).  Under connectivity 8
        a ring that passes through a diagonal contact touches itself at that vertex; such pinched rings are left as they are, and a
        strict OGC validator may call them self-touching."""
        r, v = self.numpy()
        pts = self.to_level0() if level0 else v.astype(np.int64)
        if table is not None:
            if not isinstance(table, RegionTable) or table.n != self.n:
                raise ValueError(f"table must be the RegionTable of these {self.n} regions")
            by_label = np.argsort(table.ids.cpu().numpy(), kind="stable")          # a table that sort() permuted still names its labels
            mean, peak = table.mean_score()[by_label], table.peak_score()[by_label]
            border, covered = (table.numpy()[by_label, TABLE_COLUMNS.index(c)] for c in ("border", "covered"))
        if shape is not None:
            from .morphometry import RegionShape
            if not isinstance(shape, RegionShape) or shape.n != self.n or shape.feret is None:
                raise ValueError(f"shape must be the RegionShape of these {self.n} regions, made with feret=True")
            if level0:
                sh = shape.to_level0()
                axes, feret, line = sh["axis_lengths"], sh["feret"], shape.feret_points() * int(shape.downsample) + np.asarray(shape.origin, np.int64)
            else:
                axes, feret, line = shape.axis_lengths(), shape.feret_diameter(), shape.feret_points()
        area, holes, perim = self.area(), self.n_holes(), self.perimeter()
        features = []
        for lab in range(1, self.n + 1):
            sel = self._select(lab, max_n_holes, min_hole_area)
            if len(sel) == 0:
                continue
            coords = []
            for i in sel:
                ring = pts[r[i, 1]:r[i, 1] + r[i, 2]].tolist()
                coords.append(ring + [ring[0]])
            props = {"label": lab, "area": int(area[lab - 1]), "n_holes": int(holes[lab - 1]), "perimeter": int(perim[lab - 1])}
            if table is not None:
                props["mean_score"] = float(mean[lab - 1]) if covered[lab - 1] > 0 else None
                props["peak_score"] = float(peak[lab - 1]) if covered[lab - 1] > 0 else None
                props["border"] = int(border[lab - 1])
            if shape is not None:
                props["major_axis"], props["minor_axis"] = float(axes[lab - 1, 0]), float(axes[lab - 1, 1])
                props["feret"], props["feret_line"] = float(feret[lab - 1]), line[lab - 1].tolist()
            features.append({"type": "Feature", "properties": props, "geometry": {"type": "Polygon", "coordinates": coords}})
        return {"type": "FeatureCollection", "features": features}


# ------------------------------------------------------------------------------------------------ the restatements
def _clean(labels, n) -> Tuple[np.ndarray, int]:
    lab = np.asarray(labels)
    if lab.ndim != 2 or lab.dtype != np.int32 or lab.size < 1 or lab.size > MAX_PIXELS:
        raise ValueError(f"labels must be int32 [h, w] with 1 <= h * w <= 2^28, got {lab.dtype} {lab.shape}")
    n = max(int(lab.max()), 0) if n is None else _integer(n, "n")
    if n < 0:
        raise ValueError(f"n must be >= 0, got {n}")
    return np.where((lab >= 1) & (lab <= n), lab, 0).astype(np.int64), n


def outlines_numpy(labels, connectivity: int = 8, n: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The outlines restated on the host -> (rings int64 [R,8], vertices int32 [V,2]).  ``n``: labels outside 1..n count as
    background (default: the largest label).  The successor of every edge comes from the table of the specification (numpy over the
    four sides); the rings are then walked one after the other, edge by edge, in Python."""
    connectivity, _ = check_outline_args(connectivity)
    lab, n = _clean(labels, n)
    h, w = lab.shape
    P = np.pad(lab, 2)
    sh = lambda dx, dy: P[2 + dy:2 + dy + h, 2 + dx:2 + dx + w]                     # the label at (x + dx, y + dy), 0 outside
    pix = np.arange(h * w, dtype=np.int64).reshape(h, w)
    succ = np.full(4 * h * w, -1, np.int64)
    for s in range(4):
        dx, dy, nx, ny = _DX[s], _DY[s], _DX[(s + 3) % 4], _DY[(s + 3) % 4]
        edge = (lab > 0) & (sh(nx, ny) != lab)
        ar, al = sh(dx, dy) == lab, sh(dx + nx, dy + ny) == lab
        left = al & (ar | (connectivity == 8))
        straight = ar & ~left
        nxt = np.where(left, 4 * (pix + (dy + ny) * w + dx + nx) + (s + 3) % 4,
                       np.where(straight, 4 * (pix + dy * w + dx) + s, 4 * pix + (s + 1) % 4))
        succ[4 * pix[edge] + s] = nxt[edge]
    slots = np.flatnonzero(succ >= 0)
    assert np.array_equal(np.sort(succ[slots]), slots)                            # a permutation of the edges
    pred = np.full_like(succ, -1)
    pred[succ[slots]] = slots
    corner = np.zeros(len(succ), bool)
    corner[slots] = (pred[slots] & 3) != (slots & 3)
    nxt, is_corner, seen = succ.tolist(), corner.tolist(), bytearray(len(succ))
    found = []                                                                    # (leader slot, nedge, the corner slots from the leader on)
    for e0 in slots.tolist():
        if seen[e0]:
            continue
        cyc, e = [], e0
        while not seen[e]:
            seen[e] = 1
            cyc.append(e)
            e = nxt[e]
        cs = [c for c in cyc if is_corner[c]]
        k = cs.index(min(cs))
        found.append((cs[k], len(cyc), cs[k:] + cs[:k]))
    found.sort(key=lambda t: t[0])
    rings = np.zeros((len(found), NCOLS), np.int64)
    verts = []
    start = 0
    flat = lab.ravel()
    for i, (_, nedge, cs) in enumerate(found):
        c = np.asarray(cs, np.int64)
        p, s = c >> 2, c & 3
        x, y = p % w + ((s == 1) | (s == 2)), p // w + (s >= 2)
        area2 = int(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))
        rings[i] = flat[p[0]], start, len(c), nedge, area2, x[0], y[0], area2 < 0
        verts.append(np.stack([x, y], axis=1))
        start += len(c)
    vertices = (np.concatenate(verts) if verts else np.zeros((0, 2), np.int64)).astype(np.int32)
    return rings, vertices


def draw_numpy(rgb, labels, color=(0, 0, 0), width: int = 1) -> np.ndarray:
    """The outline drawn on the host -> a new uint8 [h,w,3]: ``out[p] = color`` iff ``labels[p] = l > 0`` and some pixel of the
    ``(2 width + 1)^2`` window round p lies outside the image or has a label ``!= l``; ``rgb[p]`` elsewhere."""
    packed, width = check_draw_args(color, width)
    lab = np.asarray(labels)
    img = np.asarray(rgb)
    if lab.ndim != 2 or lab.dtype != np.int32 or img.dtype != np.uint8 or img.shape != lab.shape + (3,):
        raise ValueError(f"need int32 [h, w] labels and a uint8 [h, w, 3] image, got {lab.dtype} {lab.shape} and {img.dtype} {img.shape}")
    h, w = lab.shape
    P = np.pad(lab.astype(np.int64), width)                                       # 0 outside: never a label > 0
    same = np.ones((h, w), bool)
    for dy in range(2 * width + 1):
        for dx in range(2 * width + 1):
            same &= P[dy:dy + h, dx:dx + w] == lab
    out = img.copy()
    out[(lab > 0) & ~same] = (packed & 255, packed >> 8 & 255, packed >> 16 & 255)
    return out
