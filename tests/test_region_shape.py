"""Region shape, host side: keep_amd.morphometry.shape_numpy (the yardstick of
tests/test_region_shape_gpu.py) against per-pixel Python-integer loops, numpy's covariance, closed forms, a brute force over every
corner of every pixel and scipy's convex hull; RegionShape's conversions, the GeoJSON properties and the argument checks.  No GPU."""
import math

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel
from keep_amd.components import COLUMNS, NCOLS, RegionTable, regions_numpy
from keep_amd.lesion import camelyon16_margin
from keep_amd.morphometry import (DEFAULT_MAX_PAIRS, FERET_COLUMNS, MOMENT_COLUMNS, RegionShape, camelyon16_itc_axis, check_shape_args,
                                  shape_numpy)
from keep_amd.outline import RegionOutlines, outlines_numpy
from keep_amd.region import TissueMask
from test_regions import MASKS

COL = {name: i for i, name in enumerate(COLUMNS)}


def table_of(labels, n):
    """The geometry columns of the region table of a caller's label image, by numpy per label."""
    t = np.zeros((n, NCOLS), np.int64)
    for l in range(1, n + 1):
        ys, xs = np.nonzero(labels == l)
        if len(xs):
            t[l - 1, :9] = xs[0], ys[0], len(xs), xs.min(), ys.min(), xs.max() + 1, ys.max() + 1, xs.sum(), ys.sum()
    return t


def host_shape(labels, table, downsample=None, origin=(0, 0), feret=True) -> RegionShape:
    m, f = shape_numpy(labels, table, feret)
    regs = RegionTable(torch.from_numpy(table), torch.from_numpy(np.ascontiguousarray(labels, np.int32)), downsample, origin)
    return RegionShape(torch.from_numpy(m), None if f is None else torch.from_numpy(f), regs)


def brute_feret(labels, l, w):
    """(d2, ax, ay, bx, by) straight from the definition: every pair of corners of the pixels of label l, with the tie rule."""
    ys, xs = np.nonzero(labels == l)
    pts = sorted({(y + dy, x + dx) for y, x in zip(ys.tolist(), xs.tolist()) for dy in (0, 1) for dx in (0, 1)})
    best = (-1, 0, 0)
    for i, (ay, ax) in enumerate(pts):                                       # ascending lattice order: the first maximal pair wins
        for by, bx in pts[i + 1:]:
            d2 = (ax - bx) ** 2 + (ay - by) ** 2
            if d2 > best[0]:
                best = (d2, (ay, ax), (by, bx))
    return [best[0], best[1][1], best[1][0], best[2][1], best[2][0]], np.array([(x, y) for y, x in pts])


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name,img", MASKS, ids=[n for n, _ in MASKS])
def test_moments_match_per_pixel_loops(name, img, connectivity):
    labels, table = regions_numpy(img, connectivity, 1)
    got, none = shape_numpy(labels, table, feret=False)
    assert none is None and got.dtype == np.int64 and got.shape == (len(table), 3)
    want = [[0, 0, 0] for _ in range(len(table))]
    x0, y0 = table[:, COL["x0"]].tolist(), table[:, COL["y0"]].tolist()
    for y, row in enumerate(labels.tolist()):
        for x, l in enumerate(row):
            if l:
                u, v = x - x0[l - 1], y - y0[l - 1]
                r = want[l - 1]
                r[0] += u * u; r[1] += v * v; r[2] += u * v
    assert got.tolist() == want


@pytest.mark.parametrize("name,img", MASKS, ids=[n for n, _ in MASKS])
def test_central_moments_match_numpy_cov(name, img):
    """Tolerance: a relative 1e-12 of the covariance matrix's largest entry -- the float64 conversion of exact integers on one side,
    np.cov's own float64 mean and products on the other; not a kernel tolerance.  A covariance of zeros compares exactly."""
    labels, table = regions_numpy(img, 8, 1)
    sh = host_shape(labels, table, feret=False)
    got = sh.central_moments()
    assert got.shape == (len(table), 3)
    p = np.flatnonzero(labels.ravel())
    p = p[np.argsort(labels.ravel()[p], kind="stable")]                       # every region's pixels, region after region
    ends = np.cumsum(table[:, COL["area"]])
    for l, (a, b) in enumerate(zip(np.r_[0, ends[:-1]].tolist(), ends.tolist())):
        c = np.cov(np.stack([p[a:b] % labels.shape[1], p[a:b] // labels.shape[1]]).astype(np.float64), bias=True)
        want = np.array([c[0, 0], c[1, 1], c[0, 1]])
        assert np.abs(got[l] - want).max() <= 1e-12 * np.abs(want).max(), (l, got[l], want)


@pytest.mark.parametrize("w,h", [(37, 5), (5, 37)])
def test_rectangle_axis_lengths(w, h):
    img = np.zeros((h + 4, w + 6), np.uint8)
    img[2:2 + h, 3:3 + w] = 1
    sh = host_shape(*regions_numpy(img, 8, 1))
    a, b = 4 * math.sqrt((w * w - 1) / 12), 4 * math.sqrt((h * h - 1) / 12)
    assert sh.axis_lengths().tolist() == [[max(a, b), min(a, b)]]
    assert abs(sh.eccentricity()[0] - math.sqrt(1 - (min(w, h) ** 2 - 1) / (max(w, h) ** 2 - 1))) < 1e-15
    assert sh.orientation()[0] == (0.0 if w > h else math.pi / 2)
    assert sh.d2.tolist() == [w * w + h * h] and sh.feret_points().tolist() == [[[3, 2], [3 + w, 2 + h]]]
    assert sh.feret_diameter()[0] == math.sqrt(w * w + h * h)


def test_one_pixel_region():
    img = np.zeros((5, 9), np.uint8)
    img[3, 7] = 1
    sh = host_shape(*regions_numpy(img, 8, 1))
    assert sh.axis_lengths().tolist() == [[0.0, 0.0]] and sh.eccentricity().tolist() == [0.0]
    assert sh.feret.tolist() == [[2, 7, 3, 8, 4]] and sh.moments.tolist() == [[0, 0, 0]]
    assert [tuple(c) for c in (MOMENT_COLUMNS, FERET_COLUMNS)] == [("sum_uu", "sum_vv", "sum_uv"), ("d2", "ax", "ay", "bx", "by")]
    assert torch.equal(sh.sum_uu, sh.moments[:, 0]) and torch.equal(sh.by, sh.feret[:, 4])


@pytest.mark.parametrize("connectivity", [4, 8])
def test_feret_matches_brute_force_and_convex_hull(connectivity):
    spatial = pytest.importorskip("scipy.spatial")
    g = np.random.default_rng(11 + connectivity)
    seen_rows = seen_cols = hulls = 0
    for h, w, density in [(23, 31, 0.5), (31, 23, 0.55), (40, 40, 0.62), (9, 40, 0.7), (40, 7, 0.7)]:
        for _ in range(3):
            img = (g.random((h, w)) < density).astype(np.uint8)
            labels, table = regions_numpy(img, connectivity, 1)
            feret = shape_numpy(labels, table)[1]
            bw, bh = table[:, COL["x1"]] - table[:, COL["x0"]], table[:, COL["y1"]] - table[:, COL["y0"]]
            seen_rows, seen_cols = seen_rows + int((bh < bw).sum()), seen_cols + int((bh > bw).sum())
            for l in range(1, len(table) + 1):
                want, pts = brute_feret(labels, l, w)
                assert feret[l - 1].tolist() == want, (h, w, l)
                v = pts[spatial.ConvexHull(pts).vertices].astype(np.int64)   # a pixel's four corners already span a hull: no region is degenerate
                assert int((((v[:, None] - v[None]) ** 2).sum(-1)).max()) == want[0]
                hulls += 1
    assert seen_rows > 5 and seen_cols > 5 and hulls > 40          # both the row and the column choice were taken


@pytest.mark.parametrize("k", [1, 2, 7, 16])
def test_tie_rule_on_a_square(k):
    img = np.zeros((k + 3, k + 5), np.uint8)
    img[:k, :k] = 1
    img[k + 1:, k + 2:] = 1                                                 # a second region, so that the lattice is wider than the square
    sh = host_shape(*regions_numpy(img, 4, 1))
    assert sh.feret[0].tolist() == [2 * k * k, 0, 0, k, k]                  # not (k, 0) - (0, k)


def test_callers_labels_with_an_empty_row():
    labels = np.zeros((12, 20), np.int32)
    labels[1, 2:9] = labels[2, 4:6] = labels[5, 3:18] = labels[6, 10] = 1     # rows 3 and 4 of the box carry nothing
    labels[0:3, 15] = labels[8:11, 15] = labels[8, 16:19] = 3                 # columns and rows missing; label 2 is carried by nobody
    labels[11, 0] = 9                                                         # above n: background
    table = table_of(labels, 3)
    moments, feret = shape_numpy(labels, table)
    assert moments[1].tolist() == [0, 0, 0] and feret[1].tolist() == [0] * 5
    for l in (1, 3):
        assert feret[l - 1].tolist() == brute_feret(labels, l, 20)[0]
    ys, xs = np.nonzero(labels == 3)
    assert moments[2].tolist() == [int(((xs - 15) ** 2).sum()), int((ys ** 2).sum()), int(((xs - 15) * ys).sum())]


def test_trailing_labels_that_nobody_carries():
    """The last labels empty, and empty labels in a row: every carried label keeps all of its pixels."""
    labels = np.zeros((6, 9), np.int32)
    labels[1, 1:5] = 1
    labels[2, 0:6] = 2
    labels[4, 3:9] = labels[5, 8] = 5                                          # 3 and 4 are carried by nobody, nor are 6 and 7
    table = table_of(labels, 7)
    moments, feret = shape_numpy(labels, table)
    want = np.zeros((7, 3), np.int64)
    for y, x in zip(*np.nonzero(labels)):
        l = labels[y, x] - 1
        u, v = x - table[l, COL["x0"]], y - table[l, COL["y0"]]
        want[l] += u * u, v * v, u * v
    assert moments.tolist() == want.tolist() and moments[1].tolist() == [55, 0, 0] and moments[4].tolist() == [55 + 25, 1, 5]
    for l in range(1, 8):
        assert feret[l - 1].tolist() == (brute_feret(labels, l, 9)[0] if l in (1, 2, 5) else [0] * 5)
    only_first = shape_numpy(labels * (labels == 1), table[:3])
    assert only_first[0].tolist() == [want[0].tolist(), [0] * 3, [0] * 3] and only_first[1][1:].tolist() == [[0] * 5] * 2


def test_units_size_class_and_the_camelyon_threshold():
    assert camelyon16_itc_axis() == 275 / (0.243 * 32) and abs(camelyon16_itc_axis() - 35.4) < 0.05
    assert camelyon16_itc_axis(0.5, 16) == 275 / 8.0 and camelyon16_margin() * 2 * 275 / 75 == pytest.approx(camelyon16_itc_axis())
    img = np.zeros((40, 90), np.uint8)
    img[0, 0:3] = img[2, 0:4] = img[4, 0:39] = img[6, 0:40] = img[8, 0:41] = 1
    sh = host_shape(*regions_numpy(img, 4, 1), downsample=5, origin=(100, 200))
    # Feret diameters sqrt(len^2 + 1) mask pixels; at downsample 5 and mpp 10 one mask pixel is 50 um
    d = np.sqrt(np.array([3, 4, 39, 40, 41]) ** 2 + 1.0)
    assert sh.feret_diameter().tolist() == d.tolist()
    assert sh.to_level0()["feret"].tolist() == (d * 5).tolist() and sh.to_um(10.0)["feret"].tolist() == (d * 5 * 10.0).tolist()
    assert sh.to_level0()["feret_points"][2].tolist() == [[100.0, 220.0], [100 + 39 * 5.0, 225.0]]
    assert np.array_equal(sh.to_level0()["axis_lengths"], sh.axis_lengths() * 5)
    cls = sh.size_class(10.0)
    assert cls.dtype == np.int8 and cls.tolist() == [0, 1, 1, 2, 2]            # 158 um, 206 um, 1951 um, 2001 um, 2051 um
    assert sh.size_class(10.0, itc_um=d[1] * 50, macro_um=d[3] * 50).tolist() == [0, 1, 1, 1, 2]      # at the thresholds themselves: micro
    assert sh.size_class(10.0, itc_um=np.nextafter(d[1] * 50, 1e9), macro_um=np.nextafter(d[3] * 50, 0)).tolist() == [0, 0, 1, 2, 2]
    with pytest.raises(ValueError):
        host_shape(*regions_numpy(img, 4, 1)).to_level0()                      # no downsample
    with pytest.raises(ValueError):
        host_shape(*regions_numpy(img, 4, 1), downsample=5, feret=False).size_class(10.0)


def test_geojson_properties():
    img = np.zeros((20, 30), np.uint8)
    img[2:9, 3:25] = img[12:18, 5:9] = 1
    img[4:6, 8:12] = 0
    labels, table = regions_numpy(img, 8, 1)
    rings, vertices = outlines_numpy(labels, 8, len(table))
    out = RegionOutlines(torch.from_numpy(rings), torch.from_numpy(vertices), 4, (8, 16), len(table))
    regs = RegionTable(torch.from_numpy(table), torch.from_numpy(labels), 4, (8, 16))
    sh = host_shape(labels, table, 4, (8, 16))
    for level0 in (True, False):
        plain = out.to_geojson(regs, level0=level0)
        assert out.to_geojson(regs, level0=level0, shape=None) == plain
        with_shape = out.to_geojson(regs, level0=level0, shape=sh)
        assert len(with_shape["features"]) == len(plain["features"]) == 2
        for a, b, i in zip(with_shape["features"], plain["features"], range(2)):
            assert a["geometry"] == b["geometry"]
            extra = {k: v for k, v in a["properties"].items() if k not in b["properties"]}
            assert sorted(extra) == ["feret", "feret_line", "major_axis", "minor_axis"]
            assert {k: v for k, v in a["properties"].items() if k in b["properties"]} == b["properties"]
            s = 4 if level0 else 1
            assert extra["major_axis"] == sh.axis_lengths()[i, 0] * s and extra["minor_axis"] == sh.axis_lengths()[i, 1] * s
            assert extra["feret"] == sh.feret_diameter()[i] * s
            p = sh.feret_points()[i]
            assert extra["feret_line"] == ((p * 4 + np.array([8, 16])) if level0 else p).tolist()
    assert with_shape["features"][0]["properties"]["feret_line"] == [[3, 2], [25, 9]]
    with pytest.raises(ValueError):
        out.to_geojson(regs, shape=host_shape(labels, table, 4, (8, 16), feret=False))
    with pytest.raises(ValueError):
        out.to_geojson(regs, shape=host_shape(labels[:, :5] * 0, table[:0]))


def test_value_errors():
    assert check_shape_args(32768, 32768) == DEFAULT_MAX_PAIRS                  # a 32768 x 32768 mask passes
    assert check_shape_args(1, 1, True, 0) == 0
    for h, w in [(1 << 17, 1 << 17), (1 << 10, 1 << 20), (32768, 65536), (32768, 32769), (0, 5), (5, -1)]:      # h w <= 2^30 as the entry points ask
        with pytest.raises(ValueError):
            check_shape_args(h, w, False)
    with pytest.raises(ValueError):
        check_shape_args(1, 1 << 30)                                            # the lattice bound too, but the moments' bound comes first
    for bad in (-1, (1 << 50) + 1, 2.5):
        with pytest.raises(ValueError):
            check_shape_args(10, 10, True, bad)
    model = KEEPModel()                                                         # every check below comes before any device call
    img = np.ones((6, 9), np.uint8)
    labels, table = regions_numpy(img, 8, 1)
    with pytest.raises(ValueError, match="labels"):
        model.region_shape(RegionTable(torch.from_numpy(table)))
    with pytest.raises(ValueError):
        model.region_shape(labels)
    regs = RegionTable(torch.from_numpy(table), torch.from_numpy(labels))
    assert regs.label_order and not regs.sort("area").label_order
    with pytest.raises(ValueError, match="label order"):
        model.region_shape(regs.sort("area"))
    with pytest.raises(ValueError):
        model.region_shape(RegionTable(torch.from_numpy(table), torch.from_numpy(labels)), max_pairs=-3)
    empty = model.region_shape(RegionTable(torch.zeros((0, NCOLS), dtype=torch.int64), torch.zeros((6, 9), dtype=torch.int32)))
    assert empty.n == 0 and tuple(empty.moments.shape) == (0, 3) and tuple(empty.feret.shape) == (0, 5) and empty.axis_lengths().shape == (0, 2)
    with pytest.raises(ValueError, match="not both"):
        model.evaluation_mask(TissueMask(img, 4), 2.0, ignore_max_extent=8, ignore_major_axis=8.0)
    with pytest.raises(ValueError):
        model.evaluation_mask(TissueMask(img, 4), 2.0, ignore_major_axis=-1.0)
    with pytest.raises(ValueError):
        RegionShape(torch.zeros((2, 3), dtype=torch.int64), None, RegionTable(torch.from_numpy(table)))
    with pytest.raises(ValueError):
        shape_numpy(labels, table[:, :5])
