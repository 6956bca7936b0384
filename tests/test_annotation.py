"""Polygon annotations to masks, host side: keep_amd.annotation.fill_numpy / tile_counts_numpy (the yardsticks
of tests/test_annotation_gpu.py) held to statements that fill nothing (a brute-force crossing count per pixel in fractions, the label
image an outline came from, closed forms), the rules, clipping, the GeoJSON and ASAP XML readers and the argument checks.  Every
comparison is exact.  No GPU."""
import itertools
import json
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from keep_amd import _lib
from keep_amd.annotation import (CAMELYON16_ORDER, PolygonSet, check_fill_args, check_rings, check_tile_args, fill_numpy,
                                 tile_counts_numpy)
from keep_amd.components import regions_numpy
from keep_amd.outline import RegionOutlines, outlines_numpy
from keep_amd.region import TissueMask
from test_regions import MASKS

RULES = ("union", "evenodd")


# ------------------------------------------------------------------------------------------------ shared with the GPU tests
def random_polygon_sets(count=30, seed=11):
    """(vertices, ring_start, weight, d, (h, w), origin): 1-3 rings of 3-8 vertices, self-intersections allowed, weights +-1, shapes up
    to 13 x 13, d in {1, 2, 3, 16}, non-zero origins; every other set sits on a lattice of d / 2 (d for an odd d) from the origin, so
    that vertices and edges hit pixel centres."""
    g = np.random.default_rng(seed)
    out = []
    for k in range(count):
        d = (1, 2, 3, 16)[k % 4]
        h, w = int(g.integers(1, 14)), int(g.integers(1, 14))
        origin = (int(g.integers(-40, 40)) or 7, int(g.integers(-40, 40)) or -5)
        rings = []
        for _ in range(int(g.integers(1, 4))):
            n = int(g.integers(3, 9))
            if (k // 4) % 2:
                step = d // 2 if d % 2 == 0 else d
                pts = np.stack([g.integers(-2 * d // step, (w + 2) * d // step + 1, n), g.integers(-2 * d // step, (h + 2) * d // step + 1, n)], 1) * step
            else:
                pts = np.stack([g.integers(-2 * d, (w + 2) * d + 1, n), g.integers(-2 * d, (h + 2) * d + 1, n)], 1)
            rings.append(pts.astype(np.int64) + np.asarray(origin, np.int64))
        start = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int64)
        weight = g.choice(np.array([-1, 1], np.int32), len(rings))
        out.append((np.concatenate(rings), start, weight, d, (h, w), origin))
    return out


_OUTLINES = {}


def outline_polygons(img, connectivity, d, origin=(0, 0)):
    """A mask -> (labels int32, n, the PolygonSet of its regions' outlines on level-0 coordinates); the trace is made once per mask."""
    key = (img.tobytes(), img.shape, connectivity)
    if key not in _OUTLINES:
        labels, table = regions_numpy(img, connectivity, 1)
        _OUTLINES[key] = (labels, len(table), outlines_numpy(labels, connectivity, len(table)))
    labels, n, (rings, vertices) = _OUTLINES[key]
    o = RegionOutlines(torch.from_numpy(rings), torch.from_numpy(vertices), d, origin, n)
    return labels, n, PolygonSet.from_outlines(o)


def rect(x0, y0, x1, y1, clockwise=True):
    pts = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    return np.array(pts if clockwise else pts[::-1], np.int64)


def poly_set(*rings, roles=None, features=None):
    start = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int64)
    return PolygonSet(np.concatenate(rings), start, features, roles)


# ------------------------------------------------------------------------------------------------ brute force
def brute_force(vertices, ring_start, weight, d, shape, origin, rule):
    """Every pixel on its own: the edges that cross the horizontal line through its centre on or left of the centre, in fractions."""
    h, w = shape
    out = np.zeros((h, w), np.uint8)
    pts = vertices.tolist()
    for i in range(h):
        cy = origin[1] + Fraction(2 * i + 1, 2) * d
        for j in range(w):
            cx = origin[0] + Fraction(2 * j + 1, 2) * d
            wind = 0
            for r in range(len(ring_start) - 1):
                ring = pts[ring_start[r]:ring_start[r + 1]]
                for (xa, ya), (xb, yb) in zip(ring, ring[1:] + ring[:1]):
                    if min(ya, yb) <= cy < max(ya, yb):
                        x = xa + (cy - ya) * Fraction(xb - xa, yb - ya)
                        if x <= cx:
                            wind += int(weight[r]) * (1 if yb < ya else -1)
            out[i, j] = wind % 2 if rule == "evenodd" else wind > 0
    return out


def test_fill_numpy_equals_the_brute_force_count():
    sets = random_polygon_sets()
    assert len(sets) == 30 and {s[3] for s in sets} == {1, 2, 3, 16}
    filled = 0
    for vertices, start, weight, d, shape, origin in sets:
        for rule in RULES:
            got = fill_numpy((vertices, start, weight), d, shape, origin, rule)
            assert got.dtype == np.uint8 and np.array_equal(got, brute_force(vertices, start, weight, d, shape, origin, rule))
            filled += int(got.sum())
    assert filled > 200                                           # the sweep is not a sweep of empty masks


# ------------------------------------------------------------------------------------------------ round trip
@pytest.mark.parametrize("name,img", MASKS, ids=[n for n, _ in MASKS])
def test_outlines_filled_give_the_mask_back(name, img):
    for connectivity, d, origin, rule in itertools.product((4, 8), (1, 3, 16), ((0, 0), (-48, 96)), RULES):
        labels, n, polys = outline_polygons(img, connectivity, d, origin)
        assert np.array_equal(fill_numpy(polys, d, img.shape, origin, rule), (labels > 0).astype(np.uint8))


@pytest.mark.parametrize("density", [0.3, 0.5, 0.65, 0.8])
def test_round_trip_on_random_masks_and_label_by_label(density):
    img = (np.random.default_rng(int(density * 100)).random((37, 53)) < density).astype(np.uint8)
    for connectivity, d, origin, rule in itertools.product((4, 8), (1, 3, 16), ((0, 0), (32, -16)), RULES):
        labels, n, polys = outline_polygons(img, connectivity, d, origin)
        assert np.array_equal(fill_numpy(polys, d, img.shape, origin, rule), (labels > 0).astype(np.uint8))
    for connectivity in (4, 8):                                   # 8: pinched rings among them
        labels, n, polys = outline_polygons(img, connectivity, 3, (32, -16))
        assert n >= 1 and (connectivity == 8 or n > 3)
        out = None
        for lab in range(1, min(n, 255) + 1):
            out = fill_numpy(polys.select(groups=[str(lab)]), 3, img.shape, (32, -16), "union", lab, out)
        assert np.array_equal(out, np.where(labels <= 255, labels, 0).astype(np.uint8))


# ------------------------------------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("r", [1, 2, 7, 20])
def test_diamond_fills_2_r_squared_pixels(r):
    c = r + 3
    diamond = np.array([(c, c - r), (c + r, c), (c, c + r), (c - r, c)], np.int64)
    for rule in RULES:
        got = fill_numpy(poly_set(diamond), 1, (2 * c, 2 * c), (0, 0), rule)
        assert int(got.sum()) == 2 * r * r
        i, j = np.indices(got.shape)
        dist = np.abs(2 * i + 1 - 2 * c) + np.abs(2 * j + 1 - 2 * c)   # doubled; a centre on the boundary is in on the left sides only
        assert np.array_equal(got.astype(bool), (dist < 2 * r) | ((dist == 2 * r) & (2 * j + 1 < 2 * c)))


def test_rectangle_on_multiples_of_d():
    for d, origin in ((1, (0, 0)), (4, (0, 0)), (16, (-32, 48))):
        want = np.zeros((9, 11), np.uint8)
        want[2:7, 3:10] = 1
        ring = rect(3 * d, 2 * d, 10 * d, 7 * d) + np.asarray(origin)
        for rule in RULES:
            assert np.array_equal(fill_numpy(poly_set(ring), d, (9, 11), origin, rule), want)


def test_sides_through_pixel_centres_left_and_top_in_right_and_bottom_out():
    # d = 2: the centres are the odd coordinates; the rectangle's sides run through the centres of columns 1, 4 and rows 2, 5
    got = fill_numpy(poly_set(rect(3, 5, 9, 11)), 2, (8, 8))
    want = np.zeros((8, 8), np.uint8)
    want[2:5, 1:4] = 1
    assert np.array_equal(got, want)
    assert np.array_equal(fill_numpy(poly_set(rect(3, 5, 9, 11, clockwise=False)), 2, (8, 8)), want)


def test_two_polygons_that_share_a_slanted_edge_partition_the_pixels():
    for d, (ax, ay), (bx, by) in ((1, (2, 0), (9, 14)), (2, (3, 1), (17, 15)), (2, (1, 1), (15, 15)), (3, (0, 3), (21, 18))):
        shape = (12, 12)
        left = np.array([(0, ay), (ax, ay), (bx, by), (0, by)], np.int64)
        right = np.array([(ax, ay), (40, ay), (40, by), (bx, by)], np.int64)
        merged = np.array([(0, ay), (40, ay), (40, by), (0, by)], np.int64)
        for rule in RULES:
            a, b = fill_numpy(poly_set(left), d, shape, (0, 0), rule), fill_numpy(poly_set(right), d, shape, (0, 0), rule)
            assert a.any() and b.any() and not (a & b).any()
            assert np.array_equal(a | b, fill_numpy(poly_set(merged), d, shape, (0, 0), rule))
            assert np.array_equal(a | b, fill_numpy(poly_set(left, right), d, shape, (0, 0), "union"))


# ------------------------------------------------------------------------------------------------ rules
def test_union_unites_and_evenodd_leaves_out_the_overlap():
    a, b = np.zeros((10, 10), np.uint8), np.zeros((10, 10), np.uint8)
    a[1:6, 1:6] = 1
    b[3:9, 4:9] = 1
    polys = poly_set(rect(1, 1, 6, 6), rect(4, 3, 9, 9, clockwise=False))
    assert np.array_equal(fill_numpy(polys, 1, (10, 10), rule="union"), a | b)
    assert np.array_equal(fill_numpy(polys, 1, (10, 10), rule="evenodd"), a ^ b)
    assert polys.weights("union").tolist() == [1, -1] and polys.weights("evenodd").tolist() == [1, 1]   # the weight undoes the direction
    assert polys.area2().tolist() == [50, -60]


def test_a_hole_does_not_punch_through_another_feature():
    frame_with_hole = (rect(0, 0, 10, 10), rect(3, 3, 7, 7, clockwise=False))
    other = rect(2, 4, 8, 6)
    polys = poly_set(*frame_with_hole, other, roles=[1, -1, 1], features=[0, 0, 1])
    assert polys.weights("union").tolist() == [1, 1, 1]           # role * sign(area2): a hole drawn against its exterior keeps its direction
    want = np.ones((10, 10), np.uint8)
    want[3:7, 3:7] = 0
    want[4:6, 2:8] = 1
    assert np.array_equal(fill_numpy(polys, 1, (10, 10)), want)
    alone = poly_set(*frame_with_hole, roles=[1, -1], features=[0, 0])
    want[4:6, 3:7] = 0
    assert np.array_equal(fill_numpy(alone, 1, (10, 10)), want)
    # a hole drawn in the exterior's direction is still a hole
    same_way = poly_set(rect(0, 0, 10, 10), rect(3, 3, 7, 7), roles=[1, -1], features=[0, 0])
    assert same_way.weights("union").tolist() == [1, -1]
    assert np.array_equal(fill_numpy(same_way, 1, (10, 10)), want)


def test_drawing_direction_does_not_matter_under_union_and_zero_area_counts_nothing():
    g = np.random.default_rng(5)
    ring = np.array([(1, 1), (12, 2), (9, 6), (13, 11), (4, 12), (6, 6)], np.int64)
    a = fill_numpy(poly_set(ring), 1, (14, 14))
    assert a.sum() > 40 and np.array_equal(a, fill_numpy(poly_set(ring[::-1].copy()), 1, (14, 14)))
    flat = poly_set(np.array([(0, 0), (5, 5), (10, 10)], np.int64))
    assert flat.weights("union").tolist() == [0] and not fill_numpy(flat, 1, (12, 12)).any()


def test_into_paints_in_order_and_value_0_cuts():
    base = fill_numpy(poly_set(rect(1, 1, 9, 9)), 1, (10, 10), value=200)
    keep = base.copy()
    cut = fill_numpy(poly_set(rect(3, 3, 6, 6)), 1, (10, 10), value=0, into=base)
    want = np.zeros((10, 10), np.uint8)
    want[1:9, 1:9] = 200
    assert np.array_equal(base, keep) and np.array_equal(base, want)       # into is not written
    want[3:6, 3:6] = 0
    assert np.array_equal(cut, want)
    over = fill_numpy(poly_set(rect(0, 0, 4, 4)), 1, (10, 10), value=255, into=torch.from_numpy(cut))
    want[0:4, 0:4] = 255
    assert np.array_equal(over, want)


# ------------------------------------------------------------------------------------------------ clipping
def test_polygons_outside_the_image_and_one_that_covers_it():
    d, shape, origin = 4, (6, 9), (100, -40)
    x0, y0, x1, y1 = origin[0], origin[1], origin[0] + 9 * d, origin[1] + 6 * d
    for ring in (rect(x0 - 50, y0, x0 - 10, y1), rect(x1 + 10, y0, x1 + 90, y1), rect(x0, y0 - 30, x1, y0 - 5), rect(x0, y1 + 5, x1, y1 + 60),
                 rect(x0 - 50, y0 - 50, x0, y0), rect(x1, y0, x1 + 3, y1)):
        for rule in RULES:
            assert not fill_numpy(poly_set(ring), d, shape, origin, rule).any()
    for rule in RULES:
        assert fill_numpy(poly_set(rect(x0 - 999, y0 - 999, x1 + 999, y1 + 999)), d, shape, origin, rule).all()
    # a polygon that sticks out on every side keeps only what is inside
    tri = np.array([(x0 - 20, y0 - 20), (x1 + 60, y0 - 20), (x0 - 20, y1 + 60)], np.int64)
    got = fill_numpy(poly_set(tri), d, shape, origin)
    big = fill_numpy(poly_set(tri), d, (40, 40), (origin[0] - 40, origin[1] - 40))
    assert np.array_equal(got, big[10:16, 10:19]) and got.any()


def test_one_row_and_one_column():
    ring = np.array([(2, -3), (9, 2), (4, 5), (-2, 1)], np.int64)
    full = fill_numpy(poly_set(ring), 1, (7, 11), (-1, -2))
    assert np.array_equal(fill_numpy(poly_set(ring), 1, (1, 11), (-1, 1)), full[3:4])
    assert np.array_equal(fill_numpy(poly_set(ring), 1, (7, 1), (4, -2)), full[:, 5:6])
    assert fill_numpy(poly_set(ring), 1, (1, 1), (4, 1)).tolist() == [[int(full[3, 5])]] and full[3, 5] == 1


# ------------------------------------------------------------------------------------------------ readers
def test_geojson_of_the_outlines_round_trips_holes_included():
    img = MASKS[[n for n, _ in MASKS].index("rings")][1]
    labels, table = regions_numpy(img, 8, 1)
    rings, vertices = outlines_numpy(labels, 8, len(table))
    assert (rings[:, 7] == 1).any()                               # there are holes
    o = RegionOutlines(torch.from_numpy(rings), torch.from_numpy(vertices), 16, (64, 32), len(table))
    polys = PolygonSet.from_geojson(json.loads(json.dumps(o.to_geojson())))
    direct = PolygonSet.from_outlines(o)
    assert polys.n_features == len(table) and polys.skipped == 0 and polys.group == [str(l) for l in range(1, len(table) + 1)]
    assert np.array_equal(polys.vertices, direct.vertices) and np.array_equal(polys.role, direct.role)
    for rule in RULES:
        assert np.array_equal(fill_numpy(polys, 16, img.shape, (64, 32), rule), (labels > 0).astype(np.uint8))
    assert np.array_equal(fill_numpy(PolygonSet.from_geojson(json.dumps(o.to_geojson())), 16, img.shape, (64, 32)), (labels > 0).astype(np.uint8))
    one = PolygonSet.from_outlines(o, labels=[2])
    assert one.n_features == 1 and np.array_equal(fill_numpy(one, 16, img.shape, (64, 32)), (labels == 2).astype(np.uint8))


def test_geojson_forms():
    square = [[2, 1], [6, 1], [6, 4], [2, 4]]
    want = np.zeros((6, 8), np.uint8)
    want[1:4, 2:6] = 1
    geometry = {"type": "Polygon", "coordinates": [square + [square[0]]]}
    forms = [geometry, {"type": "Polygon", "coordinates": [square]}, {"type": "Feature", "properties": None, "geometry": geometry},
             {"type": "FeatureCollection", "features": [{"type": "Feature", "properties": {}, "geometry": geometry}]},
             [{"type": "Feature", "properties": {}, "geometry": geometry}], json.dumps(geometry)]
    for form in forms:
        p = PolygonSet.from_geojson(form)
        assert len(p) == 1 and p.vertices.tolist() == square and p.group == [""] and p.skipped == 0
        assert np.array_equal(fill_numpy(p, 1, (6, 8)), want)
    multi = PolygonSet.from_geojson({"type": "MultiPolygon", "coordinates": [[square, [[3, 2], [5, 2], [5, 3], [3, 3]]], [[[0, 5], [3, 5], [3, 6], [0, 6]]]]})
    assert multi.n_features == 1 and multi.feature.tolist() == [0, 0, 0] and multi.role.tolist() == [1, -1, 1]
    want[2, 3:5] = 0
    want[5, 0:3] = 1
    assert np.array_equal(fill_numpy(multi, 1, (6, 8)), want)
    # floats: floor(v + 0.5), so x.5 goes up and -x.5 goes up too
    p = PolygonSet.from_geojson({"type": "Polygon", "coordinates": [[[2.5, -2.5], [6.49, -0.5], [-1.5, 3.5], [0.5, 1.4999]]]})
    assert p.vertices.tolist() == [[3, -2], [6, 0], [-1, 4], [1, 1]] and p.vertices.dtype == np.int64
    # a degenerate exterior takes its holes along; a degenerate hole goes alone
    p = PolygonSet.from_geojson({"type": "FeatureCollection", "features": [
        {"type": "Feature", "properties": {"label": 7}, "geometry": {"type": "Polygon", "coordinates": [[[0, 0], [1, 1], [0, 0]], square]}},
        {"type": "Feature", "properties": {"label": 8}, "geometry": {"type": "Polygon", "coordinates": [square, [[3, 3], [4, 4]]]}}]})
    assert p.n_features == 1 and p.group == ["8"] and p.skipped == 2 and len(p) == 1


def test_qupath_export(golden_dir):
    path = os.path.join(golden_dir, "annotation_qupath.geojson")
    p = PolygonSet.from_geojson(path)
    assert p.group == ["Tumor", "Stroma"] and p.skipped == 2 and p.n_features == 2 and len(p) == 4
    assert p.role.tolist() == [1, -1, 1, 1] and p.feature.tolist() == [0, 0, 1, 1] and p.properties[0]["objectType"] == "annotation"
    want = np.zeros((9, 16), np.uint8)
    want[2:8, 2:10] = 1                                           # 1.5 -> 2, 9.5 -> 10, 7.5 -> 8
    want[3:6, 4:7] = 0
    tumor = want.copy()
    want[0:3, 11:14] = want[5:8, 11:14] = 1
    assert np.array_equal(fill_numpy(p, 1, (9, 16)), want)
    assert np.array_equal(fill_numpy(p.select(groups="Tumor"), 1, (9, 16)), tumor)
    assert np.array_equal(fill_numpy(p.select(keep=lambda q: q["classification"]["name"] != "Stroma"), 1, (9, 16)), tumor)
    only = PolygonSet.from_geojson(path, keep=lambda q: q.get("classification", {}).get("name") == "Stroma")
    assert only.group == ["Stroma"] and np.array_equal(fill_numpy(only, 1, (9, 16)), want - tumor)
    assert len(p.select(groups=["nothing"])) == 0 and not fill_numpy(p.select(groups=["nothing"]), 1, (9, 16)).any()
    assert "2 features" in repr(p)


CAMELYON_WANT = np.array([[1, 1, 1, 1, 1, 0, 0, 0, 0, 0],        # d = 2: the triangle x + y < 12 of group _0 ...
                          [1, 0, 0, 1, 0, 0, 1, 1, 1, 0],        # ... the rectangle [13, 19) x [3, 9) of group _1 (sides through centres) ...
                          [1, 0, 0, 0, 0, 0, 1, 1, 1, 0],        # ... without the exclusion [2, 6) x [2, 6) of group _2
                          [1, 1, 0, 0, 0, 0, 1, 1, 1, 0],
                          [1, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                          [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                          [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                          [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]], np.uint8)


def camelyon_paint(polys, fill):
    out = None
    for groups, value in CAMELYON16_ORDER:
        out = fill(polys.select(groups=groups), value, out)
    return out


def test_asap_xml(golden_dir):
    path = os.path.join(golden_dir, "annotation_asap.xml")
    p = PolygonSet.from_asap_xml(path)
    assert p.group == ["_0", "_1", "_2"] and p.skipped == 1 and len(p) == 3 and p.role.tolist() == [1, 1, 1]
    assert p.ring(0).tolist() == [[0, 0], [12, 0], [0, 12]]        # sorted by Order; 0.49 -> 0, -0.4 -> 0, -0.5 -> 0, 11.5 -> 12
    assert p.ring(1).tolist() == [[13, 3], [19, 3], [19, 9], [13, 9]] and p.ring(2).tolist() == [[2, 2], [6, 2], [6, 6], [2, 6]]
    assert p.properties[1] == {"name": "Annotation 1", "type": "Rectangle", "group": "_1"}
    with open(path) as f:
        again = PolygonSet.from_asap_xml(f.read())
    assert np.array_equal(again.vertices, p.vertices) and again.group == p.group
    got = camelyon_paint(p, lambda q, value, into: fill_numpy(q, 2, (8, 10), value=value, into=into))
    assert np.array_equal(got, CAMELYON_WANT)
    assert CAMELYON16_ORDER == ((("_0", "_1", "Tumor"), 1), (("_2", "Exclusion"), 0))


# ------------------------------------------------------------------------------------------------ tile counts
def loop_counts(mask, coords, patch, d, origin):
    out = np.zeros((len(coords), 2), np.int32)
    for n, (x, y) in enumerate(coords.tolist()):
        for i in range(mask.shape[0]):
            for j in range(mask.shape[1]):
                cx, cy = 2 * origin[0] + (2 * j + 1) * d, 2 * origin[1] + (2 * i + 1) * d
                if 2 * x <= cx < 2 * (x + patch) and 2 * y <= cy < 2 * (y + patch):
                    out[n, 0] += 1
                    out[n, 1] += int(mask[i, j] != 0)
    return out


@pytest.mark.parametrize("d,patch,origin", [(1, 5, (0, 0)), (1, 8, (3, -2)), (16, 40, (0, 0)), (16, 224, (-32, 64)), (16, 7, (0, 0))])
def test_tile_counts_against_a_pixel_loop(d, patch, origin):
    g = np.random.default_rng(d + patch)
    mask = (g.random((13, 17)) < 0.5).astype(np.uint8) * g.integers(1, 256, (13, 17)).astype(np.uint8)
    x = g.integers(origin[0] - 2 * patch, origin[0] + 17 * d + patch, 60)
    y = g.integers(origin[1] - 2 * patch, origin[1] + 13 * d + patch, 60)
    coords = np.stack([x, y], 1).astype(np.int64)
    coords[:4] = [[origin[0] - patch, origin[1]], [origin[0], origin[1] - patch], [origin[0] + 17 * d, origin[1]], [origin[0] - 5 * patch, origin[1] - 5 * patch]]
    got = tile_counts_numpy(mask, coords, patch, d, origin)
    assert got.dtype == np.int32 and np.array_equal(got, loop_counts(mask, coords, patch, d, origin))
    assert (got[:4] == 0).all() and got[:, 0].max() > 0
    tm = TissueMask(mask, d)
    assert np.array_equal(tile_counts_numpy(tm, coords, patch, origin=origin), got)
    assert np.array_equal(tile_counts_numpy(torch.from_numpy(mask), torch.from_numpy(coords), patch, d, origin), got)


def test_tile_label_rule_at_downsample_1():
    """The reference's rule: a tile is tumour iff more than half of its patch^2 pixels are set in the level-0 mask."""
    g = np.random.default_rng(9)
    mask = (g.random((64, 80)) < 0.5).astype(np.uint8)
    mask[:32, :40] = 1
    patch = 16
    coords = np.array([(x, y) for y in range(0, 64, patch) for x in range(0, 80, patch)], np.int64)
    counts = tile_counts_numpy(mask, coords, patch, 1)
    want = np.array([mask[y:y + patch, x:x + patch].sum() > 0.5 * patch * patch for x, y in coords])
    assert (counts[:, 0] == patch * patch).all() and np.array_equal(2 * counts[:, 1] > patch * patch, want) and 0 < want.sum() < len(want)


# ------------------------------------------------------------------------------------------------ argument checks
def test_polygon_set_checks():
    sq = rect(0, 0, 4, 4)
    with pytest.raises(ValueError):
        PolygonSet(sq, [0, 4], role=[2])
    with pytest.raises(ValueError):
        PolygonSet(sq, [0, 4], feature=[0, 1])
    with pytest.raises(ValueError):
        PolygonSet(sq, [0, 4], properties=[{}], group=["a", "b"])
    with pytest.raises(ValueError):
        PolygonSet(sq, [0, 4]).weights("nonzero")
    with pytest.raises(ValueError):
        PolygonSet.from_outlines(sq)
    with pytest.raises(ValueError):
        PolygonSet.from_outlines(RegionOutlines(torch.zeros((0, 8), dtype=torch.int64), torch.zeros((0, 2), dtype=torch.int32)))   # no downsample
    empty = PolygonSet(np.zeros((0, 2), np.int64), [0])
    assert len(empty) == 0 and empty.n_features == 0 and empty.weights().shape == (0,) and not fill_numpy(empty, 1, (3, 3)).any()


BAD_CALLS = [  # (polys, downsample, shape, keywords)
    ((np.array([(0, 0), (4, 0), ((1 << 26) + 1, 4)]), [0, 3], [1]), 1, (4, 4), {}),
    ((np.array([(0, 0), (4, 0), (4, -(1 << 26) - 1)]), [0, 3], [1]), 1, (4, 4), {}),
    ((rect(0, 0, 4, 4), [0, 4], [1]), 1, (4, 4), dict(origin=((1 << 26) + 1, 0))),
    ((rect(0, 0, 4, 4), [0, 4], [1]), 0, (4, 4), {}),
    ((rect(0, 0, 4, 4), [0, 4], [1]), 4097, (4, 4), {}),
    ((rect(0, 0, 4, 4), [0, 4], [1]), 1.5, (4, 4), {}),
    ((rect(0, 0, 4, 4), [0, 4], [1]), 1, (1 << 14, 1 << 14), {}),                     # h (w + 1) = 2^28 + 2^14
    ((rect(0, 0, 4, 4), [0, 4], [1]), 1, (0, 4), {}),
    ((rect(0, 0, 4, 4), [0, 4], [1]), 1, (4,), {}),
    ((rect(0, 0, 4, 4), [0, 2, 4], [1, 1]), 1, (4, 4), {}),                          # rings of 2 vertices
    ((rect(0, 0, 4, 4), [0, 4, 3], [1, 1]), 1, (4, 4), {}),                          # does not ascend
    ((rect(0, 0, 4, 4), [0, 3], [1]), 1, (4, 4), {}),                                # does not end at V
    ((rect(0, 0, 4, 4), [1, 4], [1]), 1, (4, 4), {}),                                # does not start at 0
    ((rect(0, 0, 4, 4), [0, 4], [2]), 1, (4, 4), {}),
    ((rect(0, 0, 4, 4), [0, 4], [1, 1]), 1, (4, 4), {}),
    ((rect(0, 0, 4, 4).astype(np.float64), [0, 4], [1]), 1, (4, 4), {}),
    ((rect(0, 0, 4, 4).ravel(), [0, 4], [1]), 1, (4, 4), {}),
    ((rect(0, 0, 4, 4), [0, 4]), 1, (4, 4), {}),
    ("polygons", 1, (4, 4), {}),
    ((rect(0, 0, 4, 4), [0, 4], [1]), 1, (4, 4), dict(value=256)),
    ((rect(0, 0, 4, 4), [0, 4], [1]), 1, (4, 4), dict(value=-1)),
    ((rect(0, 0, 4, 4), [0, 4], [1]), 1, (4, 4), dict(value=1.5)),
    ((rect(0, 0, 4, 4), [0, 4], [1]), 1, (4, 4), dict(into=np.zeros((4, 5), np.uint8))),
    ((rect(0, 0, 4, 4), [0, 4], [1]), 1, (4, 4), dict(into=np.zeros((4, 4), np.int32))),
    ((rect(0, 0, 4, 4), [0, 4], [1]), 1, (4, 4), dict(into=torch.zeros((4, 4), dtype=torch.bool))),
    ((rect(0, 0, 4, 4), [0, 4], [1]), 1, (4, 4), dict(rule="nonzero")),
    ((rect(0, 0, 4, 4), [0, 4], [1]), 1, (4, 4), dict(origin=(0,))),
]


@pytest.fixture
def no_library(monkeypatch):
    """Any touch of the library, and with it of the device, fails the test: the checks come first."""
    def boom():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", boom)
    from keep_amd import KEEPModel
    return KEEPModel()


def test_fill_argument_errors_come_before_any_device_work(no_library):
    for polys, d, shape, kw in BAD_CALLS:
        with pytest.raises(ValueError):
            fill_numpy(polys, d, shape, **kw)
        with pytest.raises(ValueError):
            no_library.fill_polygons(polys, d, shape, **kw)
    sq = PolygonSet(rect(0, 0, 4, 4), [0, 4])
    for args, kw in (((sq, 0, (4, 4)), {}), (((rect(0, 0, 4, 4), [0, 4], [1]), 1, (4, 4)), {}), ((sq, 1, (4, 4)), dict(rule="odd")),
                     ((sq, 1, (4, 4)), dict(mode="corner")), ((sq, 1, (4, 4)), dict(order=())), ((sq, 1, (4, 4)), dict(order=(("_0", 300),)))):
        with pytest.raises(ValueError):
            no_library.annotation_mask(*args, **kw)
    with pytest.raises(AssertionError):                           # a good call does reach the library
        no_library.fill_polygons(sq, 1, (4, 4))


def test_tile_count_argument_errors_come_before_any_device_work(no_library):
    mask, coords = np.zeros((4, 5), np.uint8), np.zeros((3, 2), np.int64)
    bad = [((mask, coords, 16), {}),                              # no downsample
           ((mask, coords, 16, 0), {}), ((mask, coords, 0, 1), {}), ((mask, coords, 1.5, 1), {}), ((mask, coords, (1 << 30) + 1, 1), {}),
           ((mask.astype(np.int32), coords, 16, 1), {}), ((mask[0], coords, 16, 1), {}), ((mask, coords[:, :1], 16, 1), {}),
           ((mask, coords.astype(np.float32), 16, 1), {}), ((mask, torch.zeros((3, 2)), 16, 1), {}), ((mask, coords, 16, 1), dict(origin=(0,))),
           ((mask, coords, 16, 1), dict(origin=(1 << 41, 0))), ((TissueMask(mask, 4), coords, 16, 8), {})]
    for args, kw in bad:
        with pytest.raises(ValueError):
            tile_counts_numpy(*args, **kw)
        with pytest.raises(ValueError):
            no_library.mask_tile_counts(*args, **kw)
    with pytest.raises(AssertionError):
        no_library.mask_tile_counts(mask, coords, 16, 1)


def test_check_functions_return_what_the_kernels_take():
    assert check_fill_args(np.int64(3), [5, 7], (-4, 9), "evenodd", 255) == (3, (5, 7), (-4, 9), 1, 255)
    v, rs, wt = check_rings(np.asfortranarray(rect(0, 0, 4, 4).astype(np.int32)), [0, 4], [-1])
    assert v.dtype == np.int64 and v.flags.c_contiguous and rs.dtype == np.int64 and wt.dtype == np.int32 and wt.tolist() == [-1]
    m, c, patch, d, origin = check_tile_args(TissueMask(np.ones((3, 3), np.uint8), 8), [[0, 0]], 16)
    assert d == 8 and patch == 16 and origin == (0, 0) and tuple(c.shape) == (1, 2)
