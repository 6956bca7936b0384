"""Region outlines, host side: keep_amd.outline.outlines_numpy (the yardstick of tests/test_outlines_gpu.py)
held to statements that do not trace anything (exposed pixel sides counted with shifts, the region table's areas, scipy's component
counts of the complement under the dual connectivity, an even-odd refill), hand cases, RegionOutlines, draw_numpy against a per-pixel
loop and the argument checks.  No GPU."""
import json

import numpy as np
import pytest
import torch

from keep_amd.components import COLUMNS as TABLE_COLUMNS, RegionTable, regions_numpy
from keep_amd.outline import (COLUMNS, NCOLS, RegionOutlines, check_draw_args, check_outline_args, check_ring_count, draw_numpy,
                              labels_tensor, outlines_numpy, regions_labels, rgb_tensor)
from test_regions import MASKS

COL = {name: i for i, name in enumerate(COLUMNS)}
TCOL = {name: i for i, name in enumerate(TABLE_COLUMNS)}


def exposed_sides(labels):
    """The number of (pixel, side) pairs whose neighbour across the side lies outside or carries another label."""
    P = np.pad(labels, 1)
    h, w = labels.shape
    return sum(int(((labels > 0) & (P[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] != labels)).sum()) for dx, dy in ((0, -1), (1, 0), (0, 1), (-1, 0)))


def refill(rings, vertices, label, shape):
    """Even-odd refill of one region's rings: toggle the rows of every vertical ring segment at its column, cumulative XOR along x."""
    h, w = shape
    t = np.zeros((h, w + 1), bool)
    for r in rings[rings[:, COL["label"]] == label]:
        v = vertices[r[COL["start"]]:r[COL["start"]] + r[COL["nvert"]]]
        for (x0, y0), (x1, y1) in zip(v, np.roll(v, -1, axis=0)):
            assert (x0 == x1) != (y0 == y1)                     # axis-parallel, never of length 0
            if x0 == x1:
                t[min(y0, y1):max(y0, y1), x0] ^= True
    return np.logical_xor.accumulate(t, axis=1)[:, :w]


def check_invariants(img, connectivity, min_area=1):
    ndi = pytest.importorskip("scipy.ndimage")
    labels, table = regions_numpy(img, connectivity, min_area)
    n = len(table)
    rings, vertices = outlines_numpy(labels, connectivity, n)
    assert rings.dtype == np.int64 and rings.shape[1] == NCOLS and vertices.dtype == np.int32 and vertices.shape[1:] == (2,)
    h, w = labels.shape
    assert int(rings[:, COL["nedge"]].sum()) == exposed_sides(labels)
    assert len(vertices) == rings[:, COL["nvert"]].sum()
    assert np.array_equal(rings[:, COL["start"]], np.cumsum(rings[:, COL["nvert"]]) - rings[:, COL["nvert"]])
    assert np.array_equal(rings[:, COL["hole"]], (rings[:, COL["area2"]] < 0).astype(np.int64)) and (rings[:, COL["area2"]] != 0).all()
    if len(vertices):
        assert vertices.min() >= 0 and vertices[:, 0].max() <= w and vertices[:, 1].max() <= h
        assert np.array_equal(vertices[rings[:, COL["start"]]], rings[:, [COL["lead_x"], COL["lead_y"]]])
    dual = np.ones((3, 3)) if connectivity == 4 else ndi.generate_binary_structure(2, 1)
    for l in range(1, n + 1):
        mine = rings[rings[:, COL["label"]] == l]
        assert mine[:, COL["area2"]].sum() == 2 * table[l - 1, TCOL["area"]]
        assert (mine[:, COL["area2"]] > 0).sum() == 1 and mine[0, COL["area2"]] > 0          # one outer ring, the first in leader order
        assert (mine[0, COL["lead_x"]], mine[0, COL["lead_y"]]) == (table[l - 1, TCOL["first_x"]], table[l - 1, TCOL["first_y"]])
        assert len(mine) - 1 == ndi.label(np.pad(labels != l, 1, constant_values=True), structure=dual)[1] - 1
        assert np.array_equal(refill(rings, vertices, l, (h, w)), labels == l)
    return rings, vertices


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name,img", MASKS, ids=[n for n, _ in MASKS])
def test_restatement_holds_the_independent_statements(name, img, connectivity):
    if name in ("tissue", "raw"):                               # thousands of regions: the per-region statements on a crop
        img = img[:96, :160]
    rings, _ = check_invariants(img, connectivity)
    if name == "zeros":
        assert len(rings) == 0
    if name == "all-ones":
        assert rings.tolist() == [[1, 0, 4, 2 * (13 + 200), 2 * 13 * 200, 0, 0, 0]]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("density", [0.3, 0.5, 0.65, 0.8])
def test_restatement_on_random_masks(density, connectivity):
    g = np.random.default_rng(int(density * 100) + connectivity)
    check_invariants((g.random((37, 53)) < density).astype(np.uint8), connectivity)
    check_invariants((g.random((37, 53)) < density).astype(np.uint8), connectivity, 4)


def test_one_pixel():
    for shape, at in (((1, 1), (0, 0)), ((3, 4), (1, 2))):
        lab = np.zeros(shape, np.int32)
        lab[at] = 1
        y, x = at
        rings, v = outlines_numpy(lab, 8)
        assert v.tolist() == [[x, y], [x + 1, y], [x + 1, y + 1], [x, y + 1]]
        assert rings.tolist() == [[1, 0, 4, 4, 2, x, y, 0]]


def test_two_diagonal_pixels():
    img = np.array([[1, 0], [0, 1]], np.uint8)
    lab4, t4 = regions_numpy(img, 4)
    rings, v = outlines_numpy(lab4, 4)
    assert len(t4) == 2 and rings[:, COL["label"]].tolist() == [1, 2] and rings[:, COL["nvert"]].tolist() == [4, 4]
    assert rings[:, COL["area2"]].tolist() == [2, 2] and v[4:].tolist() == [[1, 1], [2, 1], [2, 2], [1, 2]]
    lab8, t8 = regions_numpy(img, 8)
    rings, v = outlines_numpy(lab8, 8)
    assert len(t8) == 1 and rings.tolist() == [[1, 0, 8, 8, 4, 0, 0, 0]]
    assert v.tolist() == [[0, 0], [1, 0], [1, 1], [2, 1], [2, 2], [1, 2], [1, 1], [0, 1]]        # (1, 1) is visited twice
    # the other diagonal, and the same labels traced with connectivity 4: two rings of one label
    rings, v = outlines_numpy(np.array([[0, 1], [1, 0]], np.int32), 8)
    assert rings.tolist() == [[1, 0, 8, 8, 4, 1, 0, 0]] and v.tolist().count([1, 1]) == 2
    rings, _ = outlines_numpy(lab8, 4)
    assert rings[:, [COL["label"], COL["nvert"], COL["area2"]]].tolist() == [[1, 4, 2], [1, 4, 2]]


def test_square_minus_its_centre():
    lab = np.ones((3, 3), np.int32)
    lab[1, 1] = 0
    for connectivity in (4, 8):
        rings, v = outlines_numpy(lab, connectivity)
        assert rings.tolist() == [[1, 0, 4, 12, 18, 0, 0, 0], [1, 4, 4, 4, -2, 2, 1, 1]]
        assert v.tolist() == [[0, 0], [3, 0], [3, 3], [0, 3], [2, 1], [1, 1], [1, 2], [2, 2]]   # the hole runs the other way round, from the
        # bottom edge of the pixel above it (slot 6, the smallest)


def test_l_shape():
    lab = np.array([[1, 0, 0], [1, 0, 0], [1, 1, 1]], np.int32)
    rings, v = outlines_numpy(lab, 4)
    assert rings.tolist() == [[1, 0, 6, 12, 10, 0, 0, 0]]
    assert v.tolist() == [[0, 0], [1, 0], [1, 2], [3, 2], [3, 3], [0, 3]]


def test_two_labels_side_by_side_share_an_edge():
    lab = np.array([[1, 1, 2], [1, 1, 2]], np.int32)
    rings, v = outlines_numpy(lab, 8)
    assert rings.tolist() == [[1, 0, 4, 8, 8, 0, 0, 0], [2, 4, 4, 6, 4, 2, 0, 0]]
    assert v.tolist() == [[0, 0], [2, 0], [2, 2], [0, 2], [2, 0], [3, 0], [3, 2], [2, 2]]       # x = 2 from 0 to 2 in both, opposite ways
    assert int(rings[:, COL["nedge"]].sum()) == exposed_sides(lab)


def test_region_on_all_four_borders_and_foreign_labels():
    lab = np.ones((4, 6), np.int32)
    assert outlines_numpy(lab, 8)[0].tolist() == [[1, 0, 4, 20, 48, 0, 0, 0]]
    lab[1, 2], lab[2, 4] = 7, -3                                # outside 1..n: background, two holes
    rings, _ = outlines_numpy(lab, 8, 1)
    assert rings[:, [COL["label"], COL["area2"], COL["hole"]]].tolist() == [[1, 48, 0], [1, -2, 1], [1, -2, 1]]
    assert len(outlines_numpy(lab, 8)[0]) == 4                  # n defaults to the largest label: 7 is a region of its own
    assert len(outlines_numpy(lab, 8, 0)[0]) == 0 and outlines_numpy(lab, 8, 0)[1].shape == (0, 2)


def nested():
    """A 9 x 12 frame with a hole of 5 x 8, two islands inside it (one of one pixel), and a second small hole in the frame."""
    img = np.ones((9, 12), np.uint8)
    img[2:7, 2:10] = 0
    img[3:6, 3:5] = 1
    img[4, 7] = 1
    labels, table = regions_numpy(img, 4)
    rings, vertices = outlines_numpy(labels, 4)
    return labels, table, rings, vertices


def test_region_outlines_polygons_and_cuts():
    img = np.ones((12, 20), np.uint8)
    img[2:4, 2:5] = 0                                           # holes of 6, 1, 12 and 2 pixels
    img[6, 3] = 0
    img[6:9, 8:12] = 0
    img[10, 15:17] = 0
    labels, table = regions_numpy(img, 8)
    rings, vertices = outlines_numpy(labels, 8)
    o = RegionOutlines(torch.from_numpy(rings), torch.from_numpy(vertices), 16, (320, 640), n=1)
    assert o.n_rings == len(o) == 5 and o.n == 1 and o.area2.tolist() == [480, -12, -2, -24, -4] and o.hole.tolist() == [0, 1, 1, 1, 1]
    assert o.rings_of(1).tolist() == [0, 1, 2, 3, 4] and o.rings_of(2).tolist() == []
    assert o.n_holes().tolist() == [4] and o.perimeter().tolist() == [64] and o.area().tolist() == [int(img.sum())]
    polys = o.polygons(1)
    assert len(polys) == 5 and polys[0].tolist() == [[0, 0], [20, 0], [20, 12], [0, 12]] and polys[2].tolist() == [[4, 6], [3, 6], [3, 7], [4, 7]]
    assert [len(o.polygons(1, max_n_holes=k)) for k in (0, 1, 2, 9)] == [1, 2, 3, 5]
    assert [p[0].tolist() for p in o.polygons(1, max_n_holes=2)[1:]] == [[5, 2], [12, 6]]       # the two largest, in ring order
    assert [len(o.polygons(1, min_hole_area=a)) for a in (0, 1, 2, 3, 6, 7, 12, 13)] == [5, 5, 4, 3, 3, 2, 2, 1]
    assert len(o.polygons(1, max_n_holes=1, min_hole_area=13)) == 1 and o.polygons(1, 1)[1][0].tolist() == [12, 6]
    with pytest.raises(ValueError):
        o.polygons(1, max_n_holes=-1)
    lv = o.to_level0()
    assert lv.dtype == np.int64 and lv[:4].tolist() == [[320, 640], [640, 640], [640, 832], [320, 832]]
    assert np.array_equal(lv, vertices.astype(np.int64) * 16 + np.array([320, 640]))
    with pytest.raises(ValueError):
        RegionOutlines(torch.from_numpy(rings), torch.from_numpy(vertices)).to_level0()
    with pytest.raises(ValueError):
        RegionOutlines(torch.from_numpy(rings[:, :7]), torch.from_numpy(vertices))
    with pytest.raises(ValueError):
        RegionOutlines(torch.from_numpy(rings), torch.from_numpy(vertices.astype(np.int64)))
    assert RegionOutlines(torch.from_numpy(rings), torch.from_numpy(vertices)).n == 1          # n from the labels of the rings
    empty = RegionOutlines(torch.zeros((0, NCOLS), dtype=torch.int64), torch.zeros((0, 2), dtype=torch.int32), n=3)
    assert empty.n_holes().tolist() == [0, 0, 0] and empty.perimeter().tolist() == [0, 0, 0] and empty.polygons(2) == []
    assert empty.to_geojson(level0=False) == {"type": "FeatureCollection", "features": []}


def test_geojson_round_trips_and_closes_its_rings():
    labels, table, rings, vertices = nested()
    assert len(table) == 3 and rings[:, COL["label"]].tolist() == [1, 1, 2, 3]
    t = np.array(table)
    t[0, TCOL["covered"]:] = 5, 10, 5 * 65535, 65535            # region 1 is scored, the others are not
    regs = RegionTable(torch.from_numpy(t), torch.from_numpy(labels), 8, (80, 160), connectivity=4)
    o = RegionOutlines(torch.from_numpy(rings), torch.from_numpy(vertices), 8, (80, 160), n=3)
    gj = json.loads(json.dumps(o.to_geojson(table=regs)))
    assert gj["type"] == "FeatureCollection" and [f["properties"]["label"] for f in gj["features"]] == [1, 2, 3]
    for f, want_rings in zip(gj["features"], (2, 1, 1)):
        assert f["type"] == "Feature" and f["geometry"]["type"] == "Polygon" and len(f["geometry"]["coordinates"]) == want_rings
        for ring in f["geometry"]["coordinates"]:
            assert ring[0] == ring[-1] and len(ring) >= 5
        lab = f["properties"]["label"]
        assert f["properties"]["area"] == table[lab - 1, TCOL["area"]] and f["properties"]["border"] == table[lab - 1, TCOL["border"]]
    p = gj["features"][0]["properties"]
    assert p == {"label": 1, "area": 68, "n_holes": 1, "perimeter": 42, "mean_score": 0.5, "peak_score": 1.0, "border": 1}
    assert gj["features"][1]["properties"]["mean_score"] is None and gj["features"][2]["properties"]["peak_score"] is None
    assert gj["features"][0]["geometry"]["coordinates"][0] == [[80, 160], [176, 160], [176, 232], [80, 232], [80, 160]]
    assert gj["features"][0]["geometry"]["coordinates"][1][0] == [80 + 8 * 10, 160 + 8 * 2]    # the hole starts at its top-right corner
    plain = o.to_geojson(level0=False, max_n_holes=0)
    assert plain["features"][0]["geometry"]["coordinates"] == [[[0, 0], [12, 0], [12, 9], [0, 9], [0, 0]]]
    assert set(plain["features"][0]["properties"]) == {"label", "area", "n_holes", "perimeter"} and plain["features"][0]["properties"]["n_holes"] == 1
    with pytest.raises(ValueError):
        RegionOutlines(torch.from_numpy(rings), torch.from_numpy(vertices), n=3).to_geojson()   # no downsample
    with pytest.raises(ValueError):
        o.to_geojson(table=RegionTable(torch.from_numpy(t[:2])))


def loop_draw(rgb, labels, color, width):
    h, w = labels.shape
    out = rgb.copy()
    for y in range(h):
        for x in range(w):
            l = int(labels[y, x])
            if l <= 0:
                continue
            hit = False
            for dy in range(-width, width + 1):
                for dx in range(-width, width + 1):
                    yy, xx = y + dy, x + dx
                    if yy < 0 or yy >= h or xx < 0 or xx >= w or int(labels[yy, xx]) != l:
                        hit = True
            if hit:
                out[y, x] = color
    return out


@pytest.mark.parametrize("width", [1, 2, 16])
def test_draw_numpy_against_a_pixel_loop(width):
    g = np.random.default_rng(width)
    labels = np.zeros((9, 11), np.int32)
    labels[1:8, 1:10] = 1
    labels[3:5, 4:6] = 0
    labels[0, 0] = 2
    labels[8, 6:11] = 3
    labels[6, 8] = -4                                           # never drawn, but not label 1 either
    rgb = g.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    got = draw_numpy(rgb, labels, (255, 128, 1), width)
    assert got.dtype == np.uint8 and np.array_equal(got, loop_draw(rgb, labels, (255, 128, 1), width))
    assert np.array_equal(got[labels <= 0], rgb[labels <= 0]) and got is not rgb
    if width == 1:
        assert got[2, 2].tolist() == rgb[2, 2].tolist() and got[1, 1].tolist() == [255, 128, 1]
    big = np.ones((40, 45), np.int32)
    assert (draw_numpy(np.zeros((40, 45, 3), np.uint8), big, (9, 9, 9), width)[:, :, 0] == 9).sum() == 40 * 45 - max(40 - 2 * width, 0) * max(45 - 2 * width, 0)


def test_argument_checks():
    for args in [(6,), (0,), (8.5,), (True,), (8, -1), (8, 1.5)]:
        with pytest.raises(ValueError):
            check_outline_args(*args)
    assert check_outline_args(4, 0) == (4, 0) and check_outline_args(8) == (8, 1 << 20)
    ok = np.zeros((4, 5), np.int32)
    for bad in [ok.astype(np.int64), ok.astype(np.uint8), ok[0], ok[None], np.zeros((0, 5), np.int32), [[0, 1]], torch.zeros(4, 5)]:
        with pytest.raises(ValueError):
            labels_tensor(bad)
    assert labels_tensor(ok).dtype == torch.int32 and labels_tensor(torch.from_numpy(ok)).shape == (4, 5)
    for color, width in [((0, 0, 0), 0), ((0, 0, 0), 17), ((0, 0, 0), 1.5), ((0, 0), 1), ((0, 0, 256), 1), ((-1, 0, 0), 1), ((0.5, 0, 0), 1), (7, 1)]:
        with pytest.raises(ValueError):
            check_draw_args(color, width)
    assert check_draw_args((1, 2, 3), 16) == (1 | 2 << 8 | 3 << 16, 16)
    for bad in [np.zeros((4, 5), np.uint8), np.zeros((4, 5, 4), np.uint8), np.zeros((4, 5, 3), np.float32), np.zeros((5, 4, 3), np.uint8)]:
        with pytest.raises(ValueError):
            rgb_tensor(bad, (4, 5))
    assert check_ring_count(3, 3) == 3
    with pytest.raises(ValueError, match="max_rings"):
        check_ring_count(4, 3)
    table = torch.zeros((2, len(TABLE_COLUMNS)), dtype=torch.int64)
    with pytest.raises(ValueError, match="labels"):
        regions_labels(RegionTable(table))
    with pytest.raises(ValueError):
        regions_labels(RegionTable(table, torch.from_numpy(ok)), n=3)
    lab, n, conn, d, origin = regions_labels(RegionTable(table, torch.from_numpy(ok), 16, (32, 64), connectivity=4))
    assert (n, conn, d, origin) == (2, 4, 16, (32, 64)) and RegionTable(table).connectivity is None
    for n in (-1, 21, 1.5):
        with pytest.raises(ValueError):
            regions_labels(ok, n)
    for bad in [dict(connectivity=6), dict(n=-1)]:
        with pytest.raises(ValueError):
            outlines_numpy(ok, **bad)
    with pytest.raises(ValueError):
        outlines_numpy(ok.astype(np.int64))
    with pytest.raises(ValueError):
        draw_numpy(np.zeros((4, 5, 3), np.uint8), ok.astype(np.int64))
    with pytest.raises(ValueError):
        draw_numpy(np.zeros((4, 6, 3), np.uint8), ok)


def test_model_checks_arguments_before_any_device_work():
    from keep_amd import KEEPModel
    m = KEEPModel()
    ok = np.zeros((4, 5), np.int32)
    rgb = np.zeros((4, 5, 3), np.uint8)
    table = torch.zeros((1, len(TABLE_COLUMNS)), dtype=torch.int64)
    for args, kw in [((ok,), dict()),                           # a label image needs n
                     ((ok,), dict(n=-1)), ((ok,), dict(n=1, connectivity=6)), ((ok,), dict(n=1, max_rings=-1)), ((ok.astype(np.int64),), dict(n=1)),
                     ((RegionTable(table),), dict()), ((RegionTable(table, torch.from_numpy(ok)),), dict(connectivity=5))]:
        with pytest.raises(ValueError):
            m.region_outlines(*args, **kw)
    for args, kw in [((rgb, ok), dict(width=0)), ((rgb, ok), dict(width=17)), ((rgb, ok), dict(color=(0, 0, 300))), ((rgb[:3], ok), dict()),
                     ((rgb.astype(np.float32), ok), dict()), ((rgb, RegionTable(table)), dict()), ((rgb, ok.astype(np.uint8)), dict())]:
        with pytest.raises(ValueError):
            m.draw_outlines(*args, **kw)
