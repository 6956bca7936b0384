"""Region outlines on the MI355X: keep_outline_count / keep_outline_trace / keep_outline_draw,
KEEPModel.region_outlines, KEEPModel.draw_outlines.

Everything the device computes is an integer, so every comparison is exact: the yardstick is keep_amd.outline.outlines_numpy /
draw_numpy, which tests/test_outlines.py holds to statements that trace nothing; the large shapes are held to closed forms."""
import ctypes as C
import itertools
import json

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel, _lib, wsi
from keep_amd.components import COLUMNS as TABLE_COLUMNS, RegionTable, regions_numpy
from keep_amd.config import small_shape
from keep_amd.heatmap import unpack_numpy
from keep_amd.model import _ptr, _stream
from keep_amd.outline import COLUMNS, NCOLS, RegionOutlines, draw_numpy, outlines_numpy
from keep_amd.synth import synth_state_dict, synth_tile_family
from test_regions import MASKS
from test_tissue import serpentine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COL = {name: i for i, name in enumerate(COLUMNS)}


@pytest.fixture(scope="module")
def model():
    m = KEEPModel(precision="strict")
    m.load_state_dict(synth_state_dict(small_shape(2, 2), seed=5), strict=True)
    return m.to(DEV).eval()


def same(t: torch.Tensor, a: np.ndarray) -> bool:
    return t.dtype == torch.from_numpy(a).dtype and tuple(t.shape) == a.shape and torch.equal(t.cpu(), torch.from_numpy(a))


def check(o: RegionOutlines, want):
    rings, vertices = want
    assert o.rings.device == torch.device(DEV) and o.vertices.device == torch.device(DEV) and o.n_rings == len(rings)
    assert same(o.rings, rings)
    assert same(o.vertices, vertices)


@pytest.mark.parametrize("name,img", MASKS, ids=[n for n, _ in MASKS])
def test_outlines_match_the_restatement(model, name, img):
    """The sweep of tests/test_regions.py (spiral and serpentine among it: one ring of many rounds each)."""
    dev = torch.from_numpy(img).to(DEV)
    for connectivity, min_area in itertools.product((4, 8), (1, 50)):
        regs = model.mask_regions(dev, connectivity, min_area)
        assert regs.connectivity == connectivity
        o = model.region_outlines(regs)                         # the table's own connectivity
        labels = regs.labels.cpu().numpy()
        check(o, outlines_numpy(labels, connectivity, regs.n))
        assert o.n == regs.n and torch.equal(o.label, o.rings[:, COL["label"]])
        if regs.n:
            assert np.array_equal(o.area(), regs.numpy()[:, TABLE_COLUMNS.index("area")])
    other = model.region_outlines(regs, connectivity=4)         # labelled with 8, traced with 4: still the restatement
    check(other, outlines_numpy(labels, 4, regs.n))


@pytest.mark.parametrize("h,w", [(1, 1), (1, 300), (300, 1), (5, 67), (67, 129), (4, 4099)])
def test_shapes_that_break_walks_and_scans(model, h, w):
    g = np.random.default_rng(h * 7 + w)
    for img in (np.ones((h, w), np.uint8), np.zeros((h, w), np.uint8), (np.indices((h, w)).sum(0) % 2).astype(np.uint8),
                (g.random((h, w)) < 0.5).astype(np.uint8)):
        for connectivity in (4, 8):
            regs = model.mask_regions(img, connectivity)
            o = model.region_outlines(regs)
            check(o, outlines_numpy(regs.labels.cpu().numpy(), connectivity, regs.n))
            if not img.any():
                assert o.n_rings == 0 and tuple(o.vertices.shape) == (0, 2) and tuple(o.rings.shape) == (0, NCOLS)


def test_one_ring_of_a_million_edges(model):
    """A 1024 x 1024 serpentine: one region, one ring of more than 2^19 edges, twenty rounds of jumping."""
    img = serpentine(1024, 1024)
    regs = model.mask_regions(img, 4)
    o = model.region_outlines(regs)
    want = outlines_numpy(regs.labels.cpu().numpy(), 4, regs.n)
    assert regs.n == 1 and len(want[0]) == 1 and want[0][0, COL["nedge"]] > 1 << 19
    check(o, want)
    assert int(o.area2[0]) == 2 * int(img.sum())


def test_frame_with_a_hole_4096(model):
    """A 4096 x 4096 mask: a square frame [a, b)^2 without the hole [c, e)^2, and a block [p, q)^2 inside the hole: closed forms."""
    n, a, b, c, e, p, q = 4096, 100, 4000, 700, 3001, 1500, 1777
    mask = torch.zeros((n, n), dtype=torch.uint8, device=DEV)
    mask[a:b, a:b] = 1
    mask[c:e, c:e] = 0
    mask[p:q, p:q] = 1
    want = np.array([[1, 0, 4, 4 * (b - a), 2 * (b - a) ** 2, a, a, 0],
                     [1, 4, 4, 4 * (e - c), -2 * (e - c) ** 2, e, c, 1],       # led by the bottom edge of the pixel above its top-right corner
                     [2, 8, 4, 4 * (q - p), 2 * (q - p) ** 2, p, p, 0]], np.int64)
    verts = np.array([[a, a], [b, a], [b, b], [a, b], [e, c], [c, c], [c, e], [e, e], [p, p], [q, p], [q, q], [p, q]], np.int32)
    for connectivity in (4, 8):
        o = model.region_outlines(model.mask_regions(mask, connectivity))
        assert same(o.rings, want) and same(o.vertices, verts)
        assert o.n_holes().tolist() == [1, 0] and o.perimeter().tolist() == [4 * (b - a), 4 * (q - p)]


def test_a_callers_own_labels_and_input_forms(model):
    g = np.random.default_rng(3)
    labels = g.integers(-2, 6, (45, 203)).astype(np.int32)      # neighbours with different labels, values outside 1..n
    want = outlines_numpy(labels, 8, 3)
    assert (want[0][:, COL["label"]] <= 3).all() and len(want[0]) > 100
    forms = [labels, torch.from_numpy(labels), torch.from_numpy(labels).to(DEV), np.asfortranarray(labels),
             torch.from_numpy(np.concatenate([labels, labels], 1)).to(DEV)[:, :203]]
    for lab in forms:
        check(model.region_outlines(lab, 8, n=3), want)
    check(model.region_outlines(labels, n=3), want)             # a label image defaults to connectivity 8
    check(model.region_outlines(labels, 4, n=5), outlines_numpy(labels, 4, 5))
    again = model.region_outlines(labels, 8, n=3)               # two runs are equal
    first = model.region_outlines(labels, 8, n=3)
    assert torch.equal(again.rings, first.rings) and torch.equal(again.vertices, first.vertices)
    none = model.region_outlines(labels, 8, n=0)                # no region: nothing is traced
    assert none.n_rings == 0 and tuple(none.vertices.shape) == (0, 2) and none.n == 0
    assert again.downsample is None and again.origin == (0, 0)
    with pytest.raises(ValueError):
        model.region_outlines(labels)
    with pytest.raises(ValueError):
        model.region_outlines(model.mask_regions(np.ones((4, 5), np.uint8), labels=False))


def test_max_rings_and_a_following_call(model):
    checker = (np.indices((40, 100)).sum(0) % 2).astype(np.uint8)
    regs = model.mask_regions(checker, 4)
    assert regs.n == 2000
    with pytest.raises(ValueError, match="max_rings"):
        model.region_outlines(regs, max_rings=1999)
    want = outlines_numpy(regs.labels.cpu().numpy(), 4, regs.n)
    check(model.region_outlines(regs, max_rings=2000), want)    # a following call works; R = the cap is allowed
    with pytest.raises(ValueError, match="max_rings"):
        model.region_outlines(regs, max_rings=0)
    check(model.region_outlines(regs), want)
    model.check_errors()


@pytest.mark.parametrize("h,w", [(67, 129), (257, 259)])
def test_draw_outlines_matches_the_restatement(model, h, w):
    g = np.random.default_rng(h + w)
    blocks = np.kron(g.random((h // 9 + 1, w // 13 + 1)) < 0.6, np.ones((9, 13), np.uint8))[:h, :w].astype(np.uint8)
    blocks[h // 3:h // 3 + 40, w // 4:w // 4 + 50] = 1           # room for an interior at width 16
    regs = model.mask_regions(blocks, 4)
    labels = regs.labels.cpu().numpy()
    rgb = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for width in (1, 3, 16):
        want = draw_numpy(rgb, labels, (255, 0, 128), width)
        got = model.draw_outlines(rgb, regs, (255, 0, 128), width)
        assert got.device == torch.device(DEV) and same(got, want)
        assert (want != rgb).any() and (want[labels > 0] == rgb[labels > 0]).all(axis=1).any()        # a band, and an interior left alone
    dev = torch.from_numpy(rgb).to(DEV)
    assert same(model.draw_outlines(dev, regs.labels), draw_numpy(rgb, labels)) and same(dev, rgb)        # the input is left alone
    own = g.integers(-1, 4, (h, w)).astype(np.int32)
    assert same(model.draw_outlines(rgb, own, (1, 2, 3), 2), draw_numpy(rgb, own, (1, 2, 3), 2))


def test_c_abi(model):
    lib, h, st = _lib.load(), model._handle, _stream(torch.device(DEV))
    H, W = 12, 70
    labels = torch.ones((H, W), dtype=torch.int32, device=DEV)
    labels[3:5, 10:20] = 0
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    verts = torch.zeros((8, 2), dtype=torch.int32, device=DEV)
    rings = torch.zeros((2, NCOLS), dtype=torch.int64, device=DEV)
    r_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
    rgb = torch.full((H, W, 3), 200, dtype=torch.uint8, device=DEV)
    null = C.c_void_p(0)

    def count(l=_ptr(labels), Hh=H, Ww=W, n=1, conn=8, c=_ptr(counts), hh=h):
        return lib.keep_outline_count(hh, l, Hh, Ww, n, conn, c, st)

    def trace(l=_ptr(labels), Hh=H, Ww=W, n=1, conn=8, E=2 * (H + W) + 24, V=8, v=_ptr(verts), r=_ptr(rings), cap=2, ro=_ptr(r_dev), hh=h):
        return lib.keep_outline_trace(hh, l, Hh, Ww, n, conn, E, V, v, r, cap, ro, st)

    def draw(l=_ptr(labels), Hh=H, Ww=W, i=_ptr(rgb), o=_ptr(rgb), color=0x0000FF, width=1, hh=h):
        return lib.keep_outline_draw(hh, l, Hh, Ww, i, o, color, width, st)

    assert count() == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert counts.tolist() == [2 * (H + W) + 24, 8]
    assert trace() == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert int(r_dev[0]) == 2 and rings.tolist() == [[1, 0, 4, 2 * (H + W), 2 * H * W, 0, 0, 0], [1, 4, 4, 24, -40, 20, 3, 1]]
    assert verts.tolist() == [[0, 0], [W, 0], [W, H], [0, H], [20, 3], [10, 3], [10, 5], [20, 5]]
    rings.zero_()
    assert trace(cap=1) == _lib.KEEP_OK and trace(cap=0, r=null) == _lib.KEEP_OK      # R is still the whole count
    torch.cuda.synchronize()
    assert int(r_dev[0]) == 2 and rings[0, COL["area2"]] == 2 * H * W and not bool(rings[1].any())
    for kw in [dict(hh=None), dict(l=null), dict(c=null), dict(Hh=0), dict(Ww=-1), dict(Hh=1 << 14, Ww=(1 << 14) + 1), dict(Hh=1 << 31, Ww=1 << 31),
               dict(conn=6), dict(conn=0), dict(n=-1), dict(n=H * W + 1)]:
        assert count(**kw) == _lib.KEEP_EINVAL, kw
    for kw in [dict(hh=None), dict(l=null), dict(v=null), dict(r=null), dict(ro=null), dict(Hh=0), dict(Hh=1 << 14, Ww=(1 << 14) + 1), dict(conn=6),
               dict(n=0), dict(E=0), dict(V=0), dict(V=2 * (H + W) + 25), dict(E=4 * H * W + 1), dict(cap=-1)]:
        assert trace(**kw) == _lib.KEEP_EINVAL, kw
    assert lib.keep_last_error(h)
    # in place through the ABI: the frame of the region and the rim of its hole turn red, the rest stays
    assert draw() == _lib.KEEP_OK
    torch.cuda.synchronize()
    want = draw_numpy(np.full((H, W, 3), 200, np.uint8), labels.cpu().numpy(), (255, 0, 0), 1)
    assert same(rgb, want) and rgb[0, 0].tolist() == [255, 0, 0] and rgb[4, 15].tolist() == [200, 200, 200] and rgb[6, 30].tolist() == [200, 200, 200]
    for kw in [dict(hh=None), dict(l=null), dict(i=null), dict(o=null), dict(Hh=0), dict(Hh=1 << 14, Ww=(1 << 14) + 1), dict(color=-1),
               dict(color=1 << 24), dict(width=0), dict(width=17)]:
        assert draw(**kw) == _lib.KEEP_EINVAL, kw
    model.check_errors()


def test_end_to_end_at_depth_2(model):
    """encode_region(step = patch // 2) -> wsi.segment_heatmap -> wsi.segment_regions -> region_outlines -> draw_outlines over
    render_heatmap: the outlines equal the restatement fed with the device's own labels."""
    P, d = 224, 16
    tiles = synth_tile_family("stain_field", 0, 12, torch.device(DEV), seed=3)
    region = tiles.reshape(3, 4, P, P, 3).permute(0, 2, 1, 3, 4).reshape(3 * P, 4 * P, 3).contiguous()
    origin = (2 * P, P)
    feats, coords = model.encode_region(region, P, P // 2, origin=origin)
    shape = (region.shape[0] // d + 1, region.shape[1] // d + 2)
    gen = torch.Generator().manual_seed(1)
    classifier = torch.nn.functional.normalize(torch.randn(feats.shape[1], 2, generator=gen), dim=0).to(DEV)
    r = wsi.segment_heatmap(classifier, feats, coords, d, shape, patch_size=P, overlap=True, origin=origin, model=model)
    S, c = unpack_numpy(r.acc.cpu().numpy())
    thd = float(np.median(S[c > 0] / (65535.0 * c[c > 0])))
    lesions = wsi.segment_regions(r, thd, model=model)
    assert lesions.n > 0 and lesions.connectivity == 8
    o = model.region_outlines(lesions)
    labels = lesions.labels.cpu().numpy()
    check(o, outlines_numpy(labels, 8, lesions.n))
    assert o.downsample == d and o.origin == origin
    gj = json.loads(json.dumps(o.to_geojson(table=lesions)))
    areas = lesions.numpy()[:, TABLE_COLUMNS.index("area")]
    assert [f["properties"]["label"] for f in gj["features"]] == list(range(1, lesions.n + 1))
    assert [f["properties"]["area"] for f in gj["features"]] == areas.tolist()
    first = gj["features"][0]["geometry"]["coordinates"][0]
    assert first[0] == first[-1] == [origin[0] + d * int(lesions.first_x[0]), origin[1] + d * int(lesions.first_y[0])]
    picture = model.render_heatmap(r, None)
    drawn = model.draw_outlines(picture, lesions, (0, 0, 0), 1)
    assert same(drawn, draw_numpy(picture.cpu().numpy(), labels, (0, 0, 0), 1)) and not torch.equal(drawn, picture)
