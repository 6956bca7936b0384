"""Polygon annotations to masks on the MI355X: keep_poly_fill / keep_mask_tile_counts, KEEPModel.fill_polygons,
KEEPModel.annotation_mask, KEEPModel.mask_tile_counts.

Everything the device computes is an integer, so every comparison is exact: the yardstick is keep_amd.annotation.fill_numpy /
tile_counts_numpy, which tests/test_annotation.py holds to statements that fill nothing; the large shapes are held to closed forms and
to the masks their outlines came from."""
import ctypes as C
import itertools
import json

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel, _lib, wsi
from keep_amd.annotation import CAMELYON16_ORDER, PolygonSet, fill_numpy, tile_counts_numpy
from keep_amd.components import COLUMNS as TABLE_COLUMNS
from keep_amd.config import small_shape
from keep_amd.heatmap import unpack_numpy
from keep_amd.model import _ptr, _stream
from keep_amd.outline import RegionOutlines
from keep_amd.region import TissueMask
from keep_amd.synth import synth_state_dict, synth_tile_family
from test_annotation import CAMELYON_WANT, RULES, camelyon_paint, poly_set, random_polygon_sets, rect
from test_regions import MASKS
from test_tissue import serpentine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def model():
    m = KEEPModel(precision="strict")
    m.load_state_dict(synth_state_dict(small_shape(2, 2), seed=5), strict=True)
    return m.to(DEV).eval()


def same(t: torch.Tensor, a: np.ndarray) -> bool:
    return t.dtype == torch.from_numpy(a).dtype and tuple(t.shape) == a.shape and torch.equal(t.cpu(), torch.from_numpy(a))


def outlines_back(model, img, connectivity, d, origin=(0, 0)):
    """A mask -> (labels > 0 as uint8, the PolygonSet of its regions' outlines, traced on the device, at downsample d and origin)."""
    regs = model.mask_regions(img, connectivity)
    o = model.region_outlines(regs)
    polys = PolygonSet.from_outlines(RegionOutlines(o.rings, o.vertices, d, origin, o.n))
    return (regs.labels > 0).to(torch.uint8), polys


@pytest.mark.parametrize("name,img", MASKS, ids=[n for n, _ in MASKS])
def test_outlines_taken_back_match_the_restatement(model, name, img):
    """The sweep of tests/test_annotation.py.  There fill_numpy is held to labels > 0 on every combination; here the device is held to
    labels > 0 on every combination and to fill_numpy itself on one of them (a host fill of the largest mask takes a second)."""
    for connectivity in (4, 8):
        for k, (d, rule) in enumerate(itertools.product((1, 3, 16), RULES)):
            origin = ((0, 0), (-48, 96))[k % 2]
            want, polys = outlines_back(model, img, connectivity, d, origin)
            got = model.fill_polygons(polys, d, img.shape, origin, rule)
            assert got.device == torch.device(DEV) and got.dtype == torch.uint8 and torch.equal(got, want)
    assert same(got, fill_numpy(polys, d, img.shape, origin, rule))


def test_random_self_intersecting_sets(model):
    filled = 0
    for vertices, start, weight, d, shape, origin in random_polygon_sets():
        for rule in RULES:
            want = fill_numpy((vertices, start, weight), d, shape, origin, rule)
            assert same(model.fill_polygons((vertices, start, weight), d, shape, origin, rule), want)
            filled += int(want.sum())
    assert filled > 200


@pytest.mark.parametrize("h,w", [(1, 1), (1, 300), (300, 1), (5, 67), (67, 129), (4, 4099)])
def test_shapes_that_break_scans(model, h, w):
    """(4, 4099): a row wider than one chunk of the row scan.  The rectangle's long edges give many crossings to one edge each."""
    g = np.random.default_rng(h * 7 + w)
    for k, img in enumerate((np.ones((h, w), np.uint8), np.zeros((h, w), np.uint8), (np.indices((h, w)).sum(0) % 2).astype(np.uint8),
                             (g.random((h, w)) < 0.5).astype(np.uint8))):
        for connectivity, d in ((4, 1), (8, 16), (8, 3)):
            want, polys = outlines_back(model, img, connectivity, d)
            rule = RULES[(k + d) % 2]
            got = model.fill_polygons(polys, d, (h, w), rule=rule)
            assert same(got, img) and torch.equal(got, want)
        assert same(got, fill_numpy(polys, d, (h, w), rule=rule))
        if not img.any():
            assert len(polys) == 0 and model.last_fill_crossings == 0
    for d in (1, 16):
        roi = poly_set(rect(-5 * d, d // 2 + 1, (w + 2) * d, (h + 3) * d))                   # leaves on three sides, the top row cut
        want = fill_numpy(roi, d, (h, w))
        assert same(model.fill_polygons(roi, d, (h, w)), want)
        assert model.last_fill_crossings == 2 * (h - 1) and int(want.sum()) == (h - 1) * w


def test_circle_of_100000_vertices(model):
    """Rounded coordinates: most edges have length 0 or cross no row; part of the circle lies outside the mask."""
    t = np.arange(100_000) * (2 * np.pi / 100_000)
    ring = np.floor(np.stack([1000 + 1900 * np.cos(t), 2056 + 1900 * np.sin(t)], 1) + 0.5).astype(np.int64)
    polys = poly_set(ring)
    want = fill_numpy(polys, 16, (257, 259))
    got = model.fill_polygons(polys, 16, (257, 259))
    assert same(got, want) and 30_000 < int(want.sum()) < 257 * 259 and model.last_fill_crossings < 2 * 257
    assert same(model.fill_polygons(poly_set(ring[::-1].copy()), 16, (257, 259), rule="evenodd"), want)


def test_frame_with_a_hole_4096(model):
    """4096 x 4096 at d = 1: a square frame [a, b)^2 with the hole [c, e)^2 and a block [p, q)^2 inside the hole: closed forms, no host
    restatement at this size."""
    n, a, b, c, e, p, q = 4096, 100, 4000, 700, 3001, 1500, 1777
    polys = poly_set(rect(a, a, b, b), rect(c, c, e, e, clockwise=False), rect(p, p, q, q), roles=[1, -1, 1], features=[0, 0, 1])
    for rule in RULES:
        got = model.fill_polygons(polys, 1, (n, n), rule=rule, value=3)
        assert model.last_fill_crossings == 2 * ((b - a) + (e - c) + (q - p))
        assert int((got != 0).sum()) == (b - a) ** 2 - (e - c) ** 2 + (q - p) ** 2 and int(got.max()) == 3
        for row in (0, a - 1, a, c - 1, c, p - 1, p, q - 1, q, e - 1, e, b - 1, b, n - 1):
            want = np.zeros(n, np.uint8)
            if a <= row < b:
                want[a:b] = 3
                if c <= row < e:
                    want[c:e] = 0
                    if p <= row < q:
                        want[p:q] = 3
            assert same(got[row], want), row


def test_more_than_2_20_crossings(model):
    """The 1024 x 1024 serpentine's outline taken back at d = 1 gives the mask it came from.  Its long edges are horizontal and cross no
    row, so a transposed serpentine stands beside it: 515 columns of 1024 rows, more than 2^20 crossings in one call."""
    img = serpentine(1024, 1024)
    want, polys = outlines_back(model, img, 4, 1)
    assert same(model.fill_polygons(polys, 1, img.shape), img) and model.last_fill_crossings >= 2 * 1024
    img = np.ascontiguousarray(serpentine(1030, 1024).T)          # 515 columns; the 514 connectors join two runs of a row into one
    want, polys = outlines_back(model, img, 4, 1)
    for rule in RULES:
        assert same(model.fill_polygons(polys, 1, img.shape, rule=rule), img)
        assert model.last_fill_crossings == 2 * (515 * 1024 - 514) > 1 << 20


def test_calling_conventions(model):
    g = np.random.default_rng(8)
    vertices, start, weight = np.concatenate([rect(3, 2, 40, 30), np.array([(10, 5), (35, 12), (20, 28)], np.int64)]), np.array([0, 4, 7]), np.array([1, -1], np.int32)
    shape, d = (9, 12), 4
    base = g.integers(0, 256, shape, dtype=np.uint8)
    want = fill_numpy((vertices, start, weight), d, shape, value=255, into=base)
    assert (want == 255).sum() > 10 and (want == base).sum() > 10
    wide = np.zeros((7, 5), np.int64)
    wide[:, 1:3] = vertices
    forms = [(vertices, start, weight), (torch.from_numpy(vertices), torch.from_numpy(start), torch.from_numpy(weight)),
             (torch.from_numpy(vertices).to(DEV), torch.from_numpy(start).to(DEV), torch.from_numpy(weight).to(DEV)),
             (wide[:, 1:3], start.astype(np.int32), weight.astype(np.int64)), (torch.from_numpy(wide).to(DEV)[:, 1:3], start.tolist(), weight.tolist()),
             (np.asfortranarray(vertices), start, weight)]
    for polys in forms:
        for into in (base, torch.from_numpy(base), torch.from_numpy(base).to(DEV)):
            assert same(model.fill_polygons(polys, d, shape, value=255, into=into), want)
    dev = torch.from_numpy(base).to(DEV)
    assert same(model.fill_polygons(forms[0], d, shape, value=0, into=dev), fill_numpy(forms[0], d, shape, value=0, into=base)) and same(dev, base)
    first, again = model.fill_polygons(forms[0], d, shape, rule="evenodd"), model.fill_polygons(forms[0], d, shape, rule="evenodd")
    assert torch.equal(first, again) and same(first, fill_numpy(forms[0], d, shape, rule="evenodd"))
    # nothing to fill: into or zeros, and no crossing is launched
    none = (np.zeros((0, 2), np.int64), np.zeros(1, np.int64), np.zeros(0, np.int32))
    assert same(model.fill_polygons(none, d, shape), np.zeros(shape, np.uint8)) and model.last_fill_crossings == 0
    assert same(model.fill_polygons(none, d, shape, into=dev, value=9), base) and model.last_fill_crossings == 0
    assert same(model.fill_polygons(PolygonSet(none[0], none[1]), d, shape, into=base), base)
    away = poly_set(rect(1000, 1000, 1100, 1100))
    assert same(model.fill_polygons(away, d, shape, into=base), base) and model.last_fill_crossings == 0
    zero = (vertices, start, np.zeros(2, np.int32))              # weight 0: the rings count nothing
    assert same(model.fill_polygons(zero, d, shape, into=base), base) and model.last_fill_crossings == 0
    model.check_errors()


def test_annotation_mask_and_the_camelyon_order(model, golden_dir):
    p = PolygonSet.from_asap_xml(golden_dir + "/annotation_asap.xml")
    painted = camelyon_paint(p, lambda q, value, into: model.fill_polygons(q, 2, (8, 10), value=value, into=into))
    assert same(painted, CAMELYON_WANT)
    tm = model.annotation_mask(p, 2, (8, 10), order=CAMELYON16_ORDER, mode="center")
    assert isinstance(tm, TissueMask) and tm.downsample == 2 and tm.mode == "center" and tm.mask.device == torch.device(DEV)
    assert same(tm.mask, CAMELYON_WANT)
    everything = model.annotation_mask(p, 2, (8, 10))
    assert same(everything.mask, fill_numpy(p, 2, (8, 10))) and int(everything.mask.sum()) == int(CAMELYON_WANT.sum()) + 4


def test_c_abi(model):
    lib, h, st = _lib.load(), model._handle, _stream(torch.device(DEV))
    H, W, d = 12, 70, 2
    ring = rect(10, 4, 100, 20)
    v = torch.from_numpy(ring).to(DEV)
    rs = torch.tensor([0, 4], dtype=torch.int64, device=DEV)
    wt = torch.tensor([1], dtype=torch.int32, device=DEV)
    out = torch.full((H, W), 7, dtype=torch.uint8, device=DEV)
    crossings = C.c_int64(-1)
    null = C.c_void_p(0)

    def fill(hh=h, vp=_ptr(v), V=4, rp=_ptr(rs), R=1, wp=_ptr(wt), dd=d, Hh=H, Ww=W, ox=0, oy=0, rule=0, value=9, into=_ptr(out), o=_ptr(out),
             c=C.byref(crossings)):
        return lib.keep_poly_fill(hh, vp, V, rp, R, wp, dd, Hh, Ww, ox, oy, rule, value, into, o, c, st)

    want = fill_numpy((ring, [0, 4], [1]), d, (H, W), value=9, into=np.full((H, W), 7, np.uint8))
    assert fill() == _lib.KEEP_OK                                 # out aliases into
    torch.cuda.synchronize()
    assert same(out, want) and crossings.value == 16 and (want == 9).sum() == 8 * 45 and (want == 7).any()
    for kw in [dict(hh=None), dict(vp=null), dict(rp=null), dict(wp=null), dict(o=null), dict(dd=0), dict(dd=4097), dict(Hh=0), dict(Ww=0),
               dict(Hh=1 << 14, Ww=1 << 14), dict(Hh=1 << 31, Ww=1 << 31), dict(ox=(1 << 26) + 1), dict(oy=-(1 << 26) - 1), dict(rule=2), dict(rule=-1),
               dict(value=256), dict(value=-1), dict(V=-1), dict(V=(1 << 24) + 1), dict(R=(1 << 20) + 1), dict(V=2), dict(V=4, R=2), dict(V=4, R=0),
               dict(vp=C.c_void_p(v.data_ptr() + 4))]:
        assert fill(**kw) == _lib.KEEP_EINVAL, kw
    assert lib.keep_last_error(h)
    torch.cuda.synchronize()
    assert same(out, want)                                        # a refused call writes nothing
    assert fill(into=null, value=1, c=None) == _lib.KEEP_OK       # a good call follows; no into: zeros outside
    torch.cuda.synchronize()
    assert same(out, fill_numpy((ring, [0, 4], [1]), d, (H, W)))
    assert fill(V=0, R=0, vp=null, rp=null, wp=null, into=null) == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert crossings.value == 0 and not bool(out.any())
    # arrays that break the precondition add nothing and touch nothing else: a ring_start that does not enclose its vertices
    bad = torch.tensor([3, 4], dtype=torch.int64, device=DEV)
    assert fill(rp=_ptr(bad), into=null) == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert crossings.value == 0 and not bool(out.any())

    mask = torch.ones((H, W), dtype=torch.uint8, device=DEV)
    coords = torch.tensor([[0, 0], [130, 20], [-8, -8]], dtype=torch.int64, device=DEV)
    counts = torch.full((3, 2), -1, dtype=torch.int32, device=DEV)

    def tiles(hh=h, m=_ptr(mask), Hh=H, Ww=W, dd=d, ox=0, oy=0, c=_ptr(coords), N=3, patch=8, o=_ptr(counts)):
        return lib.keep_mask_tile_counts(hh, m, Hh, Ww, dd, ox, oy, c, N, patch, o, st)

    assert tiles() == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert counts.tolist() == [[16, 16], [8, 8], [0, 0]]
    for kw in [dict(hh=None), dict(m=null), dict(c=null), dict(o=null), dict(Hh=0), dict(Hh=1 << 16, Ww=1 << 15), dict(dd=0), dict(dd=(1 << 30) + 1),
               dict(patch=0), dict(patch=(1 << 30) + 1), dict(ox=(1 << 40) + 1), dict(N=-1), dict(N=1 << 24)]:
        assert tiles(**kw) == _lib.KEEP_EINVAL, kw
    assert tiles(N=0, c=null, o=null) == _lib.KEEP_OK and tiles() == _lib.KEEP_OK
    model.check_errors()


@pytest.mark.parametrize("d,patch", [(1, 16), (1, 224), (16, 16), (16, 224)])
def test_tile_counts(model, d, patch):
    g = np.random.default_rng(d * 1000 + patch)
    h, w = 300, 400
    mask = ((g.random((h, w)) < 0.4) * g.integers(1, 256, (h, w))).astype(np.uint8)
    origin = (0, 0) if patch == 16 else (-3 * d, 5 * d)
    x = g.integers(origin[0] - 2 * patch, origin[0] + w * d + patch, 5000)
    y = g.integers(origin[1] - 2 * patch, origin[1] + h * d + patch, 5000)
    coords = np.stack([x, y], 1).astype(np.int64)
    coords[:3] = [[origin[0] - 3 * patch, origin[1] + 5], [origin[0] + w * d, origin[1]], [origin[0], origin[1]]]
    want = tile_counts_numpy(mask, coords, patch, d, origin)
    assert want[0].tolist() == [0, 0] and want[1].tolist() == [0, 0] and want[2, 0] > 0 and (want[:, 0] == 0).sum() >= 2
    got = model.mask_tile_counts(mask, coords, patch, d, origin)
    assert got.device == torch.device(DEV) and same(got, want)
    assert same(model.mask_tile_counts(torch.from_numpy(mask).to(DEV), torch.from_numpy(coords).to(DEV), patch, d, origin), want)
    if origin == (0, 0):
        tm = TissueMask(mask, d)
        assert same(model.mask_tile_counts(tm, coords.astype(np.int32), patch), tile_counts_numpy(tm, coords, patch))
        assert same(model.mask_tile_counts(mask != 0, coords, patch, d), tile_counts_numpy(mask != 0, coords, patch, d))
    assert tuple(model.mask_tile_counts(mask, np.zeros((0, 2), np.int64), patch, d).shape) == (0, 2)


def test_end_to_end_at_depth_2(model):
    """encode_region -> wsi.segment_heatmap -> wsi.segment_regions -> region_outlines -> to_geojson -> json -> PolygonSet.from_geojson ->
    annotation_mask: the lesions come back as the mask they were, and the mask works wherever a TissueMask does."""
    P, d = 224, 16
    tiles = synth_tile_family("stain_field", 0, 12, torch.device(DEV), seed=3)
    region = tiles.reshape(3, 4, P, P, 3).permute(0, 2, 1, 3, 4).reshape(3 * P, 4 * P, 3).contiguous()
    feats, coords = model.encode_region(region, P, P // 2)
    shape = (region.shape[0] // d + 1, region.shape[1] // d + 2)
    gen = torch.Generator().manual_seed(1)
    classifier = torch.nn.functional.normalize(torch.randn(feats.shape[1], 2, generator=gen), dim=0).to(DEV)
    r = wsi.segment_heatmap(classifier, feats, coords, d, shape, patch_size=P, overlap=True, model=model)
    S, c = unpack_numpy(r.acc.cpu().numpy())
    thd = float(np.median(S[c > 0] / (65535.0 * c[c > 0])))
    lesions = wsi.segment_regions(r, thd, model=model)
    assert lesions.n > 0
    o = model.region_outlines(lesions)
    polys = PolygonSet.from_geojson(json.loads(json.dumps(o.to_geojson(table=lesions))))
    assert polys.n_features == lesions.n and polys.group == [str(l) for l in range(1, lesions.n + 1)]
    for rule in RULES:
        tm = model.annotation_mask(polys, d, shape, rule=rule)
        assert torch.equal(tm.mask, (lesions.labels > 0).to(torch.uint8)) and tm.downsample == d
    own = TissueMask((lesions.labels > 0).to(torch.uint8), d)
    for patch in (P, 32):
        got = model.region_grid(region, patch, tissue=tm)
        assert torch.equal(got, model.region_grid(region, patch, tissue=own)) and (patch == P or 0 < len(got))
    again = model.mask_regions(tm, lesions.connectivity)
    area = TABLE_COLUMNS.index("area")
    assert again.n == lesions.n and np.array_equal(again.numpy()[:, area], lesions.numpy()[:, area]) and again.downsample == d
    assert torch.equal(model.render_heatmap(r, None, tissue=tm), model.render_heatmap(r, None, tissue=own))
    f2, c2 = model.encode_region(region, P, tissue=tm)
    assert torch.equal(c2, model.region_grid(region, P, tissue=own)) and f2.shape[0] == c2.shape[0]
    counts = model.mask_tile_counts(tm, coords, P)
    assert same(counts, tile_counts_numpy(own, coords.cpu().numpy(), P)) and int(counts[:, 1].max()) > 0
    model.check_errors()
