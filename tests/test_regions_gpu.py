"""The region table on the MI355X: keep_regions_label / keep_regions_table, KEEPModel.mask_regions,
wsi.segment_regions.

Everything the device computes is an integer, so every comparison is exact: the yardstick is keep_amd.components.regions_numpy,
which tests/test_regions.py holds to scipy.ndimage and to per-pixel loops; where min_area = 1 the labels are held to
scipy.ndimage.label directly."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel, _lib, wsi
from keep_amd.components import COLUMNS, NCOLS, RegionTable, regions_numpy
from keep_amd.config import small_shape
from keep_amd.heatmap import TileRaster, quantize, raster_numpy, unpack_numpy
from keep_amd.model import _ptr, _stream
from keep_amd.region import TissueMask, TissueSegmentation, tissue_mask_numpy
from keep_amd.synth import synth_state_dict, synth_tile_family
from test_regions import MASKS, structure

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


def check(regs: RegionTable, want):
    labels, table = want
    assert regs.table.device == torch.device(DEV) and regs.n == len(table)
    assert same(regs.labels, labels)
    assert same(regs.table, table)


@pytest.mark.parametrize("name,img", MASKS, ids=[n for n, _ in MASKS])
def test_labels_and_table_match_the_restatement(model, name, img):
    ndi = pytest.importorskip("scipy.ndimage")
    dev = torch.from_numpy(img).to(DEV)
    for connectivity, min_area in itertools.product((4, 8), (1, 2, 50)):
        regs = model.mask_regions(dev, connectivity, min_area)
        check(regs, regions_numpy(img, connectivity, min_area))
        if min_area == 1:
            lab, n = ndi.label(img, structure=structure(ndi, connectivity))
            assert regs.n == n and same(regs.labels, lab.astype(np.int32))


def test_labels_and_table_on_the_golden_crop(model, golden_dir):
    """The sweep's last member, the mask of tests/golden/example.tif, built as tests/test_regions.py builds it."""
    ndi = pytest.importorskip("scipy.ndimage")
    Image = pytest.importorskip("PIL.Image")
    rgb = np.asarray(Image.open(golden_dir + "/example.tif"))
    img = tissue_mask_numpy(rgb, TissueSegmentation(use_otsu=True, min_hole=64, min_area=400))[0]
    dev = torch.from_numpy(img).to(DEV)
    for connectivity, min_area in itertools.product((4, 8), (1, 2, 50)):
        regs = model.mask_regions(dev, connectivity, min_area)
        check(regs, regions_numpy(img, connectivity, min_area))
        if min_area == 1:
            lab, n = ndi.label(img, structure=structure(ndi, connectivity))
            assert n > 0 and regs.n == n and same(regs.labels, lab.astype(np.int32))


def test_input_forms(model):
    g = np.random.default_rng(5)
    img = (g.random((45, 203)) < 0.5).astype(np.uint8)
    want = regions_numpy(img, 8, 3)
    forms = [img, img.astype(bool), img * 255, torch.from_numpy(img), torch.from_numpy(img.astype(bool)), torch.from_numpy(img).to(DEV),
             torch.from_numpy(img.astype(bool)).to(DEV), torch.from_numpy(np.concatenate([img, img], 1)).to(DEV)[:, :203],        # a strided view
             np.asfortranarray(img)]
    for m in forms:
        check(model.mask_regions(m, 8, 3), want)
    tm = model.mask_regions(TissueMask(img, 16, "center"), 8, 3)
    check(tm, want)
    assert tm.downsample == 16 and tm.origin == (0, 0) and model.mask_regions(img, 8, 3).downsample is None
    no_labels = model.mask_regions(img, 8, 3, labels=False)
    assert no_labels.labels is None and same(no_labels.table, want[1])
    assert torch.equal(tm.area, tm.table[:, COL["area"]]) and tm.ids.tolist() == list(range(1, tm.n + 1))


def raster_case(d, P, step, shape, seed, lattice):
    g = np.random.default_rng(seed)
    h, w = shape
    if lattice:                                                # tiles every `step` on the pixel lattice: (P / step)^2 tiles per pixel inside
        xs, ys = np.meshgrid(np.arange(0, w * d * 3 // 4, step), np.arange(0, h * d * 3 // 4, step))
        coords = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.int64)
    else:
        coords = np.stack([g.integers(-P, w * d * 3 // 4, 150), g.integers(-P, h * d, 150)], axis=1).astype(np.int64)
    values = g.random(len(coords)).astype(np.float32)
    values[g.random(len(coords)) < 0.1] = np.float32(1.0)
    values[g.random(len(coords)) < 0.05] = np.nan
    return coords, values


@pytest.mark.parametrize("d,P,step,lattice", [(4, 64, 0, False), (16, 224, 0, False), (4, 64, 32, True), (16, 256, 64, True)])
def test_with_a_raster(model, d, P, step, lattice):
    shape = (75, 211)                                          # neither a multiple of 4 rows nor of 64 columns
    coords, values = raster_case(d, P, step, shape, d + P, lattice)
    acc = raster_numpy(coords, values, P, d, shape)
    count = unpack_numpy(acc)[1]
    if lattice:
        assert int(count.max()) == (P // step) ** 2
    g = np.random.default_rng(P)
    blocks = np.kron(g.random((shape[0] // 5 + 1, shape[1] // 7 + 1)) < 0.55, np.ones((5, 7), np.uint8))[:shape[0], :shape[1]].astype(np.uint8)
    blocks[:, 165:] = 0
    blocks[10:20, 190:205] = 1                                 # right of every lattice tile: a region with no covered pixel when lattice
    r = model.tile_raster(coords, values, P, d, shape)
    assert same(r.acc, acc)
    for connectivity, min_area in ((8, 1), (4, 1), (8, 40)):
        want = regions_numpy(blocks, connectivity, min_area, acc)
        regs = model.mask_regions(torch.from_numpy(blocks).to(DEV), connectivity, min_area, raster=r)
        check(regs, want)
        assert regs.downsample == d
        again = model.mask_regions(torch.from_numpy(blocks).to(DEV), connectivity, min_area, raster=r)
        assert torch.equal(again.table, regs.table) and torch.equal(again.labels, regs.labels)        # two runs are equal
        t = want[1]
        assert (t[:, COL["covered"]] < t[:, COL["area"]]).any() and t[:, COL["sum_c"]].max() > 0
        if lattice:
            assert (t[:, COL["covered"]] == 0).any()
        ms, pk = regs.mean_score(), regs.peak_score()
        on = t[:, COL["sum_c"]] > 0
        assert np.isnan(ms[~on]).all() and (ms[on] <= pk[on] + 1 / 65535).all() and (pk <= 1).all()
    with pytest.raises(ValueError, match="downsample"):
        model.mask_regions(TissueMask(blocks, d + 1), raster=r)
    with pytest.raises(ValueError):
        model.mask_regions(blocks[:-1], raster=r)
    host = TileRaster(torch.from_numpy(acc), d, P, tiles=len(coords))
    with pytest.raises(ValueError, match="lives on"):
        model.mask_regions(blocks, raster=host)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 63), (3, 64), (5, 65), (130, 1), (2, 1025), (257, 129), (67, 4099)])
def test_odd_shapes(model, h, w):
    g = np.random.default_rng(h * 7 + w)
    for density in (0.35, 0.62, 1.0):
        img = (g.random((h, w)) < density).astype(np.uint8)
        acc = raster_numpy(np.stack([g.integers(0, w * 4, 20), g.integers(0, h * 4, 20)], axis=1).astype(np.int64),
                           g.random(20).astype(np.float32), 32, 4, (h, w))
        r = model.tile_raster(torch.zeros((0, 2), dtype=torch.int64), torch.zeros(0), 32, 4, (h, w))
        r.acc.copy_(torch.from_numpy(acc))
        for connectivity in (4, 8):
            check(model.mask_regions(img, connectivity, 1, raster=r), regions_numpy(img, connectivity, 1, acc))


def test_frame_with_a_hole_4096(model):
    """A 4096 x 4096 mask: a square frame [a, b)^2 without the hole [c, e)^2, and a block inside the hole: closed forms."""
    n, a, b, c, e, p, q = 4096, 100, 4000, 700, 3001, 1500, 1777
    mask = torch.zeros((n, n), dtype=torch.uint8, device=DEV)
    mask[a:b, a:b] = 1
    mask[c:e, c:e] = 0
    mask[p:q, p:q] = 1
    tri = lambda lo, hi: (lo + hi - 1) * (hi - lo) // 2         # sum of lo .. hi - 1
    frame_area = (b - a) ** 2 - (e - c) ** 2
    frame_sum = tri(a, b) * (b - a) - tri(c, e) * (e - c)
    want = np.array([[a, a, frame_area, a, a, b, b, frame_sum, frame_sum, 0, 0, 0, 0, 0],
                     [p, p, (q - p) ** 2, p, p, q, q, tri(p, q) * (q - p), tri(p, q) * (q - p), 0, 0, 0, 0, 0]], np.int64)
    for connectivity in (4, 8):
        regs = model.mask_regions(mask, connectivity)
        assert same(regs.table, want)
        lab = regs.labels
        assert int((lab == 1).sum()) == frame_area and int((lab == 2).sum()) == (q - p) ** 2 and int(lab.max()) == 2
        assert torch.equal(lab != 0, mask != 0) and int(lab[p, p]) == 2 and int(lab[a, a]) == 1
    only = model.mask_regions(mask, 8, (q - p) ** 2 + 1, labels=False)
    assert same(only.table, want[:1])


def test_all_ones_8192(model):
    n = 8192
    regs = model.mask_regions(torch.ones((n, n), dtype=torch.uint8, device=DEV), 4)
    s = (n - 1) * n // 2 * n
    assert same(regs.table, np.array([[0, 0, n * n, 0, 0, n, n, s, s, 1, 0, 0, 0, 0]], np.int64))
    assert n * n == 1 << 26 and bool((regs.labels == 1).all())


def test_no_regions_and_the_cap(model):
    for img, min_area in ((np.zeros((9, 70), np.uint8), 1), (np.ones((9, 70), np.uint8), 9 * 70 + 1)):
        regs = model.mask_regions(img, 8, min_area)
        assert regs.n == 0 and tuple(regs.table.shape) == (0, NCOLS) and regs.table.dtype == torch.int64
        assert regs.labels.dtype == torch.int32 and not bool(regs.labels.any())
        assert regs.centroid().shape == (0, 2) and regs.mean_score().shape == (0,)
    checker = (np.indices((40, 100)).sum(0) % 2).astype(np.uint8)
    with pytest.raises(ValueError, match="max_regions"):
        model.mask_regions(checker, 4, max_regions=1999)
    check(model.mask_regions(checker, 4, max_regions=2000), regions_numpy(checker, 4))         # a following call works; n = the cap is allowed
    assert model.mask_regions(checker, 8).n == 1
    with pytest.raises(ValueError, match="max_regions"):
        model.mask_regions(checker, 4, max_regions=0)
    model.check_errors()


def test_segment_regions_end_to_end_at_depth_2(model):
    """encode_region(step = patch // 2) -> wsi.segment_heatmap -> wsi.segment_regions equals the restatement fed with the device's
    own raster."""
    P, d = 224, 16
    tiles = synth_tile_family("stain_field", 0, 12, torch.device(DEV), seed=3)
    region = tiles.reshape(3, 4, P, P, 3).permute(0, 2, 1, 3, 4).reshape(3 * P, 4 * P, 3).contiguous()
    origin = (2 * P, P)
    feats, coords = model.encode_region(region, P, P // 2, origin=origin)
    shape = (region.shape[0] // d + 1, region.shape[1] // d + 2)
    gen = torch.Generator().manual_seed(1)
    classifier = torch.nn.functional.normalize(torch.randn(feats.shape[1], 2, generator=gen), dim=0).to(DEV)
    r = wsi.segment_heatmap(classifier, feats, coords, d, shape, patch_size=P, overlap=True, origin=origin, model=model)
    acc = r.acc.cpu().numpy()
    S, c = unpack_numpy(acc)
    S, c = S.astype(np.int64), c.astype(np.int64)
    thd = float(np.median((S[c > 0] / (65535.0 * c[c > 0]))))
    tissue = np.ones(shape, np.uint8)
    tissue[:, shape[1] // 2] = 0                                # a tissue mask that cuts the slide in two
    for kw, mask in [(dict(), (c > 0) & (S > quantize(thd) * c)),
                     (dict(tissue=TissueMask(tissue, d), connectivity=4, min_area=3), (c > 0) & (S > quantize(thd) * c) & (tissue != 0))]:
        regs = wsi.segment_regions(r, thd, model=model, **kw)
        want = regions_numpy(mask, kw.get("connectivity", 8), kw.get("min_area", 1), acc)
        check(regs, want)
        assert 0 < mask.mean() < 1 and regs.n > 0 and regs.downsample == d and regs.origin == origin
        assert (want[1][:, COL["covered"]] == want[1][:, COL["area"]]).all()
        assert (regs.mean_score() > thd - 1e-4).all()
        l0 = regs.to_level0()
        assert (l0["box"][:, 0] >= origin[0]).all() and (l0["box"][:, 1] >= origin[1]).all()
    nothing = wsi.segment_regions(r, 1.0, model=model)
    assert nothing.n == 0


def test_c_abi_argument_checks(model):
    lib, h, st = _lib.load(), model._handle, _stream(torch.device(DEV))
    H, W = 12, 70
    mask = torch.ones((H, W), dtype=torch.uint8, device=DEV)
    labels = torch.zeros((H, W), dtype=torch.int32, device=DEV)
    n_dev = torch.zeros(2, dtype=torch.int64, device=DEV)
    acc = torch.zeros((H, W + 1), dtype=torch.int64, device=DEV)
    table = torch.zeros((3, NCOLS), dtype=torch.int64, device=DEV)
    null = C.c_void_p(0)

    def off(t, nbytes):
        return C.c_void_p(t.data_ptr() + nbytes)

    def label(m=_ptr(mask), Hh=H, Ww=W, conn=8, area=1, l=_ptr(labels), n=_ptr(n_dev)):
        return lib.keep_regions_label(h, m, Hh, Ww, conn, area, l, n, st)

    def tab(l=_ptr(labels), Hh=H, Ww=W, n=1, a=_ptr(acc), t=_ptr(table)):
        return lib.keep_regions_table(h, l, Hh, Ww, n, a, t, st)

    assert label() == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert int(n_dev[0]) == 1 and bool((labels == 1).all())
    for kw in [dict(m=null), dict(l=null), dict(n=null), dict(Hh=0), dict(Ww=0), dict(Hh=-1), dict(Hh=1 << 16, Ww=(1 << 14) + 1),
               dict(Hh=1 << 31, Ww=1 << 31), dict(conn=6), dict(conn=0), dict(conn=-8), dict(area=0), dict(area=-5)]:
        assert label(**kw) == _lib.KEEP_EINVAL, kw
        assert lib.keep_last_error(h)
    assert label(area=1 << 40) == _lib.KEEP_OK                  # larger than any component: every one is dropped
    torch.cuda.synchronize()
    assert int(n_dev[0]) == 0 and not bool(labels.any())
    assert label(conn=4) == _lib.KEEP_OK and tab() == _lib.KEEP_OK and tab(a=null) == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert table[0].tolist() == [0, 0, H * W, 0, 0, W, H, (W - 1) * W // 2 * H, (H - 1) * H // 2 * W, 1, 0, 0, 0, 0]
    for kw in [dict(l=null), dict(t=null), dict(Hh=0), dict(Ww=-2), dict(Hh=1 << 16, Ww=(1 << 14) + 1), dict(n=-1), dict(a=off(acc, 4)),
               dict(n=H * W + 1)]:
        assert tab(**kw) == _lib.KEEP_EINVAL, kw
        assert lib.keep_last_error(h)
    assert tab(n=0, t=null) == _lib.KEEP_OK                     # nothing to write is no error
    assert tab(a=off(acc, 8)) == _lib.KEEP_OK                   # aligned to its element
    # labels outside 1..n are background: no row of the table is theirs
    labels[0, :5] = 7
    labels[1, :5] = -3
    assert tab(a=null) == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert int(table[0, COL["area"]]) == H * W - 10 and not bool(table[1:].any())
    assert lib.keep_regions_label(None, _ptr(mask), H, W, 8, 1, _ptr(labels), _ptr(n_dev), st) == _lib.KEEP_EINVAL
    assert lib.keep_regions_table(None, _ptr(labels), H, W, 1, null, _ptr(table), st) == _lib.KEEP_EINVAL
    model.check_errors()
