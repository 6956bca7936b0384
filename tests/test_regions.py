"""The region table, host side: keep_amd.components.regions_numpy (the yardstick of tests/test_regions_gpu.py)
against scipy.ndimage (label, find_objects, sum_labels, center_of_mass) and against per-pixel Python-integer loops, the argument
checks and RegionTable's conversions.  No GPU."""
import numpy as np
import pytest
import torch

from keep_amd.components import (COLUMNS, NCOLS, RegionTable, check_raster, check_region_count, check_regions_args, mask_tensor,
                                 regions_numpy)
from keep_amd.heatmap import Q_ONE, TileRaster, raster_numpy, unpack_numpy
from keep_amd.region import TissueMask, TissueSegmentation, saturation_numpy, tissue_mask_numpy
from keep_amd.synth import synth_thumbnail
from test_tissue import hard_shapes

COL = {name: i for i, name in enumerate(COLUMNS)}


def structure(ndi, connectivity):
    return np.ones((3, 3)) if connectivity == 8 else ndi.generate_binary_structure(2, 1)


def masks():
    """The sweep of this file and of tests/test_regions_gpu.py: (name, uint8 [h,w])."""
    rgb = synth_thumbnail()
    yield "tissue", tissue_mask_numpy(rgb, TissueSegmentation())[0]
    yield "raw", (saturation_numpy(rgb) > 8).astype(np.uint8)
    for name, img in hard_shapes():
        yield name, img
    rings = np.zeros((41, 150), np.uint8)
    for k in range(0, 20, 2):                                  # nested rings: every other one-pixel frame
        rings[k:41 - k, k] = rings[k:41 - k, 149 - k] = rings[k, k:150 - k] = rings[40 - k, k:150 - k] = 1
    yield "rings", rings
    corner = np.zeros((16, 140), np.uint8)
    corner[0:8, 0:64] = corner[8:16, 64:128] = 1               # blocks that meet at one corner, on a 64-pixel segment border
    yield "corner", corner
    yield "zeros", np.zeros((7, 70), np.uint8)
    yield "all-ones", np.ones((13, 200), np.uint8)
    yield "checker-1px", (np.indices((30, 67)).sum(0) % 2).astype(np.uint8)


MASKS = list(masks())


def scipy_table(ndi, lab, n, h, w):
    """Columns 0..9 from scipy's own measurements of a label image."""
    t = np.zeros((n, NCOLS), np.int64)
    if n == 0:
        return t
    idx = np.arange(1, n + 1)
    ys, xs = np.indices((h, w))
    one = np.ones((h, w), np.int64)
    first = ndi.minimum(np.arange(h * w).reshape(h, w), lab, idx).astype(np.int64)
    t[:, 0], t[:, 1] = first % w, first // w
    t[:, 2] = np.rint(ndi.sum_labels(one, lab, idx))
    for i, sl in enumerate(ndi.find_objects(lab)):
        t[i, 3:7] = sl[1].start, sl[0].start, sl[1].stop, sl[0].stop
    t[:, 7], t[:, 8] = np.rint(ndi.sum_labels(xs, lab, idx)), np.rint(ndi.sum_labels(ys, lab, idx))
    edge = (xs == 0) | (ys == 0) | (xs == w - 1) | (ys == h - 1)
    t[:, 9] = ndi.maximum(edge.astype(np.int64), lab, idx)
    return t


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name,img", MASKS, ids=[n for n, _ in MASKS])
def test_restatement_matches_scipy(name, img, connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    h, w = img.shape
    lab, n = ndi.label(img, structure=structure(ndi, connectivity))
    got_lab, got = regions_numpy(img, connectivity, 1)
    assert got_lab.dtype == np.int32 and got.dtype == np.int64 and got.shape == (n, NCOLS)
    assert np.array_equal(got_lab, lab)                         # scipy's own numbering
    assert np.array_equal(got, scipy_table(ndi, lab, n, h, w))
    if n:
        cm = np.asarray(ndi.center_of_mass(img, lab, np.arange(1, n + 1)))
        assert np.allclose(RegionTable(torch.from_numpy(got)).centroid(), cm[:, ::-1] + 0.5, rtol=0, atol=1e-9)
    if name == "raw":
        assert n == (17100 if connectivity == 4 else 6365)
    for min_area in (2, 50):
        area = np.bincount(lab.ravel(), minlength=n + 1)
        keep = area >= min_area
        keep[0] = False
        relab, m = ndi.label(keep[lab], structure=structure(ndi, connectivity))       # scipy relabelled: the same order, no gaps
        cut_lab, cut = regions_numpy(img, connectivity, min_area)
        assert m == keep.sum() and np.array_equal(cut_lab, relab)
        assert np.array_equal(cut, scipy_table(ndi, relab, m, h, w))
        assert np.array_equal(cut, got[keep[1:]])               # the kept rows, in order


def test_restatement_on_the_golden_crop(golden_dir):
    ndi = pytest.importorskip("scipy.ndimage")
    Image = pytest.importorskip("PIL.Image")
    rgb = np.asarray(Image.open(golden_dir + "/example.tif"))
    img = tissue_mask_numpy(rgb, TissueSegmentation(use_otsu=True, min_hole=64, min_area=400))[0]
    for connectivity in (4, 8):
        lab, n = ndi.label(img, structure=structure(ndi, connectivity))
        got_lab, got = regions_numpy(img, connectivity)
        assert n > 0 and np.array_equal(got_lab, lab) and np.array_equal(got, scipy_table(ndi, lab, n, *img.shape))


def loop_scores(labels, n, acc):
    """Columns 10..13 by a per-pixel loop in Python integers."""
    out = [[0, 0, 0, 0] for _ in range(n)]
    for (y, x), lab in np.ndenumerate(labels):
        if lab == 0:
            continue
        a = int(acc[y, x]) & ((1 << 64) - 1)
        S, c = a & ((1 << 40) - 1), a >> 40
        if c > 0:
            r = out[lab - 1]
            r[0] += 1
            r[1] += c
            r[2] += S
            r[3] = max(r[3], (2 * S + c) // (2 * c))
    return np.asarray(out, np.int64).reshape(n, 4)


def test_score_columns_against_a_python_loop():
    g = np.random.default_rng(11)
    h, w, P, d = 40, 90, 64, 4
    coords = np.stack([g.integers(-40, w * d, 60), g.integers(-40, h * d, 60)], axis=1).astype(np.int64)        # off the lattice, overlapping
    values = g.random(60).astype(np.float32)
    acc = raster_numpy(coords, values, P, d, (h, w))
    mask = (g.random((h, w)) < 0.6).astype(np.uint8)
    mask[:, 70:] = 0
    mask[5:9, 80:85] = 1                                        # may or may not be covered
    assert (unpack_numpy(acc)[1] == 0).any() and (unpack_numpy(acc)[1] > 1).any()
    for connectivity in (4, 8):
        labels, table = regions_numpy(mask, connectivity, 1, acc)
        assert np.array_equal(table[:, 10:], loop_scores(labels, len(table), acc))
        assert (table[:, 10] < table[:, 2]).any()               # pixels with c = 0 inside a region
        assert np.array_equal(regions_numpy(mask, connectivity, 1)[1][:, :10], table[:, :10])
        assert not regions_numpy(mask, connectivity, 1)[1][:, 10:].any()


def test_peak16_rounds_half_up_on_an_exact_tie():
    # two tiles over one pixel with q = 1 and q = 2: the mean is 1.5 exactly -> 2; q = 0 and 1 -> 0.5 -> 1
    acc = np.zeros((1, 3), np.int64)
    acc[0, 0] = (2 << 40) | 3
    acc[0, 1] = (2 << 40) | 1
    acc[0, 2] = (4 << 40) | 9                                   # 2.25 -> 2
    _, t = regions_numpy(np.array([[1, 0, 1]], np.uint8), 4, 1, acc)
    assert t[:, COL["peak16"]].tolist() == [2, 2] and t[:, COL["sum_s"]].tolist() == [3, 9] and t[:, COL["sum_c"]].tolist() == [2, 4]
    _, t = regions_numpy(np.array([[0, 1, 0]], np.uint8), 4, 1, acc)
    assert t[:, COL["peak16"]].tolist() == [1]
    big = np.array([[((1 << 24) - 1 << 40) | ((1 << 24) - 1) * Q_ONE]], np.uint64).view(np.int64)      # the fields at their limits
    _, t = regions_numpy(np.ones((1, 1), np.uint8), 8, 1, big)
    assert t[0, 10:].tolist() == [1, (1 << 24) - 1, ((1 << 24) - 1) * Q_ONE, Q_ONE]


def test_table_by_hand():
    img = np.array([[0, 1, 1, 0, 0, 0],
                    [0, 1, 0, 0, 1, 0],
                    [0, 0, 0, 1, 0, 0],
                    [1, 0, 0, 0, 0, 0]], np.uint8)
    lab, t = regions_numpy(img, 8)
    assert lab.tolist() == [[0, 1, 1, 0, 0, 0], [0, 1, 0, 0, 2, 0], [0, 0, 0, 2, 0, 0], [3, 0, 0, 0, 0, 0]]
    assert t[:, :10].tolist() == [[1, 0, 3, 1, 0, 3, 2, 4, 1, 1], [4, 1, 2, 3, 1, 5, 3, 7, 3, 0], [0, 3, 1, 0, 3, 1, 4, 0, 3, 1]]
    lab4, t4 = regions_numpy(img, 4)
    assert len(t4) == 4 and lab4[1, 4] == 2 and lab4[2, 3] == 3
    lab2, t2 = regions_numpy(img, 8, 2)                         # keep iff >= 2: the single pixel goes, the pair stays
    assert len(t2) == 2 and lab2[3, 0] == 0 and np.array_equal(t2, t[:2])
    assert len(regions_numpy(img, 8, 3)[1]) == 1 and len(regions_numpy(img, 8, 4)[1]) == 0


def test_region_table_conversions_by_hand():
    t = torch.tensor([[2, 1, 4, 2, 1, 4, 3, 10, 6, 0, 3, 6, 3 * Q_ONE, Q_ONE],
                      [0, 5, 1, 0, 5, 1, 6, 0, 5, 1, 0, 0, 0, 0]], dtype=torch.int64)
    r = RegionTable(t, None, 16, (320, 640))
    assert r.n == len(r) == 2 and r.area.tolist() == [4, 1] and r.x1.tolist() == [4, 1] and r.ids.tolist() == [1, 2]
    assert r.centroid().tolist() == [[3.0, 2.0], [0.5, 5.5]]
    l0 = r.to_level0()
    assert l0["box"].tolist() == [[352.0, 656.0, 384.0, 688.0], [320.0, 720.0, 336.0, 736.0]]
    assert l0["centroid"].tolist() == [[368.0, 672.0], [328.0, 728.0]] and l0["area"].tolist() == [1024.0, 256.0]
    assert np.allclose(r.area_mm2(0.25), [1024 * 0.0625e-6, 256 * 0.0625e-6], rtol=1e-15)
    ms = r.mean_score()
    assert ms[0] == 0.5 and np.isnan(ms[1]) and r.peak_score().tolist() == [1.0, 0.0]
    s = r.sort("area", descending=False)
    assert s.ids.tolist() == [2, 1] and s.area.tolist() == [1, 4] and r.area.tolist() == [4, 1]
    assert r.sort("mean_score").ids.tolist() == [1, 2]
    with pytest.raises(ValueError):
        r.sort("perimeter")
    with pytest.raises(ValueError):
        RegionTable(t).to_level0()
    with pytest.raises(ValueError):
        RegionTable(t[:, :13])


def test_sort_keeps_integer_keys_above_2_to_53_apart():
    t = torch.zeros((3, NCOLS), dtype=torch.int64)
    t[:, COL["area"]] = 1
    t[:, COL["sum_s"]] = torch.tensor([(1 << 60) + 1, (1 << 60) + 2, 1 << 60])        # one value as float64
    r = RegionTable(t)
    assert r.sort("sum_s").ids.tolist() == [2, 1, 3] and r.sort("sum_s", descending=False).ids.tolist() == [3, 1, 2]


def test_argument_checks():
    for args in [(6, 1), (0, 1), (8.5, 1), (8, 0), (8, -3), (8, 1.5), (True, 1), (8, 1, -1)]:
        with pytest.raises(ValueError):
            check_regions_args(*args)
    assert check_regions_args(4, 7, 0) == (4, 7, 0)
    for bad in [np.ones((3,), np.uint8), np.ones((2, 3, 1), np.uint8), np.ones((2, 3), np.int32), np.ones((0, 3), np.uint8), [[1, 0]],
                torch.ones(2, 3)]:
        with pytest.raises(ValueError):
            mask_tensor(bad)
    m, d = mask_tensor(TissueMask(np.ones((4, 5), bool), 16))
    assert d == 16 and m.dtype == torch.uint8 and tuple(m.shape) == (4, 5)
    assert mask_tensor(np.ones((4, 5), bool))[1] is None
    with pytest.raises(ValueError):
        regions_numpy(np.ones((3, 3), np.uint8), 6)
    with pytest.raises(ValueError):
        regions_numpy(np.ones((3, 3), np.uint8), 8, 0)
    with pytest.raises(ValueError):
        regions_numpy(np.ones((3, 3), np.uint8), 8, 1, np.zeros((3, 4), np.int64))


def test_max_regions_and_raster_checks():
    assert check_region_count(5, 5) == 5 and check_region_count(0, 0) == 0
    with pytest.raises(ValueError, match="max_regions"):
        check_region_count(6, 5)
    r = TileRaster(torch.zeros((4, 5), dtype=torch.int64), 16, 224, tiles=100_000)
    assert check_raster(None, (4, 5), 8) == 8 and check_raster(None, (4, 5), None) is None
    assert check_raster(r, (4, 5), None) == 16 and check_raster(r, (4, 5), 16) == 16
    with pytest.raises(ValueError, match="downsample"):
        check_raster(r, (4, 5), 8)
    with pytest.raises(ValueError):
        check_raster(r, (5, 4), 16)
    with pytest.raises(ValueError):
        check_raster(np.zeros((4, 5), np.int64), (4, 5), 16)
    # the overflow bound: tiles (P // d + 1)^2 65535 < 2^63.  100 000 tiles at P = 224, d = 4 are far below it ...
    assert 100_000 * (224 // 4 + 1) ** 2 * Q_ONE < 3 * 10 ** 13
    check_raster(TileRaster(torch.zeros((4, 5), dtype=torch.int64), 4, 224, tiles=100_000), (4, 5), 4)
    # ... one tile of 2^30 level-0 pixels at d = 1 is not
    with pytest.raises(ValueError, match="int64"):
        check_raster(TileRaster(torch.zeros((4, 5), dtype=torch.int64), 1, 1 << 30, tiles=1), (4, 5), 1)
    ok = TileRaster(torch.zeros((4, 5), dtype=torch.int64), 1, (1 << 23) - 1, tiles=2)          # 2 (2^23)^2 65535 < 2^63 <= 2 (2^23)^2 65536
    check_raster(ok, (4, 5), 1)
    ok.claim(1)
    with pytest.raises(ValueError, match="int64"):
        check_raster(ok, (4, 5), 1)


def test_model_checks_arguments_before_any_device_work():
    from keep_amd import KEEPModel, wsi
    m = KEEPModel()
    ok = np.ones((4, 5), np.uint8)
    r8 = TileRaster(torch.zeros((4, 5), dtype=torch.int64), 8, 224)
    for kw in [dict(connectivity=6), dict(min_area=0), dict(max_regions=-1), dict(raster=r8.acc),
               dict(raster=TileRaster(torch.zeros((5, 4), dtype=torch.int64), 8, 224))]:
        with pytest.raises(ValueError):
            m.mask_regions(ok, **kw)
    with pytest.raises(ValueError):
        m.mask_regions(ok.astype(np.float32))
    with pytest.raises(ValueError, match="downsample"):
        m.mask_regions(TissueMask(ok, 16), raster=r8)
    with pytest.raises(ValueError):
        wsi.segment_regions(r8.acc)
    with pytest.raises(ValueError):
        wsi.segment_regions(r8, tissue=TissueMask(ok, 16))
    with pytest.raises(ValueError):
        wsi.segment_regions(r8, thd=float("nan"))
