"""Lesion-level scoring on the MI355X: keep_mask_dist2 / keep_raster_peaks / keep_lesion_hits,
KEEPModel.mask_distance / dilate_mask / erode_mask / evaluation_mask / raster_peaks / lesion_hits, FrocAccumulator and
wsi.segment_lesions / eval_seg_froc.

Everything the device computes is an integer, so every comparison is exact: the yardsticks are the numpy restatements of
keep_amd.lesion, which tests/test_lesion.py holds to scipy and to brute force, and scipy itself where the issue names it."""
import math

import numpy as np
import pytest
import torch
from scipy import ndimage

from keep_amd import KEEPModel, wsi
from keep_amd.annotation import fill_numpy
from keep_amd.config import small_shape
from keep_amd.evaluation import mean16_numpy
from keep_amd.heatmap import quantize
from keep_amd.lesion import (EvaluationMask, FrocAccumulator, camelyon16_margin, candidates_numpy, dist2_numpy, distance_threshold, froc_numpy,
                             lesion_hits_numpy, peaks_numpy)
from keep_amd.region import TissueMask
from keep_amd.synth import synth_state_dict
from test_annotation import poly_set, rect

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THRESHOLDS = [camelyon16_margin(), 2.0, 5.0, math.sqrt(13)]


@pytest.fixture(scope="module")
def model():
    m = KEEPModel(precision="strict")
    m.load_state_dict(synth_state_dict(small_shape(2, 2), seed=5), strict=True)
    return m.to(DEV).eval()


def same(t: torch.Tensor, a: np.ndarray) -> bool:
    if t.dtype == torch.uint32:
        t, a = t.view(torch.int32), a.view(np.int32)
    return t.dtype == torch.from_numpy(a).dtype and tuple(t.shape) == a.shape and torch.equal(t.cpu(), torch.from_numpy(a))


def masks_of(h, w, g):
    return [("empty", np.zeros((h, w), np.uint8)), ("full", np.full((h, w), 255, np.uint8)),
            ("checkerboard", (np.indices((h, w)).sum(0) % 2).astype(np.uint8)), ("random", (g.random((h, w)) < 0.02).astype(np.uint8))]


# ------------------------------------------------------------------------------------------------ distance
@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (67, 129), (4, 4099), (1030, 1027)])
def test_mask_distance_equals_the_restatement(model, shape):
    """(1, 300) / (4, 4099) / (1030, 1027): row segments of 256 with halos that cross their boundaries; (300, 1) and (1, 1): several rows in
    one block; R = 64 on (67, 129) and R = 1024: a halo wider than the image; empty / full: the sentinel everywhere in one direction."""
    g = np.random.default_rng(shape[0] + shape[1])
    radii = [1, 2, 5, 64] + ([1024] if shape in ((300, 1), (67, 129)) else [])
    for name, m in masks_of(*shape, g):
        md = torch.from_numpy(m).to(DEV)
        for R in radii:
            for to in ("foreground", "background"):
                want = dist2_numpy(m, R, to)
                got = model.mask_distance(md, R, to)
                assert got.device == torch.device(DEV) and same(got, want), (name, R, to)
                if name in ("empty", "full") and (name == "empty") == (to == "foreground"):
                    assert int(want.min()) == R * R + 1
    assert same(model.mask_distance(m != 0, 5), dist2_numpy(m, 5))           # a bool array from the host
    assert same(model.mask_distance(TissueMask(m, 4), 2, "background"), dist2_numpy(m, 2, "background"))


@pytest.mark.parametrize("T", THRESHOLDS)
def test_dilate_and_erode_equal_scipy_edt(model, T):
    g = np.random.default_rng(int(T * 1000))
    for shape in ((67, 129), (300, 1)):
        m = (g.random(shape) < 0.02).astype(np.uint8)
        got = model.dilate_mask(TissueMask(m, 8, "center"), T)
        assert isinstance(got, TissueMask) and (got.downsample, got.mode) == (8, "center") and got.mask.device == torch.device(DEV)
        assert same(got.mask, (ndimage.distance_transform_edt(m == 0) < T).astype(np.uint8))
        big = (g.random(shape) < 0.9).astype(np.uint8)
        big[:, 0] = 0                                                    # scipy needs a background pixel to measure from
        got = model.erode_mask(torch.from_numpy(big).to(DEV), T)
        assert got.downsample == 1 and same(got.mask, (ndimage.distance_transform_edt(big != 0) >= T).astype(np.uint8))
    full = np.ones((5, 7), np.uint8)
    assert same(model.erode_mask(full, T).mask, full) and same(model.dilate_mask(1 - full, T).mask, 1 - full)      # nothing to measure from
    R, k = distance_threshold(T)
    assert same(model.dilate_mask(m, T).mask, (dist2_numpy(m, R) <= k).astype(np.uint8))


def test_distance_errors(model):
    m = np.ones((4, 4), np.uint8)
    for bad in (0, 1025, 1.5):
        with pytest.raises(ValueError):
            model.mask_distance(m, bad)
    with pytest.raises(ValueError):
        model.mask_distance(m, 3, "inside")
    with pytest.raises(ValueError):
        model.mask_distance(m.astype(np.int32), 3)
    for bad in (0.0, -2.0, 1024.5):
        with pytest.raises(ValueError):
            model.dilate_mask(m, bad)


# ------------------------------------------------------------------------------------------------ peaks
def tile_raster_of(model, shape, g, d=4, patch=32, step=16):
    """Overlapping tiles over the raster: plateaus of 4 x 4 raster pixels with equal sums side by side, values that quantise to 0 and to
    65535, tiles left out (uncovered pixels) and NaN tiles."""
    h, w = shape
    xs, ys = np.arange(-patch + d, w * d, step), np.arange(-patch + d, h * d, step)
    coords = np.stack(np.meshgrid(xs, ys, indexing="xy"), -1).reshape(-1, 2).astype(np.int64)
    coords = coords[g.random(len(coords)) < 0.5]
    v = g.choice(np.array([0.0, 1e-7, 0.25, 0.5, 0.93, 0.97, 1.0, 1.5, np.nan], np.float32), len(coords))
    return model.tile_raster(coords, v, patch, d, shape, origin=(8, -4))


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (67, 129), (1030, 1027)])
def test_raster_peaks_equal_the_restatement(model, shape):
    g = np.random.default_rng(shape[0] * 7 + shape[1])
    raster = tile_raster_of(model, shape, g)
    acc = raster.acc.cpu().numpy()
    means = set(np.unique(mean16_numpy(acc)).tolist())
    tissue = (g.random(shape) < 0.7).astype(np.uint8)
    total = 0
    for r in (1, 2, 7, 127):
        for min_score, min16 in ((0.0, 0), (0.9, quantize(0.9))):
            for tm in (None, tissue):
                want = candidates_numpy(peaks_numpy(acc, r, min16, tm), raster.downsample, raster.origin)
                got = model.raster_peaks(raster, r, min_score, None if tm is None else TissueMask(tm, raster.downsample))
                assert got.xy.device == torch.device(DEV)
                assert same(got.xy, want.xy) and same(got.scores, want.scores) and same(got.m16, want.m16), (r, min_score, tm is None)
                total += len(got)
    if shape[0] * shape[1] > 1000:
        assert total > 50 and {0, 65535, 65536} <= means                 # peaks; means of 0 and 65535 under tiles; uncovered pixels
    got = wsi.segment_lesions(raster, 2, 0.0)
    n = len(got)
    assert same(got.xy, candidates_numpy(peaks_numpy(acc, 2), raster.downsample, raster.origin).xy)
    if n > 1:
        with pytest.raises(ValueError, match=f"has {n} peaks, max_peaks is {n - 1}"):
            model.raster_peaks(raster, 2, 0.0, max_peaks=n - 1)
        with pytest.raises(ValueError, match=f"has {n} peaks, max_peaks is 0"):
            model.raster_peaks(raster, 2, 0.0, max_peaks=0)
        assert len(model.raster_peaks(raster, 2, 0.0, max_peaks=n)) == n


def test_raster_peaks_errors(model):
    raster = model.tile_raster(np.array([[0, 0]]), np.array([0.7], np.float32), 16, 4, (8, 8))
    for bad in (0, 128, 2.5):
        with pytest.raises(ValueError):
            model.raster_peaks(raster, bad)
    with pytest.raises(ValueError):
        model.raster_peaks(raster.acc, 2)
    with pytest.raises(ValueError):
        model.raster_peaks(raster, 2, tissue=TissueMask(np.ones((8, 8), np.uint8), 8))
    with pytest.raises(ValueError):
        model.raster_peaks(raster, 2, max_peaks=-1)
    assert model.raster_peaks(raster, 2).xy.tolist() == [[2, 2]]


# ------------------------------------------------------------------------------------------------ hits
def label_images():
    one = np.ones((90, 110), np.int32)
    yy, xx = np.indices((213, 213))
    on = (yy % 3 < 2) & (xx % 3 < 2)
    many = np.where(on, (yy // 3) * 71 + xx // 3 + 1, 0).astype(np.int32)           # 71 x 71 = 5041 lesions of 2 x 2 pixels
    many[0, 0], many[1, 1] = 6000, -3                                               # not labels
    return [("one", one, 1), ("many", many, 5041)]


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 4097, 70001])
def test_lesion_hits_equal_the_restatement(model, N):
    g = np.random.default_rng(N)
    d, origin = 8, (-160, 24)
    for name, lab, n in label_images():
        h, w = lab.shape
        if name == "one":                                                           # every candidate inside the one lesion: contention
            xy = np.stack([g.integers(origin[0], origin[0] + w * d, N), g.integers(origin[1], origin[1] + h * d, N)], 1)
        else:                                                                        # outside on every side, negative coordinates
            xy = np.stack([g.integers(origin[0] - 40, origin[0] + w * d + 40, N), g.integers(origin[1] - 40, origin[1] + h * d + 40, N)], 1)
        s = g.choice(np.array([np.nan, -0.0, -0.5, 0.0, 1e-40, 0.125, 0.5, 1.0, 3.0], np.float32), N)
        s = np.where(g.random(N) < 0.5, g.random(N, dtype=np.float32), s).astype(np.float32)
        wants = []
        for ignore in (None, ((g.random(n) < 0.3) | (n == 1)).astype(np.uint8)):
            em = EvaluationMask(torch.from_numpy(lab).to(DEV), n, None, torch.zeros(n, dtype=torch.uint8) if ignore is None else ignore, d, origin)
            want = lesion_hits_numpy(xy, s, lab, d, origin, n, ignore)
            got = model.lesion_hits((xy.astype(np.int64), s), em)
            assert got.hit.device == torch.device(DEV) and same(got.hit, want.hit), (name, ignore is None)
            assert same(got.lesion_max.view(torch.int32), want.lesion_max.view(np.int32)), (name, ignore is None)       # bit for bit
            assert got.n_lesions == want.n_lesions and same(got.fp_scores.view(torch.int32), want.fp_scores.view(np.int32))
            wants.append(want)
        if N >= 4097:                                                                # the cases are there
            plain, ignoring = wants
            assert (plain.hit == -1).any() and (plain.hit == 0).any() == (name == "many") and (plain.lesion_max > 0).any()
            assert np.array_equal(plain.hit, ignoring.hit) and ignoring.n_lesions < plain.n_lesions
            assert (plain.lesion_max[ignore != 0] > 0).any() and not (ignoring.lesion_max[ignore != 0] > 0).any()


def test_lesion_hits_errors(model):
    em = EvaluationMask(np.zeros((4, 4), np.int32), 0, None, np.zeros(0, np.uint8), 2)
    got = model.lesion_hits((np.array([[1, 1], [2, 2]]), np.array([0.5, np.nan], np.float32)), em)
    assert got.hit.tolist() == [0, -1] and got.lesion_max.shape == (0,) and got.fp_scores.tolist() == [0.5] and got.n_lesions == 0
    with pytest.raises(ValueError):
        model.lesion_hits((np.zeros((3, 2), np.int64), np.zeros(2, np.float32)), em)
    with pytest.raises(ValueError):
        model.lesion_hits((np.zeros((3, 2), np.float32), np.zeros(3, np.float32)), em)
    with pytest.raises(ValueError):
        model.lesion_hits((np.zeros((3, 2), np.int64), np.zeros(3, np.float32)), np.zeros((4, 4), np.int32))


# ------------------------------------------------------------------------------------------------ end to end
D, SHAPE, MARGIN = 4, (120, 160), 2.5                                            # a 640 x 480 slide


def slide_polys(k):
    """Two lesions with holes, a C whose bay is open to the border (no hole), two small lesions that the margin merges and one that the
    extent rule ignores."""
    s = 8 * k
    ring = [rect(400 + s, 300, 520 + s, 420), rect(420 + s, 320, 500 + s, 400)]
    return poly_set(rect(40 + s, 40, 200 + s, 160), rect(80 + s, 70, 150 + s, 120), rect(0, 200, 120, 330), rect(0, 230, 90, 300), *ring,
                    rect(300, 60 + s, 312, 72 + s), rect(318, 60 + s, 330, 72 + s), rect(600, 440, 608, 448),
                    roles=[1, -1, 1, -1, 1, -1, 1, 1, 1], features=[0, 0, 1, 1, 2, 2, 3, 4, 5])


def host_evaluation_mask(polys, ignore_max_extent):
    truth = fill_numpy(polys, D, SHAPE)
    grown = ndimage.distance_transform_edt(truth == 0) < MARGIN
    labels, n = ndimage.label(ndimage.binary_fill_holes(grown), structure=np.ones((3, 3), int))
    ignore = np.zeros(n, np.uint8)
    for l, sl in enumerate(ndimage.find_objects(labels)):
        ignore[l] = max(sl[0].stop - sl[0].start, sl[1].stop - sl[1].start) < ignore_max_extent
    return labels.astype(np.int32), n, ignore


def slide_tiles(k):
    g = np.random.default_rng(100 + k)
    xs, ys = np.arange(0, 640 - 32 + 1, 16), np.arange(0, 480 - 32 + 1, 16)
    coords = np.stack(np.meshgrid(xs, ys, indexing="xy"), -1).reshape(-1, 2).astype(np.int64)
    keep = g.random(len(coords)) < 0.9
    return coords[keep], g.choice(np.array([0.1, 0.3, 0.6, 0.6, 0.8, 0.95], np.float32), int(keep.sum()))


def test_froc_end_to_end(model):
    slides_host, slides_dev, pairs = [], FrocAccumulator(model), []
    for k in range(3):
        polys = slide_polys(k)
        coords, v = slide_tiles(k)
        raster = model.tile_raster(coords, v, 32, D, SHAPE)
        labels, n, ignore = host_evaluation_mask(polys, 8)
        em = model.evaluation_mask(polys, MARGIN, ignore_max_extent=8, downsample=D, shape=SHAPE)
        assert em.n == n and n >= 5 and same(em.labels, labels) and same(em.ignore, ignore) and 0 < ignore.sum() < n
        assert (em.downsample, em.origin, em.table.n) == (D, (0, 0), n)
        truth = fill_numpy(polys, D, SHAPE)
        assert truth[24, 28] == 0 and labels[24, 28] > 0 and labels[66, 10] == 0    # a filled hole; the bay of the C stays background
        cand_host = candidates_numpy(peaks_numpy(raster.acc.cpu().numpy(), 3, 32768), D)
        cand = model.raster_peaks(raster, 3, 0.5)
        assert same(cand.xy, cand_host.xy) and same(cand.scores, cand_host.scores) and len(cand) > 20
        want = lesion_hits_numpy(cand_host.xy, cand_host.scores, labels, D, (0, 0), n, ignore)
        got = model.lesion_hits(cand, em)
        assert same(got.hit, want.hit) and same(got.lesion_max, want.lesion_max) and same(got.fp_scores, want.fp_scores)
        assert (want.hit > 0).any() and (want.hit == 0).any()
        slides_host.append(want)
        slides_dev.add(got)
        pairs.append((raster, polys))
    want = froc_numpy(slides_host)
    got = slides_dev.curve()
    assert got == want and len(want.fps) > 3 and 0 < want.score < 1
    assert got.avg_fps.tolist() == want.avg_fps.tolist() and got.sensitivity.tolist() == want.sensitivity.tolist()
    assert wsi.eval_seg_froc(pairs, margin_px=MARGIN, radius=3, min_score=0.5, ignore_max_extent=8) == want
    cands = [(model.raster_peaks(r, 3, 0.5), TissueMask(fill_numpy(p, D, SHAPE), D)) for r, p in pairs]
    assert wsi.eval_seg_froc(cands, margin_px=MARGIN, ignore_max_extent=8, model=model) == want


def test_evaluation_mask_options(model):
    polys = slide_polys(0)
    truth = fill_numpy(polys, D, SHAPE)
    plain = model.evaluation_mask(TissueMask(truth, D), 0, connectivity=4, fill_holes=False)
    labels, n = ndimage.label(truth)
    assert plain.n == n and same(plain.labels, labels.astype(np.int32)) and plain.ignore.tolist() == [0] * n
    with pytest.raises(ValueError):
        model.evaluation_mask(polys, MARGIN)                                        # a PolygonSet has no geometry of its own
    with pytest.raises(ValueError):
        model.evaluation_mask(truth, MARGIN)
