"""Segmentation evaluation on the MI355X: keep_eval_roc / keep_eval_mask_counts / keep_eval_raster_hist,
KEEPModel.tile_roc / mask_overlap / raster_sweep / annotation_tile_labels, wsi.eval_seg_auc / eval_seg_coarse / segment_evaluate and
zero_shot_segment with an annotation.

Everything the device computes is an integer, or chosen by IEEE float64 operations on integers, so every comparison is exact: the
yardsticks are the numpy restatements of keep_amd.evaluation, which tests/test_evaluation.py holds to scikit-learn and to brute force."""
import json
import math

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel, wsi
from keep_amd.annotation import CAMELYON16_ORDER, PolygonSet, fill_numpy, tile_counts_numpy
from keep_amd.config import small_shape
from keep_amd.evaluation import (MaskOverlap, default_eval_shape, mask_counts_numpy, mean16_numpy, raster_hist_numpy, roc_numpy,
                                 sweep_from_hist_numpy)
from keep_amd.heatmap import pred_numpy, quantize, raster_numpy
from keep_amd.region import TissueMask
from keep_amd.synth import synth_state_dict
from test_annotation import poly_set, rect
from test_evaluation import FAMILIES, LABELLINGS, family_labels, family_scores

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def model():
    m = KEEPModel(precision="strict")
    m.load_state_dict(synth_state_dict(small_shape(2, 2), seed=5), strict=True)
    return m.to(DEV).eval()


def same(t: torch.Tensor, a: np.ndarray) -> bool:
    return t.dtype == torch.from_numpy(a).dtype and tuple(t.shape) == a.shape and torch.equal(t.cpu(), torch.from_numpy(a))


def same_roc(got, want, curve=True) -> bool:
    ok = (got.n, got.n_pos, got.n_neg, got.u2) == (want.n, want.n_pos, want.n_neg, want.u2)
    ok = ok and got.auc == want.auc and got.best_threshold == want.best_threshold
    if not curve:
        return ok and got.thresholds is None
    ok = ok and got.thresholds.device == torch.device(DEV)
    # bit for bit: a threshold of -0.0 would compare equal to +0.0
    return (ok and same(got.thresholds.view(torch.int32), want.thresholds.view(np.int32)) and same(got.fps, want.fps) and same(got.tps, want.tps)
            and same(got.kept, want.kept))


# ------------------------------------------------------------------------------------------------ tile ROC
@pytest.mark.parametrize("n", [2, 63, 64, 65, 255, 256, 257, 4096, 4097, 70001])
def test_tile_roc_equals_the_restatement(model, n):
    """4096 / 4097: the sort keeps up to 4096 values in one block and takes the digit tables above; 2048 flags make one chunk of the scan."""
    g = np.random.default_rng(n)
    infs = 0
    for family in FAMILIES:
        for labelling in LABELLINGS:
            s = family_scores(family, n, g)
            y = family_labels(labelling, s, g)
            want = roc_numpy(s, y)
            assert same_roc(model.tile_roc(s, y), want), (family, labelling)
            infs += math.isinf(want.best_threshold)
    assert infs >= 3                                             # the constant family at the least
    assert same_roc(model.tile_roc(torch.from_numpy(s).to(DEV), torch.from_numpy(y).to(DEV) != 0, curve=False), want, curve=False)


@pytest.mark.parametrize("n", [65, 4097, 70001])
def test_tile_roc_with_nans_and_minus_zero(model, n):
    g = np.random.default_rng(n + 1)
    for family in ("random", "three_ints"):
        s = family_scores(family, n, g) - (family == "three_ints")
        s[g.random(n) < 0.2] = np.nan
        s[g.random(n) < 0.2] = -0.0
        s[g.random(n) < 0.1] = 0.0
        s[:4] = [0.0, -0.0, -1.0, 1.0]
        y = family_labels("informative", np.nan_to_num(s), g)
        y[:4] = [1, 0, 0, 1]
        want = roc_numpy(s, y)
        assert want.n < n
        assert same_roc(model.tile_roc(s, y), want) and same_roc(model.tile_roc(s, y, curve=False), want, curve=False)


@pytest.mark.parametrize("n", [2, 257, 5000])
def test_tile_roc_with_one_positive_one_negative_and_equal_scores(model, n):
    g = np.random.default_rng(n + 2)
    s = family_scores("decimal", n, g)
    for lone in (0, 1):
        for at in (0, n - 1, int(np.argmax(s)), int(np.argmin(s))):
            y = np.full(n, 1 - lone, np.uint8)
            y[at] = lone
            assert same_roc(model.tile_roc(s, y), roc_numpy(s, y))
    y = family_labels("coin", s, g)
    got = model.tile_roc(np.full(n, 0.25, np.float32), y)
    assert got.best_threshold == math.inf and got.auc == 0.5 and got.kept.tolist() == [True] and got.thresholds.tolist() == [0.25]
    assert same_roc(got, roc_numpy(np.full(n, 0.25, np.float32), y))


def test_tile_roc_errors(model):
    s = np.linspace(0, 1, 9, dtype=np.float32)
    for y in (np.zeros(9, np.uint8), np.ones(9, np.uint8)):
        with pytest.raises(ValueError, match="Only one class"):
            model.tile_roc(s, y)
    with pytest.raises(ValueError, match="Only one class"):       # the only negative has no score
        model.tile_roc(np.array([np.nan, 1, 2], np.float32), np.array([0, 1, 1], np.uint8), curve=False)
    with pytest.raises(ValueError):
        model.tile_roc(np.zeros(0, np.float32), np.zeros(0, np.uint8))
    with pytest.raises(ValueError):
        model.tile_roc(s, np.zeros(8, np.uint8))
    with pytest.raises(ValueError):
        model.tile_roc(s.astype(np.int64), np.zeros(9, np.uint8))


# ------------------------------------------------------------------------------------------------ masks and the sweep
SHAPES = [(1, 1), (1, 300), (300, 1), (67, 129), (4, 4099), (1030, 1027)]


def masks_of(h, w, g):
    return [("empty", np.zeros((h, w), np.uint8)), ("full", np.full((h, w), 255, np.uint8)),
            ("checkerboard", (np.indices((h, w)).sum(0) % 2).astype(np.uint8)),
            ("random", ((g.random((h, w)) < 0.5) * g.integers(1, 256, (h, w))).astype(np.uint8))]


@pytest.mark.parametrize("h,w", SHAPES)
def test_mask_overlap_equals_the_restatement(model, h, w):
    g = np.random.default_rng(h * 5 + w)
    masks = masks_of(h, w, g)
    within = g.random((h, w)) < 0.6
    for (_, a) in masks:
        ad = torch.from_numpy(a).to(DEV)
        for (_, b) in masks:
            for wi in (None, within):
                got = model.mask_overlap(ad, b, wi)
                assert got == MaskOverlap(*mask_counts_numpy(a, b, wi))
    # masks that do not start on 16 bytes take the byte path
    flat = torch.from_numpy(g.integers(0, 3, 3 * h * w + 3).astype(np.uint8)).to(DEV)
    a, b, wi = (flat[1 + k * h * w:1 + (k + 1) * h * w].view(h, w) for k in range(3))
    assert a.data_ptr() % 16 and model.mask_overlap(a, b, wi) == MaskOverlap(*mask_counts_numpy(a, b, wi))
    assert model.mask_overlap(a, a).counts == (int((a != 0).sum()),) * 3 + (h * w,)


def overlapping_tiles(h, w, d, patch, g, n=40):
    """Tiles that overlap, hang over the border and leave pixels uncovered; values that quantise to 0 and to 65535 among them."""
    coords = np.stack([g.integers(-patch, max(w * d, 1), n), g.integers(-patch, max(h * d, 1), n)], 1)
    values = g.choice(np.array([0.0, 1e-9, 1.0, 2.0, 0.25, 0.5, 0.5 + 1 / 131070, 0.75, 0.123], np.float32), n)
    return coords, values


@pytest.mark.parametrize("h,w", SHAPES)
def test_raster_sweep_equals_the_restatement(model, h, w):
    g = np.random.default_rng(h * 3 + w)
    d, patch = 4, 4 * max(1, min(h, w, 40) // 3)
    coords, values = overlapping_tiles(h, w, d, patch, g, 40 if h * w < 10 ** 5 else 400)
    raster = model.tile_raster(coords, values, patch, d, (h, w))
    acc = raster_numpy(coords, values, patch, d, (h, w))
    assert same(raster.acc, acc)
    m16 = mean16_numpy(acc)
    if h * w > 1:
        assert (m16 == 65536).any() and (m16 <= 65535).any()
    within = g.random((h, w)) < 0.7
    for name, truth in masks_of(h, w, g):
        for wi in (None, TissueMask(within, d)):
            hist = raster_hist_numpy(acc, truth, None if wi is None else within)
            assert same(model.raster_hist(raster, truth, wi), hist), name
            got, want = model.raster_sweep(raster, torch.from_numpy(truth).to(DEV), wi), sweep_from_hist_numpy(hist)
            assert same(got.tp, want.tp) and same(got.fp, want.fp) and same(got.fn, want.fn) and same(got.dice, want.dice)
            assert (got.best_t16, got.best_dice, got.u2, got.n_pos, got.n_neg) == (want.best_t16, want.best_dice, want.u2, want.n_pos, want.n_neg)
            assert got.auc == want.auc or (math.isnan(got.auc) and math.isnan(want.auc))
            if name == "random":
                for t in (0.0, 0.2, 0.25, 0.5, 0.75, 0.999, 1.0):
                    pred = (m16 <= 65535) & (m16 > quantize(t))
                    assert got.dice_at(t) == model.mask_overlap(truth, pred, wi).dice == want.dice_at(t)


def test_a_raster_with_means_at_both_ends(model):
    """Tiles of value 0 and 1 side by side under a third of value 0.5 that covers one column of the first and three of the second, and
    an uncovered column: the bins 0, (0 + 32768) / 2, (65535 + 32768 + 1) / 2 rounded half up, 65535 and 65536."""
    coords, values = np.array([[0, 0], [32, 0], [24, 0]]), np.array([0.0, 1.0, 0.5], np.float32)
    raster = model.tile_raster(coords, values, 32, 8, (4, 9))
    truth = np.zeros((4, 9), np.uint8)
    truth[:, 4:] = 1
    hist = model.raster_hist(raster, truth)
    assert same(hist, raster_hist_numpy(raster.acc.cpu().numpy(), truth))
    assert [hist[0, 0].item(), hist[0, 16384].item(), hist[1, 49152].item(), hist[1, 65535].item()] == [12, 4, 12, 4]
    assert hist[:, 65536].tolist() == [0, 4] and hist.sum().item() == 36
    sw = model.raster_sweep(raster, truth)
    assert sw.dice_at(0.8) == 2 * 4 / (20 + 4) and sw.best_t16 == 16384 and sw.best_dice == 2 * 16 / (20 + 16) and sw.dice_at(0.0) == 32 / 40
    with pytest.raises(ValueError):
        model.raster_sweep(raster, np.zeros((4, 8), np.uint8))
    with pytest.raises(ValueError):
        model.raster_sweep(raster, TissueMask(truth, 16))
    with pytest.raises(ValueError):
        model.raster_sweep(raster.acc, truth)


# ------------------------------------------------------------------------------------------------ tile labels
W0, H0, PATCH, STEP = 640, 480, 32, 16


def slide_polys() -> PolygonSet:
    """A slanted quadrilateral with a hole, and a triangle that shares its slanted right edge: features 0 and 1."""
    quad = np.array([(100, 60), (400, 40), (460, 380), (80, 300)], np.int64)
    return poly_set(quad, rect(200, 120, 300, 220), np.array([(400, 40), (620, 200), (460, 380)], np.int64), roles=[1, -1, 1], features=[0, 0, 1])


def slide_coords() -> np.ndarray:
    xs, ys = np.arange(0, W0 - PATCH + 1, STEP), np.arange(0, H0 - PATCH + 1, STEP)
    return np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2).astype(np.int64)


@pytest.fixture(scope="module")
def slide():
    """polys, coords, the level-0 mask on the host and the tile labels the reference's rule gives on it."""
    polys, coords = slide_polys(), slide_coords()
    mask0 = fill_numpy(polys, 1, (H0, W0))
    labels = (2 * tile_counts_numpy(mask0, coords, PATCH, 1)[:, 1].astype(np.int64) > PATCH * PATCH).astype(np.uint8)
    assert 50 < labels.sum() < len(labels) - 50
    return polys, coords, mask0, labels


def test_annotation_tile_labels_do_not_depend_on_the_banding(model, slide):
    polys, coords, mask0, labels = slide
    g = np.random.default_rng(4)
    shuffled = coords[g.permutation(len(coords))][:700]          # any order, an x extent of its own
    for cap in (1 << 28, 100 * W0, PATCH * W0):                  # one band, several, one tile row per band
        got = model.annotation_tile_labels(polys, coords, PATCH, max_band_bytes=cap)
        assert got.device == torch.device(DEV) and same(got, labels)
        want = (2 * tile_counts_numpy(mask0, shuffled, PATCH, 1)[:, 1].astype(np.int64) > PATCH * PATCH).astype(np.uint8)
        assert same(model.annotation_tile_labels(polys, torch.from_numpy(shuffled).to(DEV), PATCH, max_band_bytes=cap), want)
    with pytest.raises(ValueError, match="max_band_bytes"):
        model.annotation_tile_labels(polys, coords, PATCH, max_band_bytes=PATCH * W0 - 1)
    assert same(model.annotation_tile_labels(polys, np.zeros((0, 2), np.int64), PATCH), np.zeros(0, np.uint8))
    # masks: level 0 agrees with the polygons; at downsample d the rule is 2 c1 d^2 > patch^2
    assert same(model.annotation_tile_labels(TissueMask(mask0, 1), coords, PATCH), labels)
    assert same(model.annotation_tile_labels(torch.from_numpy(mask0).to(DEV) * 255, coords, PATCH), labels)
    mask4 = fill_numpy(polys, 4, (H0 // 4, W0 // 4))
    want4 = (2 * 16 * tile_counts_numpy(mask4, coords, PATCH, 4)[:, 1].astype(np.int64) > PATCH * PATCH).astype(np.uint8)
    assert same(model.annotation_tile_labels(TissueMask(mask4, 4), coords, PATCH), want4)


def test_annotation_tile_labels_paint_in_order(model, slide):
    polys, coords, _, _ = slide
    grouped = PolygonSet(polys.vertices, polys.ring_start, [0, 1, 2], [1, 1, 1], [{}, {}, {}], ["_0", "_2", "Tumor"])
    mask0 = fill_numpy(grouped.select(groups=CAMELYON16_ORDER[1][0]), 1, (H0, W0), value=0,
                       into=fill_numpy(grouped.select(groups=CAMELYON16_ORDER[0][0]), 1, (H0, W0)))
    want = (2 * tile_counts_numpy(mask0, coords, PATCH, 1)[:, 1].astype(np.int64) > PATCH * PATCH).astype(np.uint8)
    for cap in (1 << 28, PATCH * W0):
        assert same(model.annotation_tile_labels(grouped, coords, PATCH, order=CAMELYON16_ORDER, max_band_bytes=cap), want)
    with pytest.raises(ValueError):
        model.annotation_tile_labels(TissueMask(mask0, 1), coords, PATCH, order=CAMELYON16_ORDER)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def slide_features(slide):
    """Tile features whose cosine to the second class vector grows inside the annotation, and the classifier [D, 2]."""
    polys, coords, mask0, labels = slide
    g = np.random.default_rng(12)
    u = g.normal(size=64)
    inside = mask0[coords[:, 1] + PATCH // 2, coords[:, 0] + PATCH // 2] != 0
    feats = g.normal(size=(len(coords), 64)) + np.outer(np.where(inside, 1.0, -1.0) * 1.5, u / np.linalg.norm(u))
    classifier = np.stack([-u, u], 1) / np.linalg.norm(u) + g.normal(size=(64, 2)) * 0.05
    return torch.from_numpy(feats.astype(np.float32)), torch.from_numpy(classifier.astype(np.float32))


def host_auc_dice(probs: dict, polys, mask0, shape=None):
    """eval_seg_auc and eval_seg_coarse composed from the restatements on the dict of zero_shot_segment(mask_path=None)."""
    coords = np.array([wsi.str2cood(k) for k in probs], np.int64).reshape(-1, 2)
    p = np.array(list(probs.values()), np.float32)
    labels = 2 * tile_counts_numpy(mask0, coords, PATCH, 1)[:, 1].astype(np.int64) > PATCH * PATCH
    roc = roc_numpy(p, labels)
    shape = default_eval_shape(coords, polys, PATCH, 16) if shape is None else shape
    above = (p > np.float32(roc.best_threshold)).astype(np.float32)
    pred = pred_numpy(raster_numpy(coords, above, PATCH, 16, shape))
    return roc, MaskOverlap(*mask_counts_numpy(fill_numpy(polys, 16, shape), pred)), shape


def geojson_of(polys: PolygonSet) -> dict:
    feats = []
    for f in range(polys.n_features):
        rings = [polys.ring(r).tolist() for r in range(polys.n_rings) if polys.feature[r] == f]
        feats.append({"type": "Feature", "properties": {}, "geometry": {"type": "Polygon", "coordinates": [r + r[:1] for r in rings]}})
    return {"type": "FeatureCollection", "features": feats}


def test_zero_shot_segment_with_an_annotation(model, slide, slide_features, tmp_path):
    from keep_amd.wsi_evaluation import segment_utils
    polys, coords, mask0, _ = slide
    feats, classifier = slide_features
    probs = wsi.zero_shot_segment(classifier, feats, coords, None, patch_size=PATCH, model=model)
    roc, ov, shape = host_auc_dice(probs, polys, mask0)
    assert 0.8 < roc.auc < 1 and 0 < roc.best_threshold < 1 and 0.3 < ov.dice < 1          # a heatmap worth evaluating
    want = (roc.auc, ov.dice)
    assert wsi.zero_shot_segment(classifier, feats, coords, polys, patch_size=PATCH, model=model) == want
    assert segment_utils.zero_shot_segment(classifier.to(DEV), feats.to(DEV), coords, (polys, None), patch_size=PATCH) == want
    path = tmp_path / "truth.geojson"
    path.write_text(json.dumps(geojson_of(polys)))
    assert wsi.zero_shot_segment(classifier, feats, coords, str(path), patch_size=PATCH, model=model) == want
    assert wsi.zero_shot_segment(classifier, feats, coords, path, patch_size=PATCH, model=model) == want
    # the two halves on their own, on the dict and on device tensors
    assert segment_utils.eval_seg_auc(probs, polys, patch_size=PATCH, model=model) == (roc.auc, roc.best_threshold)
    assert segment_utils.eval_seg_coarse(probs, polys, patch_size=PATCH, thd=roc.best_threshold, model=model) == ov.dice
    pair = (torch.from_numpy(coords).to(DEV), torch.tensor(list(probs.values()), dtype=torch.float32, device=DEV))
    assert wsi.eval_seg_auc(pair, polys, patch_size=PATCH, max_band_bytes=PATCH * W0) == (roc.auc, roc.best_threshold)
    for thd in (0.5, 0.0, 1.0):
        above = (np.array(list(probs.values()), np.float32) > np.float32(thd)).astype(np.float32)
        pred = pred_numpy(raster_numpy(coords, above, PATCH, 16, shape))
        assert wsi.eval_seg_coarse(pair, polys, PATCH, thd) == MaskOverlap(*mask_counts_numpy(fill_numpy(polys, 16, shape), pred)).dice
    # a truth mask at downsample 16 in place of the polygons
    t16 = TissueMask(fill_numpy(polys, 16, shape), 16)
    assert wsi.eval_seg_coarse(probs, t16, PATCH, roc.best_threshold, model=model) == ov.dice
    with pytest.raises(ValueError):
        wsi.eval_seg_coarse(probs, TissueMask(fill_numpy(polys, 8, shape), 8), PATCH, model=model)
    with pytest.raises(NotImplementedError):
        wsi.zero_shot_segment(classifier, feats, coords, "mask.tif", patch_size=PATCH, model=model)


def test_segment_evaluate(model, slide, slide_features):
    polys, coords, mask0, _ = slide
    feats, classifier = slide_features
    probs = wsi.zero_shot_segment(classifier, feats, coords, None, patch_size=PATCH, model=model)
    roc, ov, shape = host_auc_dice(probs, polys, mask0)
    got_roc, got_ov, got_sw = wsi.segment_evaluate(classifier, feats, coords, polys, patch_size=PATCH, sweep=True, model=model)
    assert same_roc(got_roc, roc) and got_ov == ov
    p = np.array(list(probs.values()), np.float32)
    want_sw = sweep_from_hist_numpy(raster_hist_numpy(raster_numpy(coords, p, PATCH, 16, shape), fill_numpy(polys, 16, shape)))
    assert same(got_sw.hist, want_sw.hist) and same(got_sw.dice, want_sw.dice)
    assert (got_sw.best_t16, got_sw.u2, got_sw.auc) == (want_sw.best_t16, want_sw.u2, want_sw.auc)
    two = wsi.segment_evaluate(classifier, feats, coords, polys, patch_size=PATCH, model=model)
    assert len(two) == 2 and two[1] == ov


def test_a_threshold_of_inf_predicts_nothing(model, slide, slide_features):
    polys, coords, mask0, _ = slide
    feats, classifier = slide_features
    flat = classifier[:, :1].repeat(1, 2)                        # both classes alike: every probability is 0.5
    roc, ov = wsi.segment_evaluate(flat, feats, coords, polys, patch_size=PATCH, model=model)
    assert roc.best_threshold == math.inf and roc.auc == 0.5 and ov.b == 0 and ov.a > 0 and ov.dice == 0
    auc, dice = wsi.zero_shot_segment(flat, feats, coords, polys, patch_size=PATCH, model=model)
    assert (auc, dice) == (0.5, 0)
    probs = wsi.zero_shot_segment(flat, feats, coords, None, patch_size=PATCH, model=model)
    assert set(probs.values()) == {0.5}
    nothing = PolygonSet(np.zeros((0, 2), np.int64), np.zeros(1, np.int64))
    assert wsi.eval_seg_coarse(probs, nothing, PATCH, math.inf, model=model) == 1
    assert wsi.eval_seg_coarse(probs, nothing, PATCH, 0.25, model=model) == 0
    with pytest.raises(ValueError, match="Only one class"):
        wsi.eval_seg_auc(probs, nothing, PATCH, model=model)
