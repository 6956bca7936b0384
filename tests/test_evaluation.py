"""The host side of the segmentation evaluation, no GPU: the numpy restatements that are the yardsticks of
tests/test_evaluation_gpu.py are held here to scikit-learn, spelled as the reference spells it (WSI_evaluation/segment_utils.py:113-117),
and to brute force in Python integers."""
import math
import os

import numpy as np
import pytest
import torch

from keep_amd import _lib, wsi
from keep_amd.annotation import PolygonSet
from keep_amd.evaluation import (HIST_BINS, MaskOverlap, RocResult, default_eval_shape, mask_counts_numpy, mean16_numpy, plan_label_bands,
                                 raster_hist_numpy, resolve_annotation, roc_numpy, sweep_from_hist_numpy)
from keep_amd.heatmap import quantize, raster_numpy
from keep_amd.region import TissueMask

FAMILIES = ("random", "six", "decimal", "three_ints", "constant")
LABELLINGS = ("coin", "informative", "worse_than_chance")


def family_scores(family: str, n: int, g) -> np.ndarray:
    if family == "random":
        return g.random(n).astype(np.float32)
    if family == "six":
        return (g.integers(0, 6, n) / 7).astype(np.float32)
    if family == "decimal":
        return np.round(g.random(n), 1).astype(np.float32)
    if family == "three_ints":
        return g.integers(0, 3, n).astype(np.float32)
    return np.full(n, 0.3, np.float32)


def family_labels(labelling: str, s: np.ndarray, g) -> np.ndarray:
    """uint8 labels with both classes present (the first two tiles are forced apart when a draw gives one class)."""
    noisy = s + g.normal(0, 0.3, len(s))
    y = {"coin": g.random(len(s)) < 0.4, "informative": noisy > 0.5, "worse_than_chance": noisy < 0.4}[labelling].astype(np.uint8)
    if y.min() == y.max():
        y[0], y[1] = 0, 1
    return y


def roc_cases(sizes, seed=3):
    g = np.random.default_rng(seed)
    for n in sizes:
        for family in FAMILIES:
            for labelling in LABELLINGS:
                s = family_scores(family, n, g)
                yield family, labelling, s, family_labels(labelling, s, g)


def test_roc_numpy_is_scikit_learn_as_the_reference_calls_it():
    metrics = pytest.importorskip("sklearn.metrics")
    infs = 0
    for family, labelling, s, y in roc_cases([2, 3, 5, 17, 64, 130, 257, 400] * 6):
        r = roc_numpy(s, y)
        fpr, tpr, thresholds = metrics.roc_curve(y, s)
        want = thresholds[np.argmax(tpr - fpr)]
        assert r.best_threshold == want, (family, labelling, len(s))
        assert int(r.kept.sum()) + 1 == len(thresholds)
        for got, ref in zip(r.sklearn_curve(), (fpr, tpr, thresholds)):
            assert np.array_equal(got, ref)
        # ours is the exact rational rounded once; scikit-learn's a pairwise float64 trapezoid sum of K terms that add up to <= 1
        assert abs(r.auc - metrics.roc_auc_score(y, s)) <= 1e-14
        infs += math.isinf(r.best_threshold)
        assert np.array_equal(r.fpr, r.fps / r.n_neg) and np.array_equal(r.tpr, r.tps / r.n_pos)
    assert infs > 20                                             # constant and worse-than-chance scores end at the prepended point


def test_u2_equals_the_double_loop():
    for family, labelling, s, y in roc_cases([2, 9, 40, 120], seed=8):
        r = roc_numpy(s, y, curve=False)
        pos, neg = s[y != 0].tolist(), s[y == 0].tolist()
        assert r.u2 == sum(2 * (b < a) + (b == a) for a in pos for b in neg)
        assert (r.n, r.n_pos, r.n_neg) == (len(s), len(pos), len(neg)) and r.thresholds is None
        assert r.auc == r.u2 / (2 * r.n_pos * r.n_neg)


def test_nan_scores_leave_and_minus_zero_is_zero():
    s = np.array([0.0, -0.0, np.nan, 0.5, np.nan, -0.25, 0.5], np.float32)
    y = np.array([1, 0, 1, 1, 0, 0, 0], np.uint8)
    r = roc_numpy(s, y)
    assert (r.n, r.n_pos, r.n_neg) == (5, 2, 3)
    assert r.thresholds.tolist() == [0.5, 0.0, -0.25] and not np.signbit(r.thresholds[1])
    assert r.tps.tolist() == [1, 2, 2] and r.fps.tolist() == [1, 2, 3]
    assert r.u2 == (2 * 2 + 1) + (2 * 1 + 1)


def test_a_single_class_is_scikit_learns_error():
    for y in (np.zeros(5, np.uint8), np.ones(5, np.uint8)):
        with pytest.raises(ValueError, match="Only one class"):
            roc_numpy(np.arange(5, dtype=np.float32), y)
    with pytest.raises(ValueError, match="Only one class"):       # the only positive has no score
        roc_numpy(np.array([np.nan, 1, 2], np.float32), np.array([1, 0, 0], np.uint8))
    with pytest.raises(ValueError, match="Only one class"):
        RocResult(3, 3, 0, 0, math.inf)
    with pytest.raises(ValueError):
        roc_numpy(np.zeros(0, np.float32), np.zeros(0, np.uint8))
    with pytest.raises(ValueError):
        roc_numpy(np.zeros(3, np.int64), np.zeros(3, np.uint8))
    with pytest.raises(ValueError):
        roc_numpy(np.zeros(3, np.float32), np.zeros(4, np.uint8))


# ------------------------------------------------------------------------------------------------ masks and the sweep
def test_mask_counts_against_a_pixel_loop():
    g = np.random.default_rng(5)
    for h, w in ((1, 1), (3, 17), (16, 16), (5, 33)):
        a, b, within = ((g.random((h, w)) < 0.4) * g.integers(1, 256, (h, w))).astype(np.uint8), g.random((h, w)) < 0.5, g.random((h, w)) < 0.7
        for wi in (None, within):
            want = [0, 0, 0, 0]
            for i in range(h):
                for j in range(w):
                    if wi is None or wi[i, j]:
                        want[0] += a[i, j] != 0
                        want[1] += bool(b[i, j])
                        want[2] += a[i, j] != 0 and bool(b[i, j])
                        want[3] += 1
            got = mask_counts_numpy(a, torch.from_numpy(b), None if wi is None else TissueMask(wi, 16))
            assert got.dtype == np.int64 and got.tolist() == want
            # the reference's wrapping uint8 product is non-zero exactly where both masks are (segment_utils.py:142-143)
            if wi is None:
                pred = np.where(b, 255, 0).astype(np.uint8)
                assert np.count_nonzero(a * pred) == want[2]
    with pytest.raises(ValueError):
        mask_counts_numpy(np.zeros((2, 2), np.uint8), np.zeros((2, 3), np.uint8))
    with pytest.raises(ValueError):
        mask_counts_numpy(np.zeros((2, 2), np.float32), np.zeros((2, 2), np.uint8))


def test_overlap_properties():
    o = MaskOverlap(6, 4, 3, 20)
    assert o.dice == 2 * 3 / 10 and o.iou == 3 / 7 and o.confusion == ((13, 1), (3, 3)) and o.counts == (6, 4, 3, 20)
    assert MaskOverlap(0, 0, 0, 9).dice == 1 and MaskOverlap(0, 0, 0, 9).iou == 1 and MaskOverlap(5, 0, 0, 9).dice == 0


def sweep_raster(seed=2):
    """Overlapping tiles on 40 x 56 pixels with values that quantise to 0 and to 65535, exact .5 ties of the mean, uncovered pixels."""
    g = np.random.default_rng(seed)
    coords = np.stack([g.integers(-8, 150, 60), g.integers(-8, 100, 60)], 1) // 4 * 4
    values = g.choice(np.array([0.0, 1e-9, 1.0, 2.0, 0.25, 0.5, 0.5 + 1 / 131070, 0.75], np.float32), 60)
    acc = raster_numpy(coords, values, 32, 4, (40, 56))
    truth = np.zeros((40, 56), np.uint8)
    truth[5:30, 10:44] = 255
    truth[g.random((40, 56)) < 0.1] ^= 255
    return acc, truth, g.random((40, 56)) < 0.8


def test_hist_and_sweep_against_painting_every_threshold():
    acc, truth, within = sweep_raster()
    m = mean16_numpy(acc)
    assert (m == 65536).any() and (m == 0).any() and (m == 65535).any()
    for wi in (None, within):
        hist = raster_hist_numpy(acc, truth, wi)
        assert hist.shape == (2, HIST_BINS) and hist.sum() == (acc.size if wi is None else wi.sum())
        sw = sweep_from_hist_numpy(hist)
        dices = {}
        for t in (0.0, 1e-6, 0.1, 0.25, 0.2500001, 0.3, 0.5, 0.50001, 0.6, 0.75, 0.9, 0.99999, 1.0):
            pred = (m <= 65535) & (m > quantize(t))
            want = MaskOverlap(*mask_counts_numpy(truth, pred, wi))
            assert sw.overlap_at(t) == want and sw.dice_at(t) == want.dice
            assert sw.dice[quantize(t)] == want.dice
            dices[quantize(t)] = want.dice
        assert sw.best_dice == sw.dice.max() >= max(dices.values())
        assert sw.best_t16 == int(np.flatnonzero(sw.dice == sw.best_dice)[0]) and sw.best_threshold == sw.best_t16 / 65535
        # the pixel-level AUROC: the same U2 as the tile ROC gives on the pixels as tiles, an uncovered pixel below every covered one
        on = np.ones(m.shape, bool) if wi is None else wi
        score = np.where(m[on] == 65536, -1, m[on]).astype(np.float32)
        r = roc_numpy(score, truth[on], curve=False)
        assert (sw.u2, sw.n_pos, sw.n_neg) == (r.u2, r.n_pos, r.n_neg) and sw.auc == r.auc


def test_best_dice_ties_go_to_the_lowest_threshold():
    hist = np.zeros((2, HIST_BINS), np.int64)
    hist[1, 40000], hist[0, 100], hist[0, 65536], hist[1, 65536] = 7, 5, 11, 2
    sw = sweep_from_hist_numpy(hist)
    # every t in [100, 40000) predicts the 7 true pixels alone: Dice 14 / 16, and the lowest such t is taken
    assert sw.best_t16 == 100 and sw.best_dice == 14 / 16 and sw.dice[39999] == 14 / 16 and sw.dice[40000] == 0 and sw.dice[99] == 14 / 21
    empty = sweep_from_hist_numpy(np.zeros((2, HIST_BINS), np.int64))
    assert empty.best_t16 == 0 and empty.best_dice == 1 and math.isnan(empty.auc)
    with pytest.raises(ValueError):
        sweep_from_hist_numpy(np.zeros((2, 65536), np.int64))


# ------------------------------------------------------------------------------------------------ bands, shapes, dispatch
def band_rows(ys, bands):
    return [[int(y) for y in np.unique(ys) if a <= y <= b] for a, b in bands]


def test_bands_cover_every_tile_row_once_and_respect_the_cap():
    ys = np.array([0, 16, 16, 32, 48, 200, 216, 1000, 64, 0])
    rows = sorted(set(ys.tolist()))
    x0, x1, patch = -40, 600, 32
    width = x1 - x0
    for cap, n_bands in ((1 << 28, 1), (patch * width, len(rows)), (64 * width, None), (300 * width, None)):
        bands = plan_label_bands(ys, x0, x1, patch, cap)
        assert sorted(sum(band_rows(ys, bands), [])) == rows                       # every row, and none twice
        assert all((b + patch - a) * width <= cap for a, b in bands)
        assert all(a in rows and b in rows and a <= b for a, b in bands)
        assert all(b < a2 for (_, b), (a2, _) in zip(bands, bands[1:]))
        if n_bands is not None:
            assert len(bands) == n_bands
    assert len(plan_label_bands(ys, x0, x1, patch, 64 * width)) > 1
    assert plan_label_bands(np.zeros(0, np.int64), 0, 32, 32, 1 << 20) == []
    with pytest.raises(ValueError, match=f"max_band_bytes = {patch * width - 1}"):
        plan_label_bands(ys, x0, x1, patch, patch * width - 1)                      # a tile row wider than the cap
    # the 2^28 cells of one fill bind before the bytes: 63 rows of 2^22 + 1 cells
    assert plan_label_bands([0, 8, 40], 0, 1 << 22, 32, 1 << 40) == [(0, 8), (40, 40)]


def test_default_shape_covers_tiles_and_vertices():
    polys = PolygonSet(np.array([[10, 10], [1000, 20], [500, 641]], np.int64), np.array([0, 3], np.int64))
    coords = np.array([[0, 0], [224, 448]])
    assert default_eval_shape(coords, polys, 224) == (math.ceil(672 / 16), math.ceil(1001 / 16))
    assert default_eval_shape(coords, None, 224) == (42, 28)
    assert default_eval_shape(np.zeros((0, 2), np.int64), polys, 224) == (41, 63)     # the vertex (.., 641) lies in pixel row 40
    assert default_eval_shape(np.array([[100, 50]]), polys, 224, 1) == (642, 1001)
    assert default_eval_shape(np.zeros((0, 2), np.int64), None, 224) == (1, 1)


def test_mask_path_dispatch(golden_dir, tmp_path):
    xml, gj = os.path.join(golden_dir, "annotation_asap.xml"), os.path.join(golden_dir, "annotation_qupath.geojson")
    a, order = resolve_annotation(xml)
    assert isinstance(a, PolygonSet) and order is None and np.array_equal(a.vertices, PolygonSet.from_asap_xml(xml).vertices)
    b, _ = resolve_annotation(gj)
    assert np.array_equal(b.vertices, PolygonSet.from_geojson(gj).vertices) and b.n_rings > 0
    as_json = tmp_path / "COPY.JSON"
    as_json.write_text(open(gj).read())
    assert np.array_equal(resolve_annotation(as_json)[0].vertices, b.vertices)
    assert resolve_annotation((a, "an order")) == (a, "an order") and resolve_annotation(a) == (a, None)
    t = TissueMask(np.ones((2, 2), np.uint8), 16)
    assert resolve_annotation(t) == (t, None)
    for other in ("mask.tif", "slide.svs", "annotation.xml.bak", 7, (1, 2)):
        assert resolve_annotation(other) is None
        with pytest.raises(NotImplementedError):
            wsi.eval_seg_auc({"0_0": 0.5}, other)
        with pytest.raises(NotImplementedError):
            wsi.eval_seg_coarse({"0_0": 0.5}, other)


def test_the_reference_module_exports_the_two_functions():
    from keep_amd.wsi_evaluation import segment_utils
    assert segment_utils.eval_seg_auc is wsi.eval_seg_auc and segment_utils.eval_seg_coarse is wsi.eval_seg_coarse
    assert {"keep_eval_roc", "keep_eval_mask_counts", "keep_eval_raster_hist"} <= set(_lib.SIGNATURES)
