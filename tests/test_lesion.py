"""The host side of the lesion-level scoring, no GPU: the numpy restatements that are the yardsticks of
tests/test_lesion_gpu.py are themselves held to independent statements -- scipy's distance_transform_edt, a double loop over every
window for the peaks, and a loop per threshold written from the published description of the CAMELYON16 FROC analysis.  Every
comparison is exact: the results are integers, or float64 computed on the host from integers."""
import math
from fractions import Fraction

import numpy as np
import pytest
from scipy import ndimage

from keep_amd import _lib
from keep_amd.heatmap import raster_numpy
from keep_amd.lesion import (FROC_POINTS, FrocAccumulator, LesionHits, camelyon16_margin, candidates_numpy, dist2_numpy, distance_threshold,
                             froc_numpy, lesion_hits_numpy, mean16_keys_numpy, peaks_numpy)

THRESHOLDS = [camelyon16_margin(), 2.0, 5.0, math.sqrt(13)]


# ------------------------------------------------------------------------------------------------ distance
def edt2(mask, R, to="foreground"):
    """rint(edt^2) capped at R^2 + 1; a mask without a target pixel is all sentinel (scipy's answer there is not a distance)."""
    target = (mask != 0) if to == "foreground" else (mask == 0)
    if not target.any():
        return np.full(mask.shape, R * R + 1, np.uint32)
    d2 = np.rint(ndimage.distance_transform_edt(~target) ** 2).astype(np.int64)
    return np.minimum(d2, R * R + 1).astype(np.uint32)


def dist_masks(h, w, g):
    corner = np.zeros((h, w), np.uint8)
    corner[h - 1, 0] = 7
    return [("empty", np.zeros((h, w), np.uint8)), ("full", np.ones((h, w), np.uint8)), ("corner", corner),
            ("sparse", (g.random((h, w)) < 0.02).astype(np.uint8))]


@pytest.mark.parametrize("shape", [(1, 1), (1, 40), (40, 1), (37, 53), (33, 65)])
@pytest.mark.parametrize("R", [1, 5, 9, 64])
def test_dist2_numpy_equals_scipy_edt(shape, R):
    g = np.random.default_rng(shape[0] * 100 + R)
    for name, m in dist_masks(*shape, g):
        for to in ("foreground", "background"):
            got = dist2_numpy(m, R, to)
            assert got.dtype == np.uint32 and np.array_equal(got, edt2(m, R, to)), (name, to)


@pytest.mark.parametrize("T", THRESHOLDS)
def test_integer_threshold_equals_float64_edt_comparison(T):
    R, k = distance_threshold(T)
    assert R == math.ceil(T) and 0 <= k <= R * R
    for v in range(R * R + 2):
        assert (v <= k) == (math.sqrt(v) < T), v
    g = np.random.default_rng(int(T * 1000))
    m = (g.random((41, 57)) < 0.01).astype(np.uint8)
    assert np.array_equal(dist2_numpy(m, R) <= k, ndimage.distance_transform_edt(m == 0) < T)
    full = (g.random((41, 57)) < 0.97).astype(np.uint8)
    assert np.array_equal(dist2_numpy(full, R, "background") > k, ndimage.distance_transform_edt(full != 0) >= T)


def test_camelyon16_margin_and_argument_errors():
    assert camelyon16_margin() == 75 / (0.243 * 32 * 2) and 4.82 < camelyon16_margin() < 4.83
    for bad in (0, -1.0, 1024.5, math.nan):
        with pytest.raises(ValueError):
            distance_threshold(bad)
    for bad in (0, 1025, 2.5):
        with pytest.raises(ValueError):
            dist2_numpy(np.ones((3, 3), np.uint8), bad)
    with pytest.raises(ValueError):
        dist2_numpy(np.ones((3, 3), np.uint8), 2, "sideways")


# ------------------------------------------------------------------------------------------------ peaks
def plateau_raster(h, w, levels, g):
    """An accumulator of h x w pixels with `levels` distinct means, large plateaus and uncovered pixels."""
    coarse = g.integers(0, levels, (h // 4 + 1, w // 4 + 1))
    q = np.kron(coarse, np.ones((4, 4), np.int64))[:h, :w] * (65535 // max(levels - 1, 1))
    c = g.integers(0, 3, (h, w))                                 # 0: uncovered
    return ((c.astype(np.uint64) << np.uint64(40)) | (q * c).astype(np.uint64)).view(np.int64), q, c


def peaks_double_loop(acc, r, min16, mask=None):
    key = mean16_keys_numpy(acc, mask)
    h, w = key.shape
    m = (key >> np.uint64(32)).astype(np.int64) - 1
    rows = []
    for y in range(h):
        for x in range(w):
            if key[y, x] == 0 or m[y, x] < min16:
                continue
            ok = True
            for yy in range(max(0, y - r), min(h, y + r + 1)):
                for xx in range(max(0, x - r), min(w, x + r + 1)):
                    if (yy, xx) != (y, x) and key[yy, xx] != 0 and (m[yy, xx] > m[y, x] or (m[yy, xx] == m[y, x] and yy * w + xx < y * w + x)):
                        ok = False
            if ok:
                rows.append((x, y, m[y, x]))
    return np.array(rows, np.int64).reshape(-1, 3)


@pytest.mark.parametrize("levels", [3, 65536])
@pytest.mark.parametrize("r", [1, 2, 5])
def test_peaks_numpy_equals_the_double_loop(levels, r):
    g = np.random.default_rng(levels + r)
    acc, q, c = plateau_raster(23, 31, levels, g)
    mask = (g.random(acc.shape) < 0.8).astype(np.uint8)
    assert np.array_equal(mean16_keys_numpy(acc) != 0, c > 0)
    for min16 in (0, 32768):
        for tissue in (None, mask):
            got = peaks_numpy(acc, r, min16, tissue)
            assert got.dtype == np.int64 and np.array_equal(got, peaks_double_loop(acc, r, min16, tissue)), (min16, tissue is None)
    assert len(peaks_numpy(acc, r)) > 0


def test_peaks_of_tile_rasters_and_candidates():
    coords = np.array([[0, 0], [8, 0], [40, 24], [40, 24]], np.int64)
    acc = raster_numpy(coords, np.array([0.5, 1.0, 0.25, 0.75], np.float32), 16, 4, (12, 16))
    p = peaks_numpy(acc, 2)
    # tile 1 alone covers columns 4, 5 (65535); its overlap with tile 0 averages to 49152 and tile 0 alone holds 32768: both suppressed.
    # Tiles 2 and 3 coincide: (16384 + 49151) / 2 rounds half up to 32768.  Of every plateau the first pixel in row-major order wins
    assert p.tolist() == [[4, 0, 65535], [10, 6, 32768]]
    cand = candidates_numpy(p, 4, (8, 4))
    assert cand.xy.tolist() == [[26, 6], [50, 30]] and cand.scores.dtype == np.float32
    assert cand.scores.tolist() == [1.0, float(np.float32(32768 / 65535))]
    assert peaks_numpy(np.zeros((5, 5), np.int64), 3).shape == (0, 3)


# ------------------------------------------------------------------------------------------------ hits and FROC
def froc_loop(slides):
    """The published rule, literally: pool the scores, then one pass over the data per threshold."""
    fp = [float(v) for s in slides for v in s.fp_scores]
    tp = [float(v) for s in slides for v in s.lesion_max]
    n_lesions = sum(s.n_lesions for s in slides)
    rows = []
    for t in sorted(set(fp) | set(tp))[1:]:
        rows.append((sum(v >= t for v in fp), sum(v >= t for v in tp)))
    rows.append((0, 0))
    avg = [f / len(slides) for f, _ in rows]
    sens = [t / n_lesions for _, t in rows]
    return rows, float(np.mean(np.interp(FROC_POINTS, avg[::-1], sens[::-1])))


def hits_loop(xy, scores, labels, d, origin, n, ignore):
    hit, best = [], [0.0] * n
    for (x, y), s in zip(xy.tolist(), scores.tolist()):
        px, py = math.floor(Fraction(x - origin[0], d)), math.floor(Fraction(y - origin[1], d))
        l = int(labels[py, px]) if 0 <= px < labels.shape[1] and 0 <= py < labels.shape[0] else 0
        l = l if 1 <= l <= n else 0
        if math.isnan(s):
            hit.append(-1)
            continue
        hit.append(l)
        if l and not ignore[l - 1]:
            best[l - 1] = max(best[l - 1], max(s, 0.0))
    return hit, best


def random_slide(g, n_cand, equal=False, ignore_some=False):
    labels = np.zeros((20, 30), np.int32)
    labels[2:6, 3:9], labels[10:12, 10:11], labels[15:19, 20:28], labels[0, 29] = 1, 2, 3, 9      # 9: not a label (n = 4), 4: never drawn
    n = 4
    xy = np.stack([g.integers(-40, 300, n_cand), g.integers(-40, 200, n_cand)], 1).astype(np.int64)
    s = (np.full(n_cand, 0.5) if equal else g.integers(0, 6, n_cand) / 5).astype(np.float32)          # few values: FP and TP tie
    if n_cand > 4 and not equal:
        s[0], s[1], s[2] = np.nan, -0.0, -0.5
    ignore = np.array([0, ignore_some, 0, 0], np.uint8)
    return xy, s, labels, n, ignore


@pytest.mark.parametrize("n_slides", [1, 3])
@pytest.mark.parametrize("case", ["ties", "equal", "ignored"])
def test_hits_and_froc_equal_the_loops(n_slides, case):
    g = np.random.default_rng(n_slides * 10 + len(case))
    slides = []
    for k in range(n_slides):
        n_cand = 0 if (k == 1 and case != "equal") else 60              # the second slide proposes nothing
        xy, s, labels, n, ignore = random_slide(g, n_cand, case == "equal", case == "ignored")
        got = lesion_hits_numpy(xy, s, labels, 8, (-16, 8), n, ignore)
        hit, best = hits_loop(xy, s, labels, 8, (-16, 8), n, ignore)
        assert got.hit.dtype == np.int32 and got.hit.tolist() == hit
        assert got.lesion_max.dtype == np.float32 and got.lesion_max.tolist() == best
        assert got.lesion_max[3] == 0 and got.n_lesions == n - int(ignore.sum())      # lesion 4 is never hit
        assert np.array_equal(got.fp_scores, s[np.array(hit, np.int64) == 0]) and not (got.fp_scores == 0)[np.signbit(got.fp_scores)].any()
        slides.append(got)
    curve = froc_numpy(slides)
    rows, score = froc_loop(slides)
    assert list(zip(curve.fps.tolist(), curve.tps.tolist())) == rows and curve.score == score
    assert (curve.n_slides, curve.n_lesions) == (n_slides, sum(s.n_lesions for s in slides))
    acc = FrocAccumulator()
    for s in slides:
        acc.add(s)
    assert acc.curve() == curve


def test_froc_worked_example():
    """2 slides, 3 lesions, 6 candidates.  Slide A: lesions 1 and 2; candidates 0.9 -> lesion 1, 0.6 -> lesion 1, 0.8 -> background,
    0.3 -> background.  Slide B: lesion 1; candidates 0.7 -> lesion 1, 0.6 -> background.  Lesion 2 of slide A is missed.
    FP = {0.8, 0.3, 0.6}, TP = {0.9, 0, 0.7}; T = 0 < 0.3 < 0.6 < 0.7 < 0.8 < 0.9, the thresholds leave out the 0."""
    lab_a = np.zeros((4, 8), np.int32)
    lab_a[1, 1], lab_a[3, 6] = 1, 2
    lab_b = np.zeros((4, 8), np.int32)
    lab_b[2, 2] = 1
    a = lesion_hits_numpy(np.array([[1, 1], [1, 1], [5, 0], [7, 7]]), np.array([0.9, 0.6, 0.8, 0.3], np.float32), lab_a, 1, (0, 0), 2)
    b = lesion_hits_numpy(np.array([[2, 2], [0, 0]]), np.array([0.7, 0.6], np.float32), lab_b, 1, (0, 0), 1)
    assert a.hit.tolist() == [1, 1, 0, 0] and a.lesion_max.tolist() == [float(np.float32(0.9)), 0.0] and b.hit.tolist() == [1, 0]
    curve = froc_numpy([a, b])
    assert curve.thresholds.tolist() == [float(np.float32(v)) for v in (0.3, 0.6, 0.7, 0.8, 0.9)]
    assert curve.fps.tolist() == [3, 2, 1, 1, 0, 0] and curve.tps.tolist() == [2, 2, 2, 1, 1, 0]
    assert curve.avg_fps.tolist() == [1.5, 1.0, 0.5, 0.5, 0.0, 0.0]
    assert curve.sensitivity.tolist() == [2 / 3, 2 / 3, 2 / 3, 1 / 3, 1 / 3, 0.0]
    # np.interp over avg_fps ascending (0, 0, .5, .5, 1, 1.5) with sensitivities (0, 1/3, 1/3, 2/3, 2/3, 2/3): at 0.25 halfway between the
    # points (0, 1/3) and (0.5, 1/3); at 0.5 the last of the equal abscissae; flat from there, and 2/3 beyond the curve's end
    want = [Fraction(1, 3), Fraction(2, 3), Fraction(2, 3), Fraction(2, 3), Fraction(2, 3), Fraction(2, 3)]
    assert curve.sensitivity_at.tolist() == [float(v) for v in want]
    assert curve.score == float(np.mean([float(v) for v in want]))


def test_froc_without_lesions_is_an_error():
    empty = LesionHits(np.zeros(2, np.int32), np.zeros(0, np.float32), 0, np.array([0.5, 0.25], np.float32))
    with pytest.raises(ValueError, match="no lesion"):
        froc_numpy([empty])
    with pytest.raises(ValueError):
        FrocAccumulator().curve()


def test_the_entry_points_are_bound():
    assert {"keep_mask_dist2", "keep_raster_peaks", "keep_lesion_hits"} <= set(_lib.SIGNATURES)
