"""Heatmap percentiles and smoothing: the numpy restatements against independent statements (scipy's ranks, a
Python sort, a per-pixel double loop in Python integers) and the host-side argument checks.  No GPU."""
import itertools
import math
import struct

import numpy as np
import pytest
import scipy.stats
import torch

from keep_amd import KEEPModel
from keep_amd.heatmap import (COUNT_SHIFT, MAX_RADIUS, check_taps, clam_blur, gaussian_taps, percentiles_numpy, rank_numpy, smooth_numpy,
                              smooth_taps, sort_numpy, unpack_numpy)

NAN_BITS = 0x7FC00000
SPECIALS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,
                     0x00800000, 0x80800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FA5A5A5, 0xFF812345, 0xBF800000, 0x3F800000,
                     0xC2F60000, 0x3EAAAAAB], np.uint32)
FAMILIES = ("normal", "seven", "equal", "ascending", "descending", "specials", "byte0", "byte1", "byte2", "byte3")


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def family(name: str, M: int, seed: int = 0) -> np.ndarray:
    """fp32 [M] of one family of values."""
    g = np.random.default_rng(seed * 1000 + M)
    if name == "normal":
        return g.standard_normal(M).astype(np.float32)
    if name == "seven":
        return g.choice(np.array([-2.5, -0.0, 0.0, 0.125, 0.5, 0.75, 3.0], np.float32), M)
    if name == "equal":
        return np.full(M, 0.3125, np.float32)
    if name == "ascending":
        return (np.arange(M, dtype=np.float32) - np.float32(M // 2)) / np.float32(7)
    if name == "descending":
        return (np.arange(M, dtype=np.float32)[::-1] - np.float32(M // 3)) / np.float32(3)
    if name == "specials":
        v = g.standard_normal(M).astype(np.float32)
        at = g.random(M) < 0.5
        v.view(np.uint32)[at] = g.choice(SPECIALS, int(at.sum()))
        return v
    b = int(name[-1])                                  # keys that differ in one of the four key bytes only
    base = np.uint32(0x3F123456) & ~np.uint32(0xFF << (8 * b))
    return (base | (g.permutation(M).astype(np.uint32) % np.uint32(256)) << np.uint32(8 * b)).view(np.float32)


def canonical(v: np.ndarray) -> list:
    """The population as Python floats: NaNs dropped, -0 as +0."""
    return [0.0 if x == 0 else float(x) for x in np.asarray(v, np.float32) if not math.isnan(x)]


@pytest.mark.parametrize("name,M", list(itertools.product(FAMILIES, (1, 2, 65, 257, 1001))))
def test_sort_and_self_ranks_against_python_and_scipy(name, M):
    v = family(name, M)
    s, n = sort_numpy(v)
    want = sorted(canonical(v))
    assert n == len(want) and s.dtype == np.float32 and s.shape == (M,)
    assert [struct.pack("<f", x) for x in s[:n]] == [struct.pack("<f", x) for x in want]        # +0 for every zero, in order
    assert np.all(bits(s[n:]) == NAN_BITS)
    pct, less, eq = rank_numpy(s, n, v, True)
    keep = ~np.isnan(v)
    assert np.all(less[~keep] == -1) and np.all(eq[~keep] == -1) and np.all(bits(pct[~keep]) == NAN_BITS)
    if n:
        ranks = scipy.stats.rankdata(np.array(canonical(v), np.float64), "average")
        r2 = 2 * less[keep].astype(np.int64) + eq[keep] + 1
        assert np.array_equal(2 * ranks, r2.astype(np.float64))
        assert np.array_equal(bits(pct[keep]), bits((r2.astype(np.float64) / (2 * n)).astype(np.float32)))
    assert np.array_equal(bits(percentiles_numpy(v)), bits(pct))


@pytest.mark.parametrize("name", FAMILIES)
def test_reference_ranks_against_percentileofscore(name):
    ref = family(name, 301, seed=1)
    s, n = sort_numpy(ref)
    pop = np.array(canonical(ref), np.float64)
    g = np.random.default_rng(4)
    with np.errstate(invalid="ignore", over="ignore"):                           # inf - inf among the specials: replaced below
        between = (s[:n - 1] + (s[1:n] - s[:n - 1]) / 2) if n > 1 else np.zeros(0, np.float32)
    q = np.concatenate([s[:n], np.where(np.isfinite(between), between, 0), [-np.inf, np.inf, -3e38, 3e38, -0.0, 0.0, np.nan],
                        g.standard_normal(40)]).astype(np.float32)
    pct, less, eq = rank_numpy(s, n, q, False)
    for i, x in enumerate(q):
        if math.isnan(x):
            assert less[i] == -1 and eq[i] == -1 and bits(pct[i:i + 1])[0] == NAN_BITS
            continue
        assert less[i] == int((pop < float(x)).sum()) and eq[i] == int((pop == float(x)).sum())
        if n:
            want = scipy.stats.percentileofscore(pop, float(x), kind="mean") / 100
            assert abs((2 * int(less[i]) + int(eq[i])) / (2 * n) - want) <= 1e-12
    assert np.array_equal(bits(percentiles_numpy(q, ref)), bits(pct))


def test_an_all_nan_population():
    v = np.array([np.nan, -np.nan, np.nan], np.float32)
    s, n = sort_numpy(v)
    assert n == 0 and np.all(bits(s) == NAN_BITS)
    pct, less, eq = rank_numpy(s, n, np.array([0.5, np.nan], np.float32), False)
    assert np.all(bits(pct) == NAN_BITS) and less.tolist() == [0, -1] and eq.tolist() == [0, -1]
    assert np.all(bits(percentiles_numpy(v)) == NAN_BITS)


# ------------------------------------------------------------------------------------------------ smoothing
def word(S: int, c: int) -> int:
    return (c << COUNT_SHIFT) | S


def random_acc(g, h, w, cover=0.7) -> np.ndarray:
    """Counts 1..4 on a random support, sums anywhere in 0..65535 c with exact .5 ties of the mean among them."""
    c = g.integers(1, 5, (h, w)) * (g.random((h, w)) < cover)
    S = g.integers(0, 65536, (h, w)) * c
    tie = (c == 2) & (g.random((h, w)) < 0.5)
    S = np.where(tie, np.maximum(S - 1, 1), S)         # an odd sum over a count of two: the mean ends in .5
    return ((c.astype(np.int64) << COUNT_SHIFT) | S.astype(np.int64)) * (c > 0)


def smooth_loops(acc, taps, mask=None):
    """keep_heat_smooth pixel by pixel in Python integers, straight from its specification."""
    h, w = acc.shape
    r = len(taps) // 2
    t = [int(x) for x in taps]
    s = [[(int(acc[y, x]) >> COUNT_SHIFT) > 0 and (mask is None or mask[y][x] != 0) for x in range(w)] for y in range(h)]
    m = [[0] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            if s[y][x]:
                S, c = int(acc[y, x]) & ((1 << COUNT_SHIFT) - 1), int(acc[y, x]) >> COUNT_SHIFT
                m[y][x] = (2 * S + c) // (2 * c)
    A = [[sum(t[k + r] * m[y][x + k] for k in range(-r, r + 1) if 0 <= x + k < w) for x in range(w)] for y in range(h)]
    B = [[sum(t[k + r] * int(s[y][x + k]) for k in range(-r, r + 1) if 0 <= x + k < w) for x in range(w)] for y in range(h)]
    out = np.zeros((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            if s[y][x]:
                Nn = sum(t[k + r] * A[y + k][x] for k in range(-r, r + 1) if 0 <= y + k < h)
                D = sum(t[k + r] * B[y + k][x] for k in range(-r, r + 1) if 0 <= y + k < h)
                assert D >= t[r] * t[r] >= 1 and Nn < 1 << 46 and max(A[y]) < 1 << 31 and max(B[y]) <= 1 << 15
                out[y, x] = (1 << COUNT_SHIFT) | ((2 * Nn + D) // (2 * D))
    return out


HAND_TAPS = np.array([3, 0, 900, 0, 17000, 0, 0, 1, 5], np.int32)                # zero taps, not symmetric: radius 4


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (9, 11), (6, 5)])
def test_smooth_numpy_against_the_per_pixel_loops(shape):
    g = np.random.default_rng(shape[0] * 31 + shape[1])
    acc = random_acc(g, *shape)
    mask = (g.random(shape) < 0.8).astype(np.uint8)
    for taps in (gaussian_taps(0.8), gaussian_taps(4.7, 14), gaussian_taps(0.3, 1), HAND_TAPS):      # radii 3, 14 (beyond the raster), 1, 4
        assert np.array_equal(smooth_numpy(acc, taps), smooth_loops(acc, taps))
        assert np.array_equal(smooth_numpy(acc, taps, mask), smooth_loops(acc, taps, mask))


def test_smoothing_properties():
    g = np.random.default_rng(9)
    h, w = 23, 31
    support = g.random((h, w)) < 0.6
    mask = g.random((h, w)) < 0.7
    taps = gaussian_taps(2.0)
    for value, c in ((65535, 1), (65535, 3), (12345, 4), (0, 2)):                # a constant support stays constant, c > 1 and the top value included
        acc = np.where(support, word(value * c, c), 0).astype(np.int64)
        out = smooth_numpy(acc, taps, mask)
        assert np.array_equal(out, np.where(support & mask, word(value, 1), 0))
    acc = random_acc(g, h, w)
    for mk in (None, mask):
        S, c = unpack_numpy(smooth_numpy(acc, taps, mk))
        on = (unpack_numpy(acc)[1] > 0) & (True if mk is None else mk)
        assert np.array_equal(c > 0, on) and np.all(c[on] == 1) and np.all(S <= 65535) and np.all(S[~on] == 0)
    one = np.zeros((h, w), np.int64)
    one[11, 17] = word(3 * 40001 + 1, 3)                                         # a single supported pixel returns its own rounded mean
    for t in (taps, gaussian_taps(60, 127), HAND_TAPS, np.array([0, 1, 0], np.int32)):
        out = smooth_numpy(one, t)
        assert int(out[11, 17]) == word((2 * (3 * 40001 + 1) + 3) // 6, 1) and int(np.count_nonzero(out)) == 1
    big = smooth_numpy(acc[:3, :4], gaussian_taps(40, 127))                      # a radius far larger than the raster
    assert np.array_equal(big, smooth_loops(acc[:3, :4], gaussian_taps(40, 127)))
    assert np.array_equal(smooth_numpy(np.zeros((4, 5), np.int64), taps), np.zeros((4, 5), np.int64))


@pytest.mark.parametrize("sigma,radius", list(itertools.product((0.05, 0.3, 0.8, 4.7, 17.3, 60), (None, 1, 14, 56, 127))))
def test_gaussian_taps(sigma, radius):
    if radius is None and math.ceil(3 * sigma) > MAX_RADIUS:
        with pytest.raises(ValueError):
            gaussian_taps(sigma)
        return
    t = gaussian_taps(sigma, radius)
    r = math.ceil(3 * sigma) if radius is None else radius
    assert t.dtype == np.int32 and t.shape == (2 * r + 1,)
    assert np.array_equal(t, t[::-1]) and np.all(np.diff(t[r:]) <= 0) and t.min() >= 0
    assert int(t.sum()) <= 32768 and int(t[r]) >= 1
    assert int(t.sum()) > 32768 - (2 * r + 1)                                    # the floor loses less than one per tap


def test_clam_blur():
    assert clam_blur(224, 4) == (0.3 * 55 + 0.8, 56) and clam_blur(224, 16) == (0.3 * 13 + 0.8, 14)
    for patch, d, factor in ((224, 4, 2), (224, 16, 2), (256, 8, 2), (512, 32, 1)):
        sigma, r = clam_blur(patch, d, factor)
        ksize = (factor * patch // d) | 1
        assert r == (ksize - 1) // 2 and sigma == 0.3 * ((ksize - 1) / 2 - 1) + 0.8
        assert gaussian_taps(sigma, r).shape == (ksize,)
    with pytest.raises(ValueError):
        clam_blur(224, 512)                                                      # kernel size 1: nothing to blur
    with pytest.raises(ValueError):
        clam_blur(4096, 4)                                                       # radius beyond 127


def test_argument_errors():
    acc = random_acc(np.random.default_rng(1), 6, 7)
    ok = gaussian_taps(1.0)
    for bad in (np.array([20000, 10000, 20000], np.int32),                      # sums to more than 32768
                np.array([5, 0, 5], np.int32),                                   # centre zero
                np.array([5, -1, 9, 1, 5], np.int32), np.array([1, 2], np.int32), np.array([7], np.int32), np.ones(2 * 128 + 1, np.int32),
                np.array([0.25, 0.5, 0.25])):
        with pytest.raises(ValueError):
            check_taps(bad)
        with pytest.raises(ValueError):
            smooth_numpy(acc, bad)
    for radius in (0, 128):
        with pytest.raises(ValueError):
            gaussian_taps(1.0, radius)
    for kw in (dict(), dict(sigma=1.0, taps=ok), dict(taps=ok, radius=2), dict(sigma=0.0), dict(sigma=float("nan"))):
        with pytest.raises(ValueError):
            smooth_taps(**kw)
    for mask in (np.ones((6, 8), np.uint8), np.ones((7, 6), np.uint8), np.ones(42, np.uint8)):
        with pytest.raises(ValueError):
            smooth_numpy(acc, ok, mask)
    with pytest.raises(ValueError):
        smooth_numpy(acc.astype(np.int32), ok)
    for values in (np.zeros(0, np.float32), np.arange(5), np.zeros((2, 3), np.float32), torch.zeros(4, dtype=torch.int64)):      # M = 0, not floating
        with pytest.raises(ValueError):
            sort_numpy(values)
        with pytest.raises(ValueError):
            percentiles_numpy(values)
    with pytest.raises(ValueError):
        rank_numpy(*sort_numpy(np.ones(3, np.float32)), np.arange(3), False)


def test_the_engine_raises_before_any_device_call():
    """ValueError from the host-side checks of the three new methods, on a model that has no device (and would fail otherwise)."""
    from keep_amd.heatmap import ScoreReference, TileRaster
    m = KEEPModel()
    for values in (np.zeros(0, np.float32), np.arange(5), torch.zeros((2, 2))):
        with pytest.raises(ValueError):
            m.score_reference(values)
        with pytest.raises(ValueError):
            m.percentiles(values)
    with pytest.raises(ValueError):
        m.percentiles(np.ones(3, np.float32), reference=np.ones(3, np.float32))
    raster = TileRaster(torch.zeros((6, 7), dtype=torch.int64), 16, 224)
    for kw in (dict(), dict(sigma=1.0, radius=0), dict(sigma=1.0, radius=128), dict(taps=np.array([5, 0, 5], np.int32)),
               dict(taps=np.array([20000, 10000, 20000], np.int32)), dict(sigma=1.0, tissue=np.ones((6, 7), np.uint8))):
        with pytest.raises(ValueError):
            m.smooth_raster(raster, **kw)
    from keep_amd.region import TissueMask
    for tissue in (TissueMask(np.ones((6, 8), np.uint8), 16), TissueMask(np.ones((6, 7), np.uint8), 8)):
        with pytest.raises(ValueError):
            m.smooth_raster(raster, sigma=1.0, tissue=tissue)
    with pytest.raises(ValueError):
        m.smooth_raster(np.zeros((6, 7), np.int64), sigma=1.0)
    with pytest.raises(ValueError):
        ScoreReference(torch.zeros(3, dtype=torch.float64), torch.zeros(1, dtype=torch.int64))
