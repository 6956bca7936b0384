"""The heatmap's host side (keep_amd/heatmap.py): the numpy restatements the device is held to are themselves
held here to independent statements of the rule -- a per-pixel membership test for the accumulator (no slices, no clipping), Python
scalar arithmetic for the quantisation, the reference's float-slice painting for the predicted mask and per-pixel Python integers
for the render -- plus every ValueError and the tile cap.  No GPU."""
import itertools

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel
from keep_amd import heatmap as hm
from keep_amd.heatmap import (MAX_TILES, TileRaster, check_raster_args, colormap, mean_numpy, pred_numpy, raster_numpy, render_numpy,
                              unpack_numpy)

DOWNSAMPLES = (1, 3, 4, 16, 32)
PATCHES = (224, 256, 512)


def tie_values():
    """float32 values whose float32 product with 65535 ends in exactly .5, below an even and below an odd integer: the cases that
    tell round-half-to-even from round-half-up."""
    out = {}
    for k in range(20000, 40000):
        v = np.float32((k + 0.5) / 65535)
        p = float(v * np.float32(65535))
        if p - np.floor(p) == 0.5 and (int(np.floor(p)) & 1) not in out:
            out[int(np.floor(p)) & 1] = v
            if len(out) == 2:
                break
    assert len(out) == 2, "no exact ties found: the tie test would show nothing"
    return [out[0], out[1]]


SPECIAL_VALUES = [np.nan, np.inf, -np.inf, -0.3, 1.7, 0.0, 1.0, -0.0, 1e-30, 0.5] + tie_values()


def case(d, P, seed=0):
    """Tiles and a raster for one (downsample, patch): random off-lattice coords, lattices of step P/2 and P/4 (4 and 16 tiles per
    pixel), footprints cut by every raster edge and tiles wholly outside, negative coords, a non-zero origin, duplicates and the
    special values -> (coords int64 [N,2], values fp32 [N], shape, origin)."""
    g = np.random.default_rng(1000 * d + P + seed)
    w, h = (5 * P) // d + 5, (4 * P) // d + 3
    origin = (-2 * d, 5 * d)
    x_lo, x_hi, y_lo, y_hi = origin[0] - P - 10, origin[0] + w * d + 10, origin[1] - P - 10, origin[1] + h * d + 10
    rnd = np.stack([g.integers(x_lo, x_hi, 40), g.integers(y_lo, y_hi, 40)], axis=1)
    lat2 = np.array([(origin[0] - P // 2 + i * (P // 2) + 1, origin[1] - P // 2 + j * (P // 2) + 2) for i in range(7) for j in range(5)])
    lat4 = np.array([(origin[0] + 7 + i * (P // 4), origin[1] + 3 + j * (P // 4)) for i in range(8) for j in range(6)])
    far = np.array([(x_hi + 5 * P, 0), (0, y_lo - 5 * P), (-(1 << 35), 17), (1 << 35, 1 << 36)])                # wholly outside
    edge = np.array([(origin[0] + w * d - P // 3, origin[1] + h * d - P // 3), (origin[0] + w * d - 1, origin[1] + 9), (origin[0] + 11, origin[1] + h * d - 1)])
    coords = np.concatenate([rnd, lat2, lat4, far, edge, rnd[:6], lat2[:3]]).astype(np.int64)
    values = g.random(len(coords)).astype(np.float32)
    values[g.choice(len(coords), len(SPECIAL_VALUES), replace=False)] = SPECIAL_VALUES
    return coords, values, (h, w), origin


def python_quantize(v):
    """-> q or None (skipped), in Python scalars: round() is round-half-to-even on the float32 product."""
    v = np.float32(v)
    if v != v:
        return None
    c = min(max(float(v), 0.0), 1.0)
    return round(float(np.float32(c) * np.float32(65535)))


def brute_force(coords, values, P, d, shape, origin):
    """For every raster pixel the tiles whose footprint contains it by the floor rule: membership per (tile, column) and (tile, row)
    from Python-integer floor divisions, no slices and no clipping -> (sum int64 [h,w], count int64 [h,w])."""
    h, w = shape
    qs = [python_quantize(v) for v in values]
    live = [n for n, q in enumerate(qs) if q is not None]
    x0 = np.array([(int(coords[n][0]) - origin[0]) // d for n in live])
    x1 = np.array([(int(coords[n][0]) - origin[0] + P) // d for n in live])
    y0 = np.array([(int(coords[n][1]) - origin[1]) // d for n in live])
    y1 = np.array([(int(coords[n][1]) - origin[1] + P) // d for n in live])
    q = np.array([qs[n] for n in live], dtype=np.int64)
    px, py = np.arange(w), np.arange(h)
    col = ((x0[:, None] <= px) & (px < x1[:, None])).astype(np.int64)            # [n, w]
    row = ((y0[:, None] <= py) & (py < y1[:, None])).astype(np.int64)            # [n, h]
    return (row * q[:, None]).T @ col, row.T @ col


@pytest.mark.parametrize("d,P", list(itertools.product(DOWNSAMPLES, PATCHES)))
def test_raster_numpy_against_a_per_pixel_brute_force(d, P):
    coords, values, shape, origin = case(d, P)
    acc = raster_numpy(coords, values, P, d, shape, origin)
    assert acc.dtype == np.int64 and acc.shape == shape
    s, c = unpack_numpy(acc)
    want_s, want_c = brute_force(coords, values, P, d, shape, origin)
    assert np.array_equal(s, want_s) and np.array_equal(c, want_c)
    assert c.max() >= 16 and (c == 0).any()                                  # 16 tiles share a pixel somewhere; something is uncovered
    for edge in (c[0], c[-1], c[:, 0], c[:, -1]):
        assert edge.any()                                                        # footprints are cut by every raster edge
    mean, count = mean_numpy(acc, uncovered=-1.0)
    assert mean.dtype == np.float32 and count.dtype == np.int32 and np.array_equal(count, want_c)
    on = want_c > 0
    assert np.array_equal(mean[on], (want_s[on] / (65535.0 * want_c[on])).astype(np.float32)) and (mean[~on] == -1.0).all()
    assert np.array_equal(pred_numpy(acc), np.where(want_s > 0, 255, 0))


def test_quantisation_rounds_half_to_even_and_skips_nan():
    even, odd = tie_values()
    q, skip = hm.quantize_numpy(np.array([even, odd, np.nan, np.inf, -np.inf, 2.0, -1.0, 1.0, 0.0], np.float32))
    pe, po = float(even * np.float32(65535)), float(odd * np.float32(65535))
    assert q[0] == int(pe - 0.5) and q[0] % 2 == 0                           # the tie below an even integer goes down
    assert q[1] == int(po + 0.5) and q[1] % 2 == 0                           # the tie below an odd integer goes up
    assert list(q[3:]) == [65535, 0, 65535, 0, 65535, 0] and list(skip) == [False, False, True] + [False] * 6
    one = raster_numpy(np.zeros((3, 2), np.int64), np.array([np.nan, 0.25, np.nan], np.float32), 32, 16, (4, 4))
    s, c = unpack_numpy(one)
    assert c.max() == 1 and s.max() == python_quantize(0.25)               # a NaN tile is not counted


@pytest.mark.parametrize("d,P", [(3, 224), (16, 256), (32, 512)])
def test_any_split_over_calls_gives_the_same_accumulator(d, P):
    coords, values, shape, origin = case(d, P, seed=1)
    whole = raster_numpy(coords, values, P, d, shape, origin)
    g = np.random.default_rng(d)
    for parts in (2, 3, 7):
        order = g.permutation(len(coords))
        acc = None
        for idx in np.array_split(order, parts):
            acc = raster_numpy(coords[idx], values[idx], P, d, shape, origin, into=acc)
        assert np.array_equal(acc, whole)
    empty = raster_numpy(np.zeros((0, 2), np.int64), np.zeros(0, np.float32), P, d, shape, origin, into=whole.copy())
    assert np.array_equal(empty, whole)


@pytest.mark.parametrize("d,P", [(1, 224), (4, 224), (16, 224), (16, 256), (32, 512), (64, 448)])
def test_pred_equals_the_float_slice_painting(d, P):
    """segment_utils.py:134-140 written afresh: mask[int(y / d):int(y / d + P / d), int(x / d):int(x / d + P / d)] = 255 for the tiles
    above the threshold (float arithmetic; exact for non-negative coords and power-of-two d)."""
    g = np.random.default_rng(P + d)
    shape = ((6 * P) // d + 2, (7 * P) // d + 1)
    coords = np.stack([g.integers(0, 7 * P, 120), g.integers(0, 6 * P, 120)], axis=1).astype(np.int64)
    coords = np.concatenate([coords, [[i * (P // 2), j * (P // 2)] for i in range(6) for j in range(5)]]).astype(np.int64)
    p = g.random(len(coords)).astype(np.float32)
    thd = 0.6
    want = np.zeros(shape, np.uint8)
    for (x, y), pv in zip(coords.tolist(), p):
        if pv > np.float32(thd):
            want[int(y / d):int(y / d + P / d), int(x / d):int(x / d + P / d)] = 255
    acc = raster_numpy(coords, (p > np.float32(thd)).astype(np.float32), P, d, shape)
    assert np.array_equal(pred_numpy(acc), want) and 0 < (want == 255).mean() < 1


# ------------------------------------------------------------------------------------------------ render
def render_by_pixel(acc, under, lut, a, lo16, hi16, min16, mask):
    """The render rule in Python integers, pixel by pixel."""
    h, w = acc.shape
    out = np.empty((h, w, 3), np.uint8)
    for y in range(h):
        for x in range(w):
            word = int(acc[y, x]) & ((1 << 64) - 1)
            S, c = word & ((1 << 40) - 1), word >> 40
            u = [int(v) for v in under[y, x][:3]]
            if c > 0 and (mask is None or mask[y, x]) and S >= min16 * c:
                idx = 0 if S < lo16 * c else min(max((2 * 255 * (S - lo16 * c) + (hi16 - lo16) * c) // (2 * (hi16 - lo16) * c), 0), 255)
                u = [(a * int(lut[idx][ch]) + (256 - a) * u[ch] + 128) >> 8 for ch in range(3)]
            out[y, x] = u
    return out


def render_case():
    coords, values, shape, origin = case(16, 224, seed=2)
    acc = raster_numpy(coords, values, 224, 16, shape, origin)
    g = np.random.default_rng(4)
    h, w = shape
    big = g.integers(0, 256, (h + 5, w + 9, 4), dtype=np.uint8)
    thumb = big[3:3 + h, 4:4 + w]                                             # an RGBA view with strided rows
    mask = (g.random(shape) < 0.7).astype(np.uint8)
    return acc, thumb, mask


def test_render_numpy_against_per_pixel_python():
    acc, thumb, mask = render_case()
    lut = colormap("jet")
    for alpha, window, min_value, m, cm in [(0.4, (0.0, 1.0), 0.0, None, "jet"), (0.75, (0.2, 0.7), 0.3, mask, "jet"), (1.0, (0.45, 0.55), 0.0, mask, "gray"),
                                            (0.5, (0.0, 0.001), 0.5, None, lut[::-1].copy())]:
        a, lo16, hi16, min16, _ = hm.render_args(alpha, window, min_value, (255, 255, 255))
        got = render_numpy(acc, thumb, alpha, cm, m, window, min_value)
        assert got.shape == acc.shape + (3,) and got.dtype == np.uint8
        assert np.array_equal(got, render_by_pixel(acc, thumb, colormap(cm), a, lo16, hi16, min16, m))
    bg = (10, 200, 30)
    under = np.broadcast_to(np.array(bg, np.uint8), acc.shape + (3,))
    assert np.array_equal(render_numpy(acc, None, 0.4, background=bg), render_by_pixel(acc, under, lut, 102, 0, 65535, 0, None))


def test_render_numpy_properties():
    acc, thumb, mask = render_case()
    s, c = unpack_numpy(acc)
    rgb, lut = thumb[..., :3], colormap("jet")
    assert np.array_equal(render_numpy(acc, thumb, alpha=0.0), rgb)                       # a = 0: the thumbnail
    full = render_numpy(acc, thumb, alpha=1.0)                                               # a = 256: the table itself where shown
    idx = np.clip((2 * 255 * s + 65535 * c) // np.maximum(2 * 65535 * c, 1), 0, 255)
    assert np.array_equal(full[c > 0], lut[idx[c > 0]]) and np.array_equal(full[c == 0], rgb[c == 0])
    m = render_numpy(acc, thumb, alpha=1.0, mask=mask)
    assert np.array_equal(m[mask == 0], rgb[mask == 0]) and np.array_equal(m[(mask == 1) & (c > 0)], full[(mask == 1) & (c > 0)])
    low = render_numpy(acc, thumb, alpha=1.0, min_value=0.5)
    below = (c > 0) & (s < hm.quantize(0.5) * c.astype(np.int64))
    assert below.any() and np.array_equal(low[below], rgb[below]) and np.array_equal(low[~below], full[~below])
    # window clamping at both ends
    win = render_numpy(acc, thumb, alpha=1.0, window=(0.4, 0.6), colormap="gray")
    lo16, hi16 = hm.quantize(0.4), hm.quantize(0.6)
    under_lo, over_hi = (c > 0) & (s <= lo16 * c.astype(np.int64)), (c > 0) & (s >= hi16 * c.astype(np.int64))
    assert under_lo.any() and over_hi.any() and (win[under_lo] == 0).all() and (win[over_hi] == 255).all()


def test_colour_index_rounds_half_up():
    """sum = count * 65535 * (2 i + 1) / 510 is an integer for count = 2 (65535 = 257 * 255): the windowed mean sits exactly half way
    between index i and i + 1 and must go up."""
    i = np.arange(255, dtype=np.int64)
    s = 257 * (2 * i + 1)                                                        # count 2: 2 * 65535 * (2 i + 1) / 510
    acc = ((2 << 40) | s).reshape(1, -1).astype(np.int64)
    out = render_numpy(acc, None, alpha=1.0, colormap="gray")
    assert np.array_equal(out[0, :, 0], i + 1)
    out = render_numpy(acc - 1, None, alpha=1.0, colormap="gray")               # one unit below the tie: down
    assert np.array_equal(out[0, :, 0], i)


def test_colour_tables():
    jet, gray = colormap("jet"), colormap("gray")
    assert jet.shape == gray.shape == (256, 3) and jet.dtype == gray.dtype == np.uint8
    assert np.array_equal(gray[:, 0], np.arange(256)) and (gray[:, 0] == gray[:, 1]).all() and (gray[:, 1] == gray[:, 2]).all()
    assert jet[0, 2] > jet[0, 0] and jet[255, 0] > jet[255, 2] and jet[128, 1] == 255       # blue end, red end, green in the middle
    for k, ch in zip((3, 2, 1), range(3)):                                                   # the formula, in Python integers
        assert [int(v) for v in jet[:, ch]] == [min(max((765 - 2 * abs(4 * i - 255 * k) + 1) // 2, 0), 255) for i in range(256)]
    own = np.arange(768, dtype=np.int64).reshape(256, 3).astype(np.uint8)
    assert np.array_equal(colormap(own), own) and np.array_equal(colormap(torch.from_numpy(own)), own)


# ------------------------------------------------------------------------------------------------ errors and the cap
def test_value_errors():
    ok = dict(patch=224, downsample=16, shape=(10, 12), origin=(0, 0))
    assert check_raster_args(**ok) == (224, 16, (10, 12), (0, 0))
    for bad in [dict(downsample=0), dict(downsample=225), dict(downsample=-16), dict(downsample=2.5), dict(downsample=True), dict(patch=0),
                dict(patch=(1 << 30) + 1, downsample=1), dict(shape=(0, 5)), dict(shape=(5, -1)), dict(shape=(1 << 15, (1 << 15) + 1)), dict(shape=(4,)),
                dict(origin=(8, 0)), dict(origin=(0, -24)), dict(origin=(0,)), dict(origin=(1.5, 0)), dict(origin=(1 << 44, 0))]:
        with pytest.raises(ValueError):
            check_raster_args(**{**ok, **bad})
    assert check_raster_args(224, 16, (1 << 15, 1 << 15), (-32, 1 << 40))[2] == (1 << 15, 1 << 15)
    c, v = np.zeros((5, 2), np.int64), np.zeros(5, np.float32)
    for cc, vv in [(c[:, :1], v), (c.reshape(-1), v), (c, v[:4]), (c, v.reshape(5, 1)), (c.astype(np.float32), v), (c, v.astype(np.int32)),
                   (c.astype(bool), v)]:
        with pytest.raises(ValueError):
            raster_numpy(cc, vv, 224, 16, (10, 12))
        with pytest.raises(ValueError):
            KEEPModel().tile_raster(torch.from_numpy(cc), vv, 224, 16, (10, 12))
    m = KEEPModel()                                                              # no device is reached: the checks come first
    for kw in [dict(downsample=0), dict(downsample=448), dict(shape=(1 << 16, 1 << 15)), dict(origin=(3, 0))]:
        with pytest.raises(ValueError):
            m.tile_raster(c, v, **{**dict(patch_size=224, downsample=16, shape=(10, 12)), **kw})
    with pytest.raises(ValueError):
        m.tile_raster(c, v, 224, 16, (10, 12), into=np.zeros((10, 12), np.int64))
    with pytest.raises(ValueError):
        raster_numpy(c, v, 224, 16, (10, 12), into=np.zeros((10, 13), np.int64))
    r = TileRaster(torch.zeros((10, 12), dtype=torch.int64), 16, 224)
    for kw in [dict(downsample=8), dict(patch_size=256), dict(shape=(12, 10)), dict(origin=(16, 0))]:
        with pytest.raises(ValueError, match="into="):
            m.tile_raster(c, v, **{**dict(patch_size=224, downsample=16, shape=(10, 12), into=r), **kw})
    for kw in [dict(alpha=-0.1), dict(alpha=1.01), dict(alpha=float("nan")), dict(window=(0.5, 0.5)), dict(window=(0.7, 0.2)), dict(window=(0.5,)),
               dict(window=(0.0, float("nan"))), dict(window=(1.0, 2.0)), dict(min_value=float("nan")), dict(background=(0, 0)),
               dict(background=(0, 0, 256)), dict(background=(0.5, 0, 0)), dict(colormap="viridis"), dict(colormap=np.zeros((256, 4), np.uint8)),
               dict(colormap=np.zeros((256, 3), np.int32)), dict(thumbnail=np.zeros((10, 13, 3), np.uint8)), dict(thumbnail=np.zeros((10, 12, 3), np.float32)),
               dict(thumbnail=np.zeros((10, 12, 2), np.uint8))]:
        with pytest.raises(ValueError):
            render_numpy(r.acc.numpy(), **kw)
        with pytest.raises(ValueError):
            m.render_heatmap(r, **kw)
    with pytest.raises(ValueError):
        render_numpy(r.acc.numpy(), mask=np.zeros((10, 13), np.uint8))
    from keep_amd.region import TissueMask
    for tissue in (TissueMask(np.ones((10, 12), np.uint8), 8), TissueMask(np.ones((10, 13), np.uint8), 16), np.ones((10, 12), np.uint8)):
        with pytest.raises(ValueError):
            m.render_heatmap(r, tissue=tissue)
    with pytest.raises(ValueError):
        m.render_heatmap(r.acc)
    for acc in (torch.zeros((4, 4), dtype=torch.int32), torch.zeros((4, 4, 1), dtype=torch.int64), torch.zeros((4, 8), dtype=torch.int64)[:, ::2],
                np.zeros((4, 4), np.int64)):
        with pytest.raises(ValueError):
            TileRaster(acc, 16, 224)
    with pytest.raises(ValueError, match="host"):
        r.mean()


def test_the_tile_cap_is_enforced_by_counting():
    assert MAX_TILES == 2 ** 24 - 1 and MAX_TILES * 65535 < 2 ** 40
    r = TileRaster(torch.zeros((4, 4), dtype=torch.int64), 16, 224, tiles=MAX_TILES - 5)
    r.claim(3)
    assert r.tiles == MAX_TILES - 2
    with pytest.raises(ValueError, match="2\\^24 - 1"):
        r.claim(3)
    assert r.tiles == MAX_TILES - 2                                              # a refused claim adds nothing
    c, v = np.zeros((3, 2), np.int64), np.zeros(3, np.float32)
    with pytest.raises(ValueError, match="2\\^24 - 1"):                          # through the public call: raised before any device work
        KEEPModel().tile_raster(c, v, 224, 16, (4, 4), into=r)
    r.claim(2)
    assert r.tiles == MAX_TILES
    with pytest.raises(ValueError):
        r.claim(1)
    with pytest.raises(ValueError):
        r.claim(-1)
    with pytest.raises(ValueError):
        TileRaster(torch.zeros((4, 4), dtype=torch.int64), 16, 224, tiles=MAX_TILES + 1)
