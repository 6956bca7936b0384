"""Heatmap percentiles and smoothing on the device against the numpy restatements, exactly: the sorted
population, n, less / eq / pct in both modes, the smoothed accumulator and what the calls downstream make of it."""
import ctypes as C

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel, _lib, wsi
from keep_amd.components import regions_numpy
from keep_amd.config import small_shape
from keep_amd.heatmap import (ScoreReference, TileRaster, gaussian_taps, mean_numpy, percentiles_numpy, quantize, rank_numpy, raster_numpy,
                              render_numpy, smooth_numpy, sort_numpy, unpack_numpy)
from keep_amd.model import _ptr, _stream
from keep_amd.region import TissueMask
from keep_amd.synth import synth_state_dict, synth_tile_family
from test_heatmap_display import FAMILIES, HAND_TAPS, NAN_BITS, bits, family, random_acc, word

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 4096, 4097, 70001)           # a wave, a block's round, the one-block path, many blocks


@pytest.fixture(scope="module")
def model():
    m = KEEPModel(precision="strict")
    m.load_state_dict(synth_state_dict(small_shape(2, 2), seed=5), strict=True)
    return m.to(DEV).eval()


def same(t: torch.Tensor, a: np.ndarray) -> bool:
    return t.dtype == torch.from_numpy(a).dtype and torch.equal(t.cpu(), torch.from_numpy(a))


def same_bits(t: torch.Tensor, a: np.ndarray) -> bool:
    return t.dtype == torch.float32 and a.dtype == np.float32 and np.array_equal(bits(t.cpu().numpy()), bits(a))


def outside_queries(v: np.ndarray, s: np.ndarray, n: int, count: int, seed: int) -> np.ndarray:
    """Queries for a reference population: below, above, equal to and between its values, zeros of both signs, NaNs."""
    g = np.random.default_rng(seed)
    pool = [np.array([-np.inf, np.inf, -3.4e38, 3.4e38, -0.0, 0.0, np.nan], np.float32), g.standard_normal(16).astype(np.float32)]
    if n:
        pool.append(g.choice(s[:n], 24))
        if n > 1:
            i = g.integers(0, n - 1, 24)
            lo, hi = s[:n][i].astype(np.float64), s[:n][i + 1].astype(np.float64)
            with np.errstate(invalid="ignore", over="ignore"):
                mid = (lo + (hi - lo) / 2).astype(np.float32)
            pool.append(np.where(np.isnan(mid), np.float32(0.25), mid))
    q = np.concatenate(pool)
    q = q[g.permutation(q.size)]
    return np.resize(q, count).astype(np.float32)


@pytest.mark.parametrize("M", SIZES)
def test_sort_and_rank_match_the_restatements(model, M):
    for name in FAMILIES:
        v = family(name, M)
        want, n = sort_numpy(v)
        ref = model.score_reference(torch.from_numpy(v).to(DEV))
        assert ref.M == M and same_bits(ref.sorted, want), (name, M)
        assert ref.n.dtype == torch.int64 and int(ref.n.item()) == n
        pct, less, eq = model._rank(ref, v, True, True, True)                       # the values among themselves
        wp, wl, we = rank_numpy(want, n, v, True)
        assert same_bits(pct, wp) and same(less, wl) and same(eq, we), (name, M)
        assert same_bits(model.percentiles(v), wp)
        q = outside_queries(v, want, n, M + 37 if M < 4096 else 1500, seed=M)       # N != M
        wp, wl, we = rank_numpy(want, n, q, False)
        got_less, got_eq = ref.rank(q)
        assert same(got_less, wl) and same(got_eq, we), (name, M)
        assert same_bits(ref.percentiles(q), wp) and same_bits(model.percentiles(q, ref), wp)
        assert np.array_equal(bits(wp), bits(percentiles_numpy(q, v)))             # two host arrays: the restatements agree with each other


def test_all_nan_empty_queries_and_two_runs(model):
    v = np.array([np.nan, -np.nan] * 2500 + [np.nan], np.float32)                   # 5001 values: the many-block path
    v.view(np.uint32)[::3] |= 0x1234
    for M in (3, 5001):
        ref = model.score_reference(v[:M])
        assert int(ref.n.item()) == 0 and np.all(bits(ref.sorted.cpu().numpy()) == NAN_BITS)
        assert np.all(bits(ref.percentiles(np.array([0.5, np.nan, -1.0], np.float32)).cpu().numpy()) == NAN_BITS)
        less, eq = ref.rank(np.array([0.5, np.nan], np.float32))
        assert less.tolist() == [0, -1] and eq.tolist() == [0, -1]
        assert np.all(bits(model.percentiles(v[:M]).cpu().numpy()) == NAN_BITS)
    ref = model.score_reference(family("normal", 300))
    assert ref.percentiles(np.zeros(0, np.float32)).shape == (0,) and ref.rank(torch.zeros(0))[0].shape == (0,)
    for name, M in (("specials", 70001), ("seven", 4096), ("normal", 12289)):
        v = torch.from_numpy(family(name, M, seed=2)).to(DEV)
        a, b = model.score_reference(v), model.score_reference(v)
        assert torch.equal(a.sorted.view(torch.int32), b.sorted.view(torch.int32)) and torch.equal(a.n, b.n)
        assert torch.equal(model.percentiles(v).view(torch.int32), model.percentiles(v).view(torch.int32))


def test_input_forms(model):
    v = family("specials", 777, seed=5)
    want, n = sort_numpy(v)
    wp = percentiles_numpy(v)
    v64 = v.astype(np.float64) * (1 + 2.0 ** -40)                                   # rounded to float32 first, on both sides
    v16 = torch.from_numpy(family("seven", 777)).to(torch.float16)
    assert np.array_equal(bits(percentiles_numpy(v64)), bits(wp))
    for form in (v, torch.from_numpy(v), torch.from_numpy(v).to(DEV), v64, torch.from_numpy(v64).to(DEV)):
        assert same_bits(model.score_reference(form).sorted, want)
        assert same_bits(model.percentiles(form), wp)
        assert same_bits(model.percentiles(form, model.score_reference(v)), percentiles_numpy(v, v))
    assert same_bits(model.percentiles(v16.to(DEV)), percentiles_numpy(v16.float().numpy()))
    strided = torch.from_numpy(np.stack([v, v], axis=1)).to(DEV)[:, 1]              # a non-contiguous device view
    assert same_bits(model.percentiles(strided), wp)
    host = ScoreReference(torch.from_numpy(want), torch.tensor([n]))
    with pytest.raises(ValueError):
        host.percentiles(v)
    for bad in (np.zeros(0, np.float32), np.arange(4), torch.zeros((2, 2), device=DEV)):
        with pytest.raises(ValueError):
            model.percentiles(bad)
        with pytest.raises(ValueError):
            model.score_reference(bad)
    with pytest.raises(ValueError):
        model.percentiles(v, reference=want)


def test_sort_and_rank_abi_rejects_bad_arguments(model):
    lib, h, st = _lib.load(), model._handle, _stream(torch.device(DEV))
    M, N = 100, 7
    values = torch.from_numpy(family("normal", M)).to(DEV)
    out = torch.empty(M, dtype=torch.float32, device=DEV)
    n = torch.zeros(2, dtype=torch.int64, device=DEV)
    q = torch.zeros(N, dtype=torch.float32, device=DEV)
    pct = torch.empty(N, dtype=torch.float32, device=DEV)
    less = torch.empty(N, dtype=torch.int32, device=DEV)
    eq = torch.empty(N, dtype=torch.int32, device=DEV)
    null = C.c_void_p(0)

    def off(t, nbytes):
        return C.c_void_p(t.data_ptr() + nbytes)

    def sort(v=_ptr(values), m=M, o=_ptr(out), nn=_ptr(n)):
        return lib.keep_sort_f32(h, v, m, o, nn, st)

    assert sort() == _lib.KEEP_OK
    for kw in [dict(v=null), dict(o=null), dict(nn=null), dict(m=0), dict(m=-1), dict(m=1 << 24), dict(v=off(values, 2)), dict(o=off(out, 1)),
               dict(nn=off(n, 4))]:
        assert sort(**kw) == _lib.KEEP_EINVAL, kw
        assert lib.keep_last_error(h)
    assert lib.keep_sort_f32(None, _ptr(values), M, _ptr(out), _ptr(n), st) == _lib.KEEP_EINVAL
    assert sort(o=_ptr(values)) == _lib.KEEP_OK                                       # in place
    torch.cuda.synchronize()
    assert torch.equal(values.view(torch.int32), out.view(torch.int32)) and int(n[0]) == M

    def rank(s=_ptr(out), m=M, nn=_ptr(n), qq=_ptr(q), k=N, self_=0, p=_ptr(pct), l=_ptr(less), e=_ptr(eq)):
        return lib.keep_rank_f32(h, s, m, nn, qq, k, self_, p, l, e, st)

    assert rank() == _lib.KEEP_OK and rank(l=null, e=null) == _lib.KEEP_OK and rank(p=null) == _lib.KEEP_OK
    assert rank(k=0, qq=null) == _lib.KEEP_OK                                         # no queries is no error
    for kw in [dict(s=null), dict(nn=null), dict(qq=null), dict(m=0), dict(m=1 << 24), dict(k=-1), dict(k=1 << 24), dict(self_=2), dict(self_=-1),
               dict(p=null, l=null, e=null), dict(s=off(out, 2)), dict(nn=off(n, 4)), dict(qq=off(q, 2)), dict(p=off(pct, 1)), dict(l=off(less, 2)),
               dict(e=off(eq, 3))]:
        assert rank(**kw) == _lib.KEEP_EINVAL, kw
        assert lib.keep_last_error(h)
    assert lib.keep_rank_f32(None, _ptr(out), M, _ptr(n), _ptr(q), N, 0, _ptr(pct), _ptr(less), _ptr(eq), st) == _lib.KEEP_EINVAL
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ smoothing
SHAPES = ((1, 1), (1, 7), (7, 1), (5, 300), (67, 129), (130, 70), (257, 259))
TAPS = {1: gaussian_taps(0.6, 1), 3: gaussian_taps(0.8), 14: gaussian_taps(4.7, 14), 127: gaussian_taps(45.0, 127), 4: HAND_TAPS}


def supports(g, h, w):
    """name -> accumulator int64 [h,w]."""
    yy, xx = np.mgrid[:h, :w]
    values = g.integers(0, 65536, (h, w)).astype(np.int64)
    one = np.zeros((h, w), np.int64)
    one[h // 2, w // 3] = word(2 * 31000 + 1, 2)
    return {"full": (np.int64(1) << 40) | values, "empty": np.zeros((h, w), np.int64), "checkerboard": np.where((yy + xx) % 2 == 0, (np.int64(1) << 40) | values, 0),
            "one": one, "random": random_acc(g, h, w), "top": np.full((h, w), word(3 * 65535, 3), np.int64)}


def raster_of(model, acc: np.ndarray, d: int = 16) -> TileRaster:
    return TileRaster(torch.from_numpy(acc).to(DEV), d, 224, model=model)


@pytest.mark.parametrize("shape", SHAPES)
def test_smoothing_matches_the_restatement(model, shape):
    g = np.random.default_rng(shape[0] * 1000 + shape[1])
    h, w = shape
    mask = g.random(shape) < 0.75
    tissue = TissueMask(mask, 16)
    for name, acc in supports(g, h, w).items():
        r = raster_of(model, acc)
        for radius, taps in TAPS.items():
            got = model.smooth_raster(r, taps=taps)
            assert got.shape == shape and got.tiles == r.tiles and got.downsample == 16 and got.patch == 224
            assert same(got.acc, smooth_numpy(acc, taps)), (name, radius)
            assert same(model.smooth_raster(r, taps=taps, tissue=tissue).acc, smooth_numpy(acc, taps, mask)), (name, radius, "mask")
    acc = supports(g, h, w)["random"]
    assert same(model.smooth_raster(raster_of(model, acc), sigma=0.8).acc, smooth_numpy(acc, gaussian_taps(0.8)))
    assert same(model.smooth_raster(raster_of(model, acc), sigma=2.0, radius=3).acc, smooth_numpy(acc, gaussian_taps(2.0, 3)))


def test_a_thumbnail_sized_raster_at_clam_radius(model):
    """1100 x 1030 at radius 56 (CLAM's at downsample 4): more than one row segment, column tiles that end inside the raster, and
    the calls downstream fed with the smoothed raster."""
    h, w, d = 1100, 1030, 4
    g = np.random.default_rng(56)
    yy, xx = np.mgrid[:h, :w]
    blob = ((yy - 500) ** 2 / 400.0 ** 2 + (xx - 480) ** 2 / 350.0 ** 2 < 1) | ((yy > 900) & (xx > 800))
    acc = np.where(blob, random_acc(g, h, w, cover=0.97), 0)
    mask = ((yy // 40 + xx // 56) % 5 != 0)
    tissue = TissueMask(mask, d)
    taps = gaussian_taps(17.3, 56)
    r = raster_of(model, acc, d)
    want = smooth_numpy(acc, taps, mask)
    got = model.smooth_raster(r, taps=taps, tissue=tissue)
    assert same(got.acc, want)
    for uncovered in (0.0, -1.0):
        assert same(got.mean(uncovered), mean_numpy(want, uncovered)[0])
    assert same(got.count, unpack_numpy(want)[1])
    kw = dict(alpha=0.7, window=(0.2, 0.8), min_value=0.1)
    assert same(model.render_heatmap(got, None, **kw), render_numpy(want, None, **kw))
    assert same(model.render_heatmap(got, None, tissue=tissue, **kw), render_numpy(want, None, mask=mask, **kw))
    S, c = unpack_numpy(want)
    for mk, ts in ((None, None), (mask, tissue)):
        above = (c > 0) & (S > quantize(0.5) * c.astype(np.int64)) & (True if mk is None else mk)
        labels, table = regions_numpy(above, 8, 20, acc=want)
        regions = wsi.segment_regions(got, 0.5, tissue=ts, min_area=20, model=model)
        assert table.shape[0] >= 1 and same(regions.table, table) and same(regions.labels, labels)


def test_smoothing_twice_and_two_runs(model):
    g = np.random.default_rng(77)
    acc = random_acc(g, 90, 140)
    taps = gaussian_taps(3.0)
    r = raster_of(model, acc)
    a, b = model.smooth_raster(r, taps=taps), model.smooth_raster(r, taps=taps)
    assert torch.equal(a.acc, b.acc) and same(r.acc, acc)                            # the input is left as it was
    once = smooth_numpy(acc, taps)
    assert same(model.smooth_raster(a, taps=taps).acc, smooth_numpy(once, taps))     # the output is an ordinary accumulator
    assert same(model.smooth_raster(r, taps=torch.from_numpy(taps).to(DEV)).acc, once)
    for bad in (dict(), dict(sigma=1.0, radius=0), dict(sigma=1.0, radius=128), dict(taps=np.array([5, 0, 5], np.int32)),
                dict(taps=np.array([20000, 10000, 20000], np.int32)), dict(sigma=1.0, tissue=TissueMask(np.ones((90, 141), np.uint8), 16)),
                dict(sigma=1.0, tissue=TissueMask(np.ones((90, 140), np.uint8), 8))):
        with pytest.raises(ValueError):
            model.smooth_raster(r, **bad)


def test_smooth_abi_rejects_bad_arguments(model):
    lib, h, st = _lib.load(), model._handle, _stream(torch.device(DEV))
    H, W = 20, 24
    acc = torch.from_numpy(random_acc(np.random.default_rng(3), H, W)).to(DEV)
    out = torch.zeros((H + 1, W), dtype=torch.int64, device=DEV)
    mask = torch.ones((H, W), dtype=torch.uint8, device=DEV)
    taps = torch.from_numpy(gaussian_taps(1.0)).to(DEV)
    null = C.c_void_p(0)

    def off(t, nbytes):
        return C.c_void_p(t.data_ptr() + nbytes)

    def smooth(a=_ptr(acc), Hh=H, Ww=W, m=_ptr(mask), t=_ptr(taps), r=3, o=_ptr(out)):
        return lib.keep_heat_smooth(h, a, Hh, Ww, m, t, r, o, st)

    assert smooth() == _lib.KEEP_OK and smooth(m=null) == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert same(out[:H], smooth_numpy(acc.cpu().numpy(), gaussian_taps(1.0))) and int(out[H].abs().max()) == 0
    for kw in [dict(a=null), dict(o=null), dict(t=null), dict(a=off(acc, 4)), dict(o=off(out, 4)), dict(t=off(taps, 2)), dict(o=_ptr(acc)), dict(r=0),
               dict(r=128), dict(r=-3), dict(Hh=0), dict(Ww=-1), dict(Hh=1 << 16, Ww=(1 << 14) + 1)]:
        assert smooth(**kw) == _lib.KEEP_EINVAL, kw
        assert lib.keep_last_error(h)
    assert lib.keep_heat_smooth(None, _ptr(acc), H, W, null, _ptr(taps), 3, _ptr(out), st) == _lib.KEEP_EINVAL
    torch.cuda.synchronize()


def test_end_to_end_at_depth_2(model):
    """segment_heatmap with percentile, blur and tissue equals percentiles_numpy -> raster_numpy -> smooth_numpy fed with the device's
    own refine output; the default keywords give the accumulator they gave before."""
    P, d = 224, 16
    tiles = synth_tile_family("stain_field", 0, 12, torch.device(DEV), seed=3)
    region = tiles.reshape(3, 4, P, P, 3).permute(0, 2, 1, 3, 4).reshape(3 * P, 4 * P, 3).contiguous()
    origin = (2 * P, P)
    feats, coords = model.encode_region(region, P, P // 2, origin=origin)
    shape = (region.shape[0] // d + 1, region.shape[1] // d + 2)
    gen = torch.Generator().manual_seed(1)
    classifier = torch.nn.functional.normalize(torch.randn(feats.shape[1], 2, generator=gen), dim=0).to(DEV)
    rc, rmean, _ = wsi.refine(wsi._probs(model, classifier, feats), coords.cpu(), P, True, model=model)
    rc, p = rc.cpu().numpy(), rmean[:, 1].cpu().numpy()
    args = (classifier, feats, coords, d, shape)
    kw = dict(patch_size=P, overlap=True, origin=origin, model=model)
    plain = raster_numpy(rc, p, P, d, shape, origin)
    assert same(wsi.segment_heatmap(*args, **kw).acc, plain)
    assert same(wsi.segment_heatmap(*args, **kw, percentile=False, reference=None, blur_sigma=None, blur_radius=None, tissue=None).acc, plain)
    g = np.random.default_rng(2)
    mask = g.random(shape) < 0.8
    tissue = TissueMask(mask, d)
    ranked = raster_numpy(rc, percentiles_numpy(p), P, d, shape, origin)
    assert not np.array_equal(ranked, plain)
    assert same(wsi.segment_heatmap(*args, **kw, percentile=True).acc, ranked)
    got = wsi.segment_heatmap(*args, **kw, percentile=True, blur_sigma=2.5, tissue=tissue)
    assert got.tiles == feats.shape[0] and same(got.acc, smooth_numpy(ranked, gaussian_taps(2.5), mask))
    assert same(wsi.segment_heatmap(*args, **kw, blur_sigma=2.5, blur_radius=4).acc, smooth_numpy(plain, gaussian_taps(2.5, 4)))
    population = g.random(500).astype(np.float32)
    ref = model.score_reference(population)
    against = raster_numpy(rc, percentiles_numpy(p, population), P, d, shape, origin)
    assert same(wsi.segment_heatmap(*args, **kw, percentile=True, reference=ref).acc, against)
    assert same(model.render_heatmap(got, None, tissue=tissue), render_numpy(smooth_numpy(ranked, gaussian_taps(2.5), mask), None, mask=mask))
    for bad in (dict(reference=ref), dict(percentile=True, reference=population), dict(blur_radius=3), dict(tissue=tissue),
                dict(blur_sigma=2.0, blur_radius=0), dict(blur_sigma=2.0, tissue=TissueMask(mask, 8)), dict(blur_sigma=2.0, tissue=mask)):
        with pytest.raises(ValueError):
            wsi.segment_heatmap(*args, **kw, **bad)
