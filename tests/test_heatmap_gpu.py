"""The heatmap on the MI355X: keep_heat_accumulate / keep_heat_mean / keep_heat_render, KEEPModel.tile_raster /
render_heatmap, wsi.segment_heatmap / segment_pred_mask.

Everything is integer arithmetic (the mean: one float64 division rounded to float32 once), so every comparison is exact: the
yardsticks are keep_amd.heatmap.raster_numpy / mean_numpy / pred_numpy / render_numpy, which tests/test_heatmap.py holds to
independent per-pixel statements of the rule."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel, _lib, wsi
from keep_amd.config import small_shape
from keep_amd.heatmap import (MAX_TILES, TileRaster, colormap, mean_numpy, pred_numpy, raster_numpy, render_numpy, unpack_numpy)
from keep_amd.model import _ptr, _stream
from keep_amd.region import TissueMask
from keep_amd.synth import synth_state_dict, synth_thumbnail, synth_tile_family
from test_heatmap import DOWNSAMPLES, PATCHES, case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def model():
    m = KEEPModel(precision="strict")
    m.load_state_dict(synth_state_dict(small_shape(2, 2), seed=5), strict=True)
    return m.to(DEV).eval()


def same(t: torch.Tensor, a: np.ndarray) -> bool:
    return t.dtype == torch.from_numpy(a).dtype and torch.equal(t.cpu(), torch.from_numpy(a))


def check_raster(r: TileRaster, want: np.ndarray):
    """Accumulator, sum, count, mean and pred of a device raster against the restatement of the same tiles."""
    s, c = unpack_numpy(want)
    assert same(r.acc, want)
    assert same(r.sum, s) and same(r.count, c)
    for uncovered in (0.0, -1.0):
        assert same(r.mean(uncovered), mean_numpy(want, uncovered)[0])
    assert same(r.pred(), pred_numpy(want))


@pytest.mark.parametrize("d,P", list(itertools.product(DOWNSAMPLES, PATCHES)))
def test_raster_and_render_match_the_restatements(model, d, P):
    coords, values, shape, origin = case(d, P)
    want = raster_numpy(coords, values, P, d, shape, origin)
    r = model.tile_raster(torch.from_numpy(coords).to(DEV), torch.from_numpy(values).to(DEV), P, d, shape, origin)
    assert r.acc.device == torch.device(DEV) and r.tiles == len(coords) and r.shape == shape
    check_raster(r, want)
    g = np.random.default_rng(d + P)
    thumb = g.integers(0, 256, shape + (3,), dtype=np.uint8)
    for kw in (dict(), dict(alpha=0.75, colormap="gray", window=(0.2, 0.7), min_value=0.3), dict(alpha=1.0, window=(0.45, 0.55))):
        assert same(model.render_heatmap(r, thumb, **kw), render_numpy(want, thumb, **kw))


def test_host_and_device_numpy_and_torch_inputs(model):
    coords, values, shape, origin = case(16, 224, seed=3)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    forms = [(coords, values, lambda a: a), (coords, values, torch.from_numpy), (coords, values, dev),
             (coords.astype(np.int32), values.astype(np.float64), lambda a: a),      # coordinates beyond int32 wrap on the way in, on both sides;
             (coords.astype(np.int32), values.astype(np.float64), dev)]              # float64 values are rounded to float32 first, on both sides
    assert np.array_equal(raster_numpy(coords, values.astype(np.float64), 224, 16, shape, origin), raster_numpy(coords, values, 224, 16, shape, origin))
    for c, v, to in forms:
        assert same(model.tile_raster(to(c), to(v), 224, 16, shape, origin).acc, raster_numpy(c, v, 224, 16, shape, origin))
    assert same(model.tile_raster(dev(coords), values, 224, 16, shape, origin).acc, raster_numpy(coords, values, 224, 16, shape, origin))
    strided = torch.from_numpy(np.concatenate([coords, coords], axis=1)).to(DEV)[:, 1:3]        # a non-contiguous device view: (y, x) pairs
    assert same(model.tile_raster(strided, values, 224, 16, shape, origin).acc, raster_numpy(np.concatenate([coords, coords], axis=1)[:, 1:3], values, 224, 16, shape, origin))
    none = model.tile_raster(np.zeros((0, 2), np.int64), np.zeros(0, np.float32), 224, 16, shape, origin)
    assert none.tiles == 0 and int(none.acc.abs().sum()) == 0


@pytest.mark.parametrize("d,P", [(3, 224), (16, 256), (4, 512)])
def test_one_call_equals_three_and_two_runs_are_equal(model, d, P):
    coords, values, shape, origin = case(d, P, seed=1)
    c, v = torch.from_numpy(coords).to(DEV), torch.from_numpy(values).to(DEV)
    one = model.tile_raster(c, v, P, d, shape, origin)
    again = model.tile_raster(c, v, P, d, shape, origin)
    assert torch.equal(one.acc, again.acc)
    order = torch.from_numpy(np.random.default_rng(d).permutation(len(coords))).to(DEV)
    r = None
    for idx in order.tensor_split(3):
        r = model.tile_raster(c[idx], v[idx], P, d, shape, origin, into=r)
    assert r.tiles == len(coords) and torch.equal(r.acc, one.acc)
    check_raster(r, raster_numpy(coords, values, P, d, shape, origin))
    near = TileRaster(torch.zeros(shape, dtype=torch.int64, device=DEV), d, P, origin, tiles=MAX_TILES - 2, model=model)
    with pytest.raises(ValueError, match="2\\^24 - 1"):
        model.tile_raster(c[:3], v[:3], P, d, shape, origin, into=near)
    assert int(near.acc.abs().sum()) == 0 and near.tiles == MAX_TILES - 2    # refused before anything was added


@pytest.mark.parametrize("step,d", [(224, 16), (112, 4)])
def test_a_slide_of_100000_tiles(model, step, d):
    """A 317 x 316 lattice of P = 224 tiles (100 172 tiles): step 224 at d = 16 (every pixel under one tile), step 112 at d = 4 (four
    tiles per pixel, 314 M adds).  The restatement's per-tile slice loop takes seconds on the host."""
    P, nx, ny = 224, 317, 316
    g = np.random.default_rng(step)
    xs, ys = np.meshgrid(np.arange(nx) * step, np.arange(ny) * step)
    coords = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.int64)
    coords = coords[g.permutation(len(coords))]
    values = g.random(len(coords)).astype(np.float32)
    shape = (((ny - 1) * step + P) // d + 3, ((nx - 1) * step + P) // d + 2)
    r = model.tile_raster(coords, values, P, d, shape)
    want = raster_numpy(coords, values, P, d, shape)
    check_raster(r, want)
    assert int(unpack_numpy(want)[1].max()) == (P // step) ** 2
    if d == 16:
        assert same(model.render_heatmap(r, None, alpha=0.6), render_numpy(want, None, alpha=0.6))


def test_byte_offsets_beyond_4_gib(model):
    """A 16 500 x 32 768 raster: 540.7 M pixels > 2^29, a 4.33 GB accumulator (beside it the int32 count, 2.15 GB, while the total is
    taken) next to a depth-2 model.  Tiles in the last rows land at byte offsets above 2^32; those rows are compared with the
    restatement of a raster that starts there, and the total of the count says that nothing landed anywhere else."""
    h, w, d, P, rows = 16500, 32768, 16, 224, 64
    assert h * w > 1 << 29 and (h - rows) * w * 8 > 1 << 32
    g = np.random.default_rng(8)
    n = 200
    coords = np.stack([g.integers(-P, w * d, n), g.integers((h - rows + 1) * d, h * d + 20, n)], axis=1).astype(np.int64)
    values = g.random(n).astype(np.float32)
    r = model.tile_raster(coords, values, P, d, (h, w))
    want = raster_numpy(coords, values, P, d, (rows, w), origin=(0, (h - rows) * d))
    assert same(r.acc[h - rows:], want)
    total = int(unpack_numpy(want)[1].sum(dtype=np.int64))
    assert total > 0 and int(r.count.sum(dtype=torch.int64)) == total
    assert int(r.acc[:h - rows].abs().max()) == 0
    tail = TileRaster(r.acc[h - rows:], d, P, (0, (h - rows) * d), model=model)       # the same words, read through the other kernels
    assert same(tail.mean(), mean_numpy(want)[0])
    del r, tail
    torch.cuda.empty_cache()


def test_render_variants(model):
    rgb = synth_thumbnail()                                                      # 384 x 512
    h, w = rgb.shape[:2]
    d, P = 16, 224
    g = np.random.default_rng(12)
    coords = np.stack([g.integers(-P, w * d, 900), g.integers(-P, h * d, 900)], axis=1).astype(np.int64)
    values = g.random(900).astype(np.float32)
    r = model.tile_raster(coords, values, P, d, (h, w))
    want = raster_numpy(coords, values, P, d, (h, w))
    tissue = model.tissue_mask(rgb, d)
    assert 0 < float(tissue.mask.float().mean()) < 1
    mask = tissue.mask.cpu().numpy()
    big = np.zeros((h + 5, w + 9, 4), np.uint8)
    big[3:3 + h, 4:4 + w, :3] = rgb
    big[..., 3] = g.integers(0, 256, big.shape[:2])
    view_host, view_dev = big[3:3 + h, 4:4 + w], torch.from_numpy(big).to(DEV)[3:3 + h, 4:4 + w]
    own = np.ascontiguousarray(colormap("jet")[::-1])
    assert same(model.render_heatmap(r), render_numpy(want))
    assert same(model.render_heatmap(r, background=(10, 200, 30), alpha=0.9), render_numpy(want, background=(10, 200, 30), alpha=0.9))
    assert same(model.render_heatmap(r, rgb), render_numpy(want, rgb))
    assert same(model.render_heatmap(r, torch.from_numpy(rgb).to(DEV), tissue=tissue), render_numpy(want, rgb, mask=mask))
    for view in (view_host, view_dev):
        got = model.render_heatmap(r, view, tissue=tissue, alpha=0.5, window=(0.1, 0.8), min_value=0.25, colormap=own)
        assert same(got, render_numpy(want, view_host, 0.5, own, mask, (0.1, 0.8), 0.25))
    assert same(model.render_heatmap(r, view_dev, colormap=torch.from_numpy(own).to(DEV), alpha=1.0), render_numpy(want, rgb, 1.0, own))
    assert same(model.render_heatmap(r, rgb, alpha=0.0), rgb)
    own_mask = TissueMask(g.random((h, w)) < 0.5, d)
    assert same(model.render_heatmap(r, rgb, tissue=own_mask), render_numpy(want, rgb, mask=own_mask.mask.numpy()))
    for bad in (dict(thumbnail=rgb[:-1]), dict(tissue=TissueMask(mask, 8)), dict(tissue=TissueMask(mask[:, :-1], d))):
        with pytest.raises(ValueError):
            model.render_heatmap(r, **bad)
    # shapes that are not multiples of four pixels, and unaligned views, take the scalar path
    for hh, ww in ((7, 9), (1, 3), (5, 1)):
        small = model.tile_raster(coords % (ww * d), values, P, d, (hh, ww))
        ws = raster_numpy(coords % (ww * d), values, P, d, (hh, ww))
        check_raster(small, ws)
        t = g.integers(0, 256, (hh, ww, 3), dtype=np.uint8)
        assert same(model.render_heatmap(small, t, alpha=0.3), render_numpy(ws, t, alpha=0.3))


def test_end_to_end_at_depth_2(model):
    """encode_region(step = patch // 2) -> wsi.segment_heatmap equals raster_numpy fed with the device's own refine output, and
    segment_pred_mask gives the same mask from the dict of zero_shot_segment(mask_path=None) as from the (coords, p) pair."""
    P, d = 224, 16
    tiles = synth_tile_family("stain_field", 0, 12, torch.device(DEV), seed=3)                  # [12,224,224,3]
    region = tiles.reshape(3, 4, P, P, 3).permute(0, 2, 1, 3, 4).reshape(3 * P, 4 * P, 3).contiguous()
    origin = (2 * P, P)
    feats, coords = model.encode_region(region, P, P // 2, origin=origin)
    assert feats.shape[0] == 5 * 7
    shape = (region.shape[0] // d + 1, region.shape[1] // d + 2)
    gen = torch.Generator().manual_seed(1)
    classifier = torch.nn.functional.normalize(torch.randn(feats.shape[1], 2, generator=gen), dim=0).to(DEV)
    r = wsi.segment_heatmap(classifier, feats, coords, d, shape, patch_size=P, overlap=True, origin=(origin[0], origin[1]), model=model)
    rc, rmean, _ = wsi.refine(wsi._probs(model, classifier, feats), coords.cpu(), P, True, model=model)
    want = raster_numpy(rc.cpu().numpy(), rmean[:, 1].cpu().numpy(), P, d, shape, origin)
    assert r.tiles == feats.shape[0]
    check_raster(r, want)
    assert int(unpack_numpy(want)[1].max()) == 4
    r0 = wsi.segment_heatmap(classifier, feats, coords, d, shape, patch_size=P, cls=0, origin=origin, model=model)
    assert same(r0.acc, raster_numpy(rc.cpu().numpy(), rmean[:, 0].cpu().numpy(), P, d, shape, origin))
    picture = model.render_heatmap(r, None)
    assert same(picture, render_numpy(want))
    probs = wsi.zero_shot_segment(classifier, feats, coords.cpu(), None, patch_size=P, overlap=True, model=model)
    p = np.array(list(probs.values()), np.float32)
    thd = float(np.median(p))
    from_dict = wsi.segment_pred_mask(probs, thd, d, shape, patch_size=P, origin=origin, model=model)
    from_pair = wsi.segment_pred_mask((rc, rmean[:, 1]), thd, d, shape, patch_size=P, origin=origin, model=model)
    assert from_dict.dtype == torch.uint8 and torch.equal(from_dict, from_pair)
    painted = pred_numpy(raster_numpy(rc.cpu().numpy(), (rmean[:, 1].cpu().numpy() > np.float32(thd)).astype(np.float32), P, d, shape, origin))
    assert same(from_dict, painted) and 0 < (painted == 255).mean() < 1
    host_pair = wsi.segment_pred_mask((rc.cpu().numpy(), rmean[:, 1].cpu().numpy()), thd, d, shape, patch_size=P, origin=origin, model=model)
    assert torch.equal(host_pair, from_dict)


def test_abi_rejects_bad_arguments(model):
    lib, h, st = _lib.load(), model._handle, _stream(torch.device(DEV))
    H, W, N = 20, 24, 6
    acc = torch.zeros((H, W), dtype=torch.int64, device=DEV)
    coords = torch.zeros((N, 2), dtype=torch.int64, device=DEV)
    values = torch.full((N,), 0.5, dtype=torch.float32, device=DEV)
    mean = torch.zeros((H, W), dtype=torch.float32, device=DEV)
    count = torch.zeros((H, W), dtype=torch.int32, device=DEV)
    pred = torch.zeros((H, W), dtype=torch.uint8, device=DEV)
    thumb = torch.zeros((H, W, 4), dtype=torch.uint8, device=DEV)
    mask = torch.ones((H, W), dtype=torch.uint8, device=DEV)
    lut = torch.from_numpy(colormap("jet")).to(DEV)
    out = torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV)
    null = C.c_void_p(0)

    def off(t, nbytes):
        return C.c_void_p(t.data_ptr() + nbytes)

    def accumulate(c=_ptr(coords), v=_ptr(values), n=N, P=224, d=16, Hh=H, Ww=W, ox=0, oy=0, zero=1, a=_ptr(acc)):
        return lib.keep_heat_accumulate(h, c, v, n, P, d, Hh, Ww, ox, oy, zero, a, st)

    assert accumulate() == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert int(acc[0, 0]) == (N << 40) | (N * 32768) and int(acc[-1, -1]) == 0
    for kw in [dict(c=null), dict(v=null), dict(a=null), dict(a=off(acc, 4)), dict(n=-1), dict(n=1 << 24), dict(P=0), dict(P=(1 << 30) + 1), dict(d=0),
               dict(d=-16), dict(d=225), dict(Hh=0), dict(Ww=0), dict(Hh=-3), dict(Hh=1 << 16, Ww=(1 << 14) + 1), dict(ox=8), dict(oy=-8),
               dict(ox=1 << 44), dict(oy=-(1 << 44))]:
        assert accumulate(**kw) == _lib.KEEP_EINVAL, kw
        assert lib.keep_last_error(h)
    assert accumulate(n=0, c=null, v=null, zero=0) == _lib.KEEP_OK                # nothing to add is no error
    assert accumulate(ox=-(1 << 40), oy=1 << 40, zero=0) == _lib.KEEP_OK          # the largest origin: every tile is off the raster
    assert accumulate(ox=32, oy=16, zero=0) == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert int(acc[0, 0]) == ((2 * N) << 40) | (2 * N * 32768)                    # the origin moved one tile over pixel (0, 0) again

    def read(a=_ptr(acc), Hh=H, Ww=W, m=_ptr(mean), c=_ptr(count), p=_ptr(pred)):
        return lib.keep_heat_mean(h, a, Hh, Ww, 0.0, m, c, p, st)

    assert read() == _lib.KEEP_OK and read(m=null, c=null) == _lib.KEEP_OK
    for kw in [dict(a=null), dict(a=off(acc, 4)), dict(Hh=0), dict(Ww=-1), dict(Hh=1 << 16, Ww=(1 << 14) + 1), dict(m=null, c=null, p=null),
               dict(m=off(mean, 2)), dict(c=off(count, 1))]:
        assert read(**kw) == _lib.KEEP_EINVAL, kw
        assert lib.keep_last_error(h)
    # pointers aligned to their element but not to 16 bytes: served by the scalar path, same numbers
    flat = torch.zeros(H * W + 1, dtype=torch.float32, device=DEV)
    assert read(m=off(flat, 4), c=null, p=off(pred, 0)) == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert torch.equal(flat[1:].reshape(H, W), mean)

    def render(a=_ptr(acc), Hh=H, Ww=W, t=_ptr(thumb), row=W * 4, ps=4, bg=0xFFFFFF, m=_ptr(mask), l=_ptr(lut), alpha=100, lo=0, hi=65535, mn=0,
               o=_ptr(out)):
        return lib.keep_heat_render(h, a, Hh, Ww, t, row, ps, bg, m, l, alpha, lo, hi, mn, o, st)

    assert render() == _lib.KEEP_OK and render(t=null, m=null) == _lib.KEEP_OK
    for kw in [dict(a=null), dict(a=off(acc, 4)), dict(l=null), dict(o=null), dict(Hh=0), dict(Ww=0), dict(Hh=1 << 16, Ww=(1 << 14) + 1), dict(ps=2),
               dict(ps=5), dict(row=W * 4 - 1), dict(ps=3, row=W * 3 - 1), dict(t=null, bg=-1), dict(t=null, bg=1 << 24), dict(alpha=-1),
               dict(alpha=257), dict(lo=-1), dict(hi=65536), dict(lo=100, hi=100), dict(lo=200, hi=100), dict(mn=-1), dict(mn=65536)]:
        assert render(**kw) == _lib.KEEP_EINVAL, kw
        assert lib.keep_last_error(h)
    for call in (lambda: lib.keep_heat_accumulate(None, _ptr(coords), _ptr(values), N, 224, 16, H, W, 0, 0, 1, _ptr(acc), st),
                 lambda: lib.keep_heat_mean(None, _ptr(acc), H, W, 0.0, _ptr(mean), _ptr(count), _ptr(pred), st),
                 lambda: lib.keep_heat_render(None, _ptr(acc), H, W, null, 0, 3, 0, null, _ptr(lut), 100, 0, 65535, 0, _ptr(out), st)):
        assert call() == _lib.KEEP_EINVAL
    with pytest.raises(ValueError, match="downsample"):
        _lib.check(h, accumulate(d=0), "heat_accumulate")
    torch.cuda.synchronize()
