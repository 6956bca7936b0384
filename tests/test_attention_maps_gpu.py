"""CLS attention maps on the MI355X: Ops.attention_cls_probs, KEEPModel.encode_image_attention /
encode_region_attention (keep_encode_image_attn), KEEPModel.cell_raster (keep_heat_accumulate_cells) and wsi.attention_heatmap.

Yardsticks, all in tests/attention_reference.py: a float64 softmax on the operands the kernel reads (operator), a float64 restatement
of the tower up to the tapped block (tower; the bar is a multiple of E16, the error of the oracle's own fp16-operand model against
that restatement on the test's tiles), and keep_amd.heatmap.cell_raster_numpy, which tests/test_attention_maps.py holds to a
triple loop (cell raster: integer-exact)."""
import math

import numpy as np
import pytest
import torch

import attention_reference as AR
from keep_amd import KEEPModel, wsi
from keep_amd.attention import cls_attention_map
from keep_amd.config import small_shape
from keep_amd.heatmap import MAX_TILES, TileRaster, cell_raster_numpy
from keep_amd.synth import normalise_u8, synth_state_dict, towers_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = {"strict": 0.05, "comp": 3.0, "fp16": 3.0}           # multiples of E16
CASES = AR.raster_cases()


# ------------------------------------------------------------------------------------------------ the operator
OP_SHAPES = [(3, 197, 16), (2, 1, 1), (1, 17, 1), (2, 64, 2), (1, 65, 1), (1, 257, 2), (1, 577, 2), (1, 1025, 1),
             (1, 256, 1)]                                   # (the last: the largest sequence of the register path, beside 257 above)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("B,T,heads", OP_SHAPES)
def test_attention_cls_probs(ops, B, T, heads, split):
    qkv = AR.rand(B * T, 3 * heads * 64, seed=T * 31 + heads, std=1.5)
    ref, A = AR.cls_probs_reference(qkv, B, T, heads, split)
    got = ops.attention_cls_probs(qkv, B, T, heads, split)
    assert got.shape == (B, heads, T) and got.dtype == torch.float32
    got = got.cpu().double()
    # fp32 accumulation of 64 products moves a score by at most 0.125 A 66 2^-24 (first order; two more roundings for the scale
    # and the subtraction of the maximum); a softmax then moves by at most expm1(2 delta) relative; 2^-20 for exp2 and the scaling
    delta = 0.125 * A * 66 * 2.0 ** -24
    bound = ref * (torch.expm1(2 * delta)[:, :, None] + 2.0 ** -20)
    err = (got - ref).abs()
    print(f"[cls_probs B={B} T={T} heads={heads} split={split}] max rel err {(err / ref).max():.3e}, bound "
          f"{(bound / ref).max():.3e}, worst err / bound {(err / bound).max():.3f}")
    assert not torch.isnan(got).any() and (got >= 0).all()
    assert (got.sum(-1) - 1).abs().max() <= 1e-5
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------ the tower
def make_model(sd, precision, dynamic=False, **opts):
    m = KEEPModel(precision=precision, towers=towers_of(sd), dynamic_img_size=dynamic)
    for k, v in opts.items():
        m.set_option(k, v)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def small():
    return {k: v for k, v in synth_state_dict(small_shape(2, 2), seed=5).items() if k.startswith("visual")}


@pytest.fixture(scope="module")
def models(small):
    return {p: make_model(small, p) for p in ("strict", "comp", "fp16")}


@pytest.fixture(scope="module")
def dyn(small):
    return make_model(small, "strict", dynamic=True)


def tiles(n, H, W, seed):
    return AR.rand(n, 3, H, W, seed=seed)


def yardstick(sd, x, block):
    """-> (float64 restatement [B, heads, T], E16): E16 is the oracle's fp16-operand model in fp32 against it, on these tiles."""
    with torch.no_grad():
        ref = AR.tower_cls_attention(sd, x, block)
        e16 = AR.max_rel(AR.tower_cls_attention(sd, x, block, dtype=torch.float32, operand_dtype=torch.float16), ref)
    return ref, e16


@pytest.fixture(scope="module")
def ref224(small):
    x = tiles(3, 224, 224, seed=11)
    return x, {b: yardstick(small, x, b) for b in (0, 1)}


@pytest.mark.parametrize("precision", ["strict", "comp", "fp16"])
def test_tower_224_every_block_and_mode(models, ref224, precision):
    m = models[precision]
    x, refs = ref224
    for block in (0, 1, -1):
        ref, e16 = refs[block % 2]
        feats, attn = m.encode_image_attention(x, block=block)
        assert feats.shape == (3, 768) and attn.shape == (3, 16, 197) and attn.dtype == torch.float32 and attn.device.type == "cpu"
        err = AR.max_rel(attn, ref)
        print(f"[tower 224 {precision} block {block}] max rel err {err:.3e}, E16 {e16:.3e}, ratio {err / e16:.3f} (bar {BAR[precision]})")
        assert (attn.sum(-1) - 1).abs().max() <= 1e-5
        assert err <= BAR[precision] * e16, (precision, block)
    assert torch.equal(m.encode_image_attention(x, block=-1)[1], m.encode_image_attention(x, block=1)[1])


@pytest.fixture(scope="module")
def ref33(small):
    x = tiles(33, 224, 224, seed=12)
    return x, yardstick(small, x, 0)


@pytest.mark.parametrize("max_tiles", [None, 8], ids=["two_lanes_17_16", "rounds_of_8_ragged"])
def test_tower_33_tiles_every_lane_and_round(small, models, ref33, max_tiles):
    """B = 33: two lanes of 17 + 16 by default; with max_tiles = 8, rounds of two lanes of 8 and a last round of one tile.  Every
    tile's rows are held to the bar: a wrong lane or round offset puts another tile's map (or none) there."""
    m = models["comp"] if max_tiles is None else make_model(small, "comp", max_tiles=max_tiles)
    x, (ref, e16) = ref33
    feats, attn = m.encode_image_attention(x, block=0)
    per_tile = ((attn.double() - ref).abs() / ref).amax(dim=(1, 2))
    print(f"[tower 33 tiles, max_tiles {max_tiles}] per-tile max rel err: worst {per_tile.max():.3e} (tile {per_tile.argmax()}), "
          f"E16 {e16:.3e}, ratio {per_tile.max() / e16:.3f}")
    assert (per_tile <= BAR["comp"] * e16).all(), per_tile
    m.set_option("graphs", 0)
    plain = m.encode_image(x)
    m.set_option("graphs", 1)
    assert torch.equal(feats, plain)


@pytest.mark.parametrize("H,W,B", [(16, 16, 3), (48, 80, 3), (256, 256, 3), (384, 384, 2)])
def test_tower_dynamic_sizes_strict(small, dyn, H, W, B):
    x = tiles(B, H, W, seed=H + W)
    T = (H // 16) * (W // 16) + 1
    for block in (0, -1):
        ref, e16 = yardstick(AR.sd_at(small, H, W), x, block)
        feats, attn = dyn.encode_image_attention(x, block=block)
        assert attn.shape == (B, 16, T)
        err = AR.max_rel(attn, ref)
        print(f"[tower {H}x{W} T={T} strict block {block}] max rel err {err:.3e}, E16 {e16:.3e}, ratio {err / e16:.4f} (bar {BAR['strict']})")
        assert (attn.sum(-1) - 1).abs().max() <= 1e-5
        assert err <= BAR["strict"] * e16, (H, W, block)
    dyn.set_option("graphs", 0)
    plain = dyn.encode_image(x)
    dyn.set_option("graphs", 1)
    assert torch.equal(feats, plain)


def test_tapped_features_are_exact_and_leave_no_state(models):
    m = models["comp"]
    x = tiles(3, 224, 224, seed=21).to(DEV)
    before = m.encode_image(x)                                # graphs on: captured here, replayed below
    feats, attn = m.encode_image_attention(x)
    assert feats.device == x.device and attn.device == x.device
    after = m.encode_image(x)
    assert torch.equal(before, after)
    m.set_option("graphs", 0)
    plain = m.encode_image(x)
    m.set_option("graphs", 1)
    assert torch.equal(feats, plain)
    assert torch.equal(m.encode_image(x), before)
    # bf16 / fp16 pixels and an empty batch take the same path as encode_image
    xb = x.to(torch.bfloat16)
    fb, ab = m.encode_image_attention(xb, block=0)
    m.set_option("graphs", 0)
    assert torch.equal(fb, m.encode_image(xb))
    m.set_option("graphs", 1)
    f0, a0 = m.encode_image_attention(x[:0])
    assert f0.shape == (0, 768) and a0.shape == (0, 16, 197)


def test_tower_errors(models, dyn):
    m = models["comp"]
    x = tiles(1, 224, 224, seed=1)
    for bad in (2, -3, 100):
        with pytest.raises(ValueError, match="block"):
            m.encode_image_attention(x, block=bad)
        with pytest.raises(ValueError, match="block"):
            m.encode_image_attention(x[:0], block=bad)
    for bad in (1.0, True, None):
        with pytest.raises(ValueError, match="block"):
            m.encode_image_attention(x, block=bad)
    for shape in ((1, 3, 256, 256), (1, 3, 16, 16)):
        with pytest.raises(ValueError, match="224x224"):
            m.encode_image_attention(torch.zeros(shape))       # a 224-only model rejects other sizes, as encode_image does
    with pytest.raises(ValueError, match="multiples of 16"):
        dyn.encode_image_attention(torch.zeros(1, 3, 200, 224))
    with pytest.raises(ValueError, match=r"\[B,3,H,W\]"):
        m.encode_image_attention(torch.zeros(1, 224, 224, 3))
    # the C ABI checks the block itself
    from keep_amd import _lib
    from keep_amd.model import _ptr, _stream
    lib = _lib.load()
    xd = x.to(DEV)
    out, attn = torch.empty(1, 768, device=DEV), torch.empty(1, 16, 197, device=DEV)
    st = _stream(xd.device)
    for block in (2, -3):
        assert lib.keep_encode_image_attn(m._handle, _ptr(xd), _lib.PIX_F32, 1, 224, 224, block, _ptr(out), _ptr(attn), st) == _lib.KEEP_EINVAL
    assert lib.keep_encode_image_attn(m._handle, _ptr(xd), _lib.PIX_F32, 1, 224, 224, 0, _ptr(out), None, st) == _lib.KEEP_EINVAL
    assert lib.keep_encode_image_attn(m._handle, _ptr(xd), _lib.PIX_F32, 1, 224, 200, 0, _ptr(out), _ptr(attn), st) == _lib.KEEP_EINVAL
    assert lib.keep_encode_image_attn(m._handle, _ptr(xd), _lib.PIX_F32, 1, 224, 224, -1, _ptr(out), _ptr(attn), st) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ regions
@pytest.fixture(scope="module")
def region():
    g = torch.Generator().manual_seed(77)
    return torch.randint(0, 256, (448, 672, 3), dtype=torch.uint8, generator=g)


@pytest.fixture(scope="module")
def region_attention(models, region):
    return models["comp"].encode_region_attention(region.to(DEV), 224, batch=4)      # two batches: 4 + 2 tiles


def test_encode_region_attention(small, models, region, region_attention):
    m = models["comp"]
    rd = region.to(DEV)
    feats, coords, attn = region_attention
    assert feats.shape == (6, 768) and coords.shape == (6, 2) and attn.shape == (6, 16, 197) and attn.device == rd.device
    m.set_option("graphs", 0)
    f_ref, c_ref = m.encode_region(rd, 224, batch=4)
    m.set_option("graphs", 1)
    assert torch.equal(coords, c_ref) and torch.equal(feats, f_ref)
    cut = normalise_u8(m.region_patches_uint8(rd, coords, 224)).cpu()
    ref, e16 = yardstick(small, cut, -1)
    err = AR.max_rel(attn.cpu(), ref)
    print(f"[region 448x672 comp block -1] max rel err {err:.3e}, E16 {e16:.3e}, ratio {err / e16:.3f} (bar {BAR['comp']})")
    assert err <= BAR["comp"] * e16
    with pytest.raises(ValueError, match="block"):
        m.encode_region_attention(rd, 224, block=2)
    f_host, c_host, a_host = m.encode_region_attention(region, 224, batch=4, block=1)      # a host region: results on the host
    assert a_host.device.type == "cpu" and torch.equal(c_host, coords.cpu()) and torch.equal(a_host, attn.cpu())
    empty = m.encode_region_attention(rd[:100], 224)
    assert empty[0].shape == (0, 768) and empty[1].shape == (0, 2) and empty[2].shape == (0, 16, 197)


# ------------------------------------------------------------------------------------------------ the cell raster
def dev(a):
    return torch.from_numpy(a).to(DEV)


def same(t: torch.Tensor, a: np.ndarray) -> bool:
    return t.dtype == torch.from_numpy(a).dtype and torch.equal(t.cpu(), torch.from_numpy(a))


@pytest.mark.parametrize("name", sorted(CASES))
def test_cell_raster_equals_the_restatement(models, name):
    m = models["strict"]
    coords, values, grid, patch, d, shape, origin = CASES[name]
    want = cell_raster_numpy(coords, values, grid, patch, d, shape, origin)
    r = m.cell_raster(dev(coords), dev(values), grid, patch, d, shape, origin)
    assert isinstance(r, TileRaster) and r.tiles == len(coords) and r.shape == shape and r.patch == patch and r.downsample == d
    assert same(r.acc, want)
    assert same(m.cell_raster(coords, values.astype(np.float64), grid, patch, d, shape, origin).acc, want)      # host numpy in, fp64 values
    # one call equals three with into=
    n = len(coords)
    cuts = (0, n // 3, n // 3 + 1, n)
    part = None
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        part = m.cell_raster(dev(coords[lo:hi]), dev(values[lo:hi]), grid, patch, d, shape, origin, into=part)
    assert part.tiles == n and same(part.acc, want)
    # tiles constant over their cells: tile_raster's raster
    per_tile = values[:, 0].copy()
    per_tile[::5] = np.nan
    const = np.repeat(per_tile[:, None], grid[0] * grid[1], axis=1)
    assert torch.equal(m.cell_raster(dev(coords), dev(const), grid, patch, d, shape, origin).acc,
                       m.tile_raster(dev(coords), dev(per_tile), patch, d, shape, origin).acc)


def test_cell_raster_feeds_the_raster_consumers_and_keeps_the_cap(models):
    m = models["strict"]
    coords, values, grid, patch, d, shape, origin = CASES["overlap_step112"]
    r = m.cell_raster(dev(coords), dev(values), grid, patch, d, shape, origin)
    mean = r.mean()
    assert mean.shape == shape and mean.dtype == torch.float32 and 0 < float(mean.max()) <= 1
    assert int(r.count.max()) == 4
    rgb = m.render_heatmap(r)
    assert rgb.shape == shape + (3,) and rgb.dtype == torch.uint8
    assert m.smooth_raster(r, sigma=1.0).shape == shape
    assert len(m.mask_regions(mean > 0.5, raster=r)) >= 1
    full = TileRaster(torch.zeros(shape, dtype=torch.int64, device=DEV), d, patch, origin, MAX_TILES - len(coords) + 1, m)
    with pytest.raises(ValueError, match="at most 2\\^24 - 1"):
        m.cell_raster(dev(coords), dev(values), grid, patch, d, shape, origin, into=full)
    assert full.tiles == MAX_TILES - len(coords) + 1 and not full.acc.any()      # refused by claim, before any device work
    with pytest.raises(ValueError, match="into= raster has patch"):
        m.cell_raster(dev(coords), dev(values), grid, patch, 8, shape, origin, into=r)
    with pytest.raises(ValueError, match="cell side"):
        m.cell_raster(dev(coords), dev(values), grid, patch, 17, shape, origin)


# ------------------------------------------------------------------------------------------------ end to end
def test_attention_heatmap_chains_the_map_and_the_cell_raster(models, region_attention):
    m = models["comp"]
    _, coords, attn = region_attention
    for kw in (dict(), dict(heads=3, normalize="sum"), dict(heads=[0, 5], normalize="none")):
        got = wsi.attention_heatmap(m, attn, coords, (14, 14), 224, 16, (28, 42), **kw)
        want = m.cell_raster(coords, cls_attention_map(attn, **kw), (14, 14), 224, 16, (28, 42))
        assert isinstance(got, TileRaster) and got.tiles == 6 and torch.equal(got.acc, want.acc)
    full = wsi.attention_heatmap(m, attn, coords, (14, 14), 224, 16, (28, 42))
    assert int(full.count.min()) == 1 and float(full.mean().max()) == 1.0        # six tiles side by side; every tile's strongest patch is 1
    host = cell_raster_numpy(coords.cpu().numpy(), cls_attention_map(attn).cpu().numpy(), (14, 14), 224, 16, (28, 42))
    assert same(full.acc, host)
    two = wsi.attention_heatmap(m, attn[:2], coords[:2], (14, 14), 224, 16, (28, 42))
    two = wsi.attention_heatmap(m, attn[2:], coords[2:], (14, 14), 224, 16, (28, 42), into=two)
    assert torch.equal(two.acc, full.acc)
