"""Attention rollout on the MI355X: Ops.attention_rollout_step (keep_op_attention_rollout_step),
KEEPModel.encode_image_rollout / encode_region_rollout (keep_encode_image_rollout) and the chain into the CLS-map consumers.

Yardsticks, all in tests/rollout_reference.py (held to brute force by tests/test_attention_rollout.py): one step in float64 on the
operands the kernel reads (operator; a derived bound), and the float64 restatement of the tower with every block's head-mean matrix
kept (tower; the bar is the project's multiple of E16, the error of the fp32 model with fp16-rounded operands against that restatement
on the test's own tiles)."""
import math

import pytest
import torch

import attention_reference as AR
import rollout_reference as RR
from keep_amd import KEEPModel, _lib, wsi
from keep_amd.attention import ROLLOUT_MAX_TOKENS, cls_attention_map
from keep_amd.config import small_shape
from keep_amd.heatmap import TileRaster
from keep_amd.synth import normalise_u8, synth_state_dict, towers_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = {"strict": 0.05, "comp": 3.0, "fp16": 3.0}           # multiples of E16: the bars of tests/test_attention_maps_gpu.py
DEPTH = 3                                                   # block 0: the step without a product, block 1: the full T x T product, block 2: the CLS row's


# ------------------------------------------------------------------------------------------------ the operator
# the edge of a 16-key tile, of a 64-row band, the 13 tiles of a 224 x 224 tile, both sides of 256
OP_SHAPES = [(2, 1, 1), (1, 2, 1), (1, 17, 1), (2, 64, 2), (1, 65, 2), (3, 197, 16), (1, 256, 1), (1, 257, 2)]
OP_CASES = {"first_all_rows": (False, 0), "product_all_rows": (True, 0), "product_cls_row": (True, 1)}


def stochastic(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(torch.randn(B, T, T, generator=g, dtype=torch.float32), dim=-1)


def step_bound(ref, A, T, split, product=True):
    """fp32 accumulation of n products (and the three of a split block) moves a score by at most 0.125 A (n + 4) 2^-24, a softmax then by
    expm1(2 delta) relative; 2^-20 for exp2 and the scaling; (T + 8) 2^-24 for the fp32 accumulation of the product and the blend.  All
    terms are non-negative, so relative perturbations of the terms carry to the sums."""
    delta = 0.125 * A * ((192 if split else 64) + 4) * 2.0 ** -24
    return ref * (torch.expm1(2 * delta)[:, None, None] + 2.0 ** -20 + ((T if product else 0) + 8) * 2.0 ** -24)


@pytest.mark.parametrize("case", sorted(OP_CASES))
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("B,T,heads", OP_SHAPES)
def test_attention_rollout_step(ops, B, T, heads, split, case):
    with_r, q_rows = OP_CASES[case]
    qkv = AR.rand(B * T, 3 * heads * 64, seed=T * 31 + heads, std=1.5)
    r_in = stochastic(B, T, seed=T + 7 * heads) if with_r else None
    ref, A = RR.rollout_step_reference(qkv, B, T, heads, split, 0.5, r_in, q_rows)
    got = ops.attention_rollout_step(qkv, B, T, heads, split=split, residual=0.5, r_in=r_in, q_rows=q_rows)
    assert got.shape == (B, 1 if q_rows else T, T) and got.dtype == torch.float32
    got = got.cpu().double()
    bound = step_bound(ref, A, T, split)
    err = (got - ref).abs()
    print(f"[rollout step B={B} T={T} heads={heads} split={split} {case}] max rel err {(err / ref).max():.3e}, bound "
          f"{(bound / ref).max():.3e}, worst err / bound {(err / bound).max():.3f}")
    assert not torch.isnan(got).any() and (got >= 0).all()
    assert (got.sum(-1) - 1).abs().max() <= 1e-5
    assert (err <= bound).all()


def test_attention_rollout_step_limits(ops):
    T = ROLLOUT_MAX_TOKENS
    qkv = AR.rand(T, 3 * 64, seed=5, std=1.5)
    ref, A = RR.rollout_step_reference(qkv, 1, T, 1, True, 0.25, None, 0)
    got = ops.attention_rollout_step(qkv, 1, T, 1, split=True, residual=0.25).cpu().double()
    assert ((got - ref).abs() <= step_bound(ref, A, T, True)).all()
    big = AR.rand(T + 1, 3 * 64, seed=5)
    with pytest.raises(ValueError, match="at most"):
        ops.attention_rollout_step(big, 1, T + 1, 1)
    for kw in (dict(q_rows=2), dict(q_rows=-1), dict(residual=1.0), dict(residual=-0.1), dict(residual=float("nan"))):
        with pytest.raises(ValueError):
            ops.attention_rollout_step(qkv, 1, T, 1, **kw)
    with pytest.raises(ValueError, match="r_in"):
        ops.attention_rollout_step(qkv, 1, T, 1, r_in=torch.zeros(1, T, T - 1))


# ------------------------------------------------------------------------------------------------ the tower
def make_model(sd, precision, dynamic=False, **opts):
    m = KEEPModel(precision=precision, towers=towers_of(sd), dynamic_img_size=dynamic)
    for k, v in opts.items():
        m.set_option(k, v)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def small():
    return {k: v for k, v in synth_state_dict(small_shape(DEPTH, 2), seed=5).items() if k.startswith("visual")}


@pytest.fixture(scope="module")
def models(small):
    return {p: make_model(small, p) for p in ("strict", "comp", "fp16")}


@pytest.fixture(scope="module")
def dyn(small):
    return make_model(small, "strict", dynamic=True)


def tiles(n, H, W, seed):
    return AR.rand(n, 3, H, W, seed=seed)


class Yardstick:
    """The float64 restatement's matrices of some tiles and the fp16-operand model's, computed once; ref(start, residual) -> (rollout
    float64 [B, T], E16)."""

    def __init__(self, sd, x):
        with torch.no_grad():
            self.mats, self.qkv = RR.tower_attention_mats(sd, x, keep_qkv=True)
            self.mats16 = RR.tower_attention_mats(sd, x, dtype=torch.float32, operand_dtype=torch.float16)

    def ref(self, start, residual):
        want = RR.rollout(self.mats, start, residual)
        return want, AR.max_rel(RR.rollout(self.mats16, start, residual), want)


@pytest.fixture(scope="module")
def ref224(small):
    x = tiles(3, 224, 224, seed=11)
    return x, Yardstick(small, x)


@pytest.mark.parametrize("precision", ["strict", "comp", "fp16"])
def test_tower_224_every_start_and_mode(models, ref224, precision):
    m = models[precision]
    x, y = ref224
    for start, residual in [(0, 0.5), (1, 0.5), (-1, 0.5)] + ([(0, 0.9)] if precision == "comp" else []):
        ref, e16 = y.ref(start, residual)
        feats, roll = m.encode_image_rollout(x, start_block=start, residual=residual)
        assert feats.shape == (3, 768) and roll.shape == (3, 1, 197) and roll.dtype == torch.float32 and roll.device.type == "cpu"
        err = AR.max_rel(roll[:, 0], ref)
        print(f"[rollout 224 {precision} start {start} residual {residual}] max rel err {err:.3e}, E16 {e16:.3e}, ratio {err / e16:.4f} "
              f"(bar {BAR[precision]})")
        assert (roll.sum(-1) - 1).abs().max() <= 1e-5 and (roll > 0).all()
        assert err <= BAR[precision] * e16, (precision, start, residual)
    assert torch.equal(m.encode_image_rollout(x, start_block=-1)[1], m.encode_image_rollout(x, start_block=DEPTH - 1)[1])
    assert torch.equal(m.encode_image_rollout(x)[1], m.encode_image_rollout(x, 0, 0.5)[1])      # the defaults


def test_last_block_without_residual_is_the_head_mean_of_the_tap(models, ref224):
    """Both are fp32 softmaxes of the same planes (hi + lo: strict), the 64 products accumulated in another order: the operator's bound,
    r_in = I, no product term; A from the float64 restatement's q / k of the last block."""
    m = models["strict"]
    x, y = ref224
    roll = m.encode_image_rollout(x, start_block=-1, residual=0.0)[1][:, 0].double()
    tap = m.encode_image_attention(x, block=-1)[1].double().mean(1)
    ref, A = RR.rollout_step_reference(y.qkv[-1].reshape(3 * 197, -1).float(), 3, 197, 16, True, 0.0, None, 1)
    bound = step_bound(ref, A, 197, True, product=False)[:, 0]
    d = (roll - tap).abs()
    print(f"[rollout start -1 residual 0 against the tap's head mean, strict] max rel diff {(d / ref[:, 0]).max():.3e}, worst diff / bound "
          f"{(d / bound).max():.4f}")
    assert (d <= bound).all()


@pytest.fixture(scope="module")
def ref33(small):
    x = tiles(33, 224, 224, seed=12)
    return x, Yardstick(small, x).ref(0, 0.5)


@pytest.mark.parametrize("max_tiles", [None, 8], ids=["two_lanes_17_16", "rounds_of_8_ragged"])
def test_tower_33_tiles_every_lane_and_round(small, models, ref33, max_tiles):
    """B = 33: two lanes of 17 + 16 by default; with max_tiles = 8, rounds of two lanes of 8 and a last round of one tile.  Every tile
    is held to the bar on its own: a wrong lane or round offset of the ping-pong buffers or the output slice shows as one bad tile."""
    m = models["comp"] if max_tiles is None else make_model(small, "comp", max_tiles=max_tiles)
    x, (ref, e16) = ref33
    feats, roll = m.encode_image_rollout(x, start_block=0)
    assert roll.shape == (33, 1, 197)
    per_tile = ((roll[:, 0].double() - ref).abs() / ref).amax(dim=1)
    print(f"[rollout 33 tiles, max_tiles {max_tiles}] per-tile max rel err: worst {per_tile.max():.3e} (tile {per_tile.argmax()}), "
          f"E16 {e16:.3e}, ratio {per_tile.max() / e16:.3f}")
    assert (per_tile <= BAR["comp"] * e16).all(), per_tile
    m.set_option("graphs", 0)
    plain = m.encode_image(x)
    m.set_option("graphs", 1)
    assert torch.equal(feats, plain)


@pytest.mark.parametrize("H,W,B", [(16, 16, 3), (48, 80, 3), (256, 256, 2)])
def test_tower_dynamic_sizes_strict(small, dyn, H, W, B):
    x = tiles(B, H, W, seed=H + W)
    T = (H // 16) * (W // 16) + 1
    ref, e16 = Yardstick(AR.sd_at(small, H, W), x).ref(0, 0.5)
    feats, roll = dyn.encode_image_rollout(x)
    assert roll.shape == (B, 1, T)
    err = AR.max_rel(roll[:, 0], ref)
    print(f"[rollout {H}x{W} T={T} strict] max rel err {err:.3e}, E16 {e16:.3e}, ratio {err / e16:.4f} (bar {BAR['strict']})")
    assert (roll.sum(-1) - 1).abs().max() <= 1e-5
    assert err <= BAR["strict"] * e16, (H, W)
    dyn.set_option("graphs", 0)
    plain = dyn.encode_image(x)
    dyn.set_option("graphs", 1)
    assert torch.equal(feats, plain)


def test_too_many_tokens_is_refused_before_any_device_work(dyn):
    H, W = 272, 256                                           # 17 x 16 + 1 = 273 tokens
    assert (H // 16) * (W // 16) + 1 == ROLLOUT_MAX_TOKENS + 1
    with pytest.raises(ValueError, match="at most"):
        dyn.encode_image_rollout(torch.zeros(1, 3, H, W))
    with pytest.raises(ValueError, match="at most"):
        dyn.encode_image_rollout(torch.zeros(0, 3, H, W))
    from keep_amd.model import _ptr, _stream
    import ctypes
    lib = _lib.load()
    xd = torch.zeros(1, 3, H, W, device=DEV)
    out, roll, need = torch.empty(1, 768, device=DEV), torch.empty(1, 1, 273, device=DEV), ctypes.c_int64(-1)
    assert lib.keep_rollout_scratch_bytes(dyn._handle, 1, H, W, ctypes.byref(need)) == _lib.KEEP_EUNSUPPORTED
    scratch = torch.empty(1024, dtype=torch.uint8, device=DEV)
    assert lib.keep_encode_image_rollout(dyn._handle, _ptr(xd), _lib.PIX_F32, 1, H, W, 0, 0.5, _ptr(out), _ptr(roll), _ptr(scratch), scratch.numel(),
                                         _stream(xd.device)) == _lib.KEEP_EUNSUPPORTED
    feats, ok = dyn.encode_image_rollout(torch.zeros(1, 3, 256, 256))      # 257 tokens: served
    assert ok.shape == (1, 1, 257)


STATE_OPTIONS = ("graphs", "precision", "max_tiles", "streams", "cls_tail", "strict_blocks", "patch_split", "grid_plan", "attn_waves",
                 "gemm_impl", "plan_custom", "bias_ready")


def test_rollout_features_are_exact_and_leave_no_state(models):
    m = models["comp"]
    lib = _lib.load()
    x = tiles(3, 224, 224, seed=21).to(DEV)
    before = m.encode_image(x)                                # graphs on: captured here, replayed below
    state = ({k: m.get_option(k) for k in STATE_OPTIONS}, int(lib.keep_workspace_bytes(m._handle)), m.get_option("graph_count"))
    assert state[2] >= 1
    feats, roll = m.encode_image_rollout(x)
    assert feats.device == x.device and roll.device == x.device
    assert ({k: m.get_option(k) for k in STATE_OPTIONS}, int(lib.keep_workspace_bytes(m._handle)), m.get_option("graph_count")) == state
    after = m.encode_image(x)
    assert torch.equal(before, after)
    m.set_option("graphs", 0)
    plain = m.encode_image(x)
    m.set_option("graphs", 1)
    assert torch.equal(feats, plain)
    assert torch.equal(m.encode_image(x), before)
    # cls_tail off: the last block's step still writes the CLS row alone, and the same one
    m.set_option("cls_tail", 0)
    f2, r2 = m.encode_image_rollout(x)
    m.set_option("graphs", 0)
    p2 = m.encode_image(x)
    m.set_option("graphs", 1)
    m.set_option("cls_tail", 1)
    assert torch.equal(f2, p2) and torch.equal(r2, roll)
    # bf16 pixels and an empty batch take the same path as encode_image
    xb = x.to(torch.bfloat16)
    fb, rb = m.encode_image_rollout(xb, start_block=1)
    m.set_option("graphs", 0)
    assert torch.equal(fb, m.encode_image(xb))
    m.set_option("graphs", 1)
    f0, r0 = m.encode_image_rollout(x[:0])
    assert f0.shape == (0, 768) and r0.shape == (0, 1, 197) and r0.dtype == torch.float32


def test_tower_errors(models, dyn):
    m = models["comp"]
    x = tiles(1, 224, 224, seed=1)
    for bad in (DEPTH, -DEPTH - 1, True, 1.5):
        for t in (x, x[:0]):
            with pytest.raises(ValueError, match="start_block"):
                m.encode_image_rollout(t, start_block=bad)
    for bad in (1.0, -0.1, float("nan")):
        for t in (x, x[:0]):
            with pytest.raises(ValueError, match="residual"):
                m.encode_image_rollout(t, residual=bad)
    with pytest.raises(ValueError, match="224x224"):
        m.encode_image_rollout(torch.zeros(1, 3, 256, 256))     # a 224-only model rejects other sizes, as encode_image does
    with pytest.raises(ValueError, match="multiples of 16"):
        dyn.encode_image_rollout(torch.zeros(1, 3, 200, 224))
    with pytest.raises(ValueError, match=r"\[B,3,H,W\]"):
        m.encode_image_rollout(torch.zeros(1, 224, 224, 3))
    # the C ABI checks its arguments itself
    import ctypes
    from keep_amd.model import _ptr, _stream
    lib = _lib.load()
    xd = x.to(DEV)
    out, roll = torch.empty(1, 768, device=DEV), torch.empty(1, 1, 197, device=DEV)
    need = ctypes.c_int64(0)
    assert lib.keep_rollout_scratch_bytes(m._handle, 1, 224, 224, ctypes.byref(need)) == 0 and need.value >= 3 * 197 * 197 * 4
    assert lib.keep_rollout_scratch_bytes(m._handle, 1, 224, 200, ctypes.byref(need)) == _lib.KEEP_EINVAL
    assert lib.keep_rollout_scratch_bytes(m._handle, 1, 224, 224, None) == _lib.KEEP_EINVAL
    assert lib.keep_rollout_scratch_bytes(m._handle, 1, 224, 224, ctypes.byref(need)) == 0
    scratch = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    st = _stream(xd.device)

    def call(start=0, residual=0.5, H=224, W=224, o=out, r=roll, s=scratch, nbytes=need.value):
        return lib.keep_encode_image_rollout(m._handle, _ptr(xd), _lib.PIX_F32, 1, H, W, start, residual, _ptr(o), _ptr(r), _ptr(s), nbytes, st)

    for start in (DEPTH, -DEPTH - 1):
        assert call(start=start) == _lib.KEEP_EINVAL
    for residual in (1.0, -0.1, float("nan"), float("inf")):
        assert call(residual=residual) == _lib.KEEP_EINVAL
    assert call(W=200) == _lib.KEEP_EINVAL
    assert call(r=None) == _lib.KEEP_EINVAL and call(s=None) == _lib.KEEP_EINVAL
    assert call(nbytes=need.value - 1) == _lib.KEEP_EINVAL      # a scratch that is too small
    assert call(start=-1) == 0 and call() == 0
    torch.cuda.synchronize()
    assert torch.equal(roll.cpu(), m.encode_image_rollout(x)[1])


# ------------------------------------------------------------------------------------------------ regions, end to end
@pytest.fixture(scope="module")
def region():
    g = torch.Generator().manual_seed(77)
    return torch.randint(0, 256, (448, 672, 3), dtype=torch.uint8, generator=g)


@pytest.fixture(scope="module")
def region_rollout(models, region):
    return models["comp"].encode_region_rollout(region.to(DEV), 224, batch=4)      # two batches: 4 + 2 tiles


def test_encode_region_rollout(small, models, region, region_rollout):
    m = models["comp"]
    rd = region.to(DEV)
    feats, coords, roll = region_rollout
    assert feats.shape == (6, 768) and coords.shape == (6, 2) and roll.shape == (6, 1, 197) and roll.device == rd.device
    m.set_option("graphs", 0)
    f_ref, c_ref = m.encode_region(rd, 224, batch=4)
    m.set_option("graphs", 1)
    assert torch.equal(coords, c_ref) and torch.equal(feats, f_ref)
    assert torch.equal(m.encode_region(rd, 224, batch=4)[1], coords)                # and the existing callers get what they got
    cut = normalise_u8(m.region_patches_uint8(rd, coords, 224)).cpu()
    ref, e16 = Yardstick(small, cut).ref(0, 0.5)
    err = AR.max_rel(roll[:, 0].cpu(), ref)
    print(f"[region 448x672 comp rollout] max rel err {err:.3e}, E16 {e16:.3e}, ratio {err / e16:.3f} (bar {BAR['comp']})")
    assert err <= BAR["comp"] * e16
    with pytest.raises(ValueError, match="start_block"):
        m.encode_region_rollout(rd, 224, start_block=DEPTH)
    with pytest.raises(ValueError, match="residual"):
        m.encode_region_rollout(rd, 224, residual=1.0)
    f_host, c_host, r_host = m.encode_region_rollout(region, 224, batch=4)          # a host region: results on the host
    assert r_host.device.type == "cpu" and torch.equal(c_host, coords.cpu()) and torch.equal(r_host, roll.cpu())
    empty = m.encode_region_rollout(rd[:100], 224)
    assert empty[0].shape == (0, 768) and empty[1].shape == (0, 2) and empty[2].shape == (0, 1, 197)


def test_attention_heatmap_takes_the_rollout_as_it_is(models, region_rollout):
    m = models["comp"]
    _, coords, roll = region_rollout
    got = wsi.attention_heatmap(m, roll, coords, (14, 14), 224, 16, (28, 42))
    want = m.cell_raster(coords, cls_attention_map(roll), (14, 14), 224, 16, (28, 42))
    assert isinstance(got, TileRaster) and got.tiles == 6 and torch.equal(got.acc, want.acc)
    assert int(got.count.min()) == 1 and float(got.mean().max()) == 1.0          # six tiles side by side; every tile's strongest patch is 1
    assert m.render_heatmap(got).shape == (28, 42, 3)
