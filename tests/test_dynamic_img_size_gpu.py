"""Tiles of any multiple-of-16 size (timm dynamic_img_size, quick_start/keep_inference.py:32-40): KEEPModel(..., dynamic_img_size=True),
keep_encode_image_hw, keep_vit_pos_embed and the long-sequence attention kernel (Ops.attention_long), on the MI355X.

Reference: oracle.keep_oracle.encode_image(sd', x), sd' = the state dict with visual.pos_embed replaced by timm's
resample_abs_pos_embed, restated below (timm is not a dependency): unchanged at 14 x 14 only; otherwise the CLS row as it is and the
14 x 14 patch table through F.interpolate(bicubic, antialias=True, align_corners=False) in fp32.  The oracle's patchify / vit_tokens are
shape-general already.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from keep_amd import KEEPModel, _lib
from keep_amd.config import KEEPShape, small_shape
from keep_amd.model import _ptr, _stream
from keep_amd.synth import normalise_u8, synth_state_dict, synth_tile_family, towers_of
from oracle import keep_oracle as O

pytestmark = pytest.mark.gpu
COS_TOL = 1e-4
FP16_TOL = 2.5e-4
TOL = {"strict": 2e-6, "comp": COS_TOL, "fp16": FP16_TOL}
SIZES = [(16, 16), (112, 112), (224, 224), (256, 256), (224, 448), (448, 224), (112, 448), (384, 384), (512, 512), (1024, 256)]


def timm_pos_embed(pos, gh, gw, old=(14, 14)):
    """timm.layers.resample_abs_pos_embed(pos, new_size=(gh, gw), old_size=old, num_prefix_tokens=1) as timm 1.0.15 computes it."""
    if gh * gw + 1 == pos.shape[1] and gh == gw:
        return pos
    D = pos.shape[-1]
    cls, grid = pos[:, :1], pos[:, 1:]
    g = grid.reshape(1, old[0], old[1], D).permute(0, 3, 1, 2).float()
    g = F.interpolate(g, size=(gh, gw), mode="bicubic", antialias=True, align_corners=False)
    return torch.cat([cls, g.permute(0, 2, 3, 1).reshape(1, gh * gw, D).to(pos.dtype)], dim=1)


def sd_at(sd, H, W):
    d = dict(sd)
    d["visual.pos_embed"] = timm_pos_embed(sd["visual.pos_embed"], H // 16, W // 16)
    return d


def tiles(n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, H, W, generator=g)


def make_model(sd, precision, dynamic=True, **opts):
    m = KEEPModel(precision=precision, towers=towers_of(sd), dynamic_img_size=dynamic)
    for k, v in opts.items():
        m.set_option(k, v)
    m.load_state_dict(sd, strict=True)
    return m.to("cuda:0").eval()


@pytest.fixture(scope="module")
def small():
    return synth_state_dict(small_shape(2, 2), seed=5)


@pytest.fixture(scope="module")
def text_bank():
    g = torch.Generator().manual_seed(99)
    return F.normalize(torch.randn(64, 768, generator=g), dim=-1)


@pytest.fixture(scope="module")
def models(small):
    return {p: make_model(small, p) for p in ("strict", "comp", "fp16")}


# ------------------------------------------------------------------------------------------------ depth 2 against the oracle
@pytest.mark.parametrize("precision", ["strict", "comp", "fp16"])
def test_depth2_every_size_vs_oracle(small, models, text_bank, precision):
    m = models[precision]
    assert m.dynamic_img_size
    for H, W in SIZES:
        x = tiles(3, H, W, seed=H * 7 + W)
        with torch.no_grad():
            ref = O.encode_image(sd_at(small, H, W), x)
        out = m.encode_image(x)
        assert out.shape == (3, 768) and out.device.type == "cpu"
        dcos = (out @ text_bank.t() - ref @ text_bank.t()).abs().max().item()
        print(f"[d2 {precision} {H}x{W}] max|dfeat|={(out - ref).abs().max():.3e} max|dcos|={dcos:.3e}")
        assert dcos < TOL[precision], (H, W)
        assert torch.equal((out @ text_bank.t()).argmax(1), (ref @ text_bank.t()).argmax(1)), (H, W)


def test_depth2_compensated_plan_at_long_grids_runs(small, text_bank):
    """A plan with the single-pass long kernel writing the CLS-row planes (KEEP_ATTN_PROJ_CLS) and the CLS-only last block, at 256 / 384 / 512 and,
    with grid_plan = 2 (the plan at every grid), at 2049 tokens.  Checked against the fp16 budget: a path check, not a compliance claim."""
    m = make_model(small, "comp", grid_plan=2)
    m.set_plan([(_lib.ATTN_PROJ_CLS, _lib.MLP_CLS), (_lib.ATTN_COMPQKV_PROJ_CLS, _lib.MLP_PLAIN)])
    for H, W in ((384, 384), (512, 512), (256, 256), (512, 1024)):
        x = tiles(3, H, W, seed=H + W + 1)
        with torch.no_grad():
            ref = O.encode_image(sd_at(small, H, W), x)
        out = m.encode_image(x)
        dcos = (out @ text_bank.t() - ref @ text_bank.t()).abs().max().item()
        print(f"[d2 comp plan, {H}x{W}] max|dcos|={dcos:.3e}")
        assert dcos < FP16_TOL


# ------------------------------------------------------------------------------------------------ opt-in and errors
def test_opt_in_and_errors(small, models):
    m = models["comp"]
    x = tiles(4, 224, 224, seed=1)
    off = make_model(small, "comp", dynamic=False)
    assert not off.dynamic_img_size
    assert torch.equal(m.encode_image(x), off.encode_image(x))                    # flag on at 224: bit-identical to flag off
    for bad in ((1, 3, 200, 224), (1, 3, 224, 8), (1, 3, 0, 224), (1, 3, 250, 250)):
        with pytest.raises(ValueError, match="multiples of 16"):
            m.encode_image(torch.zeros(bad))
    with pytest.raises(ValueError, match="multiples of 16"):
        m.encode_image_uint8(torch.zeros((1, 100, 96, 3), dtype=torch.uint8))
    for bad in ((1, 3, 256, 256), (1, 3, 240, 224), (1, 3, 16, 16)):
        with pytest.raises(ValueError, match="224x224"):
            off.encode_image(torch.zeros(bad))
    with pytest.raises(ValueError, match="224x224"):
        off.encode_image_uint8(torch.zeros((1, 256, 256, 3), dtype=torch.uint8))
    with pytest.raises(ValueError):
        m.classify(torch.zeros(1, 3, 256, 256), F.normalize(torch.randn(4, 768), dim=-1))
    # the C ABI: keep_encode_image_hw at 224 x 224 is keep_encode_image, bit for bit; sizes that are not multiples of 16 are KEEP_EINVAL
    lib = _lib.load()
    xd = x.cuda().contiguous()
    a = torch.empty(4, 768, device="cuda")
    b = torch.empty(4, 768, device="cuda")
    st = _stream(xd.device)
    assert lib.keep_encode_image(m._handle, _ptr(xd), _lib.PIX_F32, 4, _ptr(a), st) == 0
    assert lib.keep_encode_image_hw(m._handle, _ptr(xd), _lib.PIX_F32, 4, 224, 224, _ptr(b), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    for H, W in ((0, 224), (224, 0), (-16, 224), (200, 224), (224, 17)):
        assert lib.keep_encode_image_hw(m._handle, _ptr(xd), _lib.PIX_F32, 1, H, W, _ptr(b), st) == _lib.KEEP_EINVAL


def test_grid_rule_runs_unmeasured_grids_strict(models):
    """The compensated plan is calibrated on 197-token tiles and held the tolerance from 197 to 1025 tokens but not below (tools/grid_precision.py,
    DESIGN.md section 9): outside that band KEEP_PREC_COMP runs as KEEP_PREC_STRICT (option grid_plan = 1, the default)."""
    comp, strict = models["comp"], models["strict"]
    assert comp.get_option("grid_plan") == 1
    for H, W in ((1024, 512), (528, 512), (160, 160), (112, 112), (16, 16)):      # 2049, 1057, 101, 50, 2 tokens: strict
        x = tiles(2, H, W, seed=H)
        assert torch.equal(comp.encode_image(x), strict.encode_image(x)), (H, W)
    for H, W in ((224, 224), (112, 448), (256, 256), (512, 512)):                 # 197, 197, 257, 1025 tokens: the plan
        x = tiles(2, H, W, seed=H + 2)
        assert not torch.equal(comp.encode_image(x), strict.encode_image(x)), (H, W)
    comp.set_option("grid_plan", 0)                                               # every grid but 14 x 14 strict
    try:
        x = tiles(2, 256, 256, seed=3)
        assert torch.equal(comp.encode_image(x), strict.encode_image(x))
        x = tiles(2, 224, 224, seed=3)
        assert not torch.equal(comp.encode_image(x), strict.encode_image(x))
    finally:
        comp.set_option("grid_plan", 1)


# ------------------------------------------------------------------------------------------------ the position table
def test_pos_embed_table(small, models):
    m = models["strict"]
    pos = small["visual.pos_embed"]
    D = pos.shape[-1]
    lib = _lib.load()
    for gh, gw in ((14, 14), (1, 1), (7, 7), (7, 28), (16, 16), (24, 24), (32, 32), (64, 16)):
        out = torch.full((gh * gw + 1, D), float("nan"), device="cuda")
        rc = lib.keep_vit_pos_embed(m._handle, gh, gw, _ptr(out), _stream(out.device))
        _lib.check(m._handle, rc, "vit_pos_embed")
        torch.cuda.synchronize()
        ref = timm_pos_embed(pos, gh, gw)[0]
        got = out.cpu()
        if (gh, gw) == (14, 14):
            assert torch.equal(got, ref)
        else:
            err = (got - ref).abs().max().item()
            print(f"[pos {gh}x{gw}] max|d|={err:.3e}")
            assert err < 1e-6, (gh, gw)
            assert torch.equal(got[0], pos[0, 0])
    # 7 x 28: 196 patches but not square, so timm resamples it
    assert not torch.allclose(timm_pos_embed(pos, 7, 28), pos)
    assert lib.keep_vit_pos_embed(m._handle, 0, 4, _ptr(out), None) == _lib.KEEP_EINVAL


# ------------------------------------------------------------------------------------------------ the long-sequence attention kernel
def attn_ref(qkv, B, T, heads, round_ops):
    D = heads * 64
    x = qkv.reshape(B, T, 3, heads, 64).permute(2, 0, 3, 1, 4).double()
    if round_ops:
        x = x.to(torch.float16).double()
    q, k, v = x[0], x[1], x[2]
    p = torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1)
    return (p @ v).transpose(1, 2).reshape(B * T, D)


def rand_qkv(B, T, heads, seed, std=1.5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B * T, 3 * heads * 64, generator=g) * std


@pytest.fixture(scope="module")
def ops():
    from keep_amd.ops import Ops
    return Ops("cuda:0")


@pytest.mark.parametrize("T", [513, 577, 785, 1025, 2049])
@pytest.mark.parametrize("split", [False, True])
def test_attention_long(ops, T, split):
    B, heads = 2, 3
    qkv = rand_qkv(B, T, heads, seed=T)
    out = ops.attention_long(qkv, B, T, heads, split).cpu().double()
    assert (out - attn_ref(qkv, B, T, heads, not split)).abs().max() < (3e-5 if split else 4e-3)


@pytest.mark.parametrize("split", [False, True])
def test_attention_long_rescale_and_many_workgroups(ops, split):
    """A key late in the sequence whose score jumps far above everything before it (the running maximum moves by ~40 in the log2 domain at
    one block: every output accumulated so far must be rescaled exactly once), and B * heads above the CU count (320 (image, head) pairs)."""
    B, T, heads = 20, 577, 16
    qkv = rand_qkv(B, T, heads, seed=7, std=1.0)
    D = heads * 64
    x = qkv.view(B, T, 3, heads, 64)
    x[:, 530, 1] = x[:, :, 0].mean(1) * 12.0            # key 530 of every head aligned with the mean query
    x[:, 3, 1] = -x[:, :, 0].mean(1) * 6.0
    out = ops.attention_long(qkv, B, T, heads, split).cpu().double()
    assert (out - attn_ref(qkv, B, T, heads, not split)).abs().max() < (3e-5 if split else 4e-3)
    assert D == 1024


@pytest.mark.parametrize("split", [False, True])
def test_attention_long_q_rows(ops, split):
    B, T, heads = 3, 1025, 4
    qkv = rand_qkv(B, T, heads, seed=11)
    out = ops.attention_long(qkv, B, T, heads, split, q_rows=1).cpu().double().view(B, T, -1)
    ref = attn_ref(qkv, B, T, heads, not split).view(B, T, -1)
    assert (out[:, 0] - ref[:, 0]).abs().max() < (3e-5 if split else 4e-3)
    assert (out[:, 1:] == 0).all()


def test_attention_long_is_not_in_the_short_dispatch(ops):
    with pytest.raises(ValueError):
        ops.attention(rand_qkv(1, 600, 1, seed=1), 1, 600, 1)


# ------------------------------------------------------------------------------------------------ invariance
def test_invariance_512(small):
    m = make_model(small, "strict")
    x = tiles(24, 512, 512, seed=5)
    full = m.encode_image(x)
    # position inside a batch of the same size: bit-identical
    perm = torch.randperm(24, generator=torch.Generator().manual_seed(1))
    assert torch.equal(m.encode_image(x[perm]), full[perm])
    # batch size, max_tiles chunking, lanes: other sub-batch sizes pick other GEMM kernels -> within the strict-mode budget
    for opts, sel in (({}, slice(0, 1)), ({}, slice(5, 12)), ({"max_tiles": 20}, slice(None)), ({"max_tiles": 60}, slice(None)),
                      ({"streams": 1}, slice(None)), ({"streams": 3, "lane_min_tiles": 6}, slice(None))):
        for k, v in opts.items():
            m.set_option(k, v)
        out = m.encode_image(x[sel])
        assert (out - full[sel]).abs().max() < 2e-6, opts
    m.set_option("max_tiles", 256); m.set_option("streams", 2); m.set_option("lane_min_tiles", 16)
    # graph replay (256 x 256: 257 tokens, so up to 3 tiles replay a captured graph) against the plain path
    y = tiles(3, 256, 256, seed=6)
    g1 = m.encode_image(y)
    g2 = m.encode_image(y)
    m.set_option("graphs", 0)
    plain = m.encode_image(y)
    m.set_option("graphs", 1)
    assert torch.equal(g1, g2) and torch.equal(g1, plain)


def test_alternating_sizes_are_stable(small):
    m = make_model(small, "fp16")
    xs = {s: tiles(4, s, s, seed=s) for s in (224, 512, 256)}
    first = {s: m.encode_image(x) for s, x in xs.items()}
    for _ in range(2):
        for s in (224, 512, 256, 512, 224):
            assert torch.equal(m.encode_image(xs[s]), first[s]), s


def test_uint8_matches_float_at_256(small):
    m = make_model(small, "strict")
    u8 = torch.randint(0, 256, (5, 256, 256, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    a = m.encode_image_uint8(u8)
    b = m.encode_image(normalise_u8(u8))
    assert (a - b).abs().max() < 1e-5


# ------------------------------------------------------------------------------------------------ full depth, bench weights
@pytest.fixture(scope="module")
def bench():
    sd = synth_state_dict(KEEPShape(), seed=0)
    m = KEEPModel(KEEPShape(), dynamic_img_size=True)
    m.load_state_dict(sd)                   # calibrated as shipped
    return m.to("cuda:0").eval(), sd


def family_tiles(size, n=8, seed=7001):
    """n tiles per family at size x size, built from the 224 x 224 family tiles: a 2 x 2 mosaic of four tiles, bicubic-resized to the size."""
    out = []
    for fam in ("he_crops", "stain_field", "background", "half"):
        t = synth_tile_family(fam, 0, 4 * n, "cpu", seed=seed).permute(0, 3, 1, 2).float()
        t = t.view(n, 4, 3, 224, 224)
        mosaic = torch.cat([torch.cat([t[:, 0], t[:, 1]], 3), torch.cat([t[:, 2], t[:, 3]], 3)], 2)        # [n,3,448,448]
        r = F.interpolate(mosaic, size=(size, size), mode="bicubic", antialias=True, align_corners=False)
        out.append(r.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous())
    return torch.cat(out, 0)


@pytest.mark.parametrize("size", [256, 512])
def test_bench_weights_full_depth_vs_oracle(bench, text_bank, size):
    m, sd = bench
    x = normalise_u8(family_tiles(size))
    sd_dev = {k: v.to("cuda:0") for k, v in sd_at(sd, size, size).items() if k.startswith("visual")}
    with torch.no_grad():
        ref = torch.cat([O.encode_image(sd_dev, x[i:i + 8].cuda()) for i in range(0, x.shape[0], 8)]).cpu()
    out_comp = m.encode_image(x)
    m.set_precision("strict")
    out_strict = m.encode_image(x)
    m.set_precision("comp")
    for name, out in (("comp", out_comp), ("strict", out_strict)):
        dcos = (out @ text_bank.t() - ref @ text_bank.t()).abs().max().item()
        print(f"[bench weights {size}x{size} {name}] max|dcos| vs fp32 oracle = {dcos:.3e}")
        assert dcos < COS_TOL
    assert (out_comp @ text_bank.t() - out_strict @ text_bank.t()).abs().max().item() < COS_TOL
