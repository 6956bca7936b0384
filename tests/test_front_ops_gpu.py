"""What the towers run in front of their first block and behind their last one, and the kernels that move CLS rows, each against a host
reference of the same operator (through the C ABI): im2col for the four pixel types, the EPI_PATCH epilogue on every GEMM route, the BERT
embeddings, the strided final LayerNorm and pooler GEMM, the row gathers / scatter, and the two kernels of the bias compensation.

Planes and row movers are compared bit for bit; every other bound is one tests/test_ops_gpu.py already holds or is derived here from the
number formats and the length of the kernel's summation chains.  None is fitted to what the kernels return.  References come from
tests/front_reference.py (checked on the CPU by tests/test_front_ops.py) and are computed once per shape."""
import functools
import math

import pytest
import torch

import front_reference as R
from keep_amd.ops import Ops
from test_ops_gpu import r16, rand

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24            # unit roundoff of fp32
SENTINEL = 0x3C           # byte the lo plane is preset to: fp16 words 0x3C3C (1.0586), which no split of these pixels produces everywhere


def handle(**options):
    """Options are per handle: a test that sets one makes its own and leaves the session's `ops` at its defaults."""
    o = Ops(DEV)
    for k, v in options.items():
        o.set_option(k, v)
    return o


def num_cus():
    """What keep_num_cus returns for the device: the same attribute (hipDeviceAttributeMultiprocessorCount) through torch."""
    return torch.cuda.get_device_properties(torch.device(DEV)).multi_processor_count


# ------------------------------------------------------------------ a. im2col planes, bit for bit
SPECIALS = [0.0, -0.0] + [s * 2.0 ** e for e in range(-20, 16) for s in (1.0, -1.0)]
FLOAT_TYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def float_pixels(B, gh, gw, dtype, seed):
    """N(0, 1) with magnitudes from 2^-20 to 2^15 and both zeros inserted at a stride that is coprime to every extent, cast to `dtype`"""
    x = rand(B, 3, 16 * gh, 16 * gw, seed=seed)
    flat = x.view(-1)
    idx = torch.arange(0, flat.numel(), 7)[:4 * len(SPECIALS)]
    flat[idx] = torch.tensor(SPECIALS, dtype=torch.float32).repeat(4)[:idx.numel()]
    return x.to(dtype)


def u8_pixels(B, gh, gw, seed):
    """uint8 [B, H, W, 3]: every channel of every image is a sequence of permutations of 0..255, so every byte value occurs in every channel"""
    g = torch.Generator().manual_seed(seed)
    n = B * 16 * gh * 16 * gw
    chans = [torch.rand((n + 255) // 256, 256, generator=g).argsort(1).view(-1)[:n] for _ in range(3)]       # one random permutation per row
    u = torch.stack(chans, dim=1).to(torch.uint8).view(B, 16 * gh, 16 * gw, 3)
    for c in range(3):
        assert u[..., c].unique().numel() == 256
    return u


def expected_planes(pixels):
    """(hi, lo) fp16 [B gh gw, 768] of what im2col must write: split_planes of the fp32 value of the pixel at the mapped position"""
    x32 = R.normalize_u8(pixels) if pixels.dtype == torch.uint8 else pixels.float()
    return R.split_planes(R.im2col_patches(x32))


def patch_weights(D, P, seed, w_std=768 ** -0.5):
    return (rand(D, 768, seed=seed, std=w_std), rand(D, seed=seed + 1, std=0.1), rand(D, seed=seed + 2), rand(P + 1, D, seed=seed + 3))


def first_differences(got, want, n=6):
    """[(row, column, word read, word expected)] of the first n words that differ, hexadecimal"""
    at = (got != want).nonzero()[:n].tolist()
    return [(r, c, f"{got[r, c].item() & 0xffff:04x}", f"{want[r, c].item() & 0xffff:04x}") for r, c in at]


def check_planes(o, pixels, gh, gw, what):
    """split 1: both planes equal the reference's words; split 0: the hi plane does and the lo plane still holds its preset.  The CLS rows of
    the token stream equal torch's fp32 cls + pos[0].  -> the number of words compared"""
    B, P, D = pixels.shape[0], gh * gw, 128
    w, bias, cls, pos = patch_weights(D, P, seed=900)
    hi_ref, lo_ref = (R.bits16(t).to(DEV) for t in expected_planes(pixels))
    cls_ref = (cls + pos[0]).to(DEV)
    xd = pixels.to(DEV)
    for split in (1, 0):
        resid, hi, lo = o.patch_embed(xd, w, bias, cls, pos, gh, gw, split=bool(split), sentinel=SENTINEL)
        bad_hi = int((R.bits16(hi) != hi_ref).sum())
        want_lo = lo_ref if split else torch.full_like(lo_ref, SENTINEL * 257)
        bad_lo = int((R.bits16(lo) != want_lo).sum())
        print(f"[im2col {what} B {B} grid {gh}x{gw} split {split}] words differing: hi {bad_hi}, lo {bad_lo} of {hi_ref.numel()} (bound 0)")
        assert bad_hi == 0, f"{what}: {bad_hi} hi words differ: {first_differences(R.bits16(hi), hi_ref)}"
        assert bad_lo == 0, f"{what}: {bad_lo} lo words differ{'' if split else ' from the preset (the plane was written)'}: {first_differences(R.bits16(lo), want_lo)}"
        assert torch.equal(resid.view(B, P + 1, D)[:, 0], cls_ref.expand(B, D))
    return hi_ref.numel()


GRIDS = [(14, 14), (2, 3), (1, 1), (16, 16)]


@pytest.mark.parametrize("gh,gw", GRIDS)
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16", "u8"])
def test_im2col_planes_bit_exact(ops, kind, gh, gw):
    """im2col_kernel<DT, 14 | 0> and im2col_u8_kernel<14 | 0>: both planes, word for word, against split_planes of the pixel the index map of
    front_reference.im2col_patches puts there (a swapped gh / gw, a dropped or stale lo plane, a wrong half of a 16-pixel row all differ).
    Padding rows of the blk planes are not read back."""
    for B in (1, 3):
        pixels = u8_pixels(B, gh, gw, seed=10 + B) if kind == "u8" else float_pixels(B, gh, gw, FLOAT_TYPES[kind], seed=20 + B)
        if kind == "f16":           # fp16 pixels are their own hi plane: the lo plane is +0 throughout
            assert R.bits16(expected_planes(pixels)[1]).eq(0).all()
        check_planes(ops, pixels, gh, gw, kind)


# the launch is capped at 4096 workgroups of 256 work items (8 pixels of one image row each): beyond 4096 * 256 items the grid-stride loop wraps.
# float kernels: B * 3 * 16 gh * 2 gw items; uint8: B * 16 gh * 2 gw.  The smallest B past the cap, per kernel instantiation.
WRAP_CASES = [("f32", 14, 14, 56), ("f16", 14, 14, 56), ("bf16", 14, 14, 56), ("u8", 14, 14, 168),
              ("f32", 16, 16, 43), ("f16", 16, 16, 43), ("bf16", 16, 16, 43), ("u8", 16, 16, 129)]


@pytest.mark.parametrize("kind,gh,gw,B", WRAP_CASES)
def test_im2col_grid_stride_wraps(ops, kind, gh, gw, B):
    items = B * (1 if kind == "u8" else 3) * 16 * gh * 2 * gw
    assert items > 4096 * 256 >= (B - 1) * (1 if kind == "u8" else 3) * 16 * gh * 2 * gw
    pixels = u8_pixels(B, gh, gw, seed=30) if kind == "u8" else float_pixels(B, gh, gw, FLOAT_TYPES[kind], seed=31)
    check_planes(ops, pixels, gh, gw, kind + " wrap")


# ------------------------------------------------------------------ b. EPI_PATCH on every GEMM route
def route_skinny(D, ops):
    """default options, M <= gemm_skinny_m = 320: the register-direct split-K kernels (32 x 128 tiles below 64 rows, 128 x 128 from 64 up) and
    gemm_skinny_reduce_kernel<EPI_PATCH>"""
    return ops, [(14, 14, 1), (2, 3, 50), (2, 3, 3)]


def route_ksliced(D, ops):
    """default options, M > 320 and fewer than gemm_splitk_tiles = 64 tiles of 256 x 256: K cut into slices (EPI_PARTIAL) and the same reduce"""
    return ops, [(14, 14, 2), (14, 14, 5)]


def route_one_tile(D, ops):
    """no split-K path, no persistent walk: the 256-wide LDS-DMA kernel (D % 256 == 0), one tile per workgroup, with its own EPI_PATCH epilogue"""
    return handle(gemm_skinny_m=0, gemm_splitk_tiles=0, gemm_persistent=0), [(14, 14, 3), (2, 3, 3), (16, 16, 1)]


def route_one_tile_128(D, ops):
    """gemm_impl = 128: the 128-wide tiles of the same kernel (gemm_impl != 0 also bars both split-K paths)"""
    return handle(gemm_impl=128, gemm_persistent=0), [(14, 14, 3), (2, 3, 3)]


def route_persistent(D, ops):
    """gemm_persistent = 1 and more 256 x 256 tiles than CUs, the condition under which launch_gemm_f16_v2 walks the tile list with one workgroup per
    CU.  It offers the walk to the fp16 and residual epilogues of single-pass products only (launch_v2_pers is not instantiated for EPI_PATCH), so
    what runs here is the one-tile-per-workgroup kernel with more workgroups than CUs: this case pins that dispatch rule's result.  A small grid
    keeps the pixels small: 2 x 3 patches, B from the CU count."""
    nt = D // 256
    M = 256 * (num_cus() // nt) + 1                       # ceil(M / 256) * nt > CUs
    return handle(gemm_persistent=1), [(2, 3, (M + 5) // 6)]


ROUTES = {"skinny": route_skinny, "ksliced": route_ksliced, "one_tile": route_one_tile, "one_tile_128": route_one_tile_128, "persistent": route_persistent}


def assert_route(o, route, M, D):
    """The library does not report the kernel an op call took; the dispatch of launch_gemm_f16 is a function of these options and the shape,
    restated here from its source, and the options are read back from the handle."""
    impl, skinny_m, tiles_opt, pers = (int(o.get_option(k)) for k in ("gemm_impl", "gemm_skinny_m", "gemm_splitk_tiles", "gemm_persistent"))
    tiles = (M + 255) // 256 * (D // 256)
    S = min(8, 256 // tiles if tiles < tiles_opt else 1, 24 // 8)
    if route == "skinny":
        assert impl == 0 and M <= skinny_m
    elif route == "ksliced":
        assert impl == 0 and M > skinny_m and D % 256 == 0 and S >= 2
    elif route == "one_tile":
        assert impl == 0 and skinny_m == 0 and tiles_opt == 0 and pers == 0 and D % 256 == 0
    elif route == "one_tile_128":
        assert impl == 128 and pers == 0
    else:
        assert impl == 0 and pers == 1 and M > skinny_m and S < 2 and tiles > num_cus()


@functools.lru_cache(maxsize=None)
def patch_case(gh, gw, B):
    """N(0, 1) pixels on the device, their reference planes, and the rows of the token stream the patches go to"""
    pixels = rand(B, 3, 16 * gh, 16 * gw, seed=40 + gh + B)
    hi, lo = expected_planes(pixels)
    P = gh * gw
    m = torch.arange(B * P)
    return pixels.to(DEV), hi, lo, (m // P) * (P + 1) + 1 + m % P


def onehot_columns(D):
    return (torch.arange(D) * 331 + 5) % 768              # 331 is coprime to 768: every patch element is selected (D >= 768)


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("D", [1024, 768])
@pytest.mark.parametrize("route", list(ROUTES))
def test_epi_patch_structure(ops, route, D, split):
    """torch.equal on fp32: with zero pixels every patch row is pos[1 + p] (+ bias), every CLS row cls + pos[0], and no row keeps the NaN preset;
    with one-hot weight rows output (b, p, n) is hi (+ lo when split) of element j(n) of patch (b, p): the row remap b (P + 1) + 1 + p, the
    position row, and the operand's layout on this route are all exact statements."""
    o, shapes = ROUTES[route](D, ops)
    for gh, gw, B in shapes:
        P, M = gh * gw, B * gh * gw
        assert_route(o, route, M, D)
        w, bias, cls, pos = patch_weights(D, P, seed=50 + P)
        zeros = torch.zeros(B, 3, 16 * gh, 16 * gw, device=DEV)
        cls_rows = (cls + pos[0]).expand(B, D).to(DEV)
        # zero pixels, zero bias: the position table, remapped
        resid = o.patch_embed(zeros, w, torch.zeros(D), cls, pos, gh, gw, split=bool(split), lo=False)[0].view(B, P + 1, D)
        assert not torch.isnan(resid).any(), "a row of the token stream was not written"
        assert torch.equal(resid[:, 1:], pos[1:].to(DEV).expand(B, P, D)), "position rows"
        assert torch.equal(resid[:, 0], cls_rows)
        # zero pixels, zero position table: the bias
        zpos = torch.zeros(P + 1, D)
        resid = o.patch_embed(zeros, w, bias, cls, zpos, gh, gw, split=bool(split), lo=False)[0].view(B, P + 1, D)
        assert torch.equal(resid[:, 1:], bias.to(DEV).expand(B, P, D)), "bias"
        assert torch.equal(resid[:, 0], cls.to(DEV).expand(B, D))
        # one-hot weight rows: not transposed, not permuted -- channel, row and column within the patch, both 8-pixel halves
        pixels, hi, lo, rows = patch_case(gh, gw, B)
        j = onehot_columns(D)
        w1 = torch.zeros(D, 768)
        w1[torch.arange(D), j] = 1.0
        want = (hi.float() + lo.float() if split else hi.float())[:, j].to(DEV)        # hi + lo is exact in fp32 (22 significant bits at most)
        resid = o.patch_embed(pixels, w1, torch.zeros(D), cls, zpos, gh, gw, split=bool(split), lo=False)[0]
        got = resid[rows.to(DEV)]
        bad = int((got != want).sum())
        print(f"[EPI_PATCH {route} D {D} split {split} grid {gh}x{gw} B {B} M {M}] one-hot elements differing: {bad} of {want.numel()} (bound 0)")
        assert bad == 0
        assert torch.equal(resid.view(B, P + 1, D)[:, 0], cls.to(DEV).expand(B, D))


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("D", [1024, 768])
@pytest.mark.parametrize("route", list(ROUTES))
def test_epi_patch_numerics(ops, route, D, split):
    """N(0, 1) pixels, W ~ N(0, 1 / 768), bias std 0.1, pos std 1 against fp64.  Split: the bound test_linear_bias holds for split products,
    2e-5 * max(1, max |ref|).  Plain: against the fp64 product of the fp16-rounded operands with that test's accumulation term alone,
    2e-5 * sqrt(K) (the epilogue writes fp32: there is no fp16-output term)."""
    o, shapes = ROUTES[route](D, ops)
    for gh, gw, B in shapes:
        P, M = gh * gw, B * gh * gw
        assert_route(o, route, M, D)
        w, bias, cls, pos = patch_weights(D, P, seed=60 + P)
        pixels, _, _, rows = patch_case(gh, gw, B)
        where = DEV if M > 2048 else "cpu"               # the fp64 product of the largest case on the device (torch's fp64 matmul), the others on the host
        pat = R.im2col_patches(pixels.cpu())
        A, Wm = (pat.double(), w.double()) if split else (r16(pat), r16(w))
        ref = A.to(where) @ Wm.to(where).t() + bias.double().to(where) + pos[1:].double().to(where).repeat(B, 1)
        resid = o.patch_embed(pixels, w, bias, cls, pos, gh, gw, split=bool(split), lo=False)[0]
        err = (resid[rows.to(DEV)].double().to(where) - ref).abs().max().item()
        bound = 2e-5 * max(1.0, ref.abs().max().item()) if split else 2e-5 * math.sqrt(768)
        print(f"[EPI_PATCH {route} D {D} split {split} grid {gh}x{gw} B {B} M {M}] max err {err:.3e} (bound {bound:.3e})")
        assert err < bound
        assert torch.equal(resid.view(B, P + 1, D)[:, 0], (cls + pos[0]).to(DEV).expand(B, D))


# ------------------------------------------------------------------ c. BERT embeddings
VOCAB, TYPES, MAXPOS = 97, 2, 512


@functools.lru_cache(maxsize=None)
def bert_tables(H):
    """word, position and type tables of comparable size with an offset, gamma about 1, beta about 0: the LayerNorm output is O(1), as in test_layernorm"""
    return (rand(VOCAB, H, seed=70, std=2.0) + 0.7, rand(MAXPOS, H, seed=71, std=1.5), rand(TYPES, H, seed=72, std=1.0),
            1 + rand(H, seed=73, std=0.1), rand(H, seed=74, std=0.1))


def bert_ids(P, T, seed):
    g = torch.Generator().manual_seed(seed)
    ids, ty = torch.randint(VOCAB, (P, T), generator=g), torch.randint(TYPES, (P, T), generator=g)
    if P * T == 1:
        return [(torch.zeros(1, 1, dtype=torch.int64), ty), (torch.full((1, 1), VOCAB - 1), 1 - ty)]
    ids.view(-1)[0], ids.view(-1)[-1] = 0, VOCAB - 1
    ty.view(-1)[0], ty.view(-1)[-1] = 0, 1
    return [(ids, ty)]


@pytest.mark.parametrize("P,T", [(1, 1), (3, 5), (2, 64), (1, 512)])
@pytest.mark.parametrize("H", [256, 768, 1024])
def test_bert_embed(ops, H, P, T):
    """bert_embed_ln_kernel<1 | 3 | 4>: the fp32 output against the fp64 LayerNorm of the fp32 sum in HF's order to the 5e-6 test_layernorm holds;
    the planes are split_planes of that output, bit for bit; position rows by row % T (in (3, 5) a workgroup's four rows straddle prompts); a null
    type_ids; the id / type clamp and its error bit."""
    wemb, pemb, temb, gamma, beta = bert_tables(H)
    eps, worst = 1e-12, 0.0
    for ids, ty in bert_ids(P, T, seed=80 + P + T):
        for types in (ty, None):
            resid, hi, lo, err = ops.bert_embed(ids, types, wemb, pemb, temb, gamma, beta, eps)
            ref = R.bert_embed_ref(ids, types, wemb, pemb, temb, gamma, beta, eps)
            worst = max(worst, (resid.cpu().double() - ref).abs().max().item())
            assert (resid.cpu().double() - ref).abs().max().item() < 5e-6
            assert err == 0
            h_ref, l_ref = R.split_planes(resid.cpu())
            assert torch.equal(R.bits16(hi.cpu()), R.bits16(h_ref)), first_differences(R.bits16(hi.cpu()), R.bits16(h_ref))
            assert torch.equal(R.bits16(lo.cpu()), R.bits16(l_ref)), first_differences(R.bits16(lo.cpu()), R.bits16(l_ref))
            # without a lo plane (the single-pass text tower) the hi plane and the output are the same
            resid1, hi1, lo1, err1 = ops.bert_embed(ids, types, wemb, pemb, temb, gamma, beta, eps, lo=False)
            assert lo1 is None and err1 == 0 and torch.equal(resid1, resid) and torch.equal(hi1, hi)
        # out-of-table ids and types: clamped, flagged, and nobody else's row moves
        clean = ops.bert_embed(ids, ty, wemb, pemb, temb, gamma, beta, eps)[0]
        n = P * T
        for row, bad_id, bad_ty in ((0, -1, None), (n - 1, VOCAB, None), (n // 2, None, TYPES), (n // 2, -5, -1)):
            ids_b, ty_b = ids.clone(), ty.clone()
            if bad_id is not None:
                ids_b.view(-1)[row] = bad_id
            if bad_ty is not None:
                ty_b.view(-1)[row] = bad_ty
            resid, hi, lo, err = ops.bert_embed(ids_b, ty_b, wemb, pemb, temb, gamma, beta, eps)
            assert err & 1, f"id {bad_id} type {bad_ty} at row {row}: error word {err}"
            ids_c, ty_c = R.clamp_ids(ids_b, VOCAB), R.clamp_ids(ty_b, TYPES)
            ref = R.bert_embed_ref(ids_c, ty_c, wemb, pemb, temb, gamma, beta, eps)
            assert (resid.cpu().double() - ref).abs().max().item() < 5e-6
            assert torch.equal(resid, ops.bert_embed(ids_c, ty_c, wemb, pemb, temb, gamma, beta, eps)[0])       # the row at the clamped ids
            keep = torch.ones(n, dtype=torch.bool)
            keep[row] = False
            assert torch.equal(resid[keep.to(DEV)], clean[keep.to(DEV)])
    print(f"[bert_embed H {H} P {P} T {T}] max err {worst:.3e} (bound 5.000e-06); planes: 0 words differing (bound 0)")


@pytest.mark.parametrize("P,T", [(1, 7), (3, 5)])
@pytest.mark.parametrize("H", [256, 768, 1024])
def test_bert_embed_order_of_the_sum(ops, H, P, T):
    """(word + type) + position, HF's order, made visible at the 5e-6 of the test above: word rows 2^20 + a and type rows -2^20 + c with a, c
    multiples of 1/8 below 8 are exact in fp32 and so is their sum a + c, to which an N(0, 1) position row is then added with one rounding.
    Either other association first adds the position row to a number of size 2^20 and rounds it to a multiple of 1/8 (2^-4 of error at
    most, 2^-5 on average): four orders of magnitude over the bound after the LayerNorm."""
    g = torch.Generator().manual_seed(85)
    eighths = lambda *shape: torch.randint(-63, 64, shape, generator=g).float() / 8
    wemb, temb, pemb = 2.0 ** 20 + eighths(VOCAB, H), -2.0 ** 20 + eighths(TYPES, H), rand(MAXPOS, H, seed=86)
    gamma, beta = 1 + rand(H, seed=87, std=0.1), rand(H, seed=88, std=0.1)
    ids, ty = bert_ids(P, T, seed=89)[0]
    s = R.bert_embed_sum(ids, ty, wemb, pemb, temb)
    assert s.abs().max() < 32 and (s.double() - (wemb[ids].double() + temb[ty].double() + pemb[:T].double().repeat(P, 1, 1)).view(P * T, H)).abs().max() < 2e-6
    other = (wemb[ids] + (temb[ty] + pemb[:T].expand(P, T, H))).view(P * T, H)
    assert (other - s).abs().max() > 1e-2                # the reference itself tells the orders apart
    resid, hi, lo, err = ops.bert_embed(ids, ty, wemb, pemb, temb, gamma, beta, 1e-12)
    ref = R.bert_embed_ref(ids, ty, wemb, pemb, temb, gamma, beta, 1e-12)
    worst = (resid.cpu().double() - ref).abs().max().item()
    print(f"[bert_embed order H {H} P {P} T {T}] max err {worst:.3e} (bound 5.000e-06)")
    assert err == 0 and worst < 5e-6


# ------------------------------------------------------------------ d. strided tails
LN_ROWS = [1, 3, 5, 260]


@pytest.mark.parametrize("mult", [1, 197, 5])
@pytest.mark.parametrize("D", [1024, 768])
def test_layernorm_rows_strided(ops, D, mult):
    """launch_layernorm with x_stride != D (the final norm reads row 0 of every tile out of [B ntok][D]) against fp64 to the 5e-6 of
    test_layernorm.  Every element of the buffer that is not in a row to be read is NaN: a wrong stride cannot pass."""
    stride, R_max, eps = mult * D, max(LN_ROWS), 1e-6
    x = rand(R_max, D, seed=90 + mult, std=3.0) + 0.7
    g, b = 1 + rand(D, seed=91, std=0.1), rand(D, seed=92, std=0.1)
    ref = torch.nn.functional.layer_norm(x.double(), (D,), g.double(), b.double(), eps)
    buf = torch.full((R_max, stride), float("nan"), device=DEV)
    buf[:, :D] = x.to(DEV)
    worst = 0.0
    for rows in LN_ROWS:
        out = ops.layernorm_rows(buf.view(-1)[:(rows - 1) * stride + D], stride, rows, g, b, eps).cpu().double()
        assert out.shape == (rows, D) and not torch.isnan(out).any()
        worst = max(worst, (out - ref[:rows]).abs().max().item())
        assert (out - ref[:rows]).abs().max().item() < 5e-6
    print(f"[layernorm_rows D {D} x_stride {mult} D] max err {worst:.3e} (bound 5.000e-06)")


SG_M = [1, 16, 17, 70]
GAP = 7.25


@functools.lru_cache(maxsize=None)
def sgemm_case(K):
    a, b, bias = rand(max(SG_M), K, seed=100), rand(K, K, seed=101, std=0.05), rand(K, seed=102, std=0.1)
    acc = 0.5 * (a.double() @ b.double().t()) + bias.double()
    return a, b, bias, {0: acc, 2: torch.tanh(acc)}


@pytest.mark.parametrize("sgemv_m", [16, 0])
@pytest.mark.parametrize("K", [768, 1024])
def test_sgemm_leading_dimensions(K, sgemv_m):
    """launch_sgemm_f32 with lda != K (the BERT pooler reads row p T of the token stream) on both sides of the few-row switch and with the
    few-row kernel switched off, to the 2e-5 of test_sgemm_f32.  The skipped rows of A are NaN; the gap columns of the output keep their preset."""
    o = handle(sgemv_m=sgemv_m)
    assert int(o.get_option("sgemv_m")) == sgemv_m
    N = K
    a, b, bias, refs = sgemm_case(K)
    worst = 0.0
    for lda in (K, 64 * K, 5 * K):
        ldb = K + 4 if lda == 5 * K else K
        abuf = torch.full((max(SG_M), lda), float("nan"), device=DEV)
        abuf[:, :K] = a.to(DEV)
        bbuf = torch.full((N, ldb), float("nan"), device=DEV)
        bbuf[:, :K] = b.to(DEV)
        for M in SG_M:
            for ldo in (N, N + 4):
                for act in (0, 2):
                    out = torch.full((M, ldo), GAP, device=DEV)
                    o.sgemm_ld(abuf, bbuf, bias, M, N, K, lda, ldb, out, ldo, scale=0.5, act=act)
                    assert torch.equal(out[:, N:], torch.full((M, ldo - N), GAP, device=DEV)), "gap columns of the output were written"
                    err = (out[:, :N].cpu().double() - refs[act][:M]).abs().max().item()
                    worst = max(worst, err)
                    assert err < 2e-5, f"M {M} lda {lda} ldo {ldo} act {act}: {err:.3e}"
    print(f"[sgemm_ld N = K {K} sgemv_m {sgemv_m}] max err {worst:.3e} (bound 2.000e-05)")
    for M in (1, 70):
        with pytest.raises(ValueError, match="lda"):                 # KEEP_EUNSUPPORTED from the launcher
            o.sgemm_ld(torch.zeros(70 * (K + 2), device=DEV), b, bias, M, N, K, K + 2, K, torch.zeros(M, N, device=DEV), N)


# ------------------------------------------------------------------ e. row movers
MOVE_ROWS = [1, 2, 3, 256, 257, 260]


def row_pattern(n_rows, D):
    """Integers below 2048 (exact in fp16): v(r, k) = (1021 r + 3 k) mod 2039.  2039 is prime: two rows coincide only 2039 rows apart, a K slice
    shifted by 32 columns or a tile shifted by 256 rows never does."""
    r, k = torch.arange(n_rows, device=DEV).view(-1, 1), torch.arange(D, device=DEV).view(1, -1)
    return ((r * 1021 + k * 3) % 2039).float()


@pytest.mark.parametrize("stride", [197, 65, 1])
@pytest.mark.parametrize("D", [1024, 768])
def test_row_movers(ops, D, stride):
    """gather_rows_kernel, gather_rows_blk_kernel and scatter_rows_kernel with the token stream's row stride: source rows r * stride cross the
    256-row tiles of the blk layout (and from 257 rows so do the destination rows).  torch.equal throughout; after a scatter every row that is
    not a target holds its preset."""
    src = row_pattern(max(MOVE_ROWS) * stride, D)
    for rows in MOVE_ROWS:
        s = src[:rows * stride]
        want = s[::stride]
        assert want.shape == (rows, D)
        assert torch.equal(ops.gather_rows(s, stride, rows), want), f"fp32 gather, {rows} rows"
        assert torch.equal(ops.gather_rows(s, stride, rows, blk=True), want), f"blk gather, {rows} rows"
        dst = torch.full((rows * stride, D), -1.0, device=DEV)
        compact = row_pattern(rows, D) + 1.0
        ops.scatter_rows_(compact, dst, stride)
        assert torch.equal(dst[::stride], compact), f"scatter, {rows} rows"
        rest = torch.ones(rows * stride, dtype=torch.bool, device=DEV)
        rest[::stride] = False
        assert (dst[rest] == -1.0).all(), f"scatter, {rows} rows: a row that is no target was written"
    print(f"[row movers D {D} row stride {stride}] rows {MOVE_ROWS}: 0 elements differing (bound 0)")


# ------------------------------------------------------------------ f. bias-compensation sums
def gamma_n(n):
    """The constant of a length-n fp32 summation chain: |fl(sum) - sum| <= gamma_n * sum |x_k|, gamma_n = n u / (1 - n u) (Higham, Accuracy and
    Stability of Numerical Algorithms, section 4.2: any order of additions in which no term passes through more than n of them)"""
    return n * U / (1 - n * U)


@pytest.mark.parametrize("K", [64, 768])
@pytest.mark.parametrize("M", [1, 255, 256, 257, 600])
def test_blk_col_sum_accumulates(ops, M, K):
    """blk_col_sum_kernel, called twice into one accumulator, against the fp64 column sums of the fp16-rounded inputs.
    The chain a term passes through: thread (rg, k) adds rows rg, rg + 8, ... of every 256-row tile in turn, ceil(rows_t / 8) per tile, L in all;
    the 8 partials of a column are added in order (8 additions at most); the result is added to the accumulator (1), and the second call's
    result is added to that (1 more for the first call's terms).  n = L + 8 + 2; bound gamma_n * sum_k |x_k| over both calls' terms."""
    x1, x2 = rand(M, K, seed=110 + M) + 0.5, rand(M, K, seed=111 + M, std=2.0) - 0.25
    L = sum((min(256, M - t) + 7) // 8 for t in range(0, M, 256))
    n = L + 8 + 2
    acc = torch.zeros(K, device=DEV)
    ops.blk_col_sum_(x1, acc)
    first = acc.clone()
    ops.blk_col_sum_(x2, acc)
    ref1, ref = r16(x1).sum(0), r16(x1).sum(0) + r16(x2).sum(0)
    mag1, mag = r16(x1).abs().sum(0), r16(x1).abs().sum(0) + r16(x2).abs().sum(0)
    err1, err = (first.cpu().double() - ref1).abs(), (acc.cpu().double() - ref).abs()
    print(f"[blk_col_sum M {M} K {K}] chain {n}: max err {err.max():.3e} (bound {(gamma_n(n) * mag).max():.3e}, smallest {(gamma_n(n) * mag).min():.3e})")
    assert (err1 <= gamma_n(n) * mag1).all() and (err <= gamma_n(n) * mag).all()


@pytest.mark.parametrize("K", [64, 768])
@pytest.mark.parametrize("N", [4, 130, 300])
def test_bias_mean_corr(ops, N, K):
    """bias_mean_corr_kernel against fp64 of bias + (w_lo @ col_sum) * inv_rows on the lo plane split_planes gives the weight (rows past 255 are in
    the second tile of the blk plane).  A term passes through: its product (1 rounding; none when the compiler contracts it into the addition),
    the K / 64 additions of its lane, the 6 levels of the wave reduction, the multiplication by inv_rows: n = K / 64 + 8, bound
    gamma_n * inv_rows * sum_k |w_lo[n][k] col_sum[k]|; the final addition of the bias rounds the result once more: + u |ref|."""
    w, bias = rand(N, K, seed=120 + N, std=0.03), rand(N, seed=121, std=0.1)
    col_sum = rand(K, seed=122, std=100.0) + 50.0
    inv_rows = torch.tensor(1.0 / 600.0, dtype=torch.float32).item()               # the fp32 value the kernel is handed
    w_lo = R.split_planes(w)[1].double()
    assert w_lo.abs().max() > 0
    ref = bias.double() + (w_lo @ col_sum.double()) * inv_rows
    n = K // 64 + 8
    bound = gamma_n(n) * inv_rows * (w_lo.abs() @ col_sum.double().abs()) + U * ref.abs()
    out = ops.bias_mean_corr(w, col_sum, inv_rows, bias)
    err = (out.cpu().double() - ref).abs()
    # the correction itself must be visible at this resolution, or the test would pass without it
    assert ((ref - bias.double()).abs() > 4 * bound).float().mean() > 0.5
    print(f"[bias_mean_corr N {N} K {K}] chain {n}: max err {err.max():.3e} (bound {bound.max():.3e}, smallest {bound.min():.3e})")
    assert (err <= bound).all()
