"""The kernels the CLS rows run on, each against an fp64 reference of the same operator (through the C ABI): the small-M split-K GEMM
(32 x 128 and 128 x 128 partial-sum kernels + reduce), the LayerNorm fused into the split-K reduce (keep_op_linear_ln), and the q_rows /
cls_hi + cls_lo features of the short attention kernels (keep_op_attention_cls).

Every bound is one tests/test_ops_gpu.py already holds or follows from the number formats; none is fitted to what the kernels return.
Rows of a GEMM are independent: each fp64 reference is computed once at the largest M of its sweep and sliced."""
import ctypes as C
import functools
import math

import pytest
import torch

from keep_amd import _lib
from keep_amd.model import _ptr, _stream
from keep_amd.ops import EPI_F16, EPI_GELU_F16, EPI_RESID_F32, EPI_RESID_LS, Ops
from test_ops_gpu import attn_ref, gelu64, r16, rand

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def handle(**options):
    """Options are per handle: a test that sets one makes its own and leaves the session's `ops` at its defaults."""
    o = Ops(DEV)
    for k, v in options.items():
        o.set_option(k, v)
    return o


def big_kernel_handle(**more):
    """No split-K path at all: the 256 x 256 (N % 256 != 0: 256 x 128) LDS-DMA kernel, whatever M is."""
    return handle(gemm_skinny_m=0, gemm_splitk_tiles=0, **more)


def operands(M, N, K, seed):
    """activations N(0, 1), weights N(0, 1/K) (the accumulator is O(1) at every K), bias std 0.1, ls uniform in [0.05, 0.5], resid N(0, 1)"""
    a, w, b = rand(M, K, seed=seed), rand(N, K, seed=seed + 1, std=K ** -0.5), rand(N, seed=seed + 2, std=0.1)
    ls = torch.rand(N, generator=torch.Generator().manual_seed(seed + 3)) * 0.45 + 0.05
    return a, w, b, ls, rand(M, N, seed=seed + 4)


def epilogue64(acc, epi, ls, resid):
    if epi == EPI_F16:
        return acc
    if epi == EPI_GELU_F16:
        return gelu64(acc)
    return resid.double() + (ls.double() * acc if epi == EPI_RESID_LS else acc)


# ------------------------------------------------------------------ a. small-M sweep through keep_op_linear
M_SWEEP = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 320]
# (N, K) and the K steps each split-K slice gets (S and ceil(KT / S) from skinny_splits, KT = K / 32; a slice past KT is empty).  "narrow" is
# the 32 x 128 kernel (M < 64, or skinny_wide = 0), "wide" the 128 x 128 one; where one pattern is given both have it at every M of the sweep.
#   (128, 64)     KT 2    [2]                        one slice
#   (128, 96)     KT 3    [3]                        odd KT: one pair of steps, then the tail loop (a slice cannot be shorter than 2 steps unless it is the
#                                                    last one: S <= KT / 2)
#   (128, 224)    KT 7    [3 3 1]                    a last slice of ONE step: the tail loop only (narrow), a single unpaired step (wide)
#   (128, 288)    KT 9    [3 3 3 0]                  the last slice is empty
#   (384, 544)    KT 17   [3 3 3 3 3 2 0 0]          N % 256 != 0; a short slice and two empty ones
#   (1024, 1024)  KT 32   16 x 2 up to M = 129 (narrow) / 256 (wide); wide M >= 257 [3 x 10, 2]; narrow M = 255, 256 [3 x 10, 2, 0],
#                         M = 257 [3 x 10, 2], M = 320 [4 x 8, 0, 0]
#   (3072, 1024)  KT 32   narrow 16 x 2 up to M = 64, then [3 x 10, 2] (65), 8 x 4 (127, 128), [5 x 6, 2] (129), 4 x 8 (M >= 255);
#                         wide [3 x 10, 2] up to M = 128, [6 x 5, 2] up to 256, 4 x 8 above
#   (4096, 1024)  KT 32   narrow 16 x 2 up to M = 32, [3 x 10, 2, 0] up to 64, 8 x 4 (65), [6 x 5, 2] (127, 128), [7 7 7 7 4] (129), [11 11 10] (M >= 255);
#                         wide 8 x 4 up to M = 128, 4 x 8 up to 256, [11 11 10] above
#   (1024, 4096)  KT 128  16 x 8 up to M = 129 (narrow) / 256 (wide); wide M >= 257 [12 x 10, 8]; narrow [11 x 11, 7] (255, 256), [12 x 10, 8] (257),
#                         [13 x 9, 11] (320)
#   (768, 3072)   KT 96   16 x 6 up to M = 256; M >= 257 wide and narrow 257 [7 x 13, 5, 0]; narrow 320 [8 x 12, 0]
GEMM_NK = [(128, 64), (128, 96), (128, 224), (128, 288), (384, 544), (1024, 1024), (3072, 1024), (4096, 1024), (1024, 4096), (768, 3072)]
EPILOGUES = [EPI_F16, EPI_GELU_F16, EPI_RESID_LS, EPI_RESID_F32]


@functools.lru_cache(maxsize=None)
def sweep_case(N, K):
    """Operands on the device and, per (epilogue, split), the fp64 reference at the largest M (fp16-rounded operands for the single pass, exact
    ones for the split product), computed once on the CPU and left unchanged."""
    M = max(M_SWEEP)
    a, w, b, ls, resid = operands(M, N, K, seed=100 + N + K)
    acc = {False: r16(a) @ r16(w).t() + b.double(), True: a.double() @ w.double().t() + b.double()}
    ref = {(epi, sp): epilogue64(acc[sp], epi, ls, resid).to(DEV) for epi in EPILOGUES for sp in (False, True)}
    return tuple(t.to(DEV) for t in (a, w, b, ls, resid)), ref


def linear_bound(ref, epi, split, K):
    """The bounds of test_linear_bias / _gelu / _layerscale_residual / _residual_sum, elementwise."""
    if epi == EPI_RESID_LS:
        return torch.full_like(ref, 3e-5)
    if epi == EPI_RESID_F32:
        return torch.full_like(ref, 5e-5)
    if split:
        return torch.full_like(ref, 2e-5 * max(1.0, ref.abs().max().item()))
    # output rounded to fp16: half an ulp = 2^-11 relative, plus fp32 accumulation noise (GELU: 1e-4 absolute, as test_linear_gelu)
    return 5e-4 * ref.abs() + (1e-4 if epi == EPI_GELU_F16 else 2e-5 * math.sqrt(K))


def check_linear(out, ref, epi, split, K, what):
    err, bound = (out.double() - ref).abs(), linear_bound(ref, epi, split, K)
    bad = err > bound if (epi in (EPI_F16, EPI_GELU_F16) and not split) else err >= bound
    if bad.any():
        i = int((err - bound).argmax())
        r, c = divmod(i, ref.shape[1])
        rows, cols = bad.any(1).nonzero().flatten().tolist(), bad.any(0).nonzero().flatten().tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} elements over the bound; worst at row {r} col {c}: err {err[r, c]:.3e} bound {bound[r, c]:.3e}; "
                             f"rows {rows[:8]}..{rows[-1]} cols {cols[:8]}..{cols[-1]}")
    return err.max().item(), bound.max().item()


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("N,K", GEMM_NK)
def test_small_m_linear_sweep(ops, N, K, split):
    """Every M on both sides of the 32-, 64-, 128- and 256-row edges (narrow / wide switch, tile edges of both kernels, the blk layout's
    256-row tile), every epilogue, three routes: default options, skinny_wide = 0 (the 32 x 128 kernel also from 64 rows up), and the
    256-wide LDS-DMA kernel on a ragged row tile."""
    (a, w, b, ls, resid), ref = sweep_case(N, K)
    routes = [("default", ops, 1), ("narrow", handle(skinny_wide=0), 64), ("big", big_kernel_handle(), 1)]
    worst = {epi: (0.0, 0.0) for epi in EPILOGUES}
    for epi in EPILOGUES:
        kw = dict(ls=ls, resid=None) if epi == EPI_RESID_LS else {}
        for M in M_SWEEP:
            if epi in (EPI_RESID_LS, EPI_RESID_F32):
                kw["resid"] = resid[:M]
            for name, o, m_min in routes:
                if M < m_min:
                    continue
                out = o.linear(a[:M], w, b, epi, split, **kw)
                e = check_linear(out, ref[epi, split][:M], epi, split, K, f"M {M} N {N} K {K} epi {epi} split {int(split)} route {name}")
                worst[epi] = (max(worst[epi][0], e[0]), max(worst[epi][1], e[1]))
    print(f"[small-M linear {N}x{K} split {int(split)}] max err (largest bound) " +
          "  ".join(f"epi{epi} {e:.3e} ({bd:.3e})" for epi, (e, bd) in worst.items()))


@pytest.mark.parametrize("M", [32, 48])
def test_small_m_linear_is_not_transposed(ops, M):
    """The identity probe of test_linear_is_not_transposed on the 32 x 128 kernel (one full row tile; one and a half): catches row / column
    swaps in its C fragment mapping and a wrong wave -> column block assignment."""
    N = K = 256
    w = torch.arange(N * K, dtype=torch.float32).reshape(N, K) / 1024.0
    out = ops.linear(torch.eye(M, K), w, torch.zeros(N), EPI_F16, True).cpu()
    err = (out - w.t()[:M]).abs().max().item()
    print(f"[small-M transposition probe M {M}] max err {err:.3e}")
    assert err < 1e-3


# ------------------------------------------------------------------ b. LayerNorm fused into the split-K reduce (keep_op_linear_ln)
LN_NK = [(1024, 1024), (1024, 4096), (768, 768), (768, 3072)]        # (N, K) of the towers' residual GEMMs: ViT proj / fc2, BERT attention output / FFN output
LN_M_SMALL, LN_M_SLICED, LN_M_BIG = [1, 5, 63, 64, 197, 320], [394, 600], 2100
GEMM_TOL = {EPI_RESID_LS: 3e-5, EPI_RESID_F32: 5e-5}
LN_EPS = {EPI_RESID_LS: 1e-6, EPI_RESID_F32: 1e-12}                 # the towers' own


def ln64(x, g, b, eps):
    return torch.nn.functional.layer_norm(x.double(), (x.shape[1],), g.double(), b.double(), eps)


def plane_bound(y, split):
    """What the fp16 operand planes can hold of an fp32 y: hi + lo to 2^-22 |y|, hi alone to half an ulp, 2^-11 |y| (2^-25: the fp16 subnormal floor)."""
    return (2.0 ** -22 if split else 2.0 ** -11) * y.abs() + 2.0 ** -25


@functools.lru_cache(maxsize=None)
def ln_case(N, K):
    M = LN_M_BIG
    a, w, b, ls, resid = operands(M, N, K, seed=500 + N + K)
    g, bt = 1 + rand(N, seed=900 + N, std=0.1), rand(N, seed=901 + N, std=0.1)
    acc = {False: r16(a) @ r16(w).t() + b.double(), True: a.double() @ w.double().t() + b.double()}
    ref, ref_ln, factor = {}, {}, {}
    for epi in (EPI_RESID_LS, EPI_RESID_F32):
        for sp in (False, True):
            x = epilogue64(acc[sp], epi, ls, resid)
            ref[epi, sp], ref_ln[epi, sp] = x, ln64(x, g, bt, LN_EPS[epi])
            # the LayerNorm scales an error of its input by gamma * rstd: the largest such factor over the reference rows
            factor[epi, sp] = (g.abs().max() * (x.var(1, unbiased=False) + LN_EPS[epi]).rsqrt().max()).item()
    return tuple(t.to(DEV) for t in (a, w, b, ls, resid)) + (g, bt), ref, ref_ln, factor


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("epi", [EPI_RESID_LS, EPI_RESID_F32])
@pytest.mark.parametrize("N,K", LN_NK)
def test_fused_layernorm(ops, N, K, epi, split):
    """gemm_skinny_reduce_ln_kernel behind the small-M kernels (M <= 320) and behind the K-sliced 256 x 256 kernel, both residual epilogues (epi 4:
    the normalised row overwrites the sum), and the stand-alone LayerNorm kernels' blk plane stores (ln_impl 0, 1, 2) behind the plain 256-wide
    kernel on the same small shapes.

    M = 2100: with the default gemm_splitk_tiles = 64 a GEMM of ceil(2100 / 256) * N / 256 = 27 or 36 tiles is still K-sliced (the reduce then does the
    LayerNorm: did_ln = 1, checked as such), so the plain kernel is reached there on a handle with gemm_splitk_tiles = 0, where did_ln must be 0."""
    (a, w, b, ls, resid, g, bt), ref, ref_ln, factor = ln_case(N, K)
    eps, fac = LN_EPS[epi], factor[epi, split]
    assert fac < 2.0, "reference rows must not blow the LayerNorm's gain up (near-constant row?)"
    worst = dict(out=0.0, ln=0.0, ln_bound=0.0, stats=0.0, fused_vs_unfused=0.0)

    def run(o, M, want_did, what):
        out, ln_out, did, ln_hi = o.linear_ln(a[:M], w, b, g, bt, eps, epi, split, ls=ls if epi == EPI_RESID_LS else None, resid=resid[:M], hi=True)
        assert did == want_did, f"{what}: did_ln {did}"
        out, ln_out, ln_hi = out.cpu().double(), ln_out.cpu().double(), ln_hi.cpu().double()
        y_ref = ref_ln[epi, split][:M]
        gemm_part = 5e-6 + GEMM_TOL[epi] * fac
        if epi == EPI_RESID_LS:
            e = (out - ref[epi, split][:M]).abs().max().item()                       # 1. the residual stream, as in (a)
            assert e < GEMM_TOL[epi], f"{what}: out max err {e:.3e}"
            worst["out"] = max(worst["out"], e)
            y_own = ln64(out, g, bt, eps)                                             # 3. the statistics alone: LayerNorm of the row the kernel returned
            e3 = (ln_out - y_own).abs()
            assert (e3 <= 5e-6 + plane_bound(y_own, split)).all(), f"{what}: ln_out vs LayerNorm(out) max err {e3.max():.3e}"
            worst["stats"] = max(worst["stats"], e3.max().item())
        else:
            e = (out - y_ref).abs().max().item()                                      # the fp32 normalised row that replaced the sum
            assert e < gemm_part, f"{what}: fp32 normalised row max err {e:.3e} (bound {gemm_part:.3e})"
            worst["out"] = max(worst["out"], e)
            e3 = (ln_out - out).abs()                                                 # the planes are the split of exactly that row
            assert (e3 <= plane_bound(out, split)).all(), f"{what}: planes vs fp32 row max err {e3.max():.3e}"
            worst["stats"] = max(worst["stats"], e3.max().item())
            y_own = out
        # which plane is which (hi + lo is the same sum with the planes swapped): hi alone is the row to half an fp16 ulp, lo at most half an ulp of hi
        e_hi = (ln_hi - y_own).abs()
        assert (e_hi <= (5e-6 if epi == EPI_RESID_LS else 0.0) + plane_bound(y_own, False)).all(), f"{what}: the hi plane is not the fp16 rounding of the row, max err {e_hi.max():.3e}"
        assert (torch.equal(ln_hi, ln_out) if not split else ((ln_out - ln_hi).abs() <= plane_bound(ln_hi, False)).all()), f"{what}: lo is more than half an ulp of hi"
        e2, b2 = (ln_out - y_ref).abs(), gemm_part + plane_bound(y_ref, split)       # 2. against the LayerNorm of the exact residual
        if not (e2 <= b2).all():
            bad = e2 > b2
            raise AssertionError(f"{what}: ln_out: {int(bad.sum())} elements over the bound, max err {e2.max():.3e}; rows {bad.any(1).nonzero().flatten().tolist()[:8]} "
                                 f"cols {bad.any(0).nonzero().flatten().tolist()[:8]}")
        worst["ln"], worst["ln_bound"] = max(worst["ln"], e2.max().item()), max(worst["ln_bound"], b2.max().item())
        return ln_out, y_own

    fused = {}
    for M in LN_M_SMALL + LN_M_SLICED + [LN_M_BIG]:
        fused[M] = run(ops, M, 1, f"fused M {M} N {N} K {K} epi {epi} split {int(split)}")
    run(big_kernel_handle(), LN_M_BIG, 0, f"plain kernel M {LN_M_BIG} N {N} K {K} epi {epi} split {int(split)}")
    for impl in (0, 1, 2):
        o = big_kernel_handle(ln_impl=impl)
        for M in LN_M_SMALL:
            ln_out, _ = run(o, M, 0, f"unfused ln_impl {impl} M {M} N {N} K {K} epi {epi} split {int(split)}")
            f_out, y_own = fused[M]
            d = (ln_out - f_out).abs()                                                # 4. the two routes agree
            assert (d <= 2 * (5e-6 + plane_bound(y_own, split))).all(), f"fused vs unfused ln_impl {impl} M {M}: max diff {d.max():.3e}"
            worst["fused_vs_unfused"] = max(worst["fused_vs_unfused"], d.max().item())
    print(f"[fused LayerNorm {N}x{K} epi {epi} split {int(split)}] max err: {'resid' if epi == EPI_RESID_LS else 'fp32 row'} {worst['out']:.3e}  "
          f"ln_out vs fp64 {worst['ln']:.3e} (largest bound {worst['ln_bound']:.3e}, gamma * rstd <= {fac:.3f})  "
          f"{'ln_out vs LayerNorm(out)' if epi == EPI_RESID_LS else 'planes vs fp32 row'} {worst['stats']:.3e}  fused vs unfused {worst['fused_vs_unfused']:.3e}")


def test_linear_ln_rejects_bad_arguments(ops):
    lib, s = _lib.load(), _stream(ops.device)
    shapes = dict(a=(1, 1024), w=(1024, 1024), bias=(1024,), ls=(1024,), resid=(1, 1024), g=(1024,), b=(1024,), out=(1, 1024), ln_out=(1, 1024))
    t = {k: torch.zeros(*v, device=DEV) for k, v in shapes.items()}
    did = C.c_int(7)

    def call(M=1, N=1024, K=1024, epi=EPI_RESID_LS, split=0, **null):
        q = {k: (None if k in null else _ptr(v)) for k, v in t.items()}
        return lib.keep_op_linear_ln(ops._h, q["a"], q["w"], q["bias"], q["ls"], q["resid"], q["g"], q["b"], 1e-6, M, N, K, epi, split, q["out"],
                                     q["ln_out"], None, None if "did" in null else C.byref(did), s)                # (ln_hi is optional)
    assert call() == _lib.KEEP_OK and did.value == 1
    for k in ("a", "w", "bias", "ls", "resid", "g", "b", "out", "ln_out", "did"):
        assert call(**{k: None}) == _lib.KEEP_EINVAL, k
    assert call(epi=EPI_RESID_F32, ls=None) == _lib.KEEP_OK                          # ls is the ViT epilogue's only
    for bad in (dict(M=0), dict(M=-1), dict(epi=EPI_F16), dict(epi=EPI_GELU_F16), dict(epi=3), dict(split=2), dict(split=-1)):
        assert call(**bad) == _lib.KEEP_EINVAL, bad
    for bad in (dict(N=512), dict(N=896), dict(K=32), dict(K=1000)):
        assert call(**bad) == _lib.KEEP_EUNSUPPORTED, bad


# ------------------------------------------------------------------ c. short attention: q_rows and the CLS row from the accumulators
ATTN_SHAPES = [(3, 197, 16), (2, 64, 12), (1, 17, 1), (2, 256, 4), (1, 512, 2)]
ATTN_CASES = [(B, T, h, sp) for (B, T, h) in ATTN_SHAPES for sp in (False, True)] + [(2, 257, 3, True), (2, 400, 3, True)]      # the last two: two key windows, merged


@pytest.mark.parametrize("B,T,heads,split", ATTN_CASES)
def test_attention_q_rows(ops, B, T, heads, split):
    """q_rows = 1 (the CLS-only last block) and 3: the computed rows carry the bits of the full run, every other row is untouched (0), on the
    8- and the 4-wave kernels; the full run is the one keep_op_attention gives and sits within the operator's tolerance of fp64."""
    qkv = rand(B * T, 3 * heads * 64, seed=60 + T, std=1.5).to(DEV)
    ref = attn_ref(qkv.cpu(), B, T, heads, None, not split)
    for waves in (8, 4):
        o = handle(attn_waves=waves)
        full = o.attention_cls(qkv, B, T, heads, split)
        assert torch.equal(full, o.attention(qkv, B, T, heads, None, split))
        err = (full.cpu().double() - ref).abs().max().item()
        assert err < (3e-5 if split else 4e-3)
        for q_rows in (1, 3):
            part = o.attention_cls(qkv, B, T, heads, split, q_rows=q_rows).reshape(B, T, -1)
            assert torch.equal(part[:, :q_rows], full.reshape(B, T, -1)[:, :q_rows]), f"attn_waves {waves} q_rows {q_rows}: computed rows differ from the full run"
            assert not part[:, q_rows:].any(), f"attn_waves {waves} q_rows {q_rows}: a row past q_rows was written"
    print(f"[attention q_rows B {B} T {T} heads {heads} split {int(split)}] max err {err:.3e} (full run vs fp64); rows [0, q_rows) bit-identical, the rest 0")


def check_cls(out, cls_out, ref0, B, T, what):
    """cls_out = hi + lo of the accumulator value a whose fp16 rounding is the hi plane of `out` row 0."""
    out0 = out.reshape(B, T, -1)[:, 0].cpu()
    cls_out = cls_out.cpu()
    # the same accumulator: rounded to fp16, cls_out gives the hi plane of out bit for bit.  One exception is arithmetic, not the kernel's: where lo is
    # exactly half an ulp of hi (3.6e-4 of N(0, 1) values split this way), hi + lo is a tie and rounds to even -- to hi's neighbour when hi is odd.
    # There cls_out must sit exactly half an ulp from out: nothing else passes.
    miss = cls_out.half() != out0.half()
    half_ulp = torch.ldexp(torch.ones(()), torch.frexp(out0).exponent - 12).clamp_min(2.0 ** -25)
    assert ((cls_out - out0).abs()[miss] == half_ulp[miss]).all(), f"{what}: fp16(cls_out) != hi plane of out row 0 on {int(miss.sum())} elements that are no ties"
    assert int(miss.sum()) <= max(2, 4e-3 * miss.numel()), f"{what}: {int(miss.sum())} ties of {miss.numel()}"
    c, o0 = cls_out.double(), out0.double()
    e_cls, e_out = (c - ref0).abs(), (o0 - ref0).abs()
    assert (e_cls <= e_out + 2.0 ** -11 * o0.abs() + 2.0 ** -22 * c.abs()).all(), f"{what}: cls_out is further from fp64 than the accumulator can be"
    assert e_cls.max().item() < 4e-3
    return e_cls.max().item(), e_out.max().item(), int(miss.sum())


@pytest.mark.parametrize("B,T,heads", ATTN_SHAPES)
def test_attention_cls_row(B, T, heads):
    """cls_hi + cls_lo (KEEP_ATTN_PROJ_CLS's compact operand) on the 8- and the 4-wave kernels, with and without q_rows."""
    qkv = rand(B * T, 3 * heads * 64, seed=70 + T, std=1.5).to(DEV)
    ref0 = attn_ref(qkv.cpu(), B, T, heads, None, True).reshape(B, T, -1)[:, 0]
    for waves in (8, 4):
        o = handle(attn_waves=waves)
        out, cls_out = o.attention_cls(qkv, B, T, heads, False, cls=True)
        assert torch.equal(out, o.attention_cls(qkv, B, T, heads, False))             # asking for the CLS planes changes nothing else
        e = check_cls(out, cls_out, ref0, B, T, f"attn_waves {waves}")
        out1, cls1 = o.attention_cls(qkv, B, T, heads, False, q_rows=1, cls=True)
        assert torch.equal(cls1, cls_out) and torch.equal(out1.reshape(B, T, -1)[:, 0], out.reshape(B, T, -1)[:, 0])
    print(f"[attention cls_out B {B} T {T} heads {heads}] max err {e[0]:.3e} (fp16 row 0: {e[1]:.3e}; {e[2]} rounding ties)")


def test_attention_cls_row_and_q_rows_against_the_persistent_kernel(ops):
    """33 x 16 (image, head) pairs at 197 tokens: the full run takes the persistent 16-wave kernel (held to bit equality with the 8-wave one by
    test_persistent_attention_is_bit_identical), the q_rows = 1 run cannot -- row 0 of every image still carries the same bits; and the
    persistent kernel's own cls_hi / cls_lo stores."""
    B, T, heads = 33, 197, 16
    qkv = rand(B * T, 3 * heads * 64, seed=24, std=1.5).to(DEV)
    out, cls_out = ops.attention_cls(qkv, B, T, heads, False, cls=True)
    assert torch.equal(out, ops.attention(qkv, B, T, heads, None, False))
    part = ops.attention_cls(qkv, B, T, heads, False, q_rows=1).reshape(B, T, -1)
    assert torch.equal(part[:, 0], out.reshape(B, T, -1)[:, 0])
    assert not part[:, 1:].any()
    ref0 = torch.cat([attn_ref(qkv[b * T:(b + 3) * T].cpu(), min(3, B - b), T, heads, None, True).reshape(-1, T, heads * 64)[:, 0] for b in range(0, B, 3)])
    e = check_cls(out, cls_out, ref0, B, T, "persistent kernel")
    print(f"[attention cls_out persistent B {B}] max err {e[0]:.3e} (fp16 row 0: {e[1]:.3e}; {e[2]} rounding ties)")


def test_attention_cls_rejects_bad_arguments(ops):
    qkv = rand(2 * 64, 3 * 64, seed=1).to(DEV)
    with pytest.raises(ValueError, match="split"):
        ops.attention_cls(qkv, 2, 64, 1, True, cls=True)              # launch_attention refuses the CLS planes in split mode: reported, not worked round
    lib, s = _lib.load(), _stream(ops.device)
    out = torch.zeros(2 * 64, 64, device=DEV)
    assert lib.keep_op_attention_cls(ops._h, _ptr(qkv), 2, 64, 1, 1, 0, _ptr(out), _ptr(out), s) == _lib.KEEP_EUNSUPPORTED
    assert lib.keep_op_attention_cls(ops._h, _ptr(qkv), 2, 64, 1, 0, -1, _ptr(out), None, s) == _lib.KEEP_EINVAL
    assert lib.keep_op_attention_cls(ops._h, None, 2, 64, 1, 0, 0, _ptr(out), None, s) == _lib.KEEP_EINVAL
    assert lib.keep_op_attention_cls(ops._h, _ptr(qkv), 2, 64, 1, 0, 0, None, None, s) == _lib.KEEP_EINVAL
    assert lib.keep_op_attention_cls(ops._h, _ptr(qkv), 0, 64, 1, 0, 0, _ptr(out), None, s) == _lib.KEEP_EINVAL
    with pytest.raises(ValueError):
        ops.attention_cls(rand(600, 192), 1, 600, 1)                  # the short kernels end at 512 tokens
