"""The 256-wide LDS-DMA GEMM (gemm_f16_v2.hip) on the MFMA shape it is built with (KEEP_MFMA_SHAPE), through keep_op_linear / keep_op_linear_ln.

a. An exact mapping test: a one-hot A picks one column of an integer W per output row, so a permuted fragment, accumulator register or epilogue slab
   index is an exact mismatch (torch.equal), not a tolerance miss.
b. Random operands against an fp64 reference, held to the bounds DESIGN.md section 4 states for these epilogues (the ones tests/test_ops_gpu.py and
   tests/test_small_m_gpu.py hold): fp16 outputs 5e-4 |ref| + 2e-5 sqrt(K), LayerScale + residual 3e-5, residual sum 5e-5.
c. The launches that must agree bit for bit: persistent vs one tile per workgroup, 256 x 128 vs 256 x 256 tiles.

Every handle has the small-M kernels and both split-K paths off (skinny_wide = 0, gemm_skinny_m = 0, gemm_splitk_tiles = 0), so every M reaches the 256-wide
kernel; the four routes are gemm_persistent 0 / 1 x proj_impl 0 / 2128.  The launcher takes the persistent kernel only for more tiles than CUs and the
256 x 128 kernel only for more than two tiles per CU, so next to the small sizes one tall case (M = 16 897: 67 row tiles) reaches both."""
import functools
import math

import pytest
import torch

from keep_amd.ops import EPI_F16, EPI_GELU_F16, EPI_RESID_F32, EPI_RESID_LS, Ops
from test_ops_gpu import gelu64, r16, rand

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
M_SWEEP = [255, 256, 257, 513]                 # the row-tail masks on both sides of a tile
N_SWEEP = [128, 256, 768]                      # 128: the 256 x 128 tiles (8 waves of 64 x 64)
K_SWEEP = [32, 96, 256, 384]                   # one step, a ring that never fills, the persistent kernel's minimum, a non-power-of-two
M_TALL = 16897                                 # 67 row tiles: 268 tiles of 256 x 256 (> 256 CUs), 536 of 256 x 128 (> 2 per CU) at N = 1024
ROUTES = [(0, 0), (1, 0), (0, 2128), (1, 2128)]


@functools.lru_cache(maxsize=None)
def route(persistent, proj_impl):
    o = Ops(DEV)
    for k, v in dict(skinny_wide=0, gemm_skinny_m=0, gemm_splitk_tiles=0, gemm_persistent=persistent, proj_impl=proj_impl).items():
        o.set_option(k, v)
    return o


# ------------------------------------------------------------------ a. exact mapping
def mapping_case(M, N, K):
    """A[m, k] = (k == m % K); W: integers in [-1024, 1024], distinct along every row and every column (37 and 101 are coprime to 2049), integer bias
    and residual: out[m, n] = W[n, m % K] + bias[n] (+ resid[m, n]) exactly, in fp16 and in fp32."""
    m, n, k = (torch.arange(x, device=DEV) for x in (M, N, K))
    a = (k[None, :] == (m % K)[:, None]).float()
    w = ((n[:, None] * 37 + k[None, :] * 101) % 2049 - 1024).float()
    bias = (n % 64 - 32).float()
    resid = ((m[:, None] * 7 + n[None, :] * 3) % 257 - 128).float()
    want = w.t()[m % K] + bias[None, :]
    return a, w, bias, resid, want


def check_mapping(M, N, K, routes):
    a, w, bias, resid, want = mapping_case(M, N, K)
    ones = torch.ones(N, device=DEV)
    for pers, impl in routes:
        o = route(pers, impl)
        for split in (False, True):
            what = f"M {M} N {N} K {K} persistent {pers} proj_impl {impl} split {int(split)}"
            out = o.linear(a, w, bias, EPI_F16, split)
            assert torch.equal(out, want), f"EPI_F16 {what}: {int((out != want).sum())} elements differ"
            out = o.linear(a, w, bias, EPI_RESID_LS, split, ls=ones, resid=resid)
            assert torch.equal(out, want + resid), f"EPI_RESID_LS {what}: {int((out != want + resid).sum())} elements differ"


@pytest.mark.parametrize("K", K_SWEEP)
@pytest.mark.parametrize("N", N_SWEEP)
def test_mfma_shape_exact_mapping(N, K):
    for M in M_SWEEP:
        check_mapping(M, N, K, ROUTES)


def test_mfma_shape_exact_mapping_persistent_and_two_per_cu():
    """The tall case: gemm_persistent = 1 walks 268 tiles on one workgroup per CU, proj_impl = 2128 runs the LayerScale + residual product on 256 x 128 tiles."""
    check_mapping(M_TALL, 1024, 256, ROUTES)


def test_mfma_shape_exact_mapping_linear_ln():
    """keep_op_linear_ln: the same product with the LayerNorm behind it offered to the GEMM (here the plain kernel runs, then the LayerNorm kernel)."""
    N, K = 768, 96
    for M in M_SWEEP:
        a, w, bias, resid, want = mapping_case(M, N, K)
        g, b = torch.ones(N, device=DEV), torch.zeros(N, device=DEV)
        for pers, impl in ROUTES:
            out, ln_out, did = route(pers, impl).linear_ln(a, w, bias, g, b, 1e-6, EPI_RESID_LS, False, ls=g, resid=resid)
            assert did == 0
            assert torch.equal(out, want + resid), f"M {M} persistent {pers} proj_impl {impl}"
            ref_ln = torch.nn.functional.layer_norm((want + resid).double(), (N,), eps=1e-6)
            # the fp16 hi plane of the normalised row: half an ulp, 2^-11 |y|, plus the LayerNorm's own fp32 noise
            assert ((ln_out.double() - ref_ln).abs() <= 2.0 ** -11 * ref_ln.abs() + 1e-5).all()


# ------------------------------------------------------------------ b. random operands against fp64
EPILOGUES = [EPI_F16, EPI_GELU_F16, EPI_RESID_LS, EPI_RESID_F32]


@functools.lru_cache(maxsize=None)
def random_case(N, K):
    """activations N(0, 1), weights N(0, 1 / K); the fp64 reference (fp16-rounded operands: the single pass) once at the largest M, rows sliced"""
    M = max(M_SWEEP)
    a, w, b = rand(M, K, seed=700 + N + K), rand(N, K, seed=701 + N + K, std=K ** -0.5), rand(N, seed=702 + N + K, std=0.1)
    ls = torch.rand(N, generator=torch.Generator().manual_seed(703 + N + K)) * 0.45 + 0.05
    resid = rand(M, N, seed=704 + N + K)
    acc = r16(a) @ r16(w).t() + b.double()
    ref = {EPI_F16: acc, EPI_GELU_F16: gelu64(acc), EPI_RESID_LS: resid.double() + ls.double() * acc, EPI_RESID_F32: resid.double() + acc}
    return tuple(t.to(DEV) for t in (a, w, b, ls, resid)), {e: r.to(DEV) for e, r in ref.items()}


def bound(ref, epi, K):
    if epi == EPI_RESID_LS:
        return torch.full_like(ref, 3e-5)
    if epi == EPI_RESID_F32:
        return torch.full_like(ref, 5e-5)
    return 5e-4 * ref.abs() + 2e-5 * math.sqrt(K)


@pytest.mark.parametrize("K", K_SWEEP)
@pytest.mark.parametrize("N", N_SWEEP)
def test_mfma_shape_random_against_fp64(N, K):
    (a, w, b, ls, resid), ref = random_case(N, K)
    worst = {e: 0.0 for e in EPILOGUES}
    for epi in EPILOGUES:
        for M in M_SWEEP:
            kw = {}
            if epi == EPI_RESID_LS:
                kw = dict(ls=ls, resid=resid[:M])
            elif epi == EPI_RESID_F32:
                kw = dict(resid=resid[:M])
            for pers, impl in ROUTES:
                out = route(pers, impl).linear(a[:M], w, b, epi, False, **kw)
                err, bd = (out.double() - ref[epi][:M]).abs(), bound(ref[epi][:M], epi, K)
                worst[epi] = max(worst[epi], (err / bd).max().item())
                bad = err > bd
                assert not bad.any(), (f"M {M} N {N} K {K} epi {epi} persistent {pers} proj_impl {impl}: {int(bad.sum())} elements over the bound, "
                                       f"worst err / bound {(err / bd).max().item():.3f}")
    print(f"[mfma shape {N}x{K}] worst err / bound " + "  ".join(f"epi{e} {v:.3f}" for e, v in worst.items()))


# ------------------------------------------------------------------ c. launches that must agree bit for bit
@pytest.mark.parametrize("M", [513, M_TALL])
def test_mfma_shape_equal_pairs(M):
    """Persistent vs one tile per workgroup (every epilogue the persistent kernel has) and 256 x 128 vs 256 x 256 tiles (LayerScale + residual) on random
    operands: the same K loop on the same shape, so the same bits.  At M = 513 the launcher keeps all four routes on the one-tile 256 x 256 kernel; the tall
    case reaches the persistent and the 256 x 128 kernel."""
    N, K = 1024, 256
    g = torch.Generator(device=DEV).manual_seed(4242 + M)
    a = torch.randn(M, K, device=DEV, generator=g)
    w = torch.randn(N, K, device=DEV, generator=g) * K ** -0.5
    b = torch.randn(N, device=DEV, generator=g) * 0.1
    ls = torch.rand(N, device=DEV, generator=g) * 0.45 + 0.05
    resid = torch.randn(M, N, device=DEV, generator=g)
    for epi, kw in ((EPI_F16, {}), (EPI_GELU_F16, {}), (EPI_RESID_LS, dict(ls=ls, resid=resid))):
        base = route(0, 0).linear(a, w, b, epi, False, **kw)
        assert torch.isfinite(base).all()
        for pers, impl in ROUTES[1:]:
            out = route(pers, impl).linear(a, w, b, epi, False, **kw)
            assert torch.equal(out, base), f"M {M} epi {epi}: persistent {pers} proj_impl {impl} differs in {int((out != base).sum())} elements"
