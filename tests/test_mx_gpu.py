"""The MX-fp4 compensation path against its host model (tests/mx_reference.py), with operands whose block scales vary.

The older compensated tests (tests/test_ops_gpu.py) ask for less error than the plain fp16 product; on their Gaussian operands a kernel that
reads a neighbouring scale byte still delivers that.  Here the three producers of the fp4 planes (quant_blockify, the LayerNorm kernel, the
GELU epilogue of the 256x256 GEMM) are compared bit for bit with the host encoding, read back through keep_op_mx_planes; the consumer (phase 2
of the 256x256 GEMM) and the LayerNorm -> fc1 -> GELU -> fc2 chain are held to the float64 emulation of the compensated product, two-sided,
within a fraction of the nearest deliberate mistake (`mutant`) the emulation can make.  Operands and their conditions: tests/mx_cases.py."""
import numpy as np
import pytest
import torch

import mx_cases as C
import mx_reference as R
from keep_amd.ops import EPI_F16, EPI_RESID_LS, MX_BLOCKIFY, MX_GELU, MX_LAYERNORM

pytestmark = pytest.mark.gpu

SENTINEL = 0xFF          # as a scale byte outside [1, 254]: nothing a producer writes


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def f16_plane(x):
    """An fp32 tensor of fp16 values, as the op returns a plane -> numpy fp16 (exact, checked)."""
    x = x.cpu()
    h = x.to(torch.float16)
    assert torch.equal(h.to(torch.float32), x), "a plane read back is not made of fp16 values"
    return h.numpy()


def same_numbers(got, want):
    return np.array_equal(got.astype(np.float32), want.astype(np.float32))


def assert_planes_encoded(q, sc, planes, M, Cw, what):
    """Rows < M of the device bytes q / sc hold the host encoding of `planes` (fp16 [M][Cw] each, plane 0 first).  -> (codes, scale bytes) as unpacked."""
    codes, e = R.unpack_device(q.cpu().numpy(), sc.cpu().numpy(), M, Cw)
    want_codes, want_e = C.expected_planes(planes[0], planes[1] if len(planes) > 1 else None)
    for p in range(len(planes)):
        bad_e = np.argwhere(e[p, :M] != want_e[p])
        got = R.fold_zero(codes[p, :M])
        bad_c = np.argwhere(got != want_codes[p])
        if len(bad_e) or len(bad_c):
            v = R.f64(planes[p])
            msg = [f"{what}, plane {p}: {len(bad_e)} of {want_e[p].size} scale bytes and {len(bad_c)} of {got.size} nibbles differ from the host encoding"]
            for r, kt in bad_e[:6]:
                msg.append(f"  scale byte row {r} block {kt}: got {e[p, r, kt]} want {want_e[p, r, kt]} (amax {np.abs(v[r, kt * 32:kt * 32 + 32]).max():.6g})")
            if len(bad_c):
                sub = np.abs(v[bad_c[:, 0], bad_c[:, 1]]) < 2.0 ** -14
                msg.append(f"  {int(sub.sum())} of the differing nibbles encode fp16 subnormals")
            for r, k in bad_c[:6]:
                msg.append(f"  nibble row {r} k {k}: value {v[r, k]:.6g} scale byte {e[p, r, k // 32]}: got {got[r, k]} want {want_codes[p, r, k]}")
            raise AssertionError("\n".join(msg))
    return codes, e


# ---------------------------------------------------------------------------------------------- producers, bit for bit
@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("K", [64, 256, 768])
@pytest.mark.parametrize("M", [1, 255, 257, 600])
def test_blockify_writes_the_host_split_and_encoding(ops, M, K, family):
    x = C.operand(family, M, K, seed=100 + M + K, block_factor=C.pow2(np.random.default_rng(M + K), -4, 4, K // 32))
    if family != "gaussian" and M >= 255:
        assert min(C.distinct_scale_bytes(x)) >= C.MIN_SCALE_BYTES
    hi, lo, q, sc = ops.mx_planes(MX_BLOCKIFY, t(x), sentinel=SENTINEL)
    hi, lo = f16_plane(hi), f16_plane(lo)
    want_hi, want_lo = R.split_f16(x)
    assert same_numbers(hi, want_hi), f"hi plane: {(hi.astype(np.float32) != want_hi.astype(np.float32)).sum()} values differ from fp16(x)"
    bad = np.argwhere(lo.astype(np.float32) != want_lo.astype(np.float32))
    assert len(bad) == 0, (f"lo plane: {len(bad)} values differ from fp16(x - hi), {(np.abs(want_lo[bad[:, 0], bad[:, 1]].astype(np.float32)) < 2.0 ** -14).sum()} of them subnormal; "
                           f"first: x {x[tuple(bad[0])]!r} got {lo[tuple(bad[0])]!r} want {want_lo[tuple(bad[0])]!r}")
    codes, e = assert_planes_encoded(q, sc, [want_hi, want_lo], M, K, f"blockify {family} {M}x{K}")
    # the padding rows are zero blocks: zero nibbles, the clamp's lowest byte
    assert (codes[:, M:] == 0).all() and (e[:, M:] == R.ZERO_BLOCK_BYTE).all()


def layernorm64(x, g, b, eps):
    xd = x.astype(np.float64)
    mu = xd.mean(axis=1, keepdims=True)
    return (xd - mu) / np.sqrt(((xd - mu) ** 2).mean(axis=1, keepdims=True) + eps) * g.astype(np.float64) + b.astype(np.float64)


@pytest.mark.parametrize("hi_only", [False, True], ids=["both_planes", "hi_only"])
@pytest.mark.parametrize("rows", [1, 5, 257, 600])
@pytest.mark.parametrize("D", [768, 1024])
def test_layernorm_encodes_the_planes_it_wrote(ops, D, rows, hi_only):
    x, g, b = C.layernorm_inputs(rows, D, seed=200 + rows + D)
    hi, lo, q, sc = ops.mx_planes(MX_LAYERNORM, t(x), gamma=t(g), beta=t(b), eps=1e-6, hi_only=hi_only, sentinel=SENTINEL)
    planes = [f16_plane(hi)] + ([] if hi_only else [f16_plane(lo)])
    # the planes are the LayerNorm (to fp16 / to 2^-22 with the lo plane; the fp32 kernel itself is tests/test_ops_gpu.py's business)
    ref = layernorm64(x, g, b, 1e-6)
    val = sum(R.f64(p) for p in planes)
    assert (np.abs(val - ref) <= (2.0 ** -11 if hi_only else 2.0 ** -20) * np.abs(ref) + 1e-5).all()
    if rows >= 257:
        assert all(len(np.unique(R.quantize(p)[1])) >= C.MIN_SCALE_BYTES for p in planes)
    codes, e = assert_planes_encoded(q, sc, planes, rows, D, f"layernorm {rows}x{D}" + (" hi only" if hi_only else ""))
    if hi_only:
        assert (codes[1] == (SENTINEL & 15)).all() and (e[1] == SENTINEL).all(), "a one-term producer wrote into the lo plane"


@pytest.mark.parametrize("M,N,K,hi_only", [(257, 512, 256, False), (600, 1024, 512, False), (257, 512, 512, True)])
def test_gelu_epilogue_encodes_the_planes_it_wrote(ops, M, N, K, hi_only):
    a, w, b = C.gelu_inputs(M, N, K, seed=300 + M + N + K)
    hi, lo, q, sc = ops.mx_planes(MX_GELU, t(a), w=t(w), bias=t(b), hi_only=hi_only, sentinel=SENTINEL)
    planes = [f16_plane(hi)] + ([] if hi_only else [f16_plane(lo)])
    ref = C.gelu64(a.astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64))
    # the planes are the GELU of the product: operand rounding (2^-12 of |a| |w| sqrt K per term, less with the corrections) and the fp16 output
    val = sum(R.f64(p) for p in planes)
    assert R.rms(val - ref) <= (2e-3 if hi_only else 5e-4) * R.rms(ref)
    assert all(len(np.unique(R.quantize(p)[1])) >= C.MIN_SCALE_BYTES for p in planes)          # the weight rows' factors reach the output's block scales
    codes, e = assert_planes_encoded(q, sc, planes, M, N, f"gelu epilogue {M}x{N}x{K}" + (" one term" if hi_only else ""))
    if hi_only:
        assert (codes[1] == (SENTINEL & 15)).all() and (e[1] == SENTINEL).all(), "the one-term epilogue wrote into the lo plane"


# ---------------------------------------------------------------------------------------------- consumer, against the emulation
@pytest.mark.parametrize("epi", [EPI_F16, EPI_RESID_LS], ids=["f16", "resid_ls"])
@pytest.mark.parametrize("split,M,N,K", C.CONSUMER_CASES)
@pytest.mark.parametrize("family", C.FAMILIES)
def test_compensated_linear_is_the_emulated_product(ops, family, split, M, N, K, epi):
    """rms(kernel - emulation) <= 1/8 of the nearest mutant's distance, on the whole output, on every 256 x 256 tile and on the ragged rows.  Two-sided:
    a result closer to the exact product than the emulation (an exact split product instead of the fp4 phase) fails as a wrong scale byte does.
    Measured on the MI355X: see DESIGN.md, "What pins the fp4 arithmetic"."""
    case = C.product_case(family, split, M, N, K)
    case.check_conditions()
    rng = np.random.default_rng(7 + M + N + K)
    bias = (0.1 * rng.standard_normal(N)).astype(np.float32)
    ls = (rng.random(N) * 0.45 + 0.05).astype(np.float32) if epi == EPI_RESID_LS else None
    kw = dict(ls=t(ls), resid=torch.zeros(M, N)) if epi == EPI_RESID_LS else {}
    out = ops.linear(t(case.a), t(case.w), t(bias), epi, split, **kw).cpu().double().numpy()
    cw = 1.0 if ls is None else ls.astype(np.float64)[None, :]
    want = cw * (case.emu + bias.astype(np.float64))
    err = out - want
    nearest = case.nearest_mutant(ls)
    c_all, d_all, m_all = nearest["all"]
    print(f"[mx consumer {family} {M}x{N}x{K} split {split} epi {epi}] rms(out - emulation) / rms(correction) = {R.rms(err) / c_all:.3e}  "
          f"(fp32 summation of the emulation on the CPU: {R.rms(case.f32_noise * cw) / c_all:.3e}; nearest mutant {m_all}: {d_all / c_all:.3f})")
    worst = max((R.rms(err[rs, cs]) / nearest[name][1], name) for name, rs, cs in R.regions(M, N))
    print(f"    worst region {worst[1]}: {worst[0]:.3e} of its nearest mutant")
    for name, rs, cs in R.regions(M, N):
        c, d, m = nearest[name]
        assert R.rms(err[rs, cs]) <= C.CONSUMER_GATE * d, f"{name}: {R.rms(err[rs, cs]) / c:.3e} of the correction off the emulation; the nearest mutant ({m}) is {d / c:.3f} off"


# ---------------------------------------------------------------------------------------------- the chain
@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("D,F,M", C.CHAIN_CASES)
def test_mlp_chain_is_the_emulated_chain(ops, D, F, M, mode):
    """LayerNorm -> fc1 + GELU -> fc2 + LayerScale + residual with the planes handed from kernel to kernel (mode 2: both terms, mode 3: Q(X_hi) planes and
    the W_lo term only), against the same chain emulated in float64.  The gate is 1/4 of the nearest plumbing mutant (applied at fc1 or at fc2): the
    epilogue's GELU polynomial (2e-6 absolute) and the fp32 LayerNorm sit between the model and the kernels."""
    case = C.chain_case(D, F, M, mode)
    case.check_conditions()
    out = ops.mlp(t(case.x), t(case.ln_w), t(case.ln_b), t(case.w1), t(case.b1), t(case.w2), t(case.b2), t(case.ls), mode).cpu().double().numpy()
    err = out - case.emu
    nearest = case.nearest_mutant()
    _, c_all, d_all, m_all = nearest["all"]
    print(f"[mx chain D{D} F{F} M{M} mode {mode}] rms(out - emulation) / rms(fc2 correction) = {R.rms(err) / c_all:.3e}  (nearest mutant {m_all}: {d_all / c_all:.3f})")
    for name, (rs, c, d, m) in nearest.items():
        assert R.rms(err[rs]) <= C.CHAIN_GATE * d, f"{name}: {R.rms(err[rs]) / c:.3e} of the fc2 correction off the emulation; the nearest mutant ({m}) is {d / c:.3f} off"
