"""The host model of the MX-fp4 compensation path (tests/mx_reference.py) against brute force, and the input conditions of the GPU tests
(tests/mx_cases.py) -- all on the CPU.  tests/test_mx_gpu.py holds the kernels to this model; what is checked here is that the model says what
quant4.h and common.h define."""
import numpy as np
import pytest

import mx_cases as C
import mx_reference as R


def all_f16(nonneg=False):
    """Every finite fp16 value (both zeros included)."""
    v = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    v = v[np.isfinite(v)]
    return v[~np.signbit(v)] if nonneg else v


# ---------------------------------------------------------------------------------------------- split
def test_split_is_two_ieee_roundings_with_subnormals():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.standard_normal(200000) * np.exp2(rng.integers(-30, 15, 200000)),
                        all_f16().astype(np.float64), all_f16().astype(np.float64) * (1 + 2.0 ** -12), [2.0 ** -25, 3 * 2.0 ** -26, 2.0 ** -26, 65504.0]]).astype(np.float32)
    hi, lo = R.split_f16(x)
    with np.errstate(over="ignore"):
        hi_np = x.astype(np.float16)                                    # numpy's conversion: round to nearest even, subnormals kept
        lo_np = (x.astype(np.float64) - hi_np.astype(np.float64)).astype(np.float32).astype(np.float16)      # x - hi taken exactly, then rounded once
    assert np.array_equal(hi.view(np.uint16), hi_np.view(np.uint16)) and np.array_equal(lo.view(np.uint16), lo_np.view(np.uint16))
    assert (hi == 0)[np.abs(x) <= 2.0 ** -25].all() and (np.abs(hi[np.abs(x) >= 2.0 ** -24]) > 0).all()
    fin = np.isfinite(hi)
    err = np.abs(x.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64))[fin]
    assert (err <= np.maximum(np.abs(x.astype(np.float64))[fin] * 2.0 ** -22, 2.0 ** -25)).all()


# ---------------------------------------------------------------------------------------------- block exponent
def test_block_exponent_is_the_smallest_power_of_two_that_does_not_clip():
    amax = all_f16(nonneg=True).astype(np.float64)
    e = R.block_exponent(amax).astype(np.int64)
    cand = np.arange(1, 255)
    fits = amax[:, None] <= 6.0 * np.exp2(cand[None, :] - 127.0)                      # exact: 6 2^j and every fp16 value are float64 numbers
    brute = np.where(fits.any(axis=1), cand[np.argmax(fits, axis=1)], 254)
    assert np.array_equal(e, np.where(amax == 0, 1, brute))
    assert e[amax == 0] == 1 and e.min() >= 1 and e.max() == 141                      # 65504 / 6 <= 2^14


def test_block_exponent_equals_the_bit_form_of_the_kernel():
    """(bits(amax * (1 / 6f)) + 0x7fffff) >> 23 in fp32, clamped to [1, 254]: the mantissa carry rounds up to a power of two."""
    amax = all_f16(nonneg=True).astype(np.float32)
    prod = amax * (np.float32(1.0) / np.float32(6.0))
    assert prod.dtype == np.float32
    bits = prod.view(np.uint32).astype(np.uint64)
    e = np.clip((bits + 0x007FFFFF) >> 23, 1, 254)
    assert np.array_equal(R.block_exponent(amax), e.astype(np.uint8))


def test_floor_exponent_is_the_mutant_it_claims_to_be():
    amax = all_f16(nonneg=True).astype(np.float64)[1:]
    up, dn = R.block_exponent(amax).astype(int), R.block_exponent(amax, floor=True).astype(int)
    exact = amax / 6.0 == np.exp2(up - 127.0)
    assert np.array_equal(dn, np.where(exact, up, up - 1)) and exact.sum() == 39         # amax = 6 2^j: 30 normal fp16 values, 9 subnormal ones
    assert (amax >= 6.0 * np.exp2(dn - 127.0)).all()


# ---------------------------------------------------------------------------------------------- e2m1
def brute_encode(v, e):
    """argmin over the eight magnitudes; of two equally near ones the even code; the sign bit of v."""
    t = np.abs(v.astype(np.float64)) / np.exp2(e.astype(np.float64) - 127.0)
    d = np.abs(t[..., None] - R.E2M1)                                                  # exact: few-bit numbers
    best = d.min(axis=-1, keepdims=True)
    near = d == best
    even = near & (np.arange(8) % 2 == 0)
    idx = np.where(near.sum(axis=-1) > 1, np.argmax(even, axis=-1), np.argmax(near, axis=-1))
    return (idx | (np.signbit(v) << 3)).astype(np.uint8)


def test_encode_is_nearest_even_with_saturation_for_every_value_and_scale():
    v = all_f16()
    lo = R.block_exponent(np.abs(v).astype(np.float64)).astype(int)
    ties = sat = 0
    for e in range(int(lo.min()) - 2, 142):                # every scale a block holding v can have (amax >= |v|), and two below: saturation (the floor mutant's clipping)
        sel = v[lo - 2 <= e]
        ee = np.full(sel.shape, max(e, 1), dtype=np.uint8)
        got, want = R.encode(sel, ee), brute_encode(sel, ee)
        assert np.array_equal(got, want), e
        t = np.abs(sel.astype(np.float64)) / 2.0 ** (max(e, 1) - 127)
        ties += int(np.isin(t, [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]).sum())
        sat += int((t > 6).sum())
        assert ((got & 7)[t > 6] == 7).all() and ((got & 7)[t <= 0.25] == 0).all()
    assert ties >= 100 and sat >= 1000                     # the sweep did meet both (a tie needs a value of at most three significant bits)
    tie_codes = R.encode(np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -2.5, 7.0, -100.0]), np.uint8(127))
    assert tie_codes.tolist() == [0, 2, 2, 4, 4, 6, 6, 12, 7, 15]


def test_truncation_is_the_mutant_it_claims_to_be():
    v = all_f16()
    e = np.full(v.shape, 127, dtype=np.uint8)
    t = np.abs(v.astype(np.float64))
    want = (np.searchsorted(R.E2M1, np.minimum(t, 6.0), side="right") - 1) | (np.signbit(v) << 3)
    assert np.array_equal(R.encode(v, e, trunc=True), want.astype(np.uint8))


def test_decode_inverts_encode_on_the_grid_and_folds_the_zeros():
    codes = np.arange(16, dtype=np.uint8)
    for e in (1, 100, 127, 141, 254):
        val = R.decode(codes, np.uint8(e))
        assert np.array_equal(np.abs(val), np.tile(R.E2M1, 2) * 2.0 ** (e - 127)) and (np.signbit(val) == (codes >= 8)).all()
        assert np.array_equal(R.encode(val, np.uint8(e)), codes)
    assert R.fold_zero(codes).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 0, 9, 10, 11, 12, 13, 14, 15]


def test_quantize_never_clips_and_uses_the_top_of_the_grid():
    x = C.operand("outlier", 300, 256, seed=3)
    hi, lo = R.split_f16(x)
    for p in (hi, lo):
        codes, e = R.quantize(p)
        back = R.dequantize(codes, e)
        amax = np.abs(R.f64(p)).reshape(300, 8, 32).max(axis=2)
        s = np.exp2(e.astype(np.float64) - 127)
        assert (amax <= 6 * s).all() and (amax[amax > 0] > 3 * s[amax > 0]).all() and (e[amax == 0] == R.ZERO_BLOCK_BYTE).all()
        assert (np.abs(back - R.f64(p)).reshape(300, 8, 32) <= s[:, :, None]).all()         # the widest gap of the grid is 2 s


# ---------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("K", [64, 256, 768])
@pytest.mark.parametrize("rows", [1, 256, 257, 600])
def test_offsets_are_bijections(rows, K):
    Rp, KT = R.pad256(rows), K // 32
    plane, row, kt = np.meshgrid(np.arange(2), np.arange(Rp), np.arange(KT), indexing="ij")
    data = (R.q4_data_off(row, kt, plane, KT)[..., None] + np.arange(16)).ravel()
    assert np.array_equal(np.sort(data), np.arange(R.q4_data_bytes(rows, K)))
    scale = R.q4_scale_off(row, kt, plane, KT).ravel()
    assert np.array_equal(np.sort(scale), np.arange(R.q4_scale_bytes(rows, K)))
    m, k = np.meshgrid(np.arange(Rp), np.arange(K), indexing="ij")
    assert np.array_equal(np.sort(R.blk_off(m, k, KT).ravel()), np.arange(Rp * K))


def test_offsets_at_stated_positions():
    """The layout comment of quant4.h, spelled out at a few places (a bijection alone could still be the wrong one)."""
    KT = 8
    assert R.q4_data_off(0, 0, 0, KT) == 0 and R.q4_data_off(0, 0, 1, KT) == 4096 and R.q4_data_off(1, 0, 0, KT) == 16
    assert R.q4_data_off(0, 1, 0, KT) == 8192 and R.q4_data_off(256, 0, 0, KT) == KT * 8192 and R.q4_data_off(300, 3, 1, KT) == (KT + 3) * 8192 + 4096 + 44 * 16
    # rows r, r + 32, r + 64, r + 96 of a 128-row half are the four bytes of dword (r / 128) * 32 + r % 32
    for r in (0, 5, 31, 128, 140):
        assert [R.q4_scale_off(r + 32 * j, 0, 0, KT) for j in range(4)] == [((r // 128) * 32 + r % 32) * 4 + j for j in range(4)]
    assert R.q4_scale_off(0, 1, 0, KT) == 512 and R.q4_scale_off(0, 0, 1, KT) == 256 and R.q4_scale_off(256 + 33, 2, 1, KT) == (KT + 2) * 512 + 256 + 1 * 4 + 1
    assert R.blk_off(0, 31, KT) == 31 and R.blk_off(1, 0, KT) == 32 and R.blk_off(0, 32, KT) == 8192 and R.blk_off(257, 33, KT) == (KT + 1) * 8192 + 32 + 1


def test_pack_and_unpack_are_inverse():
    rng = np.random.default_rng(5)
    codes = rng.integers(0, 16, size=(2, 512, 128), dtype=np.uint8)
    e = rng.integers(1, 255, size=(2, 512, 4), dtype=np.uint8)
    q, sc = R.pack_device(codes, e)
    c2, e2 = R.unpack_device(q, sc, 300, 128)
    assert np.array_equal(c2, codes) and np.array_equal(e2, e)
    assert q[0] == codes[0, 0, 0] | (codes[0, 0, 1] << 4)              # k 2b in the low nibble of byte b


# ---------------------------------------------------------------------------------------------- the product
def test_emulation_removes_most_of_the_fp16_rounding_and_every_mutant_less():
    """What the correct arithmetic leaves of the fp16 rounding error (tools/precision_study.py: ~3 % of its variance), and what a wrong scale byte
    leaves: on Gaussian operands, whose blocks share 3 or 4 scale bytes, still half of the error goes; with a power of two per row and per block the
    same mistake adds error."""
    left = {}
    for fam in ("gaussian", "scaled"):
        a, w = C.operands(fam, 512, 512, 1024, seed=11)
        exact = a.astype(np.float64) @ w.astype(np.float64).T
        p = R.Product(a, w)
        base = p.fp16_product()
        e16 = R.rms(base - exact)
        left[fam] = {m: R.rms(base + p.correction(2, m) - exact) / e16 for m in (None, "row_scale", "kt_scale")}
    print(left)
    g, s = left["gaussian"], left["scaled"]
    assert 0.15 < g[None] < 0.20 and 0.15 < s[None] < 0.20
    assert g[None] < g["row_scale"] < 0.6 and g[None] < g["kt_scale"] < 0.6           # a test that only asks for "less error than plain fp16" passes this
    assert s["row_scale"] > 1.0 and s["kt_scale"] > 1.0
    assert np.array_equal(R.emulate(a, w, 2), base + p.correction(2)) and np.array_equal(R.correction(a, w, 1), p.term("hi", "lo"))


def test_mutants_are_what_their_names_say():
    a, w = C.operands("scaled", 300, 256, 256, seed=13)
    p = R.Product(a, w)
    t_aw, t_wa = p.term("hi", "lo"), p.term("lo", "hi")
    assert np.array_equal(p.correction(2), t_aw + t_wa) and np.array_equal(p.correction(1), t_aw)
    assert np.array_equal(p.correction(2, "no_aw"), t_wa) and np.array_equal(p.correction(2, "no_wa"), t_aw)
    assert np.array_equal(p.correction(2, "plane_swap"), p.term("lo", "lo") + t_wa) and np.array_equal(p.correction(1, "plane_swap"), p.term("lo", "lo"))
    codes, e = R.quantize(p.planes["a", "hi"])
    r = np.arange(300)
    partner = r - r % 128 + (r % 128 + 32) % 128
    ep = np.where((partner < 300)[:, None], e[np.minimum(partner, 299)], R.ZERO_BLOCK_BYTE)
    assert np.array_equal(p.q4("a", "hi", "row_scale"), R.dequantize(codes, ep.astype(np.uint8)))
    assert np.array_equal(p.q4("a", "hi", "kt_scale"), R.dequantize(codes, np.roll(e, -1, axis=1)))
    assert np.array_equal(p.q4("a", "hi", "nibble_swap")[:, 0::2], p.q4("a", "hi")[:, 1::2])
    assert np.array_equal(p.q4("w", "lo", "row_scale"), p.q4("w", "lo")) and not np.array_equal(p.q4("w", "lo", "row_scale_w"), p.q4("w", "lo"))
    with pytest.raises(AssertionError):
        p.correction(1, "no_wa")


# ---------------------------------------------------------------------------------------------- the inputs of the GPU tests
@pytest.mark.parametrize("split,M,N,K", C.CONSUMER_CASES)
@pytest.mark.parametrize("family", ["scaled", "outlier"])
def test_consumer_inputs_meet_their_conditions(family, split, M, N, K):
    case = C.product_case(family, split, M, N, K)
    case.check_conditions()
    c, d, m = case.nearest_mutant()["all"]
    print(f"[{family} {M}x{N}x{K} split {split}] nearest mutant {m}: {d / c:.3f} of the correction; fp32 accumulation of the emulation: {R.rms(case.f32_noise) / c:.2e}")
    assert R.rms(case.f32_noise) <= 0.1 * C.CONSUMER_GATE * d          # the gate leaves a correct kernel room: fp32 summation noise is far below it


def test_gaussian_inputs_have_almost_constant_scales():
    case = C.product_case("gaussian", 2, 257, 256, 256)
    assert max(C.distinct_scale_bytes(case.a) + C.distinct_scale_bytes(case.w)) <= 5


@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("D,F,M", C.CHAIN_CASES)
def test_chain_inputs_meet_their_conditions(D, F, M, mode):
    case = C.chain_case(D, F, M, mode)
    case.check_conditions()
    assert min(C.distinct_scale_bytes(case.h)) >= C.MIN_SCALE_BYTES and min(C.distinct_scale_bytes(case.g)) >= C.MIN_SCALE_BYTES
    assert min(C.distinct_scale_bytes(case.w1)) >= C.MIN_SCALE_BYTES


# ---------------------------------------------------------------------------------------------- the entry point behind the GPU tests
def test_mx_planes_export_refuses_bad_calls_before_touching_the_device():
    import ctypes as Ct
    from keep_amd import _lib, build
    vp, i64, i32, f32 = Ct.c_void_p, Ct.c_int64, Ct.c_int, Ct.c_float
    # keep_op_mx_planes(h, producer, hi_only, x, w, bias, gamma, beta, eps, M, N, K, sentinel, hi, lo, q, sc, stream)
    assert _lib.SIGNATURES["keep_op_mx_planes"] == (i32, [vp, i32, i32, vp, vp, vp, vp, vp, f32, i64, i64, i64, i32, vp, vp, vp, vp, vp])
    build.build(verbose=False)
    lib = _lib.load()
    for producer, hi_only, M, K in ((0, 0, 1, 64), (1, 1, 5, 768), (2, 0, 257, 256), (7, 0, 1, 64), (0, 0, -1, 64)):
        assert lib.keep_op_mx_planes(None, producer, hi_only, None, None, None, None, None, 1e-6, M, 256, K, 0xFF, None, None, None, None, None) == _lib.KEEP_EINVAL
