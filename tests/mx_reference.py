"""Host model of the MX-fp4 compensation path, stated from the definitions of keep_amd/csrc/quant4.h and common.h (numpy, float64 where it adds).

An fp32 operand X is held as two fp16 planes, hi = fp16(X) and lo = fp16(X - hi).  Each plane is cut into blocks of 32 consecutive k of one
row; a block is stored as 32 e2m1 codes (values {0, .5, 1, 1.5, 2, 3, 4, 6} with a sign bit) and one E8M0 byte e, its scale 2^(e - 127) the
smallest power of two s with amax / s <= 6.  The compensated product is

    A W^T  ~  A_hi W_hi^T + Q4(A_hi) Q4(W_lo)^T + Q4(A_lo) Q4(W_hi)^T          (the one-term form keeps the middle term only)

with Q4 = decode(encode(.)).  tests/test_mx_reference.py checks this file against brute force on the CPU; tests/test_mx_gpu.py holds the
kernels to it: the producers bit for bit, the consumer within a fraction of the nearest deliberate mistake (`mutant`)."""
import numpy as np
import torch

E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
ZERO_BLOCK_BYTE = 1                       # the scale byte of an all-zero block: the clamp's lower end

# the deliberate mistakes of emulate(): what a kernel on this path could get wrong while still removing most of the rounding error of well-behaved inputs
MUTANTS_TWO_TERM = ("floor", "trunc", "row_scale", "kt_scale", "row_scale_w", "kt_scale_w", "plane_swap", "no_aw", "no_wa", "nibble_swap")
MUTANTS_ONE_TERM = ("floor", "trunc", "row_scale", "kt_scale", "row_scale_w", "kt_scale_w", "plane_swap", "nibble_swap")
PLUMBING = ("row_scale", "kt_scale", "plane_swap", "no_aw", "no_wa")


def mutants_for(terms):
    return MUTANTS_TWO_TERM if terms == 2 else MUTANTS_ONE_TERM


# ---------------------------------------------------------------------------------------------- planes
def split_f16(x):
    """hi = fp16(x), lo = fp16(x - hi): IEEE round-to-nearest-even, subnormals kept (x - hi is exact in fp32)."""
    x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    hi = x.to(torch.float16)                                # (torch's conversion: the same rounding as numpy's, many times as fast)
    lo = (x - hi.to(torch.float32)).to(torch.float16)
    return hi.numpy(), lo.numpy()


def f64(plane):
    """An fp16 plane as float64 (exact)."""
    return torch.from_numpy(np.ascontiguousarray(plane)).to(torch.float64).numpy()


# ---------------------------------------------------------------------------------------------- the block format
def block_exponent(amax, floor=False):
    """Biased E8M0 byte of a block with largest magnitude `amax` (>= 0, finite): the smallest power of two s = 2^(e - 127) with amax / s <= 6,
    clamped to [1, 254]; an all-zero block gives 1.  floor=True is the mutant: the largest power of two with s <= amax / 6 (the maximum clips)."""
    amax = np.asarray(amax, dtype=np.float64)
    m, ex = np.frexp(amax)                                  # amax = m 2^ex, m in [0.5, 1);  6 s = 0.75 2^(e + 3)
    if floor:
        e = np.where(m >= 0.75, ex - 3, ex - 4)             # 0.75 2^(e+3) <= m 2^ex < 0.75 2^(e+4)
    else:
        e = np.where(m <= 0.75, ex - 3, ex - 2)             # 0.75 2^(e+2) < m 2^ex <= 0.75 2^(e+3)
    b = np.clip(e.astype(np.int64) + 127, 1, 254)
    return np.where(amax == 0, ZERO_BLOCK_BYTE, b).astype(np.uint8)


def _t64(x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64)))


def encode(v, e, trunc=False):
    """e2m1 codes (bit 3 = sign, bits 0..2 = index into E2M1) of v / 2^(e - 127): nearest grid point, ties to the even code, saturating at 6.
    trunc=True is the mutant: towards zero.  v: any float array of fp16 values; e: scale bytes broadcastable to it."""
    v = _t64(v)
    t = v.abs() * torch.exp2(127.0 - _t64(e))               # exact: a power-of-two factor
    grid = torch.from_numpy(E2M1)
    if trunc:
        idx = torch.bucketize(t, grid, right=True) - 1      # grid points <= t
    else:
        mid = (grid[1:] + grid[:-1]) / 2                    # .25 .75 1.25 1.75 2.5 3.5 5
        idx = torch.bucketize(t, mid)                       # midpoints below t: a tie stays on the lower code ...
        tie = t == torch.cat([mid, torch.tensor([float("inf")], dtype=torch.float64)])[idx]
        idx = idx + (tie & (idx % 2 == 1))                  # ... unless that code is odd: ties go to the even one
    idx = idx.clamp(0, 7)
    return (idx | (torch.signbit(v).to(torch.int64) << 3)).to(torch.uint8).numpy()


def decode(code, e):
    code = torch.from_numpy(np.ascontiguousarray(code)).to(torch.int64)
    val = torch.from_numpy(E2M1)[code & 7] * torch.exp2(_t64(e) - 127.0)
    return torch.where((code & 8) != 0, -val, val).numpy()


def fold_zero(code):
    """-0 -> +0: the two codes are the same number."""
    code = np.asarray(code)
    return np.where(code == 8, 0, code).astype(np.uint8)


def quantize(plane, floor=False, trunc=False):
    """One fp16 plane [R][K] -> (codes uint8 [R][K], scale bytes uint8 [R][K / 32])."""
    p = f64(plane) if np.asarray(plane).dtype == np.float16 else np.asarray(plane, dtype=np.float64)
    R, K = p.shape
    b = p.reshape(R, K // 32, 32)
    e = block_exponent(np.abs(b).max(axis=2), floor=floor)
    return encode(b, e[:, :, None], trunc=trunc).reshape(R, K), e


def dequantize(codes, e):
    R, K = codes.shape
    return decode(codes.reshape(R, K // 32, 32), e[:, :, None]).reshape(R, K)


# ---------------------------------------------------------------------------------------------- device layout
def pad256(n):
    return (n + 255) // 256 * 256


def blk_off(m, k, KT):
    """Element offset of X[m][k] in the K-blocked fp16 layout: [row tile of 256][K slice of 32][256 rows][32 k]."""
    return ((m // 256) * KT + k // 32) * 8192 + (m % 256) * 32 + k % 32


def q4_data_off(row, kt, plane, KT):
    """Byte offset of the 16 bytes (32 nibbles, k 2b in the low nibble of byte b) of block (row, kt) of a plane: [row tile][kt][plane][256 rows][16 B]."""
    return ((row // 256) * KT + kt) * 8192 + plane * 4096 + (row % 256) * 16


def q4_scale_off(row, kt, plane, KT):
    """Byte offset of the scale of block (row, kt) of a plane: [row tile][kt][plane][256 B], the 256 bytes permuted so that rows r, r + 32, r + 64,
    r + 96 of a 128-row half share a dword."""
    r = row % 256
    return ((row // 256) * KT + kt) * 512 + plane * 256 + ((r // 128) * 32 + r % 32) * 4 + (r % 128) // 32


def q4_data_bytes(R, K):
    return pad256(R) * K


def q4_scale_bytes(R, K):
    return pad256(R) * (K // 32) * 2


def unpack_device(q, sc, R, K):
    """Raw device bytes -> (codes uint8 [2][Rp][K], scale bytes uint8 [2][Rp][KT]) in logical order, Rp = R padded to 256."""
    q, sc = np.asarray(q, dtype=np.uint8), np.asarray(sc, dtype=np.uint8)
    Rp, KT = pad256(R), K // 32
    assert q.size == q4_data_bytes(R, K) and sc.size == q4_scale_bytes(R, K)
    plane, row, kt = np.meshgrid(np.arange(2), np.arange(Rp), np.arange(KT), indexing="ij")
    e = sc[q4_scale_off(row, kt, plane, KT)]
    by = q[q4_data_off(row, kt, plane, KT)[..., None] + np.arange(16)]               # [2][Rp][KT][16]
    codes = np.stack([by & 15, by >> 4], axis=-1).reshape(2, Rp, K)                    # k = kt * 32 + 2 b + (0: low nibble, 1: high)
    return codes, e


def pack_device(codes, e):
    """The inverse of unpack_device (codes [2][Rp][K], e [2][Rp][KT], Rp % 256 == 0) -> (q, sc)."""
    _, Rp, K = codes.shape
    KT = K // 32
    q = np.zeros(q4_data_bytes(Rp, K), dtype=np.uint8)
    sc = np.zeros(q4_scale_bytes(Rp, K), dtype=np.uint8)
    plane, row, kt = np.meshgrid(np.arange(2), np.arange(Rp), np.arange(KT), indexing="ij")
    sc[q4_scale_off(row, kt, plane, KT)] = e
    c = codes.reshape(2, Rp, KT, 16, 2)
    q[q4_data_off(row, kt, plane, KT)[..., None] + np.arange(16)] = c[..., 0] | (c[..., 1] << 4)
    return q, sc


# ---------------------------------------------------------------------------------------------- the compensated product
def _other_scale_row(e):
    """The scale of the row 32 places on within its 128-row half (the next byte of the scale dword); rows past the operand count as zero blocks."""
    R = e.shape[0]
    p = np.full((pad256(R),) + e.shape[1:], ZERO_BLOCK_BYTE, dtype=np.uint8)
    p[:R] = e
    r = np.arange(R)
    return p[r - r % 128 + (r % 128 + 32) % 128]


_AFFECTS = {"a": ("floor", "trunc", "row_scale", "kt_scale", "nibble_swap"), "w": ("floor", "trunc", "row_scale_w", "kt_scale_w")}


def _q4(quantized, mutant, operand):
    """decode(codes, scales) as float64 [R][K], with the mistakes that live in one operand's addressing (floor / trunc are in `quantized` already)."""
    codes, e = quantized
    if mutant == ("row_scale" if operand == "a" else "row_scale_w"):
        e = _other_scale_row(e)
    if mutant == ("kt_scale" if operand == "a" else "kt_scale_w"):
        e = np.roll(e, -1, axis=1)
    if mutant == "nibble_swap" and operand == "a":          # (swapped in both operands the product would not change)
        R, K = codes.shape
        codes = codes.reshape(R, K // 2, 2)[:, :, ::-1].reshape(R, K)
    return dequantize(codes, e)


class Product:
    """The operands of one product A [M][K] x W [N][K] (fp32) with their planes; quantised planes and partial products are kept, so that a
    mutant only recomputes what it changes."""

    def __init__(self, a, w):
        self.planes = dict(zip((("a", "hi"), ("a", "lo")), split_f16(a)))
        self.planes.update(zip((("w", "hi"), ("w", "lo")), split_f16(w)))
        self._q, self._t = {}, {}

    def share_w(self, other):
        """Take the quantised W planes another product of the same W has already worked out."""
        self._q.update({k: v for k, v in other._q.items() if k[0] == "w"})

    def q4(self, operand, plane, mutant=None):
        key = (operand, plane, mutant if mutant in _AFFECTS[operand] else None)
        if key not in self._q:
            ck = (operand, plane, key[2] if key[2] in ("floor", "trunc") else None, "codes")
            if ck not in self._q:
                self._q[ck] = quantize(self.planes[operand, plane], floor=key[2] == "floor", trunc=key[2] == "trunc")
            self._q[key] = _q4(self._q[ck], key[2], operand)
        return self._q[key]

    def term(self, a_plane, w_plane, mutant=None):
        key = (a_plane, w_plane, mutant if mutant in _AFFECTS["a"] else None, mutant if mutant in _AFFECTS["w"] else None)
        if key not in self._t:
            self._t[key] = self.q4("a", a_plane, mutant) @ self.q4("w", w_plane, mutant).T
        return self._t[key]

    def fp16_product(self):
        return f64(self.planes["a", "hi"]) @ f64(self.planes["w", "hi"]).T

    def correction(self, terms=2, mutant=None):
        """The MX-fp4 part of the compensated product, float64 [M][N]: Q4(A_hi) Q4(W_lo)^T (+ Q4(A_lo) Q4(W_hi)^T with terms == 2)."""
        assert terms in (1, 2) and (mutant is None or mutant in mutants_for(terms)), (terms, mutant)
        out = 0.0
        if mutant != "no_aw":
            out = out + self.term("lo" if mutant == "plane_swap" else "hi", "lo", mutant)
        if terms == 2 and mutant != "no_wa":
            out = out + self.term("lo", "hi", mutant)
        return out

    def emulate_f32_chunked(self, terms=2, chunk=32):
        """The compensated product summed the way a kernel may: one fp32 accumulator, the fp16 pass and then the correction terms added `chunk` k
        at a time -- the accumulation noise to expect of a correct kernel."""
        pairs = [(f64(self.planes["a", "hi"]), f64(self.planes["w", "hi"])), (self.q4("a", "hi"), self.q4("w", "lo"))]
        if terms == 2:
            pairs.append((self.q4("a", "lo"), self.q4("w", "hi")))
        acc = np.zeros((pairs[0][0].shape[0], pairs[0][1].shape[0]), dtype=np.float32)
        for x, y in pairs:
            x, y = x.astype(np.float32), y.astype(np.float32)
            for k0 in range(0, x.shape[1], chunk):
                acc = acc + x[:, k0:k0 + chunk] @ y[:, k0:k0 + chunk].T
        return acc.astype(np.float64)


def correction(a, w, terms=2, mutant=None):
    return Product(a, w).correction(terms, mutant)


def fp16_product(a, w):
    return Product(a, w).fp16_product()


def emulate(a, w, terms=2, mutant=None):
    """The float64 value of the compensated product of fp32 a [M][K] and w [N][K]; `mutant` applies one deliberate mistake."""
    p = Product(a, w)
    return p.fp16_product() + p.correction(terms, mutant)


def rms(x):
    x = np.asarray(x, dtype=np.float64)
    return float(np.sqrt(np.mean(x * x))) if x.size else 0.0


def regions(M, N):
    """The output regions a gate is taken on: everything, every 256 x 256 tile, and the ragged last rows (M % 256 of them) -> [(name, row slice, col slice)]."""
    out = [("all", slice(0, M), slice(0, N))]
    for m0 in range(0, M, 256):
        for n0 in range(0, N, 256):
            out.append((f"tile({m0 // 256},{n0 // 256})", slice(m0, min(m0 + 256, M)), slice(n0, min(n0 + 256, N))))
    if M % 256:
        out.append(("ragged rows", slice(M - M % 256, M), slice(0, N)))
    return out
