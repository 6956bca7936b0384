"""Operands and cases of the MX-fp4 tests (tests/test_mx_gpu.py), with the conditions that make them worth running.  Everything here is
host arithmetic on tests/mx_reference.py: tests/test_mx_reference.py runs the conditions where there is no GPU, the GPU tests assert them
again (from the same cache) before they touch the device, so a weak input fails loudly instead of letting a wrong kernel pass.

Families of a product A [M][K] x W [N][K]:
    gaussian   N(0, 1) x N(0, 0.04): what the older compensated tests use; a handful of distinct scale bytes, kept for the printout
    scaled     the same times a power of two per row (2^-6 .. 2^6, both operands) and per 32-k block (2^-4 .. 2^4 on A, its inverse on W:
               the products stay O(1))
    outlier    log-normal row gains (sigma 1.5 octaves: token norms / pre-scaled weight rows), 2 % of the channels at 64x the rest (massive
               residual channels), about 10 % of the 32-blocks of either operand all zero (dead GELU blocks)"""
import functools
import math

import numpy as np
import torch

import mx_reference as R

FAMILIES = ("gaussian", "scaled", "outlier")
MIN_SCALE_BYTES = 8          # distinct E8M0 bytes per plane of a `scaled` / `outlier` operand
MIN_MUTANT = 0.1             # every mutant's rms distance from the emulation, in units of rms(correction), on every region
CONSUMER_GATE = 1.0 / 8      # rms(kernel - emulation) <= this x the nearest mutant's distance
CHAIN_MIN_MUTANT = 0.5       # the MLP chain: every plumbing mutant's distance in units of rms(fc2 correction)
CHAIN_GATE = 1.0 / 4

CONSUMER_CASES = [(2, 257, 256, 256), (2, 600, 512, 512), (2, 300, 768, 1024), (3, 257, 256, 512), (3, 600, 512, 1024)]      # (split, M, N, K)
CHAIN_CASES = [(1024, 4096, 600), (768, 3072, 257)]                                                                        # (D, F, M)


def pow2(rng, lo, hi, n):
    return np.exp2(rng.integers(lo, hi + 1, size=n).astype(np.float64))


def _zero_blocks(rng, x, frac):
    rows, K = x.shape
    keep = rng.random((rows, K // 32)) >= frac
    return x * np.repeat(keep, 32, axis=1)


def operand(family, rows, K, seed, std=1.0, block_factor=None):
    """One fp32 operand [rows][K].  block_factor: the per-32-k-block factors of the `scaled` family (A takes them, W their inverse)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, K)) * std
    if family == "scaled":
        x = x * pow2(rng, -6, 6, rows)[:, None] * np.repeat(block_factor, 32)[None, :]
    elif family == "outlier":
        x = x * np.exp2(rng.standard_normal(rows) * 1.5)[:, None]
        ch = rng.random(K) < 0.02
        ch[rng.integers(0, K)] = True
        x = _zero_blocks(rng, x * np.where(ch, 64.0, 1.0)[None, :], 0.10)
    else:
        assert family == "gaussian", family
    return x.astype(np.float32)


def operands(family, M, N, K, seed):
    f = pow2(np.random.default_rng(seed + 7), -4, 4, K // 32)
    return operand(family, M, K, seed + 1, 1.0, f), operand(family, N, K, seed + 2, 0.04, 1.0 / f)


def distinct_scale_bytes(x):
    """Distinct E8M0 bytes per plane (hi, lo) of an operand."""
    hi, lo = R.split_f16(x)
    return tuple(len(np.unique(R.quantize(p)[1])) for p in (hi, lo))


class ProductCase:
    """A x W^T of one family and shape: the emulation, the correction term, and every mutant's difference from the emulation."""

    def __init__(self, family, terms, M, N, K, seed):
        self.family, self.terms, self.M, self.N, self.K, self.seed = family, terms, M, N, K, seed
        self.a, self.w = operands(family, M, N, K, seed)
        p = R.Product(self.a, self.w)
        self.corr = p.correction(terms)
        self.emu = p.fp16_product() + self.corr
        self.mutant_diff = {m: p.correction(terms, m) - self.corr for m in R.mutants_for(terms)}
        self.f32_noise = p.emulate_f32_chunked(terms) - self.emu

    def nearest_mutant(self, colw=None):
        """Per region: (rms of the correction, the smallest mutant rms distance and its name); colw scales the output columns (LayerScale)."""
        cw = 1.0 if colw is None else np.asarray(colw, dtype=np.float64)[None, :]
        out = {}
        for name, rs, cs in R.regions(self.M, self.N):
            d = {m: R.rms((v * cw)[rs, cs]) for m, v in self.mutant_diff.items()}
            m = min(d, key=d.get)
            out[name] = (R.rms((self.corr * cw)[rs, cs]), d[m], m)
        return out

    def check_conditions(self):
        """The input conditions of a consumer case (host model only)."""
        if self.family != "gaussian":
            for x, what in ((self.a, "A"), (self.w, "W")):
                nb = distinct_scale_bytes(x)
                assert min(nb) >= MIN_SCALE_BYTES, f"{self.family} {what}: {nb} distinct scale bytes in (hi, lo)"
            for region, (c, d, m) in self.nearest_mutant().items():
                assert d >= MIN_MUTANT * c, f"{self.family} {self.M}x{self.N}x{self.K} terms {self.terms}, {region}: mutant {m} is only {d / c:.3f} of the correction away"


@functools.lru_cache(maxsize=None)
def product_case(family, split, M, N, K):
    terms = 2 if split == 2 else 1
    return ProductCase(family, terms, M, N, K, seed=SEEDS.get((family, split, M, N, K), 1000 + M + N + K))


SEEDS = {}                   # (family, split, M, N, K) -> seed, where the default one misses a per-tile condition


# ---------------------------------------------------------------------------------------------- producers
def octave_gains(rng, D, spread=3):
    """LayerNorm gains near 1 times a power of two per 32-channel block (2^-spread .. 2^spread)."""
    return ((1.0 + 0.1 * rng.standard_normal(D)) * np.repeat(pow2(rng, -spread, spread, D // 32), 32)).astype(np.float32)


def layernorm_inputs(rows, D, seed):
    rng = np.random.default_rng(seed)
    x = operand("outlier", rows, D, seed + 1)
    return x, octave_gains(rng, D), (0.05 * rng.standard_normal(D)).astype(np.float32)


def gelu_inputs(M, N, K, seed):
    """Operands of the GELU producer: `scaled` A and W, the weight rows times a power of two per 32 output columns (the consumer-side block scales)."""
    rng = np.random.default_rng(seed)
    a, w = operands("scaled", M, N, K, seed)
    a = (a / np.maximum(np.abs(a).max(axis=1, keepdims=True), 1e-30) * 4.0).astype(np.float32)          # rows of comparable size: the accumulator decides the output's scale
    w = rng.standard_normal((N, K)) * 0.04 / np.repeat(pow2(np.random.default_rng(seed + 7), -4, 4, K // 32), 32)[None, :]
    f = np.repeat(pow2(rng, -8, 3, N // 32), 32)
    return a, (w * f[:, None]).astype(np.float32), (0.1 * rng.standard_normal(N) * f).astype(np.float32)      # (the bias scaled along: it would floor the small columns)


def expected_planes(hi, lo):
    """Host encoding of the fp16 planes hi / lo [M][C] (lo None: plane 0 only) -> (codes [P][M][C] with -0 folded, scale bytes [P][M][C / 32])."""
    planes = [hi] if lo is None else [hi, lo]
    qs = [R.quantize(np.asarray(p, dtype=np.float64)) for p in planes]
    return np.stack([R.fold_zero(c) for c, _ in qs]), np.stack([e for _, e in qs])


# ---------------------------------------------------------------------------------------------- the MLP chain
def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)) / math.sqrt(2.0)).numpy())


class ChainCase:
    """x + ls * fc2(gelu(fc1(LayerNorm(x)))) with compensated fc1 / fc2 (mode 2: both terms, mode 3: the W_lo term), emulated in float64, and the
    plumbing mutants applied at either GEMM."""

    def __init__(self, D, F, M, mode, seed):
        rng = np.random.default_rng(seed)
        self.D, self.F, self.M, self.mode = D, F, M, mode
        self.terms = terms = 2 if mode == 2 else 1
        self.x = operand("outlier", M, D, seed + 1)
        self.ln_w, self.ln_b = octave_gains(rng, D, spread=2), (0.05 * rng.standard_normal(D)).astype(np.float32)
        w1 = rng.standard_normal((F, D)) * 0.025 / np.abs(self.ln_w.astype(np.float64))[None, :]         # (the gains' octaves folded back: fc1's sums stay O(1))
        self.w1 = (w1 * np.repeat(pow2(rng, -2, 2, F // 32), 32)[:, None]).astype(np.float32)          # fc1 rows scaled per 32 hidden units
        self.b1 = (0.02 * rng.standard_normal(F)).astype(np.float32)
        self.w2 = (rng.standard_normal((D, F)) * 0.02).astype(np.float32)
        self.b2 = (0.02 * rng.standard_normal(D)).astype(np.float32)
        self.ls = (rng.random(D) * 0.45 + 0.05).astype(np.float32)
        xd = self.x.astype(np.float64)
        mu = xd.mean(axis=1, keepdims=True)
        var = ((xd - mu) ** 2).mean(axis=1, keepdims=True)
        self.h = ((xd - mu) / np.sqrt(var + 1e-6) * self.ln_w.astype(np.float64) + self.ln_b.astype(np.float64)).astype(np.float32)
        p1 = R.Product(self.h, self.w1)
        self.base1 = p1.fp16_product() + self.b1.astype(np.float64)
        self.g = self._gelu(p1.correction(terms))
        p2 = R.Product(self.g, self.w2)
        self.base2, self.corr2 = p2.fp16_product(), p2.correction(terms)
        lsd = self.ls.astype(np.float64)[None, :]
        self.fc2_corr = lsd * self.corr2
        self.emu = xd + lsd * (self.base2 + self.corr2 + self.b2.astype(np.float64))
        self.mutant_diff = {}
        for m in (m for m in R.PLUMBING if m in R.mutants_for(terms)):
            self.mutant_diff["fc2:" + m] = lsd * (p2.correction(terms, m) - self.corr2)
            pm = R.Product(self._gelu(p1.correction(terms, m)), self.w2)
            pm.share_w(p2)
            self.mutant_diff["fc1:" + m] = lsd * (pm.fp16_product() + pm.correction(terms) - self.base2 - self.corr2)

    def _gelu(self, corr1):
        return gelu64(self.base1 + corr1).astype(np.float32)

    def nearest_mutant(self):
        out = {}
        for name, rs, _ in [("all", slice(0, self.M), None)] + [(f"rows {m0}..", slice(m0, min(m0 + 256, self.M)), None) for m0 in range(0, self.M, 256)]:
            d = {m: R.rms(v[rs]) for m, v in self.mutant_diff.items()}
            m = min(d, key=d.get)
            out[name] = (rs, R.rms(self.fc2_corr[rs]), d[m], m)
        return out

    def check_conditions(self):
        _, c, d, m = self.nearest_mutant()["all"]
        assert d >= CHAIN_MIN_MUTANT * c, f"mlp D{self.D} M{self.M} mode {self.mode}: mutant {m} is only {d / c:.3f} of the fc2 correction away"
        for name, (_, c, d, m) in self.nearest_mutant().items():
            assert d >= 0.5 * CHAIN_MIN_MUTANT * c, f"mlp D{self.D} M{self.M} mode {self.mode}, {name}: mutant {m} is only {d / c:.3f} of the fc2 correction away"


@functools.lru_cache(maxsize=None)
def chain_case(D, F, M, mode):
    return ChainCase(D, F, M, mode, seed=4000 + D + M)
