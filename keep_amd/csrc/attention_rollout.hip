// Attention rollout, one block's step (Abnar & Zuidema 2020), gfx950.
//
//   A[i][j]   = (1/H) sum_h softmax_j(scale q_{b,h,i} . k_{b,h,j})        the block's head-mean attention, i, j = 0 .. T-1
//   At        = (1 - rho) A + rho I                                       the residual path
//   r_out     = At r_in   (At itself when there is no r_in)               first q_rows rows only when q_rows > 0
//
// Two kernels (and a third for the one-row product), passing At through an fp32 scratch:
//   * rollout_mean_kernel: one workgroup of NW waves per (tile, band of 16 NW query rows) loops over the heads.  Per head the K plane(s) of that head are
//     staged into LDS by LDS-DMA (row-major, 16-byte slots XOR-swizzled on the source address: attention_kernel's K image), the next head's into the
//     other half of a double buffer while this head is computed (attention_long_kernel's one-barrier-per-block scheme), and every wave forms
//     S^T = K Q^T for its 16 queries with mfma_f32_16x16x32_f16 -- attention_kernel's mapping: a lane holds, for ONE query (lane & 15), the scores of
//     keys 16 t + 4 (lane >> 4) + r, so maximum and sum are in-register plus two cross-lane steps.  Split blocks add Q_lo K_hi and Q_hi K_lo.  The
//     probabilities are never written per head: exp2 / sum is added into a second register file of the same shape, the band's head sum.
//   * rollout_product_kernel: At (band) x r_in in exact fp32 on v_mfma_f32_32x32x2_f32, a k-ordered fmaf chain (sgemm_f32.hip's inner loop):
//     64 x 64 outputs per workgroup, both operands through LDS in K chunks of 16, k-major so that the one-float-per-lane operands are
//     conflict-free reads.  Rows of T floats start at any 4-byte address (T = 197), so the global side is dword loads and stores.
//   * rollout_row_kernel: the last block's CLS row, r_out[j] = sum_k At[0][k] r_in[k][j]: 64 columns per workgroup, k split over its four waves
//     (k = w, w + 4, ...: fp32 fmaf), the four partial sums added in wave order.
// Every predicate on the MFMA paths is wave-uniform; no atomics; nothing depends on thread order.
#include "common.h"

namespace keepk {

constexpr int RO_HD = 64;                  // head width
constexpr int RO_MAX_NT = 17;              // key tiles of 16: 272 tokens
// waves per workgroup, 16 query rows each: the 13 query tiles of a 224 x 224 tile are two bands of 7 + 6 (four waves: 4 + 4 + 4 + 1, the last
// workgroup staging every head's K for one wave's rows), the 17 of 257 tokens three of 6 + 6 + 5
__host__ __device__ constexpr int ro_waves(int NT) { return NT <= 4 ? 4 : (NT <= 13 ? 7 : 6); }

typedef const __attribute__((address_space(1))) void* ro_gptr_t;
typedef __attribute__((address_space(3))) void* ro_lptr_t;

// One head's K rows [NT * 16][64] f16 into LDS: slot L (16 bytes) of the image holds columns 8 c .. 8 c + 7 of row L >> 3 with
// c = (L & 7) ^ ((row >> 1) & 7).  Rows >= ntok repeat the last row (finite; their scores are replaced by -inf).
template <int NT>
__device__ __forceinline__ void ro_stage_k(const f16* __restrict__ base, int ntok, int D3, int koff, f16* sK, int tid, int wave) {
    constexpr int THREADS = ro_waves(NT) * 64;
    constexpr int ITEMS = NT * 16 * 8;                     // a multiple of 128
    constexpr int IT = (ITEMS + THREADS - 1) / THREADS;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int L = tid + it * THREADS;
        if (L < ITEMS) {                                   // wave-uniform: ITEMS is a multiple of 64
            const int row = L >> 3, c = (L & 7) ^ ((row >> 1) & 7);
            const int rc = row < ntok ? row : ntok - 1;
            __builtin_amdgcn_global_load_lds((ro_gptr_t)(base + (int64_t)rc * D3 + koff + c * 8),
                                             (ro_lptr_t)(sK + (it * THREADS + wave * 64) * 8), 16, 0, 0);
        }
    }
}

__host__ __device__ constexpr size_t ro_lds_bytes(int NT, bool split) { return (size_t)2 * NT * 16 * RO_HD * 2 * (split ? 2 : 1); }      // two buffers of K hi (+ lo)

// out: [batch][nrows][ntok] fp32, nrows = ntok (every row) or 1 (the CLS row)
template <int NT, bool SPLIT>
__global__ __launch_bounds__(ro_waves(NT) * 64)
void rollout_mean_kernel(const f16* __restrict__ qkv_hi, const f16* __restrict__ qkv_lo, int ntok, int heads, int nrows, float sc2, float residual,
                         float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ro_smem[];
    constexpr int NW = ro_waves(NT), PLANE = NT * 16 * RO_HD, BUF = PLANE * (SPLIT ? 2 : 1);      // f16 elements: one K image; one buffer (hi, lo)
    f16* sBuf = reinterpret_cast<f16*>(ro_smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y;
    const int D = heads * RO_HD, D3 = 3 * D;
    const f16* base_hi = qkv_hi + (int64_t)b * ntok * D3;
    const f16* base_lo = SPLIT ? qkv_lo + (int64_t)b * ntok * D3 : nullptr;
    const int qi = lane & 15, g = lane >> 4;
    const int q0 = (blockIdx.x * NW + wave) * 16;
    const bool active = q0 < nrows;                        // wave-uniform; an idle wave still stages and meets the barriers
    const int q = q0 + qi;
    const unsigned qo = (unsigned)(q < ntok ? q : ntok - 1) * (unsigned)D3 + (unsigned)(g * 8);

    f32x4 acc[NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) acc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto stage = [&](int h, int buf) {
        f16* d = sBuf + buf * BUF;
        ro_stage_k<NT>(base_hi, ntok, D3, D + h * RO_HD, d, tid, wave);
        if (SPLIT) ro_stage_k<NT>(base_lo, ntok, D3, D + h * RO_HD, d + PLANE, tid, wave);
    };
    f16x8 qn[2], qln[2];                                   // the next head's Q fragments, fetched a head ahead like its K
    auto load_q = [&](int h) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            qn[ks] = *reinterpret_cast<const f16x8*>(base_hi + (qo + h * RO_HD + ks * 32));
            if (SPLIT) qln[ks] = *reinterpret_cast<const f16x8*>(base_lo + (qo + h * RO_HD + ks * 32));
        }
    };
    stage(0, 0);
    if (active) load_q(0);
    for (int h = 0; h < heads; ++h) {
        // head h has landed (this wave's DMA and Q loads by vmcnt, the others' DMA by the barrier); nobody reads the other buffer (head h - 1) any more
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        f16x8 qf[2], ql[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) { qf[ks] = qn[ks]; if (SPLIT) ql[ks] = qln[ks]; }
        if (h + 1 < heads) {
            stage(h + 1, (h + 1) & 1);
            if (active) load_q(h + 1);
        }
        if (!active) continue;
        const f16* sK = sBuf + (h & 1) * BUF;
        const f16* sKl = sK + PLANE;
        f32x4 s[NT];
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
            const int row = kt * 16 + qi;
            s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int off = row * RO_HD + (((ks * 4 + g) ^ ((row >> 1) & 7)) << 3);
                const f16x8 kf = *reinterpret_cast<const f16x8*>(sK + off);
                if (SPLIT) {
                    const f16x8 kl = *reinterpret_cast<const f16x8*>(sKl + off);
                    s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl, qf[ks], s[kt], 0, 0, 0);
                    s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, ql[ks], s[kt], 0, 0, 0);
                }
                s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[ks], s[kt], 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[kt][r] = (kt * 16 + g * 4 + r < ntok) ? s[kt][r] * sc2 : -INFINITY;      // log2-domain score; keys past the end: P = 0
                mx = fmaxf(mx, s[kt][r]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));               // finite: key 0 exists
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[kt][r] = __builtin_amdgcn_exp2f(s[kt][r] - mx);
                sum += s[kt][r];
            }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        const float inv = 1.0f / sum;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[kt][r] = fmaf(s[kt][r], inv, acc[kt][r]);
    }
    if (!active || q >= nrows) return;
    const float w = (1.0f - residual) / (float)heads;
    float* __restrict__ o = out + ((int64_t)b * nrows + q) * ntok;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = kt * 16 + g * 4 + r;
            if (k < ntok) o[k] = acc[kt][r] * w + (k == q ? residual : 0.f);
        }
}

// out[b] = a[b] r[b]: all three fp32 [ntok][ntok] row-major per tile
constexpr int RP_T = 64, RP_K = 16, RP_LD = RP_T + 1;
__global__ __launch_bounds__(256)
void rollout_product_kernel(const float* __restrict__ a, const float* __restrict__ r, int ntok, float* __restrict__ out) {
    __shared__ float sA[RP_K * RP_LD];
    __shared__ float sB[RP_K * RP_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.y * RP_T, n0 = blockIdx.x * RP_T;
    const int64_t tile = (int64_t)blockIdx.z * ntok * ntok;
    const float* __restrict__ ab = a + tile;
    const float* __restrict__ rb = r + tile;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const int arow = tid >> 2, ak = (tid & 3) * 4;         // A: 64 rows x 16 k, four k per thread
    const int bk = tid >> 4, bj = (tid & 15) * 4;          // R: 16 k x 64 columns, four columns per thread
    const int fi = lane & 31, fk = lane >> 5;
    float ra[4], rr[4];
    auto fetch = [&](int k0) {                             // outside the matrix: zeros, which add nothing
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int am = m0 + arow, akk = k0 + ak + e;
            ra[e] = (am < ntok && akk < ntok) ? ab[am * ntok + akk] : 0.f;
            const int rk = k0 + bk, rj = n0 + bj + e;
            rr[e] = (rk < ntok && rj < ntok) ? rb[rk * ntok + rj] : 0.f;
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < ntok; k0 += RP_K) {
        __syncthreads();                                   // the previous chunk has been consumed
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sA[(ak + e) * RP_LD + arow] = ra[e];
            sB[bk * RP_LD + bj + e] = rr[e];
        }
        __syncthreads();
        if (k0 + RP_K < ntok) fetch(k0 + RP_K);           // the next chunk's loads fly under this chunk's MFMAs
#pragma unroll
        for (int kk = 0; kk < RP_K; kk += 2) {
            const float fa = sA[(kk + fk) * RP_LD + wm * 32 + fi];
            const float fb = sB[(kk + fk) * RP_LD + wn * 32 + fi];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, fb, acc, 0, 0, 0);
        }
    }
    // D[i][j]: lane holds j = lane & 31, i = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int n = n0 + wn * 32 + fi;
    if (n >= ntok) return;
    float* __restrict__ ob = out + tile;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int m = m0 + wm * 32 + (i & 3) + 8 * (i >> 2) + 4 * fk;
        if (m < ntok) ob[m * ntok + n] = acc[i];
    }
}

// out[b][j] = sum_k a[b][k] r[b][k][j]
__global__ __launch_bounds__(256)
void rollout_row_kernel(const float* __restrict__ a, const float* __restrict__ r, int ntok, float* __restrict__ out) {
    __shared__ float part[4][64];
    const int c = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + c, b = blockIdx.y;
    const float* __restrict__ ab = a + (int64_t)b * ntok;
    const float* __restrict__ rb = r + (int64_t)b * ntok * ntok + j;
    float acc = 0.f;
    if (j < ntok)
        for (int k = w; k < ntok; k += 4) acc = fmaf(ab[k], rb[k * ntok], acc);
    part[w][c] = acc;
    __syncthreads();
    if (w == 0 && j < ntok) out[(int64_t)b * ntok + j] = ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
}

template <int NT, bool SPLIT>
int ro_launch_mean(const f16* qkv_hi, const f16* qkv_lo, int batch, int ntok, int heads, int nrows, float sc2, float residual, float* out, hipStream_t s) {
    constexpr size_t bytes = ro_lds_bytes(NT, SPLIT);
    if (bytes > 65536 && !keep_lds_opt_in(reinterpret_cast<const void*>(&rollout_mean_kernel<NT, SPLIT>), bytes)) return -1;
    constexpr int band = ro_waves(NT) * 16;
    const dim3 grid((nrows + band - 1) / band, batch);
    hipLaunchKernelGGL((rollout_mean_kernel<NT, SPLIT>), grid, dim3(ro_waves(NT) * 64), bytes, s, qkv_hi, qkv_lo, ntok, heads, nrows, sc2, residual, out);
    return 0;
}

}  // namespace keepk

int launch_attention_rollout_step(const f16* qkv_hi, const f16* qkv_lo, int batch, int ntok, int heads, float scale, float residual,
                                  const float* r_in, float* r_out, int q_rows, float* a_tmp, hipStream_t s) {
    using namespace keepk;
    if (!qkv_hi || !r_out || batch < 1 || ntok < 1 || heads < 1 || (q_rows != 0 && q_rows != 1)) return -1;
    if (ntok > ROLLOUT_MAX_TOKENS || batch > 65535) return -1;                     // key tiles in registers; grid y / z
    if (r_in && !a_tmp) return -1;
    if ((int64_t)ntok * 3 * heads * RO_HD >= (1ll << 31)) return -1;               // 32-bit lane offsets into one tile's qkv rows
    const int nrows = q_rows ? 1 : ntok;
    float* mean_out = r_in ? a_tmp : r_out;
    const float sc2 = scale * 1.4426950408889634f;
    const int nt = (ntok + 15) / 16;
    int rc;
    if (qkv_lo) {
        rc = nt <= 4 ? ro_launch_mean<4, true>(qkv_hi, qkv_lo, batch, ntok, heads, nrows, sc2, residual, mean_out, s)
           : nt <= 13 ? ro_launch_mean<13, true>(qkv_hi, qkv_lo, batch, ntok, heads, nrows, sc2, residual, mean_out, s)
                      : ro_launch_mean<RO_MAX_NT, true>(qkv_hi, qkv_lo, batch, ntok, heads, nrows, sc2, residual, mean_out, s);
    } else {
        rc = nt <= 4 ? ro_launch_mean<4, false>(qkv_hi, qkv_lo, batch, ntok, heads, nrows, sc2, residual, mean_out, s)
           : nt <= 13 ? ro_launch_mean<13, false>(qkv_hi, qkv_lo, batch, ntok, heads, nrows, sc2, residual, mean_out, s)
                      : ro_launch_mean<RO_MAX_NT, false>(qkv_hi, qkv_lo, batch, ntok, heads, nrows, sc2, residual, mean_out, s);
    }
    if (rc || !r_in) return rc;
    if (q_rows) {
        hipLaunchKernelGGL(rollout_row_kernel, dim3((ntok + 63) / 64, batch), dim3(256), 0, s, a_tmp, r_in, ntok, r_out);
    } else {
        const int nb = (ntok + RP_T - 1) / RP_T;
        hipLaunchKernelGGL(rollout_product_kernel, dim3(nb, nb, batch), dim3(256), 0, s, a_tmp, r_in, ntok, r_out);
    }
    return 0;
}
