// Feature PCA: the integer moments of unit feature rows [N,D], the scores of rows on k <= 64 components and the
// three-plane colour picture of a class raster.  The eigen-decomposition of the D x D covariance stays on the host in float64.
//
//   pca_sums_kernel<NI>     a workgroup owns PCA_SUM_ROWS rows.  A wave per row decides the skip rule of cluster_assign (a non-finite
//                       element or one with |x| > 1) and writes the row's flag (uint8, the Gram kernel's input); then every thread owns
//                       the columns tid, tid + 256, ... and walks the kept rows with an int64 register per column: sum[d] +=
//                       llrint(x_d 2^30) per term, ONE no-return 64-bit atomic per (workgroup, column).  count += kept, skipped += the rest.
//   pca_gram_kernel<MULTI>  a workgroup owns one pair (I <= J) of 128-column slabs and `groups` consecutive chunks of KEEP_PCA_CHUNK rows.
//                       Per 16 rows both slabs are staged through LDS once, a_i = fp32(x_i - centre) formed while they are staged (a
//                       skipped row, a row past the chunk and a column past D are zero); wave w has the 64 x 64 quadrant (w >> 1, w & 1)
//                       as 4 x 4 accumulators of v_mfma_f32_16x16x4_f32 and K runs over the chunk's rows in row order.  At the end of
//                       a chunk every accumulator is rounded ONCE, llrint(acc 2^32); MULTI sums those integers over the workgroup's
//                       chunks in registers.  One no-return 64-bit atomic per word, only for 16 x 16 tiles with tile row <= tile column.
//   pca_project_kernel<NC>  cluster_assign's operand flow (the components staged through LDS 16 k at a time, the rows streamed from HBM,
//                       a k-ordered fmaf chain per (row, component) whose order is fixed by (k / 16, k % 4, k / 4 % 4) alone); then
//                       fp32(fp32(chain + bias) * scale), each step only when its vector is given.  A skipped row gives a zero row.
//   class_render_rgb_kernel one pixel per thread: channel ch = min(255, (2 255 S + 65535 c) / (2 65535 c)) of plane planes[ch] (the
//                       index keep_heat_render gives the window [0, 65535]), blended as (alpha v + (256 - alpha) under + 128) >> 8.
//
// Fixed points.  sum: |x| <= 1 and at most 2^24 rows into one set of accumulators: |word| <= 2^30 2^24 = 2^54 (cluster.hip's word).
// gram: |x|, |centre| <= 1 give |a| <= 2, so over a chunk of KEEP_PCA_CHUNK = 512 rows |acc| <= 4 x 512 = 2^11 and a chunk adds at most
// 2^11 2^32 = 2^43 to a word; 2^24 rows are 2^15 chunks: |word| <= 2^58.  (For any other KEEP_PCA_CHUNK = c: 4 c 2^32 x 2^24 / c, the same.)
// THE WORDS OF gram DEPEND ON KEEP_PCA_CHUNK and on where the chunk boundaries fall (every call cuts its rows from its row 0); they do
// not depend on the grid, on `groups`, on the order of the calls or on a split of the rows over calls at multiples of the chunk.  sum
// and count do not depend on the split at all.
//
// Row indices are int32 (N <= 2^22, checked by the caller); element offsets are int64.
#include "common.h"
#include "../../include/keep_hip.h"

namespace keepk {

typedef unsigned long long pca_acc_t;
constexpr float PCA_SUM_ONE = 1073741824.f;            // 2^30: a multiplication by it is exact in fp32
constexpr float PCA_GRAM_ONE = 4294967296.f;           // 2^32
constexpr int PCA_SUM_ROWS = 256;                      // rows of a workgroup of pca_sums_kernel
constexpr int PCA_SLAB = 128;                          // columns of a slab
constexpr int PCA_KB = 16;                             // rows staged at a time
// 16 more than the slab: lanes (j, kq) and (j, kq + 1) of a 32-lane half then read banks 16 apart (a ds_read_b32 has 32 banks)
constexpr int PCA_LDS_STRIDE = PCA_SLAB + 16;
static_assert(KEEP_PCA_CHUNK >= 4 && KEEP_PCA_CHUNK <= 4096 && KEEP_PCA_CHUNK % 4 == 0, "KEEP_PCA_CHUNK is a multiple of 4 in 4 .. 4096");

// true for NaN, +-inf and |x| > 1: cluster_assign's rule
__device__ __forceinline__ bool pca_bad(float x) { return !(fabsf(x) <= 1.0f); }

template <int NI>
__global__ __launch_bounds__(256)
void pca_sums_kernel(const float* __restrict__ x, int N, int D, pca_acc_t* __restrict__ sum, pca_acc_t* __restrict__ count,
                     pca_acc_t* __restrict__ skipped, unsigned char* __restrict__ kept_out) {
    __shared__ unsigned char sKept[PCA_SUM_ROWS];
    __shared__ int s_kept;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * PCA_SUM_ROWS, rows = min(PCA_SUM_ROWS, N - row0);
    const int nq = D >> 2;                             // float4 per row: at most 256, lane + 64 i
    if (tid == 0) s_kept = 0;
    __syncthreads();
    int mine = 0;
    for (int r = wave; r < rows; r += 4) {
        const f32x4* xr = reinterpret_cast<const f32x4*>(x + (int64_t)(row0 + r) * D);
        bool bad = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (lane + 64 * i < nq) {
                const f32x4 a = xr[lane + 64 * i];
                bad = bad || pca_bad(a[0]) || pca_bad(a[1]) || pca_bad(a[2]) || pca_bad(a[3]);
            }
        }
        const bool keep = __ballot(bad) == 0;          // the same in every lane
        if (lane == 0) {
            sKept[r] = keep ? 1 : 0;
            if (kept_out) kept_out[row0 + r] = keep ? 1 : 0;
            mine += keep ? 1 : 0;
        }
    }
    if (lane == 0 && mine) atomicAdd(&s_kept, mine);
    __syncthreads();
    const int nk = s_kept;
    if (tid == 0) {
        if (nk) (void)__hip_atomic_fetch_add(count, (pca_acc_t)nk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (skipped && rows - nk) (void)__hip_atomic_fetch_add(skipped, (pca_acc_t)(rows - nk), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (nk == 0) return;                               // the same in the whole block
    // columns tid + 256 i.  Every load is unconditional (a column beyond D is clamped and only its atomic is left out; a row past the
    // block's last repeats it and is not added), so the 4 NI loads of a step are issued together: cluster_walk's form.
    int col[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) col[i] = min(tid + 256 * i, D - 1);
    const bool last_on = tid + 256 * (NI - 1) < D;
    long long acc[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) acc[i] = 0;
    for (int r0 = 0; r0 < rows; r0 += 4) {
        float v[4][NI];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float* xr = x + (int64_t)(row0 + min(r0 + u, rows - 1)) * D;
#pragma unroll
            for (int i = 0; i < NI; ++i) v[u][i] = xr[col[i]];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (r0 + u >= rows || !sKept[r0 + u]) continue;              // the same in every thread; a skipped row may hold anything
#pragma unroll
            for (int i = 0; i < NI; ++i) acc[i] += __float2ll_rn(__fmul_rn(v[u][i], PCA_SUM_ONE));
        }
    }
#pragma unroll
    for (int i = 0; i < NI; ++i)
        if (i < NI - 1 || last_on)
            (void)__hip_atomic_fetch_add(sum + col[i], (pca_acc_t)acc[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (P ngroups) with P = T (T + 1) / 2 slab pairs, T = ceil(D / 128): block b has pair b % P (so the workgroups that read one chunk are
// neighbours in the dispatch order) and the chunks (b / P) groups .. + groups - 1.  Lane (j, kq) of wave (wi, wj): A = a[row k0 + kq][column
// dI + 64 wi + 16 t + j], B = a[row k0 + kq][column dJ + 64 wj + 16 u + j]; register r of accumulator (t, u) is the word
// (dI + 64 wi + 16 t + 4 kq + r, dJ + 64 wj + 16 u + j).  A diagonal pair stages its slab once and reads it as both operands, so its
// 16 x 16 diagonal tiles are symmetric bit for bit (the two products of a word and its mirror commute).
template <bool MULTI>
__global__ __launch_bounds__(256)
void pca_gram_kernel(const float* __restrict__ x, const unsigned char* __restrict__ kept, const float* __restrict__ centre, int N, int D,
                     int T, int n_chunks, int groups, pca_acc_t* __restrict__ gram) {
    __shared__ __attribute__((aligned(16))) float sA[2][PCA_KB][PCA_LDS_STRIDE];
    __shared__ __attribute__((aligned(16))) float sB[2][PCA_KB][PCA_LDS_STRIDE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int P = T * (T + 1) / 2;
    int p = blockIdx.x % P, I = 0;
    const int grp = blockIdx.x / P;
    while (p >= T - I) { p -= T - I; ++I; }
    const int J = I + p;
    const bool diag = I == J;
    const int dI = I * PCA_SLAB, dJ = J * PCA_SLAB;
    const int wi = wave >> 1, wj = wave & 1;
    // staging: float4 e = tid + 256 q (q = 0, 1) of a 16 x 128 block is row e / 32, columns 4 (e % 32) ..; e % 32 is the same for both q
    const int sc = (tid & 31) * 4, sr = tid >> 5;
    const int cI = dI + sc, cJ = dJ + sc;
    const bool onI = cI < D, onJ = cJ < D && !diag;    // D is a multiple of 16: a float4 is inside or outside as a whole
    const float* xI = x + (onI ? cI : 0);
    const float* xJ = x + (onJ ? cJ : 0);
    f32x4 cenI = f32x4{0.f, 0.f, 0.f, 0.f}, cenJ = f32x4{0.f, 0.f, 0.f, 0.f};
    if (centre && onI) cenI = *reinterpret_cast<const f32x4*>(centre + cI);
    if (centre && onJ) cenJ = *reinterpret_cast<const f32x4*>(centre + cJ);
    const float (*rB)[PCA_KB][PCA_LDS_STRIDE] = diag ? sA : sB;
    long long tot[MULTI ? 4 : 1][4][4];
    if (MULTI) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) tot[t][u][r] = 0;
    }
    auto flush = [&](int t, int u, int r, long long v) {
        const int gi = dI + wi * 64 + t * 16, gj = dJ + wj * 64 + u * 16;
        if (gi <= gj && gj < D)                        // tile row <= tile column; gi < D follows
            (void)__hip_atomic_fetch_add(gram + (int64_t)(gi + kq * 4 + r) * D + gj + j, (pca_acc_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    for (int g = 0; g < groups; ++g) {
        const int c = grp * groups + g;
        if (c >= n_chunks) break;                      // the same in the whole block
        const int first = c * KEEP_PCA_CHUNK, rows = min(KEEP_PCA_CHUNK, N - first);
        const int nkb = (rows + PCA_KB - 1) / PCA_KB;
        f32x4 acc[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 nI[2], nJ[2];
        bool on[2];
        auto fetch = [&](int kb) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int row = kb * PCA_KB + sr + 8 * q, gr = first + min(row, rows - 1);
                on[q] = row < rows && kept[gr] != 0;
                nI[q] = *reinterpret_cast<const f32x4*>(xI + (int64_t)gr * D);
                if (!diag) nJ[q] = *reinterpret_cast<const f32x4*>(xJ + (int64_t)gr * D);
            }
        };
        fetch(0);
        __syncthreads();                               // the last reads of the chunk before
        for (int kb = 0; kb < nkb; ++kb) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f}, b = f32x4{0.f, 0.f, 0.f, 0.f};
                if (on[q] && onI) a = f32x4{__fsub_rn(nI[q][0], cenI[0]), __fsub_rn(nI[q][1], cenI[1]), __fsub_rn(nI[q][2], cenI[2]), __fsub_rn(nI[q][3], cenI[3])};
                if (on[q] && onJ) b = f32x4{__fsub_rn(nJ[q][0], cenJ[0]), __fsub_rn(nJ[q][1], cenJ[1]), __fsub_rn(nJ[q][2], cenJ[2]), __fsub_rn(nJ[q][3], cenJ[3])};
                *reinterpret_cast<f32x4*>(&sA[kb & 1][sr + 8 * q][sc]) = a;
                if (!diag) *reinterpret_cast<f32x4*>(&sB[kb & 1][sr + 8 * q][sc]) = b;
            }
            __syncthreads();
            if (kb + 1 < nkb) fetch(kb + 1);
#pragma unroll
            for (int kk = 0; kk < PCA_KB / 4; ++kk) {
                float av[4], bv[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    av[t] = sA[kb & 1][kk * 4 + kq][wi * 64 + t * 16 + j];
                    bv[t] = rB[kb & 1][kk * 4 + kq][wj * 64 + t * 16 + j];
                }
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], bv[u], acc[t][u], 0, 0, 0);
            }
        }
        // one rounding per chunk and word
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long long v = __float2ll_rn(__fmul_rn(acc[t][u][r], PCA_GRAM_ONE));
                    if (MULTI) tot[t][u][r] += v; else flush(t, u, r, v);
                }
    }
    if (MULTI) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) flush(t, u, r, tot[t][u][r]);
    }
}

// out fp32 [N][K]; bias / scale / kept_out / skipped may be null
template <int NC>
__global__ __launch_bounds__(256)
void pca_project_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias, const float* __restrict__ scale,
                        int N, int D, int K, float* __restrict__ out, unsigned char* __restrict__ kept_out, pca_acc_t* __restrict__ skipped) {
    __shared__ f32x4 sB[2][4][NC * 16];
    __shared__ int s_skipped;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const bool stager = tid < NC * 64;                 // one float4 of one component per thread and block of 16 k
    const int bcol = tid >> 2, bq = tid & 3;
    const float* bp = w + (int64_t)min(bcol, K - 1) * D + bq * 4;
    const int nblk = D >> 4;
    if (tid == 0) s_skipped = 0;
    const int row_base = blockIdx.x * 64 + wave * 16;
    const float* ap = x + (int64_t)min(row_base + j, N - 1) * D + kq * 4;
    f32x4 acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    bool bad = false;
    f32x4 a_next = *reinterpret_cast<const f32x4*>(ap), b_next = f32x4{0.f, 0.f, 0.f, 0.f};
    if (stager) b_next = *reinterpret_cast<const f32x4*>(bp);
    __syncthreads();
    for (int kb = 0; kb < nblk; ++kb) {
        if (stager) sB[kb & 1][bq][bcol] = b_next;
        const f32x4 a = a_next;
        __syncthreads();
        if (kb + 1 < nblk) {
            a_next = *reinterpret_cast<const f32x4*>(ap + (kb + 1) * 16);
            if (stager) b_next = *reinterpret_cast<const f32x4*>(bp + (kb + 1) * 16);
        }
        bad = bad || pca_bad(a[0]) || pca_bad(a[1]) || pca_bad(a[2]) || pca_bad(a[3]);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const f32x4 b = sB[kb & 1][kq][c * 16 + j];
            acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], acc[c], 0, 0, 0);
            acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[1], acc[c], 0, 0, 0);
            acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[2], acc[c], 0, 0, 0);
            acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[3], acc[c], 0, 0, 0);
        }
    }
    // lanes (j, 0..3) read row j between them: the row's flag, then known to all four
    int badi = bad ? 1 : 0;
    badi |= __shfl_xor(badi, 16);
    badi |= __shfl_xor(badi, 32);
    float bj[NC], sj[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int col = min(c * 16 + j, K - 1);
        bj[c] = bias ? bias[col] : 0.f;
        sj[c] = scale ? scale[col] : 1.f;
    }
    // lane (j, kq) holds rows row_base + kq*4 + r (r = 0..3) at the components c*16 + j
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int lr = kq * 4 + r, row = row_base + lr;
        const bool rbad = __shfl(badi, lr) != 0;
        if (row >= N) continue;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            float v = acc[c][r];
            if (bias) v = __fadd_rn(v, bj[c]);         // without a bias the chain's own bits, a -0 included
            if (scale) v = __fmul_rn(v, sj[c]);
            if (c * 16 + j < K) out[(int64_t)row * K + c * 16 + j] = rbad ? 0.f : v;
        }
        if (j == 0) {
            if (kept_out) kept_out[row] = rbad ? 0 : 1;
            if (rbad) atomicAdd(&s_skipped, 1);
        }
    }
    __syncthreads();
    if (tid == 0 && skipped && s_skipped) (void)__hip_atomic_fetch_add(skipped, (pca_acc_t)s_skipped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256)
void class_render_rgb_kernel(const pca_acc_t* __restrict__ acc, int h, int w, int p0, int p1, int p2, const unsigned char* __restrict__ thumb,
                             int64_t row_stride, int ps, unsigned bg, const unsigned char* __restrict__ mask, int alpha,
                             unsigned char* __restrict__ out) {
    const int n = h * w;
    const int pl[3] = {p0, p1, p2};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        unsigned under = bg;
        if (thumb) {
            const int y = i / w, xx = i - y * w;
            const unsigned char* p = thumb + (int64_t)y * row_stride + (int64_t)xx * ps;
            under = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
        }
        const bool shown = !mask || mask[i] != 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const pca_acc_t word = acc[(int64_t)pl[ch] * n + i];
            const uint64_t S = word & 0xFFFFFFFFFFull, c = word >> 40;
            unsigned v = (under >> (8 * ch)) & 255u;
            if (shown && c > 0) {
                const uint64_t q = (2 * 255 * S + 65535 * c) / (2 * 65535 * c);          // S < 2^40: the numerator is below 2^50
                const unsigned idx = q > 255 ? 255u : (unsigned)q;
                v = ((unsigned)alpha * idx + (unsigned)(256 - alpha) * v + 128u) >> 8;
            }
            out[(int64_t)i * 3 + ch] = (unsigned char)v;
        }
    }
}

}  // namespace keepk
using namespace keepk;

// chunks a workgroup of the Gram kernel walks when the caller leaves it open.  Any value gives the same words; more chunks mean fewer
// atomics (a workgroup issues 128 x 128 of them whatever it walked) and fewer workgroups to spread over the chip.
static int pca_groups(int n_chunks, int pairs) {
    return (int64_t)n_chunks * pairs >= 8192 ? 4 : 1;
}

void launch_pca_moments(const float* x, int N, int D, const float* centre, int64_t* sum, int64_t* count, int64_t* gram, int64_t* skipped,
                        unsigned char* kept_ws, int groups, hipStream_t s) {
    dim3 g((N + PCA_SUM_ROWS - 1) / PCA_SUM_ROWS), b(256);
#define KEEP_PCA_SUMS(NI) hipLaunchKernelGGL((pca_sums_kernel<NI>), g, b, 0, s, x, N, D, (pca_acc_t*)sum, (pca_acc_t*)count, (pca_acc_t*)skipped, kept_ws)
    if (D <= 256) KEEP_PCA_SUMS(1); else if (D <= 512) KEEP_PCA_SUMS(2); else if (D <= 768) KEEP_PCA_SUMS(3); else KEEP_PCA_SUMS(4);
#undef KEEP_PCA_SUMS
    if (!gram) return;
    const int T = (D + PCA_SLAB - 1) / PCA_SLAB, P = T * (T + 1) / 2;
    const int n_chunks = (N + KEEP_PCA_CHUNK - 1) / KEEP_PCA_CHUNK;
    if (groups <= 0) groups = pca_groups(n_chunks, P);
    if (groups > n_chunks) groups = n_chunks;
    const int ngroups = (n_chunks + groups - 1) / groups;
    dim3 gg((unsigned)((int64_t)P * ngroups));
    if (groups == 1)
        hipLaunchKernelGGL((pca_gram_kernel<false>), gg, b, 0, s, x, kept_ws, centre, N, D, T, n_chunks, groups, (pca_acc_t*)gram);
    else
        hipLaunchKernelGGL((pca_gram_kernel<true>), gg, b, 0, s, x, kept_ws, centre, N, D, T, n_chunks, groups, (pca_acc_t*)gram);
}

void launch_pca_project(const float* x, int N, int D, const float* w, int K, const float* bias, const float* scale, float* out,
                        unsigned char* kept_out, int64_t* skipped, hipStream_t s) {
    dim3 g((N + 63) / 64), b(256);
    const int nc = (K + 15) / 16;
#define KEEP_PCA_PROJECT(NC) hipLaunchKernelGGL((pca_project_kernel<NC>), g, b, 0, s, x, w, bias, scale, N, D, K, out, kept_out, (pca_acc_t*)skipped)
    if (nc == 1) KEEP_PCA_PROJECT(1); else if (nc == 2) KEEP_PCA_PROJECT(2); else if (nc == 3) KEEP_PCA_PROJECT(3); else KEEP_PCA_PROJECT(4);
#undef KEEP_PCA_PROJECT
}

void launch_class_render_rgb(const int64_t* acc, int h, int w, const int* planes, const unsigned char* thumb, int64_t row_stride, int ps,
                             unsigned bg, const unsigned char* mask, int alpha, unsigned char* out, hipStream_t s) {
    const int64_t blocks = ((int64_t)h * w + 255) / 256;
    hipLaunchKernelGGL(class_render_rgb_kernel, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, s, (const pca_acc_t*)acc, h, w,
                       planes[0], planes[1], planes[2], thumb, row_stride, ps, bg, mask, alpha, out);
}
