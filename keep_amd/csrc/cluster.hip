// Tile clustering: spherical k-means on L2-normalised feature rows [N,D] with 1 <= K <= 64 unit centroids.
//
//   cluster_assign      a workgroup owns 64 G tile rows (G = 1, 2 or 4 groups of 64) and all K centroids.  Per group each wave has 16 rows
//                       x NC 16-column tiles on v_mfma_f32_16x16x4_f32, sim_mid_kernel's operand flow (wsi.hip): the centroids staged
//                       through LDS 16 k at a time, the tile rows streamed straight from HBM.  An accumulator is a k-ordered fmaf chain
//                       whose order is fixed by (k / 16, k % 4, k / 4 % 4) alone, so a (row, centroid) score does not depend on N, on the
//                       row's position or on how the tiles are split over calls.  The top-2 is taken on the accumulators: the first
//                       maximum wins.  A row with a non-finite element or one with |x| > 1 is skipped: label -1, best = margin = 0.
//   block_accumulate    the integer sums of the block's rows.  The kept rows are ordered by label in LDS (a counting rank, 64 G entries);
//                       every thread owns the columns tid, tid + 256, ... and walks the ordered rows with an int64 register per column,
//                       so the block issues ONE no-return 64-bit atomic add per (label present in the block, column), 512 contiguous
//                       bytes per wave instruction, instead of one per (row, column).  The rows come back from L2 / Infinity Cache: the
//                       block streamed them a moment ago.  Integer sums: the same words for every G, grid and split over calls.
//   cluster_accumulate  block_accumulate over labels read from memory: the second launch of the two-launch form
//   cluster_update      one workgroup per centroid: S_d 2^-30 in fp64, the norm by a fixed tree, c_d = (float)(s_d / norm)
//   cluster_seed        one wave per row: nearest = max(nearest, x . c), then a packed (ordered value, row) 64-bit atomic min -- an
//                       integer minimum, so the lowest row wins a tie whatever the arrival order
//
// Row indices are int32 (N <= 2^22, checked by the caller); element offsets are int64.
#include "common.h"
#include "../../include/keep_hip.h"

namespace keepk {

typedef unsigned long long cluster_acc_t;
constexpr float CLUSTER_ONE = 1073741824.f;            // 2^30: a multiplication by it is exact in fp32
constexpr int CLUSTER_ROWS_MAX = 64 * CLUSTER_MAX_GROUPS;

__device__ __forceinline__ long long cluster_fixed(float x) { return __float2ll_rn(x * CLUSTER_ONE); }
// true for NaN, +-inf and |x| > 1
__device__ __forceinline__ bool cluster_bad(float x) { return !(fabsf(x) <= 1.0f); }

struct ClusterShared {
    int lab[CLUSTER_ROWS_MAX];                         // the block's labels, -1 for a skipped row or one beyond N
    float best[CLUSTER_ROWS_MAX];
    int order[CLUSTER_ROWS_MAX];                       // the kept rows by (label, row)
    int cnt[CLUSTER_MAX_K];
    cluster_acc_t cos;
    int kept;
};

// The walk over the kept rows in (label, row) order: one int64 register per owned column, flushed with ONE no-return atomic per column
// when the label changes.  Every load is unconditional (a column beyond D is clamped to D - 1 and only its atomic is left out), so the
// compiler issues the 4 NI loads of a step together instead of waiting for each behind a branch.
template <int NI>
__device__ __forceinline__ void cluster_walk(const float* __restrict__ x, int row0, int nk, int D, const ClusterShared& sh,
                                             cluster_acc_t* __restrict__ sums) {
    const int tid = threadIdx.x;
    int col[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) col[i] = min(tid + 256 * i, D - 1);
    const bool last_on = tid + 256 * (NI - 1) < D;     // only the last column group can be partial
    long long acc[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) acc[i] = 0;
    int cur = -1;
    auto flush = [&]() {
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (i < NI - 1 || last_on)
                (void)__hip_atomic_fetch_add(sums + (int64_t)cur * D + col[i], (cluster_acc_t)acc[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    for (int s0 = 0; s0 < nk; s0 += 4) {
        float v[4][NI];
        int lab[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = sh.order[min(s0 + u, nk - 1)];
            lab[u] = s0 + u < nk ? sh.lab[r] : -1;
            const float* xr = x + (int64_t)(row0 + r) * D;
#pragma unroll
            for (int i = 0; i < NI; ++i) v[u][i] = xr[col[i]];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (lab[u] < 0) continue;                  // past the last kept row (the same in every thread)
            if (lab[u] != cur) {
                if (cur >= 0) flush();
                cur = lab[u];
#pragma unroll
                for (int i = 0; i < NI; ++i) acc[i] = 0;
            }
#pragma unroll
            for (int i = 0; i < NI; ++i) acc[i] += cluster_fixed(v[u][i]);
        }
    }
    flush();
}

// sh.lab / sh.best hold rows row0 .. row0 + nrows - 1 (nrows <= 64 G); every thread of the block calls this
__device__ __forceinline__ void block_accumulate(const float* __restrict__ x, int row0, int nrows, int D, int K, ClusterShared& sh,
                                                 cluster_acc_t* __restrict__ sums, cluster_acc_t* __restrict__ counts,
                                                 cluster_acc_t* __restrict__ cos_sum) {
    const int tid = threadIdx.x;
    if (tid < CLUSTER_MAX_K) sh.cnt[tid] = 0;
    if (tid == 0) { sh.cos = 0; sh.kept = 0; }
    __syncthreads();
    if (tid < nrows) {
        const int l = sh.lab[tid];
        if (l >= 0) {
            int rank = 0;
            for (int u = 0; u < nrows; ++u) {
                const int lu = sh.lab[u];
                rank += (lu >= 0 && (lu < l || (lu == l && u < tid))) ? 1 : 0;
            }
            sh.order[rank] = tid;
            atomicAdd(&sh.cnt[l], 1);
            atomicAdd(&sh.cos, (cluster_acc_t)cluster_fixed(sh.best[tid]));
            atomicAdd(&sh.kept, 1);
        }
    }
    __syncthreads();
    const int nk = sh.kept;
    if (nk == 0) return;
    if (tid < K && sh.cnt[tid]) (void)__hip_atomic_fetch_add(counts + tid, (cluster_acc_t)sh.cnt[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid == 0) (void)__hip_atomic_fetch_add(cos_sum, sh.cos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // columns tid + 256 i, i < NI = ceil(D / 256) <= 4: the branch is the same in the whole block
    if (D <= 256) cluster_walk<1>(x, row0, nk, D, sh, sums);
    else if (D <= 512) cluster_walk<2>(x, row0, nk, D, sh, sums);
    else if (D <= 768) cluster_walk<3>(x, row0, nk, D, sh, sums);
    else cluster_walk<4>(x, row0, nk, D, sh, sums);
}

// label / best / margin / skipped / changed may be null (label only when sums is given: the fused launch keeps the labels in LDS);
// sums null: assign alone.  prev may be label (every row is read and written by the same lane).
template <int NC>
__global__ __launch_bounds__(256)
void cluster_assign_kernel(const float* __restrict__ x, const float* __restrict__ cen, int N, int D, int K, int G, int32_t* label,
                           float* __restrict__ best_out, float* __restrict__ margin_out, const int32_t* prev,
                           cluster_acc_t* __restrict__ skipped, cluster_acc_t* __restrict__ changed, cluster_acc_t* __restrict__ sums,
                           cluster_acc_t* __restrict__ counts, cluster_acc_t* __restrict__ cos_sum) {
    __shared__ f32x4 sB[2][4][NC * 16];
    __shared__ ClusterShared sh;
    __shared__ int s_skipped, s_changed;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int row0 = blockIdx.x * 64 * G;              // < N: the grid is ceil(N / (64 G))
    const bool stager = tid < NC * 64;                 // one float4 of one centroid per thread and block of 16 k
    const int bcol = tid >> 2, bq = tid & 3;
    const float* bp = cen + (int64_t)min(bcol, K - 1) * D + bq * 4;
    const int nblk = D >> 4;
    if (tid == 0) { s_skipped = 0; s_changed = 0; }
    for (int g = 0; g < G; ++g) {
        const int row_base = row0 + g * 64 + wave * 16;
        const float* ap = x + (int64_t)min(row_base + j, N - 1) * D + kq * 4;
        f32x4 acc[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        bool bad = false;
        f32x4 a_next = *reinterpret_cast<const f32x4*>(ap), b_next = f32x4{0.f, 0.f, 0.f, 0.f};
        if (stager) b_next = *reinterpret_cast<const f32x4*>(bp);
        __syncthreads();                               // the last reads of the group before, and s_skipped / s_changed
        for (int kb = 0; kb < nblk; ++kb) {
            if (stager) sB[kb & 1][bq][bcol] = b_next;
            const f32x4 a = a_next;
            __syncthreads();
            if (kb + 1 < nblk) {
                a_next = *reinterpret_cast<const f32x4*>(ap + (kb + 1) * 16);
                if (stager) b_next = *reinterpret_cast<const f32x4*>(bp + (kb + 1) * 16);
            }
            bad = bad || cluster_bad(a[0]) || cluster_bad(a[1]) || cluster_bad(a[2]) || cluster_bad(a[3]);
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
        // lane (j, kq) holds rows row_base + kq*4 + r (r = 0..3) at columns c*16 + j
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int lr = kq * 4 + r, row = row_base + lr;
            bool rbad = __shfl(badi, lr) != 0;
            float v1 = -INFINITY, v2 = -INFINITY; int i1 = 0x7fffffff;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const float xv = acc[c][r];
                if (c * 16 + j < K) {
                    if (xv > v1) { v2 = v1; v1 = xv; i1 = c * 16 + j; }
                    else if (xv > v2) v2 = xv;
                }
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {                           // the first maximum wins; the runner-up is the best of the rest
                const float o1 = __shfl_xor(v1, o), o2 = __shfl_xor(v2, o); const int oi = __shfl_xor(i1, o);
                if (o1 > v1 || (o1 == v1 && oi < i1)) { v2 = fmaxf(v1, o2); v1 = o1; i1 = oi; }
                else v2 = fmaxf(v2, o1);
            }
            rbad = rbad || i1 >= K;                                      // every score NaN (a centroid that is): no label to give
            if (j == 0) {
                const bool in = row < N;
                const int lab = (in && !rbad) ? i1 : -1;
                const float b = lab >= 0 ? v1 : 0.f, m = (lab >= 0 && K > 1) ? v1 - v2 : 0.f;
                sh.lab[g * 64 + wave * 16 + lr] = lab;
                sh.best[g * 64 + wave * 16 + lr] = b;
                if (in) {
                    if (rbad) atomicAdd(&s_skipped, 1);
                    if (prev && prev[row] != lab) atomicAdd(&s_changed, 1);
                    if (label) label[row] = lab;
                    if (best_out) best_out[row] = b;
                    if (margin_out) margin_out[row] = m;
                }
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        if (skipped && s_skipped) (void)__hip_atomic_fetch_add(skipped, (cluster_acc_t)s_skipped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (changed && s_changed) (void)__hip_atomic_fetch_add(changed, (cluster_acc_t)s_changed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (sums) block_accumulate(x, row0, min(64 * G, N - row0), D, K, sh, sums, counts, cos_sum);
}

// the second launch of the two-launch form: labels (-1 or 0 .. K - 1; anything else is left out) and best as the assign wrote them
__global__ __launch_bounds__(256)
void cluster_accumulate_kernel(const float* __restrict__ x, const int32_t* __restrict__ label, const float* __restrict__ best, int N, int D,
                               int K, int G, cluster_acc_t* __restrict__ sums, cluster_acc_t* __restrict__ counts,
                               cluster_acc_t* __restrict__ cos_sum) {
    __shared__ ClusterShared sh;
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * 64 * G, nrows = min(64 * G, N - row0);
    if (tid < nrows) {
        const int l = label[row0 + tid];
        sh.lab[tid] = (l >= 0 && l < K) ? l : -1;
        sh.best[tid] = best[row0 + tid];
    }
    block_accumulate(x, row0, nrows, D, K, sh, sums, counts, cos_sum);   // its first barrier orders the writes above
}

// one workgroup per centroid
__global__ __launch_bounds__(256)
void cluster_update_kernel(const int64_t* __restrict__ sums, const int64_t* __restrict__ counts, int D, float* __restrict__ cen,
                           unsigned char* __restrict__ empty) {
    __shared__ double part[256];
    const int k = blockIdx.x, tid = threadIdx.x;
    const int64_t* S = sums + (int64_t)k * D;
    double s[4], q = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        s[i] = (tid + 256 * i < D) ? (double)S[tid + 256 * i] * (1.0 / 1073741824.0) : 0.0;
        q += s[i] * s[i];
    }
    part[tid] = q;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) part[tid] += part[tid + o];
        __syncthreads();
    }
    const double norm = sqrt(part[0]);
    const bool keep = counts[k] == 0 || !(norm > 0.0);
    if (tid == 0 && empty) empty[k] = keep ? 1 : 0;
    if (keep) return;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (tid + 256 * i < D) cen[(int64_t)k * D + tid + 256 * i] = (float)(s[i] / norm);
}

// ascending unsigned order = ascending float order; -0 has been folded into +0 by the caller
__device__ __forceinline__ unsigned cluster_ordered(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// centre: fp32 [D], or row *centre_row of x when centre is null.  first = 0: nearest[r] = max(nearest[r], x_r . c) and the key of the
// smallest nearest; first = 1: nearest is not touched and the key is that of the LARGEST x_r . c.  Skipped rows take no part.
__global__ __launch_bounds__(256)
void cluster_seed_kernel(const float* __restrict__ x, int N, int D, const float* __restrict__ centre, const int64_t* __restrict__ centre_row,
                         int first, float* __restrict__ nearest, cluster_acc_t* __restrict__ key) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nq = D >> 2;                             // float4 per row: at most 256, lane + 64 i
    const float* c = centre;
    if (!c) {
        int64_t cr = *centre_row;
        cr = cr < 0 ? 0 : (cr >= N ? N - 1 : cr);      // an index no earlier step can have written is still a read inside x
        c = x + cr * D;
    }
    f32x4 cv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) cv[i] = (lane + 64 * i < nq) ? reinterpret_cast<const f32x4*>(c)[lane + 64 * i] : f32x4{0.f, 0.f, 0.f, 0.f};
    cluster_acc_t mine = ~(cluster_acc_t)0;
    for (int r = blockIdx.x * 4 + wave; r < N; r += gridDim.x * 4) {
        const f32x4* xr = reinterpret_cast<const f32x4*>(x + (int64_t)r * D);
        float dot = 0.f;
        bool bad = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (lane + 64 * i < nq) {
                const f32x4 a = xr[lane + 64 * i];
                bad = bad || cluster_bad(a[0]) || cluster_bad(a[1]) || cluster_bad(a[2]) || cluster_bad(a[3]);
                dot = fmaf(a[0], cv[i][0], dot); dot = fmaf(a[1], cv[i][1], dot);
                dot = fmaf(a[2], cv[i][2], dot); dot = fmaf(a[3], cv[i][3], dot);
            }
        }
        if (__ballot(bad)) continue;                   // the same in every lane
        dot = wave_sum(dot) + 0.0f;                    // the xor tree gives every lane the same bits; + 0 folds -0 into +0
        if (lane == 0) {
            float v = dot;
            if (!first) {
                v = fmaxf(nearest[r], dot) + 0.0f;
                nearest[r] = v;
            }
            const unsigned o = cluster_ordered(v);
            const cluster_acc_t kk = ((cluster_acc_t)(first ? ~o : o) << 32) | (unsigned)r;
            mine = kk < mine ? kk : mine;
        }
    }
    if (lane == 0 && mine != ~(cluster_acc_t)0) (void)__hip_atomic_fetch_min(key, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void cluster_seed_index_kernel(const cluster_acc_t* __restrict__ key, int64_t* __restrict__ index_out) {
    const cluster_acc_t k = *key;
    *index_out = k == ~(cluster_acc_t)0 ? -1 : (int64_t)(k & 0xffffffffull);
}

}  // namespace keepk
using namespace keepk;

// groups of 64 rows per workgroup.  Any value gives the same words; more groups mean fewer atomics per row (a label present in the
// workgroup's rows costs D of them) and fewer workgroups to spread over the chip.  Measured at N = 100 000, D = 768 (DESIGN.md section
// 23): two groups are the fastest up to K = 16 and for the assign alone, four when K = 64 accumulates (the atomics bound that shape).
static int cluster_groups(int N, int K, bool accumulate) {
    if (N < (1 << 15)) return 1;
    return (N >= (1 << 18) || (accumulate && K > 32)) ? 4 : 2;
}

void launch_cluster_assign(const float* x, int N, int D, const float* cen, int K, int32_t* label, float* best, float* margin, const int32_t* prev,
                           int64_t* skipped, int64_t* changed, int64_t* sums, int64_t* counts, int64_t* cos_sum, int two_launch, hipStream_t s) {
    const int G = cluster_groups(N, K, sums != nullptr), nc = (K + 15) / 16;
    dim3 g((N + 64 * G - 1) / (64 * G)), b(256);
    cluster_acc_t* fs = two_launch ? nullptr : (cluster_acc_t*)sums;
#define KEEP_CLUSTER_LAUNCH(NC) hipLaunchKernelGGL(cluster_assign_kernel<NC>, g, b, 0, s, x, cen, N, D, K, G, label, best, margin, prev, \
                                                   (cluster_acc_t*)skipped, (cluster_acc_t*)changed, fs, (cluster_acc_t*)counts, (cluster_acc_t*)cos_sum)
    if (nc == 1) KEEP_CLUSTER_LAUNCH(1); else if (nc == 2) KEEP_CLUSTER_LAUNCH(2); else if (nc == 3) KEEP_CLUSTER_LAUNCH(3); else KEEP_CLUSTER_LAUNCH(4);
#undef KEEP_CLUSTER_LAUNCH
    if (two_launch && sums)
        hipLaunchKernelGGL(cluster_accumulate_kernel, g, b, 0, s, x, label, best, N, D, K, G, (cluster_acc_t*)sums, (cluster_acc_t*)counts,
                           (cluster_acc_t*)cos_sum);
}

void launch_cluster_update(const int64_t* sums, const int64_t* counts, int K, int D, float* cen, unsigned char* empty, hipStream_t s) {
    hipLaunchKernelGGL(cluster_update_kernel, dim3(K), dim3(256), 0, s, sums, counts, D, cen, empty);
}

void launch_cluster_seed_step(const float* x, int N, int D, const float* centre, const int64_t* centre_row, int first, float* nearest,
                              unsigned char* ws, int64_t* index_out, hipStream_t s) {
    cluster_acc_t* key = (cluster_acc_t*)ws;
    (void)hipMemsetAsync(key, 0xFF, sizeof(cluster_acc_t), s);
    int blocks = (N + 3) / 4;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(cluster_seed_kernel, dim3(blocks), dim3(256), 0, s, x, N, D, centre, centre_row, first, nearest, key);
    hipLaunchKernelGGL(cluster_seed_index_kernel, dim3(1), dim3(1), 0, s, key, index_out);
}
