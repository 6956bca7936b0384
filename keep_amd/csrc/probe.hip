// Linear probe: multinomial logistic regression on unit feature rows [N,D] with 2 <= C <= 64 classes.  One
// pass over the features gives the softmax of every row and, with the gradient on, the integer sums an L-BFGS step on the host needs.
//
//   probe_kernel<NC, GRAD>  a workgroup owns 64 G rows (G = 1, 2 or 4 groups of 64) and all C weight vectors.  The logits are
//                       cluster_assign_kernel's operand flow (cluster.hip): per group each wave has 16 rows x NC 16-column tiles on
//                       v_mfma_f32_16x16x4_f32, the weights staged through LDS 16 k at a time, the rows streamed from HBM; an
//                       accumulator is a k-ordered fmaf chain of a fixed order and the bias is added after it, so a row's logits do
//                       not depend on N, on its position or on the split over calls.  The softmax is fp32 per row: maximum and sum
//                       over the 16 lanes x NC tiles by a fixed __shfl_xor tree; the first maximum is the label.  A row with a
//                       non-finite element or one with |x| > 1 is skipped: label -1, best = margin = 0, a zero row of probabilities.
//                       GRAD: the residual r_ic = w[y_i] (p_ic - [c = y_i]) of the block's rows goes to LDS (zero for a skipped row
//                       and for one with label -1), then probe_walk adds them up.
//   probe_walk<NI, CC>  the gradient of the block's rows, CC classes at a time: every thread owns the columns tid, tid + 256, ... and
//                       walks the rows with CC x NI int64 registers, adding llrint(fp32(r x) 2^30) per term, and issues ONE no-return
//                       64-bit atomic per (block, class, column).  The rows come back from L2 once per chunk of classes: the block
//                       streamed them a moment ago.  Every term is rounded before it is added: the same words for every G, grid and
//                       split over calls.
//   probe_check         the argument check of the gradient launch: a label outside -1 .. C - 1 or a class weight outside (0, 1]
//
// Row indices are int32 (N <= 2^22, checked by the caller); element offsets are int64.
#include "common.h"
#include "../../include/keep_hip.h"

namespace keepk {

typedef unsigned long long probe_acc_t;
constexpr float PROBE_ONE = 1073741824.f;              // 2^30: a multiplication by it is exact in fp32
constexpr float PROBE_LOSS_ONE = 16777216.f;           // 2^24
constexpr int PROBE_RES_FLOATS = PROBE_MAX_GROUP_TILES * 64 * 16;        // 64 G rows x 16 NC classes with G NC <= 8: 32 KB

// true for NaN, +-inf and |x| > 1
__device__ __forceinline__ bool probe_bad(float x) { return !(fabsf(x) <= 1.0f); }
// |v| <= 1: v 2^30 fits an int32 (round half to even, as llrint)
__device__ __forceinline__ int probe_fixed(float v) { return __float2int_rn(__fmul_rn(v, PROBE_ONE)); }

// The walk over the block's kept rows for the classes c0 .. c0 + CC - 1.  Every load is unconditional (a row beyond the block's last is
// clamped to it, a column beyond D to D - 1; only the sums leave those out).  res: [rows][rs] residuals, read as a broadcast.
template <int NI, int CC>
__device__ __forceinline__ void probe_walk(const float* __restrict__ x, int row0, int nrows, int D, int C, int c0, const float* res, int rs,
                                           const unsigned char* keep, probe_acc_t* __restrict__ grad) {
    const int tid = threadIdx.x;
    int col[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) col[i] = min(tid + 256 * i, D - 1);
    const bool last_on = tid + 256 * (NI - 1) < D;     // only the last column group can be partial
    long long acc[CC][NI];
#pragma unroll
    for (int c = 0; c < CC; ++c)
#pragma unroll
        for (int i = 0; i < NI; ++i) acc[c][i] = 0;
    for (int s0 = 0; s0 < nrows; s0 += 4) {
        float v[4][NI];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float* xr = x + (int64_t)(row0 + min(s0 + u, nrows - 1)) * D;
#pragma unroll
            for (int i = 0; i < NI; ++i) v[u][i] = xr[col[i]];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (s0 + u >= nrows || !keep[s0 + u]) continue;              // the same in every thread
            const float* rr = res + (s0 + u) * rs + c0;
#pragma unroll
            for (int c = 0; c < CC; ++c) {
                const float r = rr[c];
#pragma unroll
                for (int i = 0; i < NI; ++i) acc[c][i] += (long long)probe_fixed(__fmul_rn(r, v[u][i]));
            }
        }
    }
#pragma unroll
    for (int c = 0; c < CC; ++c) {
        if (c0 + c >= C) continue;
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (i < NI - 1 || last_on)
                (void)__hip_atomic_fetch_add(grad + (int64_t)(c0 + c) * D + col[i], (probe_acc_t)acc[c][i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <int NI>
__device__ __forceinline__ void probe_walk_classes(const float* __restrict__ x, int row0, int nrows, int D, int C, const float* res, int rs,
                                                   const unsigned char* keep, probe_acc_t* __restrict__ grad) {
    // the chunk: 2 or 4 classes when that is all of them, otherwise 8; res rows are padded with zeros up to a multiple of 16 classes
    if (C <= 2) probe_walk<NI, 2>(x, row0, nrows, D, C, 0, res, rs, keep, grad);
    else if (C <= 4) probe_walk<NI, 4>(x, row0, nrows, D, C, 0, res, rs, keep, grad);
    else
        for (int c0 = 0; c0 < C; c0 += 8) probe_walk<NI, 8>(x, row0, nrows, D, C, c0, res, rs, keep, grad);
}

// probs / label / best / margin / skipped may be null.  GRAD: y int32 [N] (-1 .. C - 1; anything else counts as -1), cw fp32 [C] or null
// (every weight 1), and the accumulators, all of them.  G NC <= PROBE_MAX_GROUP_TILES when GRAD (the residuals' LDS).
template <int NC, bool GRAD>
__global__ __launch_bounds__(256)
void probe_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias, int N, int D, int C, int G,
                  const int32_t* __restrict__ y, const float* __restrict__ cw, float* __restrict__ probs, int32_t* __restrict__ label,
                  float* __restrict__ best_out, float* __restrict__ margin_out, probe_acc_t* __restrict__ skipped,
                  probe_acc_t* __restrict__ grad, probe_acc_t* __restrict__ gbias, probe_acc_t* __restrict__ loss,
                  probe_acc_t* __restrict__ counts) {
    __shared__ f32x4 sB[2][4][NC * 16];
    __shared__ float sRes[GRAD ? PROBE_RES_FLOATS : 1];
    __shared__ unsigned char sKeep[GRAD ? 64 * PROBE_MAX_GROUPS : 1];
    __shared__ int sCnt[GRAD ? PROBE_MAX_C : 1];
    __shared__ probe_acc_t s_loss;
    __shared__ int s_skipped, s_kept;
    constexpr int RS = NC * 16;                        // floats per row of sRes
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int row0 = blockIdx.x * 64 * G;              // < N: the grid is ceil(N / (64 G))
    const bool stager = tid < NC * 64;                 // one float4 of one weight vector per thread and block of 16 k
    const int bcol = tid >> 2, bq = tid & 3;
    const float* bp = w + (int64_t)min(bcol, C - 1) * D + bq * 4;
    const int nblk = D >> 4;
    if (tid == 0) { s_skipped = 0; s_kept = 0; s_loss = 0; }
    if (GRAD && tid < PROBE_MAX_C) sCnt[tid] = 0;
    float bj[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) bj[c] = bias[min(c * 16 + j, C - 1)];
    for (int g = 0; g < G; ++g) {
        const int row_base = row0 + g * 64 + wave * 16;
        const float* ap = x + (int64_t)min(row_base + j, N - 1) * D + kq * 4;
        f32x4 acc[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        bool bad = false;
        f32x4 a_next = *reinterpret_cast<const f32x4*>(ap), b_next = f32x4{0.f, 0.f, 0.f, 0.f};
        if (stager) b_next = *reinterpret_cast<const f32x4*>(bp);
        __syncthreads();                               // the last reads of the group before, and the shared counters
        for (int kb = 0; kb < nblk; ++kb) {
            if (stager) sB[kb & 1][bq][bcol] = b_next;
            const f32x4 a = a_next;
            __syncthreads();
            if (kb + 1 < nblk) {
                a_next = *reinterpret_cast<const f32x4*>(ap + (kb + 1) * 16);
                if (stager) b_next = *reinterpret_cast<const f32x4*>(bp + (kb + 1) * 16);
            }
            bad = bad || probe_bad(a[0]) || probe_bad(a[1]) || probe_bad(a[2]) || probe_bad(a[3]);
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
            const int lr = kq * 4 + r, row = row_base + lr, brow = g * 64 + wave * 16 + lr;
            bool rbad = __shfl(badi, lr) != 0;
            float z[NC];
            float v1 = -INFINITY, v2 = -INFINITY; int i1 = 0x7fffffff;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                z[c] = __fadd_rn(acc[c][r], bj[c]);                      // the bias comes after the chain
                if (c * 16 + j < C) {
                    if (z[c] > v1) { v2 = v1; v1 = z[c]; i1 = c * 16 + j; }
                    else if (z[c] > v2) v2 = z[c];
                }
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {                           // the first maximum wins; the runner-up is the best of the rest
                const float o1 = __shfl_xor(v1, o), o2 = __shfl_xor(v2, o); const int oi = __shfl_xor(i1, o);
                if (o1 > v1 || (o1 == v1 && oi < i1)) { v2 = fmaxf(v1, o2); v1 = o1; i1 = oi; }
                else v2 = fmaxf(v2, o1);
            }
            rbad = rbad || i1 >= C || !(fabsf(v1) < INFINITY);           // a NaN or infinite logit (a weight that is): nothing to give
            const float m = rbad ? 0.f : v1;
            float e[NC], s = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                e[c] = (c * 16 + j < C) ? expf(__fsub_rn(z[c], m)) : 0.f;
                s = __fadd_rn(s, e[c]);                                  // tiles in order, then the lanes by the xor tree
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) s = __fadd_rn(s, __shfl_xor(s, o));
            const bool in = row < N;
            const bool ok = in && !rbad;
            float p[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) p[c] = ok ? __fdiv_rn(e[c], s) : 0.f;
            if (probs && in) {
#pragma unroll
                for (int c = 0; c < NC; ++c)
                    if (c * 16 + j < C) probs[(int64_t)row * C + c * 16 + j] = p[c];
            }
            if (j == 0 && in) {
                if (rbad) atomicAdd(&s_skipped, 1);
                if (label) label[row] = ok ? i1 : -1;
                if (best_out) best_out[row] = ok ? __fdiv_rn(1.0f, s) : 0.f;             // exp(0) / s: the winner's own element of probs
                if (margin_out) margin_out[row] = ok ? __fsub_rn(__fdiv_rn(1.0f, s), __fdiv_rn(expf(__fsub_rn(v2, m)), s)) : 0.f;
            }
            if (GRAD) {
                int yi = in ? y[row] : -1;
                if (yi < -1 || yi >= C) yi = -1;                         // the check launch has refused these; never an index
                const bool kept = ok && yi >= 0;
                const float wy = kept ? (cw ? cw[yi] : 1.0f) : 0.f;
                // z[y] lives in lane (y % 16), tile y / 16 of the row's 16 lanes
                float zy = 0.f;
#pragma unroll
                for (int c = 0; c < NC; ++c) zy = (c == (yi >> 4)) ? z[c] : zy;
                zy = __shfl(zy, (lane & 48) | (yi & 15));
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const float d = __fsub_rn(p[c], (c * 16 + j == yi) ? 1.0f : 0.f);    // the subtraction first, then the weight
                    sRes[brow * RS + c * 16 + j] = (kept && c * 16 + j < C) ? __fmul_rn(wy, d) : 0.f;
                }
                if (j == 0) {
                    sKeep[brow] = kept ? 1 : 0;
                    if (kept) {
                        const float li = __fsub_rn(__fadd_rn(m, logf(s)), zy);           // logsumexp(z) - z[y]
                        atomicAdd(&s_loss, (probe_acc_t)__float2ll_rn(__fmul_rn(__fmul_rn(wy, li), PROBE_LOSS_ONE)));
                        atomicAdd(&sCnt[yi], 1);
                        atomicAdd(&s_kept, 1);
                    }
                }
            }
        }
    }
    __syncthreads();
    if (tid == 0 && skipped && s_skipped) (void)__hip_atomic_fetch_add(skipped, (probe_acc_t)s_skipped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (GRAD) {
        if (s_kept == 0) return;                       // the same in the whole block
        const int nrows = min(64 * G, N - row0);
        if (tid == 0) (void)__hip_atomic_fetch_add(loss, s_loss, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid < C) {
            if (sCnt[tid]) (void)__hip_atomic_fetch_add(counts + tid, (probe_acc_t)sCnt[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            long long gb = 0;
            for (int r = 0; r < nrows; ++r) gb += (long long)probe_fixed(sRes[r * RS + tid]);       // zero for a row that is not kept
            (void)__hip_atomic_fetch_add(gbias + tid, (probe_acc_t)gb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // columns tid + 256 i, i < NI = ceil(D / 256) <= 4: the branch is the same in the whole block
        if (D <= 256) probe_walk_classes<1>(x, row0, nrows, D, C, sRes, RS, sKeep, grad);
        else if (D <= 512) probe_walk_classes<2>(x, row0, nrows, D, C, sRes, RS, sKeep, grad);
        else if (D <= 768) probe_walk_classes<3>(x, row0, nrows, D, C, sRes, RS, sKeep, grad);
        else probe_walk_classes<4>(x, row0, nrows, D, C, sRes, RS, sKeep, grad);
    }
}

// *bad = 1 for a label outside -1 .. C - 1 or a class weight outside (0, 1] (a NaN included)
__global__ __launch_bounds__(256)
void probe_check_kernel(const int32_t* __restrict__ y, int N, int C, const float* __restrict__ cw, int* __restrict__ bad) {
    bool b = false;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) b = b || y[i] < -1 || y[i] >= C;
    if (cw && blockIdx.x == 0 && threadIdx.x < C) b = b || !(cw[threadIdx.x] > 0.f && cw[threadIdx.x] <= 1.0f);
    if (b) *bad = 1;
}

}  // namespace keepk
using namespace keepk;

// Groups of 64 rows per workgroup; any value gives the same words.  The residuals of 64 G rows x 16 NC classes have 32 KB of LDS, so
// G NC <= 8 in a gradient launch.  Measured at N = 100 000, D = 768: the gradient walk is bound by its integer
// arithmetic, not by its atomics, so it wants many workgroups: one group is the fastest at C = 8 and 64 and within 6 % of two at C = 2;
// the forward alone is cluster_assign's flow and takes its two groups.
int probe_groups(int N, int C, bool grad) {
    if (grad || N < (1 << 15)) return 1;
    return 2;
}

void launch_probe_check(const int32_t* labels, int N, int C, const float* class_weight, int* bad, hipStream_t s) {
    int blocks = (N + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(probe_check_kernel, dim3(blocks), dim3(256), 0, s, labels, N, C, class_weight, bad);
}

void launch_probe(const float* x, int N, int D, const float* w, const float* bias, int C, int groups, const int32_t* labels,
                  const float* class_weight, float* probs, int32_t* label, float* best, float* margin, int64_t* skipped, int64_t* grad,
                  int64_t* gbias, int64_t* loss, int64_t* counts, hipStream_t s) {
    const bool g_on = grad != nullptr;
    const int G = groups ? groups : probe_groups(N, C, g_on), nc = (C + 15) / 16;
    dim3 g((N + 64 * G - 1) / (64 * G)), b(256);
#define KEEP_PROBE_LAUNCH(NC, GRAD) hipLaunchKernelGGL((probe_kernel<NC, GRAD>), g, b, 0, s, x, w, bias, N, D, C, G, labels, class_weight, probs, \
                                                       label, best, margin, (probe_acc_t*)skipped, (probe_acc_t*)grad, (probe_acc_t*)gbias,      \
                                                       (probe_acc_t*)loss, (probe_acc_t*)counts)
    if (g_on) {
        if (nc == 1) KEEP_PROBE_LAUNCH(1, true); else if (nc == 2) KEEP_PROBE_LAUNCH(2, true); else if (nc == 3) KEEP_PROBE_LAUNCH(3, true);
        else KEEP_PROBE_LAUNCH(4, true);
    } else {
        if (nc == 1) KEEP_PROBE_LAUNCH(1, false); else if (nc == 2) KEEP_PROBE_LAUNCH(2, false); else if (nc == 3) KEEP_PROBE_LAUNCH(3, false);
        else KEEP_PROBE_LAUNCH(4, false);
    }
#undef KEEP_PROBE_LAUNCH
}
