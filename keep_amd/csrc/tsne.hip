// Exact t-SNE of a slide's tile features: the perplexity calibration of neighbour lists, the all-pairs repulsion
// of a 2-D embedding and one gradient-descent step.  The neighbour lists come from keep_topk, the joint graph (a CSR) from the caller.
//
//   tsne_affinities_kernel  a wave per row, a neighbour per lane.  d_j = max(0, 2 - 2 s_j) over the filled slots, shifted by the row's
//                       minimum; beta by TSNE_BISECT bisection steps (van der Maaten's search: doubling / halving until bracketed, then
//                       the midpoint), every step taken, none skipped: H(beta) = log(sum P) + beta sum d P / sum P with P = exp(-beta d),
//                       the sums by a fixed xor-shuffle tree; then one more evaluation at the last beta and p = P / sum P.  expf / logf are
//                       the library's (1 ulp), the division is IEEE.  A row's bits depend on that row alone.
//   tsne_repulsion_kernel<RPT>  the n-body loop.  blockIdx.y is a segment of KEEP_TSNE_SEGMENT columns, whose y_j are staged in LDS once
//                       (every lane reads one address per j: a broadcast); a thread owns RPT rows 256 apart in registers and walks j in
//                       ascending order: dx = x_i - x_j, dy likewise, t = fma(dy, dy, fma(dx, dx, 1)), w = rcp(t) (v_rcp_f32, 1 ulp),
//                       Z += w, w2 = w w, Rx = fma(w2, dx, Rx), Ry = fma(w2, dy, Ry): 8 VALU slots and one reciprocal per pair.  The
//                       self pair is left out by a test that only the workgroup whose rows lie in the segment pays (256 RPT divides
//                       the segment).  Every operation is an explicit rounding, so the words depend on KEEP_TSNE_SEGMENT alone: not on RPT,
//                       the grid or N.  partials[seg][row] = (Rx, Ry, Z, 0).
//   tsne_reduce_kernel  a thread per row adds its partials in segment order into rz[row] = (Rx, Ry, Z_i, 0) and the workgroup adds
//                       llrint(Z_i 2^22) into sums[0]: every term rounded before it is added, integer adds, so the word has no order.
//   tsne_update_kernel  a wave per row: the attractive force over the row's CSR entries in stored order (lane l takes entries l, l + 64, ...
//                       in turn, then the xor-shuffle tree), g = 4 (exaggeration A - R / Z), the update of van der Maaten's
//                       implementation (gain + 0.2 where g and the last update differ in sign, x 0.8 otherwise, floor 0.01; u = momentum u -
//                       lr gain g; y_out = y + u).  With `stats` also the row's sum of val (log val + log Z + log t) and |g|^2, added as
//                       fixed-point words into sums[1] (2^40) and sums[2] (2^50).
//
// Fixed points.  Z_i <= N - 1 < 2^20 and N <= 2^20 rows: |sums[0]| <= 2^20 2^20 2^22 = 2^62.  sum |val| = 1 and |log| < 2^8 in fp32:
// |sums[1]| < 2^49.  sum_i |g_i| <= 4 (exaggeration / 2 + 1 / 2) (w |d| <= 1/2 and the row masses sum to 1), so |g|^2 <= 4 (exaggeration
// + 1)^2 < 2^13 for exaggeration <= 44 (the entry point takes at most 32): |sums[2]| < 2^63.
//
// Row indices are int32 (N <= 2^20, checked by the caller); element offsets are int64.
#include "common.h"
#include "../../include/keep_hip.h"

namespace keepk {

typedef unsigned long long tsne_acc_t;
constexpr int TSNE_BISECT = 64;                         // bisection steps of a row, all taken
constexpr double TSNE_Z_ONE = 4194304.0;                // 2^22
constexpr double TSNE_KL_ONE = 1099511627776.0;         // 2^40
constexpr double TSNE_G2_ONE = 1125899906842624.0;      // 2^50
static_assert(KEEP_TSNE_SEGMENT >= 1024 && KEEP_TSNE_SEGMENT <= 8192 && KEEP_TSNE_SEGMENT % 1024 == 0,
              "KEEP_TSNE_SEGMENT is a multiple of 1024 (the rows of a workgroup at RPT = 4) in 1024 .. 8192 (64 KiB of LDS)");

// the sum over the wave by a fixed butterfly: every lane ends with the same bits
__device__ __forceinline__ float tsne_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = __fadd_rn(v, __shfl_xor(v, m));
    return v;
}

__device__ __forceinline__ float tsne_wave_min(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m));
    return v;
}

__global__ __launch_bounds__(256)
void tsne_affinities_kernel(const int64_t* __restrict__ index, const float* __restrict__ score, const int32_t* __restrict__ count, int N, int k,
                            float log_perp, float* __restrict__ p_out) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;                               // wave-uniform
    const int c = min(max(count[row], 0), k);
    const int64_t at = (int64_t)row * k + lane;
    const bool on = lane < c && index[at] >= 0;
    const int filled = __popcll(__ballot(on));
    float d = on ? fmaxf(0.f, __fsub_rn(2.f, __fmul_rn(2.f, score[at]))) : INFINITY;
    const float dmin = tsne_wave_min(d);                // by every lane: a shuffle inside the `on` branch would read idle lanes
    d = on ? __fsub_rn(d, dmin) : 0.f;
    float beta = 1.f, lo = -INFINITY, hi = INFINITY;
    for (int step = 0; step < TSNE_BISECT; ++step) {
        const float P = on ? expf(-__fmul_rn(d, beta)) : 0.f;
        const float sumP = tsne_wave_sum(P), sumDP = tsne_wave_sum(__fmul_rn(d, P));
        const float H = __fadd_rn(logf(sumP), __fdiv_rn(__fmul_rn(beta, sumDP), sumP));
        if (H > log_perp) {
            lo = beta;
            beta = hi == INFINITY ? __fmul_rn(beta, 2.f) : __fmul_rn(__fadd_rn(beta, hi), 0.5f);
        } else {
            hi = beta;
            beta = lo == -INFINITY ? __fmul_rn(beta, 0.5f) : __fmul_rn(__fadd_rn(beta, lo), 0.5f);
        }
    }
    const float P = on ? expf(-__fmul_rn(d, beta)) : 0.f;
    const float sumP = tsne_wave_sum(P);
    if (lane < k) p_out[at] = filled >= 2 ? __fdiv_rn(P, sumP) : 0.f;
}

// one segment's pairs of RPT rows.  self[r]: the row's own position in the segment (DIAG only)
template <int RPT, bool DIAG>
__device__ __forceinline__ void tsne_pairs(const float2* sy, int n, const float (&xi)[RPT], const float (&yi)[RPT], const int (&self)[RPT],
                                           float (&rx)[RPT], float (&ry)[RPT], float (&z)[RPT]) {
#pragma unroll 4
    for (int j = 0; j < n; ++j) {
        const float2 q = sy[j];
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            const float dx = __fsub_rn(xi[r], q.x), dy = __fsub_rn(yi[r], q.y);
            const float t = fmaf(dy, dy, fmaf(dx, dx, 1.f));
            float w = __builtin_amdgcn_rcpf(t);
            if (DIAG) w = j == self[r] ? 0.f : w;       // dx = dy = 0 there: the force words need no test
            z[r] = __fadd_rn(z[r], w);
            const float w2 = __fmul_rn(w, w);
            rx[r] = fmaf(w2, dx, rx[r]);
            ry[r] = fmaf(w2, dy, ry[r]);
        }
    }
}

template <int RPT>
__global__ __launch_bounds__(256)
void tsne_repulsion_kernel(const float* __restrict__ y, int N, float* __restrict__ partials) {
    __shared__ float2 sy[KEEP_TSNE_SEGMENT];
    const int tid = threadIdx.x, seg = blockIdx.y, seg0 = seg * KEEP_TSNE_SEGMENT, n = min(KEEP_TSNE_SEGMENT, N - seg0);
    const int row0 = blockIdx.x * (256 * RPT);
    const float2* y2 = reinterpret_cast<const float2*>(y);
    for (int j = tid; j < n; j += 256) sy[j] = y2[seg0 + j];
    __syncthreads();
    float xi[RPT], yi[RPT], rx[RPT], ry[RPT], z[RPT];
    int self[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int row = row0 + r * 256 + tid;
        const float2 me = row < N ? y2[row] : make_float2(0.f, 0.f);
        xi[r] = me.x; yi[r] = me.y; rx[r] = ry[r] = z[r] = 0.f;
        self[r] = row - seg0;
    }
    if (row0 / KEEP_TSNE_SEGMENT == seg) tsne_pairs<RPT, true>(sy, n, xi, yi, self, rx, ry, z);
    else tsne_pairs<RPT, false>(sy, n, xi, yi, self, rx, ry, z);
    float4* out = reinterpret_cast<float4*>(partials) + (int64_t)seg * N;
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int row = row0 + r * 256 + tid;
        if (row < N) out[row] = make_float4(rx[r], ry[r], z[r], 0.f);
    }
}

__global__ __launch_bounds__(256)
void tsne_reduce_kernel(const float* __restrict__ partials, int N, int n_seg, float* __restrict__ rz, tsne_acc_t* __restrict__ sums) {
    __shared__ long long s_part[4];
    const int tid = threadIdx.x, row = blockIdx.x * 256 + tid;
    long long zi = 0;
    if (row < N) {
        const float4* p = reinterpret_cast<const float4*>(partials);
        float rx = 0.f, ry = 0.f, z = 0.f;
        for (int s = 0; s < n_seg; ++s) {
            const float4 v = p[(int64_t)s * N + row];
            rx = __fadd_rn(rx, v.x); ry = __fadd_rn(ry, v.y); z = __fadd_rn(z, v.z);
        }
        reinterpret_cast<float4*>(rz)[row] = make_float4(rx, ry, z, 0.f);
        if (z >= 0.f && z <= 1048576.f) zi = __double2ll_rn((double)z * TSNE_Z_ONE);      // a NaN (a non-finite y) adds nothing
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) zi += __shfl_xor(zi, m);
    if ((tid & 63) == 0) s_part[tid >> 6] = zi;
    __syncthreads();
    if (tid == 0) {
        const long long tot = s_part[0] + s_part[1] + s_part[2] + s_part[3];
        if (tot) (void)__hip_atomic_fetch_add(sums, (tsne_acc_t)tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256)
void tsne_update_kernel(const float* __restrict__ y, int N, const float* __restrict__ rz, const int32_t* __restrict__ row_ptr,
                        const int32_t* __restrict__ col, const float* __restrict__ val, int nnz, float exaggeration, float momentum, float lr,
                        int stats, tsne_acc_t* __restrict__ sums, float* __restrict__ grad_out, float* __restrict__ update,
                        float* __restrict__ gains, float* __restrict__ y_out) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;                               // wave-uniform
    const float2* y2 = reinterpret_cast<const float2*>(y);
    const float2 me = y2[row];
    const float Z = (float)((double)(long long)sums[0] * (1.0 / TSNE_Z_ONE));
    const float logZ = logf(Z);
    const int b = max(row_ptr[row], 0), e = min(row_ptr[row + 1], nnz);
    float ax = 0.f, ay = 0.f, kl = 0.f;
    for (int t = b + lane; t < e; t += 64) {
        const int j = col[t];
        if ((unsigned)j >= (unsigned)N) continue;       // an entry outside the embedding is no edge
        const float v = val[t];
        const float2 q = y2[j];
        const float dx = __fsub_rn(me.x, q.x), dy = __fsub_rn(me.y, q.y);
        const float tt = fmaf(dy, dy, fmaf(dx, dx, 1.f));
        const float vw = __fmul_rn(v, __builtin_amdgcn_rcpf(tt));
        ax = fmaf(vw, dx, ax);
        ay = fmaf(vw, dy, ay);
        if (stats) kl = fmaf(v, __fadd_rn(__fadd_rn(logf(v), logZ), logf(tt)), kl);
    }
    ax = tsne_wave_sum(ax); ay = tsne_wave_sum(ay);
    if (stats) kl = tsne_wave_sum(kl);
    if (lane != 0) return;
    const float4 r = reinterpret_cast<const float4*>(rz)[row];
    const float gx = __fmul_rn(4.f, fmaf(exaggeration, ax, -__fdiv_rn(r.x, Z)));
    const float gy = __fmul_rn(4.f, fmaf(exaggeration, ay, -__fdiv_rn(r.y, Z)));
    if (grad_out) { grad_out[2 * row] = gx; grad_out[2 * row + 1] = gy; }
    if (stats) {
        const double g2 = (double)gx * gx + (double)gy * gy;
        if (kl == kl && fabsf(kl) < 1024.f)
            (void)__hip_atomic_fetch_add(sums + 1, (tsne_acc_t)__double2ll_rn((double)kl * TSNE_KL_ONE), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (g2 < 8192.0)
            (void)__hip_atomic_fetch_add(sums + 2, (tsne_acc_t)__double2ll_rn(g2 * TSNE_G2_ONE), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!update) return;
    const float g[2] = {gx, gy}, p[2] = {me.x, me.y};
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float u = update[2 * row + c];
        float gain = gains[2 * row + c];
        gain = __fmul_rn(u, g[c]) < 0.f ? __fadd_rn(gain, 0.2f) : __fmul_rn(gain, 0.8f);
        gain = fmaxf(gain, 0.01f);
        const float un = fmaf(momentum, u, -__fmul_rn(lr, __fmul_rn(gain, g[c])));
        gains[2 * row + c] = gain;
        update[2 * row + c] = un;
        y_out[2 * row + c] = __fadd_rn(p[c], un);
    }
}

}  // namespace keepk
using namespace keepk;

void launch_tsne_affinities(const int64_t* index, const float* score, const int32_t* count, int N, int k, float perplexity, float* p_out,
                            hipStream_t s) {
    hipLaunchKernelGGL(tsne_affinities_kernel, dim3((N + 3) / 4), dim3(256), 0, s, index, score, count, N, k, logf(perplexity), p_out);
}

void launch_tsne_repulsion(const float* y, int N, float* partials, hipStream_t s) {
    const int n_seg = (N + KEEP_TSNE_SEGMENT - 1) / KEEP_TSNE_SEGMENT;
    // rows per thread: any value gives the same words; fewer rows make more workgroups where N alone would not fill the chip
    const int rpt = (int64_t)((N + 1023) / 1024) * n_seg >= 1024 ? 4 : (int64_t)((N + 511) / 512) * n_seg >= 1024 ? 2 : 1;
#define KEEP_TSNE_REP(RPT) hipLaunchKernelGGL((tsne_repulsion_kernel<RPT>), dim3((N + 256 * RPT - 1) / (256 * RPT), n_seg), dim3(256), 0, s, y, N, partials)
    if (rpt == 4) KEEP_TSNE_REP(4); else if (rpt == 2) KEEP_TSNE_REP(2); else KEEP_TSNE_REP(1);
#undef KEEP_TSNE_REP
}

void launch_tsne_step(const float* y, int N, const float* partials, const int32_t* row_ptr, const int32_t* col, const float* val, int nnz,
                      float exaggeration, float momentum, float lr, int stats, int64_t* sums, float* rz, float* grad_out, float* update,
                      float* gains, float* y_out, hipStream_t s) {
    const int n_seg = (N + KEEP_TSNE_SEGMENT - 1) / KEEP_TSNE_SEGMENT;
    hipLaunchKernelGGL(tsne_reduce_kernel, dim3((N + 255) / 256), dim3(256), 0, s, partials, N, n_seg, rz, (tsne_acc_t*)sums);
    hipLaunchKernelGGL(tsne_update_kernel, dim3((N + 3) / 4), dim3(256), 0, s, y, N, rz, row_ptr, col, val, nnz, exaggeration, momentum, lr,
                       stats, (tsne_acc_t*)sums, grad_out, update, gains, y_out);
}
