// Attention-based multiple-instance learning: bags of unit feature rows [N,D], an attention network of L hidden
// units (L a multiple of 16 in 16 .. 128) and a linear head, which is the linear probe's own launch (probe.hip) on the pooled rows.
// A bag is a contiguous row range; the host cuts every bag from its own first row into chunks of at most KEEP_MIL_CHUNK rows and the
// kernels see the chunk table only: int32 [n_chunks][3] of (bag, first row, rows), checked by mil_check_kernel before it is an index.
//
//   mil_scores_kernel<NC>   a workgroup owns 64 rows: h = tanh(V x + bv) through probe_kernel's operand flow (v_mfma_f32_16x16x4_f32, a
//                       k-ordered fmaf chain per hidden unit, the bias after the chain), then s = w . h over the NC = L / 16 tiles in
//                       order (fmaf) and the 16 lanes by a fixed __shfl_xor tree.  A row's s and h depend on that row alone.  A row with
//                       a non-finite element or one with |x| > 1 (or a score that is not finite) is skipped: its score is -inf.
//   mil_max_kernel          the exact maximum of a bag's scores: per 128 rows of a chunk, one integer atomicMax of an order-preserving key
//   mil_pool_kernel<NI>     per chunk: e_i = expf(s_i - m_b) (0 for a skipped row), Z_b += llrint(e_i 2^40) and P_b[d] +=
//                       llrint(fp32(e_i x_id) 2^40): every term rounded before it is added, one 64-bit atomic per (128 rows, column)
//   mil_finish_*            a_i = e_i / fp32(Z_b 2^-40) and z_b[d] = fp32(P_b[d] / Z_b); |P_b[d]| <= Z_b as integers, so |z| <= 1
//   mil_dz_kernel           dz_b = sum_c r_bc Wc[c,:] (c ascending, fmaf) with the probe's residual r_bc = cw[y_b] (p_bc - [c = y_b]) and
//                       u_b = dz_b . z_b (columns ascending per thread, the xor tree, the four waves in order)
//   mil_ds_kernel           a wave per row: da_i = dz_b . x_i (fmaf, the xor tree), ds_i = a_i (da_i - u_b)
//   mil_gradv_kernel<NLT>   gV = R^T X per chunk on v_mfma_f32_16x16x4_f32 with R_il = fp32(ds_i w_l) fp32(1 - fp32(h_il^2)) formed while
//                       the A operand is staged; K runs over the chunk's rows in row order, padded with zero rows to a multiple of 16.
//                       A workgroup owns 16 NLT hidden units x 128 columns, a wave NLT x 2 accumulators; every accumulator is
//                       rounded ONCE, llrint(acc 2^36), and added with one no-return 64-bit atomic.  The workgroups of the first
//                       column slice also add g bv[l] += llrint(R_il 2^36) and g w[l] += llrint(fp32(ds_i h_il) 2^36) per term.
//
// Fixed points.  e_i <= 1 and a bag has at most 2^22 rows: Z_b, |P_b[d]| <= 2^62.  With |x_id| <= 1: |da_i|, |u_b| <= |dz_b|_1 <=
// 2 max_c |Wc_c|_1, so sum_i |ds_i| <= 4 max_c |Wc_c|_1 per bag and a bag adds at most G = 4 max(1, |w|_inf) max_c |Wc_c|_1 to any
// word of gV, g bv or g w.  The caller holds G <= 2^10 and the bags added into one set of accumulators <= 2^16: |word| <= 2^62.
// A chunk's contribution depends on its bag alone, so every word is the same for every split of the bags over calls.
//
// Row indices are int32 (N <= 2^22, checked by the caller); element offsets are int64.
#include "common.h"
#include "../../include/keep_hip.h"

namespace keepk {

typedef unsigned long long mil_acc_t;
constexpr float MIL_GRAD_ONE = 68719476736.f;          // 2^36
constexpr int MIL_KEY_NEG_INF = (int)0x807fffffu;      // mil_key(-inf)
// The per-row kernels (max, pool, finish, ds) give a workgroup MIL_PART rows of a chunk: grid (n_chunks, KEEP_MIL_CHUNK / MIL_PART).  Their
// sums are integers of per-term-rounded values and their outputs per row, so the split changes no bit; only mil_gradv_kernel, which
// rounds once per chunk, sees the chunk whole.
constexpr int MIL_PART = 128;
static_assert(KEEP_MIL_CHUNK % MIL_PART == 0 && KEEP_MIL_CHUNK >= MIL_PART, "KEEP_MIL_CHUNK is a multiple of 128");
// the workgroup's rows of chunk c: false when the chunk ends before them (the same in the whole block)
__device__ __forceinline__ bool mil_part(const int32_t* __restrict__ chunks, int c, int& bag, int& first, int& rows) {
    bag = chunks[3 * c];
    const int p0 = blockIdx.y * MIL_PART, n = chunks[3 * c + 2];
    first = chunks[3 * c + 1] + p0;
    rows = min(n - p0, MIL_PART);
    return p0 < n;
}

// order-preserving int32 key of a float that is not NaN
__device__ __forceinline__ int mil_key(float f) { const int i = __float_as_int(f); return i >= 0 ? i : i ^ 0x7fffffff; }
__device__ __forceinline__ float mil_unkey(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }
__device__ __forceinline__ bool mil_bad(float x) { return !(fabsf(x) <= 1.0f); }
// llrint(v 2^40) for |v| <= 1 from two int32 conversions: v 2^20 = hi + f with f exact, and hi 2^20 is an even integer
__device__ __forceinline__ long long mil_fixed40(float v) {
    const float t = __fmul_rn(v, 1048576.f), hi = rintf(t), lo = __fmul_rn(__fsub_rn(t, hi), 1048576.f);
    return ((long long)__float2int_rn(hi) << 20) + (long long)__float2int_rn(lo);
}
__device__ __forceinline__ long long mil_fixed36(float v) { return __float2ll_rn(__fmul_rn(v, MIL_GRAD_ONE)); }

template <int NC>
__global__ __launch_bounds__(256)
void mil_scores_kernel(const float* __restrict__ x, const float* __restrict__ V, const float* __restrict__ bv, const float* __restrict__ w,
                       int N, int D, float* __restrict__ s_out, float* __restrict__ h_out, mil_acc_t* __restrict__ skipped) {
    constexpr int L = NC * 16, NS = (NC + 3) / 4;      // a thread stages NS float4 of V per block of 16 k: the columns tid / 4 + 64 u
    __shared__ f32x4 sB[2][4][L];
    __shared__ int s_skipped;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int row_base = blockIdx.x * 64 + wave * 16;
    const int bcol = tid >> 2, bq = tid & 3;
    const int nblk = D >> 4;
    if (tid == 0) s_skipped = 0;
    float bj[NC], wj[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) { bj[c] = bv[c * 16 + j]; wj[c] = w[c * 16 + j]; }
    const float* ap = x + (int64_t)min(row_base + j, N - 1) * D + kq * 4;
    f32x4 acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    bool bad = false;
    f32x4 a_next = *reinterpret_cast<const f32x4*>(ap), b_next[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u)
        b_next[u] = (bcol + 64 * u < L) ? *reinterpret_cast<const f32x4*>(V + (int64_t)(bcol + 64 * u) * D + bq * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < nblk; ++kb) {
#pragma unroll
        for (int u = 0; u < NS; ++u)
            if (bcol + 64 * u < L) sB[kb & 1][bq][bcol + 64 * u] = b_next[u];
        const f32x4 a = a_next;
        __syncthreads();
        if (kb + 1 < nblk) {
            a_next = *reinterpret_cast<const f32x4*>(ap + (kb + 1) * 16);
#pragma unroll
            for (int u = 0; u < NS; ++u)
                if (bcol + 64 * u < L) b_next[u] = *reinterpret_cast<const f32x4*>(V + (int64_t)(bcol + 64 * u) * D + bq * 4 + (kb + 1) * 16);
        }
        bad = bad || mil_bad(a[0]) || mil_bad(a[1]) || mil_bad(a[2]) || mil_bad(a[3]);
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
    // lane (j, kq) holds rows row_base + kq*4 + r (r = 0..3) at the hidden units c*16 + j
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int lr = kq * 4 + r, row = row_base + lr;
        bool rbad = __shfl(badi, lr) != 0;
        float t = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float hh = tanhf(__fadd_rn(acc[c][r], bj[c]));         // the bias comes after the chain
            if (h_out && row < N) h_out[(int64_t)row * L + c * 16 + j] = hh;
            t = fmaf(wj[c], hh, t);                                      // tiles in order, then the lanes by the xor tree
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) t = __fadd_rn(t, __shfl_xor(t, o));
        rbad = rbad || !(fabsf(t) < INFINITY);
        if (j == 0 && row < N) {
            s_out[row] = rbad ? -INFINITY : t;
            if (rbad) atomicAdd(&s_skipped, 1);
        }
    }
    __syncthreads();
    if (tid == 0 && s_skipped) (void)__hip_atomic_fetch_add(skipped, (mil_acc_t)s_skipped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// *bad = 1 for a chunk that leaves [0, S) or [0, N) or has no row or more than KEEP_MIL_CHUNK
__global__ __launch_bounds__(256)
void mil_check_kernel(const int32_t* __restrict__ chunks, int n_chunks, int N, int S, int* __restrict__ bad) {
    bool b = false;
    for (int c = blockIdx.x * 256 + threadIdx.x; c < n_chunks; c += gridDim.x * 256) {
        const int bag = chunks[3 * c], first = chunks[3 * c + 1], rows = chunks[3 * c + 2];
        b = b || bag < 0 || bag >= S || first < 0 || rows < 1 || rows > KEEP_MIL_CHUNK || (int64_t)first + rows > N;
    }
    if (b) *bad = 1;
}

__global__ __launch_bounds__(256)
void mil_max_kernel(const float* __restrict__ s, const int32_t* __restrict__ chunks, int* __restrict__ mkey) {
    __shared__ float sm[4];
    int bag, first, rows;
    if (!mil_part(chunks, blockIdx.x, bag, first, rows)) return;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < rows; i += 256) m = fmaxf(m, s[first + i]);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
        if (m > -INFINITY) atomicMax(mkey + bag, mil_key(m));
    }
}

// columns tid + 256 i, i < NI = ceil(D / 256).  e_out: the unnormalised e_i (mil_finish_rows_kernel divides them)
template <int NI>
__global__ __launch_bounds__(256)
void mil_pool_kernel(const float* __restrict__ x, const float* __restrict__ s, const int32_t* __restrict__ chunks, int D,
                     const int* __restrict__ mkey, float* __restrict__ e_out, mil_acc_t* __restrict__ Z, mil_acc_t* __restrict__ P,
                     int32_t* __restrict__ kept_rows) {
    __shared__ float sE[MIL_PART];
    __shared__ mil_acc_t s_z;
    __shared__ int s_kept;
    const int tid = threadIdx.x;
    int bag, first, rows;
    if (!mil_part(chunks, blockIdx.x, bag, first, rows)) return;
    const float m = mil_unkey(mkey[bag]);
    if (!(m > -INFINITY)) return;                      // no kept row in the bag: the same in the whole block
    if (tid == 0) { s_z = 0; s_kept = 0; }
    __syncthreads();
    long long zp = 0; int kp = 0;
    for (int i = tid; i < rows; i += 256) {
        const float si = s[first + i];
        const bool on = si > -INFINITY;
        const float e = on ? expf(__fsub_rn(si, m)) : 0.f;
        sE[i] = e;
        e_out[first + i] = e;
        zp += mil_fixed40(e);
        kp += on ? 1 : 0;
    }
    if (zp) atomicAdd(&s_z, (mil_acc_t)zp);
    if (kp) atomicAdd(&s_kept, kp);
    __syncthreads();
    if (tid == 0) {
        (void)__hip_atomic_fetch_add(Z + bag, s_z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (s_kept) atomicAdd(kept_rows + bag, s_kept);
    }
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
            const float* xr = x + (int64_t)(first + min(r0 + u, rows - 1)) * D;
#pragma unroll
            for (int i = 0; i < NI; ++i) v[u][i] = xr[col[i]];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (r0 + u >= rows) continue;
            const float e = sE[r0 + u];
            if (e == 0.f) continue;                    // a skipped row (its x may hold anything) or an underflow: the same in every thread
#pragma unroll
            for (int i = 0; i < NI; ++i) acc[i] += mil_fixed40(__fmul_rn(e, v[u][i]));
        }
    }
#pragma unroll
    for (int i = 0; i < NI; ++i)
        if (i < NI - 1 || last_on)
            (void)__hip_atomic_fetch_add(P + (int64_t)bag * D + col[i], (mil_acc_t)acc[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one workgroup per bag.  head_labels (may be null): y[b] (0 without y) for a bag with a kept row, -1 for one without
__global__ __launch_bounds__(256)
void mil_finish_bags_kernel(const mil_acc_t* __restrict__ Z, const mil_acc_t* __restrict__ P, const int32_t* __restrict__ y, int D,
                            float* __restrict__ z, int32_t* __restrict__ head_labels, mil_acc_t* __restrict__ skipped_bags) {
    const int b = blockIdx.x;
    const long long zb = (long long)Z[b];
    for (int d = threadIdx.x; d < D; d += 256)
        z[(int64_t)b * D + d] = zb ? (float)((double)(long long)P[(int64_t)b * D + d] / (double)zb) : 0.f;
    if (threadIdx.x == 0) {
        if (head_labels) head_labels[b] = zb ? (y ? y[b] : 0) : -1;
        if (!zb) (void)__hip_atomic_fetch_add(skipped_bags, (mil_acc_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256)
void mil_finish_rows_kernel(const int32_t* __restrict__ chunks, const mil_acc_t* __restrict__ Z, float* __restrict__ a) {
    int bag, first, rows;
    if (!mil_part(chunks, blockIdx.x, bag, first, rows)) return;
    const long long zb = (long long)Z[bag];
    const float zf = (float)((double)zb * 9.094947017729282e-13);        // 2^-40
    for (int i = threadIdx.x; i < rows; i += 256) a[first + i] = zb ? __fdiv_rn(a[first + i], zf) : 0.f;
}

// one workgroup per bag: dz [S][D], u [S]
__global__ __launch_bounds__(256)
void mil_dz_kernel(const float* __restrict__ probs, const int32_t* __restrict__ head_labels, const float* __restrict__ cw,
                   const float* __restrict__ Wc, const float* __restrict__ z, int D, int C, float* __restrict__ dz, float* __restrict__ u) {
    __shared__ float sr[PROBE_MAX_C];
    __shared__ float su[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    int yi = head_labels[b];
    if (yi < -1 || yi >= C) yi = -1;                   // the head's check launch has refused these; never an index
    if (yi < 0) {                                      // left out or without a kept row: in no sum
        for (int d = tid; d < D; d += 256) dz[(int64_t)b * D + d] = 0.f;
        if (tid == 0) u[b] = 0.f;
        return;
    }
    if (tid < C) sr[tid] = __fmul_rn(cw ? cw[yi] : 1.0f, __fsub_rn(probs[(int64_t)b * C + tid], tid == yi ? 1.0f : 0.f));
    __syncthreads();
    float part = 0.f;
    for (int d = tid; d < D; d += 256) {
        float acc = 0.f;
        for (int c = 0; c < C; ++c) acc = fmaf(sr[c], Wc[(int64_t)c * D + d], acc);
        dz[(int64_t)b * D + d] = acc;
        part = fmaf(acc, z[(int64_t)b * D + d], part);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) part = __fadd_rn(part, __shfl_xor(part, o));
    if ((tid & 63) == 0) su[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) u[b] = __fadd_rn(__fadd_rn(__fadd_rn(su[0], su[1]), su[2]), su[3]);
}

// a wave per row: ds [N]
__global__ __launch_bounds__(256)
void mil_ds_kernel(const float* __restrict__ x, const float* __restrict__ s, const float* __restrict__ a, const int32_t* __restrict__ chunks,
                   const int32_t* __restrict__ head_labels, const float* __restrict__ dz, const float* __restrict__ u, int D,
                   float* __restrict__ ds) {
    int bag, first, rows;
    if (!mil_part(chunks, blockIdx.x, bag, first, rows)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (head_labels[bag] < 0) {
        for (int i = threadIdx.x; i < rows; i += 256) ds[first + i] = 0.f;
        return;
    }
    const float ub = u[bag];
    const float* dzb = dz + (int64_t)bag * D;
    for (int i = wave; i < rows; i += 4) {
        const int row = first + i;
        if (!(s[row] > -INFINITY)) {                   // the same in the whole wave
            if (lane == 0) ds[row] = 0.f;
            continue;
        }
        float part = 0.f;
        for (int d = lane * 4; d < D; d += 256) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + (int64_t)row * D + d), gv = *reinterpret_cast<const f32x4*>(dzb + d);
            part = fmaf(gv[0], xv[0], part);
            part = fmaf(gv[1], xv[1], part);
            part = fmaf(gv[2], xv[2], part);
            part = fmaf(gv[3], xv[3], part);
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) part = __fadd_rn(part, __shfl_xor(part, o));
        if (lane == 0) ds[row] = __fmul_rn(a[row], __fsub_rn(part, ub));
    }
}

// grid (n_chunks, ceil(D / 128), ceil(L / (16 NLT))): the workgroup's tile is 16 NLT hidden units x 128 columns; wave w has the columns
// 32 w .. 32 w + 31 of it as NLT x 2 accumulators of 16 x 16.  Lane (j, kq): A = R[row k0 + kq][unit j], B = x[row k0 + kq][column j];
// accumulator register r is unit kq*4 + r, column j.
template <int NLT>
__global__ __launch_bounds__(256)
void mil_gradv_kernel(const float* __restrict__ x, const float* __restrict__ hbuf, const float* __restrict__ ds, const float* __restrict__ s,
                      const float* __restrict__ w, const int32_t* __restrict__ chunks, const int32_t* __restrict__ head_labels, int D, int L,
                      mil_acc_t* __restrict__ gV, mil_acc_t* __restrict__ gbv, mil_acc_t* __restrict__ gw) {
    constexpr int LS = NLT * 16;
    __shared__ float sR[2][16][LS + 1];
    __shared__ int sOn[2][16];
    __shared__ mil_acc_t sGb[LS], sGw[LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int c = blockIdx.x, bag = chunks[3 * c], first = chunks[3 * c + 1], rows = chunks[3 * c + 2];
    if (head_labels[bag] < 0) return;                  // every ds of the bag is 0: the same in the whole block
    const int l0 = blockIdx.z * LS, d0 = blockIdx.y * 128 + wave * 32;
    const bool sums = blockIdx.y == 0;
    if (tid < LS) { sGb[tid] = 0; sGw[tid] = 0; }
    __syncthreads();
    int bc[2];
    bc[0] = min(d0 + j, D - 1);
    bc[1] = min(d0 + 16 + j, D - 1);
    f32x4 acc[NLT][2];
#pragma unroll
    for (int t = 0; t < NLT; ++t) { acc[t][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[t][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    const int nkb = (rows + 15) >> 4;
    for (int kb = 0; kb < nkb; ++kb) {
        // R of the rows kb*16 .. kb*16 + 15: element tid + 256 q is row (.) / LS, unit (.) % LS
#pragma unroll
        for (int q = 0; q < NLT; ++q) {
            const int e = tid + 256 * q, rr = e / LS, cc = e - rr * LS;
            const int row = kb * 16 + rr, l = l0 + cc;
            float R = 0.f, G = 0.f;
            if (row < rows && l < L) {
                const int gi = first + row;
                if (s[gi] > -INFINITY) {
                    const float dsi = ds[gi], hv = hbuf[(int64_t)gi * L + l];
                    R = __fmul_rn(__fmul_rn(dsi, w[l]), __fsub_rn(1.0f, __fmul_rn(hv, hv)));
                    G = __fmul_rn(dsi, hv);
                }
            }
            sR[kb & 1][rr][cc] = R;
            if (sums) {
                if (R != 0.f) atomicAdd(&sGb[cc], (mil_acc_t)mil_fixed36(R));
                if (G != 0.f) atomicAdd(&sGw[cc], (mil_acc_t)mil_fixed36(G));
            }
        }
        if (tid < 16) sOn[kb & 1][tid] = (kb * 16 + tid < rows && s[first + kb * 16 + tid] > -INFINITY) ? 1 : 0;
        float bvals[4][2];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const float* xr = x + (int64_t)(first + min(kb * 16 + kk * 4 + kq, rows - 1)) * D;
            bvals[kk][0] = xr[bc[0]];
            bvals[kk][1] = xr[bc[1]];
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const bool on = sOn[kb & 1][kk * 4 + kq] != 0;               // a skipped row or one past the chunk is a zero row, whatever x holds
            const float b0 = on ? bvals[kk][0] : 0.f, b1 = on ? bvals[kk][1] : 0.f;
#pragma unroll
            for (int t = 0; t < NLT; ++t) {
                const float av = sR[kb & 1][kk * 4 + kq][t * 16 + j];
                acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0, acc[t][0], 0, 0, 0);
                acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1, acc[t][1], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NLT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int l = l0 + t * 16 + kq * 4 + r;
            if (l >= L) continue;
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                const int d = d0 + v * 16 + j;
                if (d < D) (void)__hip_atomic_fetch_add(gV + (int64_t)l * D + d, (mil_acc_t)mil_fixed36(acc[t][v][r]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    if (sums) {
        __syncthreads();
        if (tid < LS && l0 + tid < L) {
            (void)__hip_atomic_fetch_add(gbv + l0 + tid, sGb[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_add(gw + l0 + tid, sGw[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace keepk
using namespace keepk;

void launch_mil_check(const int32_t* chunks, int n_chunks, int N, int S, int* bad, hipStream_t s) {
    int blocks = (n_chunks + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(mil_check_kernel, dim3(blocks), dim3(256), 0, s, chunks, n_chunks, N, S, bad);
}

void launch_mil_scores(const float* x, int N, int D, const float* V, const float* bv, const float* w, int L, float* s_out, float* h_out,
                       int64_t* skipped_rows, hipStream_t s) {
    dim3 g((N + 63) / 64), b(256);
#define KEEP_MIL_SCORES(NC) hipLaunchKernelGGL((mil_scores_kernel<NC>), g, b, 0, s, x, V, bv, w, N, D, s_out, h_out, (mil_acc_t*)skipped_rows)
    switch (L / 16) {
        case 1: KEEP_MIL_SCORES(1); break;
        case 2: KEEP_MIL_SCORES(2); break;
        case 3: KEEP_MIL_SCORES(3); break;
        case 4: KEEP_MIL_SCORES(4); break;
        case 5: KEEP_MIL_SCORES(5); break;
        case 6: KEEP_MIL_SCORES(6); break;
        case 7: KEEP_MIL_SCORES(7); break;
        default: KEEP_MIL_SCORES(8); break;
    }
#undef KEEP_MIL_SCORES
}

// mkey int32 [S], Z int64 [S], P int64 [S][D] and kept_rows int32 [S] are set here; e_out fp32 [N] is zeroed here and holds the attention on return
void launch_mil_pool(const float* x, int N, int D, const float* s_in, const int32_t* chunks, int n_chunks, int S, const int32_t* y, int* mkey,
                     int64_t* Z, int64_t* P, float* a_out, float* z_out, int32_t* kept_rows, int32_t* head_labels, int64_t* skipped_bags,
                     hipStream_t s) {
    (void)hipMemsetD32Async((hipDeviceptr_t)mkey, MIL_KEY_NEG_INF, (size_t)S, s);
    (void)hipMemsetAsync(Z, 0, (size_t)S * 8, s);
    (void)hipMemsetAsync(P, 0, (size_t)S * D * 8, s);
    (void)hipMemsetAsync(kept_rows, 0, (size_t)S * 4, s);
    (void)hipMemsetAsync(a_out, 0, (size_t)N * 4, s);
    if (n_chunks > 0) {
        dim3 g(n_chunks, KEEP_MIL_CHUNK / MIL_PART), b(256);
        hipLaunchKernelGGL(mil_max_kernel, g, b, 0, s, s_in, chunks, mkey);
#define KEEP_MIL_POOL(NI) hipLaunchKernelGGL((mil_pool_kernel<NI>), g, b, 0, s, x, s_in, chunks, D, mkey, a_out, (mil_acc_t*)Z, (mil_acc_t*)P, kept_rows)
        if (D <= 256) KEEP_MIL_POOL(1); else if (D <= 512) KEEP_MIL_POOL(2); else if (D <= 768) KEEP_MIL_POOL(3); else KEEP_MIL_POOL(4);
#undef KEEP_MIL_POOL
        hipLaunchKernelGGL(mil_finish_rows_kernel, g, b, 0, s, chunks, (const mil_acc_t*)Z, a_out);
    }
    hipLaunchKernelGGL(mil_finish_bags_kernel, dim3(S), dim3(256), 0, s, (const mil_acc_t*)Z, (const mil_acc_t*)P, y, D, z_out, head_labels,
                       (mil_acc_t*)skipped_bags);
}

void launch_mil_backward(const float* x, int D, const int32_t* chunks, int n_chunks, int S, const int32_t* head_labels, const float* probs,
                         const float* Wc, int C, const float* cw, const float* w, int L, const float* s_in, const float* a, const float* z,
                         const float* hbuf, float* dz, float* u, float* ds, int64_t* gV, int64_t* gbv, int64_t* gw, hipStream_t s) {
    hipLaunchKernelGGL(mil_dz_kernel, dim3(S), dim3(256), 0, s, probs, head_labels, cw, Wc, z, D, C, dz, u);
    if (n_chunks <= 0) return;
    hipLaunchKernelGGL(mil_ds_kernel, dim3(n_chunks, KEEP_MIL_CHUNK / MIL_PART), dim3(256), 0, s, x, s_in, a, chunks, head_labels, dz, u, D, ds);
    // hidden-unit tiles per workgroup: all of them up to 4, otherwise the split with the least padding
    const int nt = L / 16, nlt = nt <= 4 ? nt : (nt <= 6 ? 3 : 4);
    dim3 g(n_chunks, (D + 127) / 128, (nt + nlt - 1) / nlt), b(256);
#define KEEP_MIL_GRADV(NLT) hipLaunchKernelGGL((mil_gradv_kernel<NLT>), g, b, 0, s, x, hbuf, ds, s_in, w, chunks, head_labels, D, L, (mil_acc_t*)gV, \
                                               (mil_acc_t*)gbv, (mil_acc_t*)gw)
    if (nlt == 1) KEEP_MIL_GRADV(1); else if (nlt == 2) KEEP_MIL_GRADV(2); else if (nlt == 3) KEEP_MIL_GRADV(3); else KEEP_MIL_GRADV(4);
#undef KEEP_MIL_GRADV
}
