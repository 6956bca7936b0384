// Macenko stain normalisation of H & E pixels.  Integer arithmetic throughout: every result is held exactly to
// keep_amd.stain's numpy restatements.  The host does the tiny dense algebra in float64 between the passes (a 3 x 3 eigh, a 3 x 2
// pinv, percentiles read off the histograms) and hands its results back quantised.
//
//   stain_moments      uint8 RGB / RGBA image (+ an optional {0,1} mask one pixel of which covers ds x ds image pixels) -> od_q per
//                      channel from a 256-entry table in LDS; a pixel is kept iff the mask allows it and all three od_q >= beta_q ->
//                      n, 3 sums, 6 products in int64 registers -> wave shuffles -> LDS -> one 64-bit atomic per workgroup and word
//   stain_angle_hist   kept pixels as above -> t = od_q . V_q (two dot products) -> the bin of atan2(t1, t0) among 4096 equal bins of
//                      [-pi, pi) by integer comparisons alone: quadrant from the signs, an exact rotation into the first quadrant,
//                      then a 10-step binary search of a table of 2^30-scaled directions by the sign of a 64-bit cross product ->
//                      LDS histogram, one global atomic per non-empty bin per workgroup
//   stain_conc_hist    every masked pixel (no beta rule) -> c_s = od_q . Minv_q[s] (Q26) -> bin clamp(c_s >> 17, 0, 4095) -> two LDS
//                      histograms, flushed the same way
//   stain_apply_u8     the hot path: contiguous uint8 [n,3] -> table -> 3 x 3 integer matrix -> table, 4 pixels (three dwords) per
//                      thread and step; both tables in LDS; no float and no branch on the data
//
// Integer sums do not depend on the order, so every output is the same from run to run and however the pixels are split over calls.
#include "common.h"
#include "../../include/keep_hip.h"

namespace keepk {

struct StainView {                                    // a strided image and the mask over it (mask = null: every pixel)
    const unsigned char* img;
    int64_t row;
    int ps, h, w;
    const unsigned char* mask;
    int64_t mh, mw, ds;
};

__device__ __forceinline__ bool stain_masked_in(const StainView& v, int x, int y) {
    if (!v.mask) return true;
    const int64_t mx = x / v.ds, my = y / v.ds;
    return mx < v.mw && my < v.mh && v.mask[my * v.mw + mx] != 0;
}

// pixel i (row-major) -> its three od_q; false if the mask drops it
__device__ __forceinline__ bool stain_pixel(const StainView& v, int i, const int* od, int* r, int* g, int* b) {
    const int y = i / v.w, x = i - y * v.w;
    if (!stain_masked_in(v, x, y)) return false;
    const unsigned char* p = v.img + (int64_t)y * v.row + (int64_t)x * v.ps;
    *r = od[p[0]]; *g = od[p[1]]; *b = od[p[2]];
    return true;
}

__device__ __forceinline__ long long stain_wave_sum(long long x) {
#pragma unroll
    for (int o = 32; o; o >>= 1) x += __shfl_down(x, o);
    return x;
}

__global__ __launch_bounds__(256)
void stain_moments_kernel(StainView v, const int* __restrict__ od_q, int beta_q, unsigned long long* __restrict__ out) {
    __shared__ int od[256];
    __shared__ long long part[4][STAIN_MOMENTS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    od[tid] = od_q[tid];
    __syncthreads();
    long long a[STAIN_MOMENTS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int n = v.h * v.w;
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)gridDim.x * 256) {
        int r, g, b;
        if (!stain_pixel(v, (int)i, od, &r, &g, &b) || r < beta_q || g < beta_q || b < beta_q) continue;
        a[0] += 1; a[1] += r; a[2] += g; a[3] += b;
        a[4] += (long long)r * r; a[5] += (long long)r * g; a[6] += (long long)r * b;
        a[7] += (long long)g * g; a[8] += (long long)g * b; a[9] += (long long)b * b;
    }
#pragma unroll
    for (int k = 0; k < STAIN_MOMENTS; ++k) {
        const long long s = stain_wave_sum(a[k]);
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    if (tid < STAIN_MOMENTS) {
        const long long s = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
        if (s) atomicAdd(out + tid, (unsigned long long)s);                  // two's complement: a negative sum adds correctly
    }
}

// The bin of atan2(y, x) among STAIN_ANGLE_BINS equal bins of [-pi, pi); (0, 0) and the angle 0 start bin BINS / 2, the angle pi
// is -pi (bin 0).  dirs[j] = (rint(2^30 cos), rint(2^30 sin)) of j 2 pi / BINS, j < BINS / 4; |x|, |y| < 2^31, so each product
// stays below 2^61.
__device__ __forceinline__ int stain_angle_bin(long long x, long long y, const int2* dirs) {
    constexpr int Q = STAIN_ANGLE_BINS / 4;
    int base;
    long long u, w;
    if (x > 0 && y >= 0) { base = 2 * Q; u = x; w = y; }
    else if (x <= 0 && y > 0) { base = 3 * Q; u = y; w = -x; }               // rotated by -pi / 2
    else if (x < 0 && y <= 0) { base = 0; u = -x; w = -y; }                  // by pi
    else if (x >= 0 && y < 0) { base = Q; u = -y; w = x; }                   // by +pi / 2
    else return 2 * Q;
    int lo = 0, hi = Q;                               // dirs[lo] is at or before (u, w), dirs[hi] (hi = Q: the next axis) after it
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        const int2 d = dirs[mid];
        if ((long long)d.x * w - (long long)d.y * u >= 0) lo = mid; else hi = mid;
    }
    return base + lo;
}

struct StainVq { int v[6]; };                         // V_q [3][2] or Minv_q [2][3], by value

__global__ __launch_bounds__(256)
void stain_angle_hist_kernel(StainView v, const int* __restrict__ od_q, int beta_q, StainVq vq, const int2* __restrict__ dirs_g,
                             int* __restrict__ hist) {
    constexpr int Q = STAIN_ANGLE_BINS / 4;
    __shared__ int od[256];
    __shared__ int2 dirs[Q];
    __shared__ int bins[STAIN_ANGLE_BINS];
    const int tid = threadIdx.x;
    od[tid] = od_q[tid];
    for (int i = tid; i < Q; i += 256) dirs[i] = dirs_g[i];
    for (int i = tid; i < STAIN_ANGLE_BINS; i += 256) bins[i] = 0;
    __syncthreads();
    const int n = v.h * v.w;
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)gridDim.x * 256) {
        int r, g, b;
        if (!stain_pixel(v, (int)i, od, &r, &g, &b) || r < beta_q || g < beta_q || b < beta_q) continue;
        const long long t0 = (long long)r * vq.v[0] + (long long)g * vq.v[2] + (long long)b * vq.v[4];
        const long long t1 = (long long)r * vq.v[1] + (long long)g * vq.v[3] + (long long)b * vq.v[5];
        atomicAdd(&bins[stain_angle_bin(t0, t1, dirs)], 1);
    }
    __syncthreads();
    for (int i = tid; i < STAIN_ANGLE_BINS; i += 256)
        if (bins[i]) atomicAdd(&hist[i], bins[i]);
}

__global__ __launch_bounds__(256)
void stain_conc_hist_kernel(StainView v, const int* __restrict__ od_q, StainVq mq, int* __restrict__ hist) {
    __shared__ int od[256];
    __shared__ int bins[2 * STAIN_CONC_BINS];
    const int tid = threadIdx.x;
    od[tid] = od_q[tid];
    for (int i = tid; i < 2 * STAIN_CONC_BINS; i += 256) bins[i] = 0;
    __syncthreads();
    const int n = v.h * v.w;
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)gridDim.x * 256) {
        int r, g, b;
        if (!stain_pixel(v, (int)i, od, &r, &g, &b)) continue;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const long long c = (long long)r * mq.v[3 * s] + (long long)g * mq.v[3 * s + 1] + (long long)b * mq.v[3 * s + 2];
            const long long k = c >> STAIN_CONC_SHIFT;
            atomicAdd(&bins[s * STAIN_CONC_BINS + (int)min(max(k, 0ll), (long long)(STAIN_CONC_BINS - 1))], 1);
        }
    }
    __syncthreads();
    for (int i = tid; i < 2 * STAIN_CONC_BINS; i += 256)
        if (bins[i]) atomicAdd(&hist[i], bins[i]);
}

// ---- the apply ---------------------------------------------------------------------------------------------------------------
// T_q = 256 hi + lo with 0 <= lo < 256 and |hi| <= 2^12; |od_q| < 2^15.  With a = sum_d hi_d od_d and l = sum_d lo_d od_d the sum of
// the contract is 256 a + l, and floor((256 a + l + 2^15) / 2^16) = floor((a + floor((l + 2^15) / 2^8)) / 2^8) because a is an integer:
// no 64-bit product, |a| < 3 * 2^27 and 0 <= |l| < 3 * 2^23 fit an int32.  The r and g terms of each sum are one 16-bit dot
// product (v_dot2_i32_i16), the b term a 24-bit multiply-add that also brings in the constant (2^15, or -lo of the exp table).
typedef short stain_s2 __attribute__((ext_vector_type(2)));
struct StainTq { int hi_rg[3], lo_rg[3], hi_b[3], lo_b[3]; };              // per output channel; *_rg: the r entry in the low half

// rg: od_r in the low half, od_g in the high half; returns exp_lut[clamp(o - lo, 0, last)], bias = -256 lo
__device__ __forceinline__ unsigned stain_out(const StainTq& t, int c, int rg, int b, const unsigned char* lut, int bias, int last) {
    const stain_s2 v = __builtin_bit_cast(stain_s2, rg);
    const int a = __builtin_amdgcn_sdot2(v, __builtin_bit_cast(stain_s2, t.hi_rg[c]), __mul24(t.hi_b[c], b) + bias, false);
    const int l = __builtin_amdgcn_sdot2(v, __builtin_bit_cast(stain_s2, t.lo_rg[c]), __mul24(t.lo_b[c], b) + (1 << 15), false);
    const int o = (a + (l >> 8)) >> 8;
    return lut[min(max(o, 0), last)];
}

// od: three tables of 256: [0] od_q & 0xffff, [256] od_q << 16, [512] od_q, so that (od_r, od_g) packs with one OR
__device__ __forceinline__ unsigned stain_pixel_out(const StainTq& t, unsigned r8, unsigned g8, unsigned b8, const int* od,
                                                    const unsigned char* lut, int bias, int last) {
    const int rg = od[r8] | od[256 + g8], b = od[512 + b8];
    return stain_out(t, 0, rg, b, lut, bias, last) | (stain_out(t, 1, rg, b, lut, bias, last) << 8) |
           (stain_out(t, 2, rg, b, lut, bias, last) << 16);
}

struct __attribute__((aligned(4))) StainU3 { unsigned a, b, c; };            // 12 bytes = 4 pixels, dword aligned
constexpr int STAIN_APPLY_UNROLL = 4;

// VEC: src and dst are dword aligned and a thread moves 4 pixels as three dwords; otherwise byte by byte.  A thread writes only the
// pixels it has read, so dst == src is fine.
template <bool VEC>
__global__ __launch_bounds__(256, 8)                  // 64 registers: 8 workgroups per CU, which is what the launch sizes its grid by
void stain_apply_kernel(const unsigned char* src, unsigned char* dst, int64_t n, const int* __restrict__ od_q, StainTq t,
                        const unsigned char* __restrict__ exp_lut, int lut_len, int lo) {
    __shared__ int od[3 * 256];
    __shared__ unsigned char lut[STAIN_LUT_MAX];      // entries from lut_len on repeat the last one: the clamp is to constants
    const int tid = threadIdx.x, bias = -256 * lo;
    constexpr int last = STAIN_LUT_MAX - 1;
    {
        const int q = od_q[tid];
        od[tid] = q & 0xffff; od[256 + tid] = q << 16; od[512 + tid] = q;
    }
    for (int i = tid; i < STAIN_LUT_MAX / 4; i += 256) {                    // exp_lut is dword aligned (checked by the caller)
        int w;
        if (4 * i + 3 < lut_len) {
            w = ((const int*)exp_lut)[i];
        } else {
            w = 0;
            for (int k = 3; k >= 0; --k) w = (w << 8) | exp_lut[min(4 * i + k, lut_len - 1)];
        }
        ((int*)lut)[i] = w;
    }
    __syncthreads();
    const int64_t groups = VEC ? n / 4 : 0;
    // STAIN_APPLY_UNROLL groups a step apart per thread and turn, all loaded before the first is worked on: a wave keeps that many
    // 768-byte loads in flight (measured: worth one point of the HBM peak over one group per turn).  A group
    // past the end is loaded from the turn's first address instead (no branch around a load) and not stored.
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t q = (int64_t)blockIdx.x * 256 + tid; q < groups; q += STAIN_APPLY_UNROLL * step) {
        StainU3 in[STAIN_APPLY_UNROLL];
#pragma unroll
        for (int u = 0; u < STAIN_APPLY_UNROLL; ++u) in[u] = *(const StainU3*)(src + 12 * (q + u * step < groups ? q + u * step : q));
        __builtin_amdgcn_sched_barrier(0);            // every load is issued before the first use (the scheduler otherwise hoists one)
#pragma unroll
        for (int u = 0; u < STAIN_APPLY_UNROLL; ++u) {
            if (q + u * step >= groups) break;
            // bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
            const unsigned p0 = stain_pixel_out(t, in[u].a & 255, (in[u].a >> 8) & 255, (in[u].a >> 16) & 255, od, lut, bias, last);
            const unsigned p1 = stain_pixel_out(t, in[u].a >> 24, in[u].b & 255, (in[u].b >> 8) & 255, od, lut, bias, last);
            const unsigned p2 = stain_pixel_out(t, (in[u].b >> 16) & 255, in[u].b >> 24, in[u].c & 255, od, lut, bias, last);
            const unsigned p3 = stain_pixel_out(t, (in[u].c >> 8) & 255, (in[u].c >> 16) & 255, in[u].c >> 24, od, lut, bias, last);
            StainU3 o;
            o.a = p0 | (p1 << 24);
            o.b = (p1 >> 8) | (p2 << 16);
            o.c = (p2 >> 16) | (p3 << 8);
            *(StainU3*)(dst + 12 * (q + u * step)) = o;
        }
    }
    for (int64_t i = groups * 4 + (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)gridDim.x * 256) {   // VEC: the < 4 pixels of the tail
        const unsigned p = stain_pixel_out(t, src[3 * i], src[3 * i + 1], src[3 * i + 2], od, lut, bias, last);
        dst[3 * i] = (unsigned char)p;
        dst[3 * i + 1] = (unsigned char)(p >> 8);
        dst[3 * i + 2] = (unsigned char)(p >> 16);
    }
}

}  // namespace keepk
using namespace keepk;

static unsigned stain_grid_for(int64_t items, int per_block, int64_t cap) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (unsigned)(b > cap ? cap : (b < 1 ? 1 : b));
}

static StainView stain_view(const unsigned char* img, int64_t row_stride, int ps, int h, int w, const unsigned char* mask, int64_t mh,
                            int64_t mw, int64_t ds) {
    StainView v;
    v.img = img; v.row = row_stride; v.ps = ps; v.h = h; v.w = w; v.mask = mask; v.mh = mh; v.mw = mw; v.ds = ds;
    return v;
}

// the fit passes keep a histogram or ten 64-bit sums per workgroup: a few pixels per thread and at most 2048 workgroups, so the flush stays small
void launch_stain_moments(const unsigned char* img, int64_t row_stride, int ps, int h, int w, const unsigned char* mask, int64_t mh, int64_t mw,
                          int64_t ds, const int* od_q, int beta_q, int64_t* out, hipStream_t s) {
    const dim3 g(stain_grid_for((int64_t)h * w, 256 * 8, 2048)), b(256);
    hipLaunchKernelGGL(stain_moments_kernel, g, b, 0, s, stain_view(img, row_stride, ps, h, w, mask, mh, mw, ds), od_q, beta_q,
                       (unsigned long long*)out);
}

void launch_stain_angle_hist(const unsigned char* img, int64_t row_stride, int ps, int h, int w, const unsigned char* mask, int64_t mh,
                             int64_t mw, int64_t ds, const int* od_q, int beta_q, const int* v_q, const int* dirs, int* hist, hipStream_t s) {
    StainVq vq;
    for (int i = 0; i < 6; ++i) vq.v[i] = v_q[i];
    const dim3 g(stain_grid_for((int64_t)h * w, 256 * 32, 2048)), b(256);
    hipLaunchKernelGGL(stain_angle_hist_kernel, g, b, 0, s, stain_view(img, row_stride, ps, h, w, mask, mh, mw, ds), od_q, beta_q, vq,
                       (const int2*)dirs, hist);
}

void launch_stain_conc_hist(const unsigned char* img, int64_t row_stride, int ps, int h, int w, const unsigned char* mask, int64_t mh,
                            int64_t mw, int64_t ds, const int* od_q, const int* minv_q, int* hist, hipStream_t s) {
    StainVq mq;
    for (int i = 0; i < 6; ++i) mq.v[i] = minv_q[i];
    const dim3 g(stain_grid_for((int64_t)h * w, 256 * 32, 2048)), b(256);
    hipLaunchKernelGGL(stain_conc_hist_kernel, g, b, 0, s, stain_view(img, row_stride, ps, h, w, mask, mh, mw, ds), od_q, mq, hist);
}

void launch_stain_apply_u8(const unsigned char* src, unsigned char* dst, int64_t n, const int* od_q, const int* t_q, const unsigned char* exp_lut,
                           int lut_len, int lo, hipStream_t s) {
    StainTq t;
    for (int c = 0; c < 3; ++c) {
        const int* q = t_q + 3 * c;
        t.hi_rg[c] = ((q[0] >> 8) & 0xffff) | ((q[1] >> 8) << 16);
        t.lo_rg[c] = (q[0] & 255) | ((q[1] & 255) << 16);
        t.hi_b[c] = q[2] >> 8;
        t.lo_b[c] = q[2] & 255;
    }
    const bool vec = (((uintptr_t)src | (uintptr_t)dst) & 3) == 0;
    // a workgroup stages 11 KiB of tables: as many workgroups as are resident at once (8 per CU) and no more, each with several steps of work
    const dim3 g(stain_grid_for(vec ? (n + 3) / 4 : n, 256 * STAIN_APPLY_UNROLL, 8 * (int64_t)keep_num_cus())), b(256);
    if (vec) hipLaunchKernelGGL(stain_apply_kernel<true>, g, b, 0, s, src, dst, n, od_q, t, exp_lut, lut_len, lo);
    else hipLaunchKernelGGL(stain_apply_kernel<false>, g, b, 0, s, src, dst, n, od_q, t, exp_lut, lut_len, lo);
}
