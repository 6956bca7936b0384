// Segmentation evaluation: the arithmetic of WSI_evaluation/segment_utils.py's eval_seg_auc (the ROC curve of
// the tile scores against the tile labels, its area and the threshold of the best tpr - fpr) and eval_seg_coarse (the overlap counts
// of two masks), and the histogram of a raster's pixel means by truth, from which a threshold sweep follows.  Every result is an
// integer (or, for the best threshold, chosen by IEEE fp64 operations on integers), so it is the same from run to run and equals
// keep_amd.evaluation.roc_numpy / mask_counts_numpy / raster_hist_numpy exactly.
//
//   roc_split         scores -> two arrays of N floats: the positives' scores (NaN elsewhere) and the negatives'.  rank.hip's sort puts
//                     the NaNs last and counts the rest: sp[0:P], sn[0:Nn] ascending, no compaction needed
//   roc_points<MARK>  one thread per sorted element.  A positive adds 2 less + eq (the negatives below / equal to it, two binary
//                     searches) to U2.  The LAST element of a tie group (of sp, or of sn when sp does not hold the value) stands for
//                     its distinct score and marks flags[slot], slot = #{scores < v} over both arrays: distinct scores, distinct slots
//   ev_scan1/2        one exclusive scan over flags: the ascending index of every distinct score, K in all
//   roc_points<EMIT>  the same threads write threshold, tps = P - #{pos < v}, fps = Nn - #{neg < v} at K - 1 - index: descending
//   roc_best          one thread per curve point: kept (first, last, or a non-zero second difference of fps or tps) and, over the kept
//                     points, J = double(tps) / double(P) - double(fps) / double(Nn); per block the largest J, the smallest k among equals
//   roc_final         one block: the blocks' candidates -> the scalars.  (max J, min k) does not depend on the order of the reduction
//   mask_counts       16 pixels per load; non-zero bytes counted by bit tricks on 32-bit words; int64 sums by integer atomics
//   raster_hist       consecutive lanes take consecutive pixels; a wave merges its runs of equal bins (__ballot of the run heads) and
//                     only a run's head adds its length: a heatmap is piecewise constant, so few atomics reach one address.  The
//                     uncovered pixels are counted in registers.  A 2 x 65537 table of int32 is 512 KiB and fits no workgroup's LDS,
//                     hence global returnless atomics rather than a privatised table
//
// Wave64; integer atomics only, none with a used result.
#include "common.h"
#include "../../include/keep_hip.h"

namespace keepk {

struct EvBest { double j; int k; int kept; };           // the best point so far (j = -2: none) and the number of kept points

__device__ __forceinline__ int ev_count(const int64_t* dev, int N) {       // whatever the word holds, the searches stay inside [0, N)
    const int64_t v = *dev;
    return v < 0 ? 0 : (v > N ? N : (int)v);
}

__device__ __forceinline__ int ev_lower(const float* __restrict__ a, int lo, int n, float q) {     // #{a[0:n] < q}, given #{..} >= lo
    int hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < q) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int ev_upper(const float* __restrict__ a, int lo, int n, float q) {     // #{a[0:n] <= q}
    int hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= q) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// 256 threads: the block's sum, valid in every thread.  s: 4 words of LDS, reusable on return
template <typename T>
__device__ __forceinline__ T ev_block_sum(T v, T* s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    const T r = s[0] + s[1] + s[2] + s[3];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256)
void roc_split_kernel(const float* __restrict__ scores, const unsigned char* __restrict__ labels, int N, float* __restrict__ posv,
                      float* __restrict__ negv) {
    const float nan = __uint_as_float(0x7FC00000u);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) {
        const float v = scores[i];
        const bool pos = labels[i] != 0;
        posv[i] = pos ? v : nan;
        negv[i] = pos ? nan : v;
    }
}

// EMIT = false: flags[slot] = 1 for every distinct score and U2 += the positives' 2 less + eq.  EMIT = true: flags holds the scan
// (within chunks of EVAL_SCAN_CHUNK, totals the chunks' offsets) and the curve is written
template <bool EMIT>
__global__ __launch_bounds__(256)
void roc_points_kernel(const float* __restrict__ sp, const float* __restrict__ sn, const int64_t* __restrict__ np_dev,
                       const int64_t* __restrict__ nn_dev, int N, int* __restrict__ flags, const int* __restrict__ totals,
                       unsigned long long* __restrict__ scalars, float* __restrict__ thr, int* __restrict__ fps, int* __restrict__ tps) {
    __shared__ unsigned long long red[4];
    const int P = ev_count(np_dev, N), Nn = ev_count(nn_dev, N);
    const long long K = EMIT ? (long long)scalars[4] : 0;
    unsigned long long u2 = 0;
    const auto point = [&](float v, int lbp, int lbn) {
        const int slot = lbp + lbn;                       // < P + Nn <= N: v itself is not below v
        if (slot >= N) return;
        if (!EMIT) {
            flags[slot] = 1;
        } else {
            const long long k = K - 1 - (flags[slot] + totals[slot / EVAL_SCAN_CHUNK]);
            if (k < 0 || k >= N) return;
            thr[k] = v;
            tps[k] = P - lbp;
            fps[k] = Nn - lbn;
        }
    };
    for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) {
        if (i < P) {
            const float v = sp[i];
            const int lbn = ev_lower(sn, 0, Nn, v);
            if (!EMIT) u2 += (unsigned long long)(lbn + ev_upper(sn, lbn, Nn, v));          // 2 less + eq = less + (less + eq)
            if (i == P - 1 || sp[i + 1] != v) point(v, ev_lower(sp, 0, i, v), lbn);
        }
        if (i < Nn) {
            const float v = sn[i];
            if (i == Nn - 1 || sn[i + 1] != v) {
                const int lbp = ev_lower(sp, 0, P, v);
                if (lbp == P || sp[lbp] != v) point(v, lbp, ev_lower(sn, 0, i, v));
            }
        }
    }
    if (!EMIT) {
        const unsigned long long total = ev_block_sum<unsigned long long>(u2, red);
        if (threadIdx.x == 0 && total) atomicAdd(&scalars[3], total);                         // result unused: a returnless add
    }
}

// exclusive scan inside every chunk of EVAL_SCAN_CHUNK entries, in place; totals[chunk] = the chunk's sum
__global__ __launch_bounds__(256)
void ev_scan1_kernel(int* __restrict__ v, int entries, int* __restrict__ totals) {
    __shared__ int scan[256];
    constexpr int PER = EVAL_SCAN_CHUNK / 256;
    const int first = blockIdx.x * EVAL_SCAN_CHUNK + threadIdx.x * PER;
    int x[PER], sum = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        x[k] = first + k < entries ? v[first + k] : 0;
        sum += x[k];
    }
    int total;
    int run = block_exclusive_scan256(sum, scan, &total);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (first + k < entries) v[first + k] = run;
        run += x[k];
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// one block: exclusive scan of the chunk totals, in place; scalars[4] = K
__global__ __launch_bounds__(256)
void ev_scan2_kernel(int* __restrict__ totals, int chunks, unsigned long long* __restrict__ scalars) {
    __shared__ int scan[256];
    int carry = 0;
    for (int first = 0; first < chunks; first += 256) {
        const int i = first + threadIdx.x;
        const int v = i < chunks ? totals[i] : 0;
        int total;
        const int ex = block_exclusive_scan256(v, scan, &total);
        if (i < chunks) totals[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) scalars[4] = (unsigned long long)carry;
}

__device__ __forceinline__ bool ev_better(double ja, int ka, double jb, int kb) { return ja > jb || (ja == jb && ka < kb); }

// 256 threads: (max j, then min k) and the sum of kept over the block, valid in thread 0
__device__ __forceinline__ EvBest ev_block_best(EvBest b, EvBest* s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double j = __shfl_xor(b.j, o);
        const int k = __shfl_xor(b.k, o);
        b.kept += __shfl_xor(b.kept, o);
        if (ev_better(j, k, b.j, b.k)) { b.j = j; b.k = k; }
    }
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            b.kept += s[w].kept;
            if (ev_better(s[w].j, s[w].k, b.j, b.k)) { b.j = s[w].j; b.k = s[w].k; }
        }
    }
    return b;
}

__global__ __launch_bounds__(256)
void roc_best_kernel(const unsigned long long* __restrict__ scalars, const int64_t* __restrict__ np_dev, const int64_t* __restrict__ nn_dev,
                     int N, const int* __restrict__ fps, const int* __restrict__ tps, unsigned char* __restrict__ kept,
                     EvBest* __restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ EvBest s[4];
    const int P = ev_count(np_dev, N), Nn = ev_count(nn_dev, N);
    const int K = scalars[4] > (unsigned long long)N ? N : (int)scalars[4];
    EvBest b{-2.0, 0x7FFFFFFF, 0};
    for (int k = blockIdx.x * 256 + threadIdx.x; k < K; k += gridDim.x * 256) {
        const int f = fps[k], t = tps[k];
        bool keep = k == 0 || k == K - 1;
        if (!keep) keep = fps[k - 1] - 2 * f + fps[k + 1] != 0 || tps[k - 1] - 2 * t + tps[k + 1] != 0;
        kept[k] = keep;
        if (!keep) continue;
        ++b.kept;
        if (P == 0 || Nn == 0) continue;
        const double j = (double)t / (double)P - (double)f / (double)Nn;               // IEEE: the build has no fast-math
        if (j > b.j) { b.j = j; b.k = k; }                                                // k ascends: the first maximum stays
    }
    b = ev_block_best(b, s);
    if (threadIdx.x == 0) partial[blockIdx.x] = b;
}

// one block.  np_dev null: no scores at all
__global__ __launch_bounds__(256)
void roc_final_kernel(const EvBest* __restrict__ partial, int nparts, const int64_t* __restrict__ np_dev, const int64_t* __restrict__ nn_dev, int N,
                      const float* __restrict__ thr, unsigned long long* __restrict__ scalars) {
    __shared__ EvBest s[4];
    EvBest b{-2.0, 0x7FFFFFFF, 0};
    for (int i = threadIdx.x; i < nparts; i += 256) {
        const EvBest p = partial[i];
        b.kept += p.kept;
        if (ev_better(p.j, p.k, b.j, b.k)) { b.j = p.j; b.k = p.k; }
    }
    b = ev_block_best(b, s);
    if (threadIdx.x != 0) return;
    const int P = np_dev ? ev_count(np_dev, N) : 0, Nn = np_dev ? ev_count(nn_dev, N) : 0;
    const bool found = b.j > 0.0 && b.k >= 0 && b.k < N;                                 // else the point (0, 0) that roc_curve prepends: inf
    scalars[0] = (unsigned long long)(P + Nn);
    scalars[1] = (unsigned long long)P;
    scalars[2] = (unsigned long long)Nn;
    scalars[5] = found ? (unsigned long long)b.k : ~0ull;
    scalars[6] = found ? (unsigned long long)__float_as_uint(thr[b.k]) : 0x7F800000ull;
    scalars[7] = (unsigned long long)b.kept;
}

// ---- mask overlap ---------------------------------------------------------------------------------------------------------------------------
// bit 7 of every byte of w that is not zero
__device__ __forceinline__ unsigned ev_nz(unsigned w) { return (((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u; }

__global__ __launch_bounds__(256)
void mask_counts_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, const unsigned char* __restrict__ within,
                        long long n, int vec, unsigned long long* __restrict__ out) {
    __shared__ unsigned red[4];
    unsigned ca = 0, cb = 0, cab = 0, cw = 0;                 // a thread sees at most 2^30 / 256 pixels
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
    const long long nv = vec ? n / 16 : 0;
    for (long long i = t; i < nv; i += step) {
        const uint4 va = reinterpret_cast<const uint4*>(a)[i], vb = reinterpret_cast<const uint4*>(b)[i];
        uint4 vw = make_uint4(~0u, ~0u, ~0u, ~0u);
        if (within) vw = reinterpret_cast<const uint4*>(within)[i];
        const unsigned wa[4] = {va.x, va.y, va.z, va.w}, wb[4] = {vb.x, vb.y, vb.z, vb.w}, ww[4] = {vw.x, vw.y, vw.z, vw.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned mw = ev_nz(ww[k]), ma = ev_nz(wa[k]) & mw, mb = ev_nz(wb[k]) & mw;
            ca += __popc(ma); cb += __popc(mb); cab += __popc(ma & mb); cw += __popc(mw);
        }
    }
    for (long long i = nv * 16 + t; i < n; i += step) {
        if (within && !within[i]) continue;
        const bool sa = a[i] != 0, sb = b[i] != 0;
        ca += sa; cb += sb; cab += sa && sb; ++cw;
    }
    const unsigned sums[4] = {ev_block_sum<unsigned>(ca, red), ev_block_sum<unsigned>(cb, red), ev_block_sum<unsigned>(cab, red),
                              ev_block_sum<unsigned>(cw, red)};      // a block sees at most 2^30 pixels
    if (threadIdx.x < 4 && sums[threadIdx.x]) atomicAdd(&out[threadIdx.x], (unsigned long long)sums[threadIdx.x]);   // returnless
}

// ---- raster histogram -------------------------------------------------------------------------------------------------------------------------
// the pixel's mean on 0..65535, rounded half up: (2 S + c) / (2 c) for c > 0 (peak16's rule, components.hip), and never above 65535
// whatever the word holds: the bin stays inside the table
__device__ __forceinline__ int ev_mean16(long long S, long long c) {
    const long long num = 2 * S + c, den = 2 * c;
    long long q = (long long)((double)num / (double)den);
    const long long r = num - q * den;
    if (r < 0) --q;
    else if (r >= den) ++q;
    return (int)(q < 0 ? 0 : (q > 65535 ? 65535 : q));
}

__global__ __launch_bounds__(256)
void raster_hist_kernel(const long long* __restrict__ acc, const unsigned char* __restrict__ truth, const unsigned char* __restrict__ within,
                        long long n, unsigned long long* __restrict__ hist) {
    __shared__ unsigned red[4];
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), waves = (long long)gridDim.x * 4;
    unsigned unc0 = 0, unc1 = 0;                              // uncovered pixels by truth: at most 2^30 in all
    for (long long base = wave * 64; base < n; base += waves * 64) {      // the bound is the wave's: every lane takes part in the ballots
        const long long p = base + lane;
        int bin = -1;                                         // outside the image or outside `within`: counted nowhere
        if (p < n && (!within || within[p])) {
            const unsigned long long word = (unsigned long long)acc[p];
            const long long c = (long long)(word >> 40), S = (long long)(word & ((1ull << 40) - 1));
            bin = (truth[p] != 0 ? EVAL_HIST_BINS : 0) + (c > 0 ? ev_mean16(S, c) : EVAL_HIST_BINS - 1);
        }
        const int before = __shfl_up(bin, 1);
        const bool head = lane == 0 || before != bin;
        const unsigned long long heads = __ballot(head);
        if (head && bin >= 0) {
            const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
            const unsigned len = above ? (unsigned)__ffsll((unsigned long long)above) : (unsigned)(64 - lane);
            if (bin == EVAL_HIST_BINS - 1) unc0 += len;
            else if (bin == 2 * EVAL_HIST_BINS - 1) unc1 += len;
            else atomicAdd(&hist[bin], (unsigned long long)len);                          // returnless
        }
    }
    const unsigned s0 = ev_block_sum<unsigned>(unc0, red), s1 = ev_block_sum<unsigned>(unc1, red);
    if (threadIdx.x == 0) {
        if (s0) atomicAdd(&hist[EVAL_HIST_BINS - 1], (unsigned long long)s0);
        if (s1) atomicAdd(&hist[2 * EVAL_HIST_BINS - 1], (unsigned long long)s1);
    }
}

}  // namespace keepk
using namespace keepk;

static inline size_t ev_align(size_t b) { return (b + 255) & ~(size_t)255; }
static int ev_chunks(int64_t N) { return (int)((N + EVAL_SCAN_CHUNK - 1) / EVAL_SCAN_CHUNK); }

namespace {
struct RocWs {
    float *sp, *sn;
    int64_t* counts;                                          // P, Nn
    unsigned char* sort;
    int *flags, *totals;
    EvBest* partial;
    float* thr; int *fps, *tps; unsigned char* kept;          // the curve, when the caller takes none
    size_t bytes;
};
RocWs roc_carve(unsigned char* ws, int64_t N, bool own_curve) {
    size_t at = 0;
    auto take = [&](size_t bytes) { unsigned char* p = ws + at; at += ev_align(bytes); return p; };
    size_t table_off, totals_off;
    RocWs r;
    r.sp = (float*)take((size_t)N * 4);
    r.sn = (float*)take((size_t)N * 4);
    r.counts = (int64_t*)take(16);
    r.sort = take(sort_workspace_bytes(N, &table_off, &totals_off));
    r.flags = (int*)take((size_t)N * 4);
    r.totals = (int*)take((size_t)ev_chunks(N) * 4);
    r.partial = (EvBest*)take((size_t)EVAL_BEST_BLOCKS * sizeof(EvBest));
    r.thr = (float*)take(own_curve ? (size_t)N * 4 : 0);
    r.fps = (int*)take(own_curve ? (size_t)N * 4 : 0);
    r.tps = (int*)take(own_curve ? (size_t)N * 4 : 0);
    r.kept = take(own_curve ? (size_t)N : 0);
    r.bytes = at;
    return r;
}
}  // namespace

size_t eval_roc_workspace_bytes(int64_t N, bool own_curve) { return N < 1 ? 0 : roc_carve(nullptr, N, own_curve).bytes; }

void launch_eval_roc(const float* scores, const unsigned char* labels, int64_t N64, unsigned char* ws, int64_t* scalars, float* thr, int* fps,
                     int* tps, unsigned char* kept, hipStream_t s) {
    unsigned long long* sc = reinterpret_cast<unsigned long long*>(scalars);
    (void)hipMemsetAsync(sc, 0, EVAL_ROC_SCALARS * 8, s);
    const int N = (int)N64;
    if (N < 1) {
        hipLaunchKernelGGL(roc_final_kernel, dim3(1), dim3(256), 0, s, (const EvBest*)nullptr, 0, (const int64_t*)nullptr, (const int64_t*)nullptr, 0,
                           (const float*)nullptr, sc);
        return;
    }
    const RocWs w = roc_carve(ws, N, thr == nullptr);
    if (!thr) { thr = w.thr; fps = w.fps; tps = w.tps; kept = w.kept; }
    const int blocks = (int)std::min<int64_t>((N64 + 255) / 256, 16384), chunks = ev_chunks(N);
    const int best_blocks = std::min(blocks, EVAL_BEST_BLOCKS);
    hipLaunchKernelGGL(roc_split_kernel, dim3(blocks), dim3(256), 0, s, scores, labels, N, w.sp, w.sn);
    launch_sort_f32(w.sp, N, w.sort, w.sp, w.counts, s);              // in place: the sort reads its input in the first pass only
    launch_sort_f32(w.sn, N, w.sort, w.sn, w.counts + 1, s);
    (void)hipMemsetAsync(w.flags, 0, (size_t)N * 4, s);
    hipLaunchKernelGGL(roc_points_kernel<false>, dim3(blocks), dim3(256), 0, s, (const float*)w.sp, (const float*)w.sn, (const int64_t*)w.counts,
                       (const int64_t*)(w.counts + 1), N, w.flags, (const int*)nullptr, sc, thr, fps, tps);
    hipLaunchKernelGGL(ev_scan1_kernel, dim3(chunks), dim3(256), 0, s, w.flags, N, w.totals);
    hipLaunchKernelGGL(ev_scan2_kernel, dim3(1), dim3(256), 0, s, w.totals, chunks, sc);
    hipLaunchKernelGGL(roc_points_kernel<true>, dim3(blocks), dim3(256), 0, s, (const float*)w.sp, (const float*)w.sn, (const int64_t*)w.counts,
                       (const int64_t*)(w.counts + 1), N, w.flags, (const int*)w.totals, sc, thr, fps, tps);
    hipLaunchKernelGGL(roc_best_kernel, dim3(best_blocks), dim3(256), 0, s, (const unsigned long long*)sc, (const int64_t*)w.counts,
                       (const int64_t*)(w.counts + 1), N, (const int*)fps, (const int*)tps, kept, w.partial);
    hipLaunchKernelGGL(roc_final_kernel, dim3(1), dim3(256), 0, s, (const EvBest*)w.partial, best_blocks, (const int64_t*)w.counts,
                       (const int64_t*)(w.counts + 1), N, (const float*)thr, sc);
}

void launch_eval_mask_counts(const unsigned char* a, const unsigned char* b, const unsigned char* within, int64_t n, int64_t* out, hipStream_t s) {
    (void)hipMemsetAsync(out, 0, 4 * 8, s);
    const int vec = !(((uintptr_t)a | (uintptr_t)b | (uintptr_t)within) & 15);
    const int64_t items = vec ? (n + 15) / 16 : n;
    const int blocks = (int)std::min<int64_t>((items + 255) / 256, 4096);
    hipLaunchKernelGGL(mask_counts_kernel, dim3(blocks), dim3(256), 0, s, a, b, within, (long long)n, vec, reinterpret_cast<unsigned long long*>(out));
}

void launch_eval_raster_hist(const int64_t* acc, const unsigned char* truth, const unsigned char* within, int64_t n, int64_t* hist, hipStream_t s) {
    (void)hipMemsetAsync(hist, 0, (size_t)2 * EVAL_HIST_BINS * 8, s);
    const int blocks = (int)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(raster_hist_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const long long*>(acc), truth, within, (long long)n,
                       reinterpret_cast<unsigned long long*>(hist));
}
