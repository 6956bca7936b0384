// Lesion-level scoring: the three device steps of a CAMELYON16-style FROC analysis that sections 10-17 lack.
// Every result is an integer, so it is the same from run to run and equals keep_amd.lesion.dist2_numpy / peaks_numpy /
// lesion_hits_numpy exactly.
//
//   dist_cols         g(y, x) = min(rows to the nearest set pixel of column x, R + 1) as uint16.  One thread per column and band of rows:
//                     a counter runs down from R rows above the band and up from R rows below it, so consecutive lanes read consecutive
//                     bytes of one row
//   dist_rows         d2(y, x) = min over |dx| <= R of g(y, x + dx)^2 + dx^2, capped at R^2 + 1.  A block stages a row segment of g with its
//                     halo of R on either side (clipped to the image) in LDS; one thread per pixel walks outwards and stops when dx^2
//                     reaches its best.  Narrow images (W <= 128) put several rows into one block
//   peak_rows         key(p) = (m + 1) << 32 | (0xFFFFFFFF - p) for an eligible pixel, 0 otherwise; the plane of the maxima over |dx| <= r,
//                     from a row segment and its halo in LDS
//   peak_cols<WRITE>  the maximum of that plane over |dy| <= r is the window's best key; a pixel is a peak iff the low word of it names
//                     the pixel itself and m >= min16.  2048 pixels per block.  WRITE = false: the block's number of peaks; WRITE = true:
//                     the rows (x, y, m) at the block's offset + the rank inside the block (ballots, no atomic append): row-major order
//   peak_scan         one block: exclusive scan of the blocks' counts, *n_out = their sum
//   lesion_hits       one thread per candidate: floor division into the label image, then the lanes of a wave that share a label reduce
//                     their score bits and the first of them issues one returnless atomicMax.  Maxima commute
//
// Wave64; integer atomics only, none with a used result.
#include "common.h"
#include "../../include/keep_hip.h"

namespace keepk {

constexpr int LS_SEG = 256;                                   // pixels of a row segment (and threads of every block here)
constexpr int LS_DIST_LDS = LS_SEG + 2 * 1024;                // uint16 entries: a segment and its halo at the largest radius
constexpr int LS_PEAK_LDS = LS_SEG + 2 * 127;                 // 64-bit keys
constexpr int LS_CHUNK = 2048;                                // pixels per block of the compaction
constexpr int LS_PER = LS_CHUNK / 256;

// A block of 256 threads covers `rows` rows x `segw` columns, segw a power of two: 256 x 1 unless the image is narrower than 129
struct LsTile { int segw, rows, xsegs; };

// the pixel's mean on 0..65535, rounded half up: (2 S + c) / (2 c) for c > 0 (peak16's rule), and never above 65535 whatever the word holds
__device__ __forceinline__ int ls_mean16(long long S, long long c) {
    const long long num = 2 * S + c, den = 2 * c;
    long long q = (long long)((double)num / (double)den);
    const long long r = num - q * den;
    if (r < 0) --q;
    else if (r >= den) ++q;
    return (int)(q < 0 ? 0 : (q > 65535 ? 65535 : q));
}

// ---- distance transform ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void dist_cols_kernel(const unsigned char* __restrict__ mask, int H, int W, int R, int invert, int band, int xblocks,
                      unsigned short* __restrict__ g) {
    const int x = (int)(blockIdx.x % (unsigned)xblocks) * 256 + threadIdx.x;
    const long long y0 = (long long)(blockIdx.x / (unsigned)xblocks) * band;
    if (x >= W || y0 >= H) return;
    const int y1 = (int)(y0 + band < H ? y0 + band : H);                    // the band is rows [y0, y1)
    const int far = R + 1;
    int d = far;
    for (int y = (int)(y0 - R > 0 ? y0 - R : 0); y < y1; ++y) {
        const bool set = (mask[(size_t)y * W + x] != 0) != (invert != 0);
        d = set ? 0 : (d < far ? d + 1 : far);
        if (y >= y0) g[(size_t)y * W + x] = (unsigned short)d;
    }
    d = far;
    for (int y = (y1 - 1 + R < H - 1 ? y1 - 1 + R : H - 1); y >= y0; --y) {
        const bool set = (mask[(size_t)y * W + x] != 0) != (invert != 0);
        d = set ? 0 : (d < far ? d + 1 : far);
        if (y < y1 && d < (int)g[(size_t)y * W + x]) g[(size_t)y * W + x] = (unsigned short)d;      // the thread's own store above
    }
}

__global__ __launch_bounds__(256)
void dist_rows_kernel(const unsigned short* __restrict__ g, int H, int W, int R, LsTile t, unsigned* __restrict__ out) {
    __shared__ unsigned short row[LS_DIST_LDS];
    const int slot = threadIdx.x / t.segw, col = threadIdx.x % t.segw;
    const int x0 = (int)(blockIdx.x % (unsigned)t.xsegs) * t.segw;
    const long long y = (long long)(blockIdx.x / (unsigned)t.xsegs) * t.rows + slot;
    const int lo = x0 - R > 0 ? x0 - R : 0, hi = x0 + t.segw + R < W ? x0 + t.segw + R : W;        // the staged columns [lo, hi)
    const int stride = t.segw + 2 * R < W ? t.segw + 2 * R : W;                                  // >= hi - lo; rows * stride <= LS_DIST_LDS
    unsigned short* mine = row + slot * stride;
    if (y < H)
        for (int xx = lo + col; xx < hi; xx += t.segw) mine[xx - lo] = g[(size_t)y * W + xx];
    __syncthreads();
    const int x = x0 + col;
    if (y >= H || x >= W) return;
    const unsigned cap = (unsigned)R * (unsigned)R + 1u;
    const unsigned g0 = mine[x - lo];
    unsigned best = g0 * g0 < cap ? g0 * g0 : cap;
    for (int dx = 1; dx <= R; ++dx) {
        const unsigned dx2 = (unsigned)dx * (unsigned)dx;
        if (dx2 >= best) break;
        if (x - dx >= lo) {
            const unsigned v = mine[x - dx - lo];
            best = v * v + dx2 < best ? v * v + dx2 : best;
        }
        if (x + dx < hi) {
            const unsigned v = mine[x + dx - lo];
            best = v * v + dx2 < best ? v * v + dx2 : best;
        }
    }
    out[(size_t)y * W + x] = best;
}

// ---- peaks -----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void peak_rows_kernel(const long long* __restrict__ acc, const unsigned char* __restrict__ mask, int H, int W, int r, LsTile t,
                      unsigned long long* __restrict__ rowmax) {
    __shared__ unsigned long long keys[LS_PEAK_LDS];
    const int slot = threadIdx.x / t.segw, col = threadIdx.x % t.segw;
    const int x0 = (int)(blockIdx.x % (unsigned)t.xsegs) * t.segw;
    const long long y = (long long)(blockIdx.x / (unsigned)t.xsegs) * t.rows + slot;
    const int lo = x0 - r > 0 ? x0 - r : 0, hi = x0 + t.segw + r < W ? x0 + t.segw + r : W;
    const int stride = t.segw + 2 * r < W ? t.segw + 2 * r : W;
    unsigned long long* mine = keys + slot * stride;
    if (y < H)
        for (int xx = lo + col; xx < hi; xx += t.segw) {
            const size_t p = (size_t)y * W + xx;
            const unsigned long long word = (unsigned long long)acc[p];
            const long long c = (long long)(word >> 40), S = (long long)(word & ((1ull << 40) - 1));
            unsigned long long key = 0;
            if (c > 0 && (!mask || mask[p])) key = ((unsigned long long)(ls_mean16(S, c) + 1) << 32) | (0xFFFFFFFFull - (unsigned long long)p);
            mine[xx - lo] = key;
        }
    __syncthreads();
    const int x = x0 + col;
    if (y >= H || x >= W) return;
    const int a = x - r > lo ? x - r : lo, b = x + r < hi - 1 ? x + r : hi - 1;
    unsigned long long best = 0;
    for (int xx = a; xx <= b; ++xx) {
        const unsigned long long k = mine[xx - lo];
        best = k > best ? k : best;
    }
    rowmax[(size_t)y * W + x] = best;
}

template <bool WRITE>
__global__ __launch_bounds__(256)
void peak_cols_kernel(const unsigned long long* __restrict__ rowmax, int H, int W, int r, int min16, int* __restrict__ counts,
                      const int* __restrict__ offsets, long long max_peaks, long long* __restrict__ peaks) {
    __shared__ int waves[LS_PER * 4];
    const long long n = (long long)H * W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int m[LS_PER], before[LS_PER];
    unsigned found = 0;
#pragma unroll
    for (int k = 0; k < LS_PER; ++k) {                                      // every lane takes part in the ballot: no early exit
        const long long p = (long long)blockIdx.x * LS_CHUNK + k * 256 + threadIdx.x;
        bool peak = false;
        m[k] = 0;
        if (p < n) {
            const int y = (int)(p / W);
            const int ya = y - r > 0 ? y - r : 0, yb = y + r < H - 1 ? y + r : H - 1;
            unsigned long long best = 0;
            for (int yy = ya; yy <= yb; ++yy) {
                const unsigned long long v = rowmax[p + (long long)(yy - y) * W];
                best = v > best ? v : best;
            }
            m[k] = (int)(best >> 32) - 1;
            peak = best != 0 && (unsigned)best == 0xFFFFFFFFu - (unsigned)p && m[k] >= min16;
        }
        const unsigned long long votes = __ballot(peak);
        before[k] = __popcll(votes & ((1ull << lane) - 1));
        if (peak) found |= 1u << k;
        if (lane == 0) waves[k * 4 + wave] = __popcll(votes);
    }
    __syncthreads();
    if (!WRITE) {
        if (threadIdx.x == 0) {
            int total = 0;
            for (int i = 0; i < LS_PER * 4; ++i) total += waves[i];
            counts[blockIdx.x] = total;
        }
        return;
    }
    if (!found) return;
    long long at = offsets[blockIdx.x];
#pragma unroll
    for (int k = 0; k < LS_PER; ++k) {
        long long mine = at + before[k];
        for (int w = 0; w < 4; ++w) {
            if (w < wave) mine += waves[k * 4 + w];
            at += waves[k * 4 + w];
        }
        if (((found >> k) & 1u) && mine < max_peaks) {
            const long long p = (long long)blockIdx.x * LS_CHUNK + k * 256 + threadIdx.x;
            peaks[3 * mine] = p % W;
            peaks[3 * mine + 1] = p / W;
            peaks[3 * mine + 2] = m[k];
        }
    }
}

// one block: exclusive scan of the blocks' counts; *n_out = the number of peaks
__global__ __launch_bounds__(256)
void peak_scan_kernel(const int* __restrict__ counts, int nblocks, int* __restrict__ offsets, long long* __restrict__ n_out) {
    __shared__ int scan[256];
    int carry = 0;
    for (int first = 0; first < nblocks; first += 256) {
        const int i = first + threadIdx.x;
        const int v = i < nblocks ? counts[i] : 0;
        int total;
        const int ex = block_exclusive_scan256(v, scan, &total);
        if (i < nblocks) offsets[i] = carry + ex;
        carry += total;                                                   // at most H W <= 2^30
    }
    if (threadIdx.x == 0) *n_out = carry;
}

// ---- candidates against the label image ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long ls_floor_div(long long a, long long d) {      // d >= 1
    const long long q = a / d;
    return a % d < 0 ? q - 1 : q;
}

__global__ __launch_bounds__(256)
void lesion_hits_kernel(const long long* __restrict__ xy, const float* __restrict__ scores, int N, const int* __restrict__ labels, int Hm, int Wm,
                        long long d, long long ox, long long oy, int n_labels, const unsigned char* __restrict__ ignore, int* __restrict__ hit,
                        unsigned* __restrict__ lesion_max) {
    const int lane = threadIdx.x & 63;
    for (long long base = (long long)blockIdx.x * 256; base < N; base += (long long)gridDim.x * 256) {    // the bound is the block's: every lane stays for the ballots
        const long long i = base + threadIdx.x;
        int label = 0;
        unsigned bits = 0;
        bool active = false;
        if (i < N) {
            const float s = scores[i];
            const long long px = ls_floor_div(xy[2 * i] - ox, d), py = ls_floor_div(xy[2 * i + 1] - oy, d);
            if (px >= 0 && px < Wm && py >= 0 && py < Hm) {
                const int v = labels[(size_t)py * Wm + px];
                if (v >= 1 && v <= n_labels) label = v;
            }
            const unsigned raw = __float_as_uint(s);
            const bool nan = (raw & 0x7FFFFFFFu) > 0x7F800000u;
            hit[i] = nan ? -1 : label;
            bits = (raw >> 31) ? 0u : raw;                                     // max(s, +0.0): -0.0 and the negatives give 0
            active = !nan && label > 0 && bits != 0 && !(ignore && ignore[label - 1]);      // a maximum with 0 changes nothing
        }
        for (;;) {
            const unsigned long long todo = __ballot(active);
            if (!todo) break;
            const int leader = __ffsll(todo) - 1;
            const int theirs = __shfl(label, leader);
            const bool same = active && label == theirs;
            unsigned v = same ? bits : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned u = __shfl_xor(v, o);
                v = u > v ? u : v;
            }
            if (lane == leader) atomicMax(&lesion_max[theirs - 1], v);        // returnless
            active = active && !same;
        }
    }
}

}  // namespace keepk
using namespace keepk;

static LsTile ls_tile(int H, int W) {
    LsTile t;
    t.segw = LS_SEG;
    if (W <= LS_SEG / 2) {
        t.segw = 1;
        while (t.segw < W) t.segw *= 2;
    }
    t.rows = LS_SEG / t.segw;
    t.xsegs = (W + t.segw - 1) / t.segw;
    return t;
}
static unsigned ls_tile_blocks(const LsTile& t, int H) { return (unsigned)(((int64_t)H + t.rows - 1) / t.rows * t.xsegs); }
static inline size_t ls_align(size_t b) { return (b + 255) & ~(size_t)255; }

size_t mask_dist2_workspace_bytes(int64_t npix) { return ls_align((size_t)npix * 2); }

void launch_mask_dist2(const unsigned char* mask, int H, int W, int R, int invert, unsigned char* ws, unsigned* out, hipStream_t s) {
    unsigned short* g = reinterpret_cast<unsigned short*>(ws);
    const int band = R < 32 ? 32 : R;                                       // a thread reads band + 2 R rows for its band
    const int xblocks = (W + 255) / 256;
    const unsigned bands = (unsigned)(((int64_t)H + band - 1) / band);
    hipLaunchKernelGGL(dist_cols_kernel, dim3((unsigned)xblocks * bands), dim3(256), 0, s, mask, H, W, R, invert, band, xblocks, g);
    const LsTile t = ls_tile(H, W);
    hipLaunchKernelGGL(dist_rows_kernel, dim3(ls_tile_blocks(t, H)), dim3(256), 0, s, (const unsigned short*)g, H, W, R, t, out);
}

static int ls_chunks(int64_t npix) { return (int)((npix + LS_CHUNK - 1) / LS_CHUNK); }

size_t raster_peaks_workspace_bytes(int64_t npix) { return ls_align((size_t)npix * 8) + 2 * ls_align((size_t)ls_chunks(npix) * 4); }

void launch_raster_peaks(const int64_t* acc, const unsigned char* mask, int H, int W, int r, int min16, int64_t max_peaks, unsigned char* ws,
                         int64_t* peaks, int64_t* n_out, hipStream_t s) {
    const int64_t npix = (int64_t)H * W;
    const int chunks = ls_chunks(npix);
    unsigned long long* rowmax = reinterpret_cast<unsigned long long*>(ws);
    int* counts = reinterpret_cast<int*>(ws + ls_align((size_t)npix * 8));
    int* offsets = reinterpret_cast<int*>(ws + ls_align((size_t)npix * 8) + ls_align((size_t)chunks * 4));
    const LsTile t = ls_tile(H, W);
    hipLaunchKernelGGL(peak_rows_kernel, dim3(ls_tile_blocks(t, H)), dim3(256), 0, s, reinterpret_cast<const long long*>(acc), mask, H, W, r, t, rowmax);
    hipLaunchKernelGGL(peak_cols_kernel<false>, dim3(chunks), dim3(256), 0, s, (const unsigned long long*)rowmax, H, W, r, min16, counts,
                       (const int*)nullptr, (long long)0, (long long*)nullptr);
    hipLaunchKernelGGL(peak_scan_kernel, dim3(1), dim3(256), 0, s, (const int*)counts, chunks, offsets, reinterpret_cast<long long*>(n_out));
    if (max_peaks > 0)
        hipLaunchKernelGGL(peak_cols_kernel<true>, dim3(chunks), dim3(256), 0, s, (const unsigned long long*)rowmax, H, W, r, min16, counts,
                           (const int*)offsets, (long long)max_peaks, reinterpret_cast<long long*>(peaks));
}

void launch_lesion_hits(const int64_t* xy, const float* scores, int64_t N, const int* labels, int Hm, int Wm, int64_t d, int64_t ox, int64_t oy,
                        int n_labels, const unsigned char* ignore, int* hit, unsigned* lesion_max, hipStream_t s) {
    if (n_labels > 0) (void)hipMemsetAsync(lesion_max, 0, (size_t)n_labels * 4, s);
    if (N < 1) return;
    const int blocks = (int)std::min<int64_t>((N + 255) / 256, 2048);
    hipLaunchKernelGGL(lesion_hits_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const long long*>(xy), scores, (int)N, labels, Hm, Wm,
                       (long long)d, (long long)ox, (long long)oy, n_labels, ignore, hit, lesion_max);
}
