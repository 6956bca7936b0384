// Tissue segmentation of a slide thumbnail and the patch grid decided by its mask.  Integer arithmetic
// throughout: every result is held exactly to keep_amd.region.tissue_mask_numpy / mask_grid_numpy.
//
//   tissue_median_hist<K>   uint8 RGB / RGBA thumbnail -> HSV saturation (0..255, rounded half up) in an LDS tile with a K/2 halo
//                           (border replicated) -> K x K median per pixel by an 8-step bitwise search that counts window values
//                           >= the candidate (registers only) -> median bytes + a 256-bin histogram (LDS integer atomics, one
//                           global integer add per used bin per workgroup: integer sums do not depend on the order)
//   tissue_box              one separable pass of the closing: row / column max (outside = 0) or min (outside = 1) over the window
//                           [x - a, x + c - 1 - a]; the first pass thresholds the median bytes as it reads them
//   cc_init / cc_merge /    connected components, templated on polarity (foreground / background) and connectivity (8 / 4):
//   cc_compress / cc_count  union-find on global int32 labels whose roots are the SMALLEST linear pixel index of their set, so
//                           the labels do not depend on the order in which the merges land.  init labels every pixel with the
//                           start of its horizontal run inside its 64-pixel wave segment (one ballot, no memory traffic);
//                           merge joins runs across segment borders and rows by atomicMin; compress points every pixel at
//                           its root; count adds the areas (one integer atomic per distinct root per wave) and ORs the
//                           border-contact bit.  A fixed number of launches; every find / merge loop is capped by the pixel
//                           count (a chain of strictly decreasing indices cannot be longer) and sets error value 4 if it runs out.
//   cc_fill_holes /         step 5: background components that touch no border and hold <= min_hole pixels become foreground;
//   cc_drop_small           step 6: foreground components of <= min_area pixels are cleared
//   tissue_grid_cells       one thread per grid cell: CLAM's four_pt / four_pt_hard / center test on the mask (at most four byte
//                           loads) -> keep flags for region.hip's stable compaction
//
// Pixel indices are int32 (H W <= 2^30, checked by the caller); every kernel walks 64 x 4 pixel tiles, one wave per row, in a
// grid-stride loop, so a wave always holds 64 consecutive pixels of one row.
#include "common.h"
#include "labelling.h"
#include "../../include/keep_hip.h"

namespace keepk {

__device__ __forceinline__ unsigned tissue_saturation(unsigned r, unsigned g, unsigned b) {
    const unsigned mx = max(r, max(g, b)), mn = min(r, min(g, b));
    return mx ? (510u * (mx - mn) + mx) / (2u * mx) : 0u;
}

constexpr int MED_TW = 64, MED_TH = 16;               // output tile of one workgroup: 4 waves x 4 rows each

template <int K>
__global__ __launch_bounds__(256)
void tissue_median_hist_kernel(const unsigned char* __restrict__ thumb, int64_t row_stride, int ps, int h, int w,
                               unsigned char* __restrict__ med, int* __restrict__ hist) {
    constexpr int R = K / 2, LW = MED_TW + 2 * R, LH = MED_TH + 2 * R, NEED = (K * K + 1) / 2;
    __shared__ unsigned char sat[LH][LW + 2];
    __shared__ int bins[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    bins[tid] = 0;
    const int tx = (w + MED_TW - 1) / MED_TW, ty = (h + MED_TH - 1) / MED_TH;
    const int64_t ntiles = (int64_t)tx * ty;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int x0 = (int)(t % tx) * MED_TW, y0 = (int)(t / tx) * MED_TH;
        __syncthreads();                              // the previous tile's window reads (and the zeroing of bins) are done
        for (int i = tid; i < LH * LW; i += 256) {
            const int ly = i / LW, lx = i - ly * LW;
            const int gy = min(max(y0 + ly - R, 0), h - 1), gx = min(max(x0 + lx - R, 0), w - 1);
            const unsigned char* p = thumb + (int64_t)gy * row_stride + (int64_t)gx * ps;
            sat[ly][lx] = (unsigned char)tissue_saturation(p[0], p[1], p[2]);
        }
        __syncthreads();
        const int x = x0 + lane;
        for (int j = 0; j < 4; ++j) {
            const int ly = wave * 4 + j, y = y0 + ly;
            if (x >= w || y >= h) continue;
            unsigned res = 0;
            if (K == 1) {
                res = sat[ly][lane];
            } else {
                // the median is the largest v with #{window >= v} >= NEED; found bit by bit from the top
                for (unsigned bit = 128; bit; bit >>= 1) {
                    const unsigned c = res | bit;
                    int n = 0;
                    for (int dy = 0; dy < K; ++dy) {
#pragma unroll
                        for (int dx = 0; dx < K; ++dx) n += sat[ly + dy][lane + dx] >= c;
                    }
                    if (n >= NEED) res = c;
                }
            }
            med[(int64_t)y * w + x] = (unsigned char)res;
            atomicAdd(&bins[res], 1);
        }
    }
    __syncthreads();
    if (bins[tid]) atomicAdd(&hist[tid], bins[tid]);
}

// out = max (is_min = 0; outside the image = 0) or min (is_min = 1; outside = 1) of in over [q - a, q + c - 1 - a] along x
// (horizontal) or y; thr >= 0: `in` holds median bytes and a pixel counts as 1 iff in > thr, else `in` is already {0, 1}
__global__ __launch_bounds__(256)
void tissue_box_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, int h, int w, int c, int a, int horizontal,
                       int is_min, int thr) {
    const int n = h * w;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
        const int q = horizontal ? x : y, dim = horizontal ? w : h;
        const int lo = max(q - a, 0), hi = min(q + c - 1 - a, dim - 1);
        const int64_t stride = horizontal ? 1 : w;
        const unsigned char* p = in + (horizontal ? (int64_t)y * w : (int64_t)x);
        int v = is_min;
        for (int k = lo; k <= hi; ++k) {
            const int u = p[k * stride];
            const int b = thr >= 0 ? u > thr : u != 0;
            v = is_min ? (v & b) : (v | b);
        }
        out[i] = (unsigned char)v;
    }
}

// ---- connected components --------------------------------------------------------------------------------------------------
__device__ __forceinline__ int cc_load(const int* L, int x) { return __hip_atomic_load(L + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x (labels only ever decrease and L[x] <= x, so a chain has fewer than n links); -1 and the error bit at the cap
__device__ __forceinline__ int cc_find(const int* L, int x, int n, int* err) {
    for (int it = 0; it <= n; ++it) {
        const int p = cc_load(L, x);
        if (p == x) return x;
        x = p;
    }
    atomicOr(err, TISSUE_ERR_BIT);
    return -1;
}

// join the sets of a and b: the larger root is hung under the smaller one by atomicMin; if another thread got there first, go on
// with the parent it installed.  Every retry means some label has decreased, which can happen fewer than n times per pixel.
__device__ __forceinline__ void cc_union(int* L, int a, int b, int n, int* err) {
    for (int it = 0; it <= n; ++it) {
        a = cc_find(L, a, n, err);
        b = cc_find(L, b, n, err);
        if (a < 0 || b < 0 || a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(L + a, b);
        if (old == a) return;
        a = old;
    }
    atomicOr(err, TISSUE_ERR_BIT);
}

template <bool FG>
__global__ __launch_bounds__(256)
void cc_init_kernel(const unsigned char* __restrict__ img, int h, int w, int* __restrict__ L, int* __restrict__ info) {
    const CcWalk walk(h, w);
    const int lane = threadIdx.x & 63;
    for (int64_t t = blockIdx.x; t < walk.ntiles; t += gridDim.x) {
        int x, y;
        if (!walk.at(t, h, &x, &y)) continue;
        const int p = y * w + x;
        const bool active = x < w && (img[p] != 0) == FG;
        const unsigned long long m = __ballot(active);
        if (x >= w) continue;
        const unsigned long long gaps = ~m & ((1ull << lane) - 1);         // inactive lanes below this one
        const int start = gaps ? 64 - __clzll(gaps) : 0;                    // first lane of this lane's run
        L[p] = active ? p - lane + start : -1;
        info[p] = 0;
    }
}

// The joins that init has not made: a run with the run left of it across a 64-pixel segment border, and a pixel with the row
// above.  A join implied by others is skipped: (p, up) when left and up-left are both set (p - left - up-left - up is a path whose
// middle link is left's own join, by induction along the run); the diagonals when up, or for up-left also left, is set.
template <bool FG, bool CONN8>
__global__ __launch_bounds__(256)
void cc_merge_kernel(const unsigned char* __restrict__ img, int h, int w, int* __restrict__ L, int* __restrict__ err) {
    const CcWalk walk(h, w);
    const int n = h * w;
    for (int64_t t = blockIdx.x; t < walk.ntiles; t += gridDim.x) {
        int x, y;
        if (!walk.at(t, h, &x, &y) || x >= w) continue;
        const int p = y * w + x;
        if ((img[p] != 0) != FG) continue;
        const bool lf = x > 0 && (img[p - 1] != 0) == FG;
        if (lf && (x & 63) == 0) cc_union(L, p, p - 1, n, err);
        if (y == 0) continue;
        const bool up = (img[p - w] != 0) == FG;
        const bool ul = x > 0 && (img[p - w - 1] != 0) == FG;
        if (up && !(lf && ul)) cc_union(L, p, p - w, n, err);
        if (CONN8) {
            const bool ur = x + 1 < w && (img[p - w + 1] != 0) == FG;
            if (ul && !up && !lf) cc_union(L, p, p - w - 1, n, err);
            if (ur && !up) cc_union(L, p, p - w + 1, n, err);
        }
    }
}

__global__ __launch_bounds__(256)
void cc_compress_kernel(int h, int w, int* __restrict__ L, int* __restrict__ err) {
    const int n = h * w;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (cc_load(L, (int)i) < 0) continue;
        const int r = cc_find(L, (int)i, n, err);
        if (r >= 0) L[i] = r;                         // a racing reader sees the old parent or the root: both are ancestors
    }
}

// info[root] += area, |= CC_BORDER.  Lanes of a wave that share a root add once (the usual case: one component per row segment).
__global__ __launch_bounds__(256)
void cc_count_kernel(int h, int w, const int* __restrict__ L, int* __restrict__ info) {
    const CcWalk walk(h, w);
    const int lane = threadIdx.x & 63;
    for (int64_t t = blockIdx.x; t < walk.ntiles; t += gridDim.x) {
        int x, y;
        if (!walk.at(t, h, &x, &y)) continue;
        const int root = x < w ? L[y * w + x] : -1;
        unsigned long long todo = __ballot(root >= 0);
        while (todo) {                                // at most 64 rounds: every round retires its leader
            const int leader = __ffsll((long long)todo) - 1;
            const int r = __shfl(root, leader);
            const unsigned long long same = __ballot(root == r);
            if (lane == leader) atomicAdd(info + r, __popcll(same));
            todo &= ~same;
        }
        if (root >= 0 && (x == 0 || y == 0 || x == w - 1 || y == h - 1)) atomicOr(info + root, CC_BORDER);
    }
}

// labels of the background: a hole (no border bit) of <= min_hole pixels becomes foreground
__global__ __launch_bounds__(256)
void cc_fill_holes_kernel(unsigned char* __restrict__ img, int h, int w, const int* __restrict__ L, const int* __restrict__ info, int min_hole) {
    const int n = h * w;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int r = L[i];
        if (r < 0) continue;
        const int v = info[r];                        // negative: touches the border
        if (v >= 0 && v <= min_hole) img[i] = 1;
    }
}

// labels of the foreground: a component of <= min_area pixels is cleared
__global__ __launch_bounds__(256)
void cc_drop_small_kernel(unsigned char* __restrict__ img, int h, int w, const int* __restrict__ L, const int* __restrict__ info, int min_area) {
    const int n = h * w;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int r = L[i];
        if (r < 0) continue;
        if ((info[r] & ~CC_BORDER) <= min_area) img[i] = 0;
    }
}

// ---- the grid on a mask ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool mask_point(const unsigned char* mask, int64_t mh, int64_t mw, int64_t ds, int64_t px, int64_t py) {
    if (px < 0 || py < 0) return false;
    const int64_t mx = px / ds, my = py / ds;
    return mx < mw && my < mh && mask[my * mw + mx] != 0;
}

__global__ __launch_bounds__(256)
void tissue_grid_cells_kernel(const unsigned char* __restrict__ mask, int64_t mh, int64_t mw, int64_t ds, int gx, int64_t ncells, int patch,
                              int step, int64_t ox, int64_t oy, int mode, unsigned char* __restrict__ keep) {
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < ncells; c += (int64_t)gridDim.x * 256) {
        const int64_t cx = ox + (c % gx) * step + patch / 2, cy = oy + (c / gx) * step + patch / 2, s = patch / 4;
        bool k;
        if (mode == KEEP_MASK_CENTER) {
            k = mask_point(mask, mh, mw, ds, cx, cy);
        } else {
            const bool a = mask_point(mask, mh, mw, ds, cx - s, cy - s), b = mask_point(mask, mh, mw, ds, cx + s, cy - s);
            const bool d = mask_point(mask, mh, mw, ds, cx - s, cy + s), e = mask_point(mask, mh, mw, ds, cx + s, cy + s);
            k = mode == KEEP_MASK_FOUR_PT_HARD ? (a && b && d && e) : (a || b || d || e);
        }
        keep[c] = k;
    }
}

}  // namespace keepk
using namespace keepk;

static unsigned tissue_grid_for(int64_t items, int per_block) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (unsigned)(b > 65536 ? 65536 : (b < 1 ? 1 : b));
}

int launch_tissue_median_hist(const unsigned char* thumb, int64_t row_stride, int ps, int h, int w, int ksize, unsigned char* med, int* hist,
                              hipStream_t s) {
    const int64_t tiles = (int64_t)((w + MED_TW - 1) / MED_TW) * ((h + MED_TH - 1) / MED_TH);
    const dim3 g(tissue_grid_for(tiles, 1)), b(256);
#define KEEP_MEDIAN_CASE(K) \
    case K: hipLaunchKernelGGL(tissue_median_hist_kernel<K>, g, b, 0, s, thumb, row_stride, ps, h, w, med, hist); return 0
    switch (ksize) {
        KEEP_MEDIAN_CASE(1); KEEP_MEDIAN_CASE(3); KEEP_MEDIAN_CASE(5); KEEP_MEDIAN_CASE(7);
        KEEP_MEDIAN_CASE(9); KEEP_MEDIAN_CASE(11); KEEP_MEDIAN_CASE(13); KEEP_MEDIAN_CASE(15);
    }
#undef KEEP_MEDIAN_CASE
    return -1;
}

template <bool FG, bool CONN8>
static void cc_label(const unsigned char* img, int h, int w, int* L, int* info, int* err, hipStream_t s) {
    const int64_t n = (int64_t)h * w, tiles = (int64_t)((w + 63) / 64) * ((h + 3) / 4);
    const dim3 gt(tissue_grid_for(tiles, 1)), gp(tissue_grid_for(n, 256)), b(256);
    hipLaunchKernelGGL((cc_init_kernel<FG>), gt, b, 0, s, img, h, w, L, info);
    hipLaunchKernelGGL((cc_merge_kernel<FG, CONN8>), gt, b, 0, s, img, h, w, L, err);
    hipLaunchKernelGGL(cc_compress_kernel, gp, b, 0, s, h, w, L, err);
    hipLaunchKernelGGL(cc_count_kernel, gt, b, 0, s, h, w, L, info);
}

void launch_cc_label(const unsigned char* img, int h, int w, int conn8, int* labels, int* info, int* err, hipStream_t s) {
    if (conn8) cc_label<true, true>(img, h, w, labels, info, err, s);
    else cc_label<true, false>(img, h, w, labels, info, err, s);
}

void launch_tissue_mask(const unsigned char* med, int h, int w, int thr, int close, int min_hole, int min_area, unsigned char* tmp, int* labels,
                        int* info, int* err, unsigned char* mask, hipStream_t s) {
    const int64_t n = (int64_t)h * w;
    const dim3 gp(tissue_grid_for(n, 256)), b(256);
    if (close > 0) {
        const int a = close / 2;
        hipLaunchKernelGGL(tissue_box_kernel, gp, b, 0, s, med, tmp, h, w, close, a, 1, 0, thr);
        hipLaunchKernelGGL(tissue_box_kernel, gp, b, 0, s, (const unsigned char*)tmp, mask, h, w, close, a, 0, 0, -1);
        hipLaunchKernelGGL(tissue_box_kernel, gp, b, 0, s, (const unsigned char*)mask, tmp, h, w, close, a, 1, 1, -1);
        hipLaunchKernelGGL(tissue_box_kernel, gp, b, 0, s, (const unsigned char*)tmp, mask, h, w, close, a, 0, 1, -1);
    } else {
        hipLaunchKernelGGL(tissue_box_kernel, gp, b, 0, s, med, mask, h, w, 1, 0, 1, 0, thr);           // a 1 x 1 window: the threshold alone
    }
    if (min_hole > 0) {                               // a hole holds >= 1 pixel: min_hole = 0 fills none
        cc_label<false, false>(mask, h, w, labels, info, err, s);
        hipLaunchKernelGGL(cc_fill_holes_kernel, gp, b, 0, s, mask, h, w, (const int*)labels, (const int*)info, min_hole);
    }
    if (min_area > 0) {                               // likewise min_area = 0 drops none
        cc_label<true, true>(mask, h, w, labels, info, err, s);
        hipLaunchKernelGGL(cc_drop_small_kernel, gp, b, 0, s, mask, h, w, (const int*)labels, (const int*)info, min_area);
    }
}

void launch_tissue_grid_cells(const unsigned char* mask, int64_t mh, int64_t mw, int64_t ds, int gx, int64_t ncells, int patch, int step,
                              int64_t ox, int64_t oy, int mode, unsigned char* keep, hipStream_t s) {
    hipLaunchKernelGGL(tissue_grid_cells_kernel, dim3(tissue_grid_for(ncells, 256)), dim3(256), 0, s, mask, mh, mw, ds, gx, ncells, patch, step,
                       ox, oy, mode, keep);
}
