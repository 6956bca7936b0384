// Region table: the connected regions of a mask, numbered in a stable order, with their geometry and their scores from a tile
// raster.  Integer arithmetic throughout: every result is held exactly to keep_amd.components.regions_numpy.
//
//   (tissue.hip)            cc_init / cc_merge / cc_compress / cc_count label the foreground: roots[p] = the smallest pixel index of
//                           p's component (-1 on the background), info[root] = area | border bit
//   regions_root_count /    dense ids without atomics: a root is kept iff its area >= min_area; per-block counts of the kept roots,
//   regions_scan /          a one-block exclusive scan of those (which also writes n), then a per-block scan that overwrites
//   regions_root_rank       info[root] with the root's 1-based rank (0: dropped).  A root is its component's first pixel in row-major
//                           order, so the ranks number the components in that order (scipy.ndimage.label's order)
//   regions_relabel         labels[p] = info[roots[p]], 0 on the background
//   regions_table_init      the identities of the table's minima
//   regions_table           one pass over labels (+ accumulator) on the 64 x 4 wave walk.  A workgroup owns a contiguous run of
//                           tiles and every lane carries ONE running region in registers across them; it gives that region up only
//                           when it meets a different non-zero label (background in between does not count).  Lanes that give up
//                           in the same step and share a label are combined by shuffles first (ballot-leader rounds as in
//                           cc_count), so a wave issues one set of atomics per distinct label.  At the end of the run each wave
//                           combines what its lanes still hold, the four waves meet in LDS, and waves that hold the same label
//                           leave as one.  A mask that is one region therefore costs one set of atomics per workgroup.
//                           64-bit integer add / min / max at agent scope, no return value: sums, minima and maxima of integers
//                           do not depend on the order, so the table is the same from run to run and for every launch grid
//   regions_table_first     column 0 held the smallest linear pixel index: -> (first_x, first_y)
//
// Pixel indices are int32 (h w <= 2^30, checked by the caller); offsets into the accumulator and the table are int64.
#include "common.h"
#include "labelling.h"
#include "../../include/keep_hip.h"

namespace keepk {

constexpr int REGIONS_PX_PER_BLOCK = REGIONS_SCAN_CHUNK;   // 8 consecutive pixels per thread
constexpr int REGIONS_PX_PER_THREAD = REGIONS_PX_PER_BLOCK / 256;
constexpr int REGIONS_TABLE_BLOCKS = 2048;            // workgroups of the table pass (8 per CU): each flushes at least once
constexpr long long REGIONS_NONE = 0x7fffffffffffffffll;
constexpr int REGIONS_COUNT_SHIFT = 40;               // the accumulator of heatmap.hip: bits 0..39 the sum, bits 40..63 the count

enum { RC_FIRST = 0, RC_FIRST_Y = 1, RC_AREA = 2, RC_X0 = 3, RC_Y0 = 4, RC_X1 = 5, RC_Y1 = 6, RC_SUM_X = 7, RC_SUM_Y = 8, RC_BORDER = 9,
       RC_COVERED = 10, RC_SUM_C = 11, RC_SUM_S = 12, RC_PEAK = 13 };

// ---- dense ids -------------------------------------------------------------------------------------------------------------
// bit j: pixel p0 + j is a root whose component is kept; *roots_mask: bit j: it is a root at all
__device__ __forceinline__ unsigned regions_thread_kept(const int* __restrict__ roots, const int* __restrict__ info, int n, int min_area,
                                                        int64_t p0, unsigned* roots_mask) {
    unsigned kept = 0, isroot = 0;
    int r[REGIONS_PX_PER_THREAD];
    if (p0 + REGIONS_PX_PER_THREAD <= n) {            // p0 is a multiple of 8 and roots 16-byte aligned (the caller's workspace)
        const int4 a = *reinterpret_cast<const int4*>(roots + p0), b = *reinterpret_cast<const int4*>(roots + p0 + 4);
        r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w; r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
    } else {
#pragma unroll
        for (int j = 0; j < REGIONS_PX_PER_THREAD; ++j) r[j] = p0 + j < n ? roots[p0 + j] : -1;
    }
#pragma unroll
    for (int j = 0; j < REGIONS_PX_PER_THREAD; ++j) {
        if (r[j] >= 0 && r[j] == (int)(p0 + j)) {
            isroot |= 1u << j;
            if ((info[p0 + j] & ~CC_BORDER) >= min_area) kept |= 1u << j;
        }
    }
    *roots_mask = isroot;
    return kept;
}

__global__ __launch_bounds__(256)
void regions_root_count_kernel(const int* __restrict__ roots, const int* __restrict__ info, int n, int min_area, int* __restrict__ counts) {
    __shared__ int s[256];
    const int64_t p0 = (int64_t)blockIdx.x * REGIONS_PX_PER_BLOCK + (int64_t)threadIdx.x * REGIONS_PX_PER_THREAD;
    unsigned isroot;
    int total;
    block_exclusive_scan256(__popc(regions_thread_kept(roots, info, n, min_area, p0, &isroot)), s, &total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// one block: offsets[b] = sum of counts[0, b); *n_out = sum of all counts
__global__ __launch_bounds__(256)
void regions_scan_kernel(const int* __restrict__ counts, int nb, int* __restrict__ offsets, int64_t* __restrict__ n_out) {
    __shared__ int s[256];
    int carry = 0;
    for (int b0 = 0; b0 < nb; b0 += 256) {
        const int b = b0 + threadIdx.x;
        int total;
        const int ex = block_exclusive_scan256(b < nb ? counts[b] : 0, s, &total);
        if (b < nb) offsets[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *n_out = carry;
}

// info[root] = the root's 1-based rank among the kept roots, 0 if its component is dropped.  A thread reads and writes its own
// eight pixels only.
__global__ __launch_bounds__(256)
void regions_root_rank_kernel(const int* __restrict__ roots, int* __restrict__ info, int n, int min_area, const int* __restrict__ offsets) {
    __shared__ int s[256];
    const int64_t p0 = (int64_t)blockIdx.x * REGIONS_PX_PER_BLOCK + (int64_t)threadIdx.x * REGIONS_PX_PER_THREAD;
    unsigned isroot;
    const unsigned kept = regions_thread_kept(roots, info, n, min_area, p0, &isroot);
    int total;
    int rank = offsets[blockIdx.x] + block_exclusive_scan256(__popc(kept), s, &total);
#pragma unroll
    for (int j = 0; j < REGIONS_PX_PER_THREAD; ++j) {
        if (isroot >> j & 1u) info[p0 + j] = (kept >> j & 1u) ? ++rank : 0;
    }
}

__global__ __launch_bounds__(256)
void regions_relabel_kernel(const int* __restrict__ roots, const int* __restrict__ info, int n, int* __restrict__ labels) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int r = roots[i];
        labels[i] = r >= 0 ? info[r] : 0;             // r < 0 also where a labelling loop ran out (the error bit is set)
    }
}

// ---- the table -------------------------------------------------------------------------------------------------------------
// what a lane, a wave or a workgroup holds of ONE region
struct RegionPart {
    int label;                                        // 0: nothing held
    int area, x0, y0, x1, y1, first, border, covered, peak;
    long long sum_x, sum_y, sum_c, sum_s;
};

__device__ __forceinline__ void region_part_start(RegionPart& a, int label) {
    a.label = label;
    a.area = a.x1 = a.y1 = a.border = a.covered = a.peak = 0;
    a.x0 = a.y0 = a.first = 0x7fffffff;
    a.sum_x = a.sum_y = a.sum_c = a.sum_s = 0;
}

__device__ __forceinline__ void region_part_merge(RegionPart& a, const RegionPart& b) {
    a.area += b.area; a.covered += b.covered;
    a.x0 = min(a.x0, b.x0); a.y0 = min(a.y0, b.y0); a.first = min(a.first, b.first);
    a.x1 = max(a.x1, b.x1); a.y1 = max(a.y1, b.y1); a.peak = max(a.peak, b.peak); a.border |= b.border;
    a.sum_x += b.sum_x; a.sum_y += b.sum_y; a.sum_c += b.sum_c; a.sum_s += b.sum_s;
}

// the pixel's mean on 0..65535, rounded half up: (2 S + c) / (2 c) for c > 0.  2 S + c < 2^42 and 2 c < 2^25 are exact doubles, so
// the rounded double quotient is off by at most one: corrected by the remainder
__device__ __forceinline__ int region_peak16(long long S, long long c) {
    const long long num = 2 * S + c, den = 2 * c;
    long long q = (long long)((double)num / (double)den);
    const long long r = num - q * den;
    if (r < 0) --q;
    else if (r >= den) ++q;
    return (int)q;
}

// the members' parts combined in every lane (a butterfly over the whole wave; the other lanes put in the identities)
__device__ __forceinline__ RegionPart region_wave_combine(const RegionPart& a, bool member) {
    RegionPart g;
    region_part_start(g, a.label);
    if (member) g = a;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        RegionPart b;
        b.area = __shfl_xor(g.area, o); b.covered = __shfl_xor(g.covered, o);
        b.x0 = __shfl_xor(g.x0, o); b.y0 = __shfl_xor(g.y0, o); b.first = __shfl_xor(g.first, o);
        b.x1 = __shfl_xor(g.x1, o); b.y1 = __shfl_xor(g.y1, o); b.peak = __shfl_xor(g.peak, o); b.border = __shfl_xor(g.border, o);
        b.sum_x = __shfl_xor(g.sum_x, o); b.sum_y = __shfl_xor(g.sum_y, o); b.sum_c = __shfl_xor(g.sum_c, o); b.sum_s = __shfl_xor(g.sum_s, o);
        region_part_merge(g, b);
    }
    return g;
}

__device__ __forceinline__ void region_add(long long* p, long long v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void region_min(long long* p, long long v) {
    (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void region_max(long long* p, long long v) {
    (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one part into its table row (the caller has checked 1 <= label <= n)
__device__ __forceinline__ void region_emit(long long* __restrict__ table, const RegionPart& g) {
    long long* row = table + (int64_t)(g.label - 1) * REGIONS_COLS;
    region_min(row + RC_FIRST, g.first);
    region_add(row + RC_AREA, g.area);
    region_min(row + RC_X0, g.x0);
    region_min(row + RC_Y0, g.y0);
    region_max(row + RC_X1, g.x1);
    region_max(row + RC_Y1, g.y1);
    region_add(row + RC_SUM_X, g.sum_x);
    region_add(row + RC_SUM_Y, g.sum_y);
    if (g.border) region_max(row + RC_BORDER, 1);
    if (g.covered) {
        region_add(row + RC_COVERED, g.covered);
        region_add(row + RC_SUM_C, g.sum_c);
        region_add(row + RC_SUM_S, g.sum_s);
        region_max(row + RC_PEAK, g.peak);
    }
}

// The lanes with `out` set give up their parts: one set of atomics per distinct label among them.  Called by the whole wave.
__device__ __forceinline__ void region_wave_flush(const RegionPart& a, bool out, long long* __restrict__ table) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(out);
    while (todo) {                                    // at most 64 rounds: every round retires its leader
        const int leader = __ffsll((long long)todo) - 1;
        const int r = __shfl(a.label, leader);
        const bool member = out && a.label == r;
        const unsigned long long same = __ballot(member);
        if (same & (same - 1)) {                      // more than one lane (wave-uniform)
            const RegionPart g = region_wave_combine(a, member);
            if (lane == leader) region_emit(table, g);
        } else if (lane == leader) {
            region_emit(table, a);
        }
        todo &= ~same;
    }
}

__global__ __launch_bounds__(256)
void regions_table_init_kernel(long long* __restrict__ table, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n * REGIONS_COLS; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % REGIONS_COLS);
        table[i] = (c == RC_FIRST || c == RC_X0 || c == RC_Y0) ? REGIONS_NONE : 0;
    }
}

template <bool ACC>
__global__ __launch_bounds__(256)
void regions_table_kernel(const int* __restrict__ labels, int h, int w, int64_t n, const unsigned long long* __restrict__ acc,
                          long long* __restrict__ table) {
    __shared__ RegionPart part[4];
    const CcWalk walk(h, w);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t per = (walk.ntiles + gridDim.x - 1) / gridDim.x;
    const int64_t t0 = blockIdx.x * per, t1 = min(t0 + per, walk.ntiles);
    RegionPart a;
    region_part_start(a, 0);
    for (int64_t t = t0; t < t1; ++t) {               // the same trip count for the whole workgroup
        int x, y, lab = 0;
        const bool in = walk.at(t, h, &x, &y) && x < w;
        const int p = in ? y * w + x : 0;
        if (in) lab = labels[p];
        if (lab < 1 || lab > n) lab = 0;              // a caller's label outside 1..n is background: no row of the table to write
        const bool out = lab != 0 && a.label != 0 && lab != a.label;
        if (__ballot(out)) region_wave_flush(a, out, table);
        if (lab == 0) continue;
        if (lab != a.label) region_part_start(a, lab);
        ++a.area;
        a.x0 = min(a.x0, x); a.y0 = min(a.y0, y); a.x1 = max(a.x1, x + 1); a.y1 = max(a.y1, y + 1); a.first = min(a.first, p);
        a.sum_x += x; a.sum_y += y;
        a.border |= x == 0 || y == 0 || x == w - 1 || y == h - 1;
        if (ACC) {
            const unsigned long long v = acc[p];
            const long long c = (long long)(v >> REGIONS_COUNT_SHIFT), S = (long long)(v & ((1ull << REGIONS_COUNT_SHIFT) - 1));
            if (c > 0) {
                ++a.covered;
                a.sum_c += c; a.sum_s += S;
                a.peak = max(a.peak, c == 1 ? (int)S : region_peak16(S, c));        // S <= 65535 c (keep_hip.h): fits an int
            }
        }
    }
    // what the lanes still hold: a wave of one label goes to LDS, where the waves that agree are combined; any other wave flushes
    const unsigned long long held = __ballot(a.label != 0);
    int mine = 0;                                     // the label this wave brings to LDS (wave-uniform), 0: none
    if (held) {
        const int r = __shfl(a.label, __ffsll((long long)held) - 1);
        if (__ballot(a.label != 0 && a.label != r) == 0) mine = r;
    }
    if (mine) {
        const RegionPart g = region_wave_combine(a, a.label != 0);
        if (lane == 0) { part[wave] = g; part[wave].label = mine; }
    } else {
        if (lane == 0) part[wave].label = 0;
        region_wave_flush(a, a.label != 0, table);
    }
    __syncthreads();
    if (lane == 0 && mine) {
        bool head = true;                             // the first wave of a label takes the later ones along
        for (int k = 0; k < wave; ++k) head = head && part[k].label != mine;
        if (head) {
            RegionPart g = part[wave];
            for (int k = wave + 1; k < 4; ++k)
                if (part[k].label == mine) region_part_merge(g, part[k]);
            region_emit(table, g);
        }
    }
}

__global__ __launch_bounds__(256)
void regions_table_first_kernel(long long* __restrict__ table, int64_t n, int w) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        long long* row = table + i * REGIONS_COLS;
        const long long p = row[RC_FIRST];
        if (p == REGIONS_NONE) {                      // a label no pixel carries (a caller's own labels): an all-zero row
            row[RC_FIRST] = row[RC_X0] = row[RC_Y0] = 0;
        } else {
            row[RC_FIRST] = p % w;
            row[RC_FIRST_Y] = p / w;
        }
    }
}

}  // namespace keepk
using namespace keepk;

static unsigned regions_grid_for(int64_t items, int per_block) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (unsigned)(b > 65536 ? 65536 : (b < 1 ? 1 : b));
}

void launch_regions_label(const unsigned char* mask, int h, int w, int conn8, int min_area, int* roots, int* info, int* counts, int* offsets,
                          int* err, int* labels_out, int64_t* n_out, hipStream_t s) {
    const int n = h * w, nb = (n + REGIONS_PX_PER_BLOCK - 1) / REGIONS_PX_PER_BLOCK;
    launch_cc_label(mask, h, w, conn8, roots, info, err, s);
    hipLaunchKernelGGL(regions_root_count_kernel, dim3(nb), dim3(256), 0, s, (const int*)roots, (const int*)info, n, min_area, counts);
    hipLaunchKernelGGL(regions_scan_kernel, dim3(1), dim3(256), 0, s, (const int*)counts, nb, offsets, n_out);
    hipLaunchKernelGGL(regions_root_rank_kernel, dim3(nb), dim3(256), 0, s, (const int*)roots, info, n, min_area, (const int*)offsets);
    hipLaunchKernelGGL(regions_relabel_kernel, dim3(regions_grid_for(n, 256)), dim3(256), 0, s, (const int*)roots, (const int*)info, n, labels_out);
}

void launch_regions_table(const int* labels, int h, int w, int64_t n, const int64_t* acc, int64_t* table, hipStream_t s) {
    if (n < 1) return;
    const int64_t tiles = (int64_t)((w + 63) / 64) * ((h + 3) / 4);
    const dim3 g((unsigned)(tiles < REGIONS_TABLE_BLOCKS ? tiles : REGIONS_TABLE_BLOCKS)), b(256);
    long long* t = reinterpret_cast<long long*>(table);
    hipLaunchKernelGGL(regions_table_init_kernel, dim3(regions_grid_for(n * REGIONS_COLS, 256)), b, 0, s, t, n);
    if (acc)
        hipLaunchKernelGGL(regions_table_kernel<true>, g, b, 0, s, labels, h, w, n, reinterpret_cast<const unsigned long long*>(acc), t);
    else
        hipLaunchKernelGGL(regions_table_kernel<false>, g, b, 0, s, labels, h, w, n, (const unsigned long long*)nullptr, t);
    hipLaunchKernelGGL(regions_table_first_kernel, dim3(regions_grid_for(n, 256)), b, 0, s, t, n, w);
}
