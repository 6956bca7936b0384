// Region shape: second moments and the exact largest diameter of every region of a label image.  Integer
// arithmetic throughout: every result is held exactly to keep_amd.morphometry.shape_numpy.
//
//   shape_moments           one pass over the labels on the 64 x 4 wave walk, in the shape of components.hip's table pass: a
//                           workgroup owns a contiguous run of tiles, every lane carries ONE running region in int64 registers and
//                           gives it up only when it meets another non-zero label; lanes that give up the same label are summed by
//                           shuffles first, the four waves meet in LDS at the end of the run, and what leaves is a 64-bit integer
//                           atomic add at agent scope.  u = x - x0 and v = y - y0 are taken from the region's box origin (read from
//                           the table when a lane takes the label up), so the sums stay small; no float and no 32-bit partial sum
//   feret_plan              one block: L_i = min(bw, bh) lines per region (rows iff bh <= bw), the exclusive scans of L_i and of the
//                           region's workgroups nb_i (nb_i + 1) / 2 (nb_i = ceil(4 L_i / 256)), and the totals the host reads back
//   feret_lines             the first and last pixel of every line of every region: integer atomic min / max by the pixels that end
//                           a run along their region's lines (interior pixels do not touch the table)
//   feret_pairs<false>      candidates = the four corners of every line's first and last pixel.  One workgroup per (region, block p,
//                           block q) of 256 candidates, p <= q: a thread holds one candidate of p and walks the 256 of q in LDS;
//                           the wave's largest squared distance leaves as one 64-bit atomic max
//   feret_pairs<true>       the same walk again: the pairs that reach d2 give (a << 32) | b with a < b their lattice indices
//                           y (W + 1) + x, and the smallest leaves as one 64-bit atomic min
//   feret_finish            (d2, packed pair) -> (d2, ax, ay, bx, by); a label no pixel carries gives a zero row
//
// Every hull vertex of a region is a corner of a pixel that is extreme in its row and of one that is extreme in its column, so the
// candidates of either choice hold every hull vertex and the largest distance over them is the largest over the region.
#include "common.h"
#include "labelling.h"
#include "../../include/keep_hip.h"

#include <algorithm>

namespace keepk {

constexpr int SHAPE_MOMENT_BLOCKS = 2048;             // workgroups of the moments pass (8 per CU), as the table pass
constexpr int SHAPE_COLS_X0 = 3, SHAPE_COLS_Y0 = 4, SHAPE_COLS_X1 = 5, SHAPE_COLS_Y1 = 6;   // columns of the region table
constexpr int FERET_BLOCK = 256;                      // candidates per block of the pair walk
constexpr long long FERET_NONE = 0x7fffffffffffffffll;
constexpr long long FERET_PAIR_CAP = 1ll << 54;       // a thread's share of the pair total saturates here: 256 of them stay in int64

__device__ __forceinline__ void shape_add(long long* p, long long v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- second moments --------------------------------------------------------------------------------------------------------
// what a lane holds of ONE region
struct MomentPart {
    int label;                                        // 0: nothing held
    int ox, oy;                                       // the region's box origin, clamped into the image
    long long uu, vv, uv;
};

__device__ __forceinline__ void moment_emit(long long* __restrict__ mom, int label, long long uu, long long vv, long long uv) {
    long long* row = mom + (int64_t)(label - 1) * 3;  // the caller has checked 1 <= label <= n
    shape_add(row, uu);
    shape_add(row + 1, vv);
    shape_add(row + 2, uv);
}

// the members' sums in every lane (a butterfly over the whole wave; the other lanes put in zeros)
__device__ __forceinline__ void moment_wave_sum(long long& uu, long long& vv, long long& uv) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        uu += __shfl_xor(uu, o); vv += __shfl_xor(vv, o); uv += __shfl_xor(uv, o);
    }
}

// The lanes with `out` set give up their parts: one set of atomics per distinct label among them.  Called by the whole wave.
__device__ __forceinline__ void moment_wave_flush(const MomentPart& a, bool out, long long* __restrict__ mom) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(out);
    while (todo) {                                    // at most 64 rounds: every round retires its leader
        const int leader = __ffsll((long long)todo) - 1;
        const int r = __shfl(a.label, leader);
        const bool member = out && a.label == r;
        const unsigned long long same = __ballot(member);
        long long uu = member ? a.uu : 0, vv = member ? a.vv : 0, uv = member ? a.uv : 0;
        if (same & (same - 1)) moment_wave_sum(uu, vv, uv);   // more than one lane (wave-uniform)
        if (lane == leader) moment_emit(mom, r, uu, vv, uv);
        todo &= ~same;
    }
}

__global__ __launch_bounds__(256)
void shape_moments_kernel(const int* __restrict__ labels, int h, int w, int64_t n, const long long* __restrict__ table,
                          long long* __restrict__ mom) {
    __shared__ long long part[4][3];
    __shared__ int part_label[4];
    const CcWalk walk(h, w);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t per = (walk.ntiles + gridDim.x - 1) / gridDim.x;
    const int64_t t0 = blockIdx.x * per, t1 = min(t0 + per, walk.ntiles);
    MomentPart a;
    a.label = a.ox = a.oy = 0;
    a.uu = a.vv = a.uv = 0;
    for (int64_t t = t0; t < t1; ++t) {               // the same trip count for the whole workgroup
        int x, y, lab = 0;
        const bool in = walk.at(t, h, &x, &y) && x < w;
        if (in) lab = labels[(int64_t)y * w + x];
        if (lab < 1 || lab > n) lab = 0;              // a caller's label outside 1..n is background: no row to write
        const bool out = lab != 0 && a.label != 0 && lab != a.label;
        if (__ballot(out)) moment_wave_flush(a, out, mom);
        if (lab == 0) continue;
        if (lab != a.label) {
            const long long* row = table + (int64_t)(lab - 1) * REGIONS_COLS;
            a.label = lab;
            a.ox = (int)min(max(row[SHAPE_COLS_X0], 0ll), (long long)w - 1); a.oy = (int)min(max(row[SHAPE_COLS_Y0], 0ll), (long long)h - 1);
            a.uu = a.vv = a.uv = 0;
        }
        const long long u = x - a.ox, v = y - a.oy;
        a.uu += u * u; a.vv += v * v; a.uv += u * v;
    }
    // what the lanes still hold: a wave of one label goes to LDS, where the waves that agree are combined; any other wave flushes
    const unsigned long long held = __ballot(a.label != 0);
    int mine = 0;                                     // the label this wave brings to LDS (wave-uniform), 0: none
    if (held) {
        const int r = __shfl(a.label, __ffsll((long long)held) - 1);
        if (__ballot(a.label != 0 && a.label != r) == 0) mine = r;
    }
    if (mine) {
        long long uu = a.label ? a.uu : 0, vv = a.label ? a.vv : 0, uv = a.label ? a.uv : 0;
        moment_wave_sum(uu, vv, uv);
        if (lane == 0) { part[wave][0] = uu; part[wave][1] = vv; part[wave][2] = uv; part_label[wave] = mine; }
    } else {
        if (lane == 0) part_label[wave] = 0;
        moment_wave_flush(a, a.label != 0, mom);
    }
    __syncthreads();
    if (lane == 0 && mine) {
        bool head = true;                             // the first wave of a label takes the later ones along
        for (int k = 0; k < wave; ++k) head = head && part_label[k] != mine;
        if (head) {
            long long uu = part[wave][0], vv = part[wave][1], uv = part[wave][2];
            for (int k = wave + 1; k < 4; ++k)
                if (part_label[k] == mine) { uu += part[k][0]; vv += part[k][1]; uv += part[k][2]; }
            moment_emit(mom, mine, uu, vv, uv);
        }
    }
}

// ---- the largest diameter --------------------------------------------------------------------------------------------------
// a region's lines: L = min(bw, bh) of them, rows iff bh <= bw.  A box that does not lie inside the image (a caller's table) has
// none, so never more than min(h, w): L <= 2^15 and 8 L^2 <= 2^33
struct FeretLines { int x0, y0, L; bool rows; };

__device__ __forceinline__ FeretLines feret_lines_of(const long long* __restrict__ table, int64_t i, int h, int w) {
    const long long* row = table + i * REGIONS_COLS;
    const long long x0 = row[SHAPE_COLS_X0], y0 = row[SHAPE_COLS_Y0], x1 = row[SHAPE_COLS_X1], y1 = row[SHAPE_COLS_Y1];
    const bool box = x0 >= 0 && y0 >= 0 && x1 > x0 && y1 > y0 && x1 <= w && y1 <= h;    // every coordinate then fits an int
    FeretLines g;
    g.x0 = box ? (int)x0 : 0; g.y0 = box ? (int)y0 : 0;
    g.rows = y1 - y0 <= x1 - x0;
    g.L = box ? (int)min(x1 - x0, y1 - y0) : 0;
    return g;
}

// one block.  line_off[i], wg_off[i]: exclusive scans over the regions ([n] holds the totals); totals: candidates, pairs, workgroups
__global__ __launch_bounds__(256)
void feret_plan_kernel(const long long* __restrict__ table, int64_t n, int h, int w, long long* __restrict__ line_off,
                       long long* __restrict__ wg_off, long long* __restrict__ totals) {
    __shared__ long long s[2][256];
    const int t = threadIdx.x;
    long long carry_l = 0, carry_g = 0, pairs = 0;
    for (int64_t b0 = 0; b0 < n; b0 += 256) {
        const int64_t i = b0 + t;
        long long L = 0, G = 0;
        if (i < n) {
            L = feret_lines_of(table, i, h, w).L;
            const long long nb = (4 * L + FERET_BLOCK - 1) / FERET_BLOCK;
            G = nb * (nb + 1) / 2;
            pairs = min(pairs + 8 * L * L, FERET_PAIR_CAP);
        }
        s[0][t] = L; s[1][t] = G;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {           // inclusive scans of both
            const long long al = t >= o ? s[0][t - o] : 0, ag = t >= o ? s[1][t - o] : 0;
            __syncthreads();
            s[0][t] += al; s[1][t] += ag;
            __syncthreads();
        }
        if (i < n) { line_off[i] = carry_l + s[0][t] - L; wg_off[i] = carry_g + s[1][t] - G; }
        carry_l += s[0][255]; carry_g += s[1][255];
        __syncthreads();
    }
    s[0][t] = pairs;
    __syncthreads();
    if (t == 0) {
        long long p = 0;
        for (int k = 0; k < 256; ++k) p += s[0][k];
        line_off[n] = carry_l; wg_off[n] = carry_g;
        totals[0] = 4 * carry_l; totals[1] = p; totals[2] = carry_g;
    }
}

// lines: (first, last) per line; feret: (d2, packed pair, 0, 0, 0) per region
__global__ __launch_bounds__(256)
void feret_init_kernel(int* __restrict__ lines, int64_t total_lines, long long* __restrict__ feret, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < 2 * total_lines; i += stride) lines[i] = (i & 1) ? -1 : 0x7fffffff;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < 5 * n; i += stride) feret[i] = (i % 5 == 1) ? FERET_NONE : 0;
}

__global__ __launch_bounds__(256)
void feret_lines_kernel(const int* __restrict__ labels, int h, int w, int64_t n, const long long* __restrict__ table,
                        const long long* __restrict__ line_off, int* __restrict__ lines) {
    const int64_t npix = (int64_t)h * w;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += (int64_t)gridDim.x * 256) {
        const int lab = labels[p];
        if (lab < 1 || lab > n) continue;
        const int x = (int)(p % w), y = (int)(p / w);
        const bool l = x == 0 || labels[p - 1] != lab, r = x == w - 1 || labels[p + 1] != lab;
        const bool u = y == 0 || labels[p - w] != lab, d = y == h - 1 || labels[p + w] != lab;
        if (!(l || r || u || d)) continue;            // inside its region along both axes: neither first nor last of any line
        const FeretLines g = feret_lines_of(table, lab - 1, h, w);
        const int line = g.rows ? y - g.y0 : x - g.x0, pos = g.rows ? x : y;
        if (line < 0 || line >= g.L) continue;        // a table that is not this label image's: nothing is written out of bounds
        int* e = lines + 2 * (line_off[lab - 1] + line);
        if (g.rows ? l : u) atomicMin(e, pos);
        if (g.rows ? r : d) atomicMax(e + 1, pos);
    }
}

// candidate c of a region: corner c & 3 of line c >> 2; x < 0: none (past the last line, or a line without pixels)
__device__ __forceinline__ int2 feret_candidate(const int* __restrict__ lines, long long off, const FeretLines& g, int c) {
    int2 none; none.x = -1; none.y = -1;
    if (c >= 4 * g.L) return none;
    const int line = c >> 2, lo = lines[2 * (off + line)], hi = lines[2 * (off + line) + 1];
    if (hi < lo) return none;
    const int along = (c & 1) ? hi + 1 : lo, across = (g.rows ? g.y0 : g.x0) + line + ((c >> 1) & 1);
    int2 v;
    v.x = g.rows ? along : across; v.y = g.rows ? across : along;
    return v;
}

template <bool PICK>
__global__ __launch_bounds__(256)
void feret_pairs_kernel(const long long* __restrict__ table, int64_t n, int h, int w, const long long* __restrict__ line_off,
                        const long long* __restrict__ wg_off, const int* __restrict__ lines, long long* __restrict__ feret) {
    __shared__ int2 other[FERET_BLOCK];
    const long long total = wg_off[n], w1 = (long long)w + 1;
    for (long long item = blockIdx.x; item < total; item += gridDim.x) {      // the same trip count for the whole workgroup
        int64_t lo = 0, hi = n - 1;                   // the first region whose workgroups end past item
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (wg_off[mid + 1] > item) hi = mid; else lo = mid + 1;
        }
        const int64_t i = lo;
        const FeretLines g = feret_lines_of(table, i, h, w);
        const int nb = (4 * g.L + FERET_BLOCK - 1) / FERET_BLOCK;
        const long long k = item - wg_off[i];
        if (nb < 1 || k < 0 || k >= (long long)nb * (nb + 1) / 2) continue;   // cannot happen with the plan of this table
        int q = (int)((sqrt(8.0 * (double)k + 1.0) - 1.0) * 0.5);             // k = q (q + 1) / 2 + p, p <= q: every block pair once
        while ((long long)q * (q + 1) / 2 > k) --q;
        while ((long long)(q + 1) * (q + 2) / 2 <= k) ++q;
        const int p = (int)(k - (long long)q * (q + 1) / 2);
        const long long off = line_off[i];
        const int2 a = feret_candidate(lines, off, g, p * FERET_BLOCK + (int)threadIdx.x);
        __syncthreads();                              // the readers of the item before are done
        other[threadIdx.x] = feret_candidate(lines, off, g, q * FERET_BLOCK + (int)threadIdx.x);
        __syncthreads();
        const long long best = PICK ? feret[i * 5] : 0, ia = a.y * w1 + a.x;
        long long m = PICK ? FERET_NONE : 0;
        if (a.x >= 0) {
            for (int j = 0; j < FERET_BLOCK; ++j) {
                const int2 b = other[j];
                if (b.x < 0) continue;
                const long long dx = a.x - b.x, dy = a.y - b.y, d2 = dx * dx + dy * dy;
                if (!PICK) {
                    m = max(m, d2);
                } else if (d2 == best) {
                    const long long ib = b.y * w1 + b.x;
                    m = min(m, ia < ib ? (ia << 32 | ib) : (ib << 32 | ia));
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const long long v = __shfl_xor(m, o);
            m = PICK ? min(m, v) : max(m, v);
        }
        if ((threadIdx.x & 63) == 0) {
            if (!PICK) { if (m > 0) (void)__hip_atomic_fetch_max(feret + i * 5, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
            else if (m != FERET_NONE) (void)__hip_atomic_fetch_min(feret + i * 5 + 1, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

__global__ __launch_bounds__(256)
void feret_finish_kernel(long long* __restrict__ feret, int64_t n, int w) {
    const long long w1 = (long long)w + 1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        long long* row = feret + i * 5;
        const long long key = row[1];
        if (row[0] == 0 || key == FERET_NONE) {       // a label no pixel carries: an all-zero row
            row[0] = row[1] = row[2] = row[3] = row[4] = 0;
        } else {
            const long long a = key >> 32, b = key & 0xffffffffll;
            row[1] = a % w1; row[2] = a / w1; row[3] = b % w1; row[4] = b / w1;
        }
    }
}

}  // namespace keepk
using namespace keepk;

static unsigned shape_grid_for(int64_t items, int per_block, int64_t cap) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (unsigned)(b > cap ? cap : (b < 1 ? 1 : b));
}

// moments: [n][3], zeroed here
void launch_regions_moments(const int* labels, int h, int w, int64_t n, const int64_t* table, int64_t* moments, hipStream_t s) {
    if (n < 1) return;
    (void)hipMemsetAsync(moments, 0, (size_t)n * 3 * sizeof(int64_t), s);
    const int64_t tiles = (int64_t)((w + 63) / 64) * ((h + 3) / 4);
    hipLaunchKernelGGL(shape_moments_kernel, dim3((unsigned)(tiles < SHAPE_MOMENT_BLOCKS ? tiles : SHAPE_MOMENT_BLOCKS)), dim3(256), 0, s, labels, h,
                       w, n, reinterpret_cast<const long long*>(table), reinterpret_cast<long long*>(moments));
}

// plan: [line_off n + 1][wg_off n + 1][totals 3] int64
size_t feret_plan_bytes(int64_t n) { return (size_t)(2 * (n + 1) + 3) * sizeof(int64_t); }
const int64_t* launch_feret_plan(const int64_t* table, int h, int w, int64_t n, unsigned char* plan, hipStream_t s) {
    long long* p = reinterpret_cast<long long*>(plan);
    hipLaunchKernelGGL(feret_plan_kernel, dim3(1), dim3(256), 0, s, reinterpret_cast<const long long*>(table), n, h, w, p, p + (n + 1), p + 2 * (n + 1));
    return reinterpret_cast<const int64_t*>(p + 2 * (n + 1));
}

// lines: 2 total_lines ints; total_lines and total_wg as the plan's totals say
void launch_regions_feret(const int* labels, int h, int w, int64_t n, const int64_t* table, const unsigned char* plan, int* lines,
                          int64_t total_lines, int64_t total_wg, int64_t* feret, hipStream_t s) {
    const long long* p = reinterpret_cast<const long long*>(plan);
    const long long *line_off = p, *wg_off = p + (n + 1), *t = reinterpret_cast<const long long*>(table);
    long long* f = reinterpret_cast<long long*>(feret);
    const dim3 b(256);
    hipLaunchKernelGGL(feret_init_kernel, dim3(shape_grid_for(std::max<int64_t>(2 * total_lines, 5 * n), 256, 65536)), b, 0, s, lines, total_lines, f, n);
    if (total_wg > 0) {
        const dim3 g(shape_grid_for(total_wg, 1, (int64_t)1 << 20));
        hipLaunchKernelGGL(feret_lines_kernel, dim3(shape_grid_for((int64_t)h * w, 256, 65536)), b, 0, s, labels, h, w, n, t, line_off, lines);
        hipLaunchKernelGGL(feret_pairs_kernel<false>, g, b, 0, s, t, n, h, w, line_off, wg_off, (const int*)lines, f);
        hipLaunchKernelGGL(feret_pairs_kernel<true>, g, b, 0, s, t, n, h, w, line_off, wg_off, (const int*)lines, f);
    }
    hipLaunchKernelGGL(feret_finish_kernel, dim3(shape_grid_for(n, 256, 65536)), b, 0, s, f, n, w);
}
