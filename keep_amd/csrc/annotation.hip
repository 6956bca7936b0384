// Polygon annotations to masks: the scan-line fill of rings on level-0 coordinates into a mask in thumbnail geometry, and the count of
// mask pixels under every tile.  Integer arithmetic throughout: every result is held exactly to
// keep_amd.annotation.fill_numpy / tile_counts_numpy.
//
// An edge (a vertex and its successor in the ring, the last joined to the first) crosses the centre line of row i iff
// 2 yl <= Cy_i < 2 yh (half-open: a vertex on a centre line counts once); the crossing takes effect from the first pixel whose centre lies
// on or right of it, column j0, where it adds s weight[ring] to delta[i][j0] (s = +1 upwards).  The prefix sums of a row of delta are the
// winding numbers of its pixels (keep_hip.h has the formulas).
//
//   poly_edges               one thread per vertex, 8 consecutive per thread: ring (binary search in ring_start), successor, signed weight,
//                            clipped row range; the crossing counts scanned inside the block (64-bit: one edge may cross 2^28 rows)
//   poly_scan                one block: the blocks' sums scanned, the total C
//   poly_crossings           one thread per crossing: its edge by two binary searches (block offsets, then the offsets inside the block),
//                            the row, one 64-bit division for j0, one returnless int32 atomicAdd into delta.  The work of a thread does not
//                            depend on the input: a rectangle's four long edges and 10^5 short ones go through the same code
//   poly_rows                one workgroup per row: the inclusive scan of its w + 1 columns in chunks of 1024 with a carried sum, the
//                            inside test, the uint8 output (reads into where given; out may alias it)
//   mask_tile_counts         one wave per tile: the pixels whose centres lie in the tile, and those of them that are set
//
// Pixel indices are int32 (h (w + 1) <= 2^28), vertex ids are int32 (V <= 2^24), crossing ids int64 below 2^31.
#include "common.h"
#include "../../include/keep_hip.h"

namespace keepk {

constexpr int PF_PER_THREAD = POLY_CHUNK / 256;           // 8 consecutive vertices per thread
constexpr int PF_ROW_PER_THREAD = 4;                      // consecutive columns per thread of the row scan
constexpr int PF_ROW_CHUNK = 256 * PF_ROW_PER_THREAD;

// ceil(a / b) for b > 0 (C division truncates towards zero)
__device__ __forceinline__ int pf_ceil_div(int a, int b) {
    const int q = a / b;
    return q + (a - q * b > 0);
}
__device__ __forceinline__ long long pf_ceil_div64(long long a, long long b) {
    const long long q = a / b;
    return q + (a - q * b > 0);
}

// 256 threads: exclusive prefix of v over the block, *total = the block's sum.  s: 4 words of LDS, reusable on return.  The 64-bit
// counterpart of block_exclusive_scan256 (common.h), by wave shuffles
template <typename T>
__device__ __forceinline__ T pf_block_exclusive_scan256(T v, T* s, T* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T a = __shfl_up(incl, o);
        if (lane >= o) incl += a;
    }
    if (lane == 63) s[wave] = incl;
    __syncthreads();
    const T s0 = s[0], s1 = s[1], s2 = s[2], s3 = s[3];
    __syncthreads();
    *total = s0 + s1 + s2 + s3;
    return incl - v + (wave > 0 ? s0 : 0) + (wave > 1 ? s1 : 0) + (wave > 2 ? s2 : 0);
}

struct PolyGeom {
    int d, h, w;
    int ox2, oy2;                                         // 2 ox + d, 2 oy + d: the doubled centre of pixel (0, 0)
};

// edge v of the rings: its successor, s weight[ring] (0 for an edge that never counts) and the clipped rows [lo, hi) it crosses.
// Every index that derives from the caller's arrays is checked: a ring_start that does not ascend, a ring of fewer than 3 vertices,
// a weight outside {-1, 0, 1} or a coordinate beyond +-2^26 leaves the edge without crossings
__device__ __forceinline__ int pf_edge(const long long* __restrict__ vertices, int V, const long long* __restrict__ ring_start, int R,
                                       const int* __restrict__ weight, const PolyGeom g, int v, int* succ, int* sw, int* lo) {
    *succ = v; *sw = 0; *lo = 0;
    int a = 0, b = R;                                     // the largest r in [0, R) with ring_start[r] <= v
    while (b - a > 1) {
        const int m = (a + b) >> 1;
        if (ring_start[m] <= v) a = m; else b = m;
    }
    const long long start = ring_start[a], end = ring_start[a + 1];
    if (start < 0 || start > v || end <= v || end > V || end - start < 3) return 0;
    const int wt = weight[a];
    if (wt != 1 && wt != -1) return 0;
    const int nx = v + 1 < end ? v + 1 : (int)start;
    const long long xa = vertices[2 * (int64_t)v], ya = vertices[2 * (int64_t)v + 1], xb = vertices[2 * (int64_t)nx], yb = vertices[2 * (int64_t)nx + 1];
    constexpr long long lim = POLY_MAX_COORD;
    if (xa < -lim || xa > lim || ya < -lim || ya > lim || xb < -lim || xb > lim || yb < -lim || yb > lim || ya == yb) return 0;
    const int yl = (int)(ya < yb ? ya : yb), yh = (int)(ya < yb ? yb : ya);
    // |2 y - 2 oy - d| < 2^27 + 2^27 + 2^12: 32-bit
    int r0 = pf_ceil_div(2 * yl - g.oy2, 2 * g.d), r1 = pf_ceil_div(2 * yh - g.oy2, 2 * g.d);
    r0 = r0 < 0 ? 0 : r0;
    r1 = r1 > g.h ? g.h : r1;
    if (r1 <= r0) return 0;
    *succ = nx;
    *sw = yb < ya ? wt : -wt;
    *lo = r0;
    return r1 - r0;
}

// ---- edges: counts and their scan -------------------------------------------------------------------------------------------------------
// info[v] = (successor, s weight, first row, 0); off[v] = the crossings of the block's edges before v; sums[block] = the block's crossings
__global__ __launch_bounds__(256)
void poly_edges_kernel(const long long* __restrict__ vertices, int V, const long long* __restrict__ ring_start, int R,
                       const int* __restrict__ weight, PolyGeom g, int4* __restrict__ info, long long* __restrict__ off,
                       long long* __restrict__ sums) {
    __shared__ long long s[4];
    const int v0 = blockIdx.x * POLY_CHUNK + threadIdx.x * PF_PER_THREAD;
    int cnt[PF_PER_THREAD];
    long long mine = 0;
#pragma unroll
    for (int j = 0; j < PF_PER_THREAD; ++j) {
        cnt[j] = 0;
        if (v0 + j < V) {
            int succ, sw, lo;
            cnt[j] = pf_edge(vertices, V, ring_start, R, weight, g, v0 + j, &succ, &sw, &lo);
            info[v0 + j] = make_int4(succ, sw, lo, 0);
            mine += cnt[j];
        }
    }
    long long total;
    long long at = pf_block_exclusive_scan256<long long>(mine, s, &total);
#pragma unroll
    for (int j = 0; j < PF_PER_THREAD; ++j) {
        if (v0 + j < V) off[v0 + j] = at;
        at += cnt[j];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one block: boff[b] = the sums of sums[0, b); *total = C
__global__ __launch_bounds__(256)
void poly_scan_kernel(const long long* __restrict__ sums, int nb, long long* __restrict__ boff, long long* __restrict__ total) {
    __shared__ long long s[4];
    long long carry = 0;
    for (int b0 = 0; b0 < nb; b0 += 256) {
        const int b = b0 + threadIdx.x;
        long long t;
        const long long e = pf_block_exclusive_scan256<long long>(b < nb ? sums[b] : 0, s, &t);
        if (b < nb) boff[b] = carry + e;
        carry += t;
    }
    if (threadIdx.x == 0) *total = carry;
}

// ---- crossings ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void poly_crossings_kernel(const long long* __restrict__ vertices, int V, PolyGeom g, const int4* __restrict__ info,
                           const long long* __restrict__ off, const long long* __restrict__ boff, int nb, long long C,
                           int* __restrict__ delta) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    int a = 0, b = nb;                                    // the largest block with boff <= c: it holds crossing c, since c < C
    while (b - a > 1) {
        const int m = (a + b) >> 1;
        if (boff[m] <= c) a = m; else b = m;
    }
    const long long k0 = c - boff[a];
    int e = a * POLY_CHUNK, e1 = e + POLY_CHUNK < V ? e + POLY_CHUNK : V;      // the largest edge of it with off <= k0: its count is > 0
    while (e1 - e > 1) {
        const int m = (e + e1) >> 1;
        if (off[m] <= k0) e = m; else e1 = m;
    }
    const int4 q = info[e];
    const long long i = q.z + (k0 - off[e]);
    if (q.y == 0 || i < 0 || i >= g.h || (unsigned)q.x >= (unsigned)V) return;      // only arrays changed under the call could ask for this
    const long long xa = vertices[2 * (int64_t)e], ya = vertices[2 * (int64_t)e + 1], xb = vertices[2 * (int64_t)q.x], yb = vertices[2 * (int64_t)q.x + 1];
    const bool up = yb < ya;
    const long long xl = up ? xb : xa, yl = up ? yb : ya, xh = up ? xa : xb, yh = up ? ya : yb;
    if (yh <= yl) return;
    // Cy_i - 2 yl lies in [0, 2 (yh - yl)) < 2^28 and |xh - xl| < 2^28; |2 xl - 2 ox - d| < 2^29: the sum stays below 2^58
    const long long cy = (long long)g.oy2 + 2 * i * g.d;
    const long long num = (cy - 2 * yl) * (xh - xl) + (2 * xl - g.ox2) * (yh - yl);
    long long j0 = pf_ceil_div64(num, 2LL * g.d * (yh - yl));
    j0 = j0 < 0 ? 0 : (j0 > g.w ? g.w : j0);
    atomicAdd(&delta[i * (g.w + 1) + j0], q.y);          // result unused: a returnless add; integer adds commute
}

// ---- rows -------------------------------------------------------------------------------------------------------------------------------------
// out may alias into: every thread reads its own pixels of into before it writes them
__global__ __launch_bounds__(256)
void poly_rows_kernel(const int* __restrict__ delta, int h, int w, int evenodd, int value, const unsigned char* into, unsigned char* out) {
    __shared__ int s[4];
    const int i = blockIdx.x;
    if (i >= h) return;
    const int* row = delta + (int64_t)i * (w + 1);
    int carry = 0;
    for (int c0 = 0; c0 < w; c0 += PF_ROW_CHUNK) {        // the dump column w is never read: nothing lies right of it
        const int j0 = c0 + threadIdx.x * PF_ROW_PER_THREAD;
        int v[PF_ROW_PER_THREAD], mine = 0;
#pragma unroll
        for (int k = 0; k < PF_ROW_PER_THREAD; ++k) {
            v[k] = j0 + k < w ? row[j0 + k] : 0;
            mine += v[k];
        }
        int total;
        int wind = carry + pf_block_exclusive_scan256<int>(mine, s, &total);
#pragma unroll
        for (int k = 0; k < PF_ROW_PER_THREAD; ++k) {
            wind += v[k];
            if (j0 + k < w) {
                const int64_t p = (int64_t)i * w + j0 + k;
                const bool inside = evenodd ? (wind & 1) : (wind > 0);
                out[p] = inside ? (unsigned char)value : (into ? into[p] : (unsigned char)0);
            }
        }
        carry += total;
    }
}

// ---- tile counts ----------------------------------------------------------------------------------------------------------------------------
// the first index whose pixel centre lies on or right of level-0 position x: ceil((2 (x - o) - d) / (2 d)), clipped to [0, n]
__device__ __forceinline__ int pf_first_index(long long x, long long o, long long d, int n) {
    const long long j = pf_ceil_div64(2 * (x - o) - d, 2 * d);
    return (int)(j < 0 ? 0 : (j > n ? n : j));
}

__global__ __launch_bounds__(256)
void mask_tile_counts_kernel(const unsigned char* __restrict__ mask, int h, int w, long long d, long long ox, long long oy,
                             const long long* __restrict__ coords, long long N, long long patch, int2* __restrict__ counts) {
    const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (n >= N) return;                                   // a whole wave leaves: the shuffles below see full waves
    const long long x = coords[2 * n], y = coords[2 * n + 1];
    const int j0 = pf_first_index(x, ox, d, w), j1 = pf_first_index(x + patch, ox, d, w);
    const int i0 = pf_first_index(y, oy, d, h), i1 = pf_first_index(y + patch, oy, d, h);
    const unsigned bw = j1 > j0 ? j1 - j0 : 0, bh = i1 > i0 ? i1 - i0 : 0;
    const unsigned area = bw * bh;                        // <= h w <= 2^30
    int nz = 0;
    for (unsigned k = lane; k < area; k += 64) {
        const unsigned r = k / bw, c = k - r * bw;
        nz += mask[(int64_t)(i0 + r) * w + j0 + c] != 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nz += __shfl_xor(nz, o);
    if (lane == 0) counts[n] = make_int2((int)area, nz);
}

}  // namespace keepk
using namespace keepk;

static inline size_t pf_align(size_t b) { return (b + 255) & ~(size_t)255; }
static int pf_chunks(int64_t V) { return (int)((V + POLY_CHUNK - 1) / POLY_CHUNK); }

size_t poly_fill_workspace_bytes(int64_t h, int64_t w, int64_t V) {
    return pf_align((size_t)h * (size_t)(w + 1) * 4) + pf_align((size_t)V * 16) + pf_align((size_t)V * 8) + 2 * pf_align((size_t)pf_chunks(V) * 8) +
           pf_align(8);
}

namespace {
struct PolyWs { int* delta; int4* info; long long *off, *sums, *boff, *total; };
PolyWs pf_carve(unsigned char* ws, int64_t h, int64_t w, int64_t V) {
    unsigned char* at = ws;
    auto take = [&](size_t bytes) { unsigned char* p = at; at += pf_align(bytes); return p; };
    PolyWs r;
    r.delta = (int*)take((size_t)h * (size_t)(w + 1) * 4);
    r.info = (int4*)take((size_t)V * 16);
    r.off = (long long*)take((size_t)V * 8);
    r.sums = (long long*)take((size_t)pf_chunks(V) * 8);
    r.boff = (long long*)take((size_t)pf_chunks(V) * 8);
    r.total = (long long*)take(8);
    return r;
}
PolyGeom pf_geom(int64_t d, int h, int w, int64_t ox, int64_t oy) {
    PolyGeom g;
    g.d = (int)d; g.h = h; g.w = w;
    g.ox2 = (int)(2 * ox + d); g.oy2 = (int)(2 * oy + d);
    return g;
}
}  // namespace

const int64_t* launch_poly_count(const int64_t* vertices, int64_t V, const int64_t* ring_start, int64_t R, const int* weight, int64_t d, int h,
                                 int w, int64_t ox, int64_t oy, unsigned char* ws, hipStream_t s) {
    const PolyWs p = pf_carve(ws, h, w, V);
    const int nb = pf_chunks(V);
    (void)hipMemsetAsync(p.delta, 0, (size_t)h * (size_t)(w + 1) * 4, s);
    hipLaunchKernelGGL(poly_edges_kernel, dim3(nb), dim3(256), 0, s, reinterpret_cast<const long long*>(vertices), (int)V,
                       reinterpret_cast<const long long*>(ring_start), (int)R, weight, pf_geom(d, h, w, ox, oy), p.info, p.off, p.sums);
    hipLaunchKernelGGL(poly_scan_kernel, dim3(1), dim3(256), 0, s, (const long long*)p.sums, nb, p.boff, p.total);
    return reinterpret_cast<const int64_t*>(p.total);
}

void launch_poly_crossings(const int64_t* vertices, int64_t V, int64_t d, int h, int w, int64_t ox, int64_t oy, int64_t C, unsigned char* ws,
                           hipStream_t s) {
    const PolyWs p = pf_carve(ws, h, w, V);
    hipLaunchKernelGGL(poly_crossings_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const long long*>(vertices), (int)V,
                       pf_geom(d, h, w, ox, oy), (const int4*)p.info, (const long long*)p.off, (const long long*)p.boff, pf_chunks(V), (long long)C,
                       p.delta);
}

void launch_poly_rows(int h, int w, int evenodd, int value, const unsigned char* into, unsigned char* out, unsigned char* ws, hipStream_t s) {
    hipLaunchKernelGGL(poly_rows_kernel, dim3(h), dim3(256), 0, s, (const int*)ws, h, w, evenodd, value, into, out);
}

void launch_mask_tile_counts(const unsigned char* mask, int h, int w, int64_t d, int64_t ox, int64_t oy, const int64_t* coords, int64_t N,
                             int64_t patch, int32_t* counts, hipStream_t s) {
    hipLaunchKernelGGL(mask_tile_counts_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, mask, h, w, (long long)d, (long long)ox,
                       (long long)oy, reinterpret_cast<const long long*>(coords), (long long)N, (long long)patch, reinterpret_cast<int2*>(counts));
}
