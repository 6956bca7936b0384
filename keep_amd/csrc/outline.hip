// Region outlines: the boundary rings of a label image on the corner lattice, with holes, and an outline drawn into an RGB image
// (DESIGN.md section 15).  Integer arithmetic throughout: every result is held exactly to keep_amd.outline.outlines_numpy / draw_numpy.
//
// A pixel p with label l in 1..n has a directed crack edge on side s (0 top +x, 1 right +y, 2 bottom -x, 3 left -y; the region on the
// walker's right) iff the pixel across that side lies outside the image or carries another label; slot = 4 p + s.  The successor map
// (keep_hip.h) is a permutation of the edges, its cycles are the rings.  No thread ever walks a ring: ring identity, order and sums are
// list ranking on cycles.
//
//   outline_count /          edges and corner edges of every pixel from its 3 x 3 neighbourhood (an edge is a corner iff its predecessor
//   outline_total            lies on another side: iff NOT (the pixel behind is in and the pixel behind on the left is out)); per-block
//                            counts, one block adds them up: E and V, no atomics
//   outline_scan /           edges compacted in slot order: pixoff[p] = the id of p's first edge, slot[e] = 4 p + s | corner bit;
//   outline_compact /        succ[e] from the labels: the side t of the pixel q that the table names, whose id is pixoff[q] + the
//   outline_succ             number of q's edges on sides < t
//   outline_min_round        pointer jumping for the ring minimum over corner edges (the leader): state k holds, for every edge, the
//                            minimum over the 2^k edges from it on and the edge 2^k steps ahead.  A minimum is idempotent, so windows
//                            that wrap round the ring are harmless.  Round k also looks whether state k - 1 was already constant along
//                            every ring and says so in flags[k] (one store per workgroup that saw a difference); round k + 1 returns at
//                            once when flags[k] is still 0, and so does every round after it: the rounds that do work follow the
//                            longest ring, ceil(log2(its edges)), not E.  outline_pick finds the state that was complete
//   outline_rank_init /      the rings cut open in front of their leaders; suffix sums by pointer jumping of three weights at once:
//   outline_rank_round       corner edges (-> the position of a vertex in its ring, and nvert at the leader), edges (nedge) and the
//                            shoelace term of the unit edge (area2).  Order-independent integer sums without one atomic: a ring of 10^6
//                            edges costs what 10^6 edges of small rings cost per round.  The same flags / pick scheme
//   outline_leader_count /   stable compaction of the leaders (edges with lead[e] = e) in edge order = ascending leader slot: the ring
//   outline_scan /           ids, and with the exclusive sums of nvert the rings' first rows; the ring rows
//   outline_rings
//   outline_vertices         every corner edge writes its start vertex to row start[ring] + nvert - (corners from it to the end)
//   outline_draw_rows /      out = color where a pixel's (2 width + 1)^2 window leaves the image or holds another label: separable, a row
//   outline_draw             pass (the window's row is uniform) into one byte per pixel, then a column pass
//
// Pixel indices, slots and edge ids are int32 (H W <= 2^28, so 4 p + s < 2^30 and bit 30 is free for the corner flag).
#include "common.h"
#include "../../include/keep_hip.h"

namespace keepk {

constexpr int OL_PER_THREAD = OUTLINE_CHUNK / 256;        // 8 consecutive pixels / edges per thread
constexpr int OL_NONE = 0x7fffffff;
constexpr int OL_CORNER = 1 << 30;
constexpr int OL_EDGE_BLOCKS = 4096;                      // cap of the grid-stride kernels over the edges

__device__ __forceinline__ bool ol_in(const int* __restrict__ labels, int H, int W, int x, int y, int l) {
    return (unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H && labels[y * W + x] == l;
}

// bits 0..3: pixel p has an edge on side s; *corners: that edge is a corner.  0 for a label outside 1..n
__device__ __forceinline__ unsigned ol_pixel_bits(const int* __restrict__ labels, int H, int W, int n, int p, unsigned* corners) {
    *corners = 0;
    const int l = labels[p];
    if (l < 1 || l > n) return 0;
    const int y = p / W, x = p - y * W;
    const bool N = ol_in(labels, H, W, x, y - 1, l), S = ol_in(labels, H, W, x, y + 1, l), Wt = ol_in(labels, H, W, x - 1, y, l),
               Et = ol_in(labels, H, W, x + 1, y, l), NW = ol_in(labels, H, W, x - 1, y - 1, l), NE = ol_in(labels, H, W, x + 1, y - 1, l),
               SW = ol_in(labels, H, W, x - 1, y + 1, l), SE = ol_in(labels, H, W, x + 1, y + 1, l);
    const unsigned e = (unsigned)!N | (unsigned)!Et << 1 | (unsigned)!S << 2 | (unsigned)!Wt << 3;
    // the predecessor runs straight into side s iff the pixel behind is in and the one behind on the left is out
    const unsigned c = (unsigned)!(Wt && !NW) | (unsigned)!(N && !NE) << 1 | (unsigned)!(Et && !SE) << 2 | (unsigned)!(S && !SW) << 3;
    *corners = c & e;
    return e;
}

// the start vertex of side s of pixel (x, y), and the edge's direction
__device__ __forceinline__ void ol_vertex(int x, int y, int s, int* vx, int* vy) {
    *vx = x + (s == 1 || s == 2);
    *vy = y + (s >= 2);
}
__device__ __forceinline__ int ol_dx(int s) { return (s == 0) - (s == 2); }
__device__ __forceinline__ int ol_dy(int s) { return (s == 1) - (s == 3); }

// ---- counting and compaction --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void outline_count_kernel(const int* __restrict__ labels, int H, int W, int n, int2* __restrict__ counts) {
    __shared__ int s[256];
    const int npix = H * W;
    const int64_t p0 = (int64_t)blockIdx.x * OUTLINE_CHUNK + (int64_t)threadIdx.x * OL_PER_THREAD;
    int e = 0, c = 0;
#pragma unroll
    for (int j = 0; j < OL_PER_THREAD; ++j) {
        if (p0 + j < npix) {
            unsigned cb;
            e += __popc(ol_pixel_bits(labels, H, W, n, (int)(p0 + j), &cb));
            c += __popc(cb);
        }
    }
    int te, tc;
    block_exclusive_scan256(e, s, &te);
    block_exclusive_scan256(c, s, &tc);
    if (threadIdx.x == 0) counts[blockIdx.x] = make_int2(te, tc);
}

// one block: out[0], out[1] = the sums of both fields
__global__ __launch_bounds__(256)
void outline_total_kernel(const int2* __restrict__ counts, int nb, int64_t* __restrict__ out) {
    __shared__ long long s[2][4];
    long long e = 0, c = 0;
    for (int b = threadIdx.x; b < nb; b += 256) { e += counts[b].x; c += counts[b].y; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { e += __shfl_xor(e, o); c += __shfl_xor(c, o); }
    if ((threadIdx.x & 63) == 0) { s[0][threadIdx.x >> 6] = e; s[1][threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = s[0][0] + s[0][1] + s[0][2] + s[0][3];
        out[1] = s[1][0] + s[1][1] + s[1][2] + s[1][3];
    }
}

// one block: offsets[b] = the sums of counts[0, b), field by field; *total_x (nullable) = the sum of all x
__global__ __launch_bounds__(256)
void outline_scan_kernel(const int2* __restrict__ counts, int nb, int2* __restrict__ offsets, int64_t* __restrict__ total_x) {
    __shared__ int s[256];
    int cx = 0, cy = 0;
    for (int b0 = 0; b0 < nb; b0 += 256) {
        const int b = b0 + threadIdx.x;
        const int2 v = b < nb ? counts[b] : make_int2(0, 0);
        int tx, ty;
        const int ex = block_exclusive_scan256(v.x, s, &tx), ey = block_exclusive_scan256(v.y, s, &ty);
        if (b < nb) offsets[b] = make_int2(cx + ex, cy + ey);
        cx += tx; cy += ty;
    }
    if (threadIdx.x == 0 && total_x) *total_x = cx;
}

__global__ __launch_bounds__(256)
void outline_compact_kernel(const int* __restrict__ labels, int H, int W, int n, const int2* __restrict__ offsets, int E,
                            int* __restrict__ pixoff, int* __restrict__ slot) {
    __shared__ int s[256];
    const int npix = H * W;
    const int64_t p0 = (int64_t)blockIdx.x * OUTLINE_CHUNK + (int64_t)threadIdx.x * OL_PER_THREAD;
    unsigned ebits = 0, cbits = 0;                    // four bits per pixel
#pragma unroll
    for (int j = 0; j < OL_PER_THREAD; ++j) {
        if (p0 + j < npix) {
            unsigned cb;
            ebits |= ol_pixel_bits(labels, H, W, n, (int)(p0 + j), &cb) << (4 * j);
            cbits |= cb << (4 * j);
        }
    }
    int total;
    int e = offsets[blockIdx.x].x + block_exclusive_scan256(__popc(ebits), s, &total);
#pragma unroll
    for (int j = 0; j < OL_PER_THREAD; ++j) {
        if (p0 + j < npix) {
            const int p = (int)(p0 + j);
            pixoff[p] = e;
#pragma unroll
            for (int sd = 0; sd < 4; ++sd) {
                if (ebits >> (4 * j + sd) & 1u) {
                    if (e < E) slot[e] = (4 * p + sd) | ((cbits >> (4 * j + sd) & 1u) ? OL_CORNER : 0);     // E is the caller's: never past it
                    ++e;
                }
            }
        }
    }
}

// succ[e] and state 0 of the minimum: (the edge itself if it is a corner, the successor)
__global__ __launch_bounds__(256)
void outline_succ_kernel(const int* __restrict__ labels, int H, int W, int conn8, const int* __restrict__ pixoff, const int* __restrict__ slot,
                         int E, int* __restrict__ succ, int2* __restrict__ state) {
    for (int e = blockIdx.x * 256 + threadIdx.x; e < E; e += gridDim.x * 256) {
        const int sl = slot[e], ps = sl & (OL_CORNER - 1), p = ps >> 2, s = ps & 3;
        const int l = labels[p];
        const int y = p / W, x = p - y * W;
        const int arx = x + ol_dx(s), ary = y + ol_dy(s);                         // ahead on the right
        const int alx = arx + ol_dx((s + 3) & 3), aly = ary + ol_dy((s + 3) & 3);  // ahead on the left: across side s
        const bool ar = ol_in(labels, H, W, arx, ary, l), al = ol_in(labels, H, W, alx, aly, l);
        int qx, qy, t;
        if (al && (ar || conn8)) { qx = alx; qy = aly; t = (s + 3) & 3; }         // left (with connectivity 8 through the saddle too)
        else if (ar) { qx = arx; qy = ary; t = s; }                               // straight
        else { qx = x; qy = y; t = (s + 1) & 3; }                                 // right
        int k = 0;                                                                // q's edges on the sides before t
        if (t > 0) k += !ol_in(labels, H, W, qx, qy - 1, l);
        if (t > 1) k += !ol_in(labels, H, W, qx + 1, qy, l);
        if (t > 2) k += !ol_in(labels, H, W, qx, qy + 1, l);
        int sc = pixoff[qy * W + qx] + k;
        sc = sc < E ? sc : E - 1;                                                 // only a wrong E could ask for this
        succ[e] = sc;
        state[e] = make_int2((sl & OL_CORNER) ? e : OL_NONE, sc);
    }
}

// ---- the leader: ring minimum over corner edges ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void outline_min_round_kernel(const int2* __restrict__ in, int2* __restrict__ out, const int* __restrict__ succ, int E,
                              int* __restrict__ flags, int k) {
    if (k >= 2 && flags[k - 1] == 0) return;          // state k - 2 was complete (or an earlier one: that round returned as well)
    int bad = 0;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < E; e += gridDim.x * 256) {
        const int2 a = in[e], b = in[a.y];
        bad |= a.x != in[succ[e]].x;
        out[e] = make_int2(min(a.x, b.x), b.y);
    }
    if (__syncthreads_or(bad) && threadIdx.x == 0) flags[k] = 1;
}

// pick[0] = the first state known to be complete: k - 1 for the first round k >= 1 whose flag stayed 0
__global__ void outline_pick_kernel(const int* __restrict__ flags, int rounds, int* __restrict__ pick) {
    if (threadIdx.x || blockIdx.x) return;
    int k = 1;
    while (k <= rounds && flags[k]) ++k;
    pick[0] = k - 1;
}

// ---- position, nvert, nedge, area2: suffix sums along the rings cut open in front of their leaders ------------------------------
// mins0 / mins1 may alias w0 (each thread reads its own entry before it writes it)
__global__ __launch_bounds__(256)
void outline_rank_init_kernel(const int2* mins0, const int2* mins1, const int* __restrict__ pick, const int* __restrict__ succ,
                              const int* __restrict__ slot, int W, int E, int* __restrict__ lead, int4* __restrict__ a0, long long* w0) {
    const int2* mins = (pick[0] & 1) ? mins1 : mins0;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < E; e += gridDim.x * 256) {
        const int m = mins[e].x;
        const int sl = slot[e], ps = sl & (OL_CORNER - 1), p = ps >> 2, s = ps & 3;
        const int y = p / W, x = p - y * W;
        int vx, vy;
        ol_vertex(x, y, s, &vx, &vy);
        const int sc = succ[e];
        lead[e] = m;
        a0[e] = make_int4(sc == m ? -1 : sc, (sl & OL_CORNER) ? 1 : 0, 1, 0);
        w0[e] = (long long)vx * ol_dy(s) - (long long)ol_dx(s) * vy;              // x0 y1 - x1 y0 of the unit edge
    }
}

__global__ __launch_bounds__(256)
void outline_rank_round_kernel(const int4* __restrict__ ina, const long long* __restrict__ inw, int4* __restrict__ outa,
                               long long* __restrict__ outw, int E, int* __restrict__ flags, int k) {
    if (k >= 2 && flags[k - 1] == 0) return;
    int bad = 0;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < E; e += gridDim.x * 256) {
        int4 a = ina[e];
        long long w = inw[e];
        if (a.x >= 0) {
            bad = 1;
            const int4 b = ina[a.x];
            w += inw[a.x];
            a.y += b.y; a.z += b.z; a.x = b.x;
        }
        outa[e] = a;
        outw[e] = w;
    }
    if (__syncthreads_or(bad) && threadIdx.x == 0) flags[k] = 1;
}

// ---- ring ids and rows ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void outline_leader_count_kernel(const int* __restrict__ lead, const int4* __restrict__ a0, const int4* __restrict__ a1,
                                 const int* __restrict__ pick, int E, int2* __restrict__ counts) {
    __shared__ int s[256];
    const int4* a = (pick[0] & 1) ? a1 : a0;
    const int64_t e0 = (int64_t)blockIdx.x * OUTLINE_CHUNK + (int64_t)threadIdx.x * OL_PER_THREAD;
    int nl = 0, nv = 0;
#pragma unroll
    for (int j = 0; j < OL_PER_THREAD; ++j) {
        const int64_t e = e0 + j;
        if (e < E && lead[e] == (int)e) { ++nl; nv += a[e].y; }
    }
    int tl, tv;
    block_exclusive_scan256(nl, s, &tl);
    block_exclusive_scan256(nv, s, &tv);
    if (threadIdx.x == 0) counts[blockIdx.x] = make_int2(tl, tv);
}

__global__ __launch_bounds__(256)
void outline_rings_kernel(const int* __restrict__ labels, int W, const int* __restrict__ slot, const int* __restrict__ lead,
                          const int4* __restrict__ a0, const int4* __restrict__ a1, const long long* w0, const long long* w1,
                          const int* __restrict__ pick, int E, const int2* __restrict__ offsets, int* __restrict__ start_of,
                          long long* __restrict__ rings, int64_t ring_cap) {
    __shared__ int s[256];
    const int4* a = (pick[0] & 1) ? a1 : a0;
    const long long* w = (pick[0] & 1) ? w1 : w0;
    const int64_t e0 = (int64_t)blockIdx.x * OUTLINE_CHUNK + (int64_t)threadIdx.x * OL_PER_THREAD;
    int nl = 0, nv = 0;
    unsigned is = 0;
#pragma unroll
    for (int j = 0; j < OL_PER_THREAD; ++j) {
        const int64_t e = e0 + j;
        if (e < E && lead[e] == (int)e) { is |= 1u << j; ++nl; nv += a[e].y; }
    }
    int tl, tv;
    int id = offsets[blockIdx.x].x + block_exclusive_scan256(nl, s, &tl);
    int start = offsets[blockIdx.x].y + block_exclusive_scan256(nv, s, &tv);
#pragma unroll
    for (int j = 0; j < OL_PER_THREAD; ++j) {
        if (!(is >> j & 1u)) continue;
        const int e = (int)(e0 + j);
        const int4 q = a[e];
        const long long area2 = w[e];
        start_of[e] = start;
        if (id < ring_cap) {
            const int ps = slot[e] & (OL_CORNER - 1), p = ps >> 2, sd = ps & 3;
            const int y = p / W, x = p - y * W;
            int vx, vy;
            ol_vertex(x, y, sd, &vx, &vy);
            long long* row = rings + (int64_t)id * OUTLINE_COLS;
            row[0] = labels[p]; row[1] = start; row[2] = q.y; row[3] = q.z; row[4] = area2; row[5] = vx; row[6] = vy; row[7] = area2 < 0;
        }
        ++id;
        start += q.y;
    }
}

__global__ __launch_bounds__(256)
void outline_vertices_kernel(int W, const int* __restrict__ slot, const int* __restrict__ lead, const int4* __restrict__ a0,
                             const int4* __restrict__ a1, const int* __restrict__ pick, int E, const int* __restrict__ start_of, int64_t V,
                             int* __restrict__ vertices) {
    const int4* a = (pick[0] & 1) ? a1 : a0;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < E; e += gridDim.x * 256) {
        const int sl = slot[e];
        if (!(sl & OL_CORNER)) continue;
        const int ps = sl & (OL_CORNER - 1), p = ps >> 2, s = ps & 3;
        const int y = p / W, x = p - y * W;
        const int m = lead[e];
        if ((unsigned)m >= (unsigned)E) continue;     // only a wrong E could leave a ring without a leader
        const int64_t row = (int64_t)start_of[m] + a[m].y - a[e].y;
        if (row < 0 || row >= V) continue;            // V is the caller's: never past it
        int vx, vy;
        ol_vertex(x, y, s, &vx, &vy);
        vertices[2 * row] = vx;
        vertices[2 * row + 1] = vy;
    }
}

// ---- drawing -----------------------------------------------------------------------------------------------------------------------
// rowok[p] = 1 iff labels[p] > 0 and the 2 width + 1 pixels of p's row around it lie inside the image and carry labels[p]
__global__ __launch_bounds__(256)
void outline_draw_rows_kernel(const int* __restrict__ labels, int H, int W, int width, unsigned char* __restrict__ rowok) {
    const int npix = H * W;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < npix; p += gridDim.x * 256) {
        const int l = labels[p];
        const int y = p / W, x = p - y * W;
        bool ok = l > 0 && x - width >= 0 && x + width < W;
        for (int k = 1; ok && k <= width; ++k) ok = labels[p - k] == l && labels[p + k] == l;
        rowok[p] = ok;
    }
}

__global__ __launch_bounds__(256)
void outline_draw_kernel(const int* __restrict__ labels, int H, int W, int width, const unsigned char* __restrict__ rowok,
                         const unsigned char* rgb_in, unsigned char* rgb_out, unsigned color) {
    const int npix = H * W;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < npix; p += gridDim.x * 256) {
        const int l = labels[p];
        const int y = p / W;
        bool inner = l <= 0 || (rowok[p] && y - width >= 0 && y + width < H);      // background is never drawn
        if (l > 0)
            for (int k = 1; inner && k <= width; ++k)
                inner = labels[p - k * W] == l && labels[p + k * W] == l && rowok[p - k * W] && rowok[p + k * W];
        const int64_t o = (int64_t)p * 3;
        if (inner) {
            if (rgb_out != rgb_in) { rgb_out[o] = rgb_in[o]; rgb_out[o + 1] = rgb_in[o + 1]; rgb_out[o + 2] = rgb_in[o + 2]; }
        } else {
            rgb_out[o] = (unsigned char)(color & 255); rgb_out[o + 1] = (unsigned char)(color >> 8 & 255); rgb_out[o + 2] = (unsigned char)(color >> 16 & 255);
        }
    }
}

}  // namespace keepk
using namespace keepk;

static inline size_t ol_align(size_t b) { return (b + 255) & ~(size_t)255; }
static unsigned ol_grid(int64_t items) {
    const int64_t b = (items + 255) / 256;
    return (unsigned)(b > OL_EDGE_BLOCKS ? OL_EDGE_BLOCKS : (b < 1 ? 1 : b));
}
static int ol_chunks(int64_t items) { return (int)((items + OUTLINE_CHUNK - 1) / OUTLINE_CHUNK); }
// jumping rounds that are launched: state k covers 2^k edges, a ring has at most E, and one more round sees that it was complete
static int ol_rounds(int64_t E) {
    int k = 0;
    while (((int64_t)1 << k) < E) ++k;
    return k + 2;
}

size_t outline_count_workspace_bytes(int64_t npix) { return ol_align((size_t)ol_chunks(npix) * sizeof(int2)); }

void launch_outline_count(const int* labels, int H, int W, int n, unsigned char* ws, int64_t* counts_out, hipStream_t s) {
    const int nb = ol_chunks((int64_t)H * W);
    int2* counts = reinterpret_cast<int2*>(ws);
    hipLaunchKernelGGL(outline_count_kernel, dim3(nb), dim3(256), 0, s, labels, H, W, n, counts);
    hipLaunchKernelGGL(outline_total_kernel, dim3(1), dim3(256), 0, s, (const int2*)counts, nb, counts_out);
}

size_t outline_trace_workspace_bytes(int64_t npix, int64_t E) {
    const size_t chunks = (size_t)ol_chunks(npix > E ? npix : E);
    return ol_align((size_t)npix * 4) + 3 * ol_align((size_t)E * 4) + 2 * ol_align((size_t)E * 16) + 2 * ol_align((size_t)E * 8) +
           2 * ol_align(chunks * sizeof(int2)) + ol_align(OUTLINE_FLAG_WORDS * sizeof(int));
}

void launch_outline_trace(const int* labels, int H, int W, int n, int conn8, int E, int64_t V, unsigned char* ws, int* vertices, int64_t* rings,
                          int64_t ring_cap, int64_t* r_out, hipStream_t s) {
    const int64_t npix = (int64_t)H * W;
    const size_t chunks = (size_t)ol_chunks(npix > E ? npix : E);
    unsigned char* at = ws;
    auto take = [&](size_t bytes) { unsigned char* p = at; at += ol_align(bytes); return p; };
    int* pixoff = (int*)take((size_t)npix * 4);
    int* slot = (int*)take((size_t)E * 4);
    int* succ = (int*)take((size_t)E * 4);                // start_of once the rings are cut open
    int* lead = (int*)take((size_t)E * 4);
    int4* a[2] = {(int4*)take((size_t)E * 16), (int4*)take((size_t)E * 16)};
    long long* w[2] = {(long long*)take((size_t)E * 8), (long long*)take((size_t)E * 8)};      // the two states of the minimum first
    int2* counts = (int2*)take(chunks * sizeof(int2));
    int2* offsets = (int2*)take(chunks * sizeof(int2));
    int* flags = (int*)take(OUTLINE_FLAG_WORDS * sizeof(int));
    int* flags1 = flags, *flags2 = flags + 40, *pick1 = flags + 80, *pick2 = flags + 81;
    int2* mins[2] = {(int2*)w[0], (int2*)w[1]};
    const dim3 b(256), ge(ol_grid(E));
    const int nbp = ol_chunks(npix), nbe = ol_chunks(E), rounds = ol_rounds(E);

    (void)hipMemsetAsync(flags, 0, OUTLINE_FLAG_WORDS * sizeof(int), s);
    hipLaunchKernelGGL(outline_count_kernel, dim3(nbp), b, 0, s, labels, H, W, n, counts);
    hipLaunchKernelGGL(outline_scan_kernel, dim3(1), b, 0, s, (const int2*)counts, nbp, offsets, (int64_t*)nullptr);
    hipLaunchKernelGGL(outline_compact_kernel, dim3(nbp), b, 0, s, labels, H, W, n, (const int2*)offsets, E, pixoff, slot);
    hipLaunchKernelGGL(outline_succ_kernel, ge, b, 0, s, labels, H, W, conn8, (const int*)pixoff, (const int*)slot, E, succ, mins[0]);
    for (int k = 1; k <= rounds; ++k)
        hipLaunchKernelGGL(outline_min_round_kernel, ge, b, 0, s, (const int2*)mins[(k - 1) & 1], mins[k & 1], (const int*)succ, E, flags1, k);
    hipLaunchKernelGGL(outline_pick_kernel, dim3(1), dim3(64), 0, s, (const int*)flags1, rounds, pick1);
    hipLaunchKernelGGL(outline_rank_init_kernel, ge, b, 0, s, (const int2*)mins[0], (const int2*)mins[1], (const int*)pick1, (const int*)succ,
                       (const int*)slot, W, E, lead, a[0], w[0]);
    for (int k = 1; k <= rounds; ++k)
        hipLaunchKernelGGL(outline_rank_round_kernel, ge, b, 0, s, (const int4*)a[(k - 1) & 1], (const long long*)w[(k - 1) & 1], a[k & 1],
                           w[k & 1], E, flags2, k);
    hipLaunchKernelGGL(outline_pick_kernel, dim3(1), dim3(64), 0, s, (const int*)flags2, rounds, pick2);
    hipLaunchKernelGGL(outline_leader_count_kernel, dim3(nbe), b, 0, s, (const int*)lead, (const int4*)a[0], (const int4*)a[1],
                       (const int*)pick2, E, counts);
    hipLaunchKernelGGL(outline_scan_kernel, dim3(1), b, 0, s, (const int2*)counts, nbe, offsets, r_out);
    hipLaunchKernelGGL(outline_rings_kernel, dim3(nbe), b, 0, s, labels, W, (const int*)slot, (const int*)lead, (const int4*)a[0],
                       (const int4*)a[1], (const long long*)w[0], (const long long*)w[1], (const int*)pick2, E, (const int2*)offsets, succ,
                       reinterpret_cast<long long*>(rings), ring_cap);
    hipLaunchKernelGGL(outline_vertices_kernel, ge, b, 0, s, W, (const int*)slot, (const int*)lead, (const int4*)a[0], (const int4*)a[1],
                       (const int*)pick2, E, (const int*)succ, V, vertices);
}

void launch_outline_draw(const int* labels, int H, int W, const unsigned char* rgb_in, unsigned char* rgb_out, unsigned color, int width,
                         unsigned char* rowok, hipStream_t s) {
    const dim3 g(ol_grid((int64_t)H * W)), b(256);
    hipLaunchKernelGGL(outline_draw_rows_kernel, g, b, 0, s, labels, H, W, width, rowok);
    hipLaunchKernelGGL(outline_draw_kernel, g, b, 0, s, labels, H, W, width, (const unsigned char*)rowok, rgb_in, rgb_out, color);
}
