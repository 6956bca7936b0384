// Tile scores rasterised onto the slide thumbnail.  Integer arithmetic throughout: every result is held
// exactly to keep_amd.heatmap.raster_numpy / mean_numpy / render_numpy.
//
//   heat_accumulate   scatter: one wave per tile.  The tile's footprint in raster pixels (floor division of its level-0 corners by
//                     the downsample, clipped to the raster) is worked out once per tile; the lanes then run along x inside a
//                     footprint row and on into the next rows, so one wave instruction adds into a few contiguous row segments.
//                     Each (tile, pixel) pair is ONE no-return 64-bit integer atomic add at agent scope of (1 << 40) | q, q the
//                     value in 16-bit fixed point: bits 0..39 of a pixel sum q, bits 40..63 count the tiles.  Integer sums do not
//                     depend on the order of arrival, so the raster is the same however the tiles are split over calls.
//   heat_mean         one pass: accumulator -> fp32 mean (sum / (65535 count), divided in double), int32 count, {0,255} sum > 0
//   heat_render       one pass: accumulator (+ thumbnail, + mask) -> colour index by an integer rule -> LUT (in LDS) -> blend.  CLAM's
//                     rank percentiles and blur come before it as calls of their own: keep_sort_f32 / keep_rank_f32 (rank.hip) on
//                     the tile values, keep_heat_smooth (below) on the accumulator
//   heat_smooth_row / _col   the Gaussian under the support, two passes (described where they stand)
//
// Pixel indices are int32 (h w <= 2^30, checked by the caller); offsets into the accumulator (8 bytes per pixel) are int64.
#include "common.h"
#include "../../include/keep_hip.h"

namespace keepk {

typedef unsigned long long heat_acc_t;
constexpr int HEAT_COUNT_SHIFT = 40;
constexpr heat_acc_t HEAT_SUM_MASK = ((heat_acc_t)1 << HEAT_COUNT_SHIFT) - 1;

// floor(a / d) for d >= 1, also for a < 0
__device__ __forceinline__ int64_t heat_floor_div(int64_t a, int64_t d) {
    const int64_t q = a / d;
    return (a % d != 0 && a < 0) ? q - 1 : q;
}

__global__ __launch_bounds__(256)
void heat_accumulate_kernel(const int64_t* __restrict__ coords, const float* __restrict__ values, int64_t n, int64_t P, int64_t d,
                            int h, int w, int64_t ox, int64_t oy, heat_acc_t* __restrict__ acc) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < n; t += nwaves) {
        const float v = values[t];
        if (v != v) continue;                         // NaN: the tile is skipped (fmaxf(NaN, 0) would make it a 0)
        const int q = __float2int_rn(fminf(fmaxf(v, 0.f), 1.f) * 65535.f);
        // the footprint, once per tile; differences wrap like numpy's int64 and the clip below keeps any result inside the raster
        const int64_t x = (int64_t)((uint64_t)coords[2 * t] - (uint64_t)ox), y = (int64_t)((uint64_t)coords[2 * t + 1] - (uint64_t)oy);
        const int64_t x0 = heat_floor_div(x, d), x1 = heat_floor_div((int64_t)((uint64_t)x + (uint64_t)P), d);
        const int64_t y0 = heat_floor_div(y, d), y1 = heat_floor_div((int64_t)((uint64_t)y + (uint64_t)P), d);
        const int64_t c0 = x0 > 0 ? x0 : 0, c1 = x1 < w ? x1 : w, r0 = y0 > 0 ? y0 : 0, r1 = y1 < h ? y1 : h;
        if (c1 <= c0 || r1 <= r0) continue;           // off the raster, or empty
        const int fw = (int)(c1 - c0), fh = (int)(r1 - r0);
        const int64_t npx = (int64_t)fw * fh;
        const int dr = 64 / fw, dc = 64 - dr * fw;    // what 64 pixels further along the footprint means in (row, column)
        int r = lane / fw, c = lane - r * fw;
        const heat_acc_t add = ((heat_acc_t)1 << HEAT_COUNT_SHIFT) | (heat_acc_t)q;
        heat_acc_t* base = acc + (r0 * (int64_t)w + c0);
        for (int64_t i = lane; i < npx; i += 64) {    // i < npx <=> r < fh, and c < fw always: inside the clipped footprint
            (void)__hip_atomic_fetch_add(base + ((int64_t)r * w + c), add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            c += dc;
            r += dr;
            if (c >= fw) {
                c -= fw;
                ++r;
            }
        }
    }
}

// Token-cell values of the tiles (keep_heat_accumulate_cells): the footprint and the walk over it are heat_accumulate's, one wave per
// tile; what a pixel adds is no longer the tile's one value but that of the cell of the tile's gh x gw grid (cells of cw x ch level-0 units) under the
// pixel's upper-left corner, clamped into the grid: a footprint pixel may start up to d - 1 units before the tile.  Still ONE add of (1 << 40) | q per
// (tile, pixel), so the count field counts tiles; a NaN cell adds nothing to its pixels.  rel = X d - x lies in (-d, P): 32 bits (P <= 2^30, d <= cw).
__global__ __launch_bounds__(256)
void heat_accumulate_cells_kernel(const int64_t* __restrict__ coords, const float* __restrict__ values, int64_t n, int gh, int gw, int cw, int ch,
                                  int64_t P, int64_t d, int h, int w, int64_t ox, int64_t oy, heat_acc_t* __restrict__ acc) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < n; t += nwaves) {
        const int64_t x = (int64_t)((uint64_t)coords[2 * t] - (uint64_t)ox), y = (int64_t)((uint64_t)coords[2 * t + 1] - (uint64_t)oy);
        const int64_t x0 = heat_floor_div(x, d), x1 = heat_floor_div((int64_t)((uint64_t)x + (uint64_t)P), d);
        const int64_t y0 = heat_floor_div(y, d), y1 = heat_floor_div((int64_t)((uint64_t)y + (uint64_t)P), d);
        const int64_t c0 = x0 > 0 ? x0 : 0, c1 = x1 < w ? x1 : w, r0 = y0 > 0 ? y0 : 0, r1 = y1 < h ? y1 : h;
        if (c1 <= c0 || r1 <= r0) continue;           // off the raster, or empty
        const int fw = (int)(c1 - c0), fh = (int)(r1 - r0);
        const int64_t npx = (int64_t)fw * fh;
        const int dr = 64 / fw, dc = 64 - dr * fw;
        int r = lane / fw, c = lane - r * fw;
        const int relx0 = (int)(c0 * d - x), rely0 = (int)(r0 * d - y), di = (int)d;     // of footprint pixel (0, 0); > -d
        const float* __restrict__ cells = values + t * ((int64_t)gh * gw);
        heat_acc_t* base = acc + (r0 * (int64_t)w + c0);
        for (int64_t i = lane; i < npx; i += 64) {    // i < npx <=> r < fh, and c < fw always: inside the clipped footprint
            const int rx = relx0 + c * di, ry = rely0 + r * di;
            const int cx = rx < 0 ? 0 : min(rx / cw, gw - 1), cy = ry < 0 ? 0 : min(ry / ch, gh - 1);
            const float v = cells[cy * gw + cx];
            if (v == v) {
                const int q = __float2int_rn(fminf(fmaxf(v, 0.f), 1.f) * 65535.f);
                (void)__hip_atomic_fetch_add(base + ((int64_t)r * w + c), ((heat_acc_t)1 << HEAT_COUNT_SHIFT) | (heat_acc_t)q, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
            }
            c += dc;
            r += dr;
            if (c >= fw) {
                c -= fw;
                ++r;
            }
        }
    }
}

__device__ __forceinline__ void heat_mean_one(heat_acc_t a, float uncovered, float& mean, int& count, unsigned char& pred) {
    const heat_acc_t s = a & HEAT_SUM_MASK, c = a >> HEAT_COUNT_SHIFT;
    count = (int)c;
    pred = s ? 255 : 0;
    mean = c ? (float)((double)s / (double)(65535ull * c)) : uncovered;
}

// four pixels per thread; vec: every pointer given is aligned for the 16-byte (pred: 4-byte) accesses
__global__ __launch_bounds__(256)
void heat_mean_kernel(const heat_acc_t* __restrict__ acc, int n, float uncovered, float* __restrict__ mean, int* __restrict__ count,
                      unsigned char* __restrict__ pred, int vec) {
    const int groups = (n + 3) / 4;
    for (int g = blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
        const int i = g * 4;
        if (vec && i + 4 <= n) {
            const ulonglong2 a01 = *reinterpret_cast<const ulonglong2*>(acc + i), a23 = *reinterpret_cast<const ulonglong2*>(acc + i + 2);
            float4 m;
            int4 c;
            uchar4 p;
            heat_mean_one(a01.x, uncovered, m.x, c.x, p.x);
            heat_mean_one(a01.y, uncovered, m.y, c.y, p.y);
            heat_mean_one(a23.x, uncovered, m.z, c.z, p.z);
            heat_mean_one(a23.y, uncovered, m.w, c.w, p.w);
            if (mean) *reinterpret_cast<float4*>(mean + i) = m;
            if (count) *reinterpret_cast<int4*>(count + i) = c;
            if (pred) *reinterpret_cast<uchar4*>(pred + i) = p;
        } else {
            for (int k = i; k < n && k < i + 4; ++k) {
                float m;
                int c;
                unsigned char p;
                heat_mean_one(acc[k], uncovered, m, c, p);
                if (mean) mean[k] = m;
                if (count) count[k] = c;
                if (pred) pred[k] = p;
            }
        }
    }
}

// one pixel: (R | G << 8 | B << 16) of the output
__device__ __forceinline__ unsigned heat_render_one(heat_acc_t a, bool masked_in, unsigned under, const unsigned char* lut, int alpha,
                                                    int64_t lo, int64_t span, int64_t min16) {
    const int64_t S = (int64_t)(a & HEAT_SUM_MASK), c = (int64_t)(a >> HEAT_COUNT_SHIFT);
    if (c == 0 || !masked_in || S < min16 * c) return under;
    // the windowed mean scaled to 0..255, rounded half up: S < 2^40, c < 2^24, span < 2^16, so everything stays below 2^50
    const int64_t rel = S - lo * c;
    int idx = 0;
    if (rel > 0) {
        const uint64_t qd = (uint64_t)(2 * 255 * rel + span * c) / (uint64_t)(2 * span * c);
        idx = qd > 255 ? 255 : (int)qd;
    }
    unsigned out = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const unsigned u = (under >> (8 * ch)) & 255u;
        out |= (((unsigned)alpha * lut[idx * 3 + ch] + (unsigned)(256 - alpha) * u + 128u) >> 8) << (8 * ch);
    }
    return out;
}

// four pixels per thread -> 12 output bytes; vec: out (and mask, if given) are 4-byte aligned.  The thumbnail is read by bytes:
// its row and pixel strides are the caller's.
__global__ __launch_bounds__(256)
void heat_render_kernel(const heat_acc_t* __restrict__ acc, int h, int w, const unsigned char* __restrict__ thumb, int64_t row_stride, int ps,
                        unsigned bg, const unsigned char* __restrict__ mask, const unsigned char* __restrict__ lut, int alpha, int lo16,
                        int hi16, int min16, unsigned char* __restrict__ out, int vec) {
    __shared__ unsigned char lut_s[768];
    for (int i = threadIdx.x; i < 768; i += 256) lut_s[i] = lut[i];
    __syncthreads();
    const int n = h * w, groups = (n + 3) / 4;
    const int64_t lo = lo16, span = hi16 - lo16;
    for (int g = blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
        const int i = g * 4;
        int y = i / w, x = i - y * w;
        unsigned m4 = 0x01010101u;
        const bool full = vec && i + 4 <= n;
        if (full && mask) m4 = *reinterpret_cast<const unsigned*>(mask + i);
        unsigned px[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            px[k] = 0;
            if (i + k < n) {
                unsigned under = bg;
                if (thumb) {
                    const unsigned char* p = thumb + (int64_t)y * row_stride + (int64_t)x * ps;
                    under = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
                }
                const bool in = full ? ((m4 >> (8 * k)) & 255u) != 0 : (mask ? mask[i + k] != 0 : true);
                px[k] = heat_render_one(acc[i + k], in, under, lut_s, alpha, lo, span, min16);
                if (++x == w) {
                    x = 0;
                    ++y;
                }
            }
        }
        if (full) {                                   // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
            unsigned* o = reinterpret_cast<unsigned*>(out + (int64_t)i * 3);
            o[0] = px[0] | (px[1] << 24);
            o[1] = (px[1] >> 8) | (px[2] << 16);
            o[2] = (px[2] >> 16) | (px[3] << 8);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (i + k < n) {
                    unsigned char* o = out + (int64_t)(i + k) * 3;
                    o[0] = (unsigned char)px[k];
                    o[1] = (unsigned char)(px[k] >> 8);
                    o[2] = (unsigned char)(px[k] >> 16);
                }
            }
        }
    }
}

// ---- Gaussian smoothing under the support ----------------------------------------------------------------
// A normalised convolution in integers.  Per pixel s = covered (and inside the mask), m = s ? (2 S + c) / (2 c) : 0.  The row pass
// writes A = sum taps m (< 2^31, bit 31 carries the pixel's own s) and B = sum taps s (<= 2^15); the column pass sums both over
// the rows into Nn (< 2^46, 64 bits) and D (< 2^30) and writes (1 << 40) | (2 Nn + D) / (2 D) on the support, 0 elsewhere.  Both
// passes stage their input span plus halo in LDS, and a thread makes eight consecutive outputs: a window value is read from LDS
// once per thread and the fifteen taps a chunk of eight window values meets are read once per chunk (the same address in every
// lane).  The taps sit in LDS shifted by 7 with zeros on both sides, so tap (offset - output) needs no bounds test.

constexpr int SMOOTH_PER = 8;                           // outputs per thread, both passes
constexpr int SMOOTH_ROW_THREADS = 128, SMOOTH_ROW_SEG = SMOOTH_ROW_THREADS * SMOOTH_PER;
constexpr int SMOOTH_MAX_CHUNKS = (2 * HEAT_SMOOTH_MAX_RADIUS + 2 * SMOOTH_PER - 1) / SMOOTH_PER;       // 33
constexpr int SMOOTH_TAPS_LDS = SMOOTH_PER * SMOOTH_MAX_CHUNKS + 2 * SMOOTH_PER;                        // 280 >= 8 chunks + 15
constexpr int SMOOTH_COL_LDS_LIMIT = 65536;

__device__ __forceinline__ int smooth_chunks(int radius) { return (2 * radius + 2 * SMOOTH_PER - 1) / SMOOTH_PER; }

// floor(a / b) for a < 2^53, 1 <= b < 2^53: both are exact doubles and the quotient is within one of the rounded division
__device__ __forceinline__ uint64_t heat_floor_quot(uint64_t a, uint64_t b) {
    uint64_t q = (uint64_t)((double)a / (double)b);
    if (q * b > a) --q;
    else if ((q + 1) * b <= a) ++q;
    return q;
}

__device__ __forceinline__ void smooth_stage_taps(const int* __restrict__ taps, int radius, int* tp, int nthreads) {
    for (int i = threadIdx.x; i < SMOOTH_TAPS_LDS; i += nthreads) {
        const int k = i - (SMOOTH_PER - 1);
        tp[i] = (k >= 0 && k <= 2 * radius) ? taps[k] : 0;
    }
}

// one block: SMOOTH_ROW_SEG outputs of one row.  win[i] is pixel (y, x0 - radius + i): m | s << 16
__global__ __launch_bounds__(SMOOTH_ROW_THREADS)
void heat_smooth_row_kernel(const heat_acc_t* __restrict__ acc, int h, int w, const unsigned char* __restrict__ mask,
                            const int* __restrict__ taps, int radius, int nseg, int64_t nblocks, unsigned* __restrict__ rowa,
                            unsigned short* __restrict__ rowb) {
    __shared__ __attribute__((aligned(16))) unsigned win[SMOOTH_ROW_SEG + SMOOTH_PER * SMOOTH_MAX_CHUNKS];
    __shared__ int tp[SMOOTH_TAPS_LDS];
    const int nch = smooth_chunks(radius);
    smooth_stage_taps(taps, radius, tp, SMOOTH_ROW_THREADS);
    for (int64_t bid = blockIdx.x; bid < nblocks; bid += gridDim.x) {
    const int y = (int)(bid / nseg), x0 = (int)(bid - (int64_t)y * nseg) * SMOOTH_ROW_SEG;
    const int64_t row = (int64_t)y * w;
    for (int i = threadIdx.x; i < SMOOTH_ROW_SEG + SMOOTH_PER * nch; i += SMOOTH_ROW_THREADS) {
        const int x = x0 - radius + i;
        unsigned p = 0;
        if (i < SMOOTH_ROW_SEG + 2 * radius && x >= 0 && x < w) {
            const heat_acc_t a = acc[row + x];
            const heat_acc_t S = a & HEAT_SUM_MASK, c = a >> HEAT_COUNT_SHIFT;
            if (c != 0 && (mask == nullptr || mask[row + x] != 0)) p = ((unsigned)heat_floor_quot(2 * S + c, 2 * c) & 0xFFFFu) | 0x10000u;
        }
        win[i] = p;
    }
    __syncthreads();
    const int first = threadIdx.x * SMOOTH_PER;
    if (x0 + first < w) {
    unsigned A[SMOOTH_PER], B[SMOOTH_PER];
#pragma unroll
    for (int j = 0; j < SMOOTH_PER; ++j) A[j] = B[j] = 0;
    for (int c = 0; c < nch; ++c) {
        const uint4 lo = *reinterpret_cast<const uint4*>(&win[first + SMOOTH_PER * c]), hi = *reinterpret_cast<const uint4*>(&win[first + SMOOTH_PER * c + 4]);
        const unsigned v[SMOOTH_PER] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        unsigned T[2 * SMOOTH_PER - 1];
#pragma unroll
        for (int i = 0; i < 2 * SMOOTH_PER - 1; ++i) T[i] = (unsigned)tp[SMOOTH_PER * c + i];
#pragma unroll
        for (int e = 0; e < SMOOTH_PER; ++e) {
            const unsigned m = v[e] & 0xFFFFu, s = v[e] >> 16;
#pragma unroll
            for (int j = 0; j < SMOOTH_PER; ++j) {
                const unsigned t = T[e - j + SMOOTH_PER - 1];          // tap (8 c + e) - j, zero outside 0 .. 2 radius
                A[j] += t * m;
                B[j] += t * s;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < SMOOTH_PER; ++j) {
        const int x = x0 + first + j;
        if (x < w) {
            rowa[row + x] = A[j] | ((win[first + j + radius] >> 16) << 31);
            rowb[row + x] = (unsigned short)B[j];
        }
    }
    }
    __syncthreads();                                  // win is staged again for the block's next segment
    }
}

// one block: cx = 1 << cshift columns by (256 / cx) * 8 rows of outputs.  LDS row i is raster row y0 - radius + i.
__global__ __launch_bounds__(256)
void heat_smooth_col_kernel(const unsigned* __restrict__ rowa, const unsigned short* __restrict__ rowb, int h, int w,
                            const int* __restrict__ taps, int radius, int cshift, int nxb, int64_t nblocks, heat_acc_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smooth_lds[];
    const int cx = 1 << cshift, ry = (256 >> cshift) * SMOOTH_PER, nch = smooth_chunks(radius);
    const int rows = ry - SMOOTH_PER + SMOOTH_PER * nch;             // the last group's window ends here
    int* tp = reinterpret_cast<int*>(smooth_lds);
    unsigned* a_s = reinterpret_cast<unsigned*>(smooth_lds + SMOOTH_TAPS_LDS * sizeof(int));
    unsigned short* b_s = reinterpret_cast<unsigned short*>(a_s + rows * cx);
    smooth_stage_taps(taps, radius, tp, 256);
    for (int64_t bid = blockIdx.x; bid < nblocks; bid += gridDim.x) {
    const int by = (int)(bid / nxb), x0 = (int)(bid - (int64_t)by * nxb) * cx, y0 = by * ry;
    for (int i = threadIdx.x; i < rows * cx; i += 256) {
        const int r = i >> cshift, x = x0 + (i & (cx - 1)), y = y0 - radius + r;
        unsigned a = 0;
        unsigned short b = 0;
        if (r < ry + 2 * radius && y >= 0 && y < h && x < w) {
            const int64_t at = (int64_t)y * w + x;
            a = rowa[at];
            b = rowb[at];
        }
        a_s[i] = a;
        b_s[i] = b;
    }
    __syncthreads();
    const int col = threadIdx.x & (cx - 1), first = (threadIdx.x >> cshift) * SMOOTH_PER;
    const int x = x0 + col;
    if (x < w && y0 + first < h) {
    uint64_t Nn[SMOOTH_PER];
    unsigned D[SMOOTH_PER];
#pragma unroll
    for (int j = 0; j < SMOOTH_PER; ++j) {
        Nn[j] = 0;
        D[j] = 0;
    }
    for (int c = 0; c < nch; ++c) {
        unsigned T[2 * SMOOTH_PER - 1];
#pragma unroll
        for (int i = 0; i < 2 * SMOOTH_PER - 1; ++i) T[i] = (unsigned)tp[SMOOTH_PER * c + i];
#pragma unroll
        for (int e = 0; e < SMOOTH_PER; ++e) {
            const int at = ((first + SMOOTH_PER * c + e) << cshift) + col;
            const unsigned a = a_s[at] & 0x7FFFFFFFu, b = b_s[at];
#pragma unroll
            for (int j = 0; j < SMOOTH_PER; ++j) {
                const unsigned t = T[e - j + SMOOTH_PER - 1];
                Nn[j] += (uint64_t)t * a;
                D[j] += t * b;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < SMOOTH_PER; ++j) {
        const int y = y0 + first + j;
        if (y < h) {
            const bool s = (a_s[((first + j + radius) << cshift) + col] >> 31) != 0 && D[j] != 0;        // D >= centre^2 >= 1 on the support
            out[(int64_t)y * w + x] = s ? ((heat_acc_t)1 << HEAT_COUNT_SHIFT) | heat_floor_quot(2 * Nn[j] + D[j], 2 * (uint64_t)D[j]) : 0;
        }
    }
    }
    __syncthreads();                                  // the planes are staged again for the block's next tile
    }
}

}  // namespace keepk
using namespace keepk;

// the column pass's LDS for cx = 1 << cshift columns: taps + (A uint32 + B uint16) per staged pixel
static size_t smooth_col_lds(int radius, int cshift) {
    const int nch = (2 * radius + 2 * SMOOTH_PER - 1) / SMOOTH_PER, rows = (256 >> cshift) * SMOOTH_PER - SMOOTH_PER + SMOOTH_PER * nch;
    return SMOOTH_TAPS_LDS * sizeof(int) + (size_t)rows * (1 << cshift) * 6;
}

// a block per tile up to 2^22 blocks; beyond that (rasters one pixel wide) the blocks stride over the tiles
static unsigned smooth_grid_for(int64_t blocks) { return (unsigned)(blocks > ((int64_t)1 << 22) ? (int64_t)1 << 22 : blocks); }

void launch_heat_smooth(const int64_t* acc, int h, int w, const unsigned char* mask, const int* taps, int radius, unsigned* rowa,
                        unsigned short* rowb, int64_t* out, hipStream_t s) {
    const int nseg = (w + SMOOTH_ROW_SEG - 1) / SMOOTH_ROW_SEG;
    const int64_t row_blocks = (int64_t)h * nseg;
    hipLaunchKernelGGL(heat_smooth_row_kernel, dim3(smooth_grid_for(row_blocks)), dim3(SMOOTH_ROW_THREADS), 0, s, (const heat_acc_t*)acc, h, w,
                       mask, taps, radius, nseg, row_blocks, rowa, rowb);
    // 64 columns by 32 rows per block while the staged rows fit 64 KiB of LDS (radius <= 64), else 32 columns by 64 rows
    const int cshift = smooth_col_lds(radius, 6) <= SMOOTH_COL_LDS_LIMIT ? 6 : 5;
    const int cx = 1 << cshift, ry = (256 >> cshift) * SMOOTH_PER;
    const int nxb = (w + cx - 1) / cx, nyb = (h + ry - 1) / ry;
    const int64_t col_blocks = (int64_t)nxb * nyb;
    hipLaunchKernelGGL(heat_smooth_col_kernel, dim3(smooth_grid_for(col_blocks)), dim3(256), smooth_col_lds(radius, cshift), s, rowa, rowb, h, w,
                       taps, radius, cshift, nxb, col_blocks, (heat_acc_t*)out);
}

static unsigned heat_grid_for(int64_t items, int per_block) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (unsigned)(b > 65536 ? 65536 : (b < 1 ? 1 : b));
}

static bool heat_aligned(const void* p, size_t a) { return p == nullptr || ((uintptr_t)p & (a - 1)) == 0; }

void launch_heat_accumulate(const int64_t* coords, const float* values, int64_t n, int64_t patch, int64_t d, int h, int w, int64_t ox,
                            int64_t oy, int64_t* acc, hipStream_t s) {
    if (n < 1) return;
    hipLaunchKernelGGL(heat_accumulate_kernel, dim3(heat_grid_for(n, 4)), dim3(256), 0, s, coords, values, n, patch, d, h, w, ox, oy,
                       (heat_acc_t*)acc);
}

void launch_heat_accumulate_cells(const int64_t* coords, const float* values, int64_t n, int gh, int gw, int64_t patch, int64_t d, int h, int w,
                                  int64_t ox, int64_t oy, int64_t* acc, hipStream_t s) {
    if (n < 1) return;
    hipLaunchKernelGGL(heat_accumulate_cells_kernel, dim3(heat_grid_for(n, 4)), dim3(256), 0, s, coords, values, n, gh, gw, (int)(patch / gw),
                       (int)(patch / gh), patch, d, h, w, ox, oy, (heat_acc_t*)acc);
}

void launch_heat_mean(const int64_t* acc, int h, int w, float uncovered, float* mean, int* count, unsigned char* pred, hipStream_t s) {
    const int n = h * w;
    const int vec = heat_aligned(acc, 16) && heat_aligned(mean, 16) && heat_aligned(count, 16) && heat_aligned(pred, 4);
    hipLaunchKernelGGL(heat_mean_kernel, dim3(heat_grid_for(n, 1024)), dim3(256), 0, s, (const heat_acc_t*)acc, n, uncovered, mean, count, pred,
                       vec);
}

void launch_heat_render(const int64_t* acc, int h, int w, const unsigned char* thumb, int64_t row_stride, int ps, unsigned bg,
                        const unsigned char* mask, const unsigned char* lut, int alpha, int lo16, int hi16, int min16, unsigned char* out,
                        hipStream_t s) {
    const int vec = heat_aligned(out, 4) && heat_aligned(mask, 4);
    hipLaunchKernelGGL(heat_render_kernel, dim3(heat_grid_for((int64_t)h * w, 1024)), dim3(256), 0, s, (const heat_acc_t*)acc, h, w, thumb,
                       row_stride, ps, bg, mask, lut, alpha, lo16, hi16, min16, out, vec);
}
