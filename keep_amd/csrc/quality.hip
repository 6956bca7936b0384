// Tile quality control: every pixel of a tile gets exactly one class (pen ink 0..3, dark, glass, tissue, other)
// and the tile's focus is the variance of an integer Laplacian of its grey levels.  Integer arithmetic throughout: every word is held
// exactly to keep_amd.quality's numpy restatements and does not depend on the band split, the launch geometry or the order.
//
//   region_quality   one workgroup per (cell, band of rows).  Pass 1 reads the band's rows and one halo row above and below (only rows
//                    of the tile itself) in groups of 4 pixels, three dwords where the group is dword aligned (four such loads in
//                    flight per thread) and bytes at a row's two ends; classifies the band's own pixels (the pen boxes are three 256-entry tables of 32-bit box masks in LDS: a
//                    pixel's boxes are lutR[r] & lutG[g] & lutB[b], whatever their number); keeps the grey bytes of every row in LDS,
//                    each row shifted so that its groups are dwords there too, and one nibble of tissue bits per group.  Pass 2 takes
//                    the Laplacian of the interior pixels from LDS, 4 pixels per thread and step: three dwords of its own row, two
//                    dwords and a byte alignment for the row above and the row below.  Partials: int32 per thread, widened to int64
//                    before the wave shuffles, LDS across the four waves, one returnless 64-bit atomic per workgroup and column.
//   pen_mask         the same classifier, one byte per thumbnail pixel, 4 pixels per thread and step.
#include "common.h"
#include "../../include/keep_hip.h"

#include <algorithm>

namespace keepk {

struct QualRules { int sat_min, white_min, dark_max, n_boxes, first1, first2, first3; };

__device__ __forceinline__ QualRules qual_rules(const int* __restrict__ blob) {
    QualRules q;
    q.sat_min = blob[0]; q.white_min = blob[1]; q.dark_max = blob[2]; q.n_boxes = blob[3];
    q.first1 = blob[4]; q.first2 = blob[5]; q.first3 = blob[6];
    return q;
}

__device__ __forceinline__ void qual_stage_lut(const int* __restrict__ blob, unsigned* lut, int tid) {
    for (int i = tid; i < 3 * 256; i += 256) lut[i] = (unsigned)blob[QUAL_BLOB_HEAD + i];
}

// 0..3 pen ink of that class, 4 dark, 5 glass, 6 tissue, 7 other: the later rule overrides the earlier, so the priority is pen, dark,
// glass, tissue.  The boxes are sorted by class, so the lowest set bit is a box of the lowest class that contains the pixel.
__device__ __forceinline__ int qual_class(int r, int g, int b, const QualRules& q, const unsigned* lut) {
    const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
    int cls = 7;
    if (mx > 0 && 255 * (mx - mn) >= __mul24(q.sat_min, mx)) cls = 6;   // sat_min is a byte: a 24-bit product
    if (mn >= q.white_min) cls = 5;
    if (mx <= q.dark_max) cls = 4;
    if (q.n_boxes) {
        const unsigned in = lut[r] & lut[256 + g] & lut[512 + b];
        if (in) {
            const int i = __ffs(in) - 1;
            cls = (i >= q.first1) + (i >= q.first2) + (i >= q.first3);
        }
    }
    return cls;
}

__device__ __forceinline__ unsigned qual_grey(int r, int g, int b) { return (unsigned)(77 * r + 150 * g + 29 * b + 128) >> 8; }

struct __attribute__((aligned(4))) QualU3 { unsigned a, b, c; };
struct __attribute__((aligned(4))) QualU4 { unsigned a, b, c, d; };
template <int PS> struct QualRaw;
template <> struct QualRaw<3> { typedef QualU3 T; };
template <> struct QualRaw<4> { typedef QualU4 T; };

struct QualArgs {
    const unsigned char* region;
    int64_t row;                                      // bytes between rows
    const int32_t* cells;
    int patch;
    int bands, R;                                     // bands per cell, rows per band
    int G, LP;                                        // 4-pixel groups per row, bytes of a row in LDS = 4 G + 8
    int GW;                                           // groups 1 .. GW of every row lie wholly inside the tile, whatever the row's alignment
    unsigned mG, mGW;                                 // ceil(2^32 / G), ceil(2^32 / GW) for qual_div
};

// i / d for 0 <= i < 2^16 and 1 <= d < 2^16 with m = ceil(2^32 / d): the error of i m / 2^32 is below i d / 2^32 / d < 1 / d
__device__ __forceinline__ int qual_div(int i, int d, unsigned m) { return d == 1 ? i : (int)__umulhi((unsigned)i, m); }

// The first pixel of a row that starts a dword: RGB pixels are 3 bytes, so pixel x of a row at address a starts a dword iff x = a mod 4;
// an RGBA row is all dwords or none.  Group g of a row holds the pixels x0 - 4 + 4 g + (0..3): group 0 the < 4 pixels before x0.
template <int PS>
__device__ __forceinline__ int qual_x0(uintptr_t a) { return PS == 3 ? (int)(a & 3) : 0; }

__device__ __forceinline__ void qual_unpack(const QualU3& v, int* r, int* g, int* b) {   // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
    r[0] = v.a & 255; g[0] = (v.a >> 8) & 255; b[0] = (v.a >> 16) & 255;
    r[1] = v.a >> 24; g[1] = v.b & 255; b[1] = (v.b >> 8) & 255;
    r[2] = (v.b >> 16) & 255; g[2] = v.b >> 24; b[2] = v.c & 255;
    r[3] = (v.c >> 8) & 255; g[3] = (v.c >> 16) & 255; b[3] = v.c >> 24;
}
__device__ __forceinline__ void qual_unpack(const QualU4& v, int* r, int* g, int* b) {
    const unsigned w[4] = {v.a, v.b, v.c, v.d};
#pragma unroll
    for (int j = 0; j < 4; ++j) { r[j] = w[j] & 255; g[j] = (w[j] >> 8) & 255; b[j] = (w[j] >> 16) & 255; }
}

// the 4 pixels at p, all inside the tile: one load of 12 (RGB: p is a dword by the choice of x0) or 16 bytes; RGBA off a dword: bytes
template <int PS>
__device__ __forceinline__ typename QualRaw<PS>::T qual_load4(const unsigned char* p) {
    if constexpr (PS == 4) {
        if ((uintptr_t)p & 3) {
            QualU4 v;
            v.a = p[0] | (p[1] << 8) | (p[2] << 16); v.b = p[4] | (p[5] << 8) | (p[6] << 16);
            v.c = p[8] | (p[9] << 8) | (p[10] << 16); v.d = p[12] | (p[13] << 8) | (p[14] << 16);
            return v;
        }
    }
    return *(const typename QualRaw<PS>::T*)p;
}

struct QualBand {                                     // what a group needs to know of its workgroup
    int P, G, LP, y0, y1;
    unsigned* grey_w;
    unsigned char* tis;
    const unsigned* lut;
};

// One group of a staged row, r g b of its 4 pixels (anything where the pixel lies outside the tile): the grey bytes go to LDS; in a row
// of the band itself the pixels' classes are counted (pen: 8-bit counters of the classes 0..3, rest: of dark, glass, tissue, other) and
// the group's tissue nibble is kept.
template <bool WHOLE>                                 // WHOLE: all 4 pixels lie inside the tile
__device__ __forceinline__ void qual_group(const QualBand& k, const QualRules& q, const int* r, const int* g, const int* b, int x, int y, int grp,
                                           unsigned& pen, unsigned& rest) {
    unsigned gw = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) gw |= qual_grey(r[j], g[j], b[j]) << (8 * j);
    k.grey_w[((y - k.y0 + 1) * k.LP + 4 + 4 * grp) >> 2] = gw;
    if (y >= k.y0 && y < k.y1) {
        unsigned nib = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xx = x + j;
            if (WHOLE || (xx >= 0 && xx < k.P)) {
                const int cls = qual_class(r[j], g[j], b[j], q, k.lut);
                const unsigned one = 1u << (8 * (cls & 3));
                pen += cls < 4 ? one : 0u;
                rest += cls < 4 ? 0u : one;
                nib |= (unsigned)(cls == 6) << j;
            }
        }
        k.tis[(y - k.y0) * k.G + grp] = (unsigned char)nib;
    }
}

template <typename T>
__device__ __forceinline__ T qual_wave_sum(T x) {
#pragma unroll
    for (int o = 32; o; o >>= 1) x += __shfl_down(x, o);
    return x;
}

typedef short qual_s2 __attribute__((ext_vector_type(2)));
// bytes of w chosen by sel (v_perm_b32 with both sources w: selector 0..3 = that byte, 0x0c = zero) as two 16-bit lanes
__device__ __forceinline__ qual_s2 qual_pair(unsigned w, unsigned sel) { return __builtin_bit_cast(qual_s2, __builtin_amdgcn_perm(w, w, sel)); }
// bits 0 and 1 -> all ones in the low and the high 16-bit lane
__device__ __forceinline__ unsigned qual_pair_mask(unsigned bits) {
    const int m0 = (int)(bits << 31) >> 31, m1 = (int)(bits << 30) >> 31;
    return ((unsigned)m0 & 0xffffu) | ((unsigned)m1 << 16);
}

constexpr int QUAL_UNROLL = 4;

template <int PS>
__global__ __launch_bounds__(256, 6)                  // 27 264 bytes of LDS whatever the patch: 6 workgroups share a CU's 160 KiB
void region_quality_kernel(QualArgs a, const int* __restrict__ blob, unsigned long long* __restrict__ out) {
    typedef typename QualRaw<PS>::T Raw;
    __shared__ unsigned lut[3 * 256];
    __shared__ unsigned grey_w[QUAL_GREY_BYTES / 4];  // (R + 2) rows of LP bytes: [4 pad][4 G grey bytes][4 pad]
    __shared__ unsigned char tis[QUAL_TIS_BYTES];     // R rows of G nibbles: bit j = pixel j of the group is tissue
    __shared__ long long part[4][QUAL_COLS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cell = blockIdx.x / a.bands, band = blockIdx.x - cell * a.bands;
    const QualRules q = qual_rules(blob);
    if (q.n_boxes) qual_stage_lut(blob, lut, tid);
    QualBand k;
    k.P = a.patch; k.G = a.G; k.LP = a.LP; k.y0 = band * a.R; k.y1 = min(k.y0 + a.R, k.P);      // y0 .. y1: the band's own rows
    k.grey_w = grey_w; k.tis = tis; k.lut = lut;
    const int P = k.P, G = k.G, LP = k.LP, y0 = k.y0, y1 = k.y1;
    const unsigned char* base = a.region + (int64_t)a.cells[2 * (int64_t)cell + 1] * a.row + (int64_t)a.cells[2 * (int64_t)cell] * PS;
    __syncthreads();

    // ---- pass 1: rows y0 - 1 .. y1 of the tile (clipped to it) -> classes counted, grey bytes and tissue nibbles in LDS
    unsigned pen = 0, rest = 0;                       // 8-bit counters: a thread sees < 128 pixels (QUAL_BAND_PIXELS)
    {
        const int ylo = max(y0 - 1, 0), rows = min(y1 + 1, P) - ylo;
        // the whole groups, QUAL_UNROLL a step apart per thread and turn, all loaded before the first is worked on: a wave keeps that
        // many 768-byte loads in flight.  A group past the end is loaded from the turn's first address instead (no branch around a
        // load) and not used.
        const int GW = a.GW, items = rows * GW;
        for (int i0 = tid; i0 < items; i0 += QUAL_UNROLL * 256) {
            Raw raw[QUAL_UNROLL];
            int where[QUAL_UNROLL];                   // y << 12 | group << 2 | x0
#pragma unroll
            for (int u = 0; u < QUAL_UNROLL; ++u) {
                const int i = i0 + u * 256 < items ? i0 + u * 256 : i0;
                const int lr = qual_div(i, GW, a.mGW), g = 1 + i - lr * GW, y = ylo + lr;
                const unsigned char* p = base + (int64_t)y * a.row;
                const int x0 = qual_x0<PS>((uintptr_t)p);
                raw[u] = qual_load4<PS>(p + (int64_t)(x0 - 4 + 4 * g) * PS);
                where[u] = (y << 12) | (g << 2) | x0;
            }
            __builtin_amdgcn_sched_barrier(0);        // every load is issued before the first use
#pragma unroll
            for (int u = 0; u < QUAL_UNROLL; ++u) {
                if (i0 + u * 256 >= items) break;
                const int y = where[u] >> 12, g = (where[u] >> 2) & 1023, x0 = where[u] & 3;
                int r[4], gg[4], b[4];
                qual_unpack(raw[u], r, gg, b);
                qual_group<true>(k, q, r, gg, b, x0 - 4 + 4 * g, y, g, pen, rest);
            }
        }
        // a row's two ends, group 0 and the groups past GW: bytes, pixel by pixel
        const int E = G - GW;
        for (int i = tid; i < rows * E; i += 256) {
            const int lr = i / E, e = i - lr * E, g = e ? GW + e : 0, y = ylo + lr;
            const unsigned char* p = base + (int64_t)y * a.row;
            const int x = qual_x0<PS>((uintptr_t)p) - 4 + 4 * g;
            int r[4], gg[4], b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int xx = x + j;
                if (xx >= 0 && xx < P) {
                    const unsigned char* t = p + (int64_t)xx * PS;
                    r[j] = t[0]; gg[j] = t[1]; b[j] = t[2];
                } else {
                    r[j] = gg[j] = b[j] = 0;
                }
            }
            qual_group<false>(k, q, r, gg, b, x, y, g, pen, rest);
        }
    }
    __syncthreads();

    // ---- pass 2: the Laplacian on the interior pixels of the band's rows
    int sl = 0, sl2 = 0, nt = 0, slt = 0, sl2t = 0;   // |L| <= 1020, L^2 <= 1 040 400, < 128 pixels per thread: far inside an int32
    {
        const int ylo = max(y0, 1), yhi = min(y1, P - 1);
        const int items = max(yhi - ylo, 0) * G;
        const uintptr_t ba = (uintptr_t)base;
        for (int i = tid; i < items; i += 256) {
            const int lr = qual_div(i, G, a.mG), g = i - lr * G, y = ylo + lr;
            const int x0 = qual_x0<PS>(ba + (uintptr_t)((int64_t)y * a.row));
            const int du = x0 - qual_x0<PS>(ba + (uintptr_t)((int64_t)(y - 1) * a.row));
            const int dd = x0 - qual_x0<PS>(ba + (uintptr_t)((int64_t)(y + 1) * a.row));
            const int x = x0 - 4 + 4 * g;
            const int c = ((y - y0 + 1) * LP + 4 + 4 * g) >> 2;              // this group's dword
            const unsigned mid = grey_w[c], left = grey_w[c - 1], right = grey_w[c + 1];
            // pixel x of the row above sits du bytes after this group's place in that row: two dwords and a byte alignment
            const int eu = du & 3, cu = c - (LP >> 2) + ((du - eu) >> 2);
            const int ed = dd & 3, cd = c + (LP >> 2) + ((dd - ed) >> 2);
            const unsigned up = __builtin_amdgcn_alignbyte(grey_w[cu + 1], grey_w[cu], (unsigned)eu);
            const unsigned dn = __builtin_amdgcn_alignbyte(grey_w[cd + 1], grey_w[cd], (unsigned)ed);
            const unsigned lrow = __builtin_amdgcn_alignbyte(mid, left, 3), rrow = __builtin_amdgcn_alignbyte(right, mid, 1);   // byte j: the pixel left / right of pixel j
            // bit j: pixel j is an interior pixel (1 <= x + j <= P - 2); and of those, the tissue ones
            const int lo = max(1 - x, 0), hi = min(P - 2 - x, 3);
            const unsigned vb = hi >= lo ? ((2u << hi) - 1u) & ~((1u << lo) - 1u) : 0u, tb = tis[(y - y0) * G + g] & vb;
            nt += __popc(tb);
            // two pixels per register as 16-bit lanes: |L| <= 1020 fits, and a dot product of the pair with itself adds both squares
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const unsigned sel = h ? 0x0c030c02u : 0x0c010c00u;                   // bytes 2 h and 2 h + 1, each widened to 16 bits
                const qual_s2 L = qual_pair(mid, sel) * (short)4 - qual_pair(lrow, sel) - qual_pair(rrow, sel) - qual_pair(up, sel) - qual_pair(dn, sel);
                const qual_s2 Lv = __builtin_bit_cast(qual_s2, __builtin_bit_cast(unsigned, L) & qual_pair_mask(vb >> (2 * h)));
                const qual_s2 Lt = __builtin_bit_cast(qual_s2, __builtin_bit_cast(unsigned, L) & qual_pair_mask(tb >> (2 * h)));
                const qual_s2 ones = {1, 1};
                sl = __builtin_amdgcn_sdot2(Lv, ones, sl, false);
                sl2 = __builtin_amdgcn_sdot2(Lv, Lv, sl2, false);
                slt = __builtin_amdgcn_sdot2(Lt, ones, slt, false);
                sl2t = __builtin_amdgcn_sdot2(Lt, Lt, sl2t, false);
            }
        }
    }

    // a wave's sums: the counters as pairs of 16-bit fields (64 lanes x 128 pixels), S L in an int32, the sums of squares in an int64
    const int w0 = (int)((pen & 255) | ((pen >> 8) & 255) << 16), w1 = (int)(((pen >> 16) & 255) | (pen >> 24) << 16);
    const int w2 = (int)((rest & 255) | ((rest >> 8) & 255) << 16), w3 = (int)(((rest >> 16) & 255) | (unsigned)nt << 16);
    const int s0 = qual_wave_sum<int>(w0), s1 = qual_wave_sum<int>(w1), s2 = qual_wave_sum<int>(w2), s3 = qual_wave_sum<int>(w3);
    const int ssl = qual_wave_sum<int>(sl), sslt = qual_wave_sum<int>(slt);
    const long long ssl2 = qual_wave_sum<long long>(sl2), ssl2t = qual_wave_sum<long long>(sl2t);
    if (lane == 0) {
        long long* o = part[wave];
        o[0] = s0 & 0xffff; o[1] = (unsigned)s0 >> 16; o[2] = s1 & 0xffff; o[3] = (unsigned)s1 >> 16;
        o[4] = s2 & 0xffff; o[5] = (unsigned)s2 >> 16; o[6] = s3 & 0xffff; o[9] = (unsigned)s3 >> 16;
        o[7] = ssl; o[8] = ssl2; o[10] = sslt; o[11] = ssl2t;
    }
    __syncthreads();
    if (tid < QUAL_COLS) {
        const long long s = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
        if (s) atomicAdd(out + (int64_t)cell * QUAL_COLS + tid, (unsigned long long)s);   // two's complement: a negative sum adds correctly
    }
}

__global__ __launch_bounds__(256)
void pen_mask_kernel(const unsigned char* __restrict__ img, int64_t row, int ps, int h, int w, const int* __restrict__ blob,
                     unsigned char* __restrict__ out) {
    __shared__ unsigned lut[3 * 256];
    const QualRules q = qual_rules(blob);
    if (q.n_boxes) qual_stage_lut(blob, lut, threadIdx.x);
    __syncthreads();
    const int gw = (w + 3) / 4;
    const int64_t items = (int64_t)h * gw;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (int64_t)gridDim.x * 256) {
        const int y = (int)(i / gw), x = 4 * (int)(i - (int64_t)y * gw);
        const unsigned char* p = img + (int64_t)y * row + (int64_t)x * ps;
        unsigned char* o = out + (int64_t)y * w + x;
        unsigned word = 0;
        const int n = min(4, w - x);
        for (int j = 0; j < n; ++j) {
            const int cls = qual_class(p[j * ps], p[j * ps + 1], p[j * ps + 2], q, lut);
            word |= (unsigned)(cls == 7 ? 0 : cls + 1) << (8 * j);
        }
        if (n == 4 && (((uintptr_t)o) & 3) == 0) {
            *(unsigned*)o = word;
        } else {
            for (int j = 0; j < n; ++j) o[j] = (unsigned char)(word >> (8 * j));
        }
    }
}

}  // namespace keepk
using namespace keepk;

// the band split of a patch: as many rows as keep a band at or below QUAL_BAND_PIXELS pixels, spread evenly
static void qual_bands(int patch, int* bands, int* R) {
    const int rmax = std::max(1, std::min(patch, QUAL_BAND_PIXELS / patch));
    *bands = (patch + rmax - 1) / rmax;
    *R = (patch + *bands - 1) / *bands;
}

int launch_region_quality(const unsigned char* region, int64_t row_stride, int ps, const int32_t* cells, int64_t n, int patch, const int* blob,
                          int64_t* out, hipStream_t s) {
    QualArgs a;
    a.region = region; a.row = row_stride; a.cells = cells; a.patch = patch;
    qual_bands(patch, &a.bands, &a.R);
    a.G = (patch + 3) / 4 + 1;
    a.LP = 4 * a.G + 8;
    a.GW = std::max(patch - 3, 0) / 4;                // x0 <= 3: group g ends at pixel x0 + 4 g <= 3 + 4 GW <= patch
    a.mG = (unsigned)((((uint64_t)1 << 32) + a.G - 1) / a.G);
    a.mGW = a.GW > 1 ? (unsigned)((((uint64_t)1 << 32) + a.GW - 1) / a.GW) : 0;
    // the LDS plan, and qual_div's range: a pass has (R + 2) G < 2^16 groups
    if ((int64_t)(a.R + 2) * a.LP > QUAL_GREY_BYTES || (int64_t)a.R * a.G > QUAL_TIS_BYTES || n * a.bands > INT32_MAX) return -1;
    const dim3 g((unsigned)(n * a.bands)), b(256);
    if (ps == 3) hipLaunchKernelGGL(region_quality_kernel<3>, g, b, 0, s, a, blob, (unsigned long long*)out);
    else hipLaunchKernelGGL(region_quality_kernel<4>, g, b, 0, s, a, blob, (unsigned long long*)out);
    return 0;
}

void launch_pen_mask(const unsigned char* img, int64_t row_stride, int ps, int h, int w, const int* blob, unsigned char* out, hipStream_t s) {
    const int64_t items = (int64_t)h * ((w + 3) / 4);
    const int64_t blocks = std::min<int64_t>(std::max<int64_t>((items + 255) / 256, 1), 16 * (int64_t)keep_num_cus());
    hipLaunchKernelGGL(pen_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, s, img, row_stride, ps, h, w, blob, out);
}
