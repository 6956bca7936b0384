// The subtype map: per-tile class probabilities [N,C] rasterised into C planes of the heatmap's accumulator word,
// the per-pixel argmax with its confidence, the confusion of two label maps and the palette render.  Integer arithmetic throughout:
// every result is held exactly to keep_amd.classmap.class_raster_numpy / class_argmax_numpy / confusion_numpy / class_render_numpy.
//
//   class_accumulate  one wave per tile, the footprint and the walk over it are heat_accumulate's (heatmap.hip).  Lanes c < C read the
//                     tile's row once and quantise it once; a NaN anywhere in the row skips the tile in every plane, so the count field
//                     is the same in all planes.  Each (tile, pixel, class) is ONE no-return 64-bit integer atomic add at agent scope
//                     of (1 << 40) | q_c into plane c; the wave walks the footprint plane after plane with the lanes along x, so a
//                     plane sees the row segments the scalar kernel makes.
//   class_argmax      one thread per pixel, plane after plane (consecutive lanes read consecutive words of a plane)
//   class_confusion   a block-local (C + 1)^2 histogram in LDS, then one 64-bit atomic add per non-zero bin
//   class_render      heat_render's frame: four pixels per thread, the palette in LDS, the thumbnail by the caller's strides
//
// Pixel indices are int32 (C h w <= 2^30, checked by the caller); offsets into the accumulator (8 bytes per word) are int64.
#include "common.h"
#include "../../include/keep_hip.h"

namespace keepk {

typedef unsigned long long class_acc_t;
constexpr int CLASS_COUNT_SHIFT = 40;
constexpr class_acc_t CLASS_SUM_MASK = ((class_acc_t)1 << CLASS_COUNT_SHIFT) - 1;

// floor(a / d) for d >= 1, also for a < 0
__device__ __forceinline__ int64_t class_floor_div(int64_t a, int64_t d) {
    const int64_t q = a / d;
    return (a % d != 0 && a < 0) ? q - 1 : q;
}

__global__ __launch_bounds__(256)
void class_accumulate_kernel(const int64_t* __restrict__ coords, const float* __restrict__ values, int64_t n, int C, int64_t P, int64_t d,
                             int h, int w, int64_t ox, int64_t oy, class_acc_t* __restrict__ acc) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const int64_t plane = (int64_t)h * w;
    for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < n; t += nwaves) {        // t is the same in every lane: the whole wave is here
        const float v = lane < C ? values[t * C + lane] : 0.f;
        if (__ballot(v != v)) continue;               // a NaN anywhere in the row: the tile is skipped in all planes
        const int q = __float2int_rn(fminf(fmaxf(v, 0.f), 1.f) * 65535.f);
        // the footprint, once per tile; differences wrap like numpy's int64 and the clip below keeps any result inside the raster
        const int64_t x = (int64_t)((uint64_t)coords[2 * t] - (uint64_t)ox), y = (int64_t)((uint64_t)coords[2 * t + 1] - (uint64_t)oy);
        const int64_t x0 = class_floor_div(x, d), x1 = class_floor_div((int64_t)((uint64_t)x + (uint64_t)P), d);
        const int64_t y0 = class_floor_div(y, d), y1 = class_floor_div((int64_t)((uint64_t)y + (uint64_t)P), d);
        const int64_t c0 = x0 > 0 ? x0 : 0, c1 = x1 < w ? x1 : w, r0 = y0 > 0 ? y0 : 0, r1 = y1 < h ? y1 : h;
        if (c1 <= c0 || r1 <= r0) continue;           // off the raster, or empty
        const int fw = (int)(c1 - c0), fh = (int)(r1 - r0);
        const int64_t npx = (int64_t)fw * fh;
        const int dr = 64 / fw, dc = 64 - dr * fw;    // what 64 pixels further along the footprint means in (row, column)
        const int r_first = lane / fw, c_first = lane - r_first * fw;
        class_acc_t* base = acc + (r0 * (int64_t)w + c0);
        for (int k = 0; k < C; ++k) {                 // plane after plane, each the scalar kernel's walk; the whole wave reads lane k's q
            const class_acc_t add = ((class_acc_t)1 << CLASS_COUNT_SHIFT) | (class_acc_t)(unsigned)__builtin_amdgcn_readlane(q, k);
            class_acc_t* pk = base + k * plane;
            int r = r_first, c = c_first;
            for (int64_t i = lane; i < npx; i += 64) {    // i < npx <=> r < fh, and c < fw always: inside the clipped footprint
                (void)__hip_atomic_fetch_add(pk + ((int64_t)r * w + c), add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                c += dc;
                r += dr;
                if (c >= fw) {
                    c -= fw;
                    ++r;
                }
            }
        }
    }
}

// label = the smallest c with the largest sum; second = the largest sum of the other classes (0 without one).  min16 / margin16: the
// thresholds on S_top / n and (S_top - S_second) / n in 16-bit fixed point, applied as products (no division)
__global__ __launch_bounds__(256)
void class_argmax_kernel(const class_acc_t* __restrict__ acc, int C, int npix, const unsigned char* __restrict__ mask, int64_t min16,
                         int64_t margin16, unsigned char* __restrict__ label, class_acc_t* __restrict__ top, class_acc_t* __restrict__ margin) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) {
        const class_acc_t a0 = acc[i];
        const int64_t n = (int64_t)(a0 >> CLASS_COUNT_SHIFT);
        unsigned char lab = 255;
        class_acc_t t = 0, m = 0;
        if (n != 0 && (mask == nullptr || mask[i] != 0)) {
            int64_t s_top = (int64_t)(a0 & CLASS_SUM_MASK), s_second = 0;
            int best = 0;
            for (int c = 1; c < C; ++c) {
                const int64_t s = (int64_t)(acc[(int64_t)c * npix + i] & CLASS_SUM_MASK);
                if (s > s_top) {
                    s_second = s_top;
                    s_top = s;
                    best = c;
                } else if (s > s_second) {
                    s_second = s;
                }
            }
            const int64_t gap = s_top - s_second;
            lab = (s_top < min16 * n || gap < margin16 * n) ? 254 : (unsigned char)best;
            t = ((class_acc_t)n << CLASS_COUNT_SHIFT) | (class_acc_t)s_top;
            m = ((class_acc_t)n << CLASS_COUNT_SHIFT) | (class_acc_t)gap;
        }
        if (label) label[i] = lab;
        if (top) top[i] = t;
        if (margin) margin[i] = m;
    }
}

// hist: (C + 1)^2 int32 counters in LDS (a block sees < 2^31 pixels); vec: a, b and within are 4-byte aligned
__global__ __launch_bounds__(256)
void class_confusion_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, const unsigned char* __restrict__ within,
                            int npix, int C, int vec, class_acc_t* __restrict__ out) {
    extern __shared__ unsigned conf_hist[];
    const int side = C + 1, bins = side * side;
    for (int i = threadIdx.x; i < bins; i += 256) conf_hist[i] = 0;
    __syncthreads();
    const int groups = (npix + 3) / 4;
    for (int g = blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
        const int i = g * 4;
        if (vec && i + 4 <= npix) {
            const unsigned a4 = *reinterpret_cast<const unsigned*>(a + i), b4 = *reinterpret_cast<const unsigned*>(b + i);
            const unsigned w4 = within ? *reinterpret_cast<const unsigned*>(within + i) : 0x01010101u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if ((w4 >> (8 * k)) & 255u) {
                    const int la = min((int)((a4 >> (8 * k)) & 255u), C), lb = min((int)((b4 >> (8 * k)) & 255u), C);
                    atomicAdd(&conf_hist[la * side + lb], 1u);
                }
            }
        } else {
            for (int k = i; k < npix && k < i + 4; ++k) {
                if (within == nullptr || within[k] != 0) {
                    const int la = min((int)a[k], C), lb = min((int)b[k], C);
                    atomicAdd(&conf_hist[la * side + lb], 1u);
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += 256) {
        const unsigned v = conf_hist[i];
        if (v) (void)__hip_atomic_fetch_add(out + i, (class_acc_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// one pixel: (R | G << 8 | B << 16) of the output.  strength: the accumulator word that scales alpha (heat_render_one's index rule), or
// no word at all (has_strength = false)
__device__ __forceinline__ unsigned class_render_one(int lab, int C, unsigned under, const unsigned char* pal, int alpha, bool has_strength,
                                                     class_acc_t sw, int64_t lo, int64_t span) {
    if (lab >= C) return under;
    int a_eff = alpha;
    if (has_strength) {
        const int64_t S = (int64_t)(sw & CLASS_SUM_MASK), c = (int64_t)(sw >> CLASS_COUNT_SHIFT);
        // the windowed mean scaled to 0..255, rounded half up: S < 2^40, c < 2^24, span < 2^16, so everything stays below 2^50
        const int64_t rel = S - lo * c;
        int idx = 0;
        if (c > 0 && rel > 0) {
            const uint64_t qd = (uint64_t)(2 * 255 * rel + span * c) / (uint64_t)(2 * span * c);
            idx = qd > 255 ? 255 : (int)qd;
        }
        a_eff = (alpha * idx + 127) / 255;
    }
    unsigned out = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const unsigned u = (under >> (8 * ch)) & 255u;
        out |= (((unsigned)a_eff * pal[lab * 3 + ch] + (unsigned)(256 - a_eff) * u + 128u) >> 8) << (8 * ch);
    }
    return out;
}

// four pixels per thread -> 12 output bytes; vec: out and label are 4-byte aligned.  The thumbnail is read by bytes: its row and pixel
// strides are the caller's.
__global__ __launch_bounds__(256)
void class_render_kernel(const unsigned char* __restrict__ label, int h, int w, int C, const unsigned char* __restrict__ thumb, int64_t row_stride,
                         int ps, unsigned bg, const unsigned char* __restrict__ palette, int alpha, const class_acc_t* __restrict__ strength,
                         int lo16, int hi16, unsigned char* __restrict__ out, int vec) {
    __shared__ unsigned char pal_s[CLASS_MAX * 3];
    for (int i = threadIdx.x; i < C * 3; i += 256) pal_s[i] = palette[i];
    __syncthreads();
    const int n = h * w, groups = (n + 3) / 4;
    const int64_t lo = lo16, span = hi16 - lo16;
    for (int g = blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
        const int i = g * 4;
        int y = i / w, x = i - y * w;
        const bool full = vec && i + 4 <= n;
        unsigned l4 = 0;
        if (full) l4 = *reinterpret_cast<const unsigned*>(label + i);
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
                const int lab = full ? (int)((l4 >> (8 * k)) & 255u) : (int)label[i + k];
                px[k] = class_render_one(lab, C, under, pal_s, alpha, strength != nullptr, strength ? strength[i + k] : 0, lo, span);
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

}  // namespace keepk
using namespace keepk;

static unsigned class_grid_for(int64_t items, int per_block, int64_t most = 65536) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (unsigned)(b > most ? most : (b < 1 ? 1 : b));
}

static bool class_aligned(const void* p, size_t a) { return p == nullptr || ((uintptr_t)p & (a - 1)) == 0; }

void launch_class_accumulate(const int64_t* coords, const float* values, int64_t n, int C, int64_t patch, int64_t d, int h, int w, int64_t ox,
                             int64_t oy, int64_t* acc, hipStream_t s) {
    if (n < 1) return;
    hipLaunchKernelGGL(class_accumulate_kernel, dim3(class_grid_for(n, 4)), dim3(256), 0, s, coords, values, n, C, patch, d, h, w, ox, oy,
                       (class_acc_t*)acc);
}

void launch_class_argmax(const int64_t* acc, int C, int h, int w, const unsigned char* mask, int min16, int margin16, unsigned char* label,
                         int64_t* top, int64_t* margin, hipStream_t s) {
    const int npix = h * w;
    hipLaunchKernelGGL(class_argmax_kernel, dim3(class_grid_for(npix, 256)), dim3(256), 0, s, (const class_acc_t*)acc, C, npix, mask,
                       (int64_t)min16, (int64_t)margin16, label, (class_acc_t*)top, (class_acc_t*)margin);
}

void launch_class_confusion(const unsigned char* a, const unsigned char* b, const unsigned char* within, int h, int w, int C, int64_t* out,
                            hipStream_t s) {
    const int npix = h * w, bins = (C + 1) * (C + 1);
    (void)hipMemsetAsync(out, 0, (size_t)bins * 8, s);
    const int vec = class_aligned(a, 4) && class_aligned(b, 4) && class_aligned(within, 4);
    // 16 pixels per thread and more: the flush of a block's histogram is then small beside its share of the pixels
    hipLaunchKernelGGL(class_confusion_kernel, dim3(class_grid_for(npix, 4096, 2048)), dim3(256), (size_t)bins * sizeof(unsigned), s, a, b, within,
                       npix, C, vec, (class_acc_t*)out);
}

void launch_class_render(const unsigned char* label, int h, int w, int C, const unsigned char* thumb, int64_t row_stride, int ps, unsigned bg,
                         const unsigned char* palette, int alpha, const int64_t* strength, int lo16, int hi16, unsigned char* out, hipStream_t s) {
    const int vec = class_aligned(out, 4) && class_aligned(label, 4);
    hipLaunchKernelGGL(class_render_kernel, dim3(class_grid_for((int64_t)h * w, 1024)), dim3(256), 0, s, label, h, w, C, thumb, row_stride, ps, bg,
                       palette, alpha, (const class_acc_t*)strength, lo16, hi16, out, vec);
}
