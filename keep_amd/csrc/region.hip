// Slide-region front end: a uint8 RGB / RGBA region already on the device -> the patch grid, an exact
// integer tissue rule per grid cell, a stable compaction of the kept cells, and the gather of kept patches into the
// [B,224,224,3] uint8 tiles keep_encode_image(..., KEEP_PIX_U8_HWC, ...) takes.
//
//   region_tissue_count   one workgroup per grid cell (grid-stride over cells): tissue-pixel count of the p x p window
//                         (max(r,g,b) > 0 and 255 (max - min) >= sat_min max) -> keep flag (count >= min_pixels)
//   region_block_count /  stable compaction without atomics: per-block kept counts, one-block exclusive scan of those
//   region_scan /         (which also writes the device count), per-block scan + scatter of the kept cells' (x, y) in
//   region_scatter        row-major grid order
//   region_check_cells    keep_region_patches_u8's argument check: any cell outside the region sets a flag
//   region_copy224        p == 224: the kept patches, alpha dropped, into contiguous tiles
//   region_resize_h_u8    p != 224: Pillow's horizontal bicubic pass read straight from the region at each cell's origin;
//                         the vertical pass is rowops.hip's resize_v_u8_kernel, unchanged
//
// Byte offsets into the region are 64-bit throughout (a 30 000 x 30 000 RGB region is 2.7 GB); origins are byte-unaligned,
// so the region is read with byte loads.
#include "common.h"

namespace keepk {

constexpr int REGION_CELLS_PER_BLOCK = REGION_GRID_CHUNK;
constexpr int REGION_CELLS_PER_THREAD = REGION_CELLS_PER_BLOCK / 256;

__device__ __forceinline__ bool region_is_tissue(unsigned r, unsigned g, unsigned b, unsigned sat_min) {
    const unsigned mx = max(r, max(g, b)), mn = min(r, min(g, b));
    return mx > 0 && 255u * (mx - mn) >= sat_min * mx;
}

// 4 waves per cell: wave w takes rows w, w + 4, ...; its lanes consecutive pixels of a row
__global__ __launch_bounds__(256)
void region_tissue_count_kernel(const unsigned char* __restrict__ region, int64_t row_stride, int ps, int gx, int64_t ncells,
                                int patch, int step, unsigned sat_min, int min_pixels, unsigned char* __restrict__ keep) {
    __shared__ int part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t c = blockIdx.x; c < ncells; c += gridDim.x) {
        const int64_t x0 = (c % gx) * step, y0 = (c / gx) * step;
        int n = 0;
        for (int y = wave; y < patch; y += 4) {
            const unsigned char* row = region + (y0 + y) * row_stride + x0 * ps;
            for (int x = lane; x < patch; x += 64) {
                const unsigned char* p = row + (int64_t)x * ps;
                n += region_is_tissue(p[0], p[1], p[2], sat_min);
            }
        }
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
        if (lane == 0) part[wave] = n;
        __syncthreads();
        if (threadIdx.x == 0) keep[c] = (part[0] + part[1] + part[2] + part[3]) >= min_pixels;
        __syncthreads();
    }
}

// kept cells among thread t's REGION_CELLS_PER_THREAD consecutive cells of block b (keep == null: every cell is kept)
__device__ __forceinline__ int region_thread_kept(const unsigned char* keep, int64_t ncells, int64_t c0) {
    int n = 0;
    for (int j = 0; j < REGION_CELLS_PER_THREAD; ++j) {
        const int64_t c = c0 + j;
        n += c < ncells && (!keep || keep[c]);
    }
    return n;
}

__global__ __launch_bounds__(256)
void region_block_count_kernel(const unsigned char* __restrict__ keep, int64_t ncells, int* __restrict__ counts) {
    __shared__ int s[256];
    const int64_t c0 = (int64_t)blockIdx.x * REGION_CELLS_PER_BLOCK + (int64_t)threadIdx.x * REGION_CELLS_PER_THREAD;
    int total;
    block_exclusive_scan256(region_thread_kept(keep, ncells, c0), s, &total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// one block: offsets[b] = sum of counts[0, b); *n_out = sum of all counts
__global__ __launch_bounds__(256)
void region_scan_kernel(const int* __restrict__ counts, int nb, int* __restrict__ offsets, int64_t* __restrict__ n_out) {
    __shared__ int s[256];
    int carry = 0;
    for (int b0 = 0; b0 < nb; b0 += 256) {
        const int b = b0 + threadIdx.x;
        const int v = b < nb ? counts[b] : 0;
        int total;
        const int ex = block_exclusive_scan256(v, s, &total);
        if (b < nb) offsets[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *n_out = carry;
}

__global__ __launch_bounds__(256)
void region_scatter_kernel(const unsigned char* __restrict__ keep, int64_t ncells, int gx, int step, const int* __restrict__ offsets,
                           int32_t* __restrict__ cell_xy) {
    __shared__ int s[256];
    const int64_t c0 = (int64_t)blockIdx.x * REGION_CELLS_PER_BLOCK + (int64_t)threadIdx.x * REGION_CELLS_PER_THREAD;
    int total;
    int pos = offsets[blockIdx.x] + block_exclusive_scan256(region_thread_kept(keep, ncells, c0), s, &total);
    for (int j = 0; j < REGION_CELLS_PER_THREAD; ++j) {
        const int64_t c = c0 + j;
        if (c < ncells && (!keep || keep[c])) {
            cell_xy[2 * (int64_t)pos] = (int32_t)((c % gx) * step);
            cell_xy[2 * (int64_t)pos + 1] = (int32_t)((c / gx) * step);
            ++pos;
        }
    }
}

__global__ __launch_bounds__(256)
void region_check_cells_kernel(const int32_t* __restrict__ cell_xy, int B, int64_t H, int64_t W, int patch, int* __restrict__ bad) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < B; i += gridDim.x * 256) {
        const int64_t x = cell_xy[2 * (int64_t)i], y = cell_xy[2 * (int64_t)i + 1];
        if (x < 0 || y < 0 || x + patch > W || y + patch > H) *bad = 1;        // every writer stores the same value
    }
}

// one wave per tile row: 224 RGB pixels = 672 bytes = 168 dwords stored whole
__global__ __launch_bounds__(256)
void region_copy224_kernel(const unsigned char* __restrict__ region, int64_t row_stride, int ps, const int32_t* __restrict__ cell_xy,
                           int B, unsigned char* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t rows = (int64_t)B * 224;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
        const int64_t b = r / 224;
        const int y = (int)(r - b * 224);
        const unsigned char* src = region + ((int64_t)cell_xy[2 * b + 1] + y) * row_stride + (int64_t)cell_xy[2 * b] * ps;
        unsigned* dst = reinterpret_cast<unsigned*>(out + r * 672);
        for (int w = lane; w < 168; w += 64) {
            unsigned v = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = 4 * w + k, px = j / 3;
                v |= (unsigned)src[(int64_t)px * ps + (j - 3 * px)] << (8 * k);
            }
            dst[w] = v;
        }
    }
}

// tmp[b][y][xx][c] = sum_x region[cy_b + y][cx_b + x0 + x][c] * k[x]    (resize_h_u8_kernel of rowops.hip, read from the region)
__global__ __launch_bounds__(256)
void region_resize_h_u8_kernel(const unsigned char* __restrict__ region, int64_t row_stride, int ps, const int32_t* __restrict__ cell_xy,
                               int B, int patch, const int* __restrict__ bounds, const int* __restrict__ kk, int ksize, int ncols,
                               unsigned char* __restrict__ tmp) {
    const int64_t total = (int64_t)B * patch * ncols;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int xx = (int)(i % ncols);
        const int64_t row = i / ncols;                            // b * patch + y
        const int64_t b = row / patch;
        const int y = (int)(row - b * patch);
        const int x0 = bounds[2 * xx], n = bounds[2 * xx + 1];
        const int* k = kk + (int64_t)xx * ksize;
        const unsigned char* s = region + ((int64_t)cell_xy[2 * b + 1] + y) * row_stride + ((int64_t)cell_xy[2 * b] + x0) * ps;
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
        for (int x = 0; x < n; ++x) {
            const int w = k[x];
            const unsigned char* p = s + (int64_t)x * ps;
            a0 += p[0] * w; a1 += p[1] * w; a2 += p[2] * w;
        }
        unsigned char* d = tmp + i * 3;
        d[0] = clip8_fixed(a0); d[1] = clip8_fixed(a1); d[2] = clip8_fixed(a2);
    }
}

}  // namespace keepk
using namespace keepk;

static unsigned grid_for(int64_t items, int per_block) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (unsigned)(b > 65536 ? 65536 : (b < 1 ? 1 : b));
}

void launch_region_grid(const unsigned char* region, int64_t row_stride, int ps, int gx, int64_t ncells, int patch, int step, int sat_min,
                        int min_pixels, unsigned char* keep, int* counts, int* offsets, int32_t* cell_xy, int64_t* n_out, hipStream_t s) {
    if (min_pixels > 0)
        hipLaunchKernelGGL(region_tissue_count_kernel, dim3(grid_for(ncells, 1)), dim3(256), 0, s, region, row_stride, ps, gx, ncells, patch,
                           step, (unsigned)sat_min, min_pixels, keep);
    else
        keep = nullptr;                                           // count >= 0 holds for every cell: no pass over the pixels
    launch_region_compact(keep, gx, ncells, step, counts, offsets, cell_xy, n_out, s);
}

void launch_region_compact(const unsigned char* keep, int gx, int64_t ncells, int step, int* counts, int* offsets, int32_t* cell_xy,
                           int64_t* n_out, hipStream_t s) {
    const int nb = (int)((ncells + REGION_CELLS_PER_BLOCK - 1) / REGION_CELLS_PER_BLOCK);
    hipLaunchKernelGGL(region_block_count_kernel, dim3(nb), dim3(256), 0, s, keep, ncells, counts);
    hipLaunchKernelGGL(region_scan_kernel, dim3(1), dim3(256), 0, s, counts, nb, offsets, n_out);
    hipLaunchKernelGGL(region_scatter_kernel, dim3(nb), dim3(256), 0, s, keep, ncells, gx, step, offsets, cell_xy);
}

void launch_region_check_cells(const int32_t* cell_xy, int B, int64_t H, int64_t W, int patch, int* bad, hipStream_t s) {
    hipLaunchKernelGGL(region_check_cells_kernel, dim3(grid_for(B, 256)), dim3(256), 0, s, cell_xy, B, H, W, patch, bad);
}

void launch_region_patches_u8(const unsigned char* region, int64_t row_stride, int ps, const int32_t* cell_xy, int B, int patch,
                              const int* xb, const int* xk, int xks, const int* yb, const int* yk, int yks, unsigned char* tmp,
                              unsigned char* out, hipStream_t s) {
    if (patch == 224) {
        hipLaunchKernelGGL(region_copy224_kernel, dim3(grid_for((int64_t)B * 224, 4)), dim3(256), 0, s, region, row_stride, ps, cell_xy, B, out);
        return;
    }
    hipLaunchKernelGGL(region_resize_h_u8_kernel, dim3(grid_for((int64_t)B * patch * 224, 256)), dim3(256), 0, s, region, row_stride, ps,
                       cell_xy, B, patch, xb, xk, xks, 224, tmp);
    launch_resize_v_u8(tmp, B, patch, 224, yb, yk, yks, 0, 224, out, s);
}
