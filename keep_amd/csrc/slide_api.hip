// The slide-geometry entry points of include/keep_hip.h: patch grid, tissue mask, stain normalisation, tile quality, heatmap, sort / rank, region table, outlines, polygon
// fill, segmentation evaluation, bootstrap resampling, the subtype map, tile clustering, the linear probe, attention MIL and nearest neighbours.  Host code only: each function validates its arguments, carves its workspace from the handle's
// arena, calls the launch_* of its kernel file (region / tissue / stain / quality / heatmap / rank / components / outline / annotation / eval / bootstrap .hip) and
// reports the launch.  Of the handle (handle.h) they use the device, the error text, the arena and the sticky error flag.
#include "handle.h"

#include <algorithm>

static size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// Checks that several entry points share; `who` is the entry point's name as its error messages spell it.
// 1 <= H, W and H W <= limit (the kernels index pixels with an int32)
static bool pixels_ok(int64_t H, int64_t W, int64_t limit) { return H >= 1 && W >= 1 && H <= limit && W <= limit && H * W <= limit; }

// level-0 origin of a raster or mask: within +-2^40, so that origin + coordinate stays far inside an int64
static int origin_check(keep_handle* h, const char* who, int64_t origin_x, int64_t origin_y) {
    constexpr int64_t omax = (int64_t)1 << 40;
    if (origin_x < -omax || origin_x > omax || origin_y < -omax || origin_y > omax)
        return h->fail(KEEP_EINVAL, "%s: origin (%lld, %lld) outside +-2^40", who, (long long)origin_x, (long long)origin_y);
    return KEEP_OK;
}

// a strided uint8 view of RGB or RGBA pixels, rows at least a row's bytes apart; two checks because tissue_median_hist has its pixel cap between them
static int pix_stride_check(keep_handle* h, const char* who, int pix_stride) {
    if (pix_stride != 3 && pix_stride != 4) return h->fail(KEEP_EINVAL, "%s: pixel stride %d (3 = RGB, 4 = RGBA)", who, pix_stride);
    return KEEP_OK;
}
static int row_stride_check(keep_handle* h, const char* who, int64_t W, int64_t row_stride_bytes, int pix_stride) {
    if (row_stride_bytes < W * pix_stride)
        return h->fail(KEEP_EINVAL, "%s: row stride %lld bytes < width %lld x pixel stride %d", who, (long long)row_stride_bytes, (long long)W, pix_stride);
    return KEEP_OK;
}

extern "C" {

static int region_view_check(keep_handle* h, const unsigned char* region, int64_t H, int64_t W, int64_t row_stride_bytes, int pix_stride,
                             int64_t patch) {
    if (!region || H < 1 || W < 1) return h->fail(KEEP_EINVAL, "region: null pointer or empty shape %lldx%lld", (long long)H, (long long)W);
    if (int rc = pix_stride_check(h, "region", pix_stride)) return rc;
    if (W > INT32_MAX || H > INT32_MAX || row_stride_bytes < W * pix_stride)
        return h->fail(KEEP_EINVAL, "region: row stride %lld bytes < width %lld x pixel stride %d (or a side >= 2^31)", (long long)row_stride_bytes,
                       (long long)W, pix_stride);
    if (patch < 16 || patch > REGION_MAX_PATCH) return h->fail(KEEP_EINVAL, "region: patch %lld outside [16, %d]", (long long)patch, REGION_MAX_PATCH);
    return KEEP_OK;
}

int keep_region_grid(keep_handle* h, const unsigned char* region, int64_t H, int64_t W, int64_t row_stride_bytes, int pix_stride, int64_t patch,
                     int64_t step, int sat_min, int64_t min_pixels, int32_t* cell_xy_out, int64_t* n_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    int rc = region_view_check(h, region, H, W, row_stride_bytes, pix_stride, patch);
    if (rc) return rc;
    if (step < 1) return h->fail(KEEP_EINVAL, "region_grid: step %lld < 1", (long long)step);
    if (sat_min < 0 || sat_min > 255) return h->fail(KEEP_EINVAL, "region_grid: sat_min %d outside [0, 255]", sat_min);
    if (min_pixels < 0 || min_pixels > patch * patch)
        return h->fail(KEEP_EINVAL, "region_grid: min_pixels %lld outside [0, patch^2 = %lld]", (long long)min_pixels, (long long)(patch * patch));
    if (!cell_xy_out || !n_out) return h->fail(KEEP_EINVAL, "region_grid: null output");
    const int64_t gx = W >= patch ? (W - patch) / step + 1 : 0, gy = H >= patch ? (H - patch) / step + 1 : 0;
    const int64_t ncells = gx * gy;
    if (ncells > INT32_MAX) return h->fail(KEEP_EINVAL, "region_grid: %lld cells (limit 2^31 - 1)", (long long)ncells);
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    if (ncells == 0) {
        HIPCHK(h, hipMemsetAsync(n_out, 0, sizeof(int64_t), s));
        return KEEP_OK;
    }
    const int64_t nb = (ncells + REGION_GRID_CHUNK - 1) / REGION_GRID_CHUNK;
    const size_t b_keep = align_up((size_t)ncells), b_counts = align_up((size_t)nb * 4);
    rc = ensure_arena(h, b_keep + 2 * b_counts);
    if (rc) return rc;
    launch_region_grid(region, row_stride_bytes, pix_stride, (int)gx, ncells, (int)patch, (int)step, sat_min, (int)min_pixels,
                       (unsigned char*)h->arena, (int*)(h->arena + b_keep), (int*)(h->arena + b_keep + b_counts), cell_xy_out, n_out, s);
    return check_launch(h, "region_grid");
}

int keep_region_patches_u8(keep_handle* h, const unsigned char* region, int64_t H, int64_t W, int64_t row_stride_bytes, int pix_stride,
                           const int32_t* cell_xy, int64_t B, int64_t patch, const int32_t* xbounds, const int32_t* xweights, int xksize,
                           const int32_t* ybounds, const int32_t* yweights, int yksize, unsigned char* out, void* stream) {
    if (!h) return KEEP_EINVAL;
    int rc = region_view_check(h, region, H, W, row_stride_bytes, pix_stride, patch);
    if (rc) return rc;
    if (B < 0 || B > INT32_MAX / 224 || (B > 0 && (!cell_xy || !out))) return h->fail(KEEP_EINVAL, "region_patches: bad B %lld or null pointer", (long long)B);
    if (patch != 224 && (!xbounds || !xweights || !ybounds || !yweights || xksize < 1 || yksize < 1))
        return h->fail(KEEP_EINVAL, "region_patches: patch %lld needs the Resize(224) tables", (long long)patch);
    if (patch > H || patch > W) return h->fail(KEEP_EINVAL, "region_patches: patch %lld larger than the region %lldx%lld", (long long)patch,
                                               (long long)W, (long long)H);
    if (B == 0) return KEEP_OK;
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    // [flag][horizontally resized rows]: the flag is read back before any pixel is touched (the one synchronisation of this call),
    // so a cell outside the region is an error, not an out-of-bounds read
    const size_t b_flag = align_up(sizeof(int)), b_tmp = patch == 224 ? 0 : align_up((size_t)B * patch * 224 * 3);
    rc = ensure_arena(h, b_flag + b_tmp);
    if (rc) return rc;
    int* bad = (int*)h->arena;
    HIPCHK(h, hipMemsetAsync(bad, 0, sizeof(int), s));
    launch_region_check_cells(cell_xy, (int)B, H, W, (int)patch, bad, s);
    rc = check_launch(h, "region_check_cells");
    if (rc) return rc;
    int bad_h = 0;
    HIPCHK(h, hipMemcpyAsync(&bad_h, bad, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (bad_h) return h->fail(KEEP_EINVAL, "region_patches: a cell (x, y) has x < 0, y < 0, x + %lld > %lld or y + %lld > %lld", (long long)patch,
                              (long long)W, (long long)patch, (long long)H);
    launch_region_patches_u8(region, row_stride_bytes, pix_stride, cell_xy, (int)B, (int)patch, xbounds, xweights, xksize, ybounds, yweights,
                             yksize, (unsigned char*)h->arena + b_flag, out, s);
    return check_launch(h, "region_patches_u8");
}

int keep_tissue_median_hist(keep_handle* h, const unsigned char* thumb, int64_t H, int64_t W, int64_t row_stride_bytes, int pix_stride,
                            int ksize, unsigned char* median_out, int32_t* hist_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!thumb || H < 1 || W < 1) return h->fail(KEEP_EINVAL, "tissue_median_hist: null pointer or empty shape %lldx%lld", (long long)H, (long long)W);
    if (int rc = pix_stride_check(h, "tissue_median_hist", pix_stride)) return rc;
    if (!pixels_ok(H, W, TISSUE_MAX_PIXELS)) return h->fail(KEEP_EINVAL, "tissue_median_hist: %lldx%lld pixels (limit H W <= 2^30)", (long long)H, (long long)W);
    if (int rc = row_stride_check(h, "tissue_median_hist", W, row_stride_bytes, pix_stride)) return rc;
    if (ksize < 1 || ksize > 15 || ksize % 2 == 0) return h->fail(KEEP_EINVAL, "tissue_median_hist: ksize %d (odd, 1..15)", ksize);
    if (!median_out || !hist_out) return h->fail(KEEP_EINVAL, "tissue_median_hist: null output");
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(h, hipMemsetAsync(hist_out, 0, 256 * sizeof(int32_t), s));
    if (launch_tissue_median_hist(thumb, row_stride_bytes, pix_stride, (int)H, (int)W, ksize, median_out, hist_out, s))
        return h->fail(KEEP_EUNSUPPORTED, "tissue_median_hist: no kernel for ksize %d", ksize);
    return check_launch(h, "tissue_median_hist");
}

int keep_tissue_mask(keep_handle* h, const unsigned char* median, int64_t H, int64_t W, int threshold, int close, int64_t min_hole,
                     int64_t min_area, unsigned char* mask_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!median || !mask_out || median == mask_out) return h->fail(KEEP_EINVAL, "tissue_mask: null pointer, or mask_out aliases median");
    if (!pixels_ok(H, W, TISSUE_MAX_PIXELS)) return h->fail(KEEP_EINVAL, "tissue_mask: %lldx%lld pixels (1 <= H W <= 2^30)", (long long)H, (long long)W);
    if (threshold < 0 || threshold > 255) return h->fail(KEEP_EINVAL, "tissue_mask: threshold %d outside [0, 255]", threshold);
    if (close < 0 || close > 31) return h->fail(KEEP_EINVAL, "tissue_mask: close %d outside [0, 31]", close);
    if (min_hole < 0 || min_area < 0) return h->fail(KEEP_EINVAL, "tissue_mask: min_hole %lld / min_area %lld < 0", (long long)min_hole, (long long)min_area);
    KEEP_ON_DEVICE(h);
    const size_t n = (size_t)(H * W);
    const bool label = min_hole > 0 || min_area > 0;
    const size_t b_tmp = close > 0 ? align_up(n) : 0, b_lab = label ? align_up(n * 4) : 0;
    int rc = ensure_arena(h, b_tmp + 2 * b_lab);
    if (rc) return rc;
    // an area never exceeds H W <= 2^30: larger bounds decide the same
    launch_tissue_mask(median, (int)H, (int)W, threshold, close, (int)std::min<int64_t>(min_hole, TISSUE_MAX_PIXELS),
                       (int)std::min<int64_t>(min_area, TISSUE_MAX_PIXELS), (unsigned char*)h->arena, (int*)(h->arena + b_tmp),
                       (int*)(h->arena + b_tmp + b_lab), h->err_flag, mask_out, (hipStream_t)stream);
    return check_launch(h, "tissue_mask");
}

int keep_region_grid_mask(keep_handle* h, const unsigned char* mask, int64_t mh, int64_t mw, int64_t downsample, int64_t H, int64_t W,
                          int64_t patch, int64_t step, int64_t origin_x, int64_t origin_y, int mode, int32_t* cell_xy_out, int64_t* n_out,
                          void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!mask || mh < 1 || mw < 1 || mh > INT32_MAX || mw > INT32_MAX)
        return h->fail(KEEP_EINVAL, "region_grid_mask: null mask or bad mask shape %lldx%lld", (long long)mh, (long long)mw);
    if (downsample < 1 || downsample > INT32_MAX) return h->fail(KEEP_EINVAL, "region_grid_mask: downsample %lld < 1", (long long)downsample);
    if (H < 1 || W < 1 || H > INT32_MAX || W > INT32_MAX) return h->fail(KEEP_EINVAL, "region_grid_mask: region shape %lldx%lld", (long long)H, (long long)W);
    if (patch < 16 || patch > REGION_MAX_PATCH) return h->fail(KEEP_EINVAL, "region_grid_mask: patch %lld outside [16, %d]", (long long)patch, REGION_MAX_PATCH);
    if (step < 1) return h->fail(KEEP_EINVAL, "region_grid_mask: step %lld < 1", (long long)step);
    if (int rc = origin_check(h, "region_grid_mask", origin_x, origin_y)) return rc;
    if (mode < KEEP_MASK_FOUR_PT || mode > KEEP_MASK_CENTER) return h->fail(KEEP_EINVAL, "region_grid_mask: mode %d (0 four_pt, 1 four_pt_hard, 2 center)", mode);
    if (!cell_xy_out || !n_out) return h->fail(KEEP_EINVAL, "region_grid_mask: null output");
    const int64_t gx = W >= patch ? (W - patch) / step + 1 : 0, gy = H >= patch ? (H - patch) / step + 1 : 0;
    const int64_t ncells = gx * gy;
    if (ncells > INT32_MAX) return h->fail(KEEP_EINVAL, "region_grid_mask: %lld cells (limit 2^31 - 1)", (long long)ncells);
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    if (ncells == 0) {
        HIPCHK(h, hipMemsetAsync(n_out, 0, sizeof(int64_t), s));
        return KEEP_OK;
    }
    const int64_t nb = (ncells + REGION_GRID_CHUNK - 1) / REGION_GRID_CHUNK;
    const size_t b_keep = align_up((size_t)ncells), b_counts = align_up((size_t)nb * 4);
    int rc = ensure_arena(h, b_keep + 2 * b_counts);
    if (rc) return rc;
    unsigned char* keep = (unsigned char*)h->arena;
    launch_tissue_grid_cells(mask, mh, mw, downsample, (int)gx, ncells, (int)patch, (int)step, origin_x, origin_y, mode, keep, s);
    launch_region_compact(keep, (int)gx, ncells, (int)step, (int*)(h->arena + b_keep), (int*)(h->arena + b_keep + b_counts), cell_xy_out, n_out, s);
    return check_launch(h, "region_grid_mask");
}

int keep_heat_accumulate(keep_handle* h, const int64_t* coords, const float* values, int64_t N, int64_t patch, int64_t downsample,
                         int64_t H, int64_t W, int64_t origin_x, int64_t origin_y, int zero_first, int64_t* acc, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!acc || ((uintptr_t)acc & 7)) return h->fail(KEEP_EINVAL, "heat_accumulate: acc is null or not 8-byte aligned");
    if (N < 0 || N > HEAT_MAX_TILES) return h->fail(KEEP_EINVAL, "heat_accumulate: %lld tiles (0 .. 2^24 - 1)", (long long)N);
    if (N > 0 && (!coords || !values)) return h->fail(KEEP_EINVAL, "heat_accumulate: null coords or values");
    if (!pixels_ok(H, W, HEAT_MAX_PIXELS)) return h->fail(KEEP_EINVAL, "heat_accumulate: %lldx%lld: raster shape (1 <= H W <= 2^30)", (long long)H, (long long)W);
    if (patch < 1 || patch > HEAT_MAX_PATCH) return h->fail(KEEP_EINVAL, "heat_accumulate: patch %lld outside [1, 2^30]", (long long)patch);
    if (downsample < 1 || downsample > patch)
        return h->fail(KEEP_EINVAL, "heat_accumulate: downsample %lld outside [1, patch = %lld]", (long long)downsample, (long long)patch);
    if (int rc = origin_check(h, "heat_accumulate", origin_x, origin_y)) return rc;
    if (origin_x % downsample || origin_y % downsample)
        return h->fail(KEEP_EINVAL, "heat_accumulate: origin (%lld, %lld) is not a multiple of downsample %lld", (long long)origin_x,
                       (long long)origin_y, (long long)downsample);
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    if (zero_first) HIPCHK(h, hipMemsetAsync(acc, 0, (size_t)(H * W) * sizeof(int64_t), s));
    launch_heat_accumulate(coords, values, N, patch, downsample, (int)H, (int)W, origin_x, origin_y, acc, s);
    return check_launch(h, "heat_accumulate");
}

int keep_heat_accumulate_cells(keep_handle* h, const int64_t* coords, const float* values, int64_t N, int64_t gh, int64_t gw, int64_t patch,
                               int64_t downsample, int64_t H, int64_t W, int64_t origin_x, int64_t origin_y, int zero_first, int64_t* acc,
                               void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!acc || ((uintptr_t)acc & 7)) return h->fail(KEEP_EINVAL, "heat_accumulate_cells: acc is null or not 8-byte aligned");
    if (N < 0 || N > HEAT_MAX_TILES) return h->fail(KEEP_EINVAL, "heat_accumulate_cells: %lld tiles (0 .. 2^24 - 1)", (long long)N);
    if (N > 0 && (!coords || !values)) return h->fail(KEEP_EINVAL, "heat_accumulate_cells: null coords or values");
    if (!pixels_ok(H, W, HEAT_MAX_PIXELS))
        return h->fail(KEEP_EINVAL, "heat_accumulate_cells: %lldx%lld: raster shape (1 <= H W <= 2^30)", (long long)H, (long long)W);
    if (patch < 1 || patch > HEAT_MAX_PATCH) return h->fail(KEEP_EINVAL, "heat_accumulate_cells: patch %lld outside [1, 2^30]", (long long)patch);
    if (gh < 1 || gw < 1 || gh > patch || gw > patch || gh * gw > HEAT_MAX_CELLS || patch % gw || patch % gh)
        return h->fail(KEEP_EINVAL, "heat_accumulate_cells: grid %lldx%lld: both sides must divide patch %lld (and gh gw <= 2^24)", (long long)gh,
                       (long long)gw, (long long)patch);
    const int64_t cmin = std::min(patch / gw, patch / gh);
    if (downsample < 1 || downsample > cmin)
        return h->fail(KEEP_EINVAL, "heat_accumulate_cells: downsample %lld outside [1, cell side = %lld]", (long long)downsample, (long long)cmin);
    if (int rc = origin_check(h, "heat_accumulate_cells", origin_x, origin_y)) return rc;
    if (origin_x % downsample || origin_y % downsample)
        return h->fail(KEEP_EINVAL, "heat_accumulate_cells: origin (%lld, %lld) is not a multiple of downsample %lld", (long long)origin_x,
                       (long long)origin_y, (long long)downsample);
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    if (zero_first) HIPCHK(h, hipMemsetAsync(acc, 0, (size_t)(H * W) * sizeof(int64_t), s));
    launch_heat_accumulate_cells(coords, values, N, (int)gh, (int)gw, patch, downsample, (int)H, (int)W, origin_x, origin_y, acc, s);
    return check_launch(h, "heat_accumulate_cells");
}

int keep_heat_mean(keep_handle* h, const int64_t* acc, int64_t H, int64_t W, float uncovered, float* mean_out, int32_t* count_out,
                   unsigned char* pred_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!acc || ((uintptr_t)acc & 7)) return h->fail(KEEP_EINVAL, "heat_mean: acc is null or not 8-byte aligned");
    if (!pixels_ok(H, W, HEAT_MAX_PIXELS)) return h->fail(KEEP_EINVAL, "heat_mean: %lldx%lld: raster shape (1 <= H W <= 2^30)", (long long)H, (long long)W);
    if (!mean_out && !count_out && !pred_out) return h->fail(KEEP_EINVAL, "heat_mean: no output");
    if (((uintptr_t)mean_out & 3) || ((uintptr_t)count_out & 3)) return h->fail(KEEP_EINVAL, "heat_mean: mean_out / count_out not 4-byte aligned");
    KEEP_ON_DEVICE(h);
    launch_heat_mean(acc, (int)H, (int)W, uncovered, mean_out, count_out, pred_out, (hipStream_t)stream);
    return check_launch(h, "heat_mean");
}

int keep_heat_render(keep_handle* h, const int64_t* acc, int64_t H, int64_t W, const unsigned char* thumb, int64_t row_stride_bytes,
                     int pix_stride, int background_rgb, const unsigned char* mask, const unsigned char* lut, int alpha, int lo16, int hi16,
                     int min16, unsigned char* out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!acc || ((uintptr_t)acc & 7)) return h->fail(KEEP_EINVAL, "heat_render: acc is null or not 8-byte aligned");
    if (!lut || !out) return h->fail(KEEP_EINVAL, "heat_render: null lut or output");
    if (!pixels_ok(H, W, HEAT_MAX_PIXELS)) return h->fail(KEEP_EINVAL, "heat_render: %lldx%lld: raster shape (1 <= H W <= 2^30)", (long long)H, (long long)W);
    if (thumb) {
        if (int rc = pix_stride_check(h, "heat_render", pix_stride)) return rc;
        if (int rc = row_stride_check(h, "heat_render", W, row_stride_bytes, pix_stride)) return rc;
    } else if (background_rgb < 0 || background_rgb > 0xFFFFFF) {
        return h->fail(KEEP_EINVAL, "heat_render: background 0x%x outside [0, 0xFFFFFF]", background_rgb);
    }
    if (alpha < 0 || alpha > 256) return h->fail(KEEP_EINVAL, "heat_render: alpha %d outside [0, 256]", alpha);
    if (lo16 < 0 || hi16 > 65535 || lo16 >= hi16) return h->fail(KEEP_EINVAL, "heat_render: window [%d, %d] (0 <= lo16 < hi16 <= 65535)", lo16, hi16);
    if (min16 < 0 || min16 > 65535) return h->fail(KEEP_EINVAL, "heat_render: min16 %d outside [0, 65535]", min16);
    KEEP_ON_DEVICE(h);
    launch_heat_render(acc, (int)H, (int)W, thumb, row_stride_bytes, pix_stride, (unsigned)background_rgb, mask, lut, alpha, lo16, hi16, min16,
                       out, (hipStream_t)stream);
    return check_launch(h, "heat_render");
}

int keep_heat_smooth(keep_handle* h, const int64_t* acc, int64_t H, int64_t W, const unsigned char* mask, const int32_t* taps, int radius,
                     int64_t* acc_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!acc || ((uintptr_t)acc & 7)) return h->fail(KEEP_EINVAL, "heat_smooth: acc is null or not 8-byte aligned");
    if (!acc_out || ((uintptr_t)acc_out & 7)) return h->fail(KEEP_EINVAL, "heat_smooth: acc_out is null or not 8-byte aligned");
    if (acc_out == acc) return h->fail(KEEP_EINVAL, "heat_smooth: acc_out aliases acc");
    if (!pixels_ok(H, W, HEAT_MAX_PIXELS)) return h->fail(KEEP_EINVAL, "heat_smooth: %lldx%lld: raster shape (1 <= H W <= 2^30)", (long long)H, (long long)W);
    if (!taps || ((uintptr_t)taps & 3)) return h->fail(KEEP_EINVAL, "heat_smooth: taps is null or not 4-byte aligned");
    if (radius < 1 || radius > HEAT_SMOOTH_MAX_RADIUS) return h->fail(KEEP_EINVAL, "heat_smooth: radius %d outside [1, %d]", radius, HEAT_SMOOTH_MAX_RADIUS);
    KEEP_ON_DEVICE(h);
    const size_t n = (size_t)(H * W), b_a = align_up(n * 4);
    int rc = ensure_arena(h, b_a + align_up(n * 2));
    if (rc) return rc;
    launch_heat_smooth(acc, (int)H, (int)W, mask, taps, radius, (unsigned*)h->arena, (unsigned short*)(h->arena + b_a), acc_out, (hipStream_t)stream);
    return check_launch(h, "heat_smooth");
}

int keep_sort_f32(keep_handle* h, const float* values, int64_t M, float* sorted_out, int64_t* n_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (M < 1 || M > SORT_MAX) return h->fail(KEEP_EINVAL, "sort_f32: %lld values (1 .. 2^24 - 1)", (long long)M);
    if (!values || !sorted_out || !n_out) return h->fail(KEEP_EINVAL, "sort_f32: null pointer");
    if (((uintptr_t)values & 3) || ((uintptr_t)sorted_out & 3) || ((uintptr_t)n_out & 7)) return h->fail(KEEP_EINVAL, "sort_f32: values / sorted_out / n_out not aligned");
    KEEP_ON_DEVICE(h);
    size_t table_off, totals_off;
    int rc = ensure_arena(h, sort_workspace_bytes(M, &table_off, &totals_off));
    if (rc) return rc;
    launch_sort_f32(values, M, (unsigned char*)h->arena, sorted_out, n_out, (hipStream_t)stream);
    return check_launch(h, "sort_f32");
}

int keep_rank_f32(keep_handle* h, const float* sorted, int64_t M, const int64_t* n_dev, const float* queries, int64_t N, int self,
                  float* pct_out, int32_t* less_out, int32_t* eq_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (M < 1 || M > SORT_MAX) return h->fail(KEEP_EINVAL, "rank_f32: a population of %lld values (1 .. 2^24 - 1)", (long long)M);
    if (N < 0 || N > SORT_MAX) return h->fail(KEEP_EINVAL, "rank_f32: %lld queries (0 .. 2^24 - 1)", (long long)N);
    if (!sorted || !n_dev || (N > 0 && !queries)) return h->fail(KEEP_EINVAL, "rank_f32: null sorted, n or queries");
    if (self != 0 && self != 1) return h->fail(KEEP_EINVAL, "rank_f32: self %d (0 or 1)", self);
    if (!pct_out && !less_out && !eq_out) return h->fail(KEEP_EINVAL, "rank_f32: no output");
    if (((uintptr_t)sorted & 3) || ((uintptr_t)n_dev & 7) || ((uintptr_t)queries & 3) || ((uintptr_t)pct_out & 3) || ((uintptr_t)less_out & 3) ||
        ((uintptr_t)eq_out & 3))
        return h->fail(KEEP_EINVAL, "rank_f32: a pointer is not aligned");
    KEEP_ON_DEVICE(h);
    launch_rank_f32(sorted, M, n_dev, queries, N, self, pct_out, less_out, eq_out, (hipStream_t)stream);
    return check_launch(h, "rank_f32");
}

int keep_regions_label(keep_handle* h, const unsigned char* mask, int64_t H, int64_t W, int connectivity, int64_t min_area, int32_t* labels_out,
                       int64_t* n_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!mask || !labels_out || !n_out) return h->fail(KEEP_EINVAL, "regions_label: null pointer");
    if (!pixels_ok(H, W, TISSUE_MAX_PIXELS)) return h->fail(KEEP_EINVAL, "regions_label: %lldx%lld pixels (1 <= H W <= 2^30)", (long long)H, (long long)W);
    if (connectivity != 4 && connectivity != 8) return h->fail(KEEP_EINVAL, "regions_label: connectivity %d (4 or 8)", connectivity);
    if (min_area < 1) return h->fail(KEEP_EINVAL, "regions_label: min_area %lld < 1", (long long)min_area);
    if (((uintptr_t)labels_out & 3) || ((uintptr_t)n_out & 7)) return h->fail(KEEP_EINVAL, "regions_label: labels_out / n_out not aligned");
    KEEP_ON_DEVICE(h);
    const size_t n = (size_t)(H * W);
    const size_t b_lab = align_up(n * 4), b_counts = align_up(((n + REGIONS_SCAN_CHUNK - 1) / REGIONS_SCAN_CHUNK) * sizeof(int));
    int rc = ensure_arena(h, 2 * b_lab + 2 * b_counts);
    if (rc) return rc;
    // an area never exceeds H W <= 2^30: a larger bound decides the same (every component is dropped)
    launch_regions_label(mask, (int)H, (int)W, connectivity == 8, (int)std::min<int64_t>(min_area, TISSUE_MAX_PIXELS + 1), (int*)h->arena,
                         (int*)(h->arena + b_lab), (int*)(h->arena + 2 * b_lab), (int*)(h->arena + 2 * b_lab + b_counts), h->err_flag,
                         labels_out, n_out, (hipStream_t)stream);
    return check_launch(h, "regions_label");
}

int keep_regions_table(keep_handle* h, const int32_t* labels, int64_t H, int64_t W, int64_t n, const int64_t* acc, int64_t* table_out,
                       void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!labels || ((uintptr_t)labels & 3)) return h->fail(KEEP_EINVAL, "regions_table: labels is null or not 4-byte aligned");
    if (!pixels_ok(H, W, TISSUE_MAX_PIXELS)) return h->fail(KEEP_EINVAL, "regions_table: %lldx%lld pixels (1 <= H W <= 2^30)", (long long)H, (long long)W);
    if (n < 0 || n > H * W) return h->fail(KEEP_EINVAL, "regions_table: n = %lld outside [0, H W]", (long long)n);
    if ((uintptr_t)acc & 7) return h->fail(KEEP_EINVAL, "regions_table: acc is not 8-byte aligned");
    if (n > 0 && (!table_out || ((uintptr_t)table_out & 7))) return h->fail(KEEP_EINVAL, "regions_table: table_out is null or not 8-byte aligned");
    KEEP_ON_DEVICE(h);
    launch_regions_table(labels, (int)H, (int)W, n, acc, table_out, (hipStream_t)stream);
    return check_launch(h, "regions_table");
}

int keep_outline_count(keep_handle* h, const int32_t* labels, int64_t H, int64_t W, int64_t n, int connectivity, int64_t* counts_out,
                       void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!labels || ((uintptr_t)labels & 3)) return h->fail(KEEP_EINVAL, "outline_count: labels is null or not 4-byte aligned");
    if (!pixels_ok(H, W, OUTLINE_MAX_PIXELS)) return h->fail(KEEP_EINVAL, "outline_count: %lldx%lld pixels (1 <= H W <= 2^28)", (long long)H, (long long)W);
    if (n < 0 || n > H * W) return h->fail(KEEP_EINVAL, "outline_count: n = %lld outside [0, H W]", (long long)n);
    if (connectivity != 4 && connectivity != 8) return h->fail(KEEP_EINVAL, "outline_count: connectivity %d (4 or 8)", connectivity);
    if (!counts_out || ((uintptr_t)counts_out & 7)) return h->fail(KEEP_EINVAL, "outline_count: counts_out is null or not 8-byte aligned");
    KEEP_ON_DEVICE(h);
    int rc = ensure_arena(h, outline_count_workspace_bytes(H * W));
    if (rc) return rc;
    launch_outline_count(labels, (int)H, (int)W, (int)n, (unsigned char*)h->arena, counts_out, (hipStream_t)stream);
    return check_launch(h, "outline_count");
}

int keep_outline_trace(keep_handle* h, const int32_t* labels, int64_t H, int64_t W, int64_t n, int connectivity, int64_t E, int64_t V,
                       int32_t* vertices_out, int64_t* rings_out, int64_t ring_cap, int64_t* r_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!labels || ((uintptr_t)labels & 3)) return h->fail(KEEP_EINVAL, "outline_trace: labels is null or not 4-byte aligned");
    if (!pixels_ok(H, W, OUTLINE_MAX_PIXELS)) return h->fail(KEEP_EINVAL, "outline_trace: %lldx%lld pixels (1 <= H W <= 2^28)", (long long)H, (long long)W);
    if (n < 1 || n > H * W) return h->fail(KEEP_EINVAL, "outline_trace: n = %lld outside [1, H W] (without a region there is nothing to trace)", (long long)n);
    if (connectivity != 4 && connectivity != 8) return h->fail(KEEP_EINVAL, "outline_trace: connectivity %d (4 or 8)", connectivity);
    if (E < 4 || E > 4 * H * W || V < 4 || V > E)
        return h->fail(KEEP_EINVAL, "outline_trace: E = %lld, V = %lld (4 <= V <= E <= 4 H W: the values keep_outline_count wrote)", (long long)E,
                       (long long)V);
    if (!vertices_out || ((uintptr_t)vertices_out & 3)) return h->fail(KEEP_EINVAL, "outline_trace: vertices_out is null or not 4-byte aligned");
    if (ring_cap < 0) return h->fail(KEEP_EINVAL, "outline_trace: ring_cap %lld < 0", (long long)ring_cap);
    if (ring_cap > 0 && (!rings_out || ((uintptr_t)rings_out & 7))) return h->fail(KEEP_EINVAL, "outline_trace: rings_out is null or not 8-byte aligned");
    if (!r_out || ((uintptr_t)r_out & 7)) return h->fail(KEEP_EINVAL, "outline_trace: r_out is null or not 8-byte aligned");
    KEEP_ON_DEVICE(h);
    int rc = ensure_arena(h, outline_trace_workspace_bytes(H * W, E));
    if (rc) return rc;
    launch_outline_trace(labels, (int)H, (int)W, (int)n, connectivity == 8, (int)E, V, (unsigned char*)h->arena, vertices_out, rings_out, ring_cap,
                         r_out, (hipStream_t)stream);
    return check_launch(h, "outline_trace");
}

int keep_outline_draw(keep_handle* h, const int32_t* labels, int64_t H, int64_t W, const unsigned char* rgb_in, unsigned char* rgb_out, int color,
                      int width, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!labels || ((uintptr_t)labels & 3)) return h->fail(KEEP_EINVAL, "outline_draw: labels is null or not 4-byte aligned");
    if (!rgb_in || !rgb_out) return h->fail(KEEP_EINVAL, "outline_draw: null image");
    if (!pixels_ok(H, W, OUTLINE_MAX_PIXELS)) return h->fail(KEEP_EINVAL, "outline_draw: %lldx%lld pixels (1 <= H W <= 2^28)", (long long)H, (long long)W);
    if (color < 0 || color > 0xFFFFFF) return h->fail(KEEP_EINVAL, "outline_draw: color 0x%x outside [0, 0xFFFFFF]", color);
    if (width < 1 || width > OUTLINE_MAX_WIDTH) return h->fail(KEEP_EINVAL, "outline_draw: width %d outside [1, %d]", width, OUTLINE_MAX_WIDTH);
    KEEP_ON_DEVICE(h);
    int rc = ensure_arena(h, align_up((size_t)(H * W)));
    if (rc) return rc;
    launch_outline_draw(labels, (int)H, (int)W, rgb_in, rgb_out, (unsigned)color, width, (unsigned char*)h->arena, (hipStream_t)stream);
    return check_launch(h, "outline_draw");
}

int keep_poly_fill(keep_handle* h, const int64_t* vertices, int64_t V, const int64_t* ring_start, int64_t R, const int32_t* weight,
                   int64_t downsample, int64_t H, int64_t W, int64_t origin_x, int64_t origin_y, int rule, int value, const unsigned char* into,
                   unsigned char* out, int64_t* crossings_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (crossings_out) *crossings_out = 0;
    if (H < 1 || W < 1 || H > POLY_MAX_CELLS || W > POLY_MAX_CELLS || H * (W + 1) > POLY_MAX_CELLS)
        return h->fail(KEEP_EINVAL, "poly_fill: %lldx%lld pixels (h, w >= 1, h (w + 1) <= 2^28)", (long long)H, (long long)W);
    if (downsample < 1 || downsample > POLY_MAX_DOWNSAMPLE) return h->fail(KEEP_EINVAL, "poly_fill: downsample %lld outside [1, 4096]", (long long)downsample);
    if (origin_x < -POLY_MAX_COORD || origin_x > POLY_MAX_COORD || origin_y < -POLY_MAX_COORD || origin_y > POLY_MAX_COORD)
        return h->fail(KEEP_EINVAL, "poly_fill: origin (%lld, %lld) outside +-2^26", (long long)origin_x, (long long)origin_y);
    if (rule != KEEP_FILL_UNION && rule != KEEP_FILL_EVENODD) return h->fail(KEEP_EINVAL, "poly_fill: rule %d (0 union, 1 evenodd)", rule);
    if (value < 0 || value > 255) return h->fail(KEEP_EINVAL, "poly_fill: value %d outside [0, 255]", value);
    if (V < 0 || V > POLY_MAX_VERTICES || R < 0 || R > POLY_MAX_RINGS || V < 3 * R || (V > 0 && R == 0))
        return h->fail(KEEP_EINVAL, "poly_fill: V = %lld, R = %lld (V <= 2^24, R <= 2^20, every ring has >= 3 vertices)", (long long)V, (long long)R);
    if (R > 0 && (!vertices || !ring_start || !weight)) return h->fail(KEEP_EINVAL, "poly_fill: null vertices, ring_start or weight");
    if (((uintptr_t)vertices & 7) || ((uintptr_t)ring_start & 7) || ((uintptr_t)weight & 3))
        return h->fail(KEEP_EINVAL, "poly_fill: vertices / ring_start / weight not aligned");
    if (!out) return h->fail(KEEP_EINVAL, "poly_fill: out is null");
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    int rc = ensure_arena(h, poly_fill_workspace_bytes(H, W, V));
    if (rc) return rc;
    unsigned char* ws = (unsigned char*)h->arena;
    if (R == 0) {
        HIPCHK(h, hipMemsetAsync(ws, 0, (size_t)H * (size_t)(W + 1) * 4, s));
    } else {
        const int64_t* c_dev = launch_poly_count(vertices, V, ring_start, R, weight, downsample, (int)H, (int)W, origin_x, origin_y, ws, s);
        rc = check_launch(h, "poly_fill (edges)");
        if (rc) return rc;
        int64_t C = 0;
        HIPCHK(h, hipMemcpyAsync(&C, c_dev, sizeof C, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));                  // the one host synchronisation: C sizes the grid
        if (crossings_out) *crossings_out = C;
        if (C < 0 || C >= POLY_MAX_CROSSINGS)
            return h->fail(KEEP_EINVAL, "poly_fill: %lld crossings of edges with rows (< 2^31): fill at a larger downsample", (long long)C);
        if (C > 0) launch_poly_crossings(vertices, V, downsample, (int)H, (int)W, origin_x, origin_y, C, ws, s);
    }
    launch_poly_rows((int)H, (int)W, rule == KEEP_FILL_EVENODD, value, into, out, ws, s);
    return check_launch(h, "poly_fill");
}

int keep_mask_tile_counts(keep_handle* h, const unsigned char* mask, int64_t H, int64_t W, int64_t downsample, int64_t origin_x, int64_t origin_y,
                          const int64_t* coords, int64_t N, int64_t patch, int32_t* counts_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!mask) return h->fail(KEEP_EINVAL, "mask_tile_counts: mask is null");
    if (!pixels_ok(H, W, TISSUE_MAX_PIXELS)) return h->fail(KEEP_EINVAL, "mask_tile_counts: %lldx%lld pixels (1 <= H W <= 2^30)", (long long)H, (long long)W);
    if (downsample < 1 || downsample > HEAT_MAX_PATCH) return h->fail(KEEP_EINVAL, "mask_tile_counts: downsample %lld outside [1, 2^30]", (long long)downsample);
    if (patch < 1 || patch > HEAT_MAX_PATCH) return h->fail(KEEP_EINVAL, "mask_tile_counts: patch %lld outside [1, 2^30]", (long long)patch);
    if (int rc = origin_check(h, "mask_tile_counts", origin_x, origin_y)) return rc;
    if (N < 0 || N > HEAT_MAX_TILES) return h->fail(KEEP_EINVAL, "mask_tile_counts: %lld tiles (0 .. 2^24 - 1)", (long long)N);
    if (N > 0 && (!coords || ((uintptr_t)coords & 7))) return h->fail(KEEP_EINVAL, "mask_tile_counts: coords is null or not 8-byte aligned");
    if (N > 0 && (!counts_out || ((uintptr_t)counts_out & 7))) return h->fail(KEEP_EINVAL, "mask_tile_counts: counts_out is null or not 8-byte aligned");
    if (N == 0) return KEEP_OK;
    KEEP_ON_DEVICE(h);
    launch_mask_tile_counts(mask, (int)H, (int)W, downsample, origin_x, origin_y, coords, N, patch, counts_out, (hipStream_t)stream);
    return check_launch(h, "mask_tile_counts");
}

int keep_eval_roc(keep_handle* h, const float* scores, const unsigned char* labels, int64_t N, int64_t* scalars_out, float* thresholds_out,
                  int32_t* fps_out, int32_t* tps_out, unsigned char* kept_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (N < 0 || N > SORT_MAX) return h->fail(KEEP_EINVAL, "eval_roc: %lld tiles (0 .. 2^24 - 1)", (long long)N);
    if (N > 0 && (!scores || !labels)) return h->fail(KEEP_EINVAL, "eval_roc: null scores or labels");
    if (!scalars_out || ((uintptr_t)scalars_out & 7)) return h->fail(KEEP_EINVAL, "eval_roc: scalars_out is null or not 8-byte aligned");
    const int given = (thresholds_out != nullptr) + (fps_out != nullptr) + (tps_out != nullptr) + (kept_out != nullptr);
    if (given != 0 && given != 4) return h->fail(KEEP_EINVAL, "eval_roc: the four curve outputs go together: all or none");
    if (((uintptr_t)scores & 3) || ((uintptr_t)thresholds_out & 3) || ((uintptr_t)fps_out & 3) || ((uintptr_t)tps_out & 3))
        return h->fail(KEEP_EINVAL, "eval_roc: scores / thresholds_out / fps_out / tps_out not 4-byte aligned");
    KEEP_ON_DEVICE(h);
    int rc = ensure_arena(h, eval_roc_workspace_bytes(N, given == 0));
    if (rc) return rc;
    launch_eval_roc(scores, labels, N, (unsigned char*)h->arena, scalars_out, thresholds_out, fps_out, tps_out, kept_out, (hipStream_t)stream);
    return check_launch(h, "eval_roc");
}

int keep_eval_mask_counts(keep_handle* h, const unsigned char* a, const unsigned char* b, const unsigned char* within, int64_t H, int64_t W,
                          int64_t* counts_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!a || !b) return h->fail(KEEP_EINVAL, "eval_mask_counts: a mask is null");
    if (!pixels_ok(H, W, TISSUE_MAX_PIXELS)) return h->fail(KEEP_EINVAL, "eval_mask_counts: %lldx%lld pixels (1 <= H W <= 2^30)", (long long)H, (long long)W);
    if (!counts_out || ((uintptr_t)counts_out & 7)) return h->fail(KEEP_EINVAL, "eval_mask_counts: counts_out is null or not 8-byte aligned");
    KEEP_ON_DEVICE(h);
    launch_eval_mask_counts(a, b, within, H * W, counts_out, (hipStream_t)stream);
    return check_launch(h, "eval_mask_counts");
}

int keep_eval_raster_hist(keep_handle* h, const int64_t* acc, const unsigned char* truth, const unsigned char* within, int64_t H, int64_t W,
                          int64_t* hist_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!acc || ((uintptr_t)acc & 7)) return h->fail(KEEP_EINVAL, "eval_raster_hist: acc is null or not 8-byte aligned");
    if (!truth) return h->fail(KEEP_EINVAL, "eval_raster_hist: truth is null");
    if (!pixels_ok(H, W, TISSUE_MAX_PIXELS)) return h->fail(KEEP_EINVAL, "eval_raster_hist: %lldx%lld pixels (1 <= H W <= 2^30)", (long long)H, (long long)W);
    if (!hist_out || ((uintptr_t)hist_out & 7)) return h->fail(KEEP_EINVAL, "eval_raster_hist: hist_out is null or not 8-byte aligned");
    KEEP_ON_DEVICE(h);
    launch_eval_raster_hist(acc, truth, within, H * W, hist_out, (hipStream_t)stream);
    return check_launch(h, "eval_raster_hist");
}

// what keep_boot_roc and keep_boot_confusion ask of the sample size, the replicates and the output alike
static int boot_check(keep_handle* h, const char* who, int64_t N, int64_t first_replicate, int64_t B, const int64_t* out) {
    if (N < 0 || N > SORT_MAX) return h->fail(KEEP_EINVAL, "%s: %lld items (0 .. 2^24 - 1)", who, (long long)N);
    if (B < 0 || B > BOOT_MAX_REPLICATES) return h->fail(KEEP_EINVAL, "%s: %lld replicates (0 .. 2^20)", who, (long long)B);
    if (first_replicate < -1) return h->fail(KEEP_EINVAL, "%s: first replicate %lld < -1", who, (long long)first_replicate);
    if (B > 0 && (!out || ((uintptr_t)out & 7))) return h->fail(KEEP_EINVAL, "%s: out is null or not 8-byte aligned", who);
    return KEEP_OK;
}

int keep_boot_roc(keep_handle* h, const float* scores, const unsigned char* labels, int64_t N, uint64_t seed, int64_t first_replicate,
                  int64_t B, int64_t* out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = boot_check(h, "boot_roc", N, first_replicate, B, out)) return rc;
    if (N > 0 && (!scores || !labels)) return h->fail(KEEP_EINVAL, "boot_roc: null scores or labels");
    if ((uintptr_t)scores & 3) return h->fail(KEEP_EINVAL, "boot_roc: scores not 4-byte aligned");
    if (B == 0) return KEEP_OK;
    KEEP_ON_DEVICE(h);
    int rc = ensure_arena(h, boot_roc_workspace_bytes(N, B));
    if (rc) return rc;
    launch_boot_roc(scores, labels, N, (unsigned long long)seed, first_replicate, B, (unsigned char*)h->arena, out, (hipStream_t)stream);
    return check_launch(h, "boot_roc");
}

int keep_boot_confusion(keep_handle* h, const unsigned char* truth, const unsigned char* pred, int64_t N, int64_t C, uint64_t seed,
                        int64_t first_replicate, int64_t B, int64_t* out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = boot_check(h, "boot_confusion", N, first_replicate, B, out)) return rc;
    if (C < 2 || C > BOOT_MAX_CLASSES) return h->fail(KEEP_EINVAL, "boot_confusion: %lld classes (2 .. 16)", (long long)C);
    if (N > 0 && (!truth || !pred)) return h->fail(KEEP_EINVAL, "boot_confusion: null truth or pred");
    if (B == 0) return KEEP_OK;
    KEEP_ON_DEVICE(h);
    int rc = ensure_arena(h, boot_confusion_workspace_bytes(N));
    if (rc) return rc;
    launch_boot_confusion(truth, pred, N, (int)C, (unsigned long long)seed, first_replicate, B, (unsigned char*)h->arena, out, (hipStream_t)stream);
    return check_launch(h, "boot_confusion");
}

}  // extern "C"

// Lesion-level scoring (lesion.hip)
constexpr int LESION_MAX_RADIUS = 1024;                  // g fits a uint16 and (R + 1)^2 a uint32; the LDS row of the row pass is 256 + 2 R entries
constexpr int LESION_MAX_PEAK_RADIUS = 127;
constexpr int64_t LESION_MAX_LABELS = (int64_t)1 << 20;
size_t mask_dist2_workspace_bytes(int64_t npix);
// ws: the uint16 plane of the column pass
void launch_mask_dist2(const unsigned char* mask, int H, int W, int R, int invert, unsigned char* ws, unsigned* out, hipStream_t s);
size_t raster_peaks_workspace_bytes(int64_t npix);
// ws: the 64-bit plane of the row pass, then the blocks' counts and offsets; mask may be null; peaks may be null when max_peaks is 0
void launch_raster_peaks(const int64_t* acc, const unsigned char* mask, int H, int W, int r, int min16, int64_t max_peaks, unsigned char* ws,
                         int64_t* peaks, int64_t* n_out, hipStream_t s);
// lesion_max: n_labels words, zeroed here; ignore may be null
void launch_lesion_hits(const int64_t* xy, const float* scores, int64_t N, const int* labels, int Hm, int Wm, int64_t d, int64_t ox, int64_t oy,
                        int n_labels, const unsigned char* ignore, int* hit, unsigned* lesion_max, hipStream_t s);

extern "C" {

int keep_mask_dist2(keep_handle* h, const unsigned char* mask, int64_t H, int64_t W, int radius, int invert, uint32_t* out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!mask) return h->fail(KEEP_EINVAL, "mask_dist2: mask is null");
    if (!pixels_ok(H, W, TISSUE_MAX_PIXELS)) return h->fail(KEEP_EINVAL, "mask_dist2: %lldx%lld pixels (1 <= H W <= 2^30)", (long long)H, (long long)W);
    if (radius < 1 || radius > LESION_MAX_RADIUS) return h->fail(KEEP_EINVAL, "mask_dist2: radius %d outside [1, %d]", radius, LESION_MAX_RADIUS);
    if (!out || ((uintptr_t)out & 3)) return h->fail(KEEP_EINVAL, "mask_dist2: out is null or not 4-byte aligned");
    KEEP_ON_DEVICE(h);
    int rc = ensure_arena(h, mask_dist2_workspace_bytes(H * W));
    if (rc) return rc;
    launch_mask_dist2(mask, (int)H, (int)W, radius, invert != 0, (unsigned char*)h->arena, out, (hipStream_t)stream);
    return check_launch(h, "mask_dist2");
}

int keep_raster_peaks(keep_handle* h, const int64_t* acc, const unsigned char* mask, int64_t H, int64_t W, int radius, int min16,
                      int64_t max_peaks, int64_t* peaks_out, int64_t* n_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!acc || ((uintptr_t)acc & 7)) return h->fail(KEEP_EINVAL, "raster_peaks: acc is null or not 8-byte aligned");
    if (!pixels_ok(H, W, HEAT_MAX_PIXELS)) return h->fail(KEEP_EINVAL, "raster_peaks: %lldx%lld: raster shape (1 <= H W <= 2^30)", (long long)H, (long long)W);
    if (radius < 1 || radius > LESION_MAX_PEAK_RADIUS) return h->fail(KEEP_EINVAL, "raster_peaks: radius %d outside [1, %d]", radius, LESION_MAX_PEAK_RADIUS);
    if (min16 < 0 || min16 > 65535) return h->fail(KEEP_EINVAL, "raster_peaks: min16 %d outside [0, 65535]", min16);
    if (max_peaks < 0) return h->fail(KEEP_EINVAL, "raster_peaks: max_peaks %lld < 0", (long long)max_peaks);
    if (max_peaks > 0 && (!peaks_out || ((uintptr_t)peaks_out & 7))) return h->fail(KEEP_EINVAL, "raster_peaks: peaks_out is null or not 8-byte aligned");
    if (!n_out || ((uintptr_t)n_out & 7)) return h->fail(KEEP_EINVAL, "raster_peaks: n_out is null or not 8-byte aligned");
    KEEP_ON_DEVICE(h);
    int rc = ensure_arena(h, raster_peaks_workspace_bytes(H * W));
    if (rc) return rc;
    launch_raster_peaks(acc, mask, (int)H, (int)W, radius, min16, max_peaks, (unsigned char*)h->arena, peaks_out, n_out, (hipStream_t)stream);
    return check_launch(h, "raster_peaks");
}

int keep_lesion_hits(keep_handle* h, const int64_t* xy, const float* scores, int64_t N, const int32_t* labels, int64_t Hm, int64_t Wm,
                     int64_t downsample, int64_t origin_x, int64_t origin_y, int64_t n_labels, const unsigned char* ignore, int32_t* hit_out,
                     uint32_t* lesion_max_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (N < 0 || N > HEAT_MAX_TILES) return h->fail(KEEP_EINVAL, "lesion_hits: %lld candidates (0 .. 2^24 - 1)", (long long)N);
    if (N > 0 && (!xy || !scores || !hit_out)) return h->fail(KEEP_EINVAL, "lesion_hits: null xy, scores or hit_out");
    if (((uintptr_t)xy & 7) || ((uintptr_t)scores & 3) || ((uintptr_t)hit_out & 3)) return h->fail(KEEP_EINVAL, "lesion_hits: xy / scores / hit_out not aligned");
    if (!labels || ((uintptr_t)labels & 3)) return h->fail(KEEP_EINVAL, "lesion_hits: labels is null or not 4-byte aligned");
    if (!pixels_ok(Hm, Wm, TISSUE_MAX_PIXELS)) return h->fail(KEEP_EINVAL, "lesion_hits: %lldx%lld pixels (1 <= H W <= 2^30)", (long long)Hm, (long long)Wm);
    if (downsample < 1 || downsample > HEAT_MAX_PATCH) return h->fail(KEEP_EINVAL, "lesion_hits: downsample %lld outside [1, 2^30]", (long long)downsample);
    if (int rc = origin_check(h, "lesion_hits", origin_x, origin_y)) return rc;
    if (n_labels < 0 || n_labels > LESION_MAX_LABELS) return h->fail(KEEP_EINVAL, "lesion_hits: n_labels %lld outside [0, 2^20]", (long long)n_labels);
    if (n_labels > 0 && (!lesion_max_out || ((uintptr_t)lesion_max_out & 3))) return h->fail(KEEP_EINVAL, "lesion_hits: lesion_max_out is null or not 4-byte aligned");
    KEEP_ON_DEVICE(h);
    launch_lesion_hits(xy, scores, N, labels, (int)Hm, (int)Wm, downsample, origin_x, origin_y, (int)n_labels, ignore, hit_out, lesion_max_out,
                       (hipStream_t)stream);
    return check_launch(h, "lesion_hits");
}

}  // extern "C"

// Region shape (shape.hip)
constexpr int64_t FERET_MAX_LATTICE = (int64_t)1 << 31;  // a lattice index y (W + 1) + x fits 32 bits
constexpr int64_t FERET_MAX_PAIRS = (int64_t)1 << 50;
// moments: n x 3 words, zeroed here
void launch_regions_moments(const int* labels, int h, int w, int64_t n, const int64_t* table, int64_t* moments, hipStream_t s);
size_t feret_plan_bytes(int64_t n);
// plan: feret_plan_bytes(n) bytes; -> the three totals on the device: candidates, pairs, workgroups
const int64_t* launch_feret_plan(const int64_t* table, int h, int w, int64_t n, unsigned char* plan, hipStream_t s);
// lines: 2 total_lines ints after the plan
void launch_regions_feret(const int* labels, int h, int w, int64_t n, const int64_t* table, const unsigned char* plan, int* lines,
                          int64_t total_lines, int64_t total_wg, int64_t* feret, hipStream_t s);

extern "C" {

int keep_regions_moments(keep_handle* h, const int32_t* labels, int64_t H, int64_t W, int64_t n, const int64_t* table, int64_t* moments_out,
                         void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!labels || ((uintptr_t)labels & 3)) return h->fail(KEEP_EINVAL, "regions_moments: labels is null or not 4-byte aligned");
    if (!pixels_ok(H, W, TISSUE_MAX_PIXELS)) return h->fail(KEEP_EINVAL, "regions_moments: %lldx%lld pixels (1 <= H W <= 2^30)", (long long)H, (long long)W);
    if (n < 0 || n > H * W) return h->fail(KEEP_EINVAL, "regions_moments: n = %lld outside [0, H W]", (long long)n);
    if (n > 0 && (!table || ((uintptr_t)table & 7))) return h->fail(KEEP_EINVAL, "regions_moments: table is null or not 8-byte aligned");
    if (n > 0 && (!moments_out || ((uintptr_t)moments_out & 7))) return h->fail(KEEP_EINVAL, "regions_moments: moments_out is null or not 8-byte aligned");
    KEEP_ON_DEVICE(h);
    launch_regions_moments(labels, (int)H, (int)W, n, table, moments_out, (hipStream_t)stream);
    return check_launch(h, "regions_moments");
}

int keep_regions_feret(keep_handle* h, const int32_t* labels, int64_t H, int64_t W, int64_t n, const int64_t* table, int64_t max_pairs,
                       int64_t* feret_out, int64_t* totals_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (totals_out) totals_out[0] = totals_out[1] = 0;
    if (!labels || ((uintptr_t)labels & 3)) return h->fail(KEEP_EINVAL, "regions_feret: labels is null or not 4-byte aligned");
    if (!pixels_ok(H, W, TISSUE_MAX_PIXELS) || (H + 1) * (W + 1) > FERET_MAX_LATTICE)
        return h->fail(KEEP_EINVAL, "regions_feret: %lldx%lld pixels (1 <= H W <= 2^30 and (H + 1) (W + 1) <= 2^31)", (long long)H, (long long)W);
    if (n < 0 || n > H * W) return h->fail(KEEP_EINVAL, "regions_feret: n = %lld outside [0, H W]", (long long)n);
    if (max_pairs < 0 || max_pairs > FERET_MAX_PAIRS) return h->fail(KEEP_EINVAL, "regions_feret: max_pairs %lld outside [0, 2^50]", (long long)max_pairs);
    if (n > 0 && (!table || ((uintptr_t)table & 7))) return h->fail(KEEP_EINVAL, "regions_feret: table is null or not 8-byte aligned");
    if (n > 0 && (!feret_out || ((uintptr_t)feret_out & 7))) return h->fail(KEEP_EINVAL, "regions_feret: feret_out is null or not 8-byte aligned");
    if (n == 0) return KEEP_OK;
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    const size_t b_plan = align_up(feret_plan_bytes(n));
    int rc = ensure_arena(h, b_plan);
    if (rc) return rc;
    const int64_t* t_dev = launch_feret_plan(table, (int)H, (int)W, n, (unsigned char*)h->arena, s);
    rc = check_launch(h, "regions_feret (plan)");
    if (rc) return rc;
    int64_t t[3] = {0, 0, 0};
    HIPCHK(h, hipMemcpyAsync(t, t_dev, sizeof t, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));                      // the one host synchronisation: the totals size the workspace and the grid
    if (totals_out) { totals_out[0] = t[0]; totals_out[1] = t[1]; }
    if (t[1] > max_pairs)
        return h->fail(KEEP_EINVAL, "regions_feret: %lld candidates make %lld pairs, max_pairs is %lld", (long long)t[0], (long long)t[1],
                       (long long)max_pairs);
    const char* before = h->arena;
    rc = ensure_arena(h, b_plan + align_up((size_t)t[0] / 2 * sizeof(int)));   // candidates / 4 lines, two ints each
    if (rc) return rc;
    if (h->arena != before) {                                // the arena moved: the plan again, from the same table
        launch_feret_plan(table, (int)H, (int)W, n, (unsigned char*)h->arena, s);
        rc = check_launch(h, "regions_feret (plan)");
        if (rc) return rc;
    }
    launch_regions_feret(labels, (int)H, (int)W, n, table, (const unsigned char*)h->arena, (int*)(h->arena + b_plan), t[0] / 4, t[2], feret_out, s);
    return check_launch(h, "regions_feret");
}

}  // extern "C"

// The subtype map (classmap.hip)
// 1 <= C <= CLASS_MAX, 1 <= H, W and C H W <= 2^30
static bool class_planes_ok(int64_t C, int64_t H, int64_t W) {
    return C >= 1 && C <= CLASS_MAX && pixels_ok(H, W, HEAT_MAX_PIXELS) && C * H * W <= HEAT_MAX_PIXELS;
}

extern "C" {

int keep_heat_accumulate_classes(keep_handle* h, const int64_t* coords, const float* values, int64_t N, int64_t C, int64_t patch,
                                 int64_t downsample, int64_t H, int64_t W, int64_t origin_x, int64_t origin_y, int64_t* acc, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!acc || ((uintptr_t)acc & 7)) return h->fail(KEEP_EINVAL, "heat_accumulate_classes: acc is null or not 8-byte aligned");
    if (N < 0 || N > HEAT_MAX_TILES) return h->fail(KEEP_EINVAL, "heat_accumulate_classes: %lld tiles (0 .. 2^24 - 1)", (long long)N);
    if (N > 0 && (!coords || !values)) return h->fail(KEEP_EINVAL, "heat_accumulate_classes: null coords or values");
    if (((uintptr_t)coords & 7) || ((uintptr_t)values & 3)) return h->fail(KEEP_EINVAL, "heat_accumulate_classes: coords / values not aligned");
    if (!class_planes_ok(C, H, W))
        return h->fail(KEEP_EINVAL, "heat_accumulate_classes: %lld planes of %lldx%lld (1 <= C <= 64, 1 <= C H W <= 2^30)", (long long)C, (long long)H,
                       (long long)W);
    if (patch < 1 || patch > HEAT_MAX_PATCH) return h->fail(KEEP_EINVAL, "heat_accumulate_classes: patch %lld outside [1, 2^30]", (long long)patch);
    if (downsample < 1 || downsample > patch)
        return h->fail(KEEP_EINVAL, "heat_accumulate_classes: downsample %lld outside [1, patch = %lld]", (long long)downsample, (long long)patch);
    if (int rc = origin_check(h, "heat_accumulate_classes", origin_x, origin_y)) return rc;
    if (origin_x % downsample || origin_y % downsample)
        return h->fail(KEEP_EINVAL, "heat_accumulate_classes: origin (%lld, %lld) is not a multiple of downsample %lld", (long long)origin_x,
                       (long long)origin_y, (long long)downsample);
    KEEP_ON_DEVICE(h);
    launch_class_accumulate(coords, values, N, (int)C, patch, downsample, (int)H, (int)W, origin_x, origin_y, acc, (hipStream_t)stream);
    return check_launch(h, "heat_accumulate_classes");
}

int keep_class_argmax(keep_handle* h, const int64_t* acc, int64_t C, int64_t H, int64_t W, const unsigned char* mask, int min16, int margin16,
                      unsigned char* label_out, int64_t* top_out, int64_t* margin_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!acc || ((uintptr_t)acc & 7)) return h->fail(KEEP_EINVAL, "class_argmax: acc is null or not 8-byte aligned");
    if (!class_planes_ok(C, H, W))
        return h->fail(KEEP_EINVAL, "class_argmax: %lld planes of %lldx%lld (1 <= C <= 64, 1 <= C H W <= 2^30)", (long long)C, (long long)H, (long long)W);
    if (min16 < 0 || min16 > 65535 || margin16 < 0 || margin16 > 65535)
        return h->fail(KEEP_EINVAL, "class_argmax: min16 %d / margin16 %d outside [0, 65535]", min16, margin16);
    if (!label_out && !top_out && !margin_out) return h->fail(KEEP_EINVAL, "class_argmax: no output");
    if (((uintptr_t)top_out & 7) || ((uintptr_t)margin_out & 7)) return h->fail(KEEP_EINVAL, "class_argmax: top_out / margin_out not 8-byte aligned");
    KEEP_ON_DEVICE(h);
    launch_class_argmax(acc, (int)C, (int)H, (int)W, mask, min16, margin16, label_out, top_out, margin_out, (hipStream_t)stream);
    return check_launch(h, "class_argmax");
}

int keep_class_confusion(keep_handle* h, const unsigned char* a, const unsigned char* b, const unsigned char* within, int64_t H, int64_t W,
                         int64_t C, int64_t* counts_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!a || !b) return h->fail(KEEP_EINVAL, "class_confusion: a label map is null");
    if (!pixels_ok(H, W, TISSUE_MAX_PIXELS)) return h->fail(KEEP_EINVAL, "class_confusion: %lldx%lld pixels (1 <= H W <= 2^30)", (long long)H, (long long)W);
    if (C < 1 || C > CLASS_MAX) return h->fail(KEEP_EINVAL, "class_confusion: %lld classes (1 .. 64)", (long long)C);
    if (!counts_out || ((uintptr_t)counts_out & 7)) return h->fail(KEEP_EINVAL, "class_confusion: counts_out is null or not 8-byte aligned");
    KEEP_ON_DEVICE(h);
    launch_class_confusion(a, b, within, (int)H, (int)W, (int)C, counts_out, (hipStream_t)stream);
    return check_launch(h, "class_confusion");
}

int keep_class_render(keep_handle* h, const unsigned char* labels, int64_t H, int64_t W, int64_t C, const unsigned char* thumb,
                      int64_t row_stride_bytes, int pix_stride, int background_rgb, const unsigned char* palette, int alpha,
                      const int64_t* strength, int lo16, int hi16, unsigned char* out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!labels || !palette || !out) return h->fail(KEEP_EINVAL, "class_render: null labels, palette or output");
    if (!pixels_ok(H, W, HEAT_MAX_PIXELS)) return h->fail(KEEP_EINVAL, "class_render: %lldx%lld pixels (1 <= H W <= 2^30)", (long long)H, (long long)W);
    if (C < 1 || C > CLASS_MAX) return h->fail(KEEP_EINVAL, "class_render: %lld classes (1 .. 64)", (long long)C);
    if (thumb) {
        if (int rc = pix_stride_check(h, "class_render", pix_stride)) return rc;
        if (int rc = row_stride_check(h, "class_render", W, row_stride_bytes, pix_stride)) return rc;
    } else if (background_rgb < 0 || background_rgb > 0xFFFFFF) {
        return h->fail(KEEP_EINVAL, "class_render: background 0x%x outside [0, 0xFFFFFF]", background_rgb);
    }
    if (alpha < 0 || alpha > 256) return h->fail(KEEP_EINVAL, "class_render: alpha %d outside [0, 256]", alpha);
    if ((uintptr_t)strength & 7) return h->fail(KEEP_EINVAL, "class_render: strength is not 8-byte aligned");
    if (lo16 < 0 || hi16 > 65535 || lo16 >= hi16) return h->fail(KEEP_EINVAL, "class_render: window [%d, %d] (0 <= lo16 < hi16 <= 65535)", lo16, hi16);
    KEEP_ON_DEVICE(h);
    launch_class_render(labels, (int)H, (int)W, (int)C, thumb, row_stride_bytes, pix_stride, (unsigned)background_rgb, palette, alpha, strength, lo16,
                        hi16, out, (hipStream_t)stream);
    return check_launch(h, "class_render");
}

}  // extern "C"

// Tile clustering (cluster.hip)
static int cluster_shape_check(keep_handle* h, const char* who, int64_t N, int64_t D, int64_t K) {
    if (N < 1 || N > CLUSTER_MAX_ROWS) return h->fail(KEEP_EINVAL, "%s: %lld rows (1 .. 2^22 per call)", who, (long long)N);
    if (D < 16 || D > CLUSTER_MAX_D || D % 16) return h->fail(KEEP_EINVAL, "%s: D = %lld (a multiple of 16, 16 .. 1024)", who, (long long)D);
    if (K < 1 || K > CLUSTER_MAX_K) return h->fail(KEEP_EINVAL, "%s: K = %lld (1 .. 64)", who, (long long)K);
    return KEEP_OK;
}

extern "C" {

int keep_cluster_assign(keep_handle* h, const float* features, int64_t N, int64_t D, const float* centroids, int64_t K, int32_t* label_out,
                        float* best_out, float* margin_out, const int32_t* prev_label, int64_t* skipped, int64_t* changed, int64_t* sums,
                        int64_t* counts, int64_t* cos_sum, int two_launch, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = cluster_shape_check(h, "cluster_assign", N, D, K)) return rc;
    if (!features || !centroids) return h->fail(KEEP_EINVAL, "cluster_assign: null features or centroids");
    if (((uintptr_t)features & 15) || ((uintptr_t)centroids & 15)) return h->fail(KEEP_EINVAL, "cluster_assign: features / centroids not 16-byte aligned");
    const int nacc = (sums ? 1 : 0) + (counts ? 1 : 0) + (cos_sum ? 1 : 0);
    if (nacc != 0 && nacc != 3) return h->fail(KEEP_EINVAL, "cluster_assign: sums, counts and cos_sum go together (%d of 3 given)", nacc);
    if (!label_out && !sums) return h->fail(KEEP_EINVAL, "cluster_assign: no output (label_out and the accumulators are both null)");
    if ((changed != nullptr) != (prev_label != nullptr)) return h->fail(KEEP_EINVAL, "cluster_assign: changed and prev_label go together");
    if (two_launch != 0 && two_launch != 1) return h->fail(KEEP_EINVAL, "cluster_assign: two_launch %d (0 or 1)", two_launch);
    if (two_launch && sums && (!label_out || !best_out)) return h->fail(KEEP_EINVAL, "cluster_assign: the two-launch form reads label_out and best_out");
    if (((uintptr_t)label_out & 3) || ((uintptr_t)best_out & 3) || ((uintptr_t)margin_out & 3) || ((uintptr_t)prev_label & 3) ||
        ((uintptr_t)skipped & 7) || ((uintptr_t)changed & 7) || ((uintptr_t)sums & 7) || ((uintptr_t)counts & 7) || ((uintptr_t)cos_sum & 7))
        return h->fail(KEEP_EINVAL, "cluster_assign: an output is not aligned to its element size");
    KEEP_ON_DEVICE(h);
    launch_cluster_assign(features, (int)N, (int)D, centroids, (int)K, label_out, best_out, margin_out, prev_label, skipped, changed, sums, counts,
                          cos_sum, two_launch, (hipStream_t)stream);
    return check_launch(h, "cluster_assign");
}

int keep_cluster_update(keep_handle* h, const int64_t* sums, const int64_t* counts, int64_t K, int64_t D, float* centroids,
                        unsigned char* empty_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = cluster_shape_check(h, "cluster_update", 1, D, K)) return rc;
    if (!sums || !counts || !centroids) return h->fail(KEEP_EINVAL, "cluster_update: null sums, counts or centroids");
    if (((uintptr_t)sums & 7) || ((uintptr_t)counts & 7) || ((uintptr_t)centroids & 3))
        return h->fail(KEEP_EINVAL, "cluster_update: sums / counts / centroids not aligned to their element size");
    KEEP_ON_DEVICE(h);
    launch_cluster_update(sums, counts, (int)K, (int)D, centroids, empty_out, (hipStream_t)stream);
    return check_launch(h, "cluster_update");
}

int keep_cluster_seed_step(keep_handle* h, const float* features, int64_t N, int64_t D, const float* centre, const int64_t* centre_row, int first,
                           float* nearest, int64_t* index_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = cluster_shape_check(h, "cluster_seed_step", N, D, 1)) return rc;
    if (!features || !index_out) return h->fail(KEEP_EINVAL, "cluster_seed_step: null features or index_out");
    if ((centre != nullptr) == (centre_row != nullptr)) return h->fail(KEEP_EINVAL, "cluster_seed_step: give centre or centre_row, one of the two");
    if (first != 0 && first != 1) return h->fail(KEEP_EINVAL, "cluster_seed_step: first %d (0 or 1)", first);
    if (!first && !nearest) return h->fail(KEEP_EINVAL, "cluster_seed_step: null nearest");
    if (((uintptr_t)features & 15) || ((uintptr_t)centre & 15) || ((uintptr_t)centre_row & 7) || ((uintptr_t)nearest & 3) || ((uintptr_t)index_out & 7))
        return h->fail(KEEP_EINVAL, "cluster_seed_step: features / centre (16 bytes), centre_row / index_out (8) or nearest (4) not aligned");
    KEEP_ON_DEVICE(h);
    int rc = ensure_arena(h, 256);
    if (rc) return rc;
    launch_cluster_seed_step(features, (int)N, (int)D, centre, centre_row, first, nearest, (unsigned char*)h->arena, index_out, (hipStream_t)stream);
    return check_launch(h, "cluster_seed_step");
}

}  // extern "C"

// Linear probe (probe.hip)
static int probe_args_check(keep_handle* h, const char* who, const float* features, int64_t N, int64_t D, const float* weight, const float* bias,
                            int64_t C, int groups, bool grad, const float* probs_out, const int32_t* label_out, const float* best_out,
                            const float* margin_out, const int64_t* skipped) {
    if (int rc = cluster_shape_check(h, who, N, D, 1)) return rc;
    if (C < 2 || C > PROBE_MAX_C) return h->fail(KEEP_EINVAL, "%s: C = %lld (2 .. 64)", who, (long long)C);
    if (!features || !weight || !bias) return h->fail(KEEP_EINVAL, "%s: null features, weight or bias", who);
    if (((uintptr_t)features & 15) || ((uintptr_t)weight & 15)) return h->fail(KEEP_EINVAL, "%s: features / weight not 16-byte aligned", who);
    if (groups != 0 && groups != 1 && groups != 2 && groups != 4) return h->fail(KEEP_EINVAL, "%s: groups %d (0 = chosen here, 1, 2 or 4)", who, groups);
    if (grad && groups * ((C + 15) / 16) > PROBE_MAX_GROUP_TILES)
        return h->fail(KEEP_EINVAL, "%s: groups %d with C = %lld (groups x ceil(C / 16) <= %d)", who, groups, (long long)C, PROBE_MAX_GROUP_TILES);
    if (((uintptr_t)bias & 3) || ((uintptr_t)probs_out & 3) || ((uintptr_t)label_out & 3) || ((uintptr_t)best_out & 3) || ((uintptr_t)margin_out & 3) ||
        ((uintptr_t)skipped & 7))
        return h->fail(KEEP_EINVAL, "%s: bias or an output is not aligned to its element size", who);
    return KEEP_OK;
}

extern "C" {

int keep_probe_forward(keep_handle* h, const float* features, int64_t N, int64_t D, const float* weight, const float* bias, int64_t C,
                       float* probs_out, int32_t* label_out, float* best_out, float* margin_out, int64_t* skipped, int groups, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = probe_args_check(h, "probe_forward", features, N, D, weight, bias, C, groups, false, probs_out, label_out, best_out, margin_out,
                                  skipped))
        return rc;
    if (!probs_out && !label_out && !best_out && !margin_out && !skipped) return h->fail(KEEP_EINVAL, "probe_forward: no output (every pointer is null)");
    KEEP_ON_DEVICE(h);
    launch_probe(features, (int)N, (int)D, weight, bias, (int)C, groups, nullptr, nullptr, probs_out, label_out, best_out, margin_out, skipped, nullptr,
                 nullptr, nullptr, nullptr, (hipStream_t)stream);
    return check_launch(h, "probe_forward");
}

int keep_probe_loss_grad(keep_handle* h, const float* features, int64_t N, int64_t D, const int32_t* labels, const float* weight, const float* bias,
                         int64_t C, const float* class_weight, int64_t* grad, int64_t* gbias, int64_t* loss, int64_t* counts, int64_t* skipped,
                         float* probs_out, int32_t* label_out, float* best_out, float* margin_out, int groups, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = probe_args_check(h, "probe_loss_grad", features, N, D, weight, bias, C, groups, true, probs_out, label_out, best_out, margin_out,
                                  skipped))
        return rc;
    if (!labels || ((uintptr_t)labels & 3)) return h->fail(KEEP_EINVAL, "probe_loss_grad: labels is null or not 4-byte aligned");
    if ((uintptr_t)class_weight & 3) return h->fail(KEEP_EINVAL, "probe_loss_grad: class_weight is not 4-byte aligned");
    if (!grad || !gbias || !loss || !counts || !skipped) return h->fail(KEEP_EINVAL, "probe_loss_grad: null grad, gbias, loss, counts or skipped");
    if (((uintptr_t)grad & 7) || ((uintptr_t)gbias & 7) || ((uintptr_t)loss & 7) || ((uintptr_t)counts & 7))
        return h->fail(KEEP_EINVAL, "probe_loss_grad: an accumulator is not 8-byte aligned");
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    // the flag is read back before a label is used (the one synchronisation of this call), as in keep_region_quality
    int rc = ensure_arena(h, align_up(sizeof(int)));
    if (rc) return rc;
    int* bad = (int*)h->arena;
    HIPCHK(h, hipMemsetAsync(bad, 0, sizeof(int), s));
    launch_probe_check(labels, (int)N, (int)C, class_weight, bad, s);
    rc = check_launch(h, "probe_check");
    if (rc) return rc;
    int bad_h = 0;
    HIPCHK(h, hipMemcpyAsync(&bad_h, bad, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (bad_h) return h->fail(KEEP_EINVAL, "probe_loss_grad: a label outside -1 .. %lld or a class weight outside (0, 1]", (long long)(C - 1));
    launch_probe(features, (int)N, (int)D, weight, bias, (int)C, groups, labels, class_weight, probs_out, label_out, best_out, margin_out, skipped, grad,
                 gbias, loss, counts, s);
    return check_launch(h, "probe_loss_grad");
}

// Attention MIL (mil.hip).  The workspace: [flag][mkey S][Z S][P S D][dz S D][u S][ds N], each 256-byte aligned.
struct MilWorkspace {
    size_t o_mkey, o_Z, o_P, o_dz, o_u, o_ds, total;
    MilWorkspace(int64_t N, int64_t D, int64_t S) {
        o_mkey = align_up(sizeof(int));
        o_Z = o_mkey + align_up((size_t)S * 4);
        o_P = o_Z + align_up((size_t)S * 8);
        o_dz = o_P + align_up((size_t)S * D * 8);
        o_u = o_dz + align_up((size_t)S * D * 4);
        o_ds = o_u + align_up((size_t)S * 4);
        total = o_ds + align_up((size_t)N * 4);
    }
};

static int mil_args_check(keep_handle* h, const char* who, const float* features, int64_t N, int64_t D, const int32_t* chunks, int64_t n_chunks,
                          int64_t S, int64_t L, const void* workspace, int64_t workspace_bytes) {
    if (int rc = cluster_shape_check(h, who, N, D, 1)) return rc;
    if (S < 1 || S > MIL_MAX_BAGS) return h->fail(KEEP_EINVAL, "%s: %lld bags (1 .. 2^16 per call)", who, (long long)S);
    if (L < 16 || L > MIL_MAX_L || L % 16) return h->fail(KEEP_EINVAL, "%s: L = %lld (a multiple of 16, 16 .. 128)", who, (long long)L);
    if (n_chunks < 0 || n_chunks > N) return h->fail(KEEP_EINVAL, "%s: %lld chunks for %lld rows", who, (long long)n_chunks, (long long)N);
    if (!features || ((uintptr_t)features & 15)) return h->fail(KEEP_EINVAL, "%s: features null or not 16-byte aligned", who);
    if (n_chunks > 0 && (!chunks || ((uintptr_t)chunks & 3))) return h->fail(KEEP_EINVAL, "%s: the chunk table is null or not 4-byte aligned", who);
    if (!workspace || ((uintptr_t)workspace & 255) || workspace_bytes < (int64_t)MilWorkspace(N, D, S).total)
        return h->fail(KEEP_EINVAL, "%s: workspace null, not 256-byte aligned or of %lld bytes, %lld needed (keep_mil_workspace_bytes)", who,
                       (long long)workspace_bytes, (long long)MilWorkspace(N, D, S).total);
    return KEEP_OK;
}

// the chunk table is read back as one flag before it is an index (the one synchronisation of the call), as in keep_probe_loss_grad
static int mil_chunks_check(keep_handle* h, const char* who, const int32_t* chunks, int64_t n_chunks, int64_t N, int64_t S, char* ws, hipStream_t s) {
    if (n_chunks == 0) return KEEP_OK;
    int* bad = (int*)ws;
    HIPCHK(h, hipMemsetAsync(bad, 0, sizeof(int), s));
    launch_mil_check(chunks, (int)n_chunks, (int)N, (int)S, bad, s);
    if (int rc = check_launch(h, "mil_check")) return rc;
    int bad_h = 0;
    HIPCHK(h, hipMemcpyAsync(&bad_h, bad, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (bad_h) return h->fail(KEEP_EINVAL, "%s: a chunk leaves [0, %lld) bags or [0, %lld) rows, or has rows outside 1 .. %d", who, (long long)S,
                              (long long)N, KEEP_MIL_CHUNK);
    return KEEP_OK;
}

int keep_mil_chunk(void) { return KEEP_MIL_CHUNK; }

int keep_mil_workspace_bytes(keep_handle* h, int64_t N, int64_t D, int64_t S, int64_t* bytes) {
    if (!h) return KEEP_EINVAL;
    if (!bytes) return h->fail(KEEP_EINVAL, "mil_workspace_bytes: null pointer");
    if (int rc = cluster_shape_check(h, "mil_workspace_bytes", N, D, 1)) return rc;
    if (S < 1 || S > MIL_MAX_BAGS) return h->fail(KEEP_EINVAL, "mil_workspace_bytes: %lld bags (1 .. 2^16 per call)", (long long)S);
    *bytes = (int64_t)MilWorkspace(N, D, S).total;
    return KEEP_OK;
}

int keep_mil_forward(keep_handle* h, const float* features, int64_t N, int64_t D, const int32_t* chunks, int64_t n_chunks, int64_t S,
                     const int32_t* labels, const float* V, const float* bv, const float* w, int64_t L, float* scores_out, float* attn_out,
                     float* pooled_out, int32_t* kept_rows_out, float* hidden_out, int32_t* head_labels_out, int64_t* skipped_rows,
                     int64_t* skipped_bags, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = mil_args_check(h, "mil_forward", features, N, D, chunks, n_chunks, S, L, workspace, workspace_bytes)) return rc;
    if (!V || !bv || !w || ((uintptr_t)V & 15) || ((uintptr_t)bv & 3) || ((uintptr_t)w & 3))
        return h->fail(KEEP_EINVAL, "mil_forward: null V, bv or w, or V not 16-byte aligned");
    if (!scores_out || !attn_out || !pooled_out || !kept_rows_out || !skipped_rows || !skipped_bags)
        return h->fail(KEEP_EINVAL, "mil_forward: null scores_out, attn_out, pooled_out, kept_rows_out, skipped_rows or skipped_bags");
    if (((uintptr_t)scores_out & 3) || ((uintptr_t)attn_out & 3) || ((uintptr_t)pooled_out & 3) || ((uintptr_t)kept_rows_out & 3) ||
        ((uintptr_t)hidden_out & 3) || ((uintptr_t)head_labels_out & 3) || ((uintptr_t)labels & 3) || ((uintptr_t)skipped_rows & 7) ||
        ((uintptr_t)skipped_bags & 7))
        return h->fail(KEEP_EINVAL, "mil_forward: labels or an output is not aligned to its element size");
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const MilWorkspace m(N, D, S);
    if (int rc = mil_chunks_check(h, "mil_forward", chunks, n_chunks, N, S, ws, s)) return rc;
    launch_mil_scores(features, (int)N, (int)D, V, bv, w, (int)L, scores_out, hidden_out, skipped_rows, s);
    if (int rc = check_launch(h, "mil_scores")) return rc;
    launch_mil_pool(features, (int)N, (int)D, scores_out, chunks, (int)n_chunks, (int)S, labels, (int*)(ws + m.o_mkey), (int64_t*)(ws + m.o_Z),
                    (int64_t*)(ws + m.o_P), attn_out, pooled_out, kept_rows_out, head_labels_out, skipped_bags, s);
    return check_launch(h, "mil_pool");
}

int keep_mil_backward(keep_handle* h, const float* features, int64_t N, int64_t D, const int32_t* chunks, int64_t n_chunks, int64_t S,
                      const int32_t* head_labels, const float* probs, const float* Wc, int64_t C, const float* class_weight, const float* w,
                      int64_t L, const float* scores, const float* attn, const float* pooled, const float* hidden, int64_t* gV, int64_t* gbv,
                      int64_t* gw, float* ds_out, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = mil_args_check(h, "mil_backward", features, N, D, chunks, n_chunks, S, L, workspace, workspace_bytes)) return rc;
    if (C < 2 || C > PROBE_MAX_C) return h->fail(KEEP_EINVAL, "mil_backward: C = %lld (2 .. 64)", (long long)C);
    if (!head_labels || !probs || !Wc || !w || !scores || !attn || !pooled || !hidden)
        return h->fail(KEEP_EINVAL, "mil_backward: null head_labels, probs, Wc, w, scores, attn, pooled or hidden");
    if (!gV || !gbv || !gw) return h->fail(KEEP_EINVAL, "mil_backward: null gV, gbv or gw");
    if (((uintptr_t)gV & 7) || ((uintptr_t)gbv & 7) || ((uintptr_t)gw & 7)) return h->fail(KEEP_EINVAL, "mil_backward: an accumulator is not 8-byte aligned");
    if (((uintptr_t)head_labels & 3) || ((uintptr_t)probs & 3) || ((uintptr_t)Wc & 3) || ((uintptr_t)class_weight & 3) || ((uintptr_t)w & 3) ||
        ((uintptr_t)scores & 3) || ((uintptr_t)attn & 3) || ((uintptr_t)pooled & 3) || ((uintptr_t)hidden & 3) || ((uintptr_t)ds_out & 3))
        return h->fail(KEEP_EINVAL, "mil_backward: an input or ds_out is not 4-byte aligned");
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const MilWorkspace m(N, D, S);
    if (int rc = mil_chunks_check(h, "mil_backward", chunks, n_chunks, N, S, ws, s)) return rc;
    launch_mil_backward(features, (int)D, chunks, (int)n_chunks, (int)S, head_labels, probs, Wc, (int)C, class_weight, w, (int)L, scores, attn, pooled,
                        hidden, (float*)(ws + m.o_dz), (float*)(ws + m.o_u), ds_out ? ds_out : (float*)(ws + m.o_ds), gV, gbv, gw, s);
    return check_launch(h, "mil_backward");
}

// Nearest neighbours (neighbours.hip)
static int topk_list_check(keep_handle* h, const char* who, int64_t Nq, int k) {
    if (Nq < 1 || Nq > CLUSTER_MAX_ROWS) return h->fail(KEEP_EINVAL, "%s: %lld query rows (1 .. 2^22 per call)", who, (long long)Nq);
    if (k < 1 || k > TOPK_MAX_K) return h->fail(KEEP_EINVAL, "%s: k = %d (1 .. %d)", who, k, TOPK_MAX_K);
    return KEEP_OK;
}

int keep_topk(keep_handle* h, const float* queries, int64_t Nq, const float* bank, int64_t M, int64_t D, int k, int64_t bank_base,
              int64_t self_first, int merge, uint64_t* keys, int64_t* query_skipped, int64_t* bank_skipped, int segments, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = topk_list_check(h, "topk", Nq, k)) return rc;
    if (int rc = cluster_shape_check(h, "topk", M, D, 1)) return rc;
    if (!queries || !bank || !keys) return h->fail(KEEP_EINVAL, "topk: null queries, bank or keys");
    if (((uintptr_t)queries & 15) || ((uintptr_t)bank & 15)) return h->fail(KEEP_EINVAL, "topk: queries / bank not 16-byte aligned");
    if (((uintptr_t)keys & 7) || ((uintptr_t)query_skipped & 7) || ((uintptr_t)bank_skipped & 7))
        return h->fail(KEEP_EINVAL, "topk: keys or a counter is not 8-byte aligned");
    if (bank_base < 0 || bank_base + M > (int64_t)0xFFFFFFFFll)
        return h->fail(KEEP_EINVAL, "topk: bank_base %lld with %lld rows (0 <= bank_base, bank_base + M <= 2^32 - 1)", (long long)bank_base, (long long)M);
    if (self_first > (int64_t)0xFFFFFFFFll) return h->fail(KEEP_EINVAL, "topk: self_first %lld (a global row index, or negative)", (long long)self_first);
    if (merge != 0 && merge != 1) return h->fail(KEEP_EINVAL, "topk: merge %d (0 or 1)", merge);
    if (segments < 0 || segments > TOPK_MAX_SEGMENTS) return h->fail(KEEP_EINVAL, "topk: segments %d (0 = chosen here, 1 .. %d)", segments, TOPK_MAX_SEGMENTS);
    KEEP_ON_DEVICE(h);
    int S = segments;
    if (S == 0) {
        int cus = 0;
        HIPCHK(h, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
        S = topk_segments((int)Nq, (int)M, cus);
    }
    uint64_t* ws = nullptr;
    if (S > 1) {
        const size_t bytes = (size_t)S * (size_t)((Nq + 63) / 64 * 64) * (size_t)k * sizeof(uint64_t);
        if (int rc = ensure_arena(h, align_up(bytes))) return rc;
        ws = (uint64_t*)h->arena;
    }
    launch_topk(queries, (int)Nq, bank, (int)M, (int)D, k, (unsigned)bank_base, self_first < 0 ? -1 : (long long)self_first, merge, keys, query_skipped,
                bank_skipped, S, ws, (hipStream_t)stream);
    return check_launch(h, "topk");
}

int keep_topk_merge(keep_handle* h, const uint64_t* a, const uint64_t* b, int64_t Nq, int k, uint64_t* out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = topk_list_check(h, "topk_merge", Nq, k)) return rc;
    if (!a || !b || !out) return h->fail(KEEP_EINVAL, "topk_merge: null a, b or out");
    if (((uintptr_t)a & 7) || ((uintptr_t)b & 7) || ((uintptr_t)out & 7)) return h->fail(KEEP_EINVAL, "topk_merge: a list is not 8-byte aligned");
    if (out == b && a != b) return h->fail(KEEP_EINVAL, "topk_merge: out may be a, not b");
    KEEP_ON_DEVICE(h);
    launch_topk_merge(a, b, (int)Nq, k, out, (hipStream_t)stream);
    return check_launch(h, "topk_merge");
}

int keep_topk_unpack(keep_handle* h, const uint64_t* keys, int64_t Nq, int k, int64_t* index_out, float* score_out, int32_t* count_out,
                     void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = topk_list_check(h, "topk_unpack", Nq, k)) return rc;
    if (!keys || ((uintptr_t)keys & 7)) return h->fail(KEEP_EINVAL, "topk_unpack: keys is null or not 8-byte aligned");
    if (!index_out && !score_out && !count_out) return h->fail(KEEP_EINVAL, "topk_unpack: no output (every pointer is null)");
    if (((uintptr_t)index_out & 7) || ((uintptr_t)score_out & 3) || ((uintptr_t)count_out & 3))
        return h->fail(KEEP_EINVAL, "topk_unpack: an output is not aligned to its element size");
    KEEP_ON_DEVICE(h);
    launch_topk_unpack(keys, (int)Nq, k, index_out, score_out, count_out, (hipStream_t)stream);
    return check_launch(h, "topk_unpack");
}

int keep_knn_vote(keep_handle* h, const uint64_t* keys, int64_t Nq, int k, const int32_t* bank_labels, int64_t n_bank, int64_t C, int mode,
                  float temperature, float* probs_out, int32_t* label_out, float* margin_out, int64_t* skipped, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = topk_list_check(h, "knn_vote", Nq, k)) return rc;
    if (!keys || ((uintptr_t)keys & 7)) return h->fail(KEEP_EINVAL, "knn_vote: keys is null or not 8-byte aligned");
    if (!bank_labels || ((uintptr_t)bank_labels & 3)) return h->fail(KEEP_EINVAL, "knn_vote: bank_labels is null or not 4-byte aligned");
    if (n_bank < 1 || n_bank > (int64_t)0xFFFFFFFFll) return h->fail(KEEP_EINVAL, "knn_vote: n_bank %lld (1 .. 2^32 - 1)", (long long)n_bank);
    if (C < 2 || C > PROBE_MAX_C) return h->fail(KEEP_EINVAL, "knn_vote: C = %lld (2 .. 64)", (long long)C);
    if (mode != KEEP_KNN_UNIFORM && mode != KEEP_KNN_SOFTMAX) return h->fail(KEEP_EINVAL, "knn_vote: mode %d (0 uniform, 1 softmax)", mode);
    if (mode == KEEP_KNN_SOFTMAX && !(temperature > 0.f && temperature <= 3.0e38f))
        return h->fail(KEEP_EINVAL, "knn_vote: temperature %g (finite and > 0)", (double)temperature);
    if (!probs_out && !label_out && !margin_out && !skipped) return h->fail(KEEP_EINVAL, "knn_vote: no output (every pointer is null)");
    if (((uintptr_t)probs_out & 3) || ((uintptr_t)label_out & 3) || ((uintptr_t)margin_out & 3) || ((uintptr_t)skipped & 7))
        return h->fail(KEEP_EINVAL, "knn_vote: an output is not aligned to its element size");
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    // the flag is read back before a label is read (the one synchronisation of this call), as in keep_probe_loss_grad
    int rc = ensure_arena(h, align_up(sizeof(int)));
    if (rc) return rc;
    int* bad = (int*)h->arena;
    HIPCHK(h, hipMemsetAsync(bad, 0, sizeof(int), s));
    launch_knn_check(keys, (int)Nq, k, n_bank, bad, s);
    rc = check_launch(h, "knn_check");
    if (rc) return rc;
    int bad_h = 0;
    HIPCHK(h, hipMemcpyAsync(&bad_h, bad, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (bad_h) return h->fail(KEEP_EINVAL, "knn_vote: a key names bank row >= n_bank = %lld", (long long)n_bank);
    launch_knn_vote(keys, (int)Nq, k, bank_labels, (int)C, mode, temperature, probs_out, label_out, margin_out, skipped, s);
    return check_launch(h, "knn_vote");
}

// Few-shot prototypes (fewshot.hip)
static int fewshot_shape_check(keep_handle* h, const char* who, int64_t E, int64_t C) {
    if (C < 2 || C > FEWSHOT_MAX_C) return h->fail(KEEP_EINVAL, "%s: C = %lld (2 .. 63)", who, (long long)C);
    if (E < 1 || E > FEWSHOT_MAX_EPISODES) return h->fail(KEEP_EINVAL, "%s: %lld episodes (1 .. 2^16 per call)", who, (long long)E);
    return KEEP_OK;
}

int keep_fewshot_sample(keep_handle* h, const int32_t* class_rows, const int64_t* class_offsets, int64_t C, int64_t shots, uint64_t seed,
                        int64_t first_episode, int64_t E, int32_t* support_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = fewshot_shape_check(h, "fewshot_sample", E, C)) return rc;
    if (shots < 1 || shots > KEEP_FEWSHOT_MAX_SHOTS) return h->fail(KEEP_EINVAL, "fewshot_sample: shots = %lld (1 .. 256)", (long long)shots);
    if (first_episode < 0 || first_episode > ((int64_t)1 << 40))
        return h->fail(KEEP_EINVAL, "fewshot_sample: first_episode %lld (0 .. 2^40)", (long long)first_episode);
    if (!class_rows || !class_offsets || !support_out) return h->fail(KEEP_EINVAL, "fewshot_sample: null class_rows, class_offsets or support_out");
    if (((uintptr_t)class_rows & 3) || ((uintptr_t)class_offsets & 7) || ((uintptr_t)support_out & 3))
        return h->fail(KEEP_EINVAL, "fewshot_sample: a pointer is not aligned to its element size");
    KEEP_ON_DEVICE(h);
    launch_fewshot_sample(class_rows, class_offsets, (int)C, (int)shots, seed, first_episode, (int)E, support_out, (hipStream_t)stream);
    return check_launch(h, "fewshot_sample");
}

int keep_fewshot_prototypes(keep_handle* h, const float* train, int64_t M, int64_t D, const int32_t* support, int64_t E, int64_t C,
                            int64_t shots, int centre, float* bank_out, float* consts_out, unsigned char* valid_out,
                            int64_t* support_skipped, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = fewshot_shape_check(h, "fewshot_prototypes", E, C)) return rc;
    if (int rc = cluster_shape_check(h, "fewshot_prototypes", M, D, 1)) return rc;
    if (shots < 1 || shots > CLUSTER_MAX_ROWS) return h->fail(KEEP_EINVAL, "fewshot_prototypes: shots = %lld (1 .. 2^22)", (long long)shots);
    if (E * C * shots > ((int64_t)1 << 31) - 1) return h->fail(KEEP_EINVAL, "fewshot_prototypes: E C shots = %lld slots (below 2^31)", (long long)(E * C * shots));
    if (centre != 0 && centre != 1) return h->fail(KEEP_EINVAL, "fewshot_prototypes: centre %d (0 or 1)", centre);
    if (!train || !support || !bank_out || !consts_out || !valid_out)
        return h->fail(KEEP_EINVAL, "fewshot_prototypes: null train, support, bank_out, consts_out or valid_out");
    if (((uintptr_t)train & 15) || ((uintptr_t)bank_out & 15)) return h->fail(KEEP_EINVAL, "fewshot_prototypes: train / bank_out not 16-byte aligned");
    if (((uintptr_t)support & 3) || ((uintptr_t)consts_out & 3) || ((uintptr_t)support_skipped & 7))
        return h->fail(KEEP_EINVAL, "fewshot_prototypes: a pointer is not aligned to its element size");
    KEEP_ON_DEVICE(h);
    launch_fewshot_prototypes(train, (int)M, (int)D, support, (int)E, (int)C, (int)shots, centre, bank_out, consts_out, valid_out, support_skipped,
                              (hipStream_t)stream);
    return check_launch(h, "fewshot_prototypes");
}

int keep_fewshot_classify(keep_handle* h, const float* feats, int64_t N, int64_t D, const float* bank, const float* consts,
                          const unsigned char* valid, int64_t E, int64_t C, const int32_t* truth, int64_t* confusion, int32_t* labels_out,
                          float* scores_out, float* margin_out, float* dots_out, int64_t* skipped, int segments, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = fewshot_shape_check(h, "fewshot_classify", E, C)) return rc;
    if (int rc = cluster_shape_check(h, "fewshot_classify", N, D, 1)) return rc;
    if (!feats || !bank || !consts || !valid) return h->fail(KEEP_EINVAL, "fewshot_classify: null feats, bank, consts or valid");
    if (((uintptr_t)feats & 15) || ((uintptr_t)bank & 15)) return h->fail(KEEP_EINVAL, "fewshot_classify: feats / bank not 16-byte aligned");
    if ((truth != nullptr) != (confusion != nullptr)) return h->fail(KEEP_EINVAL, "fewshot_classify: truth and confusion go together");
    if (E != 1 && (scores_out || margin_out || dots_out))
        return h->fail(KEEP_EINVAL, "fewshot_classify: scores_out, margin_out and dots_out take one episode, E = %lld", (long long)E);
    if (!confusion && !labels_out && !scores_out && !margin_out && !dots_out) return h->fail(KEEP_EINVAL, "fewshot_classify: no output (every pointer is null)");
    if (N * E > ((int64_t)1 << 40)) return h->fail(KEEP_EINVAL, "fewshot_classify: N E = %lld pairs (at most 2^40)", (long long)(N * E));
    if (((uintptr_t)consts & 3) || ((uintptr_t)truth & 3) || ((uintptr_t)confusion & 7) || ((uintptr_t)labels_out & 3) || ((uintptr_t)scores_out & 3) ||
        ((uintptr_t)margin_out & 3) || ((uintptr_t)dots_out & 3) || ((uintptr_t)skipped & 7))
        return h->fail(KEEP_EINVAL, "fewshot_classify: a pointer is not aligned to its element size");
    if (segments < 0 || segments > TOPK_MAX_SEGMENTS)
        return h->fail(KEEP_EINVAL, "fewshot_classify: segments %d (0 = chosen here, 1 .. %d)", segments, TOPK_MAX_SEGMENTS);
    KEEP_ON_DEVICE(h);
    int S = segments;
    if (S == 0) {
        int cus = 0;
        HIPCHK(h, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
        S = fewshot_segments((int)N, (int)E, (int)C, cus);
    }
    launch_fewshot_classify(feats, (int)N, (int)D, bank, consts, valid, (int)E, (int)C, truth, confusion, labels_out, scores_out, margin_out, dots_out,
                            skipped, S, (hipStream_t)stream);
    return check_launch(h, "fewshot_classify");
}

// the image, mask and od table that the three fit passes of the stain normalisation share
static int stain_view_check(keep_handle* h, const char* who, const unsigned char* image, int64_t H, int64_t W, int64_t row_stride_bytes,
                            int pix_stride, const unsigned char* mask, int64_t mh, int64_t mw, int64_t downsample, const int32_t* od_q) {
    if (!image || H < 1 || W < 1) return h->fail(KEEP_EINVAL, "%s: null pointer or empty shape %lldx%lld", who, (long long)H, (long long)W);
    if (int rc = pix_stride_check(h, who, pix_stride)) return rc;
    if (!pixels_ok(H, W, TISSUE_MAX_PIXELS)) return h->fail(KEEP_EINVAL, "%s: %lldx%lld pixels (limit H W <= 2^30)", who, (long long)H, (long long)W);
    if (int rc = row_stride_check(h, who, W, row_stride_bytes, pix_stride)) return rc;
    if (mask && (mh < 1 || mw < 1 || mh > INT32_MAX || mw > INT32_MAX))
        return h->fail(KEEP_EINVAL, "%s: bad mask shape %lldx%lld", who, (long long)mh, (long long)mw);
    if (mask && (downsample < 1 || downsample > INT32_MAX)) return h->fail(KEEP_EINVAL, "%s: downsample %lld < 1", who, (long long)downsample);
    if (!od_q || ((uintptr_t)od_q & 3)) return h->fail(KEEP_EINVAL, "%s: null or unaligned od_q", who);
    return KEEP_OK;
}

int keep_stain_moments(keep_handle* h, const unsigned char* image, int64_t H, int64_t W, int64_t row_stride_bytes, int pix_stride,
                       const unsigned char* mask, int64_t mh, int64_t mw, int64_t downsample, const int32_t* od_q, int beta_q, int zero_first,
                       int64_t* moments_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = stain_view_check(h, "stain_moments", image, H, W, row_stride_bytes, pix_stride, mask, mh, mw, downsample, od_q)) return rc;
    if (!moments_out || ((uintptr_t)moments_out & 7)) return h->fail(KEEP_EINVAL, "stain_moments: null or unaligned moments_out");
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    if (zero_first) HIPCHK(h, hipMemsetAsync(moments_out, 0, STAIN_MOMENTS * sizeof(int64_t), s));
    launch_stain_moments(image, row_stride_bytes, pix_stride, (int)H, (int)W, mask, mh, mw, mask ? downsample : 1, od_q, beta_q, moments_out, s);
    return check_launch(h, "stain_moments");
}

int keep_stain_angle_hist(keep_handle* h, const unsigned char* image, int64_t H, int64_t W, int64_t row_stride_bytes, int pix_stride,
                          const unsigned char* mask, int64_t mh, int64_t mw, int64_t downsample, const int32_t* od_q, int beta_q,
                          const int32_t* v_q, const int32_t* dirs, int zero_first, int32_t* hist_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = stain_view_check(h, "stain_angle_hist", image, H, W, row_stride_bytes, pix_stride, mask, mh, mw, downsample, od_q)) return rc;
    if (!v_q || !dirs || ((uintptr_t)dirs & 7) || !hist_out || ((uintptr_t)hist_out & 3))
        return h->fail(KEEP_EINVAL, "stain_angle_hist: null v_q, dirs or hist_out, or dirs / hist_out unaligned");
    for (int i = 0; i < 6; ++i)
        if (v_q[i] < -(1 << 14) || v_q[i] > (1 << 14)) return h->fail(KEEP_EINVAL, "stain_angle_hist: v_q[%d] = %d outside +-2^14", i, v_q[i]);
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    if (zero_first) HIPCHK(h, hipMemsetAsync(hist_out, 0, STAIN_ANGLE_BINS * sizeof(int32_t), s));
    launch_stain_angle_hist(image, row_stride_bytes, pix_stride, (int)H, (int)W, mask, mh, mw, mask ? downsample : 1, od_q, beta_q, v_q, dirs,
                            hist_out, s);
    return check_launch(h, "stain_angle_hist");
}

int keep_stain_conc_hist(keep_handle* h, const unsigned char* image, int64_t H, int64_t W, int64_t row_stride_bytes, int pix_stride,
                         const unsigned char* mask, int64_t mh, int64_t mw, int64_t downsample, const int32_t* od_q, const int32_t* minv_q,
                         int zero_first, int32_t* hist_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = stain_view_check(h, "stain_conc_hist", image, H, W, row_stride_bytes, pix_stride, mask, mh, mw, downsample, od_q)) return rc;
    if (!minv_q || !hist_out || ((uintptr_t)hist_out & 3)) return h->fail(KEEP_EINVAL, "stain_conc_hist: null minv_q or hist_out, or hist_out unaligned");
    for (int i = 0; i < 6; ++i)
        if (minv_q[i] < -(1 << 24) || minv_q[i] > (1 << 24))
            return h->fail(KEEP_EINVAL, "stain_conc_hist: minv_q[%d] = %d outside +-2^24", i, minv_q[i]);
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    if (zero_first) HIPCHK(h, hipMemsetAsync(hist_out, 0, 2 * STAIN_CONC_BINS * sizeof(int32_t), s));
    launch_stain_conc_hist(image, row_stride_bytes, pix_stride, (int)H, (int)W, mask, mh, mw, mask ? downsample : 1, od_q, minv_q, hist_out, s);
    return check_launch(h, "stain_conc_hist");
}

int keep_stain_apply_u8(keep_handle* h, const unsigned char* src, int64_t n, const int32_t* od_q, const int32_t* t_q,
                        const unsigned char* exp_lut, int lut_len, int lo, unsigned char* dst, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (n < 0 || n > ((int64_t)1 << 40) || (n > 0 && (!src || !dst))) return h->fail(KEEP_EINVAL, "stain_apply_u8: bad n %lld or null pointer", (long long)n);
    if (!od_q || ((uintptr_t)od_q & 3) || !t_q || !exp_lut || ((uintptr_t)exp_lut & 3))
        return h->fail(KEEP_EINVAL, "stain_apply_u8: null t_q, or od_q / exp_lut null or not 4-byte aligned");
    if (lut_len < 1 || lut_len > STAIN_LUT_MAX) return h->fail(KEEP_EINVAL, "stain_apply_u8: lut_len %d outside [1, %d]", lut_len, STAIN_LUT_MAX);
    if (lo < -(1 << 24) || lo > (1 << 24)) return h->fail(KEEP_EINVAL, "stain_apply_u8: lo %d outside +-2^24", lo);
    for (int i = 0; i < 9; ++i)
        if (t_q[i] < -STAIN_T_MAX || t_q[i] > STAIN_T_MAX)
            return h->fail(KEEP_EINVAL, "stain_apply_u8: t_q[%d] = %d: |T| > 64", i, t_q[i]);
    if (src != dst && src < dst + 3 * n && dst < src + 3 * n) return h->fail(KEEP_EINVAL, "stain_apply_u8: src and dst overlap without being equal");
    if (n == 0) return KEEP_OK;
    KEEP_ON_DEVICE(h);
    launch_stain_apply_u8(src, dst, n, od_q, t_q, exp_lut, lut_len, lo, (hipStream_t)stream);
    return check_launch(h, "stain_apply_u8");
}

int keep_region_quality(keep_handle* h, const unsigned char* region, int64_t H, int64_t W, int pix_stride, int64_t row_stride_bytes,
                        const int32_t* cell_xy, int64_t N, int64_t patch, const int32_t* rules, int zero_first, int64_t* out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!region || H < 1 || W < 1 || H > INT32_MAX || W > INT32_MAX)
        return h->fail(KEEP_EINVAL, "region_quality: null region or bad shape %lldx%lld", (long long)H, (long long)W);
    if (int rc = pix_stride_check(h, "region_quality", pix_stride)) return rc;
    if (int rc = row_stride_check(h, "region_quality", W, row_stride_bytes, pix_stride)) return rc;
    if (patch < 1 || patch > QUAL_MAX_PATCH) return h->fail(KEEP_EINVAL, "region_quality: patch %lld outside [1, %d]", (long long)patch, QUAL_MAX_PATCH);
    if (patch > H || patch > W)
        return h->fail(KEEP_EINVAL, "region_quality: patch %lld larger than the region %lldx%lld", (long long)patch, (long long)W, (long long)H);
    if (N < 0 || N > QUAL_MAX_CELLS) return h->fail(KEEP_EINVAL, "region_quality: %lld cells (0 .. 2^24 - 1)", (long long)N);
    if (N > 0 && (!cell_xy || ((uintptr_t)cell_xy & 3))) return h->fail(KEEP_EINVAL, "region_quality: cell_xy is null or not 4-byte aligned");
    if (N > 0 && (!out || ((uintptr_t)out & 7))) return h->fail(KEEP_EINVAL, "region_quality: out is null or not 8-byte aligned");
    if (!rules || ((uintptr_t)rules & 3)) return h->fail(KEEP_EINVAL, "region_quality: rules is null or not 4-byte aligned");
    if (N == 0) return KEEP_OK;
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    // the flag is read back before any pixel is touched (the one synchronisation of this call), as in keep_region_patches_u8
    int rc = ensure_arena(h, align_up(sizeof(int)));
    if (rc) return rc;
    int* bad = (int*)h->arena;
    HIPCHK(h, hipMemsetAsync(bad, 0, sizeof(int), s));
    launch_region_check_cells(cell_xy, (int)N, H, W, (int)patch, bad, s);
    rc = check_launch(h, "region_check_cells");
    if (rc) return rc;
    int bad_h = 0;
    HIPCHK(h, hipMemcpyAsync(&bad_h, bad, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (bad_h) return h->fail(KEEP_EINVAL, "region_quality: a cell (x, y) has x < 0, y < 0, x + %lld > %lld or y + %lld > %lld", (long long)patch,
                              (long long)W, (long long)patch, (long long)H);
    if (zero_first) HIPCHK(h, hipMemsetAsync(out, 0, (size_t)N * QUAL_COLS * sizeof(int64_t), s));
    if (launch_region_quality(region, row_stride_bytes, pix_stride, cell_xy, N, (int)patch, rules, out, s))
        return h->fail(KEEP_EUNSUPPORTED, "region_quality: no launch plan for patch %lld", (long long)patch);
    return check_launch(h, "region_quality");
}

int keep_pen_mask(keep_handle* h, const unsigned char* thumb, int64_t H, int64_t W, int pix_stride, int64_t row_stride_bytes,
                  const int32_t* rules, unsigned char* out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!thumb || H < 1 || W < 1) return h->fail(KEEP_EINVAL, "pen_mask: null pointer or empty shape %lldx%lld", (long long)H, (long long)W);
    if (int rc = pix_stride_check(h, "pen_mask", pix_stride)) return rc;
    if (!pixels_ok(H, W, TISSUE_MAX_PIXELS)) return h->fail(KEEP_EINVAL, "pen_mask: %lldx%lld pixels (limit H W <= 2^30)", (long long)H, (long long)W);
    if (int rc = row_stride_check(h, "pen_mask", W, row_stride_bytes, pix_stride)) return rc;
    if (!rules || ((uintptr_t)rules & 3)) return h->fail(KEEP_EINVAL, "pen_mask: rules is null or not 4-byte aligned");
    if (!out) return h->fail(KEEP_EINVAL, "pen_mask: out is null");
    KEEP_ON_DEVICE(h);
    launch_pen_mask(thumb, row_stride_bytes, pix_stride, (int)H, (int)W, rules, out, (hipStream_t)stream);
    return check_launch(h, "pen_mask");
}

}  // extern "C"

// Feature PCA (pca.hip)
extern "C" {

int keep_pca_chunk(void) { return KEEP_PCA_CHUNK; }

int keep_pca_moments(keep_handle* h, const float* features, int64_t N, int64_t D, const float* centre, int64_t* sum, int64_t* count,
                     int64_t* gram, int64_t* skipped, int groups, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = cluster_shape_check(h, "pca_moments", N, D, 1)) return rc;
    if (!features || ((uintptr_t)features & 15)) return h->fail(KEEP_EINVAL, "pca_moments: features null or not 16-byte aligned");
    if ((uintptr_t)centre & 15) return h->fail(KEEP_EINVAL, "pca_moments: centre is not 16-byte aligned");
    if (!sum || !count) return h->fail(KEEP_EINVAL, "pca_moments: null sum or count");
    if (((uintptr_t)sum & 7) || ((uintptr_t)count & 7) || ((uintptr_t)gram & 7) || ((uintptr_t)skipped & 7))
        return h->fail(KEEP_EINVAL, "pca_moments: an accumulator is not 8-byte aligned");
    if (groups < 0 || groups > PCA_MAX_GROUPS) return h->fail(KEEP_EINVAL, "pca_moments: groups %d (0 = chosen here, 1 .. %d)", groups, PCA_MAX_GROUPS);
    KEEP_ON_DEVICE(h);
    if (int rc = ensure_arena(h, align_up((size_t)N))) return rc;
    launch_pca_moments(features, (int)N, (int)D, centre, sum, count, gram, skipped, (unsigned char*)h->arena, groups, (hipStream_t)stream);
    return check_launch(h, "pca_moments");
}

int keep_pca_project(keep_handle* h, const float* features, int64_t N, int64_t D, const float* components, int64_t k, const float* bias,
                     const float* scale, float* out, unsigned char* kept_out, int64_t* skipped, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = cluster_shape_check(h, "pca_project", N, D, 1)) return rc;
    if (k < 1 || k > PCA_MAX_K) return h->fail(KEEP_EINVAL, "pca_project: k = %lld (1 .. 64)", (long long)k);
    if (!features || !components || !out) return h->fail(KEEP_EINVAL, "pca_project: null features, components or output");
    if (((uintptr_t)features & 15) || ((uintptr_t)components & 15)) return h->fail(KEEP_EINVAL, "pca_project: features / components not 16-byte aligned");
    if (((uintptr_t)bias & 3) || ((uintptr_t)scale & 3) || ((uintptr_t)out & 3) || ((uintptr_t)skipped & 7))
        return h->fail(KEEP_EINVAL, "pca_project: bias, scale or an output is not aligned to its element size");
    KEEP_ON_DEVICE(h);
    launch_pca_project(features, (int)N, (int)D, components, (int)k, bias, scale, out, kept_out, skipped, (hipStream_t)stream);
    return check_launch(h, "pca_project");
}

int keep_class_render_rgb(keep_handle* h, const int64_t* acc, int64_t C, int64_t H, int64_t W, const int* planes, const unsigned char* thumb,
                          int64_t row_stride_bytes, int pix_stride, int background_rgb, const unsigned char* mask, int alpha,
                          unsigned char* out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!acc || ((uintptr_t)acc & 7)) return h->fail(KEEP_EINVAL, "class_render_rgb: acc is null or not 8-byte aligned");
    if (!planes || !out) return h->fail(KEEP_EINVAL, "class_render_rgb: null planes or output");
    if (C < 1 || C > CLASS_MAX) return h->fail(KEEP_EINVAL, "class_render_rgb: %lld classes (1 .. 64)", (long long)C);
    if (!pixels_ok(H, W, HEAT_MAX_PIXELS) || C * H * W > HEAT_MAX_PIXELS)
        return h->fail(KEEP_EINVAL, "class_render_rgb: %lld planes of %lldx%lld pixels (1 <= C H W <= 2^30)", (long long)C, (long long)H, (long long)W);
    for (int i = 0; i < 3; ++i)
        if (planes[i] < 0 || planes[i] >= C) return h->fail(KEEP_EINVAL, "class_render_rgb: plane %d outside 0 .. %lld", planes[i], (long long)(C - 1));
    if (thumb) {
        if (int rc = pix_stride_check(h, "class_render_rgb", pix_stride)) return rc;
        if (int rc = row_stride_check(h, "class_render_rgb", W, row_stride_bytes, pix_stride)) return rc;
    } else if (background_rgb < 0 || background_rgb > 0xFFFFFF) {
        return h->fail(KEEP_EINVAL, "class_render_rgb: background 0x%x outside [0, 0xFFFFFF]", background_rgb);
    }
    if (alpha < 0 || alpha > 256) return h->fail(KEEP_EINVAL, "class_render_rgb: alpha %d outside [0, 256]", alpha);
    KEEP_ON_DEVICE(h);
    launch_class_render_rgb(acc, (int)H, (int)W, planes, thumb, row_stride_bytes, pix_stride, (unsigned)background_rgb, mask, alpha, out,
                            (hipStream_t)stream);
    return check_launch(h, "class_render_rgb");
}

}  // extern "C"

// Exact t-SNE (tsne.hip)
extern "C" {

int keep_tsne_segment(void) { return KEEP_TSNE_SEGMENT; }

static int tsne_rows_check(keep_handle* h, const char* who, int64_t N) {
    if (N < 1 || N > TSNE_MAX_ROWS) return h->fail(KEEP_EINVAL, "%s: %lld rows (1 .. 2^20)", who, (long long)N);
    return KEEP_OK;
}

int keep_tsne_affinities(keep_handle* h, const int64_t* index, const float* score, const int32_t* count, int64_t N, int k, float perplexity,
                         float* p_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = tsne_rows_check(h, "tsne_affinities", N)) return rc;
    if (k < 1 || k > TOPK_MAX_K) return h->fail(KEEP_EINVAL, "tsne_affinities: k = %d (1 .. 64)", k);
    if (!(perplexity > 1.f) || !std::isfinite(perplexity)) return h->fail(KEEP_EINVAL, "tsne_affinities: perplexity %g (finite, > 1)", (double)perplexity);
    if (!index || !score || !count || !p_out) return h->fail(KEEP_EINVAL, "tsne_affinities: null index, score, count or output");
    if (((uintptr_t)index & 7) || ((uintptr_t)score & 3) || ((uintptr_t)count & 3) || ((uintptr_t)p_out & 3))
        return h->fail(KEEP_EINVAL, "tsne_affinities: a buffer is not aligned to its element size");
    KEEP_ON_DEVICE(h);
    launch_tsne_affinities(index, score, count, (int)N, k, perplexity, p_out, (hipStream_t)stream);
    return check_launch(h, "tsne_affinities");
}

int keep_tsne_repulsion(keep_handle* h, const float* y, int64_t N, float* partials, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = tsne_rows_check(h, "tsne_repulsion", N)) return rc;
    if (!y || ((uintptr_t)y & 7)) return h->fail(KEEP_EINVAL, "tsne_repulsion: y is null or not 8-byte aligned");
    if (!partials || ((uintptr_t)partials & 15)) return h->fail(KEEP_EINVAL, "tsne_repulsion: partials is null or not 16-byte aligned");
    KEEP_ON_DEVICE(h);
    launch_tsne_repulsion(y, (int)N, partials, (hipStream_t)stream);
    return check_launch(h, "tsne_repulsion");
}

int keep_tsne_step(keep_handle* h, const float* y, int64_t N, const float* partials, const int32_t* row_ptr, const int32_t* col,
                   const float* val, int64_t nnz, float exaggeration, float momentum, float lr, int stats, int64_t* sums, float* rz,
                   float* grad_out, float* update, float* gains, float* y_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (int rc = tsne_rows_check(h, "tsne_step", N)) return rc;
    if (!y || ((uintptr_t)y & 7)) return h->fail(KEEP_EINVAL, "tsne_step: y is null or not 8-byte aligned");
    if (!partials || ((uintptr_t)partials & 15) || !rz || ((uintptr_t)rz & 15))
        return h->fail(KEEP_EINVAL, "tsne_step: partials or rz is null or not 16-byte aligned");
    if (nnz < 0 || nnz > INT32_MAX) return h->fail(KEEP_EINVAL, "tsne_step: %lld graph entries (0 .. 2^31 - 1)", (long long)nnz);
    if (!row_ptr || ((uintptr_t)row_ptr & 3) || (nnz && (!col || !val)) || ((uintptr_t)col & 3) || ((uintptr_t)val & 3))
        return h->fail(KEEP_EINVAL, "tsne_step: a graph array is null or not 4-byte aligned");
    if (!sums || ((uintptr_t)sums & 7)) return h->fail(KEEP_EINVAL, "tsne_step: sums is null or not 8-byte aligned");
    if (!(exaggeration >= 0.f && exaggeration <= TSNE_MAX_EXAGGERATION))
        return h->fail(KEEP_EINVAL, "tsne_step: exaggeration %g outside [0, 32]", (double)exaggeration);
    if (!std::isfinite(momentum) || !std::isfinite(lr)) return h->fail(KEEP_EINVAL, "tsne_step: momentum or lr is not finite");
    const int given = (update != nullptr) + (gains != nullptr) + (y_out != nullptr);
    if (given != 0 && given != 3) return h->fail(KEEP_EINVAL, "tsne_step: update, gains and y_out go together (all or none)");
    if (given && y_out == y) return h->fail(KEEP_EINVAL, "tsne_step: y_out must not be y (other rows still read it)");
    if (((uintptr_t)grad_out & 3) || ((uintptr_t)update & 3) || ((uintptr_t)gains & 3) || ((uintptr_t)y_out & 7))
        return h->fail(KEEP_EINVAL, "tsne_step: an output is not aligned");
    KEEP_ON_DEVICE(h);
    launch_tsne_step(y, (int)N, partials, row_ptr, col, val, (int)nnz, exaggeration, momentum, lr, stats ? 1 : 0, sums, rz, grad_out, update,
                     gains, y_out, (hipStream_t)stream);
    return check_launch(h, "tsne_step");
}

}  // extern "C"
