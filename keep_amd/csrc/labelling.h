// What tissue.hip's connected-component kernels (cc_init / cc_merge / cc_compress / cc_count) share with components.hip, which
// builds the region table on their labels (DESIGN.md sections 11 and 13).
#pragma once
#include "common.h"

namespace keepk {

constexpr int TISSUE_ERR_BIT = 4;                     // keep_handle::err_flag, bit 2: a labelling loop ran into its iteration cap
constexpr int CC_BORDER = (int)0x80000000;            // info[root]: bit 31 = the component touches the image border, bits 0..30 = area

// tile t of the 64 x 4 walk -> this thread's pixel (x, y); false when the WAVE's row is outside (wave-uniform), x may still be >= w
struct CcWalk {
    int tx; int64_t ntiles;
    __device__ CcWalk(int h, int w) : tx((w + 63) / 64), ntiles((int64_t)((w + 63) / 64) * ((h + 3) / 4)) {}
    __device__ bool at(int64_t t, int h, int* x, int* y) const {
        *x = (int)(t % tx) * 64 + (threadIdx.x & 63);
        *y = (int)(t / tx) * 4 + (threadIdx.x >> 6);
        return *y < h;
    }
};

}  // namespace keepk
