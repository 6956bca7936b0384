// What does the matrix pipe alone deliver at the socket's power cap?  No memory traffic inside the loop: every wave holds its operand fragments in registers and
// issues independent MFMAs on a 128 x 64 output tile (128 accumulator registers), so the pipe's inputs change with every instruction.
//   SHAPE 32: 2 A x 4 B fragments, 8 v_mfma_f32_32x32x16_f16 per iteration (all (i, j) pairs)
//   SHAPE 16: 8 A x 4 B fragments, 32 v_mfma_f32_16x16x32_f16 per two iterations (the same tile over K = 32): same FLOPs per iteration, same cycles per FLOP
// Run with high-entropy operands (randn-like fp16), with zeros and with a constant; 2 waves per SIMD (512 threads per workgroup, one per CU) as the GEMM kernels run; the two
// shapes alternate launch by launch.
//   hipcc --offload-arch=gfx950 -O3 tools/ubench/mfma_power.hip -o tools/ubench/mfma_power && tools/ubench/mfma_power
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <int SHAPE>
__global__ __launch_bounds__(512, 2) void burn(const f16x8* __restrict__ src, float* __restrict__ out, int iters, long long* clk) {
    const int t = blockIdx.x * 512 + threadIdx.x;
    float s = 0.f;
    long long c0, r0, c1, r1;
    if constexpr (SHAPE == 32) {
        f16x8 a[2], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { if (i < 2) a[i] = src[(size_t)t * 8 + i]; b[i] = src[(size_t)t * 8 + 4 + i]; }
        f32x16 acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = f32x16{};
        c0 = __builtin_readcyclecounter(); r0 = __builtin_amdgcn_s_memrealtime();
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i * 4 + j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i], b[j], acc[i * 4 + j], 0, 0, 0);
        }
        c1 = __builtin_readcyclecounter(); r1 = __builtin_amdgcn_s_memrealtime();
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) s += acc[i][r];
    } else {
        f16x8 a[8], b[4];
        const int t2 = (t + 4096) % (256 * 512);                   // (12 fragments per lane: the B set comes from another lane's slice of the buffer)
#pragma unroll
        for (int i = 0; i < 8; ++i) { a[i] = src[(size_t)t * 8 + i]; if (i < 4) b[i] = src[(size_t)t2 * 8 + 4 + i]; }
        f32x4 acc[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) acc[i] = f32x4{};
        c0 = __builtin_readcyclecounter(); r0 = __builtin_amdgcn_s_memrealtime();
        for (int it = 0; it < iters; it += 2) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i * 4 + j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(b[j], a[i], acc[i * 4 + j], 0, 0, 0);
        }
        c1 = __builtin_readcyclecounter(); r1 = __builtin_amdgcn_s_memrealtime();
#pragma unroll
        for (int i = 0; i < 32; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) s += acc[i][r];
    }
    out[t] = s;
    if (threadIdx.x == 0) { clk[blockIdx.x * 2] = c1 - c0; clk[blockIdx.x * 2 + 1] = r1 - r0; }
}
int main() {
    const int blocks = 256, threads = 512, iters = 400000;
    const size_t nfrag = (size_t)blocks * threads * 8;
    std::vector<_Float16> h(nfrag * 8);
    f16x8* src; float* out; long long* clk;
    hipMalloc(&src, nfrag * 16); hipMalloc(&out, blocks * threads * 4); hipMalloc(&clk, blocks * 16);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    for (int mode = 0; mode < 3; ++mode) {
        srand(1);
        for (size_t i = 0; i < h.size(); ++i) {
            float u1 = (rand() + 1.0f) / (RAND_MAX + 2.0f), u2 = (rand() + 1.0f) / (RAND_MAX + 2.0f);
            float g = sqrtf(-2.f * logf(u1)) * cosf(6.2831853f * u2);
            h[i] = mode == 0 ? (_Float16)(g * 0.05f) : mode == 1 ? (_Float16)0.f : (_Float16)(0.03125f);
        }
        hipMemcpy(src, h.data(), nfrag * 16, hipMemcpyHostToDevice);
        for (int rep = 0; rep < 6; ++rep) {
            const int shape = rep & 1 ? 16 : 32;
            hipEventRecord(e0, 0);
            if (shape == 32) hipLaunchKernelGGL(burn<32>, dim3(blocks), dim3(threads), 0, 0, src, out, iters, clk);
            else hipLaunchKernelGGL(burn<16>, dim3(blocks), dim3(threads), 0, 0, src, out, iters, clk);
            hipEventRecord(e1, 0); hipEventSynchronize(e1);
            float ms; hipEventElapsedTime(&ms, e0, e1);
            long long c[2]; hipMemcpy(c, clk, 16, hipMemcpyDeviceToHost);
            const double flop = (double)blocks * 8 * iters * 8 * 2.0 * 32 * 32 * 16;
            printf("%-28s %s %8.2f ms  %7.0f TFLOP/s  (%.3f of 2516.6)   shader clock %.0f MHz\n",
                   mode == 0 ? "random N(0, 0.05) operands" : mode == 1 ? "all-zero operands" : "constant 2^-5 operands", shape == 32 ? "32x32x16" : "16x16x32", ms,
                   flop / ms / 1e9, flop / ms / 1e9 / 2516.6, 100.0 * (double)c[0] / (double)c[1]);
        }
    }
    return 0;
}
