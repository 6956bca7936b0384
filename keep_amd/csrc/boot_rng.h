// The counter-based generator of the bootstrap (include/keep_hip.h and keep_amd/bootstrap.py state it), shared by
// bootstrap.hip and fewshot.hip: a draw depends on (seed, stream, position, n) alone.
#pragma once

namespace keepk {

constexpr unsigned long long BOOT_G = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ unsigned long long boot_mix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ unsigned long long boot_key(unsigned long long seed, long long b) {
    return boot_mix64(seed ^ boot_mix64((unsigned long long)(b + 1) * BOOT_G));
}

// 0 <= result < n
__device__ __forceinline__ unsigned boot_draw(unsigned long long key, unsigned j, unsigned n) {
    return (unsigned)__umul64hi(boot_mix64(key + (unsigned long long)j * BOOT_G), (unsigned long long)n);
}

}  // namespace keepk
