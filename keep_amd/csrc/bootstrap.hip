// Bootstrap resampling of the tile ROC and of a confusion matrix: B replicates of "draw n of the n items with
// replacement" in one call, every replicate's counts in integers.  The draws come from a counter-based generator (keep_hip.h states
// it), so replicate b is the same multiset whatever B, the split over calls, the grid or the order of the atomics, and the results
// equal keep_amd.bootstrap.boot_roc_numpy / boot_confusion_numpy exactly.
//
//   boot_flags        valid[i] = scores[i] is no NaN; head[i] = sorted[i] opens a run of equal scores (rank.hip's sort: NaNs last, -0 as +0)
//   boot_scan1/2      exclusive scans of both flag arrays in one pass each: a scored item's place in original order, a run's rank g
//                     among the K distinct scores
//   boot_items        one word per scored item, in original order: g << 1 | label (a binary search for the score's run)
//   boot_roc          one workgroup of 1024 threads per replicate, persistent over the replicates.  Per draw a hash, a 4-byte gather of
//                     the item's word and one integer add into the histogram bin of that word (2 K bins: wn[g], wp[g] side by side).
//                     Then one pass over the K groups: a block scan of wn gives the negatives below every group, and
//                     U2 = sum wp[g] (2 sum_{g' < g} wn[g'] + wn[g]).  The pass zeroes the bins it reads.
//                     K <= BOOT_LDS_GROUPS: the bins live in LDS (64 KiB: two workgroups on a CU are its 32 waves and 128 of its 160
//                     KiB).  Above: one slab of 2 N words per resident workgroup in global memory, at most BOOT_SLAB_BYTES in all; the
//                     workgroups without a slab leave at once.  The slab is read and zeroed with device-scope atomic loads / stores: the
//                     adds happen in L2 and a plain load could be served from the CU's vector cache
//   boot_codes        truth, pred -> one byte t C + p per item (labels clamped into [0, C): no bin leaves the table)
//   boot_conf         one workgroup of 256 threads per replicate, persistent.  C <= 4: every thread counts in its own column of LDS
//                     (16 bins x 256 threads), no atomics at all: with C = 2 there are four hot bins.  C > 4: sixteen copies of the
//                     table (wave x lane % 4, rows of 257 words so that equal codes in different copies fall into different banks) and
//                     returnless LDS adds
//
// Wave64; integer atomics only, none with a used result.
#include "common.h"
#include "boot_rng.h"
#include "../../include/keep_hip.h"

namespace keepk {

static_assert(BOOT_LDS_GROUPS == KEEP_BOOT_LDS_GROUPS, "the cap the header exports is the kernel's");
constexpr int BOOT_THREADS = 1024;
constexpr int BOOT_WAVES = BOOT_THREADS / 64;
constexpr int BOOT_SCAN_CHUNK = 2048;

__device__ __forceinline__ int boot_count(const int64_t* dev, int N) {     // whatever the word holds, the indices stay inside [0, N)
    const int64_t v = *dev;
    return v < 0 ? 0 : (v > N ? N : (int)v);
}

// flags: [valid: chunks * BOOT_SCAN_CHUNK][head: chunks * BOOT_SCAN_CHUNK], the tails zero
__global__ __launch_bounds__(256)
void boot_flags_kernel(const float* __restrict__ scores, const float* __restrict__ sorted, const int64_t* __restrict__ n_dev, int N, int padded,
                       int* __restrict__ flags) {
    const int n = boot_count(n_dev, N);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < padded; i += gridDim.x * 256) {
        int valid = 0, head = 0;
        if (i < N) {
            const float v = scores[i];
            valid = v == v;
            head = i < n && (i == 0 || sorted[i - 1] != sorted[i]);
        }
        flags[i] = valid;
        flags[padded + i] = head;
    }
}

// exclusive scan inside every chunk of BOOT_SCAN_CHUNK entries, in place; totals[chunk] = the chunk's sum
__global__ __launch_bounds__(256)
void boot_scan1_kernel(int* __restrict__ v, int* __restrict__ totals) {
    __shared__ int scan[256];
    constexpr int PER = BOOT_SCAN_CHUNK / 256;
    const int64_t first = (int64_t)blockIdx.x * BOOT_SCAN_CHUNK + threadIdx.x * PER;
    int x[PER], sum = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        x[k] = v[first + k];
        sum += x[k];
    }
    int total;
    int run = block_exclusive_scan256(sum, scan, &total);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        v[first + k] = run;
        run += x[k];
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// block 0: the chunk totals of the valid flags, block 1: those of the head flags; exclusive scans in place, meta[block] = the sum (n, K)
__global__ __launch_bounds__(256)
void boot_scan2_kernel(int* __restrict__ totals, int chunks, int* __restrict__ meta) {
    __shared__ int scan[256];
    int* mine = totals + (int64_t)blockIdx.x * chunks;
    int carry = 0;
    for (int first = 0; first < chunks; first += 256) {
        const int i = first + threadIdx.x;
        const int v = i < chunks ? mine[i] : 0;
        int total;
        const int ex = block_exclusive_scan256(v, scan, &total);
        if (i < chunks) mine[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) meta[blockIdx.x] = carry;
}

__global__ __launch_bounds__(256)
void boot_items_kernel(const float* __restrict__ scores, const unsigned char* __restrict__ labels, const float* __restrict__ sorted,
                       const int64_t* __restrict__ n_dev, int N, int padded, int chunks, const int* __restrict__ flags,
                       const int* __restrict__ totals, unsigned* __restrict__ items) {
    const int n = boot_count(n_dev, N);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) {
        const float v = scores[i];
        if (!(v == v)) continue;
        const int at = flags[i] + totals[i / BOOT_SCAN_CHUNK];
        int lo = 0, hi = n;
        while (lo < hi) {                                       // the first sorted value that is not below v: the head of v's run
            const int mid = (lo + hi) >> 1;
            if (sorted[mid] < v) lo = mid + 1; else hi = mid;
        }
        if (lo >= N) lo = N - 1;
        const unsigned g = (unsigned)(flags[padded + lo] + totals[chunks + lo / BOOT_SCAN_CHUNK]);
        if (at >= 0 && at < N) items[at] = (g << 1) | (labels[i] != 0 ? 1u : 0u);
    }
}

// out[r] = n, P_b, Nn_b, U2_b for b = first + r.  slabs: nslabs x 2 N words (used when K > BOOT_LDS_GROUPS; nslabs >= 1 then)
__global__ __launch_bounds__(BOOT_THREADS, 8)                   // 8 waves per SIMD = two workgroups on a CU: at most 64 registers
void boot_roc_kernel(const unsigned* __restrict__ items, const int* __restrict__ meta, int N, unsigned long long seed, long long first, int B,
                     unsigned* __restrict__ slabs, int nslabs, long long* __restrict__ out) {
    __shared__ unsigned long long hist[BOOT_LDS_GROUPS];        // wn in the low word, wp in the high one: bins 2 g and 2 g + 1
    __shared__ unsigned wsum[BOOT_WAVES];
    __shared__ unsigned long long red[3][BOOT_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n = meta[0] < 0 ? 0 : (meta[0] > N ? N : meta[0]);
    const int K = meta[1] < 0 ? 0 : (meta[1] > n ? n : meta[1]);
    const bool lds = K <= BOOT_LDS_GROUPS;
    int stride = gridDim.x;
    if (!lds) {
        if ((int)blockIdx.x >= nslabs) return;                    // uniform over the workgroup
        stride = nslabs < stride ? nslabs : stride;
    }
    const unsigned bins = 2u * (unsigned)K;
    unsigned* hist32 = reinterpret_cast<unsigned*>(hist);
    unsigned long long* slab = reinterpret_cast<unsigned long long*>(slabs + (size_t)blockIdx.x * 2 * (size_t)N);
    if (lds) {
        for (int g = t; g < K; g += BOOT_THREADS) hist[g] = 0;
    } else {
        for (int g = t; g < K; g += BOOT_THREADS) __hip_atomic_store(&slab[g], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
    }
    __syncthreads();
    for (int r = blockIdx.x; r < B; r += stride) {
        const long long b = first + r;
        const unsigned long long key = boot_key(seed, b);
        if (lds) {
            for (int j = t; j < n; j += BOOT_THREADS) {
                const unsigned w = items[b < 0 ? (unsigned)j : boot_draw(key, (unsigned)j, (unsigned)n)];
                if (w < bins) atomicAdd(&hist32[w], 1u);          // result unused: a returnless add
            }
        } else {
            unsigned* slab32 = reinterpret_cast<unsigned*>(slab);
            for (int j = t; j < n; j += BOOT_THREADS) {
                const unsigned w = items[b < 0 ? (unsigned)j : boot_draw(key, (unsigned)j, (unsigned)n)];
                if (w < bins) atomicAdd(&slab32[w], 1u);
            }
            __threadfence();
        }
        __syncthreads();
        unsigned long long u2 = 0, carry = 0;
        unsigned p = 0, nn = 0;
        for (int g0 = 0; g0 < K; g0 += BOOT_THREADS) {           // the bound is the workgroup's: barriers and shuffles inside
            const int g = g0 + t;
            unsigned long long word = 0;
            if (g < K) {
                if (lds) {
                    word = hist[g];
                    hist[g] = 0;
                } else {
                    word = __hip_atomic_load(&slab[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&slab[g], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            const unsigned wn = (unsigned)word, wp = (unsigned)(word >> 32);
            unsigned incl = wn;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned up = __shfl_up(incl, o);
                if (lane >= o) incl += up;
            }
            if (lane == 63) wsum[wave] = incl;
            __syncthreads();
            unsigned below = 0, total = 0;
#pragma unroll
            for (int w = 0; w < BOOT_WAVES; ++w) {
                const unsigned s = wsum[w];
                below += w < wave ? s : 0u;
                total += s;
            }
            __syncthreads();
            const unsigned long long less = carry + below + (incl - wn);
            u2 += (unsigned long long)wp * (2 * less + wn);
            p += wp;
            nn += wn;
            carry += total;
        }
        unsigned long long v0 = u2, v1 = p, v2 = nn;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            v0 += __shfl_xor(v0, o);
            v1 += __shfl_xor(v1, o);
            v2 += __shfl_xor(v2, o);
        }
        if (lane == 0) { red[0][wave] = v0; red[1][wave] = v1; red[2][wave] = v2; }
        if (!lds) __threadfence();                                // the zeroes are in place before the next replicate adds
        __syncthreads();
        if (t == 0) {
            unsigned long long s0 = 0, s1 = 0, s2 = 0;
            for (int w = 0; w < BOOT_WAVES; ++w) { s0 += red[0][w]; s1 += red[1][w]; s2 += red[2][w]; }
            long long* row = out + (size_t)r * 4;
            row[0] = n; row[1] = (long long)s1; row[2] = (long long)s2; row[3] = (long long)s0;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256)
void boot_codes_kernel(const unsigned char* __restrict__ truth, const unsigned char* __restrict__ pred, int N, int C,
                       unsigned char* __restrict__ codes) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) {
        const int a = truth[i] < C ? truth[i] : C - 1, b = pred[i] < C ? pred[i] : C - 1;
        codes[i] = (unsigned char)(a * C + b);
    }
}

constexpr int BOOT_CONF_ROW = 257;                               // words per copy of the table in the general kernel

// SMALL: C <= 4.  out[r][code] for b = first + r
template <bool SMALL>
__global__ __launch_bounds__(256)
void boot_conf_kernel(const unsigned char* __restrict__ codes, int N, int C, unsigned long long seed, long long first, int B,
                      long long* __restrict__ out) {
    __shared__ unsigned tab[SMALL ? 16 * 256 : 16 * BOOT_CONF_ROW];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, cc = C * C;
    const int copy = (wave * 4 + (lane & 3)) * BOOT_CONF_ROW;
    if (SMALL) {
        for (int c = 0; c < 16; ++c) tab[c * 256 + t] = 0;
    } else {
        for (int i = t; i < 16 * BOOT_CONF_ROW; i += 256) tab[i] = 0;
    }
    __syncthreads();
    for (int r = blockIdx.x; r < B; r += gridDim.x) {
        const long long b = first + r;
        const unsigned long long key = boot_key(seed, b);
        for (int j = t; j < N; j += 256) {
            const unsigned c = codes[b < 0 ? (unsigned)j : boot_draw(key, (unsigned)j, (unsigned)N)];
            if (SMALL) {
                if (c < 16) tab[c * 256 + t] += 1;                // this thread's own column
            } else {
                atomicAdd(&tab[copy + c], 1u);                    // c <= 255 < BOOT_CONF_ROW; returnless
            }
        }
        __syncthreads();
        long long* row = out + (size_t)r * cc;
        if (SMALL) {
            for (int c = wave; c < cc; c += 4) {
                unsigned v = tab[c * 256 + lane] + tab[c * 256 + 64 + lane] + tab[c * 256 + 128 + lane] + tab[c * 256 + 192 + lane];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
                if (lane == 0) row[c] = v;
            }
            __syncthreads();
            for (int c = 0; c < cc; ++c) tab[c * 256 + t] = 0;
        } else {
            if (t < cc) {
                unsigned v = 0;
                for (int k = 0; k < 16; ++k) v += tab[k * BOOT_CONF_ROW + t];
                row[t] = v;
            }
            __syncthreads();
            for (int i = t; i < 16 * BOOT_CONF_ROW; i += 256) tab[i] = 0;
        }
        __syncthreads();
    }
}

}  // namespace keepk
using namespace keepk;

static inline size_t boot_align(size_t b) { return (b + 255) & ~(size_t)255; }

namespace {
struct BootWs {
    float* sorted;
    int64_t* n_dev;
    int* meta;                                                // n, K
    unsigned char* sort;
    int *flags, *totals;
    unsigned* items;
    unsigned* slabs;
    int padded, chunks, nslabs;
    size_t bytes;
};
BootWs boot_carve(unsigned char* ws, int64_t N, int grid) {
    size_t at = 0;
    auto take = [&](size_t bytes) { unsigned char* p = ws + at; at += boot_align(bytes); return p; };
    size_t table_off, totals_off;
    BootWs r;
    r.chunks = (int)((N + BOOT_SCAN_CHUNK - 1) / BOOT_SCAN_CHUNK);
    r.padded = r.chunks * BOOT_SCAN_CHUNK;
    r.sorted = (float*)take((size_t)N * 4);
    r.n_dev = (int64_t*)take(8);
    r.meta = (int*)take(8);
    r.sort = take(sort_workspace_bytes(N, &table_off, &totals_off));
    r.flags = (int*)take((size_t)2 * r.padded * 4);
    r.totals = (int*)take((size_t)2 * r.chunks * 4);
    r.items = (unsigned*)take((size_t)N * 4);
    r.nslabs = 0;
    if (N > BOOT_LDS_GROUPS) {                                // K <= N: below the cap no slab is ever touched
        const int64_t fit = (int64_t)(BOOT_SLAB_BYTES / ((size_t)N * 8));
        r.nslabs = (int)std::max<int64_t>(1, std::min<int64_t>(fit, grid));
    }
    r.slabs = (unsigned*)take((size_t)r.nslabs * (size_t)N * 8);
    r.bytes = at;
    return r;
}
int boot_roc_grid(int64_t B) { return (int)std::max<int64_t>(1, std::min<int64_t>(B, 2 * (int64_t)keep_num_cus())); }
}  // namespace

size_t boot_roc_workspace_bytes(int64_t N, int64_t B) { return N < 1 || B < 1 ? 0 : boot_carve(nullptr, N, boot_roc_grid(B)).bytes; }

void launch_boot_roc(const float* scores, const unsigned char* labels, int64_t N64, unsigned long long seed, int64_t first, int64_t B,
                     unsigned char* ws, int64_t* out, hipStream_t s) {
    if (B < 1) return;
    if (N64 < 1) {
        (void)hipMemsetAsync(out, 0, (size_t)B * 4 * 8, s);
        return;
    }
    const int N = (int)N64, grid = boot_roc_grid(B);
    const BootWs w = boot_carve(ws, N, grid);
    const int blocks = (int)std::min<int64_t>((N64 + 255) / 256, 16384);
    launch_sort_f32(scores, N, w.sort, w.sorted, w.n_dev, s);
    hipLaunchKernelGGL(boot_flags_kernel, dim3(std::min(w.padded / 256, 16384)), dim3(256), 0, s, scores,
                       (const float*)w.sorted, (const int64_t*)w.n_dev, N, w.padded, w.flags);
    hipLaunchKernelGGL(boot_scan1_kernel, dim3(2 * w.chunks), dim3(256), 0, s, w.flags, w.totals);
    hipLaunchKernelGGL(boot_scan2_kernel, dim3(2), dim3(256), 0, s, w.totals, w.chunks, w.meta);
    hipLaunchKernelGGL(boot_items_kernel, dim3(blocks), dim3(256), 0, s, scores, labels, (const float*)w.sorted, (const int64_t*)w.n_dev, N,
                       w.padded, w.chunks, (const int*)w.flags, (const int*)w.totals, w.items);
    hipLaunchKernelGGL(boot_roc_kernel, dim3(grid), dim3(BOOT_THREADS), 0, s, (const unsigned*)w.items, (const int*)w.meta, N, seed,
                       (long long)first, (int)B, w.slabs, w.nslabs, reinterpret_cast<long long*>(out));
}

size_t boot_confusion_workspace_bytes(int64_t N) { return N < 1 ? 0 : boot_align((size_t)N); }

void launch_boot_confusion(const unsigned char* truth, const unsigned char* pred, int64_t N64, int C, unsigned long long seed, int64_t first,
                           int64_t B, unsigned char* ws, int64_t* out, hipStream_t s) {
    if (B < 1) return;
    if (N64 < 1) {
        (void)hipMemsetAsync(out, 0, (size_t)B * C * C * 8, s);
        return;
    }
    const int N = (int)N64;
    const int blocks = (int)std::min<int64_t>((N64 + 255) / 256, 16384);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(B, 8 * (int64_t)keep_num_cus()));
    hipLaunchKernelGGL(boot_codes_kernel, dim3(blocks), dim3(256), 0, s, truth, pred, N, C, ws);
    if (C <= 4)
        hipLaunchKernelGGL(boot_conf_kernel<true>, dim3(grid), dim3(256), 0, s, (const unsigned char*)ws, N, C, seed, (long long)first, (int)B,
                           reinterpret_cast<long long*>(out));
    else
        hipLaunchKernelGGL(boot_conf_kernel<false>, dim3(grid), dim3(256), 0, s, (const unsigned char*)ws, N, C, seed, (long long)first, (int)B,
                           reinterpret_cast<long long*>(out));
}
