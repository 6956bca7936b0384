// Sorted score population and rank percentiles: what CLAM's heatmap does with scipy.stats.rankdata /
// percentileofscore before it colours a slide.  Every result is unique (a sorted array, counts of smaller and equal values), so it is
// the same from run to run and equals keep_amd.heatmap.sort_numpy / rank_numpy exactly.
//
//   sort_small        M <= 4096: one block, the keys stay in LDS for the four passes
//   sort_hist         per pass: the digit counts of every block's tile of 4096 keys -> table[digit][block]
//   sort_scan1/2      one exclusive scan over the digit-major table (chunks of 2048 entries, then the chunk totals)
//   sort_scatter      per pass: keys to their places; stable within a block (lanes ranked against equal digits with __ballot, waves
//                     and rounds in order), which LSD passes need
//   sort_count        n = the first NaN of the sorted array (a binary search by one thread)
//   rank              one thread per query: lower and upper bound in the sorted population
//
// Keys: bits ^ (sign ? 0xFFFFFFFF : 0x80000000) after -0 -> +0; a NaN becomes 0xFFFFFFFF, which no other float maps to (it would need
// the bits 0x7FFFFFFF, a NaN), and leaves as the canonical 0x7FC00000.  The first pass reads the floats, the last writes them.
#include "common.h"
#include "../../include/keep_hip.h"

namespace keepk {

constexpr int SORT_ROUNDS = SORT_TILE / 256;
constexpr unsigned SORT_NAN_KEY = 0xFFFFFFFFu;

__device__ __forceinline__ unsigned sort_key(float v) {
    unsigned b = __float_as_uint(v);
    if (v != v) return SORT_NAN_KEY;
    if (b == 0x80000000u) b = 0;
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

__device__ __forceinline__ unsigned sort_unkey(unsigned k) {
    if (k == SORT_NAN_KEY) return 0x7FC00000u;
    return (k & 0x80000000u) ? k ^ 0x80000000u : ~k;
}

// One round: 256 keys in thread order -> this thread's place.  base[256]: where the next key of each digit goes; wcnt[4][256]: zero
// on entry and on return.  Every thread of the block calls it (barriers and ballots inside); an inactive thread's result is unused.
__device__ __forceinline__ unsigned sort_round_place(unsigned digit, bool active, unsigned* base, unsigned* wcnt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long peers = __ballot(active);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (digit >> b) & 1u;
        const unsigned long long m = __ballot(bit);
        peers &= bit ? m : ~m;
    }
    const unsigned rank = __popcll(peers & (((unsigned long long)1 << lane) - 1));
    if (active && rank == 0) wcnt[wave * 256 + digit] = __popcll(peers);
    __syncthreads();
    unsigned place = 0;
    if (active) {
        place = base[digit] + rank;
        for (int w = 0; w < wave; ++w) place += wcnt[w * 256 + digit];
    }
    __syncthreads();
    unsigned add = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        add += wcnt[w * 256 + threadIdx.x];
        wcnt[w * 256 + threadIdx.x] = 0;
    }
    base[threadIdx.x] += add;
    __syncthreads();
    return place;
}

__global__ __launch_bounds__(256)
void sort_small_kernel(const float* __restrict__ values, int M, unsigned* __restrict__ out, int64_t* __restrict__ n_out) {
    __shared__ unsigned keys[2][SORT_TILE];
    __shared__ unsigned base[256], wcnt[4 * 256];
    __shared__ int scan[256];
    __shared__ unsigned valid;
    const int t = threadIdx.x;
    if (t == 0) valid = 0;
    for (int i = t; i < 4 * 256; i += 256) wcnt[i] = 0;
    __syncthreads();
    unsigned mine = 0;
    for (int i = t; i < M; i += 256) {
        const unsigned k = sort_key(values[i]);
        keys[0][i] = k;
        mine += k != SORT_NAN_KEY;
    }
    if (mine) atomicAdd(&valid, mine);
    const int rounds = (M + 255) / 256;
    for (int pass = 0; pass < 4; ++pass) {
        const unsigned* src = keys[pass & 1];
        unsigned* dst = keys[(pass & 1) ^ 1];
        const int shift = 8 * pass;
        base[t] = 0;
        __syncthreads();                              // also: the keys of the pass before (or the load) are in place
        for (int i = t; i < M; i += 256) atomicAdd(&base[(src[i] >> shift) & 255u], 1u);
        __syncthreads();
        int total;
        const int first = block_exclusive_scan256((int)base[t], scan, &total);
        base[t] = (unsigned)first;
        __syncthreads();
        for (int r = 0; r < rounds; ++r) {
            const int i = r * 256 + t;
            const bool active = i < M;
            const unsigned k = active ? src[i] : 0u;
            const unsigned place = sort_round_place((k >> shift) & 255u, active, base, wcnt);
            if (active) dst[place] = k;               // place < M: the digit counts sum to M
        }
    }
    __syncthreads();
    for (int i = t; i < M; i += 256) out[i] = sort_unkey(keys[0][i]);
    if (t == 0) *n_out = (int64_t)valid;
}

template <bool FIRST>
__device__ __forceinline__ unsigned sort_load(const void* in, int64_t i) {
    return FIRST ? sort_key(reinterpret_cast<const float*>(in)[i]) : reinterpret_cast<const unsigned*>(in)[i];
}

// table[digit * nb + block] = the number of keys of the block's tile with that digit
template <bool FIRST>
__global__ __launch_bounds__(256)
void sort_hist_kernel(const void* __restrict__ in, int M, int shift, int nb, unsigned* __restrict__ table) {
    __shared__ unsigned hist[256];
    const int t = threadIdx.x, b = blockIdx.x;
    hist[t] = 0;
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < SORT_ROUNDS; ++r) {
        const int i = b * SORT_TILE + r * 256 + t;
        if (i < M) atomicAdd(&hist[(sort_load<FIRST>(in, i) >> shift) & 255u], 1u);
    }
    __syncthreads();
    table[(int64_t)t * nb + b] = hist[t];
}

// exclusive scan inside every chunk of SORT_SCAN_CHUNK entries, in place; totals[chunk] = the chunk's sum
__global__ __launch_bounds__(256)
void sort_scan1_kernel(unsigned* __restrict__ table, int entries, unsigned* __restrict__ totals) {
    __shared__ int scan[256];
    constexpr int PER = SORT_SCAN_CHUNK / 256;
    const int first = blockIdx.x * SORT_SCAN_CHUNK + threadIdx.x * PER;
    unsigned v[PER], sum = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        v[k] = first + k < entries ? table[first + k] : 0u;
        sum += v[k];
    }
    int total;
    unsigned run = (unsigned)block_exclusive_scan256((int)sum, scan, &total);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (first + k < entries) table[first + k] = run;
        run += v[k];
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = (unsigned)total;
}

// one block: exclusive scan of the chunk totals, in place
__global__ __launch_bounds__(256)
void sort_scan2_kernel(unsigned* __restrict__ totals, int chunks) {
    __shared__ int scan[256];
    unsigned carry = 0;
    for (int first = 0; first < chunks; first += 256) {
        const int i = first + threadIdx.x;
        const unsigned v = i < chunks ? totals[i] : 0u;
        int total;
        const unsigned ex = (unsigned)block_exclusive_scan256((int)v, scan, &total);
        if (i < chunks) totals[i] = carry + ex;
        carry += (unsigned)total;
    }
}

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(256)
void sort_scatter_kernel(const void* __restrict__ in, int M, int shift, int nb, const unsigned* __restrict__ table,
                         const unsigned* __restrict__ totals, unsigned* __restrict__ out) {
    __shared__ unsigned base[256], wcnt[4 * 256];
    const int t = threadIdx.x, b = blockIdx.x;
    const int64_t e = (int64_t)t * nb + b;
    base[t] = table[e] + totals[e / SORT_SCAN_CHUNK];
    for (int i = t; i < 4 * 256; i += 256) wcnt[i] = 0;
    __syncthreads();
    for (int r = 0; r < SORT_ROUNDS; ++r) {
        const int i = b * SORT_TILE + r * 256 + t;
        const bool active = i < M;
        const unsigned k = active ? sort_load<FIRST>(in, i) : 0u;
        const unsigned place = sort_round_place((k >> shift) & 255u, active, base, wcnt);
        if (active && place < (unsigned)M) out[place] = LAST ? sort_unkey(k) : k;      // place < M always: the table sums to M
    }
}

// n = the number of leading non-NaN values of the sorted array
__global__ void sort_count_kernel(const float* __restrict__ sorted, int M, int64_t* __restrict__ n_out) {
    int lo = 0, hi = M;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const float v = sorted[mid];
        if (v == v) lo = mid + 1; else hi = mid;
    }
    *n_out = lo;
}

__global__ __launch_bounds__(256)
void rank_kernel(const float* __restrict__ sorted, int M, const int64_t* __restrict__ n_dev, const float* __restrict__ queries, int N,
                 int self, float* __restrict__ pct, int* __restrict__ less, int* __restrict__ eq) {
    const int64_t nn = *n_dev;
    const int n = nn < 0 ? 0 : (nn > M ? M : (int)nn);                 // whatever the word holds, the search stays inside sorted[0:M]
    for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) {
        const float q = queries[i];
        int lt = -1, same = -1;
        float p = __uint_as_float(0x7FC00000u);
        if (q == q) {
            int lo = 0, hi = n;
            while (lo < hi) {                                           // lower bound: #{sorted < q}
                const int mid = (lo + hi) >> 1;
                if (sorted[mid] < q) lo = mid + 1; else hi = mid;
            }
            lt = lo;
            hi = n;
            while (lo < hi) {                                           // upper bound: #{sorted <= q}
                const int mid = (lo + hi) >> 1;
                if (sorted[mid] <= q) lo = mid + 1; else hi = mid;
            }
            same = lo - lt;
            if (n > 0) p = (float)((double)(2ll * lt + same + self) / (double)(2ll * n));
        }
        if (pct) pct[i] = p;
        if (less) less[i] = lt;
        if (eq) eq[i] = same;
    }
}

}  // namespace keepk
using namespace keepk;

size_t sort_workspace_bytes(int64_t M, size_t* table_off, size_t* totals_off) {
    const int64_t nb = (M + SORT_TILE - 1) / SORT_TILE, entries = 256 * nb, chunks = (entries + SORT_SCAN_CHUNK - 1) / SORT_SCAN_CHUNK;
    const auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    if (M <= SORT_TILE) {
        *table_off = *totals_off = 0;
        return 0;
    }
    *table_off = up((size_t)M * 4);
    *totals_off = *table_off + up((size_t)entries * 4);
    return *totals_off + up((size_t)chunks * 4);
}

void launch_sort_f32(const float* values, int64_t M64, unsigned char* ws, float* sorted_out, int64_t* n_out, hipStream_t s) {
    const int M = (int)M64;
    unsigned* out = reinterpret_cast<unsigned*>(sorted_out);
    if (M <= SORT_TILE) {
        hipLaunchKernelGGL(sort_small_kernel, dim3(1), dim3(256), 0, s, values, M, out, n_out);
        return;
    }
    size_t table_off, totals_off;
    (void)sort_workspace_bytes(M, &table_off, &totals_off);
    unsigned* keys = reinterpret_cast<unsigned*>(ws);
    unsigned* table = reinterpret_cast<unsigned*>(ws + table_off);
    unsigned* totals = reinterpret_cast<unsigned*>(ws + totals_off);
    const int nb = (M + SORT_TILE - 1) / SORT_TILE, entries = 256 * nb, chunks = (entries + SORT_SCAN_CHUNK - 1) / SORT_SCAN_CHUNK;
    // values -> keys -> sorted_out (as keys) -> keys -> sorted_out (as floats)
    const void* src[4] = {values, keys, out, keys};
    unsigned* dst[4] = {keys, out, keys, out};
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 8 * pass;
        if (pass == 0) hipLaunchKernelGGL(sort_hist_kernel<true>, dim3(nb), dim3(256), 0, s, src[pass], M, shift, nb, table);
        else hipLaunchKernelGGL(sort_hist_kernel<false>, dim3(nb), dim3(256), 0, s, src[pass], M, shift, nb, table);
        hipLaunchKernelGGL(sort_scan1_kernel, dim3(chunks), dim3(256), 0, s, table, entries, totals);
        hipLaunchKernelGGL(sort_scan2_kernel, dim3(1), dim3(256), 0, s, totals, chunks);
        if (pass == 0) hipLaunchKernelGGL((sort_scatter_kernel<true, false>), dim3(nb), dim3(256), 0, s, src[pass], M, shift, nb, table, totals, dst[pass]);
        else if (pass == 3) hipLaunchKernelGGL((sort_scatter_kernel<false, true>), dim3(nb), dim3(256), 0, s, src[pass], M, shift, nb, table, totals, dst[pass]);
        else hipLaunchKernelGGL((sort_scatter_kernel<false, false>), dim3(nb), dim3(256), 0, s, src[pass], M, shift, nb, table, totals, dst[pass]);
    }
    hipLaunchKernelGGL(sort_count_kernel, dim3(1), dim3(1), 0, s, sorted_out, M, n_out);
}

void launch_rank_f32(const float* sorted, int64_t M, const int64_t* n_dev, const float* queries, int64_t N, int self, float* pct,
                     int* less, int* eq, hipStream_t s) {
    if (N < 1) return;
    const int64_t blocks = (N + 255) / 256;
    hipLaunchKernelGGL(rank_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, s, sorted, (int)M, n_dev, queries, (int)N,
                       self, pct, less, eq);
}
