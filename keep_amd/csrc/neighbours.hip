// Nearest neighbours: the k bank rows with the largest q . b for every query row, as sorted lists of 64-bit keys
// (KEEP_TOPK_KEY of include/keep_hip.h: the ordered score in the high word, 0xFFFFFFFF - global bank index in the low word, 0 = empty).
//
//   topk           a workgroup owns 64 query rows (4 waves of 16) and one segment of the bank, walked in tiles of 64 bank rows with
//                  cluster_assign_kernel's operand flow: the bank tile staged through LDS 16 k at a time, double buffered, the query rows
//                  streamed (they come back from L2 for every tile), 4 accumulators per wave on v_mfma_f32_16x16x4_f32; four steps
//                  of both operands are in flight in registers.  A score is
//                  the k-ordered fmaf chain of cluster_assign ((k / 16, k % 4, k / 4 % 4), from 0), so its bits depend on the two rows
//                  alone.  Selection: every query row keeps its k keys in LDS, descending; a lane compares its 16 scores against its
//                  rows' k-th key (a register copy); a row with survivors takes its list into registers (one key per lane), the
//                  survivors are serialised by ballot and inserted by counting rank, and the list goes back.  A wave owns its 16
//                  lists outright: no atomics, no cross-wave ordering.
//   topk_merge     the k largest keys of S lists per query row: a workgroup per row, each wave merges every fourth list into a list
//                  it holds in registers (one key per lane), wave 0 then merges the four.  It reduces the segments' partial lists and
//                  is exported to merge two lists of the same queries.
//   topk_unpack    keys -> index int64, score fp32, count int32
//   knn_vote       one wave per query: the labelled neighbours' votes, added in list order in fp32
//
// The top k of a union is the k largest keys of the union: associative and commutative, so the words do not depend on tiles,
// segments, calls or chunk order.  Row indices are int32 (Nq, M <= 2^22 per call, checked by the caller); element offsets are int64.
#include "common.h"
#include "../../include/keep_hip.h"

namespace keepk {

typedef unsigned long long topk_key_t;
constexpr int TOPK_PREFETCH = 4;                     // steps of 16 k of both operands in flight per thread

// cluster_bad's rule: true for NaN, +-inf and |x| > 1
__device__ __forceinline__ bool topk_bad4(const f32x4 v) {
    return !(fabsf(v[0]) <= 1.0f) || !(fabsf(v[1]) <= 1.0f) || !(fabsf(v[2]) <= 1.0f) || !(fabsf(v[3]) <= 1.0f);
}
// src is the same in every lane of the wave: two v_readlane, no trip through the LDS crossbar
__device__ __forceinline__ topk_key_t topk_shfl(topk_key_t v, int src) {
    const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)v, src), hi = __builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src);
    return ((topk_key_t)hi << 32) | lo;
}
// lane l takes lane l - 1's value (DPP wave_shr:1); lane 0 keeps its own, which no caller uses
__device__ __forceinline__ topk_key_t topk_shfl_up1(topk_key_t v) {
    const int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
    const unsigned ulo = __builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xF, 0xF, false), uhi = __builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xF, 0xF, false);
    return ((topk_key_t)uhi << 32) | ulo;
}
__device__ __forceinline__ topk_key_t topk_make_key(float score, unsigned g) {
    const unsigned u = __float_as_uint(score + 0.0f);                    // + 0 folds -0 into +0
    return KEEP_TOPK_KEY(KEEP_TOPK_ORD(u), g);
}
__device__ __forceinline__ float topk_key_score(topk_key_t key) {
    const unsigned o = (unsigned)(key >> 32);
    return __uint_as_float(KEEP_TOPK_SCORE_BITS(o));
}

// keys: [Nq][k] in/out (read with merge, by segment 0; written when ws is null); ws: [gridDim.y][64 gridDim.x][k] partial lists
__global__ __launch_bounds__(256)
void topk_kernel(const float* __restrict__ q, int Nq, const float* __restrict__ bank, int M, int D, int k, unsigned g_base, long long self_first,
                 int merge, int tiles_per_seg, topk_key_t* keys, topk_key_t* ws, topk_key_t* __restrict__ q_skipped,
                 topk_key_t* __restrict__ b_skipped) {
    __shared__ f32x4 sB[2][4][64];
    __shared__ topk_key_t sList[64][64];               // row's keys, descending; entries k .. 63 stay 0
    __shared__ int sColBad[64];
    __shared__ int s_qbad, s_bbad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int q0 = blockIdx.x * 64, seg = blockIdx.y;  // q0 < Nq: the grid is ceil(Nq / 64)
    const int ntiles = (M + 63) >> 6;
    const int t0 = min(ntiles, seg * tiles_per_seg), t1 = min(ntiles, t0 + tiles_per_seg);
    for (int i = tid; i < 64 * 64; i += 256) {
        const int r = i >> 6, e = i & 63;
        topk_key_t v = 0;
        if (merge && seg == 0 && e < k && q0 + r < Nq) v = keys[(int64_t)(q0 + r) * k + e];
        sList[r][e] = v;
    }
    if (tid == 0) { s_qbad = 0; s_bbad = 0; }
    __syncthreads();
    const int row_base = q0 + wave * 16;
    const bool wact = row_base < Nq;                   // a wave without a query row stages the bank and does nothing else
    const int bcol = tid >> 2, bq = tid & 3;           // one float4 of one bank row per thread and block of 16 k
    const int nblk = D >> 4;
    const float* ap = q + (int64_t)min(row_base + j, Nq - 1) * D + kq * 4;
    topk_key_t thr[4];                                 // the k-th keys of rows kq*4 + r: never above the lists' own, refreshed after inserts
#pragma unroll
    for (int r = 0; r < 4; ++r) thr[r] = sList[wave * 16 + kq * 4 + r][k - 1];
    int rowok = 0;                                     // bit r: row kq*4 + r exists and is kept (known after the first tile)
    // The walk is one sequence of steps (tile, block of 16 k) with TOPK_PREFETCH steps of both operands in flight in registers: a
    // workgroup that has the CU almost to itself (few queries, many segments) would otherwise wait a memory latency per step.
    int lt = t0, lkb = 0;                              // the load stream's tile and block
    const float* lbp = bank + (int64_t)min(t0 * 64 + bcol, M - 1) * D + bq * 4;
    auto issue = [&](f32x4& A, f32x4& B) {
        if (lt >= t1) return;
        A = *reinterpret_cast<const f32x4*>(ap + lkb * 16);
        B = *reinterpret_cast<const f32x4*>(lbp + lkb * 16);
        if (++lkb == nblk) {
            lkb = 0;
            ++lt;
            lbp = bank + (int64_t)min(lt * 64 + bcol, M - 1) * D + bq * 4;
        }
    };
    f32x4 ra[TOPK_PREFETCH], rb[TOPK_PREFETCH];
#pragma unroll
    for (int u = 0; u < TOPK_PREFETCH; ++u) {
        ra[u] = rb[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        issue(ra[u], rb[u]);
    }
    f32x4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    bool abad = false, bbad = false;
    int t = t0, kb = 0, step = 0;
    auto tile_end = [&]() {
        // threads (bcol, 0..3) read bank row bcol between them: its flag, and the rows beyond M, are never candidates
        int bb = bbad ? 1 : 0;
        bb |= __shfl_xor(bb, 1);
        bb |= __shfl_xor(bb, 2);
        if (bq == 0) {
            const bool in = t * 64 + bcol < M;
            sColBad[bcol] = (bb || !in) ? 1 : 0;
            if (bb && in && blockIdx.x == 0) atomicAdd(&s_bbad, 1);          // a bank row is counted once per call
        }
        if (t == t0 && wact) {
            // lanes (j, 0..3) read query row j between them
            int badi = abad ? 1 : 0;
            badi |= __shfl_xor(badi, 16);
            badi |= __shfl_xor(badi, 32);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int lr = kq * 4 + r;
                if (__shfl(badi, lr) == 0 && row_base + lr < Nq) rowok |= 1 << r;
            }
            if (kq == 0 && badi && row_base + j < Nq && seg == 0) atomicAdd(&s_qbad, 1);
        }
        __syncthreads();                               // sColBad
        if (!wact) return;
        const unsigned g_tile = g_base + (unsigned)(t * 64);
        int colbad[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) colbad[c] = sColBad[c * 16 + j];
        // lane (j, kq) holds query rows row_base + kq*4 + r (r = 0..3) at bank rows t*64 + c*16 + j
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long self = self_first >= 0 ? self_first + row_base + kq * 4 + r : -1;
            topk_key_t key[4];
            unsigned long long mask[4], any = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const unsigned g = g_tile + (unsigned)(c * 16 + j);
                key[c] = topk_make_key(acc[c][r], g);
                const bool pass = ((rowok >> r) & 1) && !colbad[c] && key[c] > thr[r] && (long long)g != self;
                mask[c] = __ballot(pass);
                any |= mask[c];
            }
            if (!any) continue;                    // the same in every lane: after the first tiles, almost always
            for (int grp = 0; grp < 4; ++grp) {    // the 16 lanes of a group hold ONE query row: its list comes into registers once
                if (!((any >> (16 * grp)) & 0xFFFFull)) continue;
                topk_key_t* lst = sList[wave * 16 + grp * 4 + r];
                topk_key_t e = lst[lane];          // lane l holds entry l; lanes >= k hold 0
                topk_key_t kth = topk_shfl(e, k - 1);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    unsigned m = (unsigned)(mask[c] >> (16 * grp)) & 0xFFFFu;
                    while (m) {                    // the survivors, serialised; insertion by counting rank
                        const int src = 16 * grp + __ffs(m) - 1;
                        m &= m - 1;
                        const topk_key_t x = topk_shfl(key[c], src);
                        if (x > kth) {             // thr may be stale (lower): the list decides
                            const int pos = __popcll(__ballot(e > x));   // < k
                            const topk_key_t up = topk_shfl_up1(e);
                            e = lane < pos ? e : (lane == pos ? x : up);
                            if (lane >= k) e = 0;
                            kth = topk_shfl(e, k - 1);
                        }
                    }
                }
                lst[lane] = e;                     // every lane reads and writes its own entry alone
                if (kq == grp) thr[r] = kth;
            }
        }
    };
    while (t < t1) {
#pragma unroll
        for (int u = 0; u < TOPK_PREFETCH; ++u) {
            if (t >= t1) break;                        // the same in the whole workgroup
            sB[step & 1][bq][bcol] = rb[u];
            bbad = bbad || topk_bad4(rb[u]);
            const f32x4 a = ra[u];
            __syncthreads();                           // a buffer is rewritten two steps later, after the barrier of the step between
            issue(ra[u], rb[u]);
            if (wact) {
                abad = abad || topk_bad4(a);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const f32x4 b = sB[step & 1][kq][c * 16 + j];
                    acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], acc[c], 0, 0, 0);
                    acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[1], acc[c], 0, 0, 0);
                    acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[2], acc[c], 0, 0, 0);
                    acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[3], acc[c], 0, 0, 0);
                }
            }
            ++step;
            if (++kb == nblk) {
                tile_end();
                kb = 0;
                ++t;
                bbad = false;
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        if (q_skipped && s_qbad) (void)__hip_atomic_fetch_add(q_skipped, (topk_key_t)s_qbad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (b_skipped && s_bbad) (void)__hip_atomic_fetch_add(b_skipped, (topk_key_t)s_bbad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    topk_key_t* dst = ws ? ws + ((int64_t)seg * gridDim.x * 64 + q0) * k : keys + (int64_t)q0 * k;
    const int nrows = ws ? 64 : min(64, Nq - q0);
    for (int i = tid; i < nrows * k; i += 256) dst[i] = sList[i / k][i % k];
}

// cur and src: lane l holds entry l of a descending list, lanes >= k hold 0.  cur becomes the k largest of both.
__device__ __forceinline__ void topk_merge_in(topk_key_t& cur, topk_key_t src, int k, int lane) {
    topk_key_t thr = topk_shfl(cur, k - 1);
    for (int i = 0; i < k; ++i) {
        const topk_key_t x = topk_shfl(src, i);
        if (x <= thr) break;                           // descending: nothing after it gets in either (an empty slot is 0)
        const int pos = __popcll(__ballot(cur > x));   // < k
        const topk_key_t up = topk_shfl_up1(cur);
        cur = lane < pos ? cur : (lane == pos ? x : up);
        if (lane >= k) cur = 0;
        thr = topk_shfl(cur, k - 1);
    }
}

// list 0 of row q is a + q k, list s >= 1 is b + (s - 1) b_stride + q k; out may be a
__global__ __launch_bounds__(256)
void topk_merge_kernel(const topk_key_t* a, const topk_key_t* __restrict__ b, int64_t b_stride, int S, int k, topk_key_t* out) {
    __shared__ topk_key_t sL[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t off = (int64_t)blockIdx.x * k;
    topk_key_t cur = 0;
    for (int s0 = wave; s0 < S; s0 += 32) {            // eight lists in flight
        topk_key_t src[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int s = s0 + 4 * u;
            src[u] = 0;
            if (s < S && lane < k) src[u] = s == 0 ? a[off + lane] : b[(int64_t)(s - 1) * b_stride + off + lane];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) topk_merge_in(cur, src[u], k, lane);
    }
    sL[wave][lane] = cur;
    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < 4; ++w) topk_merge_in(cur, sL[w][lane], k, lane);
    if (lane < k) out[off + lane] = cur;
}

// one wave per query row
__global__ __launch_bounds__(256)
void topk_unpack_kernel(const topk_key_t* __restrict__ keys, int Nq, int k, int64_t* __restrict__ index, float* __restrict__ score,
                        int32_t* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int qr = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qr >= Nq) return;
    const topk_key_t key = lane < k ? keys[(int64_t)qr * k + lane] : 0;
    const int n = __popcll(__ballot(key != 0));
    if (lane < k) {
        if (index) index[(int64_t)qr * k + lane] = key ? (int64_t)KEEP_TOPK_INDEX(key) : -1;
        if (score) score[(int64_t)qr * k + lane] = key ? topk_key_score(key) : 0.f;
    }
    if (count && lane == 0) count[qr] = n;
}

__global__ void knn_check_kernel(const topk_key_t* __restrict__ keys, int64_t n, int64_t n_bank, int* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const topk_key_t key = keys[i];
    if (key && (int64_t)KEEP_TOPK_INDEX(key) >= n_bank) *bad = 1;
}

// one wave per query row; lane r holds neighbour r, lane c class c
__global__ __launch_bounds__(256)
void knn_vote_kernel(const topk_key_t* __restrict__ keys, int Nq, int k, const int32_t* __restrict__ bank_labels, int C, int mode, float T,
                     float* __restrict__ probs, int32_t* __restrict__ label_out, float* __restrict__ margin_out,
                     topk_key_t* __restrict__ skipped) {
    const int lane = threadIdx.x & 63;
    const int qr = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qr >= Nq) return;
    const topk_key_t key = lane < k ? keys[(int64_t)qr * k + lane] : 0;
    int lab = -1;
    if (key) {
        const int l = bank_labels[KEEP_TOPK_INDEX(key)];
        if (l >= 0 && l < C) lab = l;
    }
    const float s = key ? topk_key_score(key) : 0.f;
    const float s0 = __shfl(s, 0);
    float w = 1.0f;
    if (mode == KEEP_KNN_SOFTMAX) w = expf((s - s0) / T);
    float v = 0.f;
    for (int r = 0; r < k; ++r) {                      // list order
        const int lr = __shfl(lab, r);
        const float wr = __shfl(w, r);
        if (lr == lane) v += wr;
    }
    float tot = 0.f;
    for (int c = 0; c < C; ++c) tot += __shfl(v, c);   // class order
    if (!(tot > 0.f)) {                                // no voting neighbour (or, at a tiny T, every voter's weight underflowed)
        if (probs && lane < C) probs[(int64_t)qr * C + lane] = 0.f;
        if (lane == 0) {
            if (label_out) label_out[qr] = -1;
            if (margin_out) margin_out[qr] = 0.f;
            if (skipped) (void)__hip_atomic_fetch_add(skipped, (topk_key_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return;
    }
    const float p = lane < C ? v / tot : -1.f;
    float v1 = lane < C ? v : -1.f;
    int i1 = lane;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {                 // the smallest class with the largest sum
        const float ov = __shfl_xor(v1, o); const int oi = __shfl_xor(i1, o);
        if (ov > v1 || (ov == v1 && oi < i1)) { v1 = ov; i1 = oi; }
    }
    const float p1 = __shfl(p, i1);
    float p2 = lane == i1 ? -1.f : p;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) p2 = fmaxf(p2, __shfl_xor(p2, o));
    if (probs && lane < C) probs[(int64_t)qr * C + lane] = p;
    if (lane == 0) {
        if (label_out) label_out[qr] = i1;
        if (margin_out) margin_out[qr] = p1 - p2;
    }
}

}  // namespace keepk
using namespace keepk;

// Segments of the bank when the query blocks alone cannot fill the chip: as many workgroups as are resident at once (three per CU: the
// lists' 32 KiB of LDS), in segments of equal tile counts and none of them empty.  Measured at D = 768, M = 100 000 (DESIGN.md section
// 28): fewer segments leave CUs idle, more of them pay the lists' first fill (k inserts per row and segment) and the merge again.
int topk_segments(int Nq, int M, int cus) {
    const int qblocks = (Nq + 63) / 64, ntiles = (M + 63) / 64;
    if (qblocks >= cus) return 1;
    int s = 3 * cus / qblocks;
    s = s < 1 ? 1 : (s > TOPK_MAX_SEGMENTS ? TOPK_MAX_SEGMENTS : s);
    const int tps = (ntiles + s - 1) / s;
    return (ntiles + tps - 1) / tps;
}

void launch_topk(const float* q, int Nq, const float* bank, int M, int D, int k, unsigned g_base, long long self_first, int merge, uint64_t* keys,
                 int64_t* q_skipped, int64_t* b_skipped, int S, uint64_t* ws, hipStream_t s) {
    const int qblocks = (Nq + 63) / 64, ntiles = (M + 63) / 64;
    const int tps = (ntiles + S - 1) / S;
    topk_key_t* w = S > 1 ? (topk_key_t*)ws : nullptr;
    hipLaunchKernelGGL(topk_kernel, dim3(qblocks, S), dim3(256), 0, s, q, Nq, bank, M, D, k, g_base, self_first, merge, tps, (topk_key_t*)keys, w,
                       (topk_key_t*)q_skipped, (topk_key_t*)b_skipped);
    if (S > 1) {
        const int64_t stride = (int64_t)qblocks * 64 * k;
        hipLaunchKernelGGL(topk_merge_kernel, dim3(Nq), dim3(256), 0, s, w, w + stride, stride, S, k, (topk_key_t*)keys);
    }
}

void launch_topk_merge(const uint64_t* a, const uint64_t* b, int Nq, int k, uint64_t* out, hipStream_t s) {
    hipLaunchKernelGGL(topk_merge_kernel, dim3(Nq), dim3(256), 0, s, (const topk_key_t*)a, (const topk_key_t*)b, (int64_t)0, 2, k, (topk_key_t*)out);
}

void launch_topk_unpack(const uint64_t* keys, int Nq, int k, int64_t* index, float* score, int32_t* count, hipStream_t s) {
    hipLaunchKernelGGL(topk_unpack_kernel, dim3((Nq + 3) / 4), dim3(256), 0, s, (const topk_key_t*)keys, Nq, k, index, score, count);
}

void launch_knn_check(const uint64_t* keys, int Nq, int k, int64_t n_bank, int* bad, hipStream_t s) {
    const int64_t n = (int64_t)Nq * k;
    hipLaunchKernelGGL(knn_check_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const topk_key_t*)keys, n, n_bank, bad);
}

void launch_knn_vote(const uint64_t* keys, int Nq, int k, const int32_t* bank_labels, int C, int mode, float T, float* probs, int32_t* label,
                     float* margin, int64_t* skipped, hipStream_t s) {
    hipLaunchKernelGGL(knn_vote_kernel, dim3((Nq + 3) / 4), dim3(256), 0, s, (const topk_key_t*)keys, Nq, k, bank_labels, C, mode, T, probs, label,
                       margin, (topk_key_t*)skipped);
}
