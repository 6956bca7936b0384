// Few-shot prototypes: SimpleShot (centre, L2-normalise, nearest class mean) over E random support sets at once.
// include/keep_hip.h states the arithmetic.
//
//   fewshot_sample       one wave per (episode, class): the first `shots` distinct draws of the bootstrap's generator (boot_rng.h), the
//                        accepted list in registers (slot s in lane s % 64, register s / 64), a draw compared against it by all lanes
//   fewshot_prototypes   ONE WORKGROUP PER EPISODE WALKS THE SLOTS IN (class, slot) ORDER: that fixes the summation order.  The slots of a
//                        class go in chunks of 256: the waves share a chunk's rows between them (the skip rule, then |s - mu|), the 256
//                        threads then add the kept rows column by column (column d in thread d % 256) in slot order.  Two passes: mu,
//                        then the class means; the dots of consts by one wave each.  No atomics but the dropped-row counter
//   fewshot_classify     topk_kernel's operand flow (neighbours.hip): a workgroup owns 64 test rows (4 waves of 16) and one segment of
//                        the episodes' tiles; a tile is 64 bank rows = floor(64 / (C + 1)) whole episodes (p_0 .. p_{C-1}, mu each) and
//                        padding, staged through LDS 16 k at a time, double buffered, the test rows streamed, FS_PREFETCH steps of both
//                        operands in flight; 4 accumulators per wave on v_mfma_f32_16x16x4_f32, the k-ordered chain of cluster_assign.
//                        After a tile the 64 x 64 dots go through LDS to one thread per (row, episode): r, the t_c, the first-maximum
//                        argmax over the valid classes, the label, one LDS add into the tile's confusion bins; the bins are flushed by
//                        one no-return 64-bit atomic per non-zero bin.  No [N, E C] matrix exists anywhere.
//
// The fp32 operations after the dots, each rounded once, in this order: a = fma(-2, x.mu, 1); b = a + |mu|^2; r = sqrt(max(b, 0));
// u = x.p_c - mu.p_c; w = h_c * r; t_c = u - w.  Wave64; integer atomics only, none with a used result.
#include "common.h"
#include "boot_rng.h"
#include "../../include/keep_hip.h"

namespace keepk {

typedef unsigned long long fs_word_t;
constexpr int FS_PREFETCH = 4;                       // steps of 16 k of both operands in flight per thread
constexpr int FS_CHUNK = 256;                        // slots of a class the prototype builder holds in LDS at once
static_assert(KEEP_FEWSHOT_MAX_SHOTS == 256, "the sampler holds four accepted draws per lane");

// cluster_bad's rule: true for NaN, +-inf and |x| > 1
__device__ __forceinline__ bool fs_bad4(const f32x4 v) {
    return !(fabsf(v[0]) <= 1.0f) || !(fabsf(v[1]) <= 1.0f) || !(fabsf(v[2]) <= 1.0f) || !(fabsf(v[3]) <= 1.0f);
}
// the 64 lanes' values added by the xor butterfly 32, 16, .. 1: the same word in every lane
__device__ __forceinline__ float fs_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o));
    return v;
}
// a . b over D columns: lane l adds d = l, l + 64, .. ascending by fmaf from 0, then the butterfly
__device__ __forceinline__ float fs_dot(const float* a, const float* b, int D, int lane) {
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s = fmaf(a[d], b[d], s);
    return fs_wave_sum(s);
}

__global__ __launch_bounds__(256)
void fewshot_sample_kernel(const int32_t* __restrict__ class_rows, const int64_t* __restrict__ class_offsets, int C, int shots,
                           unsigned long long seed, long long first_episode, int E, int32_t* __restrict__ support) {
    const int lane = threadIdx.x & 63;
    const long long pair = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= (long long)E * C) return;
    const int e = (int)(pair / C), c = (int)(pair % C);
    const int64_t off = class_offsets[c];
    const int64_t n64 = class_offsets[c + 1] - off;
    const unsigned n = n64 < 0 ? 0u : (n64 > CLUSTER_MAX_ROWS ? (unsigned)CLUSTER_MAX_ROWS : (unsigned)n64);
    int32_t* out = support + pair * shots;
    if (n <= (unsigned)shots) {                        // every row of the class, in stored order
        for (int s = lane; s < shots; s += 64) out[s] = (unsigned)s < n ? class_rows[off + s] : -1;
        return;
    }
    const unsigned long long key = boot_key(seed, (first_episode + e) * 64 + c);
    unsigned acc[4] = {0u, 0u, 0u, 0u};                // slot s: register s / 64 of lane s % 64
    int cnt = 0;
    for (unsigned j = 0; cnt < shots && j < (unsigned)KEEP_FEWSHOT_MAX_DRAWS; ++j) {
        const unsigned r = boot_draw(key, j, n);       // the same in every lane
        bool hit = false;
#pragma unroll
        for (int g = 0; g < 4; ++g) hit = hit || (g * 64 + lane < cnt && acc[g] == r);
        if (__any(hit)) continue;
#pragma unroll
        for (int g = 0; g < 4; ++g)
            if ((cnt >> 6) == g && (cnt & 63) == lane) acc[g] = r;
        ++cnt;
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int s = g * 64 + lane;
        if (s < shots) out[s] = s < cnt ? class_rows[off + acc[g]] : -1;
    }
}

__global__ __launch_bounds__(256)
void fewshot_prototypes_kernel(const float* __restrict__ train, int M, int D, const int32_t* __restrict__ support, int C, int shots, int centre,
                               float* __restrict__ bank, float* __restrict__ consts, unsigned char* __restrict__ valid,
                               fs_word_t* __restrict__ skipped) {
    __shared__ float sMu[CLUSTER_MAX_D], sP[CLUSTER_MAX_D];
    __shared__ int sRow[FS_CHUNK];                     // a chunk's kept rows, -1 for an unused or dropped slot
    __shared__ float sNorm[FS_CHUNK];
    __shared__ int sDrop;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e = blockIdx.x;
    const int32_t* sup = support + (int64_t)e * C * shots;
    float* bk = bank + (int64_t)e * (C + 1) * D;
    float* cs = consts + (int64_t)e * (2 * C + 1);
    if (tid == 0) sDrop = 0;
    // a chunk's rows under the skip rule; with norms, |s - mu| of the kept ones as well
    auto stage = [&](int c, int s0, bool norms) {
        const int ns = min(FS_CHUNK, shots - s0);
        for (int s = wave; s < ns; s += 4) {
            const int row = sup[(int64_t)c * shots + s0 + s];
            int keep = -1;
            float n2 = 0.f;
            if (row >= 0 && row < M) {
                const float* x = train + (int64_t)row * D;
                bool bad = false;
                for (int d = lane * 4; d < D; d += 256) bad = bad || fs_bad4(*reinterpret_cast<const f32x4*>(x + d));
                bad = __any(bad);
                if (!bad) {
                    keep = row;
                    if (norms) {
                        for (int d = lane; d < D; d += 64) {
                            const float v = __fsub_rn(x[d], sMu[d]);
                            n2 = fmaf(v, v, n2);
                        }
                        n2 = fs_wave_sum(n2);
                    }
                } else if (!norms && lane == 0) {
                    atomicAdd(&sDrop, 1);
                }
            }
            if (lane == 0) {
                sRow[s] = keep;
                sNorm[s] = sqrtf(n2);
            }
        }
        return ns;
    };
    // pass 1: mu
    float mu[4] = {0.f, 0.f, 0.f, 0.f};
    int nkept = 0;
    for (int c = 0; c < C; ++c)
        for (int s0 = 0; s0 < shots; s0 += FS_CHUNK) {
            __syncthreads();                           // the chunk before is read
            const int ns = stage(c, s0, false);
            __syncthreads();
            for (int s = 0; s < ns; ++s) {
                const int row = sRow[s];
                if (row < 0) continue;
                ++nkept;
                const float* x = train + (int64_t)row * D;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int d = tid + 256 * i;
                    if (d < D) mu[i] = __fadd_rn(mu[i], x[d]);
                }
            }
        }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int d = tid + 256 * i;
        mu[i] = (centre && nkept > 0) ? __fdiv_rn(mu[i], (float)nkept) : 0.f;
        if (d < D) {
            sMu[d] = mu[i];
            bk[(int64_t)C * D + d] = mu[i];
        }
    }
    __syncthreads();
    if (wave == 2) {
        const float mm = fs_dot(sMu, sMu, D, lane);
        if (lane == 0) cs[2 * C] = mm;
    }
    // pass 2: the class means of the centred, normalised rows
    for (int c = 0; c < C; ++c) {
        float p[4] = {0.f, 0.f, 0.f, 0.f};
        int m = 0;
        for (int s0 = 0; s0 < shots; s0 += FS_CHUNK) {
            __syncthreads();
            const int ns = stage(c, s0, true);
            __syncthreads();
            for (int s = 0; s < ns; ++s) {
                const int row = sRow[s];
                if (row < 0) continue;
                ++m;
                const float nrm = sNorm[s];
                if (!(nrm > 0.f)) continue;            // a row equal to mu contributes a zero row
                const float* x = train + (int64_t)row * D;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int d = tid + 256 * i;
                    if (d < D) p[i] = __fadd_rn(p[i], __fdiv_rn(__fsub_rn(x[d], mu[i]), nrm));
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int d = tid + 256 * i;
            if (m > 0) p[i] = __fdiv_rn(p[i], (float)m);
            if (d < D) {
                sP[d] = p[i];
                bk[(int64_t)c * D + d] = p[i];
            }
        }
        __syncthreads();                               // sP; it is rewritten after the next chunk's two barriers
        if (wave == 0) {
            const float mp = fs_dot(sMu, sP, D, lane);
            if (lane == 0) cs[c] = mp;
        } else if (wave == 1) {
            const float pp = fs_dot(sP, sP, D, lane);
            if (lane == 0) {
                cs[C + c] = __fmul_rn(0.5f, pp);
                valid[(int64_t)e * C + c] = m > 0 ? 1 : 0;
            }
        }
    }
    __syncthreads();
    if (tid == 0 && skipped && sDrop) (void)__hip_atomic_fetch_add(skipped, (fs_word_t)sDrop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// confusion: [E][C][C], added into; labels: [Nq][E]; scores [Nq][C], margin [Nq], dots [Nq][C + 1] with E == 1 only
__global__ __launch_bounds__(256)
void fewshot_classify_kernel(const float* __restrict__ q, int Nq, const float* __restrict__ bank, int D, const float* __restrict__ consts,
                             const unsigned char* __restrict__ valid, int E, int C, int tiles_per_seg, const int32_t* __restrict__ truth,
                             fs_word_t* __restrict__ confusion, int32_t* __restrict__ labels, float* __restrict__ scores,
                             float* __restrict__ margin, float* __restrict__ dots, fs_word_t* __restrict__ skipped) {
    __shared__ f32x4 sB[2][4][64];
    __shared__ float sS[64][65];                       // the tile's dots: [test row][bank column]
    __shared__ int sConf[64 * FEWSHOT_MAX_C];          // floor(64 / (C + 1)) C C < 64 C bins of the tile's episodes
    __shared__ int sRowBad[64];
    __shared__ int s_qbad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int q0 = blockIdx.x * 64, seg = blockIdx.y;  // q0 < Nq: the grid is ceil(Nq / 64)
    const int C1 = C + 1, ept = 64 / C1, ncols = ept * C1, CC = C * C;
    const int nbank = E * C1;
    const int ntiles = (E + ept - 1) / ept;
    const int t0 = min(ntiles, seg * tiles_per_seg), t1 = min(ntiles, t0 + tiles_per_seg);
    for (int i = tid; i < ept * CC; i += 256) sConf[i] = 0;
    if (tid == 0) s_qbad = 0;
    __syncthreads();
    const int row_base = q0 + wave * 16;
    const bool wact = row_base < Nq;                   // a wave without a test row stages the bank and does nothing else
    const int bcol = tid >> 2, bq = tid & 3;           // one float4 of one bank row per thread and block of 16 k
    const int nblk = D >> 4;
    const float* ap = q + (int64_t)min(row_base + j, Nq - 1) * D + kq * 4;
    // column bcol of tile t is bank row t ncols + bcol; a padding column and a column past the last episode read the last row (never used)
    auto bank_ptr = [&](int t) {
        int r = t * ncols + bcol;
        if (bcol >= ncols || r >= nbank) r = nbank - 1;
        return bank + (int64_t)r * D + bq * 4;
    };
    int lt = t0, lkb = 0;                              // the load stream's tile and block
    const float* lbp = bank_ptr(min(t0, ntiles - 1));
    auto issue = [&](f32x4& A, f32x4& B) {
        if (lt >= t1) return;
        A = *reinterpret_cast<const f32x4*>(ap + lkb * 16);
        B = *reinterpret_cast<const f32x4*>(lbp + lkb * 16);
        if (++lkb == nblk) {
            lkb = 0;
            ++lt;
            lbp = bank_ptr(min(lt, ntiles - 1));
        }
    };
    f32x4 ra[FS_PREFETCH], rb[FS_PREFETCH];
#pragma unroll
    for (int u = 0; u < FS_PREFETCH; ++u) {
        ra[u] = rb[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        issue(ra[u], rb[u]);
    }
    f32x4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    bool abad = false;
    int t = t0, kb = 0, step = 0;
    auto tile_end = [&]() {
        if (t == t0 && wact) {
            // lanes (j, 0..3) read test row j between them
            int badi = abad ? 1 : 0;
            badi |= __shfl_xor(badi, 16);
            badi |= __shfl_xor(badi, 32);
            if (kq == 0) {
                sRowBad[wave * 16 + j] = badi;
                if (badi && row_base + j < Nq && seg == 0) atomicAdd(&s_qbad, 1);      // a test row is counted once per call
            }
        }
        // lane (j, kq) holds test rows wave*16 + kq*4 + r (r = 0..3) at tile columns c*16 + j
        if (wact) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) sS[wave * 16 + kq * 4 + r][c * 16 + j] = acc[c][r];
        }
        __syncthreads();                               // sS, sRowBad
        const int e0 = t * ept, ne = min(ept, E - e0);
        if (wact) {
            for (int p = lane; p < 16 * ne; p += 64) { // one thread per (row, episode)
                const int lr = wave * 16 + (p & 15), ei = p >> 4;
                const int row = q0 + lr;
                if (row >= Nq) continue;
                const int e = e0 + ei;
                const float* sc = &sS[lr][ei * C1];
                const float* cs = consts + (int64_t)e * (2 * C + 1);
                const unsigned char* vl = valid + (int64_t)e * C;
                int lab = -1;
                float r = 0.f, tb = -INFINITY, t2 = -INFINITY;
                if (!sRowBad[lr]) {
                    const float a = __fmaf_rn(-2.0f, sc[C], 1.0f);
                    r = sqrtf(fmaxf(__fadd_rn(a, cs[2 * C]), 0.f));
                    if (r > 0.f) {
                        for (int c = 0; c < C; ++c) {
                            if (!vl[c]) continue;
                            const float tc = __fsub_rn(__fsub_rn(sc[c], cs[c]), __fmul_rn(cs[C + c], r));
                            if (tc > tb) {             // the first maximum wins
                                t2 = tb;
                                tb = tc;
                                lab = c;
                            } else if (tc > t2) {
                                t2 = tc;
                            }
                        }
                    }
                }
                if (labels) labels[(int64_t)row * E + e] = lab;
                if (confusion && lab >= 0) {
                    const int tr = truth[row];
                    if (tr >= 0 && tr < C) atomicAdd(&sConf[ei * CC + tr * C + lab], 1);
                }
                if (scores) {                          // E == 1
                    for (int c = 0; c < C; ++c) {
                        float v = 0.f;
                        if (lab >= 0)
                            v = vl[c] ? __fdiv_rn(__fsub_rn(__fsub_rn(sc[c], cs[c]), __fmul_rn(cs[C + c], r)), r) : -INFINITY;
                        scores[(int64_t)row * C + c] = v;
                    }
                }
                if (margin) margin[row] = (lab >= 0 && t2 > -INFINITY) ? __fdiv_rn(__fsub_rn(tb, t2), r) : 0.f;
                if (dots)
                    for (int c = 0; c < C1; ++c) dots[(int64_t)row * C1 + c] = sc[c];
            }
        }
        if (confusion) {
            __syncthreads();                           // the tile's counts are in; the next tile adds after the barrier of its first step
            for (int b = tid; b < ne * CC; b += 256) {
                const int v = sConf[b];
                if (v) {
                    (void)__hip_atomic_fetch_add(confusion + (int64_t)e0 * CC + b, (fs_word_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    sConf[b] = 0;
                }
            }
        }
    };
    while (t < t1) {
#pragma unroll
        for (int u = 0; u < FS_PREFETCH; ++u) {
            if (t >= t1) break;                        // the same in the whole workgroup
            sB[step & 1][bq][bcol] = rb[u];
            const f32x4 a = ra[u];
            __syncthreads();                           // a buffer is rewritten two steps later, after the barrier of the step between
            issue(ra[u], rb[u]);
            if (wact) {
                abad = abad || fs_bad4(a);
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
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    }
    __syncthreads();
    if (tid == 0 && skipped && s_qbad) (void)__hip_atomic_fetch_add(skipped, (fs_word_t)s_qbad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace keepk
using namespace keepk;

// Segments of the episodes' tiles when the row blocks alone cannot fill the chip: as many workgroups as are resident at once (three per
// CU: 41 KiB of LDS each), in segments of equal tile counts and none of them empty.
int fewshot_segments(int N, int E, int C, int cus) {
    const int ept = 64 / (C + 1);
    const int qblocks = (N + 63) / 64, ntiles = (E + ept - 1) / ept;
    if (qblocks >= cus) return 1;
    int s = 3 * cus / qblocks;
    s = s < 1 ? 1 : (s > TOPK_MAX_SEGMENTS ? TOPK_MAX_SEGMENTS : s);
    s = s > ntiles ? ntiles : s;
    const int tps = (ntiles + s - 1) / s;
    return (ntiles + tps - 1) / tps;
}

void launch_fewshot_sample(const int32_t* class_rows, const int64_t* class_offsets, int C, int shots, uint64_t seed, int64_t first_episode,
                           int E, int32_t* support, hipStream_t s) {
    const int64_t pairs = (int64_t)E * C;
    hipLaunchKernelGGL(fewshot_sample_kernel, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, s, class_rows, class_offsets, C, shots,
                       (unsigned long long)seed, (long long)first_episode, E, support);
}

void launch_fewshot_prototypes(const float* train, int M, int D, const int32_t* support, int E, int C, int shots, int centre, float* bank,
                               float* consts, unsigned char* valid, int64_t* skipped, hipStream_t s) {
    hipLaunchKernelGGL(fewshot_prototypes_kernel, dim3(E), dim3(256), 0, s, train, M, D, support, C, shots, centre, bank, consts, valid,
                       (fs_word_t*)skipped);
}

void launch_fewshot_classify(const float* x, int N, int D, const float* bank, const float* consts, const unsigned char* valid, int E, int C,
                             const int32_t* truth, int64_t* confusion, int32_t* labels, float* scores, float* margin, float* dots,
                             int64_t* skipped, int S, hipStream_t s) {
    const int ept = 64 / (C + 1);
    const int qblocks = (N + 63) / 64, ntiles = (E + ept - 1) / ept;
    S = S > ntiles ? ntiles : S;
    const int tps = (ntiles + S - 1) / S;
    S = (ntiles + tps - 1) / tps;
    hipLaunchKernelGGL(fewshot_classify_kernel, dim3(qblocks, S), dim3(256), 0, s, x, N, bank, D, consts, valid, E, C, tps, truth,
                       (fs_word_t*)confusion, labels, scores, margin, dots, (fs_word_t*)skipped);
}
