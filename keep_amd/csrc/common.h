// Shared device/host helpers for libkeep_hip (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef _Float16 f16;
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define KEEP_WAVE 64

// MFMA shape of the plain (not fp4-compensated) K loops of gemm_f16_v2.hip, and of the ceiling probe (keep_mfma_probe): 32 = v_mfma_f32_32x32x16_f16, 16 = v_mfma_f32_16x16x32_f16.  Same cycles per FLOP, same 12 ds_read_b128 per K tile
// and wave; under load the chip holds a higher clock on the 16 shape (profiles/mfma_shape_ladder.txt, profiles/ab_mfma_shape.txt).  A build-time property
// (KEEP_BUILD_DEFINES=-DKEEP_MFMA_SHAPE=32 for the other arm of an A/B); the compensated kernels stay on 32x32x16, whose accumulator layout their MX-fp4 phase shares.
#ifndef KEEP_MFMA_SHAPE
#define KEEP_MFMA_SHAPE 16
#endif
static_assert(KEEP_MFMA_SHAPE == 16 || KEEP_MFMA_SHAPE == 32, "KEEP_MFMA_SHAPE: 16 (16x16x32) or 32 (32x32x16)");

// fp16 has 65504 as its largest finite value: saturate instead of producing inf
// (ViT residual streams can carry outlier channels; the stream itself stays fp32).
// hi/lo split used by the "strict" (3-pass) precision mode: x ~= hi + lo with
// hi = fp16(x), lo = fp16(x - hi).  |x - hi - lo| <= 2^-22 |x| (2^-25 abs floor).
// No saturation: a value beyond the fp16 range (65504) becomes inf on purpose -- it turns into NaN at the next LayerNorm / softmax and the
// final normalisation kernel raises the handle's "non-finite features" flag (the reference computes in fp32 and would not overflow;
// clamping would return plausible garbage instead).
__device__ __forceinline__ void split_f16(float x, f16& hi, f16& lo) {
    // x is pinned as ONE materialised fp32 value.  Without this hipcc (-ffp-contract=fast) folds the multiply / fma that produced x into
    // v_fma_mixlo_f16 for the hi that feeds `lo` (exact product rounded once to fp16) while the STORED hi is v_cvt(v_mul) (rounded twice):
    // the two disagree by an fp16 ulp on a few values per thousand, and hi + lo is then 1e-3 off instead of 2^-22 (found by the split-attention
    // operator test when the saturating clamp, which happened to block the pattern, was removed).
    asm("" : "+v"(x));
    hi = (f16)x;
    lo = (f16)(x - (float)hi);
}

// Exact (erf) GELU: timm nn.GELU and HF hidden_act="gelu".
// Pillow's 8-bit resample: 22-bit fixed-point accumulator (started at 1 << 21 for rounding) -> uint8 (rowops.hip, region.hip)
__device__ __forceinline__ unsigned char clip8_fixed(int v) {
    v >>= 22;
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
__device__ __forceinline__ float gelu_erf(float x) {
    return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// ---------------------------------------------------------------------------
// K-blocked fp16 operand layout ("blk").  Every fp16 matrix that a GEMM reads as an operand (LN output,
// attention output, MLP hidden, im2col patches, all weights) is stored as
//     X[m][k]  ->  ((m / 256) * KT + k / 32) * 8192 + (m % 256) * 32 + (k % 32),     KT = K / 32
// i.e. tile-major [row tile of 256][K slice of 32][256 rows][32 k]: the 16 KiB that one workgroup needs
// for one K step of one operand is ONE contiguous block.  Measured with tools/ubench/glds_tile_bw.hip:
// the LDS-DMA stream of the 256x256 GEMM runs at 21.5 TB/s on this layout against 13.7 TB/s on
// row-major [M][K] (64-byte pieces at a 2 KiB pitch), which was what bounded the K loop.
// Rows are padded to a multiple of 256 (padding rows are never stored by a consumer).
// ---------------------------------------------------------------------------
__host__ __device__ __forceinline__ int64_t blk_off(int m, int k, int KT) {
    return ((int64_t)(m >> 8) * KT + (k >> 5)) * 8192 + ((m & 255) << 5) + (k & 31);
}
static inline size_t blk_elems(int64_t M, int64_t K) { return (size_t)((M + 255) / 256 * 256) * (size_t)K; }

// ---------------------------------------------------------------------------
// Kernel launch parameter blocks (plain structs, passed by value)
// ---------------------------------------------------------------------------

// Kernel-selection knobs.  They belong to a handle (keep_set_option) and travel inside the launch parameter blocks:
// there is no process-wide kernel state, so two handles (two GPUs, two threads) never see each other's settings.
struct KeepTune {
    int gemm_impl = 0;           // 0 auto | 128 / 256: LDS-DMA tile width 
    int gemm_skinny_m = 320;     // calls with M <= this take the register-direct split-K kernel (0: never)
    int skinny_wide = 1;         // 1: small-M calls with M >= 64 on the 128x128 / 64x64-per-wave kernel (two MFMAs per fragment loaded); 0: 32x128 tiles always (A/B)
    int gemm_splitk_tiles = 64;  // a 256x256 GEMM with fewer tiles than this is cut into K slices (0: never)
    int sgemv_m = 16;            // rows up to which the few-row fp32 kernel is used (0: never)
    int ln_impl = 2;             // 2 (default): LDS-transposed blk stores from 4-wave workgroups (one 56-register wave per SIMD: fits beside two waves of the other lane's
                                 //    persistent fc1 GEMM; +0.32 % end to end in a six-round rotated A/B, profiles/r05_ab_layernorm_workgroups.txt); 1: the same from 8-wave
                                 //    workgroups (512-byte runs: 2 % faster alone); 0: per-row stores
    int attn_waves = 16;         // 16: image-tower calls with >= 512 (image, head) pairs take the persistent double-buffered kernel (13 compute + 3 loader waves),
                                 //     everything else 8 waves per workgroup; 8 / 4: one (image, head) pair per workgroup of that many waves
    int gemm_persistent = 1;     // 1: plain 256x256 GEMMs with more tiles than CUs run as one workgroup per CU walking the tile list, the next tile's
                                 //    first three K steps prefetched under the epilogue (0: one tile per workgroup; n > 1: n workgroups, experiments)
    int gemm_ablate = 0;         // diagnostics (KEEP_DIAGNOSTICS builds only)
    long long* dbg = nullptr;    // diagnostics: per-workgroup shader-clock stamps
};

// Epilogue selector of the fp16 MFMA GEMM  C[m][n] = sum_k A[m][k] W[n][k].
enum GemmEpi : int {
    EPI_F16      = 0,   // out_f16 = acc + bias                                   (QKV)
    EPI_GELU_F16 = 1,   // out_f16 = gelu(acc + bias)                             (fc1)
    EPI_RESID_LS = 2,   // resid  += ls[n] * (acc + bias)   fp32, in place        (proj / fc2, ViT)
    EPI_PATCH    = 3,   // resid[b*(P+1)+1+p] = acc + bias + pos[1+p], P = patches_per_img  (patch embed)
    EPI_RESID_F32= 4,   // out_f32 = acc + bias + resid      (BERT pre-LN sum; may alias resid)
    EPI_PARTIAL  = 5,   // internal: fp32 partial sums of one K slice -> splitk_ws[slice][M][N] (no bias); the
                        // split-K reduce kernel of gemm_f16_skinny.hip then applies the real epilogue
    EPI_TOP2     = 6,   // prompt screening (WSI_evaluation/utils.py:107-130): columns are K classifiers x C classes (C = 2 or 4,
                        // consecutive); per (row, classifier) top-2 margin score (v1 - v2) - |v1 + v2 - 1| taken in the
                        // accumulator registers and summed over the tile's rows -> top2_partial[row slot][classifier].
                        // No logit is ever written.
};

struct GemmParams {
    const f16* a_hi; const f16* a_lo;     // activations [M][K] in blk layout (row-major for the v1 kernel); lo only when nseg==3
    const f16* w_hi; const f16* w_lo;     // weights [N][K], same layout as A
    int M, N, K;                          // K = per-segment depth; multiples: N%128==0, K%64==0
    int nseg;                             // 1: A_hi*W_hi ; 3: A_hi*W_hi + A_lo*W_hi + A_hi*W_lo
    // comp != 0: after the fp16 pass the correction terms run on the MX-fp4 pipe (quant4.h): needs the fp4 side planes
    // of both operands, K % 128 == 0, nseg == 1, and the 256x256 kernel (the small-M paths use nseg = 3 instead).
    //   2 (or any value but 1): both first-order terms  W_lo A_hi + W_hi A_lo
    //   1: the weight-rounding term W_lo A_hi only (reads plane 0 of a_q and plane 1 of w_q; K >= 512); with out_q set, writes plane 0 only
    int comp;
    const unsigned char* a_q; const unsigned char* a_sc;
    const unsigned char* w_q; const unsigned char* w_sc;
    unsigned char* out_q; unsigned char* out_sc;   // EPI_GELU_F16 with out_kt > 0: also emit the fp4 planes of the output (K = N of this GEMM)
    const float* bias;                    // [N]
    const float* ls;                      // [N]   (EPI_RESID_LS)
    const float* pos;                     // [patches_per_img + 1][N] (EPI_PATCH)
    float* resid;                         // fp32 [M'][N]
    float* out_f32;                       // EPI_RESID_F32
    f16* out_hi; f16* out_lo;             // fp16 outputs (lo optional)
    int out_kt;                           // > 0: fp16 output in blk layout with KT = out_kt (= N/32); 0: row-major [M][N]
    int patches_per_img;                  // EPI_PATCH: gh * gw (196 at 224 x 224)
    // optional LayerNorm of the updated row, fused into the split-K reduce (EPI_RESID_LS / EPI_RESID_F32, N <= 1024);
    // launch_gemm_f16 reports through its return value whether it was applied (bit 0) -- the big kernel never does
    const float* ln_gamma; const float* ln_beta; float ln_eps;
    f16* ln_out_hi; f16* ln_out_lo; float* ln_out_f32;   // fp16 in blk layout (KT = N / 32); fp32 row-major [M][N], may alias resid / out_f32
    int top2_c; float* top2_partial; int top2_kpad;   // EPI_TOP2: classes per classifier, [2 * ceil(M/256)][top2_kpad] partial sums
    int impl_hint;                        // per-call kernel choice of the caller (engine option "proj_impl"): 2128 = 256x128 tiles, 4 waves, 3-stage ring, TWO
                                          // workgroups per CU (72 KiB of LDS each) -- one workgroup's epilogue runs under the other's K loop; 0 = the default choice
    int ksplit;                           // internal (EPI_PARTIAL): number of K slices the grid is replicated over
    float* splitk_ws; size_t splitk_bytes; // scratch for the small-M split-K kernel (gemm_f16_skinny.hip); null: never used
    long long* dbg;                       // diagnostics: per-workgroup [start, first tile landed, loop end, end] shader clocks
    int ablate;                           // diagnostics only: 1 = skip staging DMA, 2 = skip MFMA loop (results wrong)
    const KeepTune* tune;                 // kernel selection of the calling handle (null: defaults)
};

int launch_gemm_f16(const GemmParams& p, int epi, hipStream_t s);             // blk-layout operands (product path); returns GEMM_DID_LN or 0
constexpr int GEMM_DID_LN = 1;
// split-K scratch: 30 MiB cover every small-M shape (M <= SKINNY_MAX_M: <= 768 + 1024 partial tiles of 32 x 128 fp32);
// the mid-size path (256x256 tiles x K slices when a GEMM has fewer tiles than CUs) needs <= 448 tiles of 256 KiB
constexpr int SKINNY_MAX_M = 1024;
constexpr size_t SKINNY_WS_BYTES = (size_t)448 * 256 * 256 * 4;
int launch_gemm_splitk_reduce(const GemmParams& p, int epi, const float* ws, int S, hipStream_t s);   // returns 0 or GEMM_DID_LN
int launch_gemm_f16_skinny(const GemmParams& p, int epi, float* ws, size_t ws_bytes, hipStream_t s);

// Attention over a fused [M][3*D] qkv buffer (token-major; q|k|v, head-major inside each).
struct AttnParams {
    const f16* qkv_hi; const f16* qkv_lo; // lo only in split mode
    f16* out_hi; f16* out_lo;             // [M][D] row-major, or blk layout when out_kt > 0
    int out_kt;
    const int64_t* mask;                  // [batch][ntok] (1 = attend) or nullptr
    int batch, ntok, heads;               // head_dim fixed at 64
    int q_rows;                           // > 0: only the first q_rows query rows of every image are computed (CLS-only last block)
    int split;                            // 0/1
    // nullable (single-pass mode only): the attention output of query row 0 (the CLS row) of image b, from the fp32 accumulators, ALSO as hi + lo
    // planes into row b of a compact [batch][D] operand in the layout of `out_*` (KEEP_ATTN_PROJ_CLS: the CLS rows' proj runs again as a split product)
    f16* cls_hi; f16* cls_lo;
    // split mode with 256 < ntok <= 512: the K / V planes (hi + lo) of more than 256 keys do not fit the LDS, so the keys are processed in two
    // windows of <= 256 (two launches) and merged like an online softmax.  part_ws: caller's scratch, batch * heads * ntok * ATT_PART_FLOATS floats
    // (unnormalised output row + running maximum + sum per query); launch_attention fills key0 / kcount / part_out / part_in itself.
    float* part_ws; size_t part_bytes;
    int key0, kcount;                     // internal: key window [key0, key0 + kcount) of this launch (kcount 0 = all keys)
    float* part_out; const float* part_in;   // internal: first window writes its partial state, second window merges it and stores the result
    float scale;                          // 1/sqrt(64)
    long long* dbg;                       // diagnostics: per-workgroup [start, staged, end] shader clocks (tools/attn_timeline.py)
    const KeepTune* tune;
};
int launch_attention(const AttnParams& p, hipStream_t s);   // returns 0 or -1 (unsupported ntok)
// Key-blocked online-softmax attention for ntok > 512 (the image tower at grids beyond 22 x 22 patches): K / V stream through an LDS double
// buffer, so the sequence length is bounded only by the 32-bit offsets.  No key mask; split, q_rows, cls_hi / cls_lo and out_kt as above
// (part_ws is not used).  A separate entry point: launch_attention's own dispatch is unchanged.  Returns 0 or -1.
int launch_attention_long(const AttnParams& p, hipStream_t s);
constexpr int ATT_PART_FLOATS = 66;       // 64 output features + maximum + sum
// The CLS query's attention probabilities of one block: out fp32 [batch][heads][ntok] = softmax_k(scale q_{b,h,0} . k_{b,h,k}) from the
// row-major qkv planes above (qkv_lo null: the hi plane alone; else every operand value is hi + lo), fp32 products and sums on the VALU.  Any ntok >= 1;
// no LDS, no scratch, no atomics.  Returns 0 or -1.
int launch_attention_cls_probs(const f16* qkv_hi, const f16* qkv_lo, int batch, int ntok, int heads, float scale, float* out, hipStream_t s);
// One block's step of the attention rollout (attention_rollout.hip): with A the block's head-mean softmax(scale q k^T) from the
// planes above (fp16 MFMA products, fp32 sums) and At = (1 - residual) A + residual I, r_out = At r_in in exact fp32, or At itself when r_in is null.
// r_in, r_out: fp32 [batch][ntok][ntok] row-major; q_rows = 1: only the CLS row, r_out [batch][ntok] (q_rows = 0: every row).  a_tmp: At's way from the
// first kernel to the product, fp32 [batch][ntok or q_rows][ntok], needed when r_in is given.  1 <= ntok <= ROLLOUT_MAX_TOKENS.  Returns 0 or -1.
constexpr int ROLLOUT_MAX_TOKENS = 272;   // 17 key tiles of 16 in registers: every tile up to 256 x 256 pixels (257 tokens)
int launch_attention_rollout_step(const f16* qkv_hi, const f16* qkv_lo, int batch, int ntok, int heads, float scale, float residual,
                                  const float* r_in, float* r_out, int q_rows, float* a_tmp, hipStream_t s);

// LayerNorm over rows of D in {768,1024}; fp32 in, fp16 (hi[,lo]) and/or fp32 out.
struct LnParams {
    const float* x; int64_t x_stride;     // row stride in elements
    const float* add;                     // optional second addend (same stride as x)   [unused when null]
    const float* gamma; const float* beta;
    int rows, D; float eps;
    f16* out_hi; f16* out_lo;             // [rows][D] dense (nullable); blk layout when out_kt > 0
    int out_kt;
    float* out_f32; int64_t out_f32_stride;   // nullable
    unsigned char* out_q; unsigned char* out_sc;   // nullable: fp4 side planes of the output (quant4.h), blk path only; needs out_lo semantics internally
    int out_q_hi_only;                    // 1: only plane 0 (Q(x_hi)) and its scales are written (the consumer is a one-term compensated GEMM)
    const KeepTune* tune;
};
int launch_layernorm(const LnParams& p, hipStream_t s);

// fp32 "NT" GEMM on the f32 MFMA: out[m][n] = act(scale * sum_k A[m][k] B[n][k] + bias[n])
enum SgemmAct : int { ACT_NONE = 0, ACT_GELU = 1, ACT_TANH = 2 };
struct SgemmParams {
    const float* a; int64_t lda;
    const float* b; int64_t ldb;
    float* out; int64_t ldo;
    const float* bias;                    // nullable
    int M, N, K;                          // K % 16 == 0
    float scale; int act;
    const KeepTune* tune;
};
int launch_sgemm_f32(const SgemmParams& p, hipStream_t s);

// 256 threads: exclusive prefix of v over the block; *total = the block's sum.  s: 256 ints of LDS, reusable on return.
__device__ __forceinline__ int block_exclusive_scan256(int v, int* s, int* total) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int a = t >= o ? s[t - o] : 0;
        __syncthreads();
        s[t] += a;
        __syncthreads();
    }
    const int incl = s[t];
    *total = s[255];
    __syncthreads();
    return incl - v;
}

// Slide-region front end (region.hip): patch grid + tissue rule + stable compaction, patch gather.
// keep: ncells bytes, counts / offsets: ceil(ncells / 2048) ints each; tmp (patch != 224): B * patch * 224 * 3 bytes
void launch_region_grid(const unsigned char* region, int64_t row_stride, int ps, int gx, int64_t ncells, int patch, int step, int sat_min,
                        int min_pixels, unsigned char* keep, int* counts, int* offsets, int32_t* cell_xy, int64_t* n_out, hipStream_t s);
void launch_region_check_cells(const int32_t* cell_xy, int B, int64_t H, int64_t W, int patch, int* bad, hipStream_t s);   // *bad = 1 if a cell is outside
void launch_region_patches_u8(const unsigned char* region, int64_t row_stride, int ps, const int32_t* cell_xy, int B, int patch,
                              const int* xb, const int* xk, int xks, const int* yb, const int* yk, int yks, unsigned char* tmp,
                              unsigned char* out, hipStream_t s);
// the stable compaction alone: keep [ncells] flags (null: every cell) -> the kept cells' (x, y) in grid order + the device count
void launch_region_compact(const unsigned char* keep, int gx, int64_t ncells, int step, int* counts, int* offsets, int32_t* cell_xy,
                           int64_t* n_out, hipStream_t s);
constexpr int REGION_MAX_PATCH = 32768;
constexpr int REGION_GRID_CHUNK = 2048;                 // cells per block of the compaction

// Thumbnail tissue segmentation and the grid on a mask (tissue.hip)
constexpr int64_t TISSUE_MAX_PIXELS = (int64_t)1 << 30;   // int32 pixel indices and areas
// uint8 RGB / RGBA thumbnail -> ksize x ksize median of the saturation (bytes) and its histogram (added into hist: the caller zeroes it); -1: ksize unsupported
int launch_tissue_median_hist(const unsigned char* thumb, int64_t row_stride, int ps, int h, int w, int ksize, unsigned char* med, int* hist,
                              hipStream_t s);
// median bytes -> {0,1} mask: > thr, closing, holes <= min_hole filled, components <= min_area dropped.  tmp: h w bytes; labels, info:
// h w int32 each; err: the handle's sticky error word (value 4: a labelling loop hit its cap)
void launch_tissue_mask(const unsigned char* med, int h, int w, int thr, int close, int min_hole, int min_area, unsigned char* tmp, int* labels,
                        int* info, int* err, unsigned char* mask, hipStream_t s);
void launch_tissue_grid_cells(const unsigned char* mask, int64_t mh, int64_t mw, int64_t ds, int gx, int64_t ncells, int patch, int step,
                              int64_t ox, int64_t oy, int mode, unsigned char* keep, hipStream_t s);

// Macenko stain normalisation (stain.hip).  img / mask as above: a strided RGB / RGBA view and a nullable {0,1}
// mask [mh,mw] one pixel of which covers ds x ds image pixels (outside the mask: not allowed).  od_q: int32 [256] on the device.
constexpr int STAIN_MOMENTS = 10;                       // n, S_r, S_g, S_b, S_rr, S_rg, S_rb, S_gg, S_gb, S_bb
constexpr int STAIN_ANGLE_BINS = 4096;                  // equal bins of [-pi, pi); the direction table holds the first quarter
constexpr int STAIN_CONC_BINS = 4096, STAIN_CONC_SHIFT = 17;   // Q26 >> 17: bins 1 / 512 wide over 0 .. 8
constexpr int STAIN_LUT_MAX = 8192;                     // bytes of the exp table in LDS (8 OD units in Q10) beside the 3 KiB of od tables
constexpr int64_t STAIN_T_MAX = (int64_t)64 << 14;      // |T_q|: keeps the apply's split products inside an int32
// all three add into their output (the caller zeroes it); v_q [3][2], minv_q [2][3] and t_q [3][3] are HOST arrays, passed by value
void launch_stain_moments(const unsigned char* img, int64_t row_stride, int ps, int h, int w, const unsigned char* mask, int64_t mh, int64_t mw,
                          int64_t ds, const int* od_q, int beta_q, int64_t* out, hipStream_t s);
void launch_stain_angle_hist(const unsigned char* img, int64_t row_stride, int ps, int h, int w, const unsigned char* mask, int64_t mh,
                             int64_t mw, int64_t ds, const int* od_q, int beta_q, const int* v_q, const int* dirs, int* hist, hipStream_t s);
void launch_stain_conc_hist(const unsigned char* img, int64_t row_stride, int ps, int h, int w, const unsigned char* mask, int64_t mh,
                            int64_t mw, int64_t ds, const int* od_q, const int* minv_q, int* hist, hipStream_t s);
void launch_stain_apply_u8(const unsigned char* src, unsigned char* dst, int64_t n, const int* od_q, const int* t_q, const unsigned char* exp_lut,
                           int lut_len, int lo, hipStream_t s);

// Tile quality control (quality.hip).  blob: int32 [QUAL_BLOB_WORDS] on the device: sat_min, white_min, dark_max, the
// number of pen boxes, the index of the first box of class 1, 2 and 3 (the boxes are sorted by class), 0, then three tables of 256 words:
// bit i of table c's word v is set iff box i holds the value v in channel c.
constexpr int QUAL_COLS = 12;                           // pen 0..3, dark, glass, tissue, S L, S L^2, n_t, S L and S L^2 over tissue
constexpr int QUAL_BLOB_HEAD = 8, QUAL_BLOB_WORDS = QUAL_BLOB_HEAD + 3 * 256;
constexpr int QUAL_MAX_PATCH = 1024, QUAL_MAX_BOXES = 32;
constexpr int QUAL_BAND_PIXELS = 16384;                 // a workgroup's band of rows holds at most this many pixels (or one row)
constexpr int QUAL_GREY_BYTES = 19456, QUAL_TIS_BYTES = 4352;   // LDS of the largest band: (R + 2) (4 G + 8) <= 18720 (patch 1024), R G <= 4224 (patch 128)
constexpr int64_t QUAL_MAX_CELLS = ((int64_t)1 << 24) - 1;     // cells x bands (<= 128) is the grid
// adds into out [n][QUAL_COLS] (the caller zeroes it); every cell lies inside the region (the caller checks); -1: the patch does not fit the LDS plan
int launch_region_quality(const unsigned char* region, int64_t row_stride, int ps, const int32_t* cells, int64_t n, int patch, const int* blob,
                          int64_t* out, hipStream_t s);
// one class byte per pixel: 0 none, 1..4 pen class + 1, 5 dark, 6 glass, 7 tissue
void launch_pen_mask(const unsigned char* img, int64_t row_stride, int ps, int h, int w, const int* blob, unsigned char* out, hipStream_t s);

// the labelling alone: foreground components of img, 8- or 4-connected -> labels[p] = the component's smallest pixel index (-1 on the
// background), info[root] = area | CC_BORDER (labelling.h)
void launch_cc_label(const unsigned char* img, int h, int w, int conn8, int* labels, int* info, int* err, hipStream_t s);

// Region table (components.hip)
constexpr int REGIONS_COLS = 14;
constexpr int REGIONS_SCAN_CHUNK = 2048;               // pixels per block of the rank scan
// mask -> dense labels 1..n in the order of the components' first pixels, components of < min_area pixels dropped; *n_out = n.
// roots, info: h w int32 each; counts / offsets: ceil(h w / REGIONS_SCAN_CHUNK) ints each
void launch_regions_label(const unsigned char* mask, int h, int w, int conn8, int min_area, int* roots, int* info, int* counts, int* offsets,
                          int* err, int* labels_out, int64_t* n_out, hipStream_t s);
// labels (values outside 1..n count as background) + acc (nullable) -> table [n][REGIONS_COLS]
void launch_regions_table(const int* labels, int h, int w, int64_t n, const int64_t* acc, int64_t* table, hipStream_t s);

// Region outlines (outline.hip)
constexpr int64_t OUTLINE_MAX_PIXELS = (int64_t)1 << 28;  // an edge slot 4 p + side fits an int32 with a bit to spare
constexpr int OUTLINE_COLS = 8;
constexpr int OUTLINE_CHUNK = 2048;                     // pixels / edges per block of the scans
constexpr int OUTLINE_FLAG_WORDS = 96;                  // the per-round flags of both jumping passes and their picks
constexpr int OUTLINE_MAX_WIDTH = 16;
size_t outline_count_workspace_bytes(int64_t npix);
// counts_out[0] = E (edges), counts_out[1] = V (corner edges)
void launch_outline_count(const int* labels, int H, int W, int n, unsigned char* ws, int64_t* counts_out, hipStream_t s);
size_t outline_trace_workspace_bytes(int64_t npix, int64_t E);
// E, V as read back from launch_outline_count (E >= 1); all V vertices, the first min(R, ring_cap) ring rows, *r_out = R
void launch_outline_trace(const int* labels, int H, int W, int n, int conn8, int E, int64_t V, unsigned char* ws, int* vertices, int64_t* rings,
                          int64_t ring_cap, int64_t* r_out, hipStream_t s);
// rowok: H W bytes; rgb_out may be rgb_in
void launch_outline_draw(const int* labels, int H, int W, const unsigned char* rgb_in, unsigned char* rgb_out, unsigned color, int width,
                         unsigned char* rowok, hipStream_t s);

// Polygon annotations to masks (annotation.hip)
constexpr int64_t POLY_MAX_COORD = (int64_t)1 << 26;      // every coordinate and origin component: the products of the fill fit an int64
constexpr int64_t POLY_MAX_CELLS = (int64_t)1 << 28;      // h (w + 1): int32 indices into delta
constexpr int64_t POLY_MAX_VERTICES = (int64_t)1 << 24;
constexpr int64_t POLY_MAX_RINGS = (int64_t)1 << 20;
constexpr int64_t POLY_MAX_DOWNSAMPLE = 4096;
constexpr int64_t POLY_MAX_CROSSINGS = (int64_t)1 << 31;  // exclusive
constexpr int POLY_CHUNK = 2048;                        // vertices per block of the edge pass
size_t poly_fill_workspace_bytes(int64_t h, int64_t w, int64_t V);
// zeroes delta, counts and scans the crossings of every edge (V >= 3, R >= 1) -> the device address of their total C inside ws
const int64_t* launch_poly_count(const int64_t* vertices, int64_t V, const int64_t* ring_start, int64_t R, const int* weight, int64_t d, int h,
                                 int w, int64_t ox, int64_t oy, unsigned char* ws, hipStream_t s);
// C as read back from launch_poly_count, 1 <= C < 2^31: every crossing added into delta
void launch_poly_crossings(const int64_t* vertices, int64_t V, int64_t d, int h, int w, int64_t ox, int64_t oy, int64_t C, unsigned char* ws,
                           hipStream_t s);
// the rows of delta (the head of ws) scanned, the inside test, out; out may be into
void launch_poly_rows(int h, int w, int evenodd, int value, const unsigned char* into, unsigned char* out, unsigned char* ws, hipStream_t s);
void launch_mask_tile_counts(const unsigned char* mask, int h, int w, int64_t d, int64_t ox, int64_t oy, const int64_t* coords, int64_t N,
                             int64_t patch, int32_t* counts, hipStream_t s);

// Tile scores rasterised onto the thumbnail (heatmap.hip).  acc: one 64-bit word per raster pixel, bits 0..39 the sum
// of the 16-bit fixed-point values of the covering tiles, bits 40..63 their number
constexpr int64_t HEAT_MAX_PIXELS = (int64_t)1 << 30;     // int32 pixel indices
constexpr int64_t HEAT_MAX_TILES = ((int64_t)1 << 24) - 1;  // the count field; (2^24 - 1) 65535 < 2^40, so neither field can overflow
constexpr int64_t HEAT_MAX_PATCH = (int64_t)1 << 30;
// adds every tile's footprint into acc (integer atomics; the caller zeroes acc when it starts a raster)
void launch_heat_accumulate(const int64_t* coords, const float* values, int64_t n, int64_t patch, int64_t d, int h, int w, int64_t ox,
                            int64_t oy, int64_t* acc, hipStream_t s);
// the same with one value per cell of every tile's gh x gw grid: values fp32 [n][gh gw], row-major (y, x); patch % gw == 0, patch % gh == 0 and
// d <= min(patch / gw, patch / gh) are the caller's to check
constexpr int64_t HEAT_MAX_CELLS = (int64_t)1 << 24;      // cells per tile
void launch_heat_accumulate_cells(const int64_t* coords, const float* values, int64_t n, int gh, int gw, int64_t patch, int64_t d, int h, int w,
                                  int64_t ox, int64_t oy, int64_t* acc, hipStream_t s);
// any of mean / count / pred may be null
void launch_heat_mean(const int64_t* acc, int h, int w, float uncovered, float* mean, int* count, unsigned char* pred, hipStream_t s);
// thumb null: the constant bg (R | G << 8 | B << 16); mask null: every pixel
void launch_heat_render(const int64_t* acc, int h, int w, const unsigned char* thumb, int64_t row_stride, int ps, unsigned bg,
                        const unsigned char* mask, const unsigned char* lut, int alpha, int lo16, int hi16, int min16, unsigned char* out,
                        hipStream_t s);
// Gaussian smoothing under the support.  taps: int32 [2 radius + 1] on the device; rowa (h w uint32) and rowb
// (h w uint16) hold the row pass; out must not be acc
constexpr int HEAT_SMOOTH_MAX_RADIUS = 127;
void launch_heat_smooth(const int64_t* acc, int h, int w, const unsigned char* mask, const int* taps, int radius, unsigned* rowa,
                        unsigned short* rowb, int64_t* out, hipStream_t s);

// The subtype map (classmap.hip).  acc: C planes of the accumulator word above, [C][h][w]
constexpr int CLASS_MAX = 64;                           // one lane of a wave per class
// adds every tile's footprint into all C planes (integer atomics; the caller zeroes acc when it starts a raster); values fp32 [n][C]
void launch_class_accumulate(const int64_t* coords, const float* values, int64_t n, int C, int64_t patch, int64_t d, int h, int w, int64_t ox,
                             int64_t oy, int64_t* acc, hipStream_t s);
// mask may be null; any of label / top / margin may be null
void launch_class_argmax(const int64_t* acc, int C, int h, int w, const unsigned char* mask, int min16, int margin16, unsigned char* label,
                         int64_t* top, int64_t* margin, hipStream_t s);
// out: int64 [(C + 1)^2], zeroed here; within may be null; a and b may be the same map
void launch_class_confusion(const unsigned char* a, const unsigned char* b, const unsigned char* within, int h, int w, int C, int64_t* out,
                            hipStream_t s);
// thumb null: the constant bg (R | G << 8 | B << 16); strength null: the plain alpha; palette: uint8 [C][3]
void launch_class_render(const unsigned char* label, int h, int w, int C, const unsigned char* thumb, int64_t row_stride, int ps, unsigned bg,
                         const unsigned char* palette, int alpha, const int64_t* strength, int lo16, int hi16, unsigned char* out, hipStream_t s);

// Tile clustering (cluster.hip).  x: fp32 [N][D] unit rows, cen: fp32 [K][D]; sums int64 [K][D], counts int64 [K]
constexpr int CLUSTER_MAX_K = 64;                       // every result fits a class raster (CLASS_MAX)
constexpr int CLUSTER_MAX_D = 1024;                     // four columns per thread of the accumulate walk
constexpr int64_t CLUSTER_MAX_ROWS = (int64_t)1 << 22;  // per call; 2^24 rows of |x| 2^30 <= 2^30 fit an int64 sum with room to spare
constexpr int CLUSTER_MAX_GROUPS = 4;                   // groups of 64 rows per workgroup
// label / best / margin / prev / skipped / changed may be null; sums, counts and cos_sum all or none; two_launch (with sums) needs label
// and best.  Everything is added into skipped / changed / sums / counts / cos_sum: the caller zeroes them.
void launch_cluster_assign(const float* x, int N, int D, const float* cen, int K, int32_t* label, float* best, float* margin, const int32_t* prev,
                           int64_t* skipped, int64_t* changed, int64_t* sums, int64_t* counts, int64_t* cos_sum, int two_launch, hipStream_t s);
// empty: uint8 [K], may be null
void launch_cluster_update(const int64_t* sums, const int64_t* counts, int K, int D, float* cen, unsigned char* empty, hipStream_t s);
// centre fp32 [D], or null and centre_row one int64 on the device; ws: 8 bytes
void launch_cluster_seed_step(const float* x, int N, int D, const float* centre, const int64_t* centre_row, int first, float* nearest,
                              unsigned char* ws, int64_t* index_out, hipStream_t s);

// Linear probe (probe.hip).  x: fp32 [N][D] unit rows, w: fp32 [C][D], bias: fp32 [C]; the limits on N and D are
// those of the clustering above.
constexpr int PROBE_MAX_C = 64;
constexpr int PROBE_MAX_GROUPS = 4;                     // groups of 64 rows per workgroup
constexpr int PROBE_MAX_GROUP_TILES = 8;                // groups x ceil(C / 16) of a gradient launch: its residuals have 32 KB of LDS
// groups: 0 (probe_groups chooses), 1, 2 or 4.  grad null: the forward alone (labels, class_weight, gbias, loss, counts unused); otherwise
// labels int32 [N], class_weight fp32 [C] or null, and grad int64 [C][D], gbias int64 [C], loss int64 [1], counts int64 [C] are ADDED
// into.  probs / label / best / margin / skipped may be null.
int probe_groups(int N, int C, bool grad);
void launch_probe(const float* x, int N, int D, const float* w, const float* bias, int C, int groups, const int32_t* labels,
                  const float* class_weight, float* probs, int32_t* label, float* best, float* margin, int64_t* skipped, int64_t* grad,
                  int64_t* gbias, int64_t* loss, int64_t* counts, hipStream_t s);
// *bad = 1 for a label outside -1 .. C - 1 or a class weight (may be null) outside (0, 1]
void launch_probe_check(const int32_t* labels, int N, int C, const float* class_weight, int* bad, hipStream_t s);

// Attention MIL (mil.hip).  x: fp32 [N][D] unit rows with the limits of the clustering above; chunks: int32
// [n_chunks][3] of (bag, first row, rows <= KEEP_MIL_CHUNK), checked by launch_mil_check before any other launch reads it.
constexpr int MIL_MAX_L = 128;                          // hidden units: a multiple of 16 in 16 .. 128
constexpr int64_t MIL_MAX_BAGS = (int64_t)1 << 16;      // per call, and in all into one set of accumulators
// *bad = 1 for a chunk outside [0, S) x [0, N) or with rows outside 1 .. KEEP_MIL_CHUNK
void launch_mil_check(const int32_t* chunks, int n_chunks, int N, int S, int* bad, hipStream_t s);
// s_out fp32 [N] (-inf for a skipped row), h_out fp32 [N][L] or null; skipped_rows is ADDED into
void launch_mil_scores(const float* x, int N, int D, const float* V, const float* bv, const float* w, int L, float* s_out, float* h_out,
                       int64_t* skipped_rows, hipStream_t s);
// mkey int32 [S], Z int64 [S], P int64 [S][D]: workspace, set here.  a_out fp32 [N], z_out fp32 [S][D], kept_rows int32 [S]; y and
// head_labels (int32 [S]) may be null; skipped_bags is ADDED into
void launch_mil_pool(const float* x, int N, int D, const float* s_in, const int32_t* chunks, int n_chunks, int S, const int32_t* y, int* mkey,
                     int64_t* Z, int64_t* P, float* a_out, float* z_out, int32_t* kept_rows, int32_t* head_labels, int64_t* skipped_bags,
                     hipStream_t s);
// dz fp32 [S][D], u fp32 [S], ds fp32 [N]: workspace; cw may be null; gV int64 [L][D], gbv and gw int64 [L] are ADDED into
void launch_mil_backward(const float* x, int D, const int32_t* chunks, int n_chunks, int S, const int32_t* head_labels, const float* probs,
                         const float* Wc, int C, const float* cw, const float* w, int L, const float* s_in, const float* a, const float* z,
                         const float* hbuf, float* dz, float* u, float* ds, int64_t* gV, int64_t* gbv, int64_t* gw, hipStream_t s);

// Feature PCA (pca.hip).  x: fp32 [N][D] unit rows with the limits of the clustering above.
constexpr int PCA_MAX_K = 64;
constexpr int PCA_MAX_GROUPS = 64;                      // chunks a workgroup of the Gram kernel walks
// sum int64 [D], count int64 [1], gram int64 [D][D] (null: sum and count alone), skipped (may be null) are ADDED into; centre fp32 [D] or
// null; kept_ws: N bytes of workspace (the rows' flags); groups: 0 (chosen there) or the chunks per workgroup
void launch_pca_moments(const float* x, int N, int D, const float* centre, int64_t* sum, int64_t* count, int64_t* gram, int64_t* skipped,
                        unsigned char* kept_ws, int groups, hipStream_t s);
// w fp32 [K][D]; bias / scale fp32 [K] or null; out fp32 [N][K]; kept_out uint8 [N] and skipped (ADDED into) may be null
void launch_pca_project(const float* x, int N, int D, const float* w, int K, const float* bias, const float* scale, float* out,
                        unsigned char* kept_out, int64_t* skipped, hipStream_t s);
// acc: the class raster [C][h][w]; planes: three plane indices on the host; thumb / mask may be null
void launch_class_render_rgb(const int64_t* acc, int h, int w, const int* planes, const unsigned char* thumb, int64_t row_stride, int ps,
                             unsigned bg, const unsigned char* mask, int alpha, unsigned char* out, hipStream_t s);

// Exact t-SNE (tsne.hip).  Every buffer is the caller's; y: fp32 [N][2], N <= TSNE_MAX_ROWS.
constexpr int TSNE_MAX_ROWS = 1 << 20;
constexpr float TSNE_MAX_EXAGGERATION = 32.f;           // keeps the squared gradient norm's word inside 63 bits
// index int64 [N][k], score fp32 [N][k], count int32 [N] (the lists of topk_unpack) -> p_out fp32 [N][k]
void launch_tsne_affinities(const int64_t* index, const float* score, const int32_t* count, int N, int k, float perplexity, float* p_out,
                            hipStream_t s);
// partials fp32 [ceil(N / KEEP_TSNE_SEGMENT)][N][4]
void launch_tsne_repulsion(const float* y, int N, float* partials, hipStream_t s);
// sums int64 [3] is ADDED into; rz fp32 [N][4] scratch; grad_out may be null; update / gains / y_out all null or none
void launch_tsne_step(const float* y, int N, const float* partials, const int32_t* row_ptr, const int32_t* col, const float* val, int nnz,
                      float exaggeration, float momentum, float lr, int stats, int64_t* sums, float* rz, float* grad_out, float* update,
                      float* gains, float* y_out, hipStream_t s);

// Nearest neighbours (neighbours.hip).  q: fp32 [Nq][D] and bank: fp32 [M][D] unit rows with the limits of the
// clustering above; keys: uint64 [Nq][k] descending lists of KEEP_TOPK_KEY words, 1 <= k <= TOPK_MAX_K.
constexpr int TOPK_MAX_K = 64;                          // a list is one key per lane of a wave
constexpr int TOPK_MAX_SEGMENTS = 1024;
int topk_segments(int Nq, int M, int cus);
// S segments; ws: S ceil64(Nq) k keys when S > 1 (unused otherwise); g_base: global index of bank row 0; self_first < 0: no exclusion;
// q_skipped / b_skipped may be null and are ADDED into
void launch_topk(const float* q, int Nq, const float* bank, int M, int D, int k, unsigned g_base, long long self_first, int merge, uint64_t* keys,
                 int64_t* q_skipped, int64_t* b_skipped, int S, uint64_t* ws, hipStream_t s);
void launch_topk_merge(const uint64_t* a, const uint64_t* b, int Nq, int k, uint64_t* out, hipStream_t s);     // out may be a
void launch_topk_unpack(const uint64_t* keys, int Nq, int k, int64_t* index, float* score, int32_t* count, hipStream_t s);   // outputs may be null
void launch_knn_check(const uint64_t* keys, int Nq, int k, int64_t n_bank, int* bad, hipStream_t s);           // *bad = 1 for an index >= n_bank
void launch_knn_vote(const uint64_t* keys, int Nq, int k, const int32_t* bank_labels, int C, int mode, float T, float* probs, int32_t* label,
                     float* margin, int64_t* skipped, hipStream_t s);

// Few-shot prototypes (fewshot.hip).  Feature rows with the limits of the clustering above.
constexpr int FEWSHOT_MAX_C = 63;                       // an episode's C + 1 bank rows fit one tile of 64
constexpr int64_t FEWSHOT_MAX_EPISODES = (int64_t)1 << 16;
// support: int32 [E][C][shots], shots <= KEEP_FEWSHOT_MAX_SHOTS
void launch_fewshot_sample(const int32_t* class_rows, const int64_t* class_offsets, int C, int shots, uint64_t seed, int64_t first_episode,
                           int E, int32_t* support, hipStream_t s);
// bank fp32 [E][C + 1][D], consts fp32 [E][2 C + 1], valid uint8 [E][C]; skipped may be null and is ADDED into
void launch_fewshot_prototypes(const float* train, int M, int D, const int32_t* support, int E, int C, int shots, int centre, float* bank,
                               float* consts, unsigned char* valid, int64_t* skipped, hipStream_t s);
int fewshot_segments(int N, int E, int C, int cus);
// S segments of the episodes' tiles; truth / confusion both or neither; confusion and skipped are ADDED into; scores / margin / dots with
// E == 1 only; every output may be null
void launch_fewshot_classify(const float* x, int N, int D, const float* bank, const float* consts, const unsigned char* valid, int E, int C,
                             const int32_t* truth, int64_t* confusion, int32_t* labels, float* scores, float* margin, float* dots,
                             int64_t* skipped, int S, hipStream_t s);

// Sorted score population and rank percentiles (rank.hip)
constexpr int SORT_TILE = 4096;                         // keys per block; up to this many are sorted by one block in LDS
constexpr int SORT_SCAN_CHUNK = 2048;                   // entries of the digit table per block of the scan
constexpr int64_t SORT_MAX = ((int64_t)1 << 24) - 1;
// bytes of workspace for M values (0 up to SORT_TILE) and where the digit table and the chunk totals start in it
size_t sort_workspace_bytes(int64_t M, size_t* table_off, size_t* totals_off);
void launch_sort_f32(const float* values, int64_t M, unsigned char* ws, float* sorted_out, int64_t* n_out, hipStream_t s);
// any of pct / less / eq may be null
void launch_rank_f32(const float* sorted, int64_t M, const int64_t* n_dev, const float* queries, int64_t N, int self, float* pct,
                     int* less, int* eq, hipStream_t s);

// Segmentation evaluation (eval.hip)
constexpr int EVAL_SCAN_CHUNK = 2048;                   // entries per block of the scan over the distinct-score flags
constexpr int EVAL_BEST_BLOCKS = 1024;                  // blocks (and candidates) of the best-threshold reduction
constexpr int EVAL_HIST_BINS = 65537;                   // per truth value: the means 0..65535, then the uncovered pixels
constexpr int EVAL_ROC_SCALARS = 8;
size_t eval_roc_workspace_bytes(int64_t N, bool own_curve);
// scalars: int64 [EVAL_ROC_SCALARS]; thr / fps / tps / kept: N entries each, or all null (the curve then lives in ws)
void launch_eval_roc(const float* scores, const unsigned char* labels, int64_t N, unsigned char* ws, int64_t* scalars, float* thr, int* fps,
                     int* tps, unsigned char* kept, hipStream_t s);
// out: int64 [4], zeroed here; within may be null
void launch_eval_mask_counts(const unsigned char* a, const unsigned char* b, const unsigned char* within, int64_t n, int64_t* out, hipStream_t s);
// hist: int64 [2][EVAL_HIST_BINS], zeroed here; within may be null
void launch_eval_raster_hist(const int64_t* acc, const unsigned char* truth, const unsigned char* within, int64_t n, int64_t* hist, hipStream_t s);

// Bootstrap resampling (bootstrap.hip)
constexpr int BOOT_LDS_GROUPS = 8192;                   // = KEEP_BOOT_LDS_GROUPS: distinct scores up to which a replicate's 2 K counters live in LDS (64 KiB)
constexpr size_t BOOT_SLAB_BYTES = (size_t)256 << 20;   // above it: all the workgroups' slabs of 8 N bytes together (never less than one slab)
constexpr int64_t BOOT_MAX_REPLICATES = (int64_t)1 << 20;
constexpr int BOOT_MAX_CLASSES = 16;                    // C^2 <= 256: a draw's (truth, pred) is one byte
size_t boot_roc_workspace_bytes(int64_t N, int64_t B);
// out: int64 [B][4] (n, P_b, Nn_b, U2_b), row r = replicate first + r (first >= -1; -1 = the sample itself)
void launch_boot_roc(const float* scores, const unsigned char* labels, int64_t N, unsigned long long seed, int64_t first, int64_t B,
                     unsigned char* ws, int64_t* out, hipStream_t s);
size_t boot_confusion_workspace_bytes(int64_t N);
// out: int64 [B][C][C]; labels >= C are clamped to C - 1 (the entry point's precondition rules them out)
void launch_boot_confusion(const unsigned char* truth, const unsigned char* pred, int64_t N, int C, unsigned long long seed, int64_t first,
                           int64_t B, unsigned char* ws, int64_t* out, hipStream_t s);

// Row-wise helpers (rowops.hip)
// pixels [B,3,16 gh,16 gw] (or uint8 [B,16 gh,16 gw,3]) -> patches [B * gh * gw][768], row-major (y, x) patch order; CLS rows of resid
void launch_im2col(const void* pixels, int dtype, int B, int gh, int gw, f16* out_hi, f16* out_lo,      // out in blk layout (KT = 24)
                   const float* cls, const float* pos, float* resid, int D, hipStream_t s);
// position-embedding resample: out[1 + y gw + x][d] = sum_ij wy[y][i] wx[x][j] pos[1 + (y0[y] + i) gs + x0[x] + j][d], out[0] = pos[0];
// ybeg / xbeg: first input index per output row / column, wy / wx: ytaps / xtaps weights each (zero-padded), gs: source grid side
void launch_pos_resample(const float* pos, int gs, int D, int gh, int gw, const int* ybeg, const double* wy, int ytaps,
                         const int* xbeg, const double* wx, int xtaps, float* out, hipStream_t s);
// Pillow-exact bicubic Resize + CenterCrop of raw uint8 HWC images (weights / windows from keep_amd/preprocess.py)
void launch_resize_crop_u8(const unsigned char* src, int B, int H, int W, const int* xb, const int* xk, int xks, int col0, int ncols,
                           const int* yb, const int* yk, int yks, int row0, int nrows, unsigned char* tmp, unsigned char* out, hipStream_t s);
// the vertical pass alone: tmp [B,H,ncols,3] (already resized horizontally) -> out [B,nrows,ncols,3], output rows row0.. of the table
void launch_resize_v_u8(const unsigned char* tmp, int B, int H, int ncols, const int* yb, const int* yk, int yks, int row0, int nrows,
                        unsigned char* out, hipStream_t s);
void launch_split_f16(const float* src, f16* hi, f16* lo, int64_t n, hipStream_t s);
// row-major fp32 [M][K] -> blk-layout fp16 hi (+lo); rows M..pad are zero-filled
void launch_split_blockify(const float* src, f16* hi, f16* lo, int M, int K, hipStream_t s);
// the same plus the MX-fp4 side planes of quant4.h (q: both planes, sc: scales); K % 32 == 0; lo may be null
void launch_quant_blockify(const float* src, f16* hi, f16* lo, unsigned char* q, unsigned char* sc, int M, int K, hipStream_t s);
// blk-layout fp16 hi (+lo) -> row-major fp32 [M][K]; lo null: the hi plane's values as they are (the sign of a zero included)
void launch_unblockify_f32(const f16* hi, const f16* lo, float* out, int M, int K, hipStream_t s);
// stats2[0] = max |w| (read as float), stats2[1] = sum w^2 -- the load-time range check of the fp16 operand planes
void launch_weight_stats(const float* w, int64_t n, float* stats2, hipStream_t s);
void launch_l2norm_rows(float* x, int rows, int D, float eps, hipStream_t s, int* err_flag = nullptr);   // err_flag |= 2 if a row is not finite
void launch_row_argmax(const float* x, int rows, int cols, int32_t* out, hipStream_t s);
void launch_row_softmax(const float* x, int rows, int cols, float scale, float* out, hipStream_t s);
void launch_row_softmax_f16(const float* x, int rows, int cols, float scale, f16* out, hipStream_t s);
void launch_top2_score(const float* x, int rows, int cols, float* partial, float* out, hipStream_t s);
void launch_bert_embed_ln(const int64_t* ids, const int64_t* type_ids, const float* wemb, const float* pemb,
                          const float* temb, const float* gamma, const float* beta, float eps,
                          int P, int T, int D, int vocab, int type_vocab,
                          float* resid, f16* out_hi, f16* out_lo /* blk layout */, int* err_flag, hipStream_t s);
// mean-input compensation (keep_calibrate_bias): column sums of a blk-layout fp16 matrix (accumulating, deterministic), and
// out[n] = bias[n] + sum_k w_lo[n][k] * col_sum[k] * inv_rows for a GEMM weight's lo plane
void launch_blk_col_sum(const f16* x, int M, int K, float* out, hipStream_t s);
void launch_bias_mean_corr(const f16* w_lo, const float* col_sum, float inv_rows, const float* bias, float* out, int N, int K, hipStream_t s);
void launch_gather_rows_f32(const float* src, int64_t src_stride, float* dst, int rows, int D, hipStream_t s);
void launch_scatter_rows_f32(const float* src, float* dst, int64_t dst_stride, int rows, int D, hipStream_t s);   // dst row r * dst_stride <- src row r
// blk-layout fp16 [*, D]: dst row r <- src row r * row_stride
void launch_gather_rows_blk(const f16* src, int row_stride, f16* dst, int rows, int D, hipStream_t s);

// wsi.hip
void launch_group_top2(const float* logits, int n, int K, int C, float* partial, int max_row_blocks, float* sums, hipStream_t s);
void launch_top2_slots_reduce(const float* partial, int nslots, int kpad, int K, float scale, float* out, hipStream_t s);
void launch_scale_vec(const float* in, int n, float f, float* out, hipStream_t s);
int launch_sim_small(const float* img, const float* txt, int N, int P, int D, float scale, int mode, void* out, int32_t* amax,
                     hipStream_t s);            // 0 handled, -1 not eligible (P > 8, D not 768/1024)
int launch_sim_mid(const float* img, const float* txt, int N, int P, int D, float scale, int mode, void* out, int32_t* amax,
                   hipStream_t s);              // 9 <= P <= 64: fused fp32-MFMA similarity + argmax / softmax; 0 handled, -1 not eligible
void launch_diag_rank(const float* sim, int rows, int n_img, const int* target, int row0, int* rank, hipStream_t s);
// keep_classify: ordered list of the rows whose top-2 margin is below `bound` (count on the device), tile / row movers
void launch_top2_margin_flags(const float* sim, int N, int P, float bound, int* flags, int* list, int* count, hipStream_t s);
void launch_gather_tiles(const void* src, int64_t tile_bytes, const int* list, int n, void* dst, hipStream_t s);     // tile_bytes % 16 == 0
void launch_scatter_rows(const float* src, const int* list, int n, int D, float* dst, hipStream_t s);
void launch_refine(const float* probs, const long long* coords, int n, int C, long long patch, int overlap,
                   unsigned long long* keys, int* first, unsigned table_size, float* out, int* is_first, hipStream_t s);

// launch_util.hip: per-(kernel, device) opt-in to more than 64 KiB of dynamic LDS (cached, thread-safe; a refusal leaves no sticky HIP error behind),
// and the CU count of the current device
bool keep_lds_opt_in(const void* kernel, size_t bytes);
int keep_num_cus();

enum PixelDType : int { PIX_F32 = 0, PIX_F16 = 1, PIX_BF16 = 2, PIX_U8_HWC = 3 };
