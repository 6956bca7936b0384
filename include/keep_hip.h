/*
 * libkeep_hip -- C ABI of the MI355X (gfx950) KEEP zero-shot inference engine.
 *
 * This is the drop-in boundary for the hot path of MAGIC-AI4Med/KEEP: everything below
 * `KEEPModel.encode_image` / `encode_text` / the tile x prompt similarity.  Each entry point names
 * the reference interface it replaces (paths relative to the reference repo root).
 *
 * Conventions
 *   - all functions return 0 on success or a negative KEEP_E* code; keep_last_error(h) gives text
 *   - every data pointer is a raw DEVICE pointer on the handle's GPU unless stated otherwise
 *     (e.g. torch.Tensor.data_ptr()); the caller owns all I/O buffers, the engine owns weights,
 *     repacked fp16 planes and its workspace
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous on
 *     it, with no hidden device synchronisation once the workspace is large enough
 *     (keep_reserve() up front avoids the allocation a first call would otherwise do)
 *   - a handle is not thread-safe: one handle per GPU per host thread
 *   - no torch / C++ types cross this boundary
 *   - multi-GPU: one handle per GPU per process.  The path shards without a data-path collective (tiles are independent through
 *     keep_encode_image and keep_similarity); the one exchange step of a slide -- the all-gather of the per-tile embeddings this
 *     library writes into the caller's buffer -- is the HOST's: ncclAllGather / torch.distributed.all_gather_into_tensor on that
 *     buffer, ordered after the encode by the stream both were given (keep_amd/distributed.py).  There is deliberately no
 *     keep_allgather(): the library neither links RCCL nor owns a communicator.
 */
#ifndef KEEP_HIP_H
#define KEEP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct keep_handle keep_handle;

enum {
    KEEP_OK = 0,
    KEEP_EINVAL = -1,       /* bad argument / shape / dtype                                  */
    KEEP_ESTATE = -2,       /* call out of order (weights not finalised, ...)                */
    KEEP_EKEY = -3,         /* unexpected or missing state_dict key (load_state_dict strict) */
    KEEP_EHIP = -4,         /* HIP runtime error                                             */
    KEEP_EUNSUPPORTED = -5, /* shape outside what the kernels implement                      */
    KEEP_ENOMEM = -6
};

/* pixel dtypes accepted by keep_encode_image */
enum { KEEP_PIX_F32 = 0, KEEP_PIX_F16 = 1, KEEP_PIX_BF16 = 2,   /* [B,3,224,224] NCHW, already ImageNet-normalised */
       KEEP_PIX_U8_HWC = 3 };                                   /* [B,224,224,3] raw uint8 RGB: ToTensor + Normalize fused on the device */

/* similarity modes */
enum {
    KEEP_SIM_RAW = 0,         /* out f32 [N,P] = scale * img @ txt^T          keep_inference.py:104          */
    KEEP_SIM_ARGMAX = 1,      /* RAW + argmax_out int32 [N] (out may be NULL)                                */
    KEEP_SIM_SOFTMAX = 2,     /* out f32 [N,P] = softmax(scale*cos, dim=1)    subtyping_utils.py:72 (scale 10)*/
    KEEP_SIM_SOFTMAX_F16 = 3, /* same, out fp16 [N,P]                          (BASELINE config 5)            */
    KEEP_SIM_TOP2SCORE = 4    /* out f32 [1] = mean_t[(v1-v2)-|v1+v2-1|]      WSI_evaluation/utils.py:107-117 */
};

/* precision modes (keep_set_option "precision") */
enum {
    KEEP_PREC_FP16 = 0,   /* fp16 MFMA operands, fp32 accumulate, fp32 residual/LN/softmax/GELU: fastest, cosines    */
                          /* within ~1.5e-4 of the fp32 reference (outside the 1e-4 north-star tolerance)          */
    KEEP_PREC_STRICT = 1, /* hi/lo split operands, 3 MFMA passes: fp32-class accuracy (4e-7), ~0.4x the speed       */
    KEEP_PREC_COMP = 2    /* DEFAULT.  fp16 pass + first-order correction terms where the error budget needs them: */
                          /* a per-block plan for the image tower (keep_set_block_precision: MLP GEMMs on the       */
                          /* MX-fp4 MFMA pipe, attention side as split products), the whole text tower as split     */
                          /* products.  Cosines within 1e-4 of the fp32 reference.                                  */
};

/* per-block treatment of the image tower in KEEP_PREC_COMP (keep_set_block_precision) */
enum {
    KEEP_ATTN_PLAIN = 0,          /* qkv, q/k/v storage, attention, proj: single fp16 passes                                       */
    KEEP_ATTN_SPLIT = 1,          /* all four as split products (three fp16 passes; q/k/v and the attention output stored hi + lo)  */
    KEEP_ATTN_SPLIT_COMPQKV = 2,  /* the same with the qkv GEMM as a compensated product (fp16 pass + MX-fp4 correction terms)      */
    KEEP_ATTN_COMPQKV = 3,        /* only the qkv GEMM compensated; attention and proj plain                                       */
    KEEP_ATTN_PROJ_CLS = 4        /* single fp16 passes for every row; the attention output of the CLS row of every tile is ALSO kept */
                                  /* hi + lo from the fp32 accumulators and its proj runs again as a split product (B rows): on      */
                                  /* spatially correlated tiles the proj GEMM carries ~70 % of the attention side's rounding error   */
                                  /* and the CLS row's own share of it is what reaches the pooled feature (round 6)                  */
    , KEEP_ATTN_COMPQKV_PROJ_CLS = 5 /* KEEP_ATTN_COMPQKV and KEEP_ATTN_PROJ_CLS together: compensated qkv GEMM, plain attention, plain     */
                                  /* proj + the CLS rows' proj again as a split product -- between "CLS-row proj" and "everything split"   */
};
enum {
    KEEP_MLP_PLAIN = 0,           /* fc1 / fc2: single fp16 passes                                                                  */
    KEEP_MLP_SPLIT = 1,           /* split products (three fp16 passes)                                                             */
    KEEP_MLP_COMP = 2,            /* compensated: fp16 pass + both first-order terms W_lo A_hi + W_hi A_lo on the MX-fp4 pipe       */
    KEEP_MLP_COMP_W = 3,          /* compensated, weight-rounding term W_lo A_hi only (half the fp4 MFMAs and operand bytes; the    */
                                  /* LayerNorm / GELU epilogues write Q(x_hi) only): removes the W half of the fp16 rounding error  */
    KEEP_MLP_CLS = 4              /* single fp16 passes for every row, then the CLS row of every tile AGAIN as split products: B rows */
                                  /* through LayerNorm-2 -> fc1 -> GELU -> fc2 on the small-M kernels, written over the fp16 result.  */
                                  /* The pooled output IS the CLS row (global_pool='token', keep_inference.py:32-40): its own rounding */
                                  /* errors reach the feature directly, the other 196 rows' only through attention averages          */
};

const char* keep_version(void);

/* ---- lifetime ---------------------------------------------------------------------------------
 * Replaces: `AutoModel.from_config(config)` + `.to(device)`  (quick_start/keep_inference.py:81,
 * WSI_evaluation/zeroshot_subtyping_WSI.py:44-46). */
int keep_create(int device_id, keep_handle** out);
int keep_destroy(keep_handle* h);
const char* keep_last_error(keep_handle* h);
/* Notes collected by keep_load_tensor since the last call ('\n'-separated, "" if none; the call clears them): e.g. a GEMM weight whose rms is so
 * small that its entries fall into fp16 subnormals.  Such a tensor LOADS (torch's load_state_dict, keep_inference.py:83, has no such notion);
 * the Python binding turns each line into a warnings.warn.  The pointer is valid until the calling thread's next keep_load_warnings call. */
const char* keep_load_warnings(keep_handle* h);

/* ---- weights ----------------------------------------------------------------------------------
 * Replaces: `model.load_state_dict(state_dict, strict=True)`  (quick_start/keep_inference.py:82-83).
 * Call keep_load_tensor once per state_dict entry using the release key names (SURVEY.md A.3:
 * "visual.blocks.3.attn.qkv.weight", "text.encoder.layer.0.attention.self.query.weight", ...),
 * fp32 data, then keep_finalize_weights(), which fails with KEEP_EKEY if any expected key is missing
 * (strict semantics).  Data is copied / repacked; the caller's buffer may be freed afterwards.
 * `on_device` != 0: `data` is a device pointer on the handle's GPU; 0: host pointer. */
int keep_load_tensor(keep_handle* h, const char* key, const float* data, int ndim, const int64_t* shape,
                     int on_device);
int keep_finalize_weights(keep_handle* h);
/* after finalize: depth / layer counts actually loaded (0 if that tower was not loaded) */
int keep_vit_depth(keep_handle* h);
int keep_bert_layers(keep_handle* h);

/* ---- options ----------------------------------------------------------------------------------
 *   "precision"       KEEP_PREC_COMP (default) | KEEP_PREC_FP16 | KEEP_PREC_STRICT
 *   "strict_blocks"   run the first n ViT blocks (+ patch embed) / BERT layers in split mode (default 0)
 *   "comp_full_blocks" KEEP_PREC_COMP, prefix shorthand: the first n ViT blocks get KEEP_ATTN_SPLIT, the rest KEEP_ATTN_PLAIN (1 unless set)
 *   "comp_mlp_blocks"  KEEP_PREC_COMP, prefix shorthand: the first n ViT blocks get KEEP_MLP_COMP, the rest KEEP_MLP_PLAIN (8 unless set).
 *                     Setting any of the four comp_* shorthands REWRITES the whole per-block plan (keep_set_block_precision below) to that prefix
 *                     family.  A handle STARTS with another plan: block 0 KEEP_ATTN_SPLIT_COMPQKV + KEEP_MLP_COMP, every other block
 *                     KEEP_ATTN_PLAIN + KEEP_MLP_CLS -- until KEEPModel.calibrate / keep_set_block_precision replace it.
 *   "plan_custom"      (read only) 1 if keep_set_block_precision changed the plan since the last shorthand
 *   "graph_count"      (read only) the captured graphs the handle holds; a graph made stale by an option change is dropped when its call comes again
 *   "comp_min_tiles"   sub-batches with fewer tiles use split products instead of compensated ones (default 32)
 *   "comp_qkv"         KEEP_PREC_COMP: 1 = the qkv GEMM of the split-attention blocks as a compensated product instead of a split one
 *                     (default 0: +0.9 % at equal settings, but calibrate() then needs more compensated MLP blocks -- a net loss)
 *   "comp_qkv_from"    the same for the split-attention blocks with index >= n only (default: none; round 4: 2 / 6 with n = 1 misses the rms target 1 / 8 meets)
 *   "label_margin"     keep_classify: cosine margin below which a tile's label is re-derived in KEEP_PREC_STRICT (default 2.5e-4)
 *   "fused_screening"  keep_prompt_scores with C in {2, 4}: 1 (default) one compensated GEMM with the top-2 score taken in the
 *                     accumulator registers (no logits in HBM) | 2 the same with three fp16 passes | 0 chunked fp32 GEMM + reduction
 *   "max_tiles"       tiles per internal sub-batch of keep_encode_image (default 256)
 *   "max_prompts"     prompts per internal sub-batch of keep_encode_text (default 64)
 *   "streams"         concurrent sub-batches inside keep_encode_image (default 2, 1..4): the batch is split
 *                     into that many lanes on internal HIP streams, issued layer-interleaved, and joined
 *                     back onto the caller's stream with events (no host synchronisation)
 *   "cls_tail"        1 (default): in the last ViT block run proj / MLP for the CLS rows only (exact: the
 *                     pooled output reads nothing else); 0: evaluate every token as the reference does
 *   "proj_impl"       2128 (default): the plain proj GEMMs on the 256x128 / 4-wave / two-workgroups-per-CU kernel (one workgroup's residual epilogue under the
 *                     other's K loop): -8.5 % on the proj launches, +0.57 % end to end (profiles/r05_ab_two_workgroups_per_cu.txt) | 0: the persistent 256x256 kernel.
 *                     Bit-identical results.
 *   "bias_correction" 1 (default): plain launches use the mean-input-compensated biases once keep_calibrate_bias has run | 0: the checkpoint's biases
 *   "gemm_impl"       0 auto | 128 | 256: LDS-DMA tile width override.  Like every option it belongs to the handle.
 *   "graphs"          1 (default): launch-bound calls -- keep_encode_image of at most 1024 token rows (5 tiles), keep_encode_text of at most
 *                     4096 token rows (e.g. 64 prompts x 64 tokens) -- are captured once per shape and replayed as one hipGraph launch (~100
 *                     dependent kernels of a few microseconds each); 0: always launch kernels
 *   "gemm_skinny_m"   calls with at most this many rows take the small-M split-K GEMM (default 320, 0 never).  The two GEMM paths agree to rounding, each is bit-reproducible
 *   "gemm_splitk_tiles"  a larger call whose 256x256 tiling has fewer tiles than this (default 64, 0 never) is cut into
 *                     K slices with fp32 partials + the same reduce/epilogue kernel (8-16 tiles per call: -16..-26 %)
 *   "gemm_persistent" 1 (default): a plain (one fp16 pass, hi-only output) 256x256 GEMM with more tiles than the device has CUs runs as one
 *                     workgroup per CU walking the tile list, the next tile's first three K steps staged under the epilogue; 0: one
 *                     tile per workgroup.  Bit-identical results either way.
 *   "sgemv_m"         same for the few-row fp32 kernel of the projection head / pooler / similarity (default 16)
 *   "ln_impl"         2 (default) LayerNorm with LDS-transposed K-blocked stores from 4-wave workgroups (co-resident with the other lane's persistent fc1 GEMM:
 *                     +0.3 % end to end) | 1 the same from 8-wave workgroups | 0 per-row stores.  Same results bit for bit.
 *   "attn_waves"      16 (default): image-tower attention of >= 512 (image, head) pairs on the persistent double-buffered kernel (bit-identical
 *                     to 8, the K / V staging of the next pair runs under the current one's compute), 8 waves per workgroup elsewhere | 8 | 4
 *   "gemm_ablate", "gemm_dbg"   timing diagnostics (results are wrong when ablating): -DKEEP_DIAGNOSTICS builds only
 */
int keep_set_option(keep_handle* h, const char* name, double value);
double keep_get_option(keep_handle* h, const char* name);
/* The per-block plan of KEEP_PREC_COMP: block `block` (0 .. 63) of the image tower gets attention-side treatment `attn_mode` (KEEP_ATTN_*) and
 * MLP treatment `mlp_mode` (KEEP_MLP_*); a negative mode leaves that half as it is.  Replaces nothing in the reference (which computes in fp32,
 * quick_start/keep_inference.py:54-58): it is how this engine spends its precision budget -- where the fp16 rounding of a block matters for the
 * final cosine is a property of the checkpoint, measured by KEEPModel.calibrate / tools/precision_budget.py.  Sub-batches below "comp_min_tiles"
 * run split products wherever a compensated one is planned.  KEEP_PREC_STRICT / "strict_blocks" override the plan; KEEP_PREC_FP16 ignores it. */
int keep_set_block_precision(keep_handle* h, int block, int attn_mode, int mlp_mode);
/* Mean-input compensation of the weight-rounding error (replaces nothing in the reference, which multiplies in fp32: quick_start/keep_inference.py:54-58).
 * A single-pass fp16 GEMM drops the term W_lo A_hi^T.  Part of it is the same for every row: W_lo a_mean, a_mean = the mean input row of that GEMM (GELU
 * outputs are positive, LayerNorm outputs carry their bias, attention outputs are averages) -- 10-50 % of that GEMM's weight-rounding variance on the
 * synthetic checkpoints, and the one part of the rounding error that does not average out over a slide's tiles.  It is a constant vector per GEMM: this call
 * encodes the B calibration tiles (>= 8; KEEP_PIX_* layouts as keep_encode_image) in split products, averages the input rows of the four GEMMs of every ViT
 * block and stores bias + W_lo a_mean; every PLAIN launch (KEEP_ATTN_PLAIN / KEEP_MLP_PLAIN, KEEP_PREC_FP16) then uses that bias -- zero cost per call.  Split and
 * compensated launches compute the term itself and keep the checkpoint's bias.  B = 0 forgets the calibration; loading weights forgets it too.
 * Option "bias_correction" (default 1) switches the use on and off; option "bias_ready" (read only) says whether a calibration is held. */
int keep_calibrate_bias(keep_handle* h, const void* pixels, int pix_dtype, int64_t B, void* stream);
int keep_get_block_precision(keep_handle* h, int block, int* attn_mode, int* mlp_mode);

/* ---- preprocessing on the device -----------------------------------------------------------------
 * Replaces: transforms.Resize(224, BICUBIC) + CenterCrop((224,224))  (quick_start/keep_inference.py:88-90) for raw uint8
 * RGB images [B,H,W,3] of one size.  The fixed-point windows / weights of Pillow's resample are built by the caller
 * (keep_amd/preprocess.py: pil_bicubic_coeffs) -- bounds [out,2] = (first input index, count), weights [out,ksize] -- and the
 * two integer passes run here, so the result is bit-identical to PIL's.  out: uint8 [B,size,size,3], ready for
 * keep_encode_image(..., KEEP_PIX_U8_HWC, ...). */
int keep_resize_crop_u8(keep_handle* h, const unsigned char* src, int64_t B, int64_t H, int64_t W, const int32_t* xbounds,
                        const int32_t* xweights, int xksize, int64_t out_w, const int32_t* ybounds, const int32_t* yweights, int yksize,
                        int64_t out_h, int64_t crop_left, int64_t crop_top, int64_t size, unsigned char* out, void* stream);

/* ---- slide regions on the device ------------------------------------------
 * region: uint8 [H,W,C] RGB (pix_stride 3) or RGBA (pix_stride 4, alpha ignored), rows row_stride_bytes apart (>= W * pix_stride,
 * so a cropped view of a larger image needs no copy).  Grid cells of side `patch` (>= 16) sit at (gx * step, gy * step) for every
 * cell that lies wholly inside the region, row-major (y outer, x inner).
 *
 * Replaces: the CLAM patching + segmentation step the reference's README (README.md:74) runs before any WSI script, i.e. the
 * tile grid and coords of the CLAM .h5 files.  A pixel is tissue iff max(r,g,b) > 0 and 255 (max - min) >= sat_min max (HSV
 * saturation >= sat_min, integer-exact); a cell is kept iff it holds >= min_pixels tissue pixels (min_pixels = 0: every cell).
 * cell_xy_out: int32 [gx * gy, 2] device buffer; its first *n_out rows receive the kept cells' (x, y) pixel offsets in grid order
 * (stable compaction, deterministic).  n_out: ONE int64 on the device. */
int keep_region_grid(keep_handle* h, const unsigned char* region, int64_t H, int64_t W, int64_t row_stride_bytes, int pix_stride,
                     int64_t patch, int64_t step, int sat_min, int64_t min_pixels, int32_t* cell_xy_out, int64_t* n_out, void* stream);
/* Replaces: the host patch cut (openslide read_region per coord + PIL convert("RGB")) and transforms.Resize(224, BICUBIC) +
 * CenterCrop((224,224)) (quick_start/keep_inference.py:88-90) of every patch.  out: uint8 [B,224,224,3] for
 * keep_encode_image(..., KEEP_PIX_U8_HWC, ...).  patch == 224: the patches themselves (tables may be NULL); otherwise Pillow's
 * bicubic resize of the patch to 224 x 224 with the tables of keep_resize_crop_u8 (pil_bicubic_coeffs(patch, 224) for both
 * axes), bit-identical to PIL.  A cell outside the region is KEEP_EINVAL: the cells are checked on the device and the flag read
 * back before any pixel is read (one stream synchronisation per call). */
int keep_region_patches_u8(keep_handle* h, const unsigned char* region, int64_t H, int64_t W, int64_t row_stride_bytes, int pix_stride,
                           const int32_t* cell_xy, int64_t B, int64_t patch, const int32_t* xbounds, const int32_t* xweights, int xksize,
                           const int32_t* ybounds, const int32_t* yweights, int yksize, unsigned char* out, void* stream);

/* ---- tissue mask from a thumbnail, and the grid decided by a mask -----------
 * Replaces: the tissue segmentation of the CLAM step the reference's README (README.md:74) runs before any WSI script
 * (CLAM's segmentTissue: HSV saturation, medianBlur, fixed or Otsu threshold, morphological closing, contour / hole area
 * filters), restated on the pixel mask instead of on contour polygons; integer arithmetic, exact.
 * thumb: uint8 [H,W,C] RGB / RGBA with the layout contract of keep_region_grid, H W <= 2^30.  ksize: odd, 1 (off) .. 15, border
 * replicated.  median_out: uint8 [H,W]: the median of S = (2 * 255 (max - min) + max) / (2 max) (0 where max = 0).
 * hist_out: int32 [256] on the device, zeroed here and filled with the histogram of median_out (for Otsu's threshold, which
 * the caller picks: keep_amd.region.otsu_threshold). */
int keep_tissue_median_hist(keep_handle* h, const unsigned char* thumb, int64_t H, int64_t W, int64_t row_stride_bytes, int pix_stride,
                            int ksize, unsigned char* median_out, int32_t* hist_out, void* stream);
/* Replaces: the rest of segmentTissue.  median: uint8 [H,W] contiguous.  Foreground iff median > threshold (0..255); closing by a
 * close x close box (0 = off, <= 31; anchor close / 2, OpenCV's constant borders); background 4-components that touch no border
 * and hold <= min_hole pixels are filled; foreground 8-components of <= min_area pixels are dropped.  mask_out: uint8 {0,1}
 * [H,W] (must not alias median).  A labelling loop that runs into its iteration cap sets bit 2 (value 4) of the handle's sticky
 * error word (keep_token_error). */
int keep_tissue_mask(keep_handle* h, const unsigned char* median, int64_t H, int64_t W, int threshold, int close, int64_t min_hole,
                     int64_t min_area, unsigned char* mask_out, void* stream);

/* how a grid cell is tested against a mask: CLAM's isInContour family */
enum { KEEP_MASK_FOUR_PT = 0,       /* any of the four points (c.x +- patch / 4, c.y +- patch / 4), c = cell origin + patch / 2 */
       KEEP_MASK_FOUR_PT_HARD = 1,  /* all four                                                                              */
       KEEP_MASK_CENTER = 2 };      /* c itself                                                                              */
/* Replaces: CLAM's patch-level contour test (isInContourV3_Easy / _Hard / V2) in the patching step of README.md:74.  mask: uint8
 * [mh,mw] contiguous on the device, one pixel = downsample x downsample pixels of the level being tiled.  The grid is that of
 * keep_region_grid over an H x W region whose first pixel sits at (origin_x, origin_y) of the level; a point (px, py) is tissue
 * iff mask[py / downsample][px / downsample] != 0, outside the mask it is not.  No region pixel is read.  Outputs as
 * keep_region_grid's. */
int keep_region_grid_mask(keep_handle* h, const unsigned char* mask, int64_t mh, int64_t mw, int64_t downsample, int64_t H, int64_t W,
                          int64_t patch, int64_t step, int64_t origin_x, int64_t origin_y, int mode, int32_t* cell_xy_out, int64_t* n_out,
                          void* stream);

/* ---- Macenko stain normalisation ---------------------------------------------
 * Replaces: nothing the reference runs (its WSI scripts read features of tiles as they were scanned); it stands where a host
 * library (torchstain, staintools) would otherwise sit between the patch cut and quick_start/keep_inference.py:54-58's
 * encode_image.  Macenko et al. 2009 restated in fixed point, integer arithmetic, exact against keep_amd.stain's numpy restatements;
 * the dense algebra between the passes (3 x 3 eigh, 3 x 2 pinv, percentiles off the histograms) is the caller's, in float64.
 * image: uint8 [H,W,C] RGB / RGBA with the layout contract of keep_region_grid, H W <= 2^30.  mask: NULL (every pixel) or uint8
 * [mh,mw] contiguous on the device, one pixel = downsample x downsample image pixels: pixel (x, y) reads
 * mask[y / downsample][x / downsample], outside the mask it is not allowed.  od_q: int32 [256] on the device,
 * rint(-ln((v + 1) / Io) * 2^12), |od_q| < 2^15.  A pixel is KEPT iff the mask allows it and all three od_q >= beta_q.
 * moments_out: int64 [10] on the device, 8-byte aligned: n, S_r, S_g, S_b, S_rr, S_rg, S_rb, S_gg, S_gb, S_bb over the kept pixels.
 * zero_first != 0 starts a new sum, 0 adds to the one there: integer sums, so the result is the same however the pixels are split
 * over calls (bands of a region, slides of a cohort). */
int keep_stain_moments(keep_handle* h, const unsigned char* image, int64_t H, int64_t W, int64_t row_stride_bytes, int pix_stride,
                       const unsigned char* mask, int64_t mh, int64_t mw, int64_t downsample, const int32_t* od_q, int beta_q, int zero_first,
                       int64_t* moments_out, void* stream);
/* Replaces: numpy.arctan2 of the kept pixels' plane coordinates + the histogram behind numpy.percentile.  v_q: int32 [3][2] ON THE
 * HOST, |v_q| <= 2^14 (rint(V * 2^14) of two unit vectors); t = od_q . v_q per kept pixel, |t| < 2^31.  hist_out: int32 [4096] on
 * the device: the bin of atan2(t1, t0) among 4096 equal bins of [-pi, pi), decided by integer comparisons against dirs: int32
 * [1024][2] on the device, (rint(2^30 cos), rint(2^30 sin)) of j 2 pi / 4096; t = (0, 0) counts as the angle 0, the angle pi as -pi.
 * zero_first as above; at most 2^31 - 1 pixels may ever be added into one histogram. */
int keep_stain_angle_hist(keep_handle* h, const unsigned char* image, int64_t H, int64_t W, int64_t row_stride_bytes, int pix_stride,
                          const unsigned char* mask, int64_t mh, int64_t mw, int64_t downsample, const int32_t* od_q, int beta_q,
                          const int32_t* v_q, const int32_t* dirs, int zero_first, int32_t* hist_out, void* stream);
/* Replaces: numpy.linalg.lstsq(HE, OD) over every pixel the mask allows (no beta rule, as the float method has none there) + the
 * histograms behind the 99th percentiles.  minv_q: int32 [2][3] ON THE HOST, rint(pinv(HE) * 2^14), |minv_q| <= 2^24; c_s = od_q .
 * minv_q[s] in Q26; hist_out: int32 [2][4096] on the device, bin clamp(c_s >> 17, 0, 4095) (1 / 512 wide, 0 .. 8). */
int keep_stain_conc_hist(keep_handle* h, const unsigned char* image, int64_t H, int64_t W, int64_t row_stride_bytes, int pix_stride,
                         const unsigned char* mask, int64_t mh, int64_t mw, int64_t downsample, const int32_t* od_q, const int32_t* minv_q,
                         int zero_first, int32_t* hist_out, void* stream);
/* Replaces: Io * exp(-HERef . (C * maxCRef / maxC)) of the float method, and its colour deconvolution images, as ONE 3 x 3 matrix
 * between two tables.  src, dst: uint8 [n,3] contiguous on the device, dst == src allowed (no other overlap).  t_q: int32 [3][3] ON
 * THE HOST, rint(T * 2^14), |T| <= 64 or KEEP_EINVAL.  Per pixel and output channel o = (sum_d t_q[c][d] od_q[src_d] + 2^15) >> 16
 * (Q10, arithmetic shift) and dst_c = exp_lut[clamp(o - lo, 0, lut_len - 1)]; exp_lut: uint8 [lut_len] on the device, 4-byte aligned,
 * 1 <= lut_len <= 8192. */
int keep_stain_apply_u8(keep_handle* h, const unsigned char* src, int64_t n, const int32_t* od_q, const int32_t* t_q,
                        const unsigned char* exp_lut, int lut_len, int lo, unsigned char* dst, void* stream);

/* ---- tile quality control: pen ink, dark, glass, tissue share and focus -----
 * Replaces: nothing the reference runs (its WSI scripts take the tiles CLAM kept); it stands where HistoQC-style filters sit in the
 * pipelines around it, between the patch grid and quick_start/keep_inference.py:54-58's encode_image.  Integer arithmetic, exact
 * against keep_amd.quality's numpy restatements.
 * rules: int32 [776] ON THE DEVICE, 4-byte aligned (keep_amd.quality.QualityRules.blob()): sat_min, white_min, dark_max, the number
 * of pen boxes (0..32), the index of the first box of class 1, of class 2 and of class 3 (the boxes sorted by class), 0, then three
 * tables of 256 words for r, g and b: bit i of word v is set iff box i holds the value v in that channel.  Every pixel has ONE class,
 * the first that applies of: pen ink of the lowest class with a box that holds it; dark, max(r,g,b) <= dark_max; glass,
 * min(r,g,b) >= white_min; tissue, max > 0 and 255 (max - min) >= sat_min max (keep_region_grid's rule); other.
 * region, H, W, pix_stride, row_stride_bytes: the layout contract of keep_region_grid; cell_xy: int32 [N][2] (x, y) offsets of N
 * cells of side patch, 1 <= patch <= 1024, as keep_region_patches_u8 takes them (overlapping cells are fine; a cell outside the
 * region is KEEP_EINVAL: checked on the device, one stream synchronisation per call); 0 <= N <= 2^24 - 1.  A contiguous batch of tiles
 * [N][S][S][3] is the region H = N S, W = S with the cells (0, i S).
 * out: int64 [N][12] on the device, 8-byte aligned; zero_first != 0 starts new sums, 0 adds to the words there.  Columns: 0-3 the
 * pixels of pen class 0..3, 4 dark, 5 glass, 6 tissue (P^2 minus their sum is "other"); with g = (77 r + 150 g + 29 b + 128) >> 8 and
 * L = 4 g(x,y) - g(x-1,y) - g(x+1,y) - g(x,y-1) - g(x,y+1) over the (patch - 2)^2 interior pixels of the cell itself (no pixel
 * outside the cell is read): 7 sum L, 8 sum L^2; 9 the interior pixels whose own class is tissue, 10 and 11 sum L and sum L^2 over
 * those.  patch < 3: columns 7-11 are 0. */
int keep_region_quality(keep_handle* h, const unsigned char* region, int64_t H, int64_t W, int pix_stride, int64_t row_stride_bytes,
                        const int32_t* cell_xy, int64_t N, int64_t patch, const int32_t* rules, int zero_first, int64_t* out, void* stream);
/* The class of every pixel of a thumbnail, with the classifier above.  thumb: uint8 [H,W,pix_stride] as keep_tissue_median_hist takes
 * it, H W <= 2^30; out: uint8 [H][W] contiguous on the device: 0 none, 1-4 pen class + 1, 5 dark, 6 glass, 7 tissue. */
int keep_pen_mask(keep_handle* h, const unsigned char* thumb, int64_t H, int64_t W, int pix_stride, int64_t row_stride_bytes,
                  const int32_t* rules, unsigned char* out, void* stream);

/* ---- tile scores rasterised onto the slide thumbnail -------------------------
 * The accumulator `acc` is int64 [H,W] contiguous on the device, 8-byte aligned, H W <= 2^30, one word per raster pixel read as
 * unsigned: bits 0..39 hold the sum of q over the tiles that cover the pixel, bits 40..63 their number, q = rint(clip(value, 0, 1) *
 * 65535) (round half to even).  At most 2^24 - 1 tiles may ever be added into one accumulator (the caller counts them), so that
 * neither field can overflow; integer sums do not depend on the order, so a raster is the same however its tiles are split
 * over calls.
 *
 * Replaces: the pred-mask painting of eval_seg_coarse (WSI_evaluation/segment_utils.py:134-140: every tile above the threshold
 * painted into a level-16 array) and, with keep_heat_render, the heatmap that closes CLAM's step of README.md:74.
 * coords: int64 [N,2] level-0 (x, y); values: fp32 [N]; a tile covers raster columns [floor((x - origin_x) / downsample),
 * floor((x - origin_x + patch) / downsample)) and rows likewise, clipped to the raster; a NaN value skips its tile.  1 <= downsample
 * <= patch <= 2^30, origin a multiple of downsample within +-2^40, 0 <= N <= 2^24 - 1.  zero_first != 0 starts a new raster, 0 adds
 * into the one in acc. */
int keep_heat_accumulate(keep_handle* h, const int64_t* coords, const float* values, int64_t N, int64_t patch, int64_t downsample,
                         int64_t H, int64_t W, int64_t origin_x, int64_t origin_y, int zero_first, int64_t* acc, void* stream);
/* keep_heat_accumulate with one value per cell of a gh x gw grid inside every tile (the token grid of the image
 * tower, 14 x 14 cells of 16 pixels in a 224 tile): values fp32 [N, gh gw], row-major (y, x).  A tile's pixel footprint is exactly
 * keep_heat_accumulate's; footprint pixel (X, Y) takes the cell cx = clamp(floor((X downsample + origin_x - x) / cw), 0, gw - 1), cy
 * likewise, cw = patch / gw, ch = patch / gh: the cell under the pixel's upper-left corner in level-0 units.  Each (tile, pixel) adds
 * (1 << 40) | q of that cell, so the count field still counts tiles and the 2^24 - 1 cap is a cap on tiles; a NaN cell adds nothing
 * to its pixels, neither sum nor count.  Needs patch % gw == 0, patch % gh == 0, gh gw <= 2^24 and 1 <= downsample <= min(cw, ch);
 * everything else as keep_heat_accumulate.  Integer arithmetic: the same however the tiles are split over calls. */
int keep_heat_accumulate_cells(keep_handle* h, const int64_t* coords, const float* values, int64_t N, int64_t gh, int64_t gw, int64_t patch,
                               int64_t downsample, int64_t H, int64_t W, int64_t origin_x, int64_t origin_y, int zero_first, int64_t* acc,
                               void* stream);
/* Replaces: reading the raster back as numbers (the probability map in slide geometry; the {0,255} pred_mask of
 * segment_utils.py:134-140 when the values were p > thd).  mean_out: fp32 [H,W] = float(double(sum) / double(65535 count)) where
 * count > 0, else `uncovered`; count_out: int32 [H,W]; pred_out: uint8 [H,W], 255 where sum > 0.  Any of the three may be null, not
 * all. */
int keep_heat_mean(keep_handle* h, const int64_t* acc, int64_t H, int64_t W, float uncovered, float* mean_out, int32_t* count_out,
                   unsigned char* pred_out, void* stream);
/* Replaces: the heatmap blended over the thumbnail that closes CLAM's step of README.md:74.  CLAM's percentile ranks and blur are
 * calls of their own, made before this one: keep_sort_f32 / keep_rank_f32 on the tile values, keep_heat_smooth on the accumulator.
 * thumb: uint8 [H,W,C] RGB / RGBA with the layout contract of keep_region_grid, or null for the constant background_rgb
 * (R | G << 8 | B << 16).  mask: uint8 [H,W] contiguous (non-zero = show), or null.  lut: uint8 [256,3].  With S = sum, c = count a
 * pixel is shown iff c > 0, the mask is set and S >= min16 c; its colour index is clamp((2 255 (S - lo16 c) + (hi16 - lo16) c) /
 * (2 (hi16 - lo16) c), 0, 255) (0 when S < lo16 c) and out = (alpha lut[idx] + (256 - alpha) under + 128) >> 8 per channel; other
 * pixels pass `under` through.  0 <= alpha <= 256, 0 <= lo16 < hi16 <= 65535, 0 <= min16 <= 65535.  out: uint8 [H,W,3] contiguous. */
int keep_heat_render(keep_handle* h, const int64_t* acc, int64_t H, int64_t W, const unsigned char* thumb, int64_t row_stride_bytes,
                     int pix_stride, int background_rgb, const unsigned char* mask, const unsigned char* lut, int alpha, int lo16, int hi16,
                     int min16, unsigned char* out, void* stream);

/* ---- heatmap percentiles and smoothing ---------------------------------------
 * Replaces: the Gaussian blur of the overlay in the heatmap that closes CLAM's step of README.md:74, restated as a normalised
 * convolution in integers (no parity with an image library's border handling is claimed).  acc as above; mask: uint8 [H,W]
 * contiguous (non-zero = inside), or null; taps: int32 [2 radius + 1] ON THE DEVICE, every tap >= 0, the centre tap >= 1, their sum
 * <= 32768 (the caller's precondition: a table that breaks it gives meaningless values, nothing worse); 1 <= radius <= 127.
 * With S, c the fields of a pixel: s = c > 0 and the mask is set; m = s ? (2 S + c) / (2 c) : 0 (the mean in 16-bit fixed point,
 * rounded half up: peak16's rule).  A = sum_k taps[k] m(y, x + k), B = sum_k taps[k] s(y, x + k) along the row, Nn = sum_k taps[k]
 * A(y + k, x), D = sum_k taps[k] B(y + k, x) along the column, pixels outside the raster without support;
 * acc_out = s ? (1 << 40) | (2 Nn + D) / (2 D) : 0, an accumulator of count 1 that every call above reads unchanged.  Pixels
 * without support neither give nor receive; a constant region stays constant.  PRECONDITION on acc: S <= 65535 c (see
 * keep_regions_table).  acc_out: int64 [H,W], 8-byte aligned, not acc.  Workspace (6 bytes per pixel) comes from the handle's arena. */
int keep_heat_smooth(keep_handle* h, const int64_t* acc, int64_t H, int64_t W, const unsigned char* mask, const int32_t* taps, int radius,
                     int64_t* acc_out, void* stream);
/* Replaces: the sorted score population behind CLAM's percentile heatmaps (scipy.stats.rankdata over the slide's own tiles,
 * percentileofscore against a reference population; the step of README.md:74).  values: fp32 [M], 1 <= M <= 2^24 - 1.  NaNs of any
 * payload or sign are not part of the population and -0.0 counts as +0.0: sorted_out[0:n] holds the n other values in ascending
 * order (-0 stored as +0), sorted_out[n:M] the NaN 0x7FC00000, *n_out = n (one int64 ON THE DEVICE).  sorted_out may be values.
 * No host synchronisation; workspace (4 bytes per value + the digit tables, none up to 4096 values) comes from the handle's arena. */
int keep_sort_f32(keep_handle* h, const float* values, int64_t M, float* sorted_out, int64_t* n_out, void* stream);
/* Replaces: scipy.stats.rankdata(v, 'average') (self = 1: the queries ARE the population, r2 = 2 less + eq + 1 = twice the average
 * rank) and scipy.stats.percentileofscore(ref, q, kind='mean') (self = 0: r2 = 2 less + eq) of CLAM's heatmap step.  sorted, M: the
 * output of keep_sort_f32; n_dev: its n_out, read on the device.  queries: fp32 [N], 0 <= N <= 2^24 - 1.  For a query q that is
 * not NaN: less = #{sorted[0:n] < q}, eq = #{sorted[0:n] == q} by float comparison, pct = float(double(r2) / double(2 n)), NaN
 * when n = 0.  A NaN query gives pct = NaN and less = eq = -1.  pct_out fp32 [N], less_out / eq_out int32 [N]: any may be null,
 * not all. */
int keep_rank_f32(keep_handle* h, const float* sorted, int64_t M, const int64_t* n_dev, const float* queries, int64_t N, int self,
                  float* pct_out, int32_t* less_out, int32_t* eq_out, void* stream);

/* Region table: the connected regions of a mask, numbered, with geometry and scores.
 * Replaces: the list of tissue contours with areas and boxes that CLAM's segmentTissue hands back (the step of README.md:74), and
 * the per-lesion reading of a tumour-probability map that follows WSI_evaluation/segment_utils.py's pred_mask; restated on the
 * pixel mask, integer arithmetic, exact.
 * keep_regions_label: mask uint8 [H,W] contiguous, non-zero = foreground, 1 <= H W <= 2^30.  Components are 4- or 8-connected
 * (connectivity); one is KEPT iff it holds >= min_area pixels (min_area >= 1; keep_tissue_mask's rule is the other way round:
 * DROPPED iff <= min_area).  The kept components are numbered 1..n in the row-major order of their first pixels, which is
 * scipy.ndimage.label's numbering with the dropped ones removed.  labels_out: int32 [H,W], 0 = background or dropped; n_out: one
 * int64 ON THE DEVICE.  Workspace (8 bytes per pixel) comes from the handle's arena.  A labelling loop that runs into its
 * iteration cap sets bit 2 (value 4) of the handle's sticky error word (keep_token_error).
 * keep_regions_table: labels int32 [H,W] with values 0..n (a value outside 1..n counts as background), n >= 0 as read back from
 * n_out; acc: the int64 [H,W] accumulator of keep_heat_accumulate (bits 0..39 the sum S, bits 40..63 the count c), 8-byte aligned,
 * or NULL.  table_out: int64 [n,14] (may be NULL when n = 0), row i - 1 for label i:
 *   0 first_x, 1 first_y  the region's first pixel in row-major order     7 sum_x, 8 sum_y  sums of the pixels' column / row indices
 *   2 area                pixels                                           9 border          1 iff a pixel lies in row 0 / H - 1 or column 0 / W - 1
 *   3 x0, 4 y0, 5 x1, 6 y1  bounding box, x1 / y1 exclusive               10 covered         pixels with c > 0
 *  11 sum_c, 12 sum_s     sums of c and of S over the region              13 peak16          max over covered pixels of (2 S + c) / (2 c)
 * Columns 10..13 are 0 without acc.  sum_s must fit: the caller checks tiles * (patch / downsample + 1)^2 * 65535 < 2^63.
 * PRECONDITION on acc: every word satisfies S <= 65535 c, as every word keep_heat_accumulate writes does (each tile adds at most
 * 65535 to S and 1 to c).  The pixel mean is then <= 65535 and peak16 is carried in 32 bits; a word that breaks this (c = 1 with
 * S >= 2^31, say) is not detected and its peak16 is truncated to 32 bits.  The other columns do not depend on it.
 * Integer sums, minima and maxima: the table is the same from run to run. */
int keep_regions_label(keep_handle* h, const unsigned char* mask, int64_t H, int64_t W, int connectivity, int64_t min_area,
                       int32_t* labels_out, int64_t* n_out, void* stream);
int keep_regions_table(keep_handle* h, const int32_t* labels, int64_t H, int64_t W, int64_t n, const int64_t* acc, int64_t* table_out,
                       void* stream);

/* Region shape: second moments and the exact largest diameter of every region.
 * Replaces: scikit-image's regionprops(...).major_axis_length, by which the CAMELYON16 evaluation sets isolated tumour cells aside,
 * and the "largest dimension" a pathologist reads off a lesion; integer arithmetic on the device, exact, the same from run to run.
 * labels: int32 [H,W] as keep_regions_label writes it (a value outside 1..n counts as background), 1 <= H W <= 2^30; table: the
 * int64 [n,14] table of keep_regions_table ON THE DEVICE, of which only the box (x0, y0, x1, y1) is read.
 * keep_regions_moments: moments_out int64 [n,3], row i - 1 for label i: sum_uu, sum_vv, sum_uv over the region's pixels with
 * u = x - x0, v = y - y0 (the box origin; only x0, y0 are read).  A label no pixel carries gives a zero row.  The caller checks
 * H W max(H, W)^2 < 3 * 2^63, under which no sum leaves int64.  No workspace, no host synchronisation.
 * keep_regions_feret: needs (H + 1) (W + 1) <= 2^31 as well.  Region i is the union of the closed unit squares of its pixels;
 * feret_out int64 [n,5], row i - 1: d2, ax, ay, bx, by: the largest squared distance between two corner-lattice points of the
 * region and the pair that reaches it, a < b in lattice row-major order y (W + 1) + x, the smallest a first, then the smallest b.
 * A label no pixel carries gives a zero row.  Candidates are the corners of the first and last pixel of every row of the region
 * (every column where the box is taller than wide): 4 min(bw, bh) per region.  The candidate total and the pair total (the sum of
 * c^2 / 2 over the regions) are read back once -- the call's one host synchronisation -- and written to totals_out (two int64 ON
 * THE HOST, may be NULL); more than max_pairs (0 .. 2^50) pairs is KEEP_EINVAL and nothing is computed.  Workspace (16 bytes per
 * region and 2 bytes per candidate) comes from the handle's arena.  A table that is not the labels' own gives wrong rows, never
 * a write out of bounds. */
int keep_regions_moments(keep_handle* h, const int32_t* labels, int64_t H, int64_t W, int64_t n, const int64_t* table,
                         int64_t* moments_out, void* stream);
int keep_regions_feret(keep_handle* h, const int32_t* labels, int64_t H, int64_t W, int64_t n, const int64_t* table, int64_t max_pairs,
                       int64_t* feret_out, int64_t* totals_out, void* stream);

/* ---- the subtype map ----------------------------------------------------------
 * Replaces: nothing the reference draws; it gives the subtyping flow of WSI_evaluation/subtyping_utils.py:67-83 (refined tile
 * probabilities -> argmax -> tile shares -> one slide label) the spatial output the other two flows have.  The class raster `acc`
 * is int64 [C,H,W] contiguous on the device, 8-byte aligned, 1 <= C <= 64, C H W <= 2^30; plane c is an accumulator of
 * keep_heat_accumulate (sum of q in bits 0..39, number of tiles in bits 40..63) over the tiles' values of class c.
 *
 * keep_heat_accumulate_classes (subtyping_utils.py:67-83: the [U,C] refined probabilities, kept where the reference reduces them):
 * coords int64 [N,2], values fp32 [N,C] row-major; footprint, quantisation, limits and checks of keep_heat_accumulate; every (tile,
 * pixel, class) adds (1 << 40) | q_c into plane c.  A tile whose row holds a NaN is skipped in every plane, so the count is the
 * same in all planes.  It always adds into acc: the caller zeroes a new raster.  Integer sums: the same however the tiles are
 * split over calls. */
int keep_heat_accumulate_classes(keep_handle* h, const int64_t* coords, const float* values, int64_t N, int64_t C, int64_t patch,
                                 int64_t downsample, int64_t H, int64_t W, int64_t origin_x, int64_t origin_y, int64_t* acc, void* stream);
/* The per-pixel call of subtyping_utils.py:67-83 (`argmax(dim=1)` there per tile, here per pixel over the covering tiles' sums).  With
 * n = the count of plane 0 and S_c the sums: n = 0, or a zero in mask (uint8 [H,W], may be null), gives label 255 and top = margin
 * = 0.  Otherwise label = the smallest c with the largest S_c, S_second = the largest S_c over c != label (0 when C = 1), top =
 * (n << 40) | S_label, margin = (n << 40) | (S_label - S_second), and the label becomes 254 (undecided) iff S_label < min16 n or
 * S_label - S_second < margin16 n.  0 <= min16, margin16 <= 65535.  label_out uint8 [H,W], top_out / margin_out int64 [H,W] (8-byte
 * aligned; both are accumulators every keep_heat_* call reads): any may be null, not all. */
int keep_class_argmax(keep_handle* h, const int64_t* acc, int64_t C, int64_t H, int64_t W, const unsigned char* mask, int min16, int margin16,
                      unsigned char* label_out, int64_t* top_out, int64_t* margin_out, void* stream);
/* The confusion of two label maps, the multi-class counterpart of keep_eval_mask_counts for the labels of subtyping_utils.py:67-83.
 * a, b: uint8 [H,W]; within: uint8 [H,W] or null (non-zero = counted); 1 <= C <= 64, 1 <= H W <= 2^30.  counts_out: int64
 * [(C + 1)^2], 8-byte aligned, zeroed by the call; counts[i (C + 1) + j] = the pixels inside `within` with a = i and b = j, every
 * label >= C (254 and 255 among them) counted at index C.  a and b may be the same map: the diagonal then holds the class areas. */
int keep_class_confusion(keep_handle* h, const unsigned char* a, const unsigned char* b, const unsigned char* within, int64_t H, int64_t W,
                         int64_t C, int64_t* counts_out, void* stream);
/* The label map of subtyping_utils.py:67-83's classes as a picture.  labels: uint8 [H,W]; palette: uint8 [C,3]; thumb / row stride /
 * pixel stride / background_rgb as keep_heat_render.  A pixel with label >= C passes `under` through.  Otherwise a_eff = alpha, or
 * with strength (an int64 [H,W] accumulator, 8-byte aligned, or null) a_eff = (alpha idx + 127) / 255 with idx the colour index
 * keep_heat_render gives that word in the window [lo16, hi16] (0 where its count is 0), and out = (a_eff palette[label] +
 * (256 - a_eff) under + 128) >> 8 per channel.  0 <= alpha <= 256, 0 <= lo16 < hi16 <= 65535.  out: uint8 [H,W,3] contiguous. */
int keep_class_render(keep_handle* h, const unsigned char* labels, int64_t H, int64_t W, int64_t C, const unsigned char* thumb,
                      int64_t row_stride_bytes, int pix_stride, int background_rgb, const unsigned char* palette, int alpha,
                      const int64_t* strength, int lo16, int hi16, unsigned char* out, void* stream);

/* ---- tile clustering -------------------------------------------------------------
 * Replaces: nothing in the reference, which has no unsupervised path; on this engine the host round trip keep_similarity(ARGMAX) +
 * an index_add of the feature rows + a normalise, which reads the features twice per iteration, writes an [N,K] matrix and sums the
 * centroids in float in arrival order.  Spherical k-means: features fp32 [N,D] row-major unit rows, centroids fp32 [K,D] unit rows,
 * both 16-byte aligned; 1 <= N <= 2^22 per call, D a multiple of 16 in 16 .. 1024, 1 <= K <= 64 (every result fits a class raster);
 * at most 2^24 rows may be added into one set of accumulators (2^30 2^24 = 2^54 fits the word).  Anything else is KEEP_EINVAL and
 * nothing is launched.
 *
 * keep_cluster_assign: score = x . c as a k-ordered fp32 fma chain (v_mfma_f32_16x16x4_f32) whose order does not depend on N, on the
 * row's position or on the split over calls.  label_out int32 [N]: the smallest k with the largest score; best_out fp32 [N]: that
 * score; margin_out fp32 [N]: best minus the largest score of the other centroids (0 when K = 1).  A row holding a non-finite value
 * or an element with |x| > 1 is skipped: label -1, best = margin = 0, one added to *skipped, absent from every sum.  *changed +=
 * the rows with label != prev_label[row] (prev_label int32 [N]; it may be label_out).  With accumulators the same launch adds every
 * kept row: sums int64 [K,D] += llrint(x 2^30) into row `label`, counts int64 [K] += 1, *cos_sum += llrint(best 2^30).  Integer
 * sums: the same words however the rows are ordered or split over calls.  The call ALWAYS ADDS into skipped, changed, sums, counts
 * and cos_sum (int64, 8-byte aligned, on the device): the caller zeroes them.  May be null: best_out, margin_out, skipped; changed
 * and prev_label (both or neither); sums, counts and cos_sum (all or none); label_out when the accumulators are given.
 * two_launch = 1 runs the accumulate as a second launch over label_out / best_out (both then required): the same words, kept for
 * measurement (tools/cluster_bench.py).
 * keep_cluster_update: centroids[k] = (float)(s / sqrt(sum s^2)) with s_d = (double)sums[k,d] 2^-30, in fp64.  A cluster with
 * counts[k] = 0 or a zero sum keeps its row of `centroids` bit for bit; empty_out uint8 [K] (may be null) is written 1 for those, 0 for
 * the others.  One launch; sums and counts are only read.
 * keep_cluster_seed_step: one step of farthest-point seeding.  The centre is `centre` (fp32 [D], 16-byte aligned) or, with centre
 * null, row *centre_row of features (one int64 ON THE DEVICE, e.g. the index_out of the step before; clamped into 0 .. N - 1).
 * first = 0: nearest[r] = max(nearest[r], x_r . c) (fp32 [N], the caller starts it at -inf) and *index_out = the row with the smallest
 * nearest, the lowest row on a tie.  first = 1: nearest is not touched (may be null) and *index_out = the row with the LARGEST x_r . c,
 * the lowest row on a tie.  Skipped rows (the rule above) take no part and keep their nearest; with every row skipped *index_out =
 * -1.  index_out: one int64 ON THE DEVICE.  No host synchronisation; workspace: 8 bytes of the handle's arena. */
int keep_cluster_assign(keep_handle* h, const float* features, int64_t N, int64_t D, const float* centroids, int64_t K, int32_t* label_out,
                        float* best_out, float* margin_out, const int32_t* prev_label, int64_t* skipped, int64_t* changed, int64_t* sums,
                        int64_t* counts, int64_t* cos_sum, int two_launch, void* stream);
int keep_cluster_update(keep_handle* h, const int64_t* sums, const int64_t* counts, int64_t K, int64_t D, float* centroids,
                        unsigned char* empty_out, void* stream);
int keep_cluster_seed_step(keep_handle* h, const float* features, int64_t N, int64_t D, const float* centre, const int64_t* centre_row, int first,
                           float* nearest, int64_t* index_out, void* stream);

/* ---- linear probe ----------------------------------------------------------------
 * Replaces: nothing in the reference, which scores frozen features against prompts only; on this engine the round trip through
 * sklearn.linear_model.LogisticRegression on the host, or per iteration x @ W.T + b, softmax and (p - onehot).T @ x in torch, which
 * reads the features twice, writes two [N,C] matrices and sums the gradient in float in an order the library picks.  Multinomial
 * logistic regression: features fp32 [N,D] row-major unit rows and weight fp32 [C,D], both 16-byte aligned, bias fp32 [C];
 * 1 <= N <= 2^22 per call, D a multiple of 16 in 16 .. 1024, 2 <= C <= 64; at most 2^24 rows may be added into one set of
 * accumulators.  groups: 0, or 1 / 2 / 4 groups of 64 rows per workgroup (any value gives the same words; for measurement), with
 * groups ceil(C / 16) <= 8 in keep_probe_loss_grad.  Anything else is KEEP_EINVAL and nothing is launched.
 *
 * keep_probe_forward: z_c = x . w_c as a k-ordered fp32 fma chain (v_mfma_f32_16x16x4_f32) plus bias[c]; a row's logits do not depend
 * on N, on its position or on the split over calls.  probs_out fp32 [N,C]: exp(z_c - max z) / sum, fp32, the sum in one fixed order;
 * label_out int32 [N]: the smallest c with the largest logit; best_out fp32 [N]: its probability; margin_out fp32 [N]: best minus the
 * runner-up's probability.  A row holding a non-finite value or an element with |x| > 1 (or whose logits are not finite) is skipped:
 * label -1, best = margin = 0, a zero row of probs, one added to *skipped (int64 on the device, ADDED into).  Every output may be
 * null, not all of them.  No host synchronisation.
 * keep_probe_loss_grad: the same forward (its outputs optional) and the integer sums of F = (1/S) sum_i w[y_i] loss_i with loss_i =
 * logsumexp(z_i) - z_i[y_i].  labels int32 [N]: -1 (unlabelled: in no sum, still predicted) or 0 .. C - 1; class_weight fp32 [C] in
 * (0, 1], or null for 1.  A label or weight outside that is KEEP_EINVAL, found by one check launch and a 4-byte read-back (the one
 * host synchronisation) before a label is used.  With r_ic = w[y_i] (p_ic - [c = y_i]) (the subtraction, then the product, single
 * fp32 operations) every kept row adds grad[c,d] += llrint(fp32(r_ic x_id) 2^30), gbias[c] += llrint(r_ic 2^30), *loss +=
 * llrint(fp32(w[y_i] loss_i) 2^24), counts[y_i] += 1; a skipped row adds one to *skipped.  grad int64 [C,D], gbias int64 [C], loss
 * int64 [1], counts int64 [C], skipped int64 [1], 8-byte aligned on the device, all required: the call ALWAYS ADDS, the caller
 * zeroes.  Every term is rounded before it is added, so the words are the same however the rows are ordered, grouped or split over
 * calls.  loss_i < 2^15 keeps the loss word exact: the caller holds max_c(|w_c| + |b_c|) under 8192. */
int keep_probe_forward(keep_handle* h, const float* features, int64_t N, int64_t D, const float* weight, const float* bias, int64_t C,
                       float* probs_out, int32_t* label_out, float* best_out, float* margin_out, int64_t* skipped, int groups, void* stream);
int keep_probe_loss_grad(keep_handle* h, const float* features, int64_t N, int64_t D, const int32_t* labels, const float* weight, const float* bias,
                         int64_t C, const float* class_weight, int64_t* grad, int64_t* gbias, int64_t* loss, int64_t* counts, int64_t* skipped,
                         float* probs_out, int32_t* label_out, float* best_out, float* margin_out, int groups, void* stream);

/* ---- attention MIL ---------------------------------------------------------------
 * Replaces: nothing in the reference, which has no slide-level supervised protocol; on this engine a torch loop of x @ V.T, tanh, a
 * segment softmax, index_add_ and R.T @ x, whose float sums depend on the order the library picks.  Attention-based multiple-instance
 * learning (Ilse, Tomczak and Welling 2018): features fp32 [N,D] row-major unit rows in S bags of contiguous rows; V fp32 [L,D], bv and
 * w fp32 [L]; features and V 16-byte aligned; 1 <= N <= 2^22 and 1 <= S <= 2^16 per call, D a multiple of 16 in 16 .. 1024, L a
 * multiple of 16 in 16 .. 128.  chunks int32 [n_chunks,3] on the device: (bag, first row, rows), every bag cut from its own first
 * row into runs of at most KEEP_MIL_CHUNK rows (an empty bag has none).  THE WORDS DEPEND ON KEEP_MIL_CHUNK: it is part of the
 * contract.  A chunk outside [0,S) x [0,N) or with rows outside 1 .. KEEP_MIL_CHUNK is KEEP_EINVAL, found by one check launch and a
 * 4-byte read-back (the one host synchronisation of each call) before the table is an index.  Anything else above is KEEP_EINVAL
 * too and nothing is launched.  workspace: device memory of at least keep_mil_workspace_bytes(N, D, S) bytes, 256-byte aligned, the
 * caller's; keep_mil_backward reads what keep_mil_forward left in it for the same features and table.
 *
 * keep_mil_forward: h_i = tanhf(V x_i + bv) (a k-ordered fp32 fma chain on v_mfma_f32_16x16x4_f32, the bias after it), s_i = w . h_i in
 * one fixed order; a row's s and h depend on that row alone.  Per bag: m_b = max s, e_i = expf(s_i - m_b), Z_b = sum llrint(e_i 2^40),
 * P_b[d] = sum llrint(fp32(e_i x_id) 2^40) (integers: any order), attn_out[i] = e_i / fp32(Z_b 2^-40), pooled_out[b,d] =
 * fp32(P_b[d] / Z_b).  A row holding a non-finite value or an element with |x| > 1 (or whose score is not finite) is skipped:
 * scores_out -inf, attention 0, in no sum, one added to *skipped_rows.  A bag without a kept row: a zero pooled row, kept_rows_out
 * 0, head label -1, one added to *skipped_bags.  scores_out / attn_out fp32 [N], pooled_out fp32 [S,D], kept_rows_out int32 [S]:
 * required.  hidden_out fp32 [N,L] (the backward needs it) and head_labels_out int32 [S] (labels[b], or 0 without labels, for a bag
 * with a kept row, else -1: the labels of the head, keep_probe_loss_grad on pooled_out) may be null; labels int32 [S] may be null.
 * skipped_rows / skipped_bags: int64 on the device, ADDED into.
 * keep_mil_backward: after the head.  probs fp32 [S,C] and head_labels as the head saw them, Wc fp32 [C,D], class_weight fp32 [C] or
 * null, 2 <= C <= 64.  r_bc = cw[y_b] (p_bc - [c = y_b]) as the probe forms it, dz_b = sum_c r_bc Wc[c,:] (c ascending, fma), u_b =
 * dz_b . z_b, da_i = dz_b . x_i, ds_i = a_i (da_i - u_b), each in one fixed order; R_il = fp32(ds_i w_l) fp32(1 - fp32(h_il^2)).  Per
 * chunk gV[l,d] += llrint(acc 2^36), acc the fp32 MFMA chain of R_il x_id over the chunk's rows in row order (one rounding per
 * chunk and word); gbv[l] += llrint(R_il 2^36) and gw[l] += llrint(fp32(ds_i h_il) 2^36) per term.  gV int64 [L,D], gbv / gw int64
 * [L], 8-byte aligned, all required: the call ALWAYS ADDS, the caller zeroes.  A bag with head label -1 adds nothing.  A bag's
 * contribution to every word depends on that bag alone: the same words for every split of the bags over calls and every order.
 * A bag adds at most G = 4 max(1, max|w|) max_c |Wc_c|_1 to a word: the caller holds G <= 2^10 and the bags added into one set of
 * accumulators <= 2^16, which keeps |word| <= 2^62.  ds_out fp32 [N] (may be null): the rows' ds_i, 0 for a row in no sum. */
#ifndef KEEP_MIL_CHUNK
#define KEEP_MIL_CHUNK 512
#endif
int keep_mil_chunk(void);
int keep_mil_workspace_bytes(keep_handle* h, int64_t N, int64_t D, int64_t S, int64_t* bytes);
int keep_mil_forward(keep_handle* h, const float* features, int64_t N, int64_t D, const int32_t* chunks, int64_t n_chunks, int64_t S,
                     const int32_t* labels, const float* V, const float* bv, const float* w, int64_t L, float* scores_out, float* attn_out,
                     float* pooled_out, int32_t* kept_rows_out, float* hidden_out, int32_t* head_labels_out, int64_t* skipped_rows,
                     int64_t* skipped_bags, void* workspace, int64_t workspace_bytes, void* stream);
int keep_mil_backward(keep_handle* h, const float* features, int64_t N, int64_t D, const int32_t* chunks, int64_t n_chunks, int64_t S,
                      const int32_t* head_labels, const float* probs, const float* Wc, int64_t C, const float* class_weight, const float* w,
                      int64_t L, const float* scores, const float* attn, const float* pooled, const float* hidden, int64_t* gV, int64_t* gbv,
                      int64_t* gw, float* ds_out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- nearest neighbours ----------------------------------------------------------
 * Replaces: the [N,M] keep_similarity matrix + torch.topk round trip on this engine, and the reference's
 * arr.argsort()[-50:][::-1] over a host similarity row (training/path_training/zero_shot.py:168-171), which lists the HIGHER index
 * first among equal scores; here the lower index comes first.  queries fp32 [Nq,D] and bank fp32 [M,D], row-major unit rows, both
 * 16-byte aligned; 1 <= Nq, M <= 2^22 per call, D a multiple of 16 in 16 .. 1024, 1 <= k <= 64, 0 <= bank_base and bank_base + M <=
 * 2^32 - 1.  Anything else is KEEP_EINVAL and nothing is launched.
 *
 * The order is total.  A neighbour is one 64-bit key, KEEP_TOPK_KEY(KEEP_TOPK_ORD(bits of score + 0.0f), g) with g the row's GLOBAL
 * bank index (bank_base + its row in this call): a larger key is a larger score, and of equal scores the lower index.  0 is the empty
 * slot, below the key of every finite score.  A list is k keys in descending order, its empty slots last; the top k of a union of
 * candidates is the k largest keys of the union, so lists merge exactly across calls, chunks, files and devices.  The keys are
 * part of the ABI.
 * keep_topk: score = q . b as cluster_assign's k-ordered fp32 fma chain from 0 (v_mfma_f32_16x16x4_f32; the score of (query i, bank
 * row r) is the `best` of keep_cluster_assign(queries, bank + r D, K = 1) bit for bit).  A row holding a non-finite value or an element
 * with |x| > 1 is skipped: a skipped bank row is never a candidate, a skipped query row's list is left as it was (empty with merge =
 * 0); *query_skipped / *bank_skipped (int64 on the device, may be null) are ADDED into, a bank row counted once per call.  keys:
 * uint64 [Nq,k], 8-byte aligned.  merge = 0: the lists are written; merge = 1: the descending lists already there are candidates too
 * (zeroed by the caller before the first call).  Offering the same global row twice across merged calls is the caller's error and
 * is not detected: the row then appears twice.  self_first >= 0: query row i never takes global row self_first + i.  With fewer than
 * k candidates the tail slots stay empty.  segments: 0 (chosen here), or 1 .. 1024 cuts of the bank run by different workgroups
 * and merged by keys (any value gives the same words; for measurement); workspace segments ceil64(Nq) k 8 bytes of the handle's
 * arena.  No host synchronisation.
 * keep_topk_merge: out = the k largest keys of lists a and b of the same queries (out may be a).
 * keep_topk_unpack: index_out int64 [Nq,k] (the global index, -1 for an empty slot), score_out fp32 [Nq,k] (exactly the fp32 in the
 * key, 0 for an empty slot), count_out int32 [Nq] (the filled slots); each may be null, not all.
 * keep_knn_vote: neighbour r = 0 .. k - 1 in list order votes for bank_labels[g_r] (int32 [n_bank]) when that lies in 0 .. C - 1
 * (anything else, such as -1, does not vote) with weight 1 (KEEP_KNN_UNIFORM) or expf((s_r - s_0) / temperature) (KEEP_KNN_SOFTMAX;
 * s_0 the list's best score, temperature > 0, the subtraction and the division single fp32 operations).  v_c = the fp32 sum of class
 * c's weights in list order, probs_out fp32 [Nq,C] = v_c / (v_0 + v_1 + .. in class order), label_out int32 [Nq] = the smallest c
 * with the largest v_c, margin_out fp32 [Nq] = the winner's probability minus the runner-up's.  A query without a voting neighbour
 * (or whose votes sum to 0): label -1, a zero row, margin 0, one ADDED to *skipped (int64 on the device).  2 <= C <= 64; outputs may
 * be null, not all.  A key whose index is >= n_bank is KEEP_EINVAL, found by one check launch and a 4-byte read-back (the one host
 * synchronisation) before a label is read. */
#define KEEP_TOPK_EMPTY 0ull
#define KEEP_TOPK_ORD(u) ((uint32_t)(u) ^ ((((uint32_t)(u)) >> 31) ? 0xFFFFFFFFu : 0x80000000u))       /* u: the bits of score + 0.0f */
#define KEEP_TOPK_KEY(ord, g) (((uint64_t)(uint32_t)(ord) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)(g)))
#define KEEP_TOPK_INDEX(key) (0xFFFFFFFFu - (uint32_t)(key))
#define KEEP_TOPK_SCORE_BITS(ord) ((((uint32_t)(ord)) & 0x80000000u) ? ((uint32_t)(ord) ^ 0x80000000u) : ~(uint32_t)(ord))
enum { KEEP_KNN_UNIFORM = 0, KEEP_KNN_SOFTMAX = 1 };
int keep_topk(keep_handle* h, const float* queries, int64_t Nq, const float* bank, int64_t M, int64_t D, int k, int64_t bank_base,
              int64_t self_first, int merge, uint64_t* keys, int64_t* query_skipped, int64_t* bank_skipped, int segments, void* stream);
int keep_topk_merge(keep_handle* h, const uint64_t* a, const uint64_t* b, int64_t Nq, int k, uint64_t* out, void* stream);
int keep_topk_unpack(keep_handle* h, const uint64_t* keys, int64_t Nq, int k, int64_t* index_out, float* score_out, int32_t* count_out,
                     void* stream);
int keep_knn_vote(keep_handle* h, const uint64_t* keys, int64_t Nq, int k, const int32_t* bank_labels, int64_t n_bank, int64_t C, int mode,
                  float temperature, float* probs_out, int32_t* label_out, float* margin_out, int64_t* skipped, void* stream);

/* ---- feature PCA ------------------------------------------------------------------
 * Replaces: nothing in the reference, which never looks at the feature space itself; on this engine xc = x - x.mean(0); xc.T @ xc in
 * torch, which reads the features twice, materialises xc, sums in an order the library picks and loses the small eigenvalues to the
 * features' common mean.  features fp32 [N,D] row-major unit rows, 16-byte aligned; 1 <= N <= 2^22 per call, D a multiple of 16 in
 * 16 .. 1024; at most 2^24 rows may be added into one set of accumulators.  Anything else is KEEP_EINVAL and nothing is launched.  A
 * row holding a non-finite value or an element with |x| > 1 is skipped exactly as in keep_cluster_assign: in no sum, one added to
 * *skipped.  No host synchronisation.
 *
 * keep_pca_moments: sum int64 [D] += llrint(x_d 2^30) per kept row and column (every term rounded before it is added: the fixed
 * point of keep_cluster_assign's sums), count int64 [1] += the kept rows.  gram int64 [D,D] (may be NULL: sum and count alone): the
 * rows of the call are cut from its row 0 into chunks of KEEP_PCA_CHUNK rows; per chunk and word acc = the fp32
 * v_mfma_f32_16x16x4_f32 chain of a_id a_ie over the chunk's rows in row order, a_i = fp32(x_i - centre) (one fp32 subtraction per
 * element; a skipped row is a zero row; the tail padded with zero rows to a multiple of 4), and gram[d,e] += llrint(acc 2^32): one
 * rounding per chunk and word, one no-return 64-bit atomic.  centre: fp32 [D], 16-byte aligned, |c_d| <= 1 (THE CALLER'S
 * precondition, not checked on the device), or NULL for zero.  Only the 16 x 16 tiles with tile row <= tile column are written,
 * the diagonal tiles in full (and symmetric bit for bit); the words below are never touched.  |a| <= 2, so |acc| <= 4 x 512 =
 * 2^11, a chunk adds at most 2^43 to a word and the 2^15 chunks of 2^24 rows at most 2^58.  sum, count, gram, skipped: int64, 8-byte
 * aligned, on the device; sum and count are required, skipped may be NULL.  The call ALWAYS ADDS: the caller zeroes.
 * THE WORDS OF gram DEPEND ON KEEP_PCA_CHUNK and on where the chunk boundaries fall: both are part of the contract.  They do not
 * depend on the grid, on how many chunks a workgroup walks, on the order of the calls or on a split of the rows over calls at
 * multiples of the chunk; sum and count do not depend on the split at all.  groups: 0 (chosen here) or 1 .. 64 chunks walked by
 * a workgroup before it issues its atomics, the per-chunk rounded integers summed in registers: any value gives the same words
 * (for measurement, tools/pca_bench.py).  Workspace (one byte per row) comes from the handle's arena.
 * keep_pca_project: out fp32 [N,k], out[i,j] = fp32(fp32(chain_j(x_i) + bias[j]) * scale[j]) with chain_j the k-ordered fp32 fma chain
 * of x_i . w_j in keep_cluster_assign's operand flow; components fp32 [k,D], 16-byte aligned, 1 <= k <= 64; bias / scale fp32 [k] or
 * NULL, and a step whose vector is NULL is not made: with both NULL out[:,j] is the `best` of keep_cluster_assign(features, w_j,
 * K = 1) bit for bit.  A row's scores depend on that row alone.  A skipped row: a zero row of out, kept_out[i] = 0 (uint8 [N], may be
 * NULL; 1 for the other rows), one added to *skipped (may be NULL).
 * keep_class_render_rgb: three planes of a class raster (acc int64 [C,H,W] as keep_heat_accumulate_classes leaves it) as one
 * colour picture.  planes: three ints ON THE HOST in 0 .. C - 1, for red, green and blue.  With S, c the fields of a plane's word a
 * pixel is shown iff c > 0 and the mask (uint8 [H,W] or NULL) is set; its channel is v = min(255, (2 255 S + 65535 c) / (2 65535 c))
 * (the colour index keep_heat_render gives the window [0, 65535]) and out = (alpha v + (256 - alpha) under + 128) >> 8; other pixels
 * pass `under` through.  thumb / row stride / pixel stride / background_rgb as keep_heat_render; 0 <= alpha <= 256.  out: uint8
 * [H,W,3] contiguous. */
#ifndef KEEP_PCA_CHUNK
#define KEEP_PCA_CHUNK 512
#endif
int keep_pca_chunk(void);
int keep_pca_moments(keep_handle* h, const float* features, int64_t N, int64_t D, const float* centre, int64_t* sum, int64_t* count,
                     int64_t* gram, int64_t* skipped, int groups, void* stream);
int keep_pca_project(keep_handle* h, const float* features, int64_t N, int64_t D, const float* components, int64_t k, const float* bias,
                     const float* scale, float* out, unsigned char* kept_out, int64_t* skipped, void* stream);
int keep_class_render_rgb(keep_handle* h, const int64_t* acc, int64_t C, int64_t H, int64_t W, const int* planes, const unsigned char* thumb,
                          int64_t row_stride_bytes, int pix_stride, int background_rgb, const unsigned char* mask, int alpha,
                          unsigned char* out, void* stream);

/* ---- exact t-SNE of tile features --------------------------------------------------
 * Replaces: nothing in the reference; on this engine a trip to scikit-learn or openTSNE on the host.  Every buffer is the caller's: no
 * workspace comes from the handle.  1 <= N <= 2^20 rows; anything else named below is KEEP_EINVAL and nothing is launched.  No host
 * synchronisation.
 *
 * keep_tsne_affinities: neighbour lists (index int64 [N,k], score fp32 [N,k], count int32 [N] as keep_topk_unpack leaves them, 1 <= k <=
 * 64) -> p_out fp32 [N,k], the conditional probabilities p_{j|i} at `perplexity` (finite, > 1).  Slot j of a row is filled iff j <
 * count and index >= 0; d_j = max(0, 2 - 2 s_j) over the filled slots, shifted by the row's minimum; beta by 64 bisection steps on the
 * entropy of p_j ~ exp(-beta d_j), all of them taken; p_out is 0 in an empty slot and a row with fewer than two filled slots is a zero
 * row.  A row's bits depend on that row alone.
 * keep_tsne_repulsion: y fp32 [N,2] (8-byte aligned) -> partials fp32 [n_seg, N, 4] (16-byte aligned), n_seg = ceil(N /
 * KEEP_TSNE_SEGMENT): for row i and segment s the sums over j in the segment, j != i, ascending, of w^2 (y_i - y_j) (words 0 and 1)
 * and of w (word 2), w = rcp(1 + |y_i - y_j|^2) in fp32 with the hardware reciprocal; word 3 is 0.  Every word is written.  THE WORDS
 * DEPEND ON KEEP_TSNE_SEGMENT and on nothing else about the launch or N.
 * keep_tsne_step: the rest of an iteration at y, two launches.  Adds a row's partials in segment order into rz fp32 [N,4] (scratch,
 * 16-byte aligned; every word written) and sums[0] += llrint(Z_i 2^22) per row; then per row the attractive force A = sum val w (y_i -
 * y_j) over its CSR entries (row_ptr int32 [N+1], col int32 [nnz], val fp32 [nnz]; an entry whose column lies outside 0 .. N - 1 is no
 * edge) in stored order and g = 4 (exaggeration A - R / Z), Z = fp32(sums[0] 2^-22); grad_out fp32 [N,2] (may be NULL) takes g.  With
 * update / gains / y_out (fp32 [N,2] each; all three or none; y_out must not be y): gain += 0.2 where g and update differ in sign, x 0.8
 * otherwise, floor 0.01; update = momentum update - lr gain g; y_out = y + update.  stats != 0: sums[1] += llrint(2^40 row sum of val
 * (log val + log Z - log w)) and sums[2] += llrint(2^50 |g_i|^2) per row.  sums: int64 [3], 8-byte aligned, ALWAYS ADDED into: the
 * caller zeroes; integer adds of terms rounded before they are added, so the words do not depend on the order.  0 <= exaggeration <= 32
 * keeps sums[2] inside 63 bits. */
#ifndef KEEP_TSNE_SEGMENT
#define KEEP_TSNE_SEGMENT 2048
#endif
int keep_tsne_segment(void);
int keep_tsne_affinities(keep_handle* h, const int64_t* index, const float* score, const int32_t* count, int64_t N, int k, float perplexity,
                         float* p_out, void* stream);
int keep_tsne_repulsion(keep_handle* h, const float* y, int64_t N, float* partials, void* stream);
int keep_tsne_step(keep_handle* h, const float* y, int64_t N, const float* partials, const int32_t* row_ptr, const int32_t* col,
                   const float* val, int64_t nnz, float exaggeration, float momentum, float lr, int stats, int64_t* sums, float* rz,
                   float* grad_out, float* update, float* gains, float* y_out, void* stream);

/* ---- few-shot prototypes: SimpleShot episodes -------------------------------------
 * Replaces: nothing in the reference; on this engine, per episode, a torch loop of centre, normalise and x @ P.T over the whole test set
 * (E reads of the features, an [N,C] matrix per episode, a summation order the library picks).  2 <= C <= 63 classes, D a multiple of
 * 16 in 16 .. 1024, 1 <= E <= 2^16 episodes per call, 1 <= N, M <= 2^22 rows per call; features are fp32 row-major unit rows, 16-byte
 * aligned, under keep_cluster_assign's skip rule (a row holding a non-finite value or an element with |x| > 1 is skipped).  Anything
 * else is KEEP_EINVAL and nothing is launched.  No host synchronisation.
 *
 * keep_fewshot_sample: the support sets.  class_rows int32 [M'] (the labelled training rows grouped by class) and class_offsets int64
 * [C + 1] (class c is class_rows[class_offsets[c] .. class_offsets[c + 1]), n_c its size, at most 2^22) are the caller's and are
 * trusted.  With the bootstrap's generator (section 24), for GLOBAL episode g = first_episode + e and class c: key = key(seed, 64 g +
 * c), r_j = (mix64(key + j G) n_c) >> 64 for j = 0, 1, 2, ..; the support is the first `shots` DISTINCT values of r_j in order of first
 * appearance, each mapped through class_rows[class_offsets[c] + r].  n_c <= shots: all of the class's rows in stored order.  At most
 * KEEP_FEWSHOT_MAX_DRAWS draws are made (never reached in practice: the slots left are unused).  support_out int32 [E,C,shots], unused
 * slots -1.  Episode g is the same list whatever E, first_episode or the grid.  1 <= shots <= KEEP_FEWSHOT_MAX_SHOTS, 0 <=
 * first_episode <= 2^40.
 * keep_fewshot_prototypes: train fp32 [M,D]; support int32 [E,C,shots] as above, but any 1 <= shots <= 2^22 (a slot outside 0 .. M - 1
 * is unused).  One workgroup per episode walks the slots in (class, slot) order; every sum below is a sequential fp32 sum in that
 * order per column.  A sampled row the skip rule drops is left out and one is ADDED to *support_skipped (int64, may be NULL).  mu = the
 * sum of the kept rows / their number (one fp32 division per column), 0 with centre = 0 or no kept row; per kept row v = s - mu (one
 * fp32 subtraction per element), n = sqrtf(the chain of v_d^2: lane l of a wave adds d = l, l + 64, .. ascending by fmaf from 0, the
 * 64 partial sums are added by the xor butterfly 32, 16, .. 1), z = v / n (a zero row when n = 0); p_c = the sum of class c's z / their
 * number.  bank_out fp32 [E,C + 1,D]: p_0 .. p_{C-1}, then mu; the row of a class without a kept row is zero and valid_out uint8 [E,C]
 * is 0 for it, 1 otherwise.  consts_out fp32 [E,2 C + 1]: mu . p_c (C words), h_c = fp32(0.5 |p_c|^2) (C words), |mu|^2; each dot by
 * the lane chain above.  An episode's words depend on train and that episode's support list alone.
 * keep_fewshot_classify: feats fp32 [N,D]; bank / consts / valid as written above.  For row x and episode e the C + 1 dots x . p_c and
 * x . mu are keep_cluster_assign's k-ordered fma chain from 0 on v_mfma_f32_16x16x4_f32, K never split (dots_out[:, j] is the `best` of
 * keep_cluster_assign against the one-row bank j bit for bit).  Then, each a single fp32 operation in this order: r = sqrtf(max(0,
 * fma(-2, x.mu, 1) + |mu|^2)); t_c = ((x.p_c - mu.p_c) - h_c * r); label = the first valid c with the largest t_c (the nearest
 * prototype of q = (x - mu) / |x - mu|, since t_c / r = q.p_c - h_c); -1 when r = 0, when no class is valid, or for a skipped row.
 * labels_out int32 [N,E] (may be NULL).  truth int32 [N] with confusion int64 [E,C,C] (both or neither): confusion[e, truth, label] is
 * ADDED into for every labelled pair whose truth lies in 0 .. C - 1 (anything else, such as -1, leaves the row out); integer counts,
 * gathered per workgroup and tile in LDS and flushed by one no-return 64-bit atomic per non-zero bin.  E == 1 only (NULL otherwise):
 * scores_out fp32 [N,C] = t_c / r (-inf for an invalid class; a zero row with label -1), margin_out fp32 [N] = (t_best - t_second) / r
 * (0 with fewer than two valid classes or label -1), dots_out fp32 [N,C + 1] the raw dots.  *skipped (int64, may be NULL) is ADDED
 * into once per skipped test row.  At least one of labels_out / confusion / scores_out / margin_out / dots_out.  segments: 0 (chosen
 * here) or 1 .. 1024 cuts of the episodes run by different workgroups (any value gives the same words; for measurement). */
#define KEEP_FEWSHOT_MAX_SHOTS 256
#define KEEP_FEWSHOT_MAX_DRAWS (1 << 20)
int keep_fewshot_sample(keep_handle* h, const int32_t* class_rows, const int64_t* class_offsets, int64_t C, int64_t shots, uint64_t seed,
                        int64_t first_episode, int64_t E, int32_t* support_out, void* stream);
int keep_fewshot_prototypes(keep_handle* h, const float* train, int64_t M, int64_t D, const int32_t* support, int64_t E, int64_t C,
                            int64_t shots, int centre, float* bank_out, float* consts_out, unsigned char* valid_out,
                            int64_t* support_skipped, void* stream);
int keep_fewshot_classify(keep_handle* h, const float* feats, int64_t N, int64_t D, const float* bank, const float* consts,
                          const unsigned char* valid, int64_t E, int64_t C, const int32_t* truth, int64_t* confusion, int32_t* labels_out,
                          float* scores_out, float* margin_out, float* dots_out, int64_t* skipped, int segments, void* stream);

/* Region outlines: the boundary rings of a label image, with holes, and an outline drawn into an image.
 * Replaces: the contour polygons with a hole list per contour that CLAM's segmentTissue hands back (cv2.findContours with
 * RETR_CCOMP; the step of README.md:74) and the polygon annotation a viewer takes a lesion of WSI_evaluation/segment_utils.py's
 * pred_mask as; restated on the pixel mask as rings of pixel-crack edges on the corner lattice, integer arithmetic, exact and unique.
 * labels: int32 [H,W] as keep_regions_label writes it, values 0..n (a value outside 1..n counts as background), n >= 0,
 * 1 <= H W <= 2^28 (an edge slot 4 p + side fits an int32), connectivity 4 or 8.
 * Edges: pixel p = y W + x with label l > 0 has a directed edge on side s iff the pixel across that side lies outside the image or
 * carries a label != l: side 0 top, direction +x, start vertex (x, y); 1 right, +y, (x + 1, y); 2 bottom, -x, (x + 1, y + 1); 3 left,
 * -y, (x, y + 1) (x to the right, y down: the region is on the walker's right).  Slot = 4 p + s.
 * Successor at the end vertex of side s of p, with AR = p moved one step along the direction, AL = AR moved one step across side s,
 * "in" = inside the image with label l:  AR in, AL in: side (s + 3) % 4 of AL;  AR in, AL out: side s of AR;  AR out, AL out: side
 * (s + 1) % 4 of p;  AR out, AL in: side (s + 1) % 4 of p with connectivity 4, side (s + 3) % 4 of AL with connectivity 8 (the
 * ring passes through the diagonal contact and touches itself there).  The cycles of this permutation are the rings.
 * An edge is a corner iff its predecessor lies on another side.  A ring's leader is its corner edge with the smallest slot; its
 * vertices are the start vertices of its corner edges in walking order from the leader; rings are numbered in ascending leader slot.
 * With labels of keep_regions_label and the same connectivity a region's first ring is its one outer ring, every other a hole.
 * keep_outline_count: counts_out int64 [2] ON THE DEVICE: E (edges) and V (corner edges).  Workspace: 8 ceil(H W / 2048) bytes.
 * keep_outline_trace: E, V as read back from keep_outline_count (V = 0 needs no call; 4 <= V <= E, n >= 1).  vertices_out: int32
 * [V,2] (x, y) on 0..W / 0..H, ring after ring, all V rows; rings_out: int64 [ring_cap,8], the first min(R, ring_cap) rows (may be NULL
 * when ring_cap = 0); r_out: R, one int64 ON THE DEVICE.  Ring columns:
 *   0 label    1 start (row of the first vertex)    2 nvert    3 nedge (crack edges: the perimeter in pixel sides)
 *   4 area2    sum of x_i y_{i+1} - x_{i+1} y_i: twice the enclosed area, > 0 for an outer ring, < 0 for a hole
 *   5 lead_x, 6 lead_y  the first vertex                       7 hole   1 iff area2 < 0
 * Workspace: 60 E + 4 H W + 16 ceil(max(H W, E) / 2048) bytes (each part rounded up to 256) + 512.  No host synchronisation; the
 * number of jumping rounds that do work follows the longest ring (2 ceil(log2(its edges))), the others return at once.
 * keep_outline_draw: rgb_in / rgb_out uint8 [H,W,3]; out[p] = color (R | G << 8 | B << 16) iff labels[p] = l > 0 and some q with
 * max(|dx|, |dy|) <= width lies outside the image or has a label != l, else rgb_in[p].  1 <= width <= 16; rgb_out may be rgb_in.
 * Workspace: H W bytes. */
int keep_outline_count(keep_handle* h, const int32_t* labels, int64_t H, int64_t W, int64_t n, int connectivity, int64_t* counts_out,
                       void* stream);
int keep_outline_trace(keep_handle* h, const int32_t* labels, int64_t H, int64_t W, int64_t n, int connectivity, int64_t E, int64_t V,
                       int32_t* vertices_out, int64_t* rings_out, int64_t ring_cap, int64_t* r_out, void* stream);
int keep_outline_draw(keep_handle* h, const int32_t* labels, int64_t H, int64_t W, const unsigned char* rgb_in, unsigned char* rgb_out,
                      int color, int width, void* stream);

/* Polygon annotations to masks: the inverse of the outlines above.
 * Replaces: the raster a viewer makes of a pathologist's polygons (ASAP's conversion of CAMELYON16's annotation XML into the
 * test_040_mask.tif that WSI_evaluation/segment_utils.py reads; a QuPath export painted with an image library), restated as a
 * scan-line fill at pixel centres in integers, exact; and the per-tile label rule of WSI_evaluation/segment_utils.py:99-103.
 * keep_poly_fill: vertices int64 [V,2] level-0 (x, y), ring after ring, rings open (the first point not repeated), x to the right,
 * y down; ring_start int64 [R+1] ascending from 0 to V, ring r owns rows ring_start[r] : ring_start[r+1], at least 3 of them; weight
 * int32 [R] in {-1, 0, +1}; all three ON THE DEVICE, 8 / 8 / 4-byte aligned.  Mask pixel (i, j) covers level-0 [ox + j d, ox + (j+1) d)
 * x [oy + i d, oy + (i+1) d); its centre in doubled units is Cx_j = 2 ox + (2 j + 1) d, Cy_i = 2 oy + (2 i + 1) d.
 * For the edge (xa, ya) -> (xb, yb) of ring r (the last vertex joins the first; skipped if ya == yb): s = +1 if yb < ya else -1,
 * (xl, yl) the endpoint with the smaller y, (xh, yh) the other.  It crosses row i iff 2 yl <= Cy_i < 2 yh: the rows
 * [ceil((2 yl - 2 oy - d) / (2 d)), ceil((2 yh - 2 oy - d) / (2 d))) clipped to [0, H).  In row i, with
 * num = (Cy_i - 2 yl) (xh - xl) + (2 xl - 2 ox - d) (yh - yl) and j0 = clamp(ceil(num / (2 d (yh - yl))), 0, W):
 * delta[i][j0] += s weight[r] (W is a dump column).  wind[i][j] = the sum of delta[i][0..j]; a pixel is inside iff wind > 0
 * (KEEP_FILL_UNION) or wind odd (KEEP_FILL_EVENODD); out[i][j] = value (0..255) if inside, else into[i][j], or 0 when into is NULL.
 * out: uint8 [H,W]; into: uint8 [H,W] or NULL; out may be into.
 * Limits (KEEP_EINVAL before any device work): 1 <= downsample <= 4096; H, W >= 1 and H (W + 1) <= 2^28; |origin| <= 2^26;
 * V <= 2^24; R <= 2^20; V >= 3 R; value in 0..255.  PRECONDITION on the arrays, which are not read on the host: every coordinate
 * within +-2^26 (all products then fit an int64), ring_start and weight as above.  An edge that breaks it (a coordinate beyond the
 * limit, a ring_start that does not enclose the vertex, a ring of < 3 vertices, a weight outside {-1, 0, 1}) adds nothing; no index
 * derived from the arrays leaves the workspace.  R = 0 (then V = 0) writes into, or zeros.
 * C, the number of crossings of edges with rows, is read back once to size the grid: ONE host synchronisation per call (none when
 * R = 0).  C >= 2^31 is KEEP_EINVAL after that read.  crossings_out (a HOST int64, may be NULL) receives C.
 * Workspace from the handle's arena: 4 H (W + 1) bytes of delta, zeroed at the head of the call, + 24 V + 16 ceil(V / 2048) + 8 (each
 * part rounded up to 256).  Integer adds commute: the mask is the same from run to run.
 * keep_mask_tile_counts: mask uint8 [H,W] (non-zero = set), 1 <= H W <= 2^30, pixel geometry as above with 1 <= downsample <= 2^30 and
 * |origin| <= 2^40; coords int64 [N,2] level-0 top-left (x, y) ON THE DEVICE, within +-2^60 (not read on the host), N <= 2^24 - 1;
 * 1 <= patch <= 2^30.  counts_out int32 [N,2]: column 0 the pixels whose centre lies in [x, x + patch) x [y, y + patch) and inside the
 * mask: columns [ceil((2 (x - ox) - d) / (2 d)), ceil((2 (x + patch - ox) - d) / (2 d))) clipped to [0, W], rows likewise; column 1
 * those of them that are non-zero.  At downsample 1 and origin 0, 2 counts[n][1] > patch^2 is the label rule of segment_utils.py:99-103.
 * No workspace, no host synchronisation. */
enum { KEEP_FILL_UNION = 0, KEEP_FILL_EVENODD = 1 };
int keep_poly_fill(keep_handle* h, const int64_t* vertices, int64_t V, const int64_t* ring_start, int64_t R, const int32_t* weight,
                   int64_t downsample, int64_t H, int64_t W, int64_t origin_x, int64_t origin_y, int rule, int value,
                   const unsigned char* into, unsigned char* out, int64_t* crossings_out, void* stream);
int keep_mask_tile_counts(keep_handle* h, const unsigned char* mask, int64_t H, int64_t W, int64_t downsample, int64_t origin_x,
                          int64_t origin_y, const int64_t* coords, int64_t N, int64_t patch, int32_t* counts_out, void* stream);

/* Segmentation evaluation: tile ROC, mask overlap, threshold sweep.
 * keep_eval_roc replaces: the arithmetic of eval_seg_auc (WSI_evaluation/segment_utils.py:105-119): roc_auc_score, roc_curve and
 * thresholds[np.argmax(tpr - fpr)] of scikit-learn over the tiles of a slide.  scores fp32 [N], labels uint8 [N] (non-zero =
 * positive), both ON THE DEVICE, 0 <= N <= 2^24 - 1.  A NaN score removes its tile and -0.0 counts as +0.0, as in keep_sort_f32.
 * scalars_out: int64 [8] ON THE DEVICE:
 *   0 n   the scored tiles      1 P   the positives among them      2 Nn  the negatives
 *   3 U2  the sum over the positives of 2 less + eq, less / eq the negatives below / equal to the positive's score (<= 2^49);
 *         AUC = double(U2) / (2.0 P Nn): the exact area under the ROC curve, ties as the trapezoid takes them, rounded once
 *   4 K   the distinct scores = the points of the curve
 *   5 best_k   the row of the best threshold, or -1 for the point (0, 0) with threshold +inf that roc_curve prepends
 *   6 the best threshold's fp32 bits, zero-extended (0x7F800000 = +inf)      7 the number of kept points
 * The curve, rows 0..K-1 for the distinct scores in DESCENDING order: thresholds_out fp32, fps_out / tps_out int32 (the negatives /
 * positives with score >= threshold), kept_out uint8: 1 for what roc_curve(drop_intermediate=True) keeps: the first and the last
 * point and every point between where the second difference of fps or of tps is not zero.  Each has room for N entries (K <= n <=
 * N; the rows from K on are not written); all four may be NULL together, and the scalars are the same.
 * Best threshold: over the kept points J = double(tps) / double(P) - double(fps) / double(Nn) in IEEE fp64, the first maximum in
 * row order; when no kept point has J > 0 (constant scores, scores worse than chance) the answer is +inf, as np.argmax picks the
 * prepended point.  P = 0 or Nn = 0 (N = 0 included) is reported in the scalars, with best_k = -1, and is no error here.
 * No host synchronisation.  Workspace from the handle's arena: 12 N bytes + the sort's (4 N + its digit tables, none up to 4096
 * values) + 4 ceil(N / 2048) + 16 KiB, and 13 N more when the curve outputs are NULL (each part rounded up to 256).  Integer
 * arithmetic, integer atomics and one order-independent (max J, min row) reduction: the same from run to run.
 * keep_eval_mask_counts replaces: the counting of eval_seg_coarse (segment_utils.py:130-151).  a, b: uint8 [H,W], within: uint8
 * [H,W] or NULL, contiguous, non-zero = set, 1 <= H W <= 2^30.  counts_out: int64 [4] ON THE DEVICE, over the pixels where within
 * is set (all when NULL): set in a, set in b, set in both, considered.  The reference's uint8 product mask_img * pred_mask is
 * non-zero exactly where both are (255 v = -v mod 256), so "set in both" is its count.  No workspace, no host synchronisation.
 * keep_eval_raster_hist: a threshold sweep at pixel level, which the reference does not have (it takes Dice at one threshold).
 * acc: the int64 [H,W] accumulator of keep_heat_accumulate, 8-byte aligned, under the PRECONDITION S <= 65535 c stated at
 * keep_regions_table (a word that breaks it counts in bin 65535); truth: uint8 [H,W]; within: uint8 [H,W] or NULL.  hist_out:
 * int64 [2,65537] ON THE DEVICE, row = truth set: bin m <= 65535 counts the covered pixels (c > 0) whose mean in 16-bit fixed point
 * (2 S + c) / (2 c) is m, bin 65536 the uncovered ones; pixels outside within count nowhere.  No workspace, no host synchronisation. */
int keep_eval_roc(keep_handle* h, const float* scores, const unsigned char* labels, int64_t N, int64_t* scalars_out, float* thresholds_out,
                  int32_t* fps_out, int32_t* tps_out, unsigned char* kept_out, void* stream);
int keep_eval_mask_counts(keep_handle* h, const unsigned char* a, const unsigned char* b, const unsigned char* within, int64_t H, int64_t W,
                          int64_t* counts_out, void* stream);
int keep_eval_raster_hist(keep_handle* h, const int64_t* acc, const unsigned char* truth, const unsigned char* within, int64_t H, int64_t W,
                          int64_t* hist_out, void* stream);

/* Bootstrap resampling: the counts behind a confidence interval, B replicates per call.
 * Replaces: nothing the reference runs (WSI_evaluation/zeroshot_subtyping_WSI.py:24 sets `bootstrapping = 1000` and never uses
 * it); on the host, B calls of scikit-learn on B resampled copies, each with its own sort.
 * The resampling.  All arithmetic modulo 2^64, G = 0x9E3779B97F4A7C15:
 *   mix64(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
 *   key(seed, b) = mix64(seed ^ mix64((b + 1) G))                               b >= 0: the replicate
 *   draw(seed, b, j, n) = (mix64(key(seed, b) + j G) n) >> 64                   the high half of the 128-bit product, j = 0..n-1
 * Replicate b >= 0 of a sample of n items is the multiset { item[draw(seed, b, j, n)] : j = 0..n-1 }; replicate -1 is the sample
 * itself.  A replicate depends on (seed, b, n) alone: not on B, on the split of the replicates over calls, on the launch or on the
 * order of the atomics; two calls with equal seed and n draw the same positions (paired replicates).  The index bias is below
 * n / 2^64.  Row r of `out` holds replicate first_replicate + r; first_replicate >= -1, 0 <= B <= 2^20, 0 <= N <= 2^24 - 1.
 * keep_boot_roc: scores fp32 [N] (4-byte aligned), labels uint8 [N] (non-zero = positive), ON THE DEVICE; NaN and -0.0 as in
 * keep_eval_roc.  The sample is the n scored items in their original order.  out: int64 [B,4] ON THE DEVICE, 8-byte aligned:
 *   0 n (the same in every row)    1 P_b, 2 Nn_b  the drawn positives / negatives
 *   3 U2_b  over the drawn positives the sum of 2 less + eq, less / eq the drawn negatives below / equal to the positive's score,
 *           each with its multiplicity: keep_eval_roc's U2 of the resampled arrays (<= 2 n^2 < 2^49)
 * A replicate with one class only is reported as it is (P_b = 0 or Nn_b = 0).  Row b = -1 equals scalars 0..3 of keep_eval_roc.
 * One sort per call gives every scored item the rank g of its score among the K distinct ones; a replicate is then n x (hash,
 * 4-byte gather, integer add into a histogram of 2 K counters) and one scan over K.  The counters live in LDS up to
 * K = KEEP_BOOT_LDS_GROUPS, above it in one slab of 8 N bytes per resident workgroup.
 * Workspace from the handle's arena: 8 N bytes + the sort's (4 N + its digit tables, none up to 4096 values) + 8 (2048 ceil(N /
 * 2048)) + 8 ceil(N / 2048) + 16 and, for N > KEEP_BOOT_LDS_GROUPS, the slabs: min(B, 2 x the CUs, 256 MiB / 8 N, at least 1) x
 * 8 N bytes (each part rounded up to 256).
 * keep_boot_confusion: truth, pred uint8 [N] ON THE DEVICE, 2 <= C <= 16.  PRECONDITION: every truth[i], pred[i] < C (not read on
 * the host; a larger label counts as C - 1, no index leaves the table).  out: int64 [B,C,C] ON THE DEVICE, 8-byte aligned:
 * out[r][t][p] = the draws of replicate first_replicate + r that landed on an item with truth t and pred p; every row sums to N and
 * row b = -1 is the plain confusion matrix.  Workspace: N bytes.
 * Both: no host synchronisation; integer adds only: the same from run to run.  N = 0 writes zeros; B = 0 writes nothing.
 * KEEP_EINVAL, nothing written: N or B or first_replicate or C outside the ranges above, a null array with N > 0, a null or
 * misaligned out with B > 0. */
enum { KEEP_BOOT_LDS_GROUPS = 8192 };
int keep_boot_roc(keep_handle* h, const float* scores, const unsigned char* labels, int64_t N, uint64_t seed, int64_t first_replicate,
                  int64_t B, int64_t* out, void* stream);
int keep_boot_confusion(keep_handle* h, const unsigned char* truth, const unsigned char* pred, int64_t N, int64_t C, uint64_t seed,
                        int64_t first_replicate, int64_t B, int64_t* out, void* stream);

/* Lesion-level scoring: distance bands, peaks, candidates against lesions.  Beyond the reference, which stops
 * at AUC and Dice (WSI_evaluation/segment_utils.py); the yardsticks are scipy and restatements of the published CAMELYON16 rule.
 * keep_mask_dist2 replaces: rint(scipy.ndimage.distance_transform_edt(mask == 0) ** 2), capped.  mask uint8 [H,W] ON THE DEVICE,
 * contiguous, non-zero = set, 1 <= H W <= 2^30; 1 <= radius R <= 1024.  out uint32 [H,W]: the squared Euclidean distance in pixels from
 * every pixel to the nearest SET pixel (invert != 0: to the nearest ZERO pixel), exact where it is <= R^2 and the sentinel R^2 + 1
 * elsewhere, a mask with no such pixel at all included.  Pixels outside the image do not exist: they are neither set nor zero.  Two
 * passes: g(y, x) = min(rows to such a pixel in column x, R + 1) as uint16 (one thread per column and band of rows, an R-row halo on
 * either side), then min over |dx| <= R of g(y, x + dx)^2 + dx^2 from a row segment of g with its 2 R halo in LDS, one thread per
 * pixel walking outwards until dx^2 reaches its best.  Workspace from the arena: 2 H W bytes.  No host synchronisation.
 * keep_raster_peaks replaces: non-maximum suppression of a heatmap with a rule that does not depend on thread order.  acc: the int64
 * [H,W] accumulator of keep_heat_accumulate, 8-byte aligned, under the PRECONDITION S <= 65535 c stated at keep_regions_table; mask:
 * uint8 [H,W] or NULL; 1 <= H W <= 2^30; 1 <= radius r <= 127; 0 <= min16 <= 65535.  A pixel is ELIGIBLE iff its count c > 0 and the
 * mask, if given, is set there; its value is m = (2 S + c) / (2 c), peak16's rule.  An eligible pixel p with m >= min16 is a PEAK iff
 * no other eligible pixel q of the window |dx|, |dy| <= r has m_q > m_p, or m_q == m_p and a lower row-major index: of a plateau the
 * first pixel wins, and pixels below min16 still suppress.  Computed as a separable maximum (rows, then columns) of the 64-bit key
 * (m + 1) << 32 | (0xFFFFFFFF - index), 0 for ineligible pixels: a peak's key equals its window's maximum.  peaks_out: int64
 * [max_peaks,3] ON THE DEVICE, rows (x, y, m) in ascending row-major order (block counts, a scan and ranks from ballots: no atomic
 * append); *n_out (int64 ON THE DEVICE): the true number of peaks, also when it exceeds max_peaks; the rows beyond the cap are not
 * written (max_peaks = 0: peaks_out may be NULL).  Workspace: 8 H W bytes + 8 ceil(H W / 2048).  No host synchronisation.
 * keep_lesion_hits replaces: the look-up of every detection in the evaluation mask and the per-lesion maximum of the CAMELYON16
 * evaluation (computeITCList / compute_FP_TP_Probs as published).  xy int64 [N,2] level-0 (x, y) within +-2^62, scores fp32 [N],
 * labels int32 [Hm,Wm] (1 <= Hm Wm <= 2^30), ignore uint8 [n_labels] or NULL, all ON THE DEVICE; 0 <= N <= 2^24 - 1; 1 <= downsample
 * <= 2^30; origin within +-2^40; 0 <= n_labels <= 2^20.  Candidate i reads labels[floor((y - origin_y) / d)][floor((x - origin_x) / d)]
 * (floor division also below zero); outside the array, or a value not in 1..n_labels, is background.  hit_out int32 [N]: the label, 0
 * for background, -1 for a NaN score, which takes no part.  lesion_max_out uint32 [n_labels], zeroed at the head of the call: entry
 * l - 1 is the maximum of the bit patterns of s = max(score, +0.0) (-0.0 read as +0.0; the patterns of non-negative floats order as
 * the floats) over the candidates that hit label l; it stays 0 for a label whose ignore byte is set, while hit_out still reports that
 * label, so that the caller does not count the hit as a false positive.  One returnless 32-bit atomicMax per distinct label of a
 * wave: the lanes that share a label reduce first.  Maxima commute: the same from run to run.  No workspace, no host synchronisation. */
int keep_mask_dist2(keep_handle* h, const unsigned char* mask, int64_t H, int64_t W, int radius, int invert, uint32_t* out, void* stream);
int keep_raster_peaks(keep_handle* h, const int64_t* acc, const unsigned char* mask, int64_t H, int64_t W, int radius, int min16,
                      int64_t max_peaks, int64_t* peaks_out, int64_t* n_out, void* stream);
int keep_lesion_hits(keep_handle* h, const int64_t* xy, const float* scores, int64_t N, const int32_t* labels, int64_t Hm, int64_t Wm,
                     int64_t downsample, int64_t origin_x, int64_t origin_y, int64_t n_labels, const unsigned char* ignore, int32_t* hit_out,
                     uint32_t* lesion_max_out, void* stream);

/* Pre-allocate workspace for calls of up to `tiles` tiles and `prompts` x `seq` tokens. */
int keep_reserve(keep_handle* h, int64_t tiles, int64_t prompts, int64_t seq);
int64_t keep_workspace_bytes(keep_handle* h);

/* ---- the hot path -----------------------------------------------------------------------------
 * Replaces: KEEPModel.encode_image  (quick_start/keep_inference.py:54-58)
 *   pixels: [B,3,224,224] NCHW, ImageNet-normalised, dtype per `pix_dtype` (or raw uint8 [B,224,224,3] with
 *   KEEP_PIX_U8_HWC: the /255 and mean/std steps of keep_inference.py:91-92 run on the device); out: fp32 [B,768],
 *   L2-normalised (F.normalize semantics). */
int keep_encode_image(keep_handle* h, const void* pixels, int pix_dtype, int64_t B, float* out, void* stream);

/* Replaces: KEEPModel.encode_image on tiles of any size  (quick_start/keep_inference.py:32-40 builds the ViT with
 *   timm.create_model(..., dynamic_img_size=True): the patch embedding runs on any H, W divisible by 16 and the position
 *   embedding is resampled to the gh x gw = H/16 x W/16 patch grid by timm's resample_abs_pos_embed -- bicubic, antialiased,
 *   the CLS row kept; unchanged at 14 x 14 only).  pixels: [B,3,H,W] NCHW (or uint8 [B,H,W,3] with KEEP_PIX_U8_HWC), one size
 *   per call; out: fp32 [B,768].  KEEP_EINVAL unless H and W are positive multiples of 16.  At 224 x 224 the same computation as
 *   keep_encode_image, bit for bit.  KEEP_PREC_COMP keeps its per-block plan (calibrated on 224 x 224 tiles) for
 *   197 to 1025 tokens per tile, the band its tolerance was measured in, and runs other grids as KEEP_PREC_STRICT (option
 *   "grid_plan": 1 default, 0 every non-224 grid strict, 2 the plan everywhere -- measurements only). */
int keep_encode_image_hw(keep_handle* h, const void* pixels, int pix_dtype, int64_t B, int64_t H, int64_t W, float* out,
                         void* stream);

/* keep_encode_image_hw with the CLS query's attention over the tokens of one block beside the feature: what a
 *   DINO / UNI / HIPT figure shows per head, which the reference can only produce by hooking timm's Attention.forward
 *   (quick_start/keep_inference.py:32-40 builds the tower).  out: fp32 [B,768], exactly what keep_encode_image_hw writes for the
 *   same call made with option "graphs" = 0; attn_out: fp32 [B, heads, gh gw + 1], row (b, h) = softmax_k(q_{b,h,0} . k_{b,h,k} / 8)
 *   of block `block` (0 .. depth - 1, or negative counting from the end), column 0 the CLS -> CLS weight, columns 1.. the patches in
 *   row-major (y, x) order.  The operands are the block's own fp16 q / k planes (hi + lo where the block runs as split products),
 *   products and sums in fp32.  The call runs the ordinary stream path (it is never captured or replayed as a graph) and leaves
 *   the handle's options and graphs as they were.  KEEP_EINVAL: block out of range, a null pointer, H or W not a positive
 *   multiple of 16. */
int keep_encode_image_attn(keep_handle* h, const void* pixels, int pix_dtype, int64_t B, int64_t H, int64_t W, int block, float* out,
                           float* attn_out, void* stream);

/* keep_encode_image_hw with the attention rollout of the tile beside the feature (Abnar & Zuidema 2020): the CLS
 *   token's relevance over the tokens through every block from `start_block` on, which the reference can only produce by hooking all of
 *   timm's Attention.forward calls (quick_start/keep_inference.py:32-40 builds the tower) and multiplying T x T matrices on the host.
 *   With A_l the head mean of block l's softmax(q k^T / 8), all T query rows, and At_l = (1 - residual) A_l + residual I:
 *   rollout_out[b] = row 0 of At_{depth-1} ... At_{start_block}, fp32 [B, gh gw + 1]; every row sums to 1, column 0 is CLS -> CLS, columns
 *   1.. the patches in row-major (y, x) order.  start_block: 0 .. depth - 1, or negative counting from the end (depth - 1 and residual 0:
 *   the head mean of keep_encode_image_attn's last block).  The scores are fp16 MFMA products of the block's own q / k planes (hi + lo
 *   products where the block runs split) with fp32 sums, the matrix products exact fp32.  out: fp32 [B,768], exactly what
 *   keep_encode_image_hw writes with option "graphs" = 0.  scratch: device memory of at least keep_rollout_scratch_bytes(h, B, H, W)
 *   bytes, the caller's (nothing is taken from the handle's arena); the call is never captured or replayed as a graph and leaves options
 *   and graphs as they were.  KEEP_EINVAL: start_block outside [-depth, depth), residual outside [0, 1) or not finite, a null pointer,
 *   H or W not a positive multiple of 16, a scratch that is too small; KEEP_EUNSUPPORTED: more than 272 tokens per tile. */
int keep_rollout_scratch_bytes(keep_handle* h, int64_t B, int64_t H, int64_t W, int64_t* bytes);
int keep_encode_image_rollout(keep_handle* h, const void* pixels, int pix_dtype, int64_t B, int64_t H, int64_t W, int start_block,
                              float residual, float* out, float* rollout_out, void* scratch, int64_t scratch_bytes, void* stream);

/* Replaces: timm.layers.resample_abs_pos_embed(visual.pos_embed, new_size=(gh, gw), old_size=(14, 14), num_prefix_tokens=1)
 *   (the step timm's dynamic_img_size takes per forward, quick_start/keep_inference.py:32-40).  out: fp32 [gh*gw+1, D], the table
 *   keep_encode_image_hw uses for that grid: visual.pos_embed itself at 14 x 14, else the CLS row + the patch rows through
 *   F.interpolate(mode="bicubic", antialias=True, align_corners=False).  Cached per grid inside the handle. */
int keep_vit_pos_embed(keep_handle* h, int gh, int gw, float* out, void* stream);

/* Replaces: KEEPModel.encode_text  (quick_start/keep_inference.py:60-62)
 *   input_ids / token_type_ids / attention_mask: int64 [P,T] (the tokenizer's return_tensors='pt'
 *   layout, keep_inference.py:99); token_type_ids and attention_mask may be NULL (zeros / ones, as
 *   HF BertModel defaults).  out: fp32 [P,768] L2-normalised.  T <= 512 (BertModel's max_position_embeddings) in every precision mode: above 256 keys
 *   the split-product attention of KEEP_PREC_COMP / KEEP_PREC_STRICT runs over two key windows and merges them (the exact softmax over all keys). */
int keep_encode_text(keep_handle* h, const int64_t* input_ids, const int64_t* token_type_ids,
                     const int64_t* attention_mask, int64_t P, int64_t T, float* out, void* stream);

/* The handle's sticky error bits, set by encode calls on `stream` SINCE THE LAST TIME THIS RETURNED NON-ZERO:
 *   bit 0 (1): a token / type id of a keep_encode_text call was out of range (the kernel clamps it; the reference's nn.Embedding
 *              would raise IndexError);
 *   bit 1 (2): an output feature row of keep_encode_image / keep_encode_text was not finite: an activation left the fp16 range
 *              (|x| > 65504 in a qkv / MLP-hidden store -- conversions do not saturate, so the overflow reaches the output as NaN
 *              instead of as plausible garbage; the fp32 reference would not overflow);
 *   bit 2 (4): a component-labelling loop of keep_tissue_mask / keep_regions_label ran into its iteration cap (cannot happen unless the labels were
 *              corrupted: a chain of strictly decreasing pixel indices is shorter than the image); the mask is not valid.
 * Encode calls only ever SET bits; they are cleared here, once the host has seen them, so an error can not be lost between calls.
 * Synchronises `stream`. */
int keep_token_error(keep_handle* h, void* stream);
/* The same without a host synchronisation: enqueues a copy of the (sticky) flag into `host_flag` (pinned host memory owned by the
 * caller, which must stay alive until the stream has passed that point) behind the work already on `stream`.  Does not clear the flag:
 * a caller that reads a 1 calls keep_token_error() to acknowledge it.  This is how the reference's CUDA path reports an out-of-range
 * index too: asynchronously. */
int keep_token_error_async(keep_handle* h, int32_t* host_flag, void* stream);

/* Replaces: `img_feature @ text_feature.T` (keep_inference.py:104), `image_features @ cls`
 * (WSI_evaluation/utils.py:128) and the softmax / top-2 score that follow it in the WSI scripts.
 *   img fp32 [N,D], txt fp32 [P,D] (row-major; a reference classifier [D,C] is passed transposed). */
int keep_similarity(keep_handle* h, const float* img, const float* txt, int64_t N, int64_t P, int64_t D,
                    float scale, int mode, void* out, int32_t* argmax_out, void* stream);

/* Replaces: `img_feature = model.encode_image(img_input)` + `img_feature @ text_feature.T` + the row argmax taken from it
 * (quick_start/keep_inference.py:101,104; BASELINE config 3) when the LABELS must be the fp32 reference's.
 *   The default precision keeps every cosine within 1e-4 of the fp32 reference, which cannot decide a tile whose two best prompts are
 *   closer than that.  keep_classify encodes all B tiles in the handle's precision, takes sim = scale * feats @ txt^T and its row argmax,
 *   then re-encodes ONLY the tiles whose top-2 margin (in cosine units, i.e. / scale) is below `margin` in KEEP_PREC_STRICT (split
 *   products, ~5e-7) and takes those rows again.  margin < 0: the handle's "label_margin" option (default 2.5e-4 = 2 x tolerance + 25 %);
 *   margin == 0: no second look.  One host synchronisation of `stream` (the number of flagged tiles).
 *   The labels are those of the split-product arithmetic provided the first pass is within margin / 2 of it: true in KEEP_PREC_COMP (<= 1e-4 against
 *   2.5e-4); in KEEP_PREC_FP16 (~2e-4) pass a margin of at least twice that mode's error.
 *   pixels / pix_dtype / B as keep_encode_image (16-byte aligned); txt fp32 [P,D] L2-normalised text features (keep_encode_text);
 *   feats_out fp32 [B,D] or NULL; sim_out fp32 [B,P] or NULL; labels_out int32 [B] (first maximum wins, as torch.argmax);
 *   n_rechecked (HOST pointer or NULL): how many tiles were encoded twice. */
int keep_classify(keep_handle* h, const void* pixels, int pix_dtype, int64_t B, const float* txt, int64_t P, float scale, float margin,
                  float* feats_out, float* sim_out, int32_t* labels_out, int64_t* n_rechecked, void* stream);

/* ---- slide-level zero-shot steps ---------------------------------
 * Replaces the loop of `zero_shot_prompt_select` (WSI_evaluation/utils.py:127-130: one GEMM + one
 * rank_cls_score + one .item() sync per prompt classifier).  feats fp32 [N,D] already L2-normalised
 * (utils.py:125), bank fp32 [K*C, D] = the K classifiers stacked, classifier k occupying rows k*C..k*C+C-1
 * (i.e. each [D,C] classifier transposed); scores_out fp32 [K] (device) = rank_cls_score of every k. */
int keep_prompt_scores(keep_handle* h, const float* feats, const float* bank, int64_t N, int64_t K, int64_t C,
                       int64_t D, float* scores_out, void* stream);

/* ---- tile-level zero-shot evaluation ------------------------------------------
 * Replaces the 50-round loop of training/path_training/zero_shot.py:124-136 (per round: one numpy GEMM
 * `image_embeddings.dot(each_round.T)` + a Python argmax per tile).  feats fp32 [N,D] L2-normalised (zero_shot.py:
 * 121-122), bank fp32 [K*C, D]: round k's C normalised class embeddings in rows k*C..k*C+C-1.
 * labels_out int32 [N,K] (device): argmax class of tile n in round k, first maximum wins (numpy.argmax). */
int keep_group_argmax(keep_handle* h, const float* feats, const float* bank, int64_t N, int64_t K, int64_t C,
                      int64_t D, int32_t* labels_out, void* stream);

/* Replaces the retrieval loop of zero_shot.py:168-171 + retrieval_metrics (zeroshot_metrics.py:6-17).
 * txt fp32 [P,D], img fp32 [N,D], both L2-normalised; target int32 [P] = the image each text must retrieve
 * (NULL: text t -> image t, as the reference).  rank_out int32 [P] (device) = position of the target in the
 * descending score list (0 = best; equal scores: higher index first); p@k = mean(rank < k). */
int keep_retrieval_rank(keep_handle* h, const float* txt, const float* img, int64_t P, int64_t N, int64_t D,
                        const int32_t* target, int32_t* rank_out, void* stream);

/* Replaces `refine_seg` (subtyping_utils.py:38-65, detection_utils.py:39-74, segment_utils.py:63-89).
 * probs fp32 [N,C] (softmax(10*cos)), coords int64 [N,2].  out_mean fp32 [N,C]: for the first tile of
 * every distinct coordinate, the float32 mean of the existing tiles among (x-p,y-p),(x,y-p),(x-p,y),(x,y)
 * (or its own row when overlap == 0); is_first int32 [N]: 1 for those tiles, 0 for later duplicates. */
int keep_refine(keep_handle* h, const float* probs, const int64_t* coords, int64_t N, int64_t C, int64_t patch,
                int overlap, float* out_mean, int32_t* is_first, void* stream);

/* ---- profiling (HIP events on the launch stream) ----------------------------------------------
 * tag names: "vit.im2col" "vit.patch" "vit.ln" "vit.qkv" "vit.attn" "vit.proj" "vit.fc1" "vit.fc2"
 * "vit.head" "text.embed" "text.ln" "text.qkv" "text.attn" "text.out" "text.ffn1" "text.ffn2"
 * "text.pool" "sim", and -- so that each plain image-tower tag times ONE kernel instantiation -- "vit.qkv.x" "vit.attn.x" "vit.proj.x"
 * "vit.fc1.x" "vit.fc2.x" (the launches that carry extra passes: split / compensated products of the blocks the precision setting
 * names) and "vit.tail" (the CLS-rows-only operators of the last block).  keep_profile_enable(h, NULL) times every tag, a name (or
 * several separated by commas) times only those, "" disables.  keep_profile_read synchronises the recorded events and returns the accumulated
 * milliseconds, launch count and (for GEMM tags) executed FLOPs 2*M*N*K for `tag` since the last
 * keep_profile_reset.  Lanes on different internal streams overlap, so per-tag times can sum to more than
 * the wall time. */
int keep_profile_enable(keep_handle* h, const char* tag_or_null);
int keep_profile_read(keep_handle* h, const char* tag, double* total_ms, int64_t* launches, double* flops);
int keep_profile_reset(keep_handle* h);

/* ---- single-operator entry points (used by the parity tests; fp32 in/out on device) -----------
 * keep_op_linear: out = epilogue(A[M,K] @ W[N,K]^T + bias) through the fp16 MFMA GEMM.
 *   epi 0: out[M,N] = acc+bias            1: gelu(acc+bias)
 *       2: out = resid + ls*(acc+bias)    4: out = resid + acc + bias      (resid, ls fp32)
 *   split 1 runs the 3-pass hi/lo product, split 2 the compensated product (fp16 pass + MX-fp4 correction terms;
 *   N % 256 == 0, K % 128 == 0, K >= 256, epi 0..2), split 3 the compensated product with the W_lo A_hi term only (K >= 512).  Outputs of epi 0/1 are the fp16-rounded values (hi, or hi+lo when
 *   split != 0) converted back to fp32. */
int keep_op_linear(keep_handle* h, const float* a, const float* w, const float* bias, const float* ls,
                   const float* resid, int64_t M, int64_t N, int64_t K, int epi, int split, float* out,
                   void* stream);
/* keep_op_linear for the residual epilogues (epi 2 or 4 only) with the LayerNorm that follows offered to the GEMM, as the towers do (the small-M and the
 *   K-sliced split-K paths take it in their reduce kernel; when the GEMM does not, the stand-alone LayerNorm kernel runs on the same parameters).
 *   epi 2 (ViT): out = resid + ls*(acc+bias), ln_out = LayerNorm(out).   epi 4 (BERT, the normalised row replaces the sum): out = ln_out in fp32.
 *   ln_out fp32 [M,N]: the fp16 operand planes the kernel wrote in blk layout, read back (hi + lo when split == 1, hi alone when 0); ln_hi fp32 [M,N] or
 *   NULL: the hi plane alone (a sum cannot tell a swapped pair of planes from a right one).  *did_ln (host): 1 when the GEMM's reduce did the LayerNorm.
 *   N in {768, 1024}; split 0 / 1. */
int keep_op_linear_ln(keep_handle* h, const float* a, const float* w, const float* bias, const float* ls,
                      const float* resid, const float* ln_gamma, const float* ln_beta, float ln_eps, int64_t M, int64_t N,
                      int64_t K, int epi, int split, float* out, float* ln_out, float* ln_hi, int* did_ln, void* stream);
/* One MLP half of a ViT block through the tower's own kernels (timm Block: x + ls2 * fc2(gelu(fc1(norm2(x))))):
 *   LayerNorm (writes the fp16 operand and, per mode, its lo plane / MX-fp4 side planes) -> fc1 + GELU -> fc2 + LayerScale + residual.
 *   mode = KEEP_MLP_* 0..3: 0 plain fp16 | 1 split | 2 compensated | 3 compensated, W_lo term only.  x, out fp32 [M, D]; D in {768, 1024}; F % 256 == 0. */
int keep_op_mlp(keep_handle* h, const float* x, const float* ln_w, const float* ln_b, const float* fc1_w, const float* fc1_b,
                const float* fc2_w, const float* fc2_b, const float* ls, int64_t M, int64_t D, int64_t F, int mode, float* out,
                void* stream);
/* One producer of the MX-fp4 side planes (the operands of the compensated product's correction terms) run on its own, and what it wrote read back:
 *   KEEP_MX_BLOCKIFY   the weight / op-input conversion on x fp32 [M,K] (K % 32 == 0; always both planes: hi_only = 0)
 *   KEEP_MX_LAYERNORM  LayerNorm(x [M,K]; gamma, beta [K], eps) with the side planes of its output; K in {768, 1024}
 *   KEEP_MX_GELU       the compensated 256x256 GEMM gelu(x [M,K] @ w [N,K]^T + bias [N]) with the side planes of its output [M,N]
 *                      (N % 256 == 0, K % 128 == 0, K >= 256; the one-term launch K >= 512)
 *   hi_only 0: both planes, as a two-term consumer needs them; 1: Q(X_hi) and its scales only, as the producers of a one-term chain write them
 *   (the GEMM then is a one-term launch itself); lo must then be NULL.
 * With C = K (N for KEEP_MX_GELU) the width of the operand written: hi, lo fp32 [M,C] row-major, the fp16 planes converted back; q uint8
 * [ceil(M/256)*256 * C] and sc uint8 [ceil(M/256)*256 * C/32 * 2]: the e2m1 bytes and the E8M0 scale bytes exactly as they lie on the device
 * (both planes, padding rows included).  Every byte of q and sc is set to `sentinel` (0..255) before the producer runs: what still holds it was
 * not written.  All pointers but h are device pointers. */
enum { KEEP_MX_BLOCKIFY = 0, KEEP_MX_LAYERNORM = 1, KEEP_MX_GELU = 2 };
int keep_op_mx_planes(keep_handle* h, int producer, int hi_only, const float* x, const float* w, const float* bias,
                      const float* gamma, const float* beta, float eps, int64_t M, int64_t N, int64_t K, int sentinel,
                      float* hi, float* lo, unsigned char* q, unsigned char* sc, void* stream);
/* qkv fp32 [B*T, 3*heads*64] (q|k|v), mask int64 [B,T] or NULL -> out fp32 [B*T, heads*64] */
int keep_op_attention(keep_handle* h, const float* qkv, const int64_t* mask, int64_t B, int64_t T, int heads,
                      int split, float* out, void* stream);
/* keep_op_attention without a mask, with the CLS features of the image tower: q_rows > 0 computes only the first q_rows queries of every sequence
 * (the CLS-only last block; other rows 0); cls_out fp32 [B, heads*64] or NULL: query row 0 of every sequence once more from the fp32 accumulators as
 * hi + lo (the compact operand of KEEP_ATTN_PROJ_CLS), single pass only -- with split != 0 the launcher refuses it: KEEP_EUNSUPPORTED. */
int keep_op_attention_cls(keep_handle* h, const float* qkv, int64_t B, int64_t T, int heads, int split, int q_rows,
                          float* out, float* cls_out, void* stream);
/* The image tower's attention beyond 512 tokens (timm Attention.forward, scaled_dot_product_attention without a mask, at the
 * sequence lengths of quick_start/keep_inference.py:32-40 with dynamic_img_size): key-blocked online softmax, any T >= 1.
 * qkv fp32 [B*T, 3*heads*64] -> out fp32 [B*T, heads*64]; q_rows > 0: only the first q_rows queries of every sequence (other rows 0) */
int keep_op_attention_long(keep_handle* h, const float* qkv, int64_t B, int64_t T, int heads, int split, int q_rows,
                           float* out, void* stream);
/* The CLS query's attention probabilities (the kernel behind keep_encode_image_attn): qkv fp32 [B*T, 3*heads*64], turned into fp16 planes as
 * keep_op_attention does (split != 0: hi + lo) -> out fp32 [B, heads, T] = softmax_k(q_{b,h,0} . k_{b,h,k} / 8), any T >= 1 */
int keep_op_attention_cls_probs(keep_handle* h, const float* qkv, int64_t B, int64_t T, int heads, int split, float* out, void* stream);
/* One block's step of the attention rollout (the kernels behind keep_encode_image_rollout): qkv as above; with A the head mean of
 * softmax(q k^T / 8) over all T query rows and At = (1 - residual) A + residual I, r_out = At r_in in fp32, or At itself when r_in is NULL.
 * r_in, r_out: fp32 [B, T, T]; q_rows = 1: only the CLS row, r_out [B, T] (q_rows = 0: every row).  1 <= T <= 272, else KEEP_EUNSUPPORTED */
int keep_op_attention_rollout_step(keep_handle* h, const float* qkv, int64_t B, int64_t T, int heads, int split, float residual,
                                   const float* r_in, int q_rows, float* r_out, void* stream);
int keep_op_layernorm(keep_handle* h, const float* x, const float* add, const float* gamma, const float* beta,
                      int64_t rows, int64_t D, float eps, float* out, void* stream);
/* out[M,N] = act(scale * A[M,K] @ B[N,K]^T + bias); act 0 none, 1 gelu, 2 tanh (exact fp32 MFMA) */
int keep_op_sgemm(keep_handle* h, const float* a, const float* b, const float* bias, int64_t M, int64_t N,
                  int64_t K, float scale, int act, float* out, void* stream);
int keep_op_l2norm(keep_handle* h, float* x, int64_t rows, int64_t D, void* stream);
/* The image tower in front of its first block (timm PatchEmbed + cls_token + pos_embed), as the engine runs it: im2col of the pixels into
 *   the fp16 operand planes (and the CLS rows cls + pos[0] of the token stream), then the patch-embedding GEMM with the EPI_PATCH epilogue, which writes
 *   patch p of image b to row b*(gh*gw+1)+1+p and adds pos[1+p]; the split-K scratch is attached, so the handle's options pick the GEMM route as they do
 *   in the towers.  pixels: pix_dtype 0 fp32 / 1 fp16 / 2 bf16 [B,3,16 gh,16 gw], 3 uint8 [B,16 gh,16 gw,3] (normalised on the fly); w fp32 [D,768]
 *   (the conv weight flattened), bias, cls fp32 [D], pos fp32 [gh*gw+1, D]; D % 128 == 0.  split 1: hi + lo planes and the 3-pass product; 0: the hi
 *   plane and one pass.
 *   resid fp32 [B*(gh*gw+1), D]: every byte is set to 0xFF (a NaN) before the launches, so a row nobody wrote shows up.  pat_hi, pat_lo fp32
 *   [B*gh*gw, 768]: the two im2col planes read back SEPARATELY (fp16 values, exact in fp32); pat_lo may be NULL.  Every byte of the lo plane is set to
 *   `sentinel` (0..255) before im2col runs, and with split 0 im2col is not given the plane (as in the engine): it then reads back as the sentinel. */
int keep_op_patch_embed(keep_handle* h, const void* pixels, int pix_dtype, int64_t B, int64_t gh, int64_t gw, int64_t D, const float* w,
                        const float* bias, const float* cls, const float* pos, int split, int sentinel, float* resid, float* pat_hi,
                        float* pat_lo, void* stream);
/* The text tower in front of its first layer (HF BertEmbeddings: LayerNorm((word + token_type) + position)): ids, type_ids int64 [P,T]
 *   (type_ids NULL: all 0), wemb fp32 [vocab,H], pemb fp32 [max_pos,H] (T <= max_pos), temb fp32 [type_vocab,H], gamma, beta fp32 [H]; H in {256, 768, 1024}.
 *   resid fp32 [P*T, H]: the fp32 output; hi, lo fp32 [P*T, H]: the fp16 operand planes the kernel wrote in blk layout, read back separately (lo NULL: the
 *   kernel is not given a lo plane).  *err_word (host): an error word of this call, zeroed before the launch -- bit 0: an id or type outside its table
 *   (clamped into it); the handle's sticky error word is not touched. */
int keep_op_bert_embed(keep_handle* h, const int64_t* ids, const int64_t* type_ids, const float* wemb, const float* pemb, const float* temb,
                       const float* gamma, const float* beta, float eps, int64_t P, int64_t T, int64_t H, int64_t vocab, int64_t type_vocab,
                       int64_t max_pos, float* resid, float* hi, float* lo, int* err_word, void* stream);
/* keep_op_layernorm on rows that lie x_stride elements apart (x_stride >= D, a multiple of 4), as the image tower's final norm reads row 0 of every
 *   tile out of the token stream: out fp32 [rows, D] dense = LayerNorm(x[r * x_stride .. + D]) */
int keep_op_layernorm_rows(keep_handle* h, const float* x, int64_t x_stride, const float* gamma, const float* beta, int64_t rows, int64_t D,
                           float eps, float* out, void* stream);
/* keep_op_sgemm with explicit leading dimensions, as the BERT pooler reads row p*T of the token stream: row m of A at a + m*lda, row n of B at
 *   b + n*ldb, row m of the output at out + m*ldo (lda, ldb >= K; ldo >= N; columns N..ldo of the output are not written).  lda % 4 != 0 or
 *   ldb % 4 != 0: KEEP_EUNSUPPORTED. */
int keep_op_sgemm_ld(keep_handle* h, const float* a, int64_t lda, const float* b, int64_t ldb, const float* bias, int64_t M, int64_t N, int64_t K,
                     float scale, int act, float* out, int64_t ldo, void* stream);
/* The kernels that move the CLS rows between the token stream (row stride `row_stride` rows: the tokens per tile) and the compact [rows, D] operands:
 *   KEEP_ROWS_GATHER_F32   dst fp32 [rows, D]: row r <- row r*row_stride of src fp32 [rows*row_stride, D]
 *   KEEP_ROWS_SCATTER_F32  row r*row_stride of dst fp32 [rows*row_stride, D] <- row r of src fp32 [rows, D]; the other rows of dst are the caller's
 *   KEEP_ROWS_GATHER_BLK   src fp32 [rows*row_stride, D] is written as an fp16 plane in blk layout (D % 32 == 0), its rows r*row_stride are gathered into a
 *                          compact blk plane, and that plane comes back as dst fp32 [rows, D] (fp16 values) */
enum { KEEP_ROWS_GATHER_F32 = 0, KEEP_ROWS_SCATTER_F32 = 1, KEEP_ROWS_GATHER_BLK = 2 };
int keep_op_rows(keep_handle* h, int kind, const float* src, int64_t row_stride, int64_t rows, int64_t D, float* dst, void* stream);
/* The two kernels of the mean-input bias compensation (keep_calibrate_bias), one per call; K % 32 == 0:
 *   KEEP_BIAS_COL_SUM    x fp32 [rows, K] is written as an fp16 hi plane in blk layout and its column sums are ADDED into col_sum fp32 [K] (the caller zeroes
 *                        it; a second call continues the sum).  inv_rows, bias and out are not used.
 *   KEEP_BIAS_MEAN_CORR  x is a GEMM weight fp32 [rows = N, K]: out[n] = bias[n] + inv_rows * sum_k w_lo[n][k] col_sum[k] on the lo plane of its blk-layout
 *                        hi / lo split; col_sum fp32 [K] is read only; bias, out fp32 [N] */
enum { KEEP_BIAS_COL_SUM = 0, KEEP_BIAS_MEAN_CORR = 1 };
int keep_op_bias_corr(keep_handle* h, int step, const float* x, int64_t rows, int64_t K, float* col_sum, float inv_rows, const float* bias,
                      float* out, void* stream);
/* measurement aid: one wavefront spins for ~spin_us microseconds and writes {shader-clock cycles, 100 MHz reference ticks} to device_out2
 * (two int64 on the device): effective shader clock = cycles / ticks * 100 MHz.  Launched on a side stream next to a running workload it
 * reads the clock the part actually sustains under that load (bench.py records it; the MFMA peak is quoted at 2.4 GHz). */
int keep_clock_probe(keep_handle* h, int spin_us, long long* device_out2, void* stream);
/* measurement aid: what the matrix pipes alone deliver on this part with the caller's operand values.  One 8-wave workgroup per CU; every wave loads
 * 6 fp16 fragments (6 x 16 B per lane: operands_f16 holds CUs x 512 x 48 fp16 values) and issues `iters` x 8 independent v_mfma_f32_32x32x16_f16 with no
 * memory access in the loop; sink (fp32, CUs x 512) receives one value per lane.  *flops_out (host) = the FLOPs of the launch; time it with events on
 * `stream`.  With N(0, 1)-like operands the socket's power cap holds the pipes at ≈1.6 GHz: ≈1 590 TFLOP/s = 0.63 of the nominal dense peak that the roofline
 * fractions are quoted against; with zeros 2 480 (profiles/r04_mfma_power_ceiling.txt).  bench.py reports it as context next to `roofline`. */
int keep_mfma_probe(keep_handle* h, const void* operands_f16, float* sink, int iters, double* flops_out, void* stream);
/* diagnostics: with option "gemm_dbg"=1 every GEMM launch records, per workgroup, four shader-clock
 * stamps [start, first K tile landed, main loop end, end]; this copies them to host memory. */
int keep_debug_read(keep_handle* h, void* host_dst, int64_t bytes);
/* test hook: fills the handle's scratch memory -- the whole workspace arena (keep_workspace_bytes) and keep_classify's buffer -- with the 32-bit `word`
 * on `stream`, and writes the number of bytes filled to *bytes_out (0, and still KEEP_OK, on a handle that has carved nothing yet).  It allocates and
 * frees nothing.  No entry point may read a workspace byte it has not written in the same call, so a result must not depend on `word`
 * (tests/test_workspace_poison_gpu.py); production code has no use for it. */
int keep_debug_fill_workspace(keep_handle* h, uint32_t word, int64_t* bytes_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KEEP_HIP_H */
