// The image tower's precision plan and what it means for one block of one lane.  No HIP in here: PrecisionPlan is the plan state the handle
// (handle.h) derives from, resolve_block turns it into the steps vit_layer (engine.hip) issues, and tests/block_plan_dump.cpp enumerates the
// resolver on the CPU.
#pragma once
#include "../../include/keep_hip.h"

enum Tag {
    T_VIT_IM2COL, T_VIT_PATCH, T_VIT_LN, T_VIT_QKV, T_VIT_ATTN, T_VIT_PROJ, T_VIT_FC1, T_VIT_FC2, T_VIT_HEAD,
    T_TXT_EMBED, T_TXT_LN, T_TXT_QKV, T_TXT_ATTN, T_TXT_OUT, T_TXT_FFN1, T_TXT_FFN2, T_TXT_POOL, T_SIM,
    // image-tower launches that are NOT the plain single-pass kernel of their operator: split products / compensated (MX-fp4) products of the
    // blocks the precision setting names ("x" = extra passes), and the CLS-rows-only operators of the last block ("tail": small-M kernels).
    // The plain tags above then time one kernel instantiation each (bench.py's roofline block needs a per-kernel figure).
    T_VIT_QKV_X, T_VIT_ATTN_X, T_VIT_PROJ_X, T_VIT_FC1_X, T_VIT_FC2_X, T_VIT_TAIL, T_COUNT
};

struct PrecisionPlan {
    int precision = KEEP_PREC_COMP;
    int strict_blocks = 0;       // first n blocks / layers as full hi/lo split products (any mode)
    // The prefix shorthands (state of the last keep_set_option; they only take effect once one of them is set -- see plan_default below)
    int comp_full_blocks = 1;    // KEEP_PREC_COMP: first n ViT blocks run qkv / attention / proj as split products as well
    int comp_mlp_blocks = 8;     // KEEP_PREC_COMP: first n ViT blocks run fc1 / fc2 as compensated (fp16 + MX-fp4) products
    int comp_min_tiles = 32;     // lanes with fewer tiles take the split product where a compensated one is asked for (small-M kernels)
    int comp_qkv = 0;            // 1: KEEP_PREC_COMP, blocks < comp_full_blocks: the qkv GEMM as a compensated product (x1.5) instead of a split one (x3);
                                 // q / k / v still stored as hi + lo planes, attention still a split product.  Measured (round 3): +0.9 % at equal settings,
                                 // but block 0's qkv is where the error budget is tightest (the 3 % of the rounding variance the fp4 terms leave is
                                 // amplified by all 24 blocks): calibrate() then needs 10 compensated MLP blocks instead of 6 -- a net loss.  Off.
    int comp_qkv_from = 1 << 20; // the same for the split-attention blocks with index >= this only (block 0 keeps its three-pass qkv)
    int cls_tail = 1;            // last ViT block: proj / MLP on the CLS rows only (exact; 0 = evaluate every token)
    int vit_depth = 0;           // filled at finalize
    bool vit_has_q = false;      // every fc1 / fc2 weight has its fp4 side planes (dims % 128 == 0)
    // The per-block plan of KEEP_PREC_COMP (keep_set_block_precision; the four comp_* options above are prefix shorthands that rewrite it):
    //   attn_mode[i]  attention side of block i: KEEP_ATTN_PLAIN | KEEP_ATTN_SPLIT (qkv, q/k/v storage, attention, proj as split products) |
    //                 KEEP_ATTN_SPLIT_COMPQKV (the same with the qkv GEMM as a compensated product) | KEEP_ATTN_COMPQKV (compensated qkv only) |
    //                 KEEP_ATTN_PROJ_CLS (plain for every row + the CLS rows' proj again as a split product on their fp32-grade attention output) |
    //                 KEEP_ATTN_COMPQKV_PROJ_CLS (both of the last two)
    //   mlp_mode[i]   fc1 / fc2 of block i: KEEP_MLP_PLAIN | KEEP_MLP_SPLIT | KEEP_MLP_COMP (both MX-fp4 correction terms) | KEEP_MLP_COMP_W (the W_lo term only) |
    //                 KEEP_MLP_CLS (plain for every row + the CLS rows again as split products)
    // Which block gets what is a measured, per-checkpoint decision (tools/precision_budget.py, KEEPModel.calibrate).
    static constexpr int MAX_BLOCKS = 64;
    unsigned char attn_mode[MAX_BLOCKS] = {}, mlp_mode[MAX_BLOCKS] = {};
    bool plan_custom = false;    // keep_set_block_precision was called since the last prefix option
    void plan_from_prefix() {
        for (int i = 0; i < MAX_BLOCKS; ++i) {
            attn_mode[i] = i < comp_full_blocks ? ((comp_qkv || i >= comp_qkv_from) ? KEEP_ATTN_SPLIT_COMPQKV : KEEP_ATTN_SPLIT) : KEEP_ATTN_PLAIN;
            mlp_mode[i] = i < comp_mlp_blocks ? KEEP_MLP_COMP : KEEP_MLP_PLAIN;
        }
        plan_custom = false;
    }
    // The plan a handle starts with (no calibration has seen the weights yet): block 0's attention side as split products with a compensated qkv
    // and its MLP compensated -- the first block's rounding errors, in EVERY row, are amplified by all the attention layers that follow: 45-48 % of the
    // all-fp16 error variance on the synthetic checkpoints --, every other block plain with the CLS rows' MLP redone as split products (the pooled
    // feature is a CLS row).  profiles/r05_precision_budget.md: cosine rms 8.5e-6 on the bench weights, a quarter of what the 1e-4 tolerance allows a
    // 100 000-tile slide, 3 % slower than what KEEPModel.calibrate picks for them.
    void plan_default() {
        for (int i = 0; i < MAX_BLOCKS; ++i) { attn_mode[i] = KEEP_ATTN_PLAIN; mlp_mode[i] = KEEP_MLP_CLS; }
        attn_mode[0] = KEEP_ATTN_SPLIT_COMPQKV; mlp_mode[0] = KEEP_MLP_COMP;
        plan_custom = false;
    }
    PrecisionPlan() { plan_default(); }
    // the text tower is 1 % of a slide's work: in the compensated mode it simply runs split products throughout, at every length BertModel accepts
    // (T <= 512 = max_position_embeddings; above 256 keys the split attention runs as two key windows of <= 256, merged like an online softmax)
    bool txt_split(int l, int T) const { (void)T; return precision == KEEP_PREC_STRICT || l < strict_blocks || precision == KEEP_PREC_COMP; }
    bool any_split() const { return precision != KEEP_PREC_FP16 || strict_blocks > 0; }
    bool any_comp() const {
        if (precision != KEEP_PREC_COMP || !vit_has_q) return false;
        for (int i = 0; i < MAX_BLOCKS && i < (vit_depth ? vit_depth : MAX_BLOCKS); ++i)
            if (mlp_mode[i] == KEEP_MLP_COMP || mlp_mode[i] == KEEP_MLP_COMP_W || attn_mode[i] == KEEP_ATTN_SPLIT_COMPQKV || attn_mode[i] == KEEP_ATTN_COMPQKV || attn_mode[i] == KEEP_ATTN_COMPQKV_PROJ_CLS) return true;
        return false;
    }
};

// One GEMM site of a block (qkv, proj, fc1, fc2) as its all-rows launch runs
struct SiteStep {
    bool split;             // three fp16 passes on hi + lo operands
    int comp;               // GemmParams.comp: 0 | 1 fp16 pass + the W_lo MX-fp4 term | 2 fp16 pass + both MX-fp4 terms
    bool corrected_bias;    // a PLAIN launch (neither of the above): takes the bias with W_lo a_mean folded in (mean-input compensation), where one is calibrated
    int tag;                // profile tag of the launch
};
// What a LayerNorm writes beside the hi plane of its output
struct LnStep {
    bool lo;                // the lo plane: a split product reads it
    bool fp4;               // the MX-fp4 planes: a compensated product reads them
    bool fp4_hi_only;       // ... of Q(x_hi) only (KEEP_MLP_COMP_W)
};
// Everything vit_layer needs to know to issue block i of one lane
struct BlockSteps {
    // Last block: everything after the attention is per-token and only the CLS token is pooled (global_pool='token'), so its queries / proj / MLP
    // are evaluated for the B CLS rows only.  Exact (same arithmetic on the rows that matter); the skipped FLOPs still count as algorithmic work.
    bool cls_only;
    bool attn_split;        // q / k / v and the attention output stored hi + lo, attention and proj as split products
    // qkv of a block in the compensated mode: fp16 pass + MX-fp4 correction terms instead of three fp16 passes (lanes large enough for the 256x256
    // kernel; LayerNorm-1 then writes the fp4 planes of its output instead of the lo plane).
    // KNOWN DEFECT, kept as it is (a fix changes features): false whenever the previous block's fc2 already wrote this block's LayerNorm-1 output
    // (xn_ready: its fused LayerNorm writes no fp4 planes).  KEEP_ATTN_COMPQKV / KEEP_ATTN_COMPQKV_PROJ_CLS on a large lane then runs a PLAIN qkv with
    // the corrected bias, although attn_split above was decided as if the qkv were compensated.  Reached only with grid_plan = 2 on small grids.
    bool qkv_comp;
    bool cls_proj;          // KEEP_ATTN_PROJ_CLS: every row plain; the attention kernel also writes the CLS rows' output hi + lo (compact), and their proj runs again as a split product
    bool cls_mlp;           // KEEP_MLP_CLS: every row plain, then the CLS rows again as split products on the compact rows
    SiteStep qkv, proj, fc1, fc2;
    int attn_tag;
    LnStep ln1, ln2;        // (ln1: of the LayerNorm-1 this block launches itself, i.e. unless xn_ready)
    // The plain proj is offered LayerNorm-2 (the fused LayerNorm of the small-M path does not write fp4 planes).
    // KNOWN DEFECT, kept as it is (a fix changes features): also with cls_proj && !cls_mlp.  Where proj takes the offer, the CLS rows'
    // LayerNorm-2 output is computed from the plain proj's rows BEFORE scatter_after_proj replaces them with the split result: the MLP input of
    // those rows keeps the rounding error KEEP_ATTN_PROJ_CLS is there to remove.
    bool ln2_to_proj;
    bool next_ln1_to_fc2;   // fc2 is offered the next block's LayerNorm-1: it reads exactly the rows written there (not when CLS rows are still to be replaced)
    bool next_ln1_lo;       // ... which then writes the lo plane (the next block's attention side is split)
    bool gather_before_proj;    // the CLS rows' residual as it enters proj -> compact rows (the plain proj updates these rows too; the split result replaces that); not when live
    bool gather_before_mlp;     // the CLS rows' residual as it enters the MLP, i.e. BEHIND this block's proj (a live compact copy is the residual in front of it): always gathered
    bool scatter_after_proj;    // no CLS-row MLP behind the CLS-row proj: the rows go back before LayerNorm-2 reads them
    bool scatter_after_fc2;     // the chain's rows replace what the plain fc2 wrote
    bool cls_proj_fuses_ln2;    // the CLS-row proj is offered LayerNorm-2 of the compact rows (the CLS-row MLP reads it)
    bool c_resid_live_after;    // the compact rows hold the CLS rows of the token stream as this block leaves them (any other block's proj / fc2 moved them on without the compact copy)
};

// What block `block` of a lane of lane_tiles tiles does.  xn_ready: the previous block's fc2 already wrote this block's LayerNorm-1 output;
// fp4_planes_available: the qkv weight and the workspace have their MX-fp4 side planes; c_resid_live: the compact rows hold the CLS rows of the
// token stream as they are now.
// Where the 11 bits of an fp16 operand are not enough (tools/precision_study.py: block 0 alone is 41 % of the cosine error variance, blocks 0-1 52 %,
// and outside them the MLP GEMMs carry > 80 %), a block runs what the plan names; KEEP_PREC_STRICT and the first strict_blocks blocks run split
// products whatever it names, KEEP_PREC_FP16 plain ones.
inline BlockSteps resolve_block(const PrecisionPlan& p, int block, int lane_tiles, bool xn_ready, bool fp4_planes_available, bool c_resid_live) {
    auto strict = [&](int i) { return p.precision == KEEP_PREC_STRICT || i < p.strict_blocks; };
    auto planned = [&](int i) { return !strict(i) && p.precision == KEEP_PREC_COMP && i >= 0 && i < PrecisionPlan::MAX_BLOCKS; };
    // lanes too small for the 256x256 kernel take split products wherever a compensated one is asked for (they run on the small-M / K-sliced kernels)
    auto takes_comp = [&](int tiles) { return tiles >= p.comp_min_tiles && p.vit_has_q; };
    auto compqkv_only = [](int a) { return a == KEEP_ATTN_COMPQKV || a == KEEP_ATTN_COMPQKV_PROJ_CLS; };
    auto attn_mode = [&](int i) { return planned(i) ? p.attn_mode[i] : int(strict(i) ? KEEP_ATTN_SPLIT : KEEP_ATTN_PLAIN); };
    auto attn_split = [&](int i) { const int a = attn_mode(i); return a == KEEP_ATTN_SPLIT || a == KEEP_ATTN_SPLIT_COMPQKV || (compqkv_only(a) && !takes_comp(lane_tiles)); };
    const int attn = attn_mode(block);
    BlockSteps s{};
    s.cls_only = block == p.vit_depth - 1 && p.cls_tail;
    s.attn_split = attn_split(block);
    s.qkv_comp = (attn == KEEP_ATTN_SPLIT_COMPQKV || compqkv_only(attn)) && takes_comp(lane_tiles) && fp4_planes_available && !xn_ready;
    s.cls_proj = !s.attn_split && !s.cls_only && (attn == KEEP_ATTN_PROJ_CLS || attn == KEEP_ATTN_COMPQKV_PROJ_CLS);
    // fc1 / fc2.  The last block's CLS-rows-only tail is no lane for a compensated product (it counts as 0 tiles), and it IS the "CLS rows as
    // split products" half of KEEP_MLP_CLS on its own.
    int mlp = planned(block) ? p.mlp_mode[block] : int(strict(block) ? KEEP_MLP_SPLIT : KEEP_MLP_PLAIN);
    if ((mlp == KEEP_MLP_COMP || mlp == KEEP_MLP_COMP_W) && !takes_comp(s.cls_only ? 0 : lane_tiles)) mlp = KEEP_MLP_SPLIT;
    if (mlp == KEEP_MLP_CLS && s.cls_only) mlp = KEEP_MLP_SPLIT;
    s.cls_mlp = mlp == KEEP_MLP_CLS;
    const bool mlp_split = mlp == KEEP_MLP_SPLIT, mlp_plain = mlp == KEEP_MLP_PLAIN || s.cls_mlp;
    const int mlp_comp = mlp == KEEP_MLP_COMP ? 2 : mlp == KEEP_MLP_COMP_W ? 1 : 0;

    s.qkv = {s.attn_split && !s.qkv_comp, s.qkv_comp ? 2 : 0, !s.attn_split && !s.qkv_comp, (s.attn_split || s.qkv_comp) ? T_VIT_QKV_X : T_VIT_QKV};
    s.attn_tag = s.attn_split ? T_VIT_ATTN_X : T_VIT_ATTN;
    s.proj = {s.attn_split, 0, !s.attn_split, s.cls_only ? T_VIT_TAIL : s.attn_split ? T_VIT_PROJ_X : T_VIT_PROJ};
    s.fc1 = {mlp_split, mlp_comp, mlp_plain, s.cls_only ? T_VIT_TAIL : !mlp_plain ? T_VIT_FC1_X : T_VIT_FC1};
    s.fc2 = {mlp_split, mlp_comp, mlp_plain, s.cls_only ? T_VIT_TAIL : !mlp_plain ? T_VIT_FC2_X : T_VIT_FC2};
    s.ln1 = {s.qkv.split, s.qkv_comp, false};
    s.ln2 = {mlp_split, mlp_comp != 0, mlp_comp == 1};
    s.ln2_to_proj = !mlp_comp;
    s.next_ln1_to_fc2 = block + 1 < p.vit_depth && !s.cls_only && !s.cls_mlp;
    s.next_ln1_lo = s.next_ln1_to_fc2 && attn_split(block + 1);
    s.gather_before_proj = s.cls_proj && !c_resid_live;
    s.gather_before_mlp = s.cls_mlp && !s.cls_proj;
    s.scatter_after_proj = s.cls_proj && !s.cls_mlp;
    s.scatter_after_fc2 = s.cls_mlp;
    s.cls_proj_fuses_ln2 = s.cls_proj && s.cls_mlp;
    s.c_resid_live_after = s.cls_mlp;
    return s;
}
