// Prints resolve_block (keep_amd/csrc/block_plan.h) over every combination of its inputs as CSV: one header line, one row per case.
// tests/test_block_plan.py compiles it with a host compiler, runs it and checks every row.  Every block of the plan gets the same
// (attention, MLP) mode pair; the depth is 3, so block 0 / 1 / 2 are a first, a middle and the last block.
#include "../keep_amd/csrc/block_plan.h"

#include <cstdio>

int main() {
    printf("precision,strict_blocks,attn_mode,mlp_mode,lane_tiles,comp_min_tiles,vit_has_q,cls_tail,block,depth,xn_ready,fp4_planes_available,c_resid_live,"
           "any_split,any_comp,txt_split,"
           "cls_only,attn_split,qkv_comp,cls_proj,cls_mlp,"
           "qkv_split,qkv_comp_terms,qkv_corrected_bias,qkv_tag,attn_tag,"
           "proj_split,proj_comp_terms,proj_corrected_bias,proj_tag,"
           "fc1_split,fc1_comp_terms,fc1_corrected_bias,fc1_tag,"
           "fc2_split,fc2_comp_terms,fc2_corrected_bias,fc2_tag,"
           "ln1_lo,ln1_fp4,ln1_fp4_hi_only,ln2_lo,ln2_fp4,ln2_fp4_hi_only,"
           "ln2_to_proj,next_ln1_to_fc2,next_ln1_lo,gather_before_proj,gather_before_mlp,scatter_after_proj,scatter_after_fc2,"
           "cls_proj_fuses_ln2,c_resid_live_after\n");
    const int precisions[] = {KEEP_PREC_FP16, KEEP_PREC_STRICT, KEEP_PREC_COMP};
    const int depth = 3;
    auto site = [](const SiteStep& s) { printf("%d,%d,%d,%d,", s.split, s.comp, s.corrected_bias, s.tag); };
    for (int precision : precisions)
    for (int strict_blocks = 0; strict_blocks <= 1; ++strict_blocks)
    for (int attn = KEEP_ATTN_PLAIN; attn <= KEEP_ATTN_COMPQKV_PROJ_CLS; ++attn)
    for (int mlp = KEEP_MLP_PLAIN; mlp <= KEEP_MLP_CLS; ++mlp)
    for (int small_lane = 1; small_lane >= 0; --small_lane)
    for (int has_q = 0; has_q <= 1; ++has_q)
    for (int cls_tail = 0; cls_tail <= 1; ++cls_tail) {
        PrecisionPlan p;
        p.precision = precision; p.strict_blocks = strict_blocks; p.vit_has_q = has_q; p.cls_tail = cls_tail; p.vit_depth = depth;
        for (int i = 0; i < PrecisionPlan::MAX_BLOCKS; ++i) { p.attn_mode[i] = (unsigned char)attn; p.mlp_mode[i] = (unsigned char)mlp; }
        const int lane_tiles = p.comp_min_tiles - small_lane;
        for (int block = 0; block < depth; ++block)
        for (int xn_ready = 0; xn_ready <= 1; ++xn_ready)
        for (int fp4 = 0; fp4 <= 1; ++fp4)
        for (int live = 0; live <= 1; ++live) {
            const BlockSteps s = resolve_block(p, block, lane_tiles, xn_ready, fp4, live);
            printf("%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,", precision, strict_blocks, attn, mlp, lane_tiles, p.comp_min_tiles, has_q, cls_tail, block, depth, xn_ready, fp4, live);
            printf("%d,%d,%d,", p.any_split(), p.any_comp(), p.txt_split(block, 64));
            printf("%d,%d,%d,%d,%d,", s.cls_only, s.attn_split, s.qkv_comp, s.cls_proj, s.cls_mlp);
            site(s.qkv); printf("%d,", s.attn_tag); site(s.proj); site(s.fc1); site(s.fc2);
            printf("%d,%d,%d,%d,%d,%d,", s.ln1.lo, s.ln1.fp4, s.ln1.fp4_hi_only, s.ln2.lo, s.ln2.fp4, s.ln2.fp4_hi_only);
            printf("%d,%d,%d,%d,%d,%d,%d,%d,%d\n", s.ln2_to_proj, s.next_ln1_to_fc2, s.next_ln1_lo, s.gather_before_proj, s.gather_before_mlp,
                   s.scatter_after_proj, s.scatter_after_fc2, s.cls_proj_fuses_ln2, s.c_resid_live_after);
        }
    }
    return 0;
}
