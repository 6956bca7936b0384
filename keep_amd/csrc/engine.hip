// Host side of libkeep_hip: workspace arena, graph replay, tower orchestration, options and the encoder's part of the extern "C"
// boundary declared in include/keep_hip.h.  The handle itself is handle.h, the decision what a block of the image tower runs under the
// precision plan block_plan.h (vit_layer here only issues what it resolves); weight ingestion is weights.hip; the single-operator
// entry points and probes are op_api.hip; the slide-geometry entry points (patch grid, tissue mask, heatmap, sort / rank, regions,
// outlines, polygon fill, evaluation) are slide_api.hip.
//
// Orchestration mirrors the reference's call order, not its code:
//   encode_image  quick_start/keep_inference.py:54-58  -> timm VisionTransformer.forward
//   encode_text   quick_start/keep_inference.py:60-62  -> HF BertModel.forward           
#include "handle.h"
#include "quant4.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

// encode_text calls of up to this many token rows (64 prompts x 64 tokens after padding trim: a whole classifier bank chunk) are captured once per shape
// and replayed as one graph launch: ~90 dependent kernels of 10-25 us whose host-side issue (1.4 ms) otherwise runs next to them
constexpr int64_t TXT_GRAPH_ROWS = 4096;

const char* kTagNames[T_COUNT] = {
    "vit.im2col", "vit.patch", "vit.ln", "vit.qkv", "vit.attn", "vit.proj", "vit.fc1", "vit.fc2", "vit.head",
    "text.embed", "text.ln", "text.qkv", "text.attn", "text.out", "text.ffn1", "text.ffn2", "text.pool", "sim",
    "vit.qkv.x", "vit.attn.x", "vit.proj.x", "vit.fc1.x", "vit.fc2.x", "vit.tail"};

struct Scope {     // RAII profile bracket
    keep_handle* h; int tag; hipStream_t s;
    Scope(keep_handle* h_, int t, hipStream_t s_) : h(h_), tag(t), s(s_) { h->prof_begin(tag, s); }
    ~Scope() { h->prof_end(tag, s); }
};

size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// Hands out 256-byte-aligned pieces of an arena.  Without a base it only measures: every pointer is null and `off` is what the layout consumes,
// so a workspace is described once (carve_vit / carve_txt) and its size is whatever that description took.
struct Carver {
    char* base; size_t off = 0;
    explicit Carver(char* b) : base(b) {}
    template <typename T> T* take(size_t n) { T* p = base ? reinterpret_cast<T*>(base + off) : nullptr; off += align_up(n * sizeof(T)); return p; }
};
// Every tower workspace is this much larger than the buffers carved from it.  Kept from the hand-written size formulas the carve-derived sizes
// replace (they ended in "+ 4096"); the reason is not recorded.  Arena sizes, and with them the staging offsets behind a workspace, depend on it.
constexpr size_t WS_TAIL_BYTES = 4096;

// What both towers carve, in this order: M token rows of width D and hidden width F (lo planes in split mode only), and -- last in either
// tower -- the state split attention parks per (item, head, query) between its two key windows of <= 256 keys (launch_attention).
struct TowerWs { float* splitk; float* resid; f16 *xn_hi, *xn_lo, *qkv_hi, *qkv_lo, *att_hi, *att_lo, *mlp_hi, *mlp_lo;
                 float* part; size_t part_bytes;
                 size_t bytes; };                            // the whole layout, WS_TAIL_BYTES included
struct VitWs : TowerWs { f16 *pat_hi, *pat_lo; float *cls, *h1;
               unsigned char *xn_q, *xn_sc, *mlp_q, *mlp_sc;     // MX-fp4 side planes of the LayerNorm-2 output and of the MLP hidden (compensated mode)
               // compact CLS-row buffers for the last block
               float* c_resid; f16 *c_att_hi, *c_att_lo, *c_xn_hi, *c_xn_lo, *c_mlp_hi, *c_mlp_lo; };

void carve_tower(Carver& c, TowerWs& w, size_t M, size_t D, size_t F, bool split) {
    w.splitk = c.take<float>(SKINNY_WS_BYTES / 4);
    w.resid = c.take<float>(M * D);
    w.xn_hi = c.take<f16>(blk_elems(M, D));  w.xn_lo = split ? c.take<f16>(blk_elems(M, D)) : nullptr;
    w.qkv_hi = c.take<f16>(M * 3 * D);       w.qkv_lo = split ? c.take<f16>(M * 3 * D) : nullptr;
    w.att_hi = c.take<f16>(blk_elems(M, D)); w.att_lo = split ? c.take<f16>(blk_elems(M, D)) : nullptr;
    w.mlp_hi = c.take<f16>(blk_elems(M, F)); w.mlp_lo = split ? c.take<f16>(blk_elems(M, F)) : nullptr;
}
void carve_part(Carver& c, TowerWs& w, size_t queries, bool windowed) {      // queries = items x heads x tokens
    w.part_bytes = windowed ? queries * ATT_PART_FLOATS * sizeof(float) : 0;
    if (w.part_bytes) w.part = c.take<float>(w.part_bytes / sizeof(float));
    w.bytes = c.off + WS_TAIL_BYTES;
}
VitWs carve_vit(const keep_handle* h, char* arena, int64_t Bc, bool split, int ntok = 197) {
    const size_t M = (size_t)Bc * ntok, Mp = (size_t)Bc * (ntok - 1), D = h->vit_D, F = h->vit_F;
    Carver c(arena); VitWs w{};
    carve_tower(c, w, M, D, F, split);
    w.pat_hi = c.take<f16>(blk_elems(Mp, 768)); w.pat_lo = c.take<f16>(blk_elems(Mp, 768));
    w.cls = c.take<float>((size_t)Bc * D);
    w.h1 = c.take<float>((size_t)Bc * h->proj_dim);
    w.c_resid = c.take<float>((size_t)Bc * D);
    w.c_att_hi = c.take<f16>(blk_elems(Bc, D)); w.c_att_lo = c.take<f16>(blk_elems(Bc, D));
    w.c_xn_hi = c.take<f16>(blk_elems(Bc, D));  w.c_xn_lo = c.take<f16>(blk_elems(Bc, D));
    w.c_mlp_hi = c.take<f16>(blk_elems(Bc, F)); w.c_mlp_lo = c.take<f16>(blk_elems(Bc, F));
    if (h->any_comp()) {
        w.xn_q = c.take<unsigned char>(keepk::q4_data_bytes(M, D));  w.xn_sc = c.take<unsigned char>(keepk::q4_scale_bytes(M, D));
        w.mlp_q = c.take<unsigned char>(keepk::q4_data_bytes(M, F)); w.mlp_sc = c.take<unsigned char>(keepk::q4_scale_bytes(M, F));
    }
    carve_part(c, w, M * h->vit_heads, split && ntok > 256 && ntok <= 512);   // beyond 512 tokens the key-blocked kernel runs, which keeps no state
    return w;
}
TowerWs carve_txt(const keep_handle* h, char* arena, int64_t Pc, int64_t T, bool split) {
    Carver c(arena); TowerWs w{};
    carve_tower(c, w, (size_t)Pc * T, h->bert_H, h->bert_F, split);
    carve_part(c, w, (size_t)Pc * T * h->bert_heads, split && T > 256);
    return w;
}
size_t vit_ws_bytes(const keep_handle* h, int64_t Bc, bool split, int ntok = 197) { return carve_vit(h, nullptr, Bc, split, ntok).bytes; }
size_t txt_ws_bytes(const keep_handle* h, int64_t Pc, int64_t T, bool split) { return carve_txt(h, nullptr, Pc, T, split).bytes; }

// How one keep_encode_image call of B tiles of ntok tokens lays the arena out: `lanes` concurrent sub-batches of at most `per` tiles, each on
// lane_bytes of workspace.  staged: the call is replayed as a captured graph (or, for keep_reserve, may be), which runs as ONE lane of all B
// tiles on copies of the pixels and of the output parked behind the workspace (at most SKINNY_MAX_M token rows: never enough for a second lane).
struct VitPlan { int lanes; int64_t per; bool split; size_t lane_bytes, o_pix, o_out, total; };
VitPlan vit_plan(const keep_handle* h, int64_t B, int ntok, size_t tile_bytes, bool staged) {
    VitPlan p{};
    // lanes: split the batch over n_streams concurrent sub-batches once there is enough work for each (in 197-token tile equivalents)
    p.lanes = h->n_streams;
    while (p.lanes > 1 && B * ntok < (int64_t)p.lanes * h->lane_min_tiles * 197) --p.lanes;
    p.per = (B + p.lanes - 1) / p.lanes;
    // sub-batches are bounded in tokens: per * ntok <= max_tiles * 197 (a 512 x 512 call needs the arena of a 224 x 224 one)
    const int64_t per_max = std::max<int64_t>((int64_t)h->max_tiles * 197 / ntok, 1);
    if (p.per > per_max && !(staged && B <= h->max_tiles)) p.per = per_max;
    p.split = h->any_split();
    p.lane_bytes = align_up(vit_ws_bytes(h, p.per, p.split, ntok));
    p.total = p.lane_bytes * p.lanes;
    if (staged) {
        p.o_pix = p.total;
        p.o_out = p.o_pix + align_up((size_t)B * tile_bytes);
        p.total = p.o_out + align_up((size_t)B * h->proj_dim * sizeof(float));
    }
    return p;
}
// The same for one keep_encode_text call of P prompts of T tokens: chunks of at most `pc` prompts on one workspace; a graph-replayed call runs
// on staged ids / types / mask and a staged output behind it.
struct TxtPlan { int64_t pc; bool split; size_t ws_bytes, o_ids, o_types, o_mask, o_out, total; };
TxtPlan txt_plan(const keep_handle* h, int64_t P, int64_t T, bool staged) {
    TxtPlan p{};
    p.pc = P < h->max_prompts ? P : h->max_prompts;
    p.split = h->any_split();
    p.total = p.ws_bytes = align_up(txt_ws_bytes(h, p.pc, T, p.split));
    if (staged) {
        const size_t nb = align_up((size_t)P * T * sizeof(int64_t));
        p.o_ids = p.ws_bytes; p.o_types = p.o_ids + nb; p.o_mask = p.o_types + nb; p.o_out = p.o_mask + nb;
        p.total = p.o_out + align_up((size_t)P * h->bert_H * sizeof(float));
    }
    return p;
}
}  // namespace

int ensure_arena(keep_handle* h, size_t bytes) {
    if (bytes <= h->arena_bytes) return KEEP_OK;
    HIPCHK(h, hipDeviceSynchronize());
    if (h->arena) HIPCHK(h, hipFree(h->arena));
    h->arena = nullptr; h->arena_bytes = 0;
    HIPCHK(h, hipMalloc(&h->arena, bytes));
    h->arena_bytes = bytes;
    return KEEP_OK;
}

int check_launch(keep_handle* h, const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return h->fail(KEEP_EHIP, "%s: %s", what, hipGetErrorString(e));
    return KEEP_OK;
}

namespace {

void drop_graphs(keep_handle* h) {
    for (auto& kv : h->graphs) (void)hipGraphExecDestroy(kv.second.exec);
    h->graphs.clear();
}

// Replays `body` (which must only enqueue work on the stream it is given: no allocation, no synchronisation) as one
// graph launch on `s`; captures it on first use.
template <class F>
int graph_run(keep_handle* h, const std::string& key, hipStream_t s, F&& body) {
    auto it = h->graphs.find(key);
    if (it != h->graphs.end() && (it->second.epoch != h->opt_epoch || it->second.arena != h->arena)) {
        (void)hipGraphExecDestroy(it->second.exec);
        h->graphs.erase(it);
        it = h->graphs.end();
    }
    if (it == h->graphs.end()) {
        if (!h->cap_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking));
        HIPCHK(h, hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal));
        const int rc = body(h->cap_stream);
        hipGraph_t g = nullptr;
        const hipError_t e = hipStreamEndCapture(h->cap_stream, &g);
        if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
        HIPCHK(h, e);
        hipGraphExec_t ex = nullptr;
        const hipError_t ei = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        HIPCHK(h, ei);
        it = h->graphs.emplace(key, keep_handle::GraphSlot{ex, h->opt_epoch, h->arena}).first;
    }
    HIPCHK(h, hipGraphLaunch(it->second.exec, s));
    return KEEP_OK;
}

int run_gemm(keep_handle* h, int tag, GemmParams p, int epi, hipStream_t s, float* splitk) {
    h->prof_add_flops(tag, 2.0 * p.M * (double)p.N * p.K);     // algorithmic FLOPs: extra passes of a split / compensated product are not counted
    p.splitk_ws = splitk; p.splitk_bytes = SKINNY_WS_BYTES;
    return launch_gemm_f16(p, epi, s);
}

// ---------------------------------------------------------------------------------------------
// One sub-batch of tiles in flight on one stream ("lane").  keep_encode_image runs up to n_streams lanes
// concurrently and issues their kernels layer-interleaved, so one lane's memory-bound phases (LayerNorm,
// attention staging, GEMM epilogues, partial last rounds of workgroups) overlap the other lane's MFMA phases.
struct VitLane {
    const void* pixels; int pix_dtype; int Bc; float* out; hipStream_t s; VitWs ws; bool cls_compact = false;
    int gh = 14, gw = 14, ntok = 197;                     // patch grid and tokens per tile (gh gw + 1)
    const float* pos = nullptr;                           // position table of that grid, [ntok][D] (vit_pos_table)
    bool xn_ready = false;                                // the previous block's fc2 already wrote this block's LayerNorm-1 output
    bool c_resid_live = false;                            // ws.c_resid holds the CLS rows of ws.resid as they are NOW (left there by the previous block's CLS-row chain): no gather
    int tap_block = -1; float* tap_out = nullptr;         // keep_encode_image_attn: the block whose CLS-row attention probabilities go to tap_out, this lane's [Bc][heads][ntok]
    // keep_encode_image_rollout: a step behind the attention launch of every block >= roll_start (-1: none).  roll_r: the lane's two
    // [Bc][ntok][ntok] ping-pong buffers (roll_cur holds the running product), roll_a: the same size, At between the step's two kernels; roll_out: this
    // lane's [Bc][ntok] of the result, written by the last block's step
    int roll_start = -1; float roll_res = 0.5f; float* roll_r[2] = {nullptr, nullptr}; float* roll_a = nullptr; float* roll_out = nullptr; int roll_cur = 0;
};

int vit_begin(keep_handle* h, VitLane& L) {
    const int D = h->vit_D, Bc = L.Bc;
    hipStream_t s = L.s; VitWs& ws = L.ws; const void* pixels = L.pixels; const int pix_dtype = L.pix_dtype;
    // The patch embed is 0.25 % of the FLOPs but its rounding error feeds all 24 blocks: it runs as the hi/lo split product
    // (option "patch_split" = 0, experiments: one fp16 pass -- KEEP_PREC_FP16 and KEEP_PREC_COMP only).
    const bool sp0 = h->patch_split || h->precision == KEEP_PREC_STRICT || h->strict_blocks > 0;
    {
        Scope sc(h, T_VIT_IM2COL, s);
        launch_im2col(pixels, pix_dtype, Bc, L.gh, L.gw, ws.pat_hi, sp0 ? ws.pat_lo : nullptr,
                      find_weight(h, "visual.cls_token")->f32, L.pos, ws.resid, D, s);
    }
    {
        Scope sc(h, T_VIT_PATCH, s);
        GemmParams p = gemm_params(h, ws.pat_hi, ws.pat_lo, find_weight(h, "visual.patch_embed.proj.weight"), Bc * (L.ntok - 1), sp0,
                                   find_weight(h, "visual.patch_embed.proj.bias")->f32);
        p.pos = L.pos; p.patches_per_img = L.ntok - 1;
        p.resid = ws.resid;
        if (run_gemm(h, T_VIT_PATCH, p, EPI_PATCH, s, ws.splitk) < 0) return h->fail(KEEP_EUNSUPPORTED, "patch-embedding GEMM launch failed");
    }
    return KEEP_OK;
}

// mean-input compensation: a PLAIN launch of site k of block i uses the bias with W_lo a_mean folded in; while calibrating, every site's input is summed
const float* site_bias(const keep_handle* h, int i, int site, const float* orig, bool plain) {
    return (plain && h->bias_ready && h->bias_correction && i < (int)h->cal.size() && h->cal[i].bias[site]) ? (const float*)h->cal[i].bias[site] : orig;
}
void capture(keep_handle* h, int i, int site, const f16* a_hi, int rows, int K, hipStream_t s) {
    if (!h->capture || i >= (int)h->cal.size() || !h->cal[i].sum[site]) return;
    launch_blk_col_sum(a_hi, rows, K, h->cal[i].sum[site], s);
    h->cal[i].rows[site] += rows;
}

// The rows a block's per-token operators (proj, LayerNorm-2, fc1, fc2) run on: every token row of the lane, or the compact CLS rows (one per tile)
struct RowSet { int M; float* resid; const f16 *att_hi, *att_lo; f16 *xn_hi, *xn_lo, *mlp_hi, *mlp_lo; };
RowSet all_rows(const VitLane& L) { const VitWs& w = L.ws; return {L.Bc * L.ntok, w.resid, w.att_hi, w.att_lo, w.xn_hi, w.xn_lo, w.mlp_hi, w.mlp_lo}; }
RowSet cls_rows(const VitLane& L) { const VitWs& w = L.ws; return {L.Bc, w.c_resid, w.c_att_hi, w.c_att_lo, w.c_xn_hi, w.c_xn_lo, w.c_mlp_hi, w.c_mlp_lo}; }
// every site of the CLS-row chain: a split product with the checkpoint's own bias; its LayerNorm-2 writes hi + lo
constexpr SiteStep kClsSite{true, 0, false, T_VIT_TAIL};
constexpr LnStep kClsLn{true, false, false};

// the CLS rows of the token stream's residual -> compact rows, and back
void gather_cls_resid(keep_handle* h, VitLane& L) {
    Scope sc(h, T_VIT_TAIL, L.s);
    launch_gather_rows_f32(L.ws.resid, (int64_t)L.ntok * h->vit_D, L.ws.c_resid, L.Bc, h->vit_D, L.s);
}
void scatter_cls_resid(keep_handle* h, VitLane& L) {
    Scope sc(h, T_VIT_TAIL, L.s);
    launch_scatter_rows_f32(L.ws.c_resid, L.ws.resid, (int64_t)L.ntok * h->vit_D, L.Bc, h->vit_D, L.s);
}

// a LayerNorm of a block over `rows` rows of x: the hi plane of its output always, the other planes as `w` says
LnParams block_ln(const keep_handle* h, const VitWs& ws, const float* x, int rows, f16* out_hi, f16* out_lo, const LnStep& w, const float* gamma, const float* beta) {
    LnParams ln = ln_params(h, x, h->vit_D, rows, h->vit_D, 1e-6f);
    ln.out_hi = out_hi; ln.out_lo = w.lo ? out_lo : nullptr; ln.out_kt = h->vit_D / 32;
    ln.out_q = w.fp4 ? ws.xn_q : nullptr; ln.out_sc = w.fp4 ? ws.xn_sc : nullptr; ln.out_q_hi_only = w.fp4_hi_only;
    ln.gamma = gamma; ln.beta = beta;
    return ln;
}
// proj / fc1 / fc2 of block i on the rows `r`, run as `st` says
GemmParams proj_gemm(const keep_handle* h, int i, const RowSet& r, const SiteStep& st) {
    const VitBlock& b = h->vblocks[i];
    GemmParams p = gemm_params(h, r.att_hi, r.att_lo, b.proj, r.M, st.split, site_bias(h, i, 1, b.proj_b, st.corrected_bias));
    p.ls = b.ls1; p.resid = r.resid;
    return p;
}
GemmParams fc1_gemm(const keep_handle* h, int i, const VitWs& ws, const RowSet& r, const SiteStep& st) {
    const VitBlock& b = h->vblocks[i];
    GemmParams p = gemm_params(h, r.xn_hi, r.xn_lo, b.fc1, r.M, st.split, site_bias(h, i, 2, b.fc1_b, st.corrected_bias));
    p.out_hi = r.mlp_hi; p.out_lo = st.split ? r.mlp_lo : nullptr; p.out_kt = h->vit_F / 32;
    if (st.comp) {
        p.comp = st.comp; p.a_q = ws.xn_q; p.a_sc = ws.xn_sc; p.w_q = b.fc1->q; p.w_sc = b.fc1->sc;
        p.out_q = ws.mlp_q; p.out_sc = ws.mlp_sc;
    }
    return p;
}
GemmParams fc2_gemm(const keep_handle* h, int i, const VitWs& ws, const RowSet& r, const SiteStep& st) {
    const VitBlock& b = h->vblocks[i];
    GemmParams p = gemm_params(h, r.mlp_hi, r.mlp_lo, b.fc2, r.M, st.split, site_bias(h, i, 3, b.fc2_b, st.corrected_bias));
    p.ls = b.ls2; p.resid = r.resid;
    if (st.comp) { p.comp = st.comp; p.a_q = ws.mlp_q; p.a_sc = ws.mlp_sc; p.w_q = b.fc2->q; p.w_sc = b.fc2->sc; }
    return p;
}

// LayerNorm-1 (unless the previous block's fc2 wrote it), qkv, attention, and what taps the attention: the CLS attention map and the rollout step
int vit_attn_side(keep_handle* h, VitLane& L, int i, const BlockSteps& st) {
    const int D = h->vit_D, Bc = L.Bc, ntok = L.ntok, M = Bc * ntok;
    hipStream_t s = L.s; VitWs& ws = L.ws;
    const VitBlock& b = h->vblocks[i];
    const bool sp = st.attn_split;
    if (!L.xn_ready) {
        Scope sc(h, T_VIT_LN, s);
        if (launch_layernorm(block_ln(h, ws, ws.resid, M, ws.xn_hi, ws.xn_lo, st.ln1, b.n1w, b.n1b), s)) return h->fail(KEEP_EUNSUPPORTED, "layernorm width %d", D);
    }
    L.xn_ready = false;
    {
        Scope sc(h, st.qkv.tag, s);
        capture(h, i, 0, ws.xn_hi, M, D, s);
        GemmParams p = gemm_params(h, ws.xn_hi, ws.xn_lo, b.qkv, M, st.qkv.split, site_bias(h, i, 0, b.qkv_b, st.qkv.corrected_bias));
        p.out_hi = ws.qkv_hi; p.out_lo = sp ? ws.qkv_lo : nullptr;
        if (st.qkv.comp) { p.comp = st.qkv.comp; p.a_q = ws.xn_q; p.a_sc = ws.xn_sc; p.w_q = b.qkv->q; p.w_sc = b.qkv->sc; }
        if (run_gemm(h, st.qkv.tag, p, EPI_F16, s, ws.splitk) < 0) return h->fail(KEEP_EUNSUPPORTED, "qkv GEMM launch failed");
    }
    {
        Scope sc(h, st.attn_tag, s);
        AttnParams a = attn_params(h, ws.qkv_hi, ws.qkv_lo, ws.att_hi, sp ? ws.att_lo : nullptr, Bc, ntok, h->vit_heads, sp, D / 32);
        a.q_rows = st.cls_only ? 1 : 0;
        if (st.cls_proj) { a.cls_hi = ws.c_att_hi; a.cls_lo = ws.c_att_lo; }
        a.part_ws = ws.part; a.part_bytes = ws.part_bytes;
        // beyond 512 tokens (grids past 22 x 22 patches) the key-blocked kernel; up to 512 the whole-sequence kernels of the 224 path
        if ((ntok > 512 ? launch_attention_long(a, s) : launch_attention(a, s))) return h->fail(KEEP_EUNSUPPORTED, "attention launch failed (%d tokens)", ntok);
    }
    if (i == L.tap_block && launch_attention_cls_probs(ws.qkv_hi, sp ? ws.qkv_lo : nullptr, Bc, ntok, h->vit_heads, 0.125f, L.tap_out, s))
        return h->fail(KEEP_EUNSUPPORTED, "CLS attention map launch failed (%d tokens)", ntok);
    if (L.roll_start >= 0 && i >= L.roll_start) {
        const bool first = i == L.roll_start, last = i == h->vit_depth - 1;      // the last block's step: the CLS row only, whether or not cls_tail is on
        float* r_out = last ? L.roll_out : L.roll_r[first ? L.roll_cur : L.roll_cur ^ 1];
        if (launch_attention_rollout_step(ws.qkv_hi, sp ? ws.qkv_lo : nullptr, Bc, ntok, h->vit_heads, 0.125f, L.roll_res, first ? nullptr : L.roll_r[L.roll_cur],
                                          r_out, last ? 1 : 0, L.roll_a, s))
            return h->fail(KEEP_EUNSUPPORTED, "attention rollout launch failed (%d tokens, at most %d)", ntok, ROLLOUT_MAX_TOKENS);
        if (!first && !last) L.roll_cur ^= 1;
    }
    return KEEP_OK;
}

// proj + LayerScale + residual on the rows `r`, offered their LayerNorm-2 (`ln`); in front of it the gathers into the compact rows.
// -> the GEMM_DID_* flags of the launch, or < 0
int vit_proj(keep_handle* h, VitLane& L, int i, const BlockSteps& st, const RowSet& r, const LnParams& ln) {
    hipStream_t s = L.s; VitWs& ws = L.ws;
    if (st.cls_only) {
        Scope sc(h, T_VIT_HEAD, s);
        launch_gather_rows_f32(ws.resid, (int64_t)L.ntok * h->vit_D, ws.c_resid, L.Bc, h->vit_D, s);
        launch_gather_rows_blk(ws.att_hi, L.ntok, ws.c_att_hi, L.Bc, h->vit_D, s);
        if (st.attn_split) launch_gather_rows_blk(ws.att_lo, L.ntok, ws.c_att_lo, L.Bc, h->vit_D, s);
        L.cls_compact = true;
    }
    if (st.gather_before_proj) gather_cls_resid(h, L);
    Scope sc(h, st.proj.tag, s);
    capture(h, i, 1, r.att_hi, r.M, h->vit_D, s);
    GemmParams p = proj_gemm(h, i, r, st.proj);
    p.impl_hint = h->proj_impl;
    if (st.ln2_to_proj) offer_ln(p, ln);
    const int did = run_gemm(h, st.proj.tag, p, EPI_RESID_LS, s, ws.splitk);
    return did < 0 ? h->fail(KEEP_EUNSUPPORTED, "proj GEMM launch failed") : did;
}

// The CLS-row chain of this block (KEEP_ATTN_PROJ_CLS and / or KEEP_MLP_CLS) on the compact [Bc, D] rows, in the lane's own stream: issued between the
// plain proj and LayerNorm-2, and scattered behind the plain fc2 (whose rows it replaces).  The small kernels then sit between the lane's two light kernels
// instead of between two persistent GEMMs: +1.5 % against the whole chain behind fc2.  On a side stream of its own the chain cost 11 %: a cross-queue
// dependency is a barrier packet the next persistent GEMM sits behind (both measured in round 6: tools/experiments/README.md).
int vit_cls_chain(keep_handle* h, VitLane& L, int i, const BlockSteps& st) {
    hipStream_t s = L.s; VitWs& ws = L.ws;
    const VitBlock& b = h->vblocks[i];
    const RowSet c = cls_rows(L);
    if (st.gather_before_mlp) gather_cls_resid(h, L);
    bool cls_ln_done = false;   // LayerNorm-2 of the compact CLS rows already written (hi + lo) by the CLS-row proj's epilogue
    const LnParams cl = block_ln(h, ws, c.resid, c.M, c.xn_hi, c.xn_lo, kClsLn, b.n2w, b.n2b);      // LayerNorm-2 of the compact CLS rows (KEEP_MLP_CLS)
    if (st.cls_proj) {
        // [Bc, D] x W_proj^T as a split product on the small-M kernels: the CLS rows' attention output from the fp32 accumulators (hi + lo) against W hi + lo,
        // + LayerScale + the residual.  With KEEP_MLP_CLS in the same block the chain continues on the compact rows (its LayerNorm-2 is fused into this GEMM's reduce)
        Scope sc(h, T_VIT_TAIL, s);
        GemmParams r = proj_gemm(h, i, c, kClsSite);
        if (st.cls_proj_fuses_ln2) offer_ln(r, cl);
        const int rc = run_gemm(h, T_VIT_TAIL, r, EPI_RESID_LS, s, ws.splitk);
        if (rc < 0) return h->fail(KEEP_EUNSUPPORTED, "CLS-row proj GEMM launch failed");
        cls_ln_done = st.cls_proj_fuses_ln2 && (rc & GEMM_DID_LN);
    }
    if (st.cls_mlp) {
        // LayerNorm-2 -> fc1 + GELU -> fc2 + LayerScale + residual as split products on the compact rows.  0.5 % of the rows; the feature is pooled from them.
        Scope sc(h, T_VIT_TAIL, s);
        if (!cls_ln_done && launch_layernorm(cl, s)) return h->fail(KEEP_EUNSUPPORTED, "layernorm width %d", h->vit_D);
        if (run_gemm(h, T_VIT_TAIL, fc1_gemm(h, i, ws, c, kClsSite), EPI_GELU_F16, s, ws.splitk) < 0) return h->fail(KEEP_EUNSUPPORTED, "CLS-row fc1 GEMM launch failed");
        if (run_gemm(h, T_VIT_TAIL, fc2_gemm(h, i, ws, c, kClsSite), EPI_RESID_LS, s, ws.splitk) < 0) return h->fail(KEEP_EUNSUPPORTED, "CLS-row fc2 GEMM launch failed");
    }
    if (st.scatter_after_proj) scatter_cls_resid(h, L);
    return KEEP_OK;
}

// fc1 + GELU and fc2 + LayerScale + residual on the rows `r`; fc2 is offered the next block's LayerNorm-1, and the CLS-row chain's rows go back behind it
int vit_mlp(keep_handle* h, VitLane& L, int i, const BlockSteps& st, const RowSet& r) {
    hipStream_t s = L.s; VitWs& ws = L.ws;
    {
        Scope sc(h, st.fc1.tag, s);
        capture(h, i, 2, r.xn_hi, r.M, h->vit_D, s);
        if (run_gemm(h, st.fc1.tag, fc1_gemm(h, i, ws, r, st.fc1), EPI_GELU_F16, s, ws.splitk) < 0) return h->fail(KEEP_EUNSUPPORTED, "fc1 GEMM launch failed");
    }
    {
        Scope sc(h, st.fc2.tag, s);
        capture(h, i, 3, r.mlp_hi, r.M, h->vit_F, s);
        GemmParams p = fc2_gemm(h, i, ws, r, st.fc2);
        if (st.next_ln1_to_fc2) {
            const VitBlock& nb = h->vblocks[i + 1];
            offer_ln(p, block_ln(h, ws, ws.resid, L.Bc * L.ntok, ws.xn_hi, ws.xn_lo, LnStep{st.next_ln1_lo, false, false}, nb.n1w, nb.n1b));
        }
        const int rc = run_gemm(h, st.fc2.tag, p, EPI_RESID_LS, s, ws.splitk);
        if (rc < 0) return h->fail(KEEP_EUNSUPPORTED, "fc2 GEMM launch failed");
        L.xn_ready = (rc & GEMM_DID_LN) != 0;
    }
    if (st.scatter_after_fc2) scatter_cls_resid(h, L);
    L.c_resid_live = st.c_resid_live_after;
    return KEEP_OK;
}

// One block of one lane: what it does is resolved once (block_plan.h); the rest issues launches
int vit_layer(keep_handle* h, VitLane& L, int i) {
    const VitBlock& b = h->vblocks[i];
    const BlockSteps st = resolve_block(*h, i, L.Bc, L.xn_ready, b.qkv->q && L.ws.xn_q, L.c_resid_live);
    if (int rc = vit_attn_side(h, L, i, st)) return rc;
    const RowSet r = st.cls_only ? cls_rows(L) : all_rows(L);
    const LnParams ln2 = block_ln(h, L.ws, r.resid, r.M, r.xn_hi, r.xn_lo, st.ln2, b.n2w, b.n2b);
    const int did = vit_proj(h, L, i, st, r, ln2);
    if (did < 0) return did;
    if (int rc = vit_cls_chain(h, L, i, st)) return rc;
    if (!(did & GEMM_DID_LN)) {
        Scope sc(h, T_VIT_LN, L.s);
        if (launch_layernorm(ln2, L.s)) return h->fail(KEEP_EUNSUPPORTED, "layernorm width %d", h->vit_D);
    }
    return vit_mlp(h, L, i, st, r);
}

int vit_end(keep_handle* h, VitLane& L) {
    const int D = h->vit_D, Bc = L.Bc;
    hipStream_t s = L.s; VitWs& ws = L.ws; float* out = L.out;
    {
        // final LayerNorm is per-token, global_pool='token' reads row 0 only -> normalise CLS rows only
        Scope sc(h, T_VIT_HEAD, s);
        LnParams ln = ln_params(h, L.cls_compact ? ws.c_resid : ws.resid, L.cls_compact ? (int64_t)D : (int64_t)L.ntok * D, Bc, D, 1e-6f);
        ln.gamma = find_weight(h, "visual.norm.weight")->f32; ln.beta = find_weight(h, "visual.norm.bias")->f32;
        ln.out_f32 = ws.cls; ln.out_f32_stride = D;
        launch_layernorm(ln, s);
        const WTensor* w0 = find_weight(h, "visual_head.0.weight");
        const WTensor* w2 = find_weight(h, "visual_head.2.weight");
        SgemmParams g{};
        g.tune = &h->tune;
        g.a = ws.cls; g.lda = D; g.b = w0->f32; g.ldb = D; g.out = ws.h1; g.ldo = h->proj_dim;
        g.bias = find_weight(h, "visual_head.0.bias")->f32; g.M = Bc; g.N = h->proj_dim; g.K = D; g.scale = 1.f; g.act = ACT_GELU;
        if (launch_sgemm_f32(g, s)) return h->fail(KEEP_EUNSUPPORTED, "visual_head.0 shape");
        g.a = ws.h1; g.lda = h->proj_dim; g.b = w2->f32; g.ldb = h->proj_dim; g.out = out; g.ldo = h->proj_dim;
        g.bias = find_weight(h, "visual_head.2.bias")->f32; g.K = h->proj_dim; g.act = ACT_NONE;
        if (launch_sgemm_f32(g, s)) return h->fail(KEEP_EUNSUPPORTED, "visual_head.2 shape");
        launch_l2norm_rows(out, Bc, h->proj_dim, 1e-12f, s, h->err_flag);
    }
    return check_launch(h, "encode_image");
}

int txt_chunk(keep_handle* h, const int64_t* ids, const int64_t* types, const int64_t* mask, int Pc, int T,
              float* out, hipStream_t s) {
    const bool any_split = h->any_split();
    const int H = h->bert_H, M = Pc * T;
    TowerWs ws = carve_txt(h, h->arena, Pc, T, any_split);
    {
        Scope sc(h, T_TXT_EMBED, s);
        launch_bert_embed_ln(ids, types, find_weight(h, "text.embeddings.word_embeddings.weight")->f32,
                             find_weight(h, "text.embeddings.position_embeddings.weight")->f32,
                             find_weight(h, "text.embeddings.token_type_embeddings.weight")->f32,
                             find_weight(h, "text.embeddings.LayerNorm.weight")->f32,
                             find_weight(h, "text.embeddings.LayerNorm.bias")->f32, 1e-12f, Pc, T, H, h->bert_vocab,
                             h->bert_types, ws.resid, ws.xn_hi, any_split ? ws.xn_lo : nullptr, h->err_flag, s);
    }
    for (int l = 0; l < h->bert_layers; ++l) {
        const BertLayer& b = h->blayers[l];
        const bool sp = h->txt_split(l, T);
        const bool sp_next = (l + 1 < h->bert_layers) && h->txt_split(l + 1, T);
        {
            Scope sc(h, T_TXT_QKV, s);
            GemmParams p = gemm_params(h, ws.xn_hi, ws.xn_lo, &b.qkv, M, sp, b.qkv_b);
            p.out_hi = ws.qkv_hi; p.out_lo = sp ? ws.qkv_lo : nullptr;
            if (run_gemm(h, T_TXT_QKV, p, EPI_F16, s, ws.splitk) < 0) return h->fail(KEEP_EUNSUPPORTED, "text qkv GEMM launch failed");
        }
        {
            Scope sc(h, T_TXT_ATTN, s);
            AttnParams a = attn_params(h, ws.qkv_hi, ws.qkv_lo, ws.att_hi, sp ? ws.att_lo : nullptr, Pc, T, h->bert_heads, sp, H / 32);
            a.mask = mask;
            a.part_ws = ws.part; a.part_bytes = ws.part_bytes;
            if (launch_attention(a, s)) return h->fail(KEEP_EUNSUPPORTED, "sequence length %d unsupported (max 512)", T);
        }
        LnParams ln = ln_params(h, ws.resid, H, M, H, 1e-12f);
        ln.out_f32 = ws.resid; ln.out_f32_stride = H; ln.out_hi = ws.xn_hi; ln.out_kt = H / 32;
        ln.gamma = b.ln1w; ln.beta = b.ln1b; ln.out_lo = sp ? ws.xn_lo : nullptr;
        int did;
        {
            Scope sc(h, T_TXT_OUT, s);
            GemmParams p = gemm_params(h, ws.att_hi, ws.att_lo, b.o, M, sp, b.o_b);
            p.resid = ws.resid; p.out_f32 = ws.resid;
            offer_ln(p, ln);
            did = run_gemm(h, T_TXT_OUT, p, EPI_RESID_F32, s, ws.splitk);
            if (did < 0) return h->fail(KEEP_EUNSUPPORTED, "text attention-output GEMM launch failed");
        }
        if (!(did & GEMM_DID_LN)) {
            Scope sc(h, T_TXT_LN, s);
            if (launch_layernorm(ln, s)) return h->fail(KEEP_EUNSUPPORTED, "layernorm width %d", H);
        }
        {
            Scope sc(h, T_TXT_FFN1, s);
            GemmParams p = gemm_params(h, ws.xn_hi, ws.xn_lo, b.i, M, sp, b.i_b);
            p.out_hi = ws.mlp_hi; p.out_lo = sp ? ws.mlp_lo : nullptr; p.out_kt = h->bert_F / 32;
            if (run_gemm(h, T_TXT_FFN1, p, EPI_GELU_F16, s, ws.splitk) < 0) return h->fail(KEEP_EUNSUPPORTED, "text FFN GEMM launch failed");
        }
        ln.gamma = b.ln2w; ln.beta = b.ln2b; ln.out_lo = sp_next ? ws.xn_lo : nullptr;
        {
            Scope sc(h, T_TXT_FFN2, s);
            GemmParams p = gemm_params(h, ws.mlp_hi, ws.mlp_lo, b.d, M, sp, b.d_b);
            p.resid = ws.resid; p.out_f32 = ws.resid;
            offer_ln(p, ln);
            did = run_gemm(h, T_TXT_FFN2, p, EPI_RESID_F32, s, ws.splitk);
            if (did < 0) return h->fail(KEEP_EUNSUPPORTED, "text FFN GEMM launch failed");
        }
        if (!(did & GEMM_DID_LN)) {
            Scope sc(h, T_TXT_LN, s);
            launch_layernorm(ln, s);
        }
    }
    {
        Scope sc(h, T_TXT_POOL, s);
        SgemmParams g{};
        g.tune = &h->tune;
        g.a = ws.resid; g.lda = (int64_t)T * H;            // row p*T: the [CLS] token of prompt p
        g.b = find_weight(h, "text.pooler.dense.weight")->f32; g.ldb = H; g.out = out; g.ldo = H;
        g.bias = find_weight(h, "text.pooler.dense.bias")->f32; g.M = Pc; g.N = H; g.K = H; g.scale = 1.f; g.act = ACT_TANH;
        if (launch_sgemm_f32(g, s)) return h->fail(KEEP_EUNSUPPORTED, "pooler shape");
        launch_l2norm_rows(out, Pc, H, 1e-12f, s, h->err_flag);
    }
    return check_launch(h, "encode_text");
}


int tag_by_name(const char* name) {
    for (int i = 0; i < T_COUNT; ++i) if (!strcmp(name, kTagNames[i])) return i;
    return -1;
}


// ATen's antialiased bicubic resample (F.interpolate(mode="bicubic", antialias=True, align_corners=False), what timm's
// resample_abs_pos_embed calls) as a weight table, in double: Keys cubic with a = -0.5, support 2 max(in / out, 1), window clipped at the
// edges (not edge-replicated), weights normalised per output.  beg[o]: first input index of output o; w[o][0..taps): its weights (zero-padded).
void aa_bicubic_table(int in, int out, std::vector<int>& beg, std::vector<double>& w, int& taps) {
    const double scale = (double)in / out;
    const double support = scale >= 1.0 ? 2.0 * scale : 2.0;
    const double invscale = scale >= 1.0 ? 1.0 / scale : 1.0;
    taps = (int)std::ceil(support) * 2 + 1;
    beg.assign(out, 0); w.assign((size_t)out * taps, 0.0);
    auto cubic = [](double x) {
        const double a = -0.5;
        x = std::fabs(x);
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
        if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
        return 0.0;
    };
    for (int o = 0; o < out; ++o) {
        const double center = scale * (o + 0.5);
        const int64_t lo = std::max<int64_t>((int64_t)(center - support + 0.5), 0);      // (int64_t) truncates, as ATen's cast does
        const int64_t n = std::min<int64_t>((int64_t)(center + support + 0.5), in) - lo;
        double total = 0.0;
        for (int64_t j = 0; j < n && j < taps; ++j) { const double v = cubic(((double)(j + lo) - center + 0.5) * invscale); w[(size_t)o * taps + j] = v; total += v; }
        if (total != 0.0)
            for (int j = 0; j < taps; ++j) w[(size_t)o * taps + j] /= total;
        beg[o] = (int)lo;
    }
}

// The position table of a gh x gw grid: the checkpoint's own at 14 x 14 (timm returns it unchanged there and only there), otherwise the
// CLS row as it is + the 14 x 14 patch table resampled to gh x gw (cached per grid, POS_CACHE grids).  Allocates and synchronises: never
// called inside a graph capture (encode_image_run asks for it before graph_run).
int vit_pos_table(keep_handle* h, int gh, int gw, const float** out) {
    const float* pos = find_weight(h, "visual.pos_embed")->f32;
    if (gh == 14 && gw == 14) { *out = pos; return KEEP_OK; }
    for (const auto& e : h->pos_cache) if (e.gh == gh && e.gw == gw) { *out = e.buf; return KEEP_OK; }
    if ((int)h->pos_cache.size() >= keep_handle::POS_CACHE) {
        HIPCHK(h, hipDeviceSynchronize());
        (void)hipFree(h->pos_cache.front().buf);
        h->pos_cache.erase(h->pos_cache.begin());
        ++h->opt_epoch;                          // a captured graph may hold the freed table's address
    }
    const int D = h->vit_D;
    std::vector<int> yb, xb;
    std::vector<double> wy, wx;
    int ty = 0, tx = 0;
    aa_bicubic_table(14, gh, yb, wy, ty);
    aa_bicubic_table(14, gw, xb, wx, tx);
    float* buf = nullptr;
    HIPCHK(h, hipMalloc(&buf, (size_t)(gh * gw + 1) * D * sizeof(float)));
    Tmp t;
    int* d_yb = t.get<int>(yb.size()); int* d_xb = t.get<int>(xb.size());
    double* d_wy = t.get<double>(wy.size()); double* d_wx = t.get<double>(wx.size());
    if (!t.ok) { (void)hipFree(buf); return h->fail(KEEP_ENOMEM, "position table: temp alloc"); }
    hipError_t e = hipMemcpy(d_yb, yb.data(), yb.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_xb, xb.data(), xb.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_wy, wy.data(), wy.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_wx, wx.data(), wx.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch_pos_resample(pos, 14, D, gh, gw, d_yb, d_wy, ty, d_xb, d_wx, tx, buf, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();         // the tables above are freed on return
    if (e != hipSuccess) { (void)hipFree(buf); return h->fail(KEEP_EHIP, "position table: %s", hipGetErrorString(e)); }
    h->pos_cache.push_back({gh, gw, buf});
    *out = buf;
    return KEEP_OK;
}

// the image tower on B tiles of a gh x gw patch grid (arguments checked, device selected by the caller)
// tap_out: fp32 [B][heads][ntok], the CLS-row attention probabilities of block tap_block (keep_encode_image_attn); such a call is never captured or replayed
// roll: keep_encode_image_rollout's start block, residual weight, output [B][ntok] and scratch (rollout_scratch); never captured or replayed either
struct RollArgs { int start; float residual; float* out; char* scratch; int64_t scratch_bytes; };
// what the rollout of one call keeps live: per lane of a round, two ping-pong [per][ntok][ntok] and At of the same size
struct RollPlan { size_t buf, lane, total; };
RollPlan rollout_scratch(int64_t B, int ntok, const VitPlan& plan) {
    RollPlan r{};
    const int64_t live = std::min<int64_t>(B, plan.per * plan.lanes);             // only the tiles of one round of lanes are live at a time
    r.buf = align_up((size_t)plan.per * ntok * ntok * sizeof(float));
    r.lane = 3 * r.buf;
    r.total = r.lane * (size_t)((live + plan.per - 1) / plan.per);
    return r;
}
int encode_image_run(keep_handle* h, const void* pixels, int pix_dtype, int64_t B, float* out, hipStream_t s, int gh = 14, int gw = 14,
                     int tap_block = -1, float* tap_out = nullptr, const RollArgs* roll = nullptr) {
    const int ntok = gh * gw + 1;
    const bool g14 = gh == 14 && gw == 14;
    const float* pos = nullptr;
    int rc = vit_pos_table(h, gh, gw, &pos);            // outside any capture: it may allocate
    if (rc) return rc;
    const size_t px = pix_dtype == KEEP_PIX_F32 ? 4 : (pix_dtype == KEEP_PIX_U8_HWC ? 1 : 2);    // bytes per value; 3 * 16 gh * 16 gw values per tile in every layout
    const size_t tile_vals = (size_t)3 * (gh * 16) * (gw * 16);
    const bool graph = h->use_graphs && !h->prof_mode && B * ntok <= SKINNY_MAX_M && B <= h->max_tiles && !tap_out && !roll;
    const VitPlan plan = vit_plan(h, B, ntok, tile_vals * px, graph);
    const RollPlan rp = roll ? rollout_scratch(B, ntok, plan) : RollPlan{};
    if (roll && (int64_t)rp.total > roll->scratch_bytes)
        return h->fail(KEEP_EINVAL, "rollout scratch of %lld bytes, %lld needed (keep_rollout_scratch_bytes)", (long long)roll->scratch_bytes, (long long)rp.total);
    rc = ensure_arena(h, plan.total);
    if (rc) return rc;
    if (graph) {
        const size_t ob = (size_t)B * h->proj_dim * sizeof(float);
        char* st_pix = h->arena + plan.o_pix;
        float* st_out = (float*)(h->arena + plan.o_out);
        HIPCHK(h, hipMemcpyAsync(st_pix, pixels, (size_t)B * tile_vals * px, hipMemcpyDeviceToDevice, s));
        char key[96];
        if (g14) snprintf(key, sizeof key, "img|%lld|%d|%d", (long long)B, pix_dtype, h->precision);     // (keep_classify switches the precision per call, without an option epoch)
        else snprintf(key, sizeof key, "img|%lld|%d|%d|%dx%d", (long long)B, pix_dtype, h->precision, gh, gw);
        rc = graph_run(h, key, s, [&](hipStream_t cs) {
            VitLane L{};
            L.Bc = (int)B; L.pixels = st_pix; L.pix_dtype = pix_dtype; L.out = st_out; L.s = cs;
            L.gh = gh; L.gw = gw; L.ntok = ntok; L.pos = pos;
            L.ws = carve_vit(h, h->arena, L.Bc, plan.split, ntok);
            int r = vit_begin(h, L);
            for (int i = 0; !r && i < h->vit_depth; ++i) r = vit_layer(h, L, i);
            return r ? r : vit_end(h, L);
        });
        if (rc) return rc;
        HIPCHK(h, hipMemcpyAsync(out, st_out, ob, hipMemcpyDeviceToDevice, s));
        return KEEP_OK;
    }
    const int lanes = plan.lanes;
    const int64_t per = plan.per;
    if (lanes > 1) {
        if (!h->ev_fork) HIPCHK(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
        for (int l = 0; l < lanes; ++l) {
            if (!h->aux[l]) HIPCHK(h, hipStreamCreateWithFlags(&h->aux[l], hipStreamNonBlocking));
            if (!h->ev_join[l]) HIPCHK(h, hipEventCreateWithFlags(&h->ev_join[l], hipEventDisableTiming));
        }
        HIPCHK(h, hipEventRecord(h->ev_fork, s));
        for (int l = 0; l < lanes; ++l) HIPCHK(h, hipStreamWaitEvent(h->aux[l], h->ev_fork, 0));
    }
    for (int64_t b0 = 0; b0 < B; b0 += per * lanes) {
        VitLane L[4];
        int nl = 0;
        for (int l = 0; l < lanes; ++l) {
            const int64_t lo = b0 + l * per;
            if (lo >= B) break;
            VitLane& x = L[nl++];
            x.Bc = (int)((B - lo) < per ? (B - lo) : per);
            x.pixels = (const char*)pixels + (size_t)lo * tile_vals * px;
            x.pix_dtype = pix_dtype;
            x.out = out + lo * h->proj_dim;
            x.s = lanes > 1 ? h->aux[l] : s;
            x.gh = gh; x.gw = gw; x.ntok = ntok; x.pos = pos;
            if (tap_out) { x.tap_block = tap_block; x.tap_out = tap_out + lo * h->vit_heads * ntok; }
            if (roll) {
                float* base = (float*)(roll->scratch + (size_t)l * rp.lane);
                x.roll_start = roll->start; x.roll_res = roll->residual; x.roll_out = roll->out + lo * ntok;
                x.roll_r[0] = base; x.roll_r[1] = base + rp.buf / sizeof(float); x.roll_a = base + 2 * (rp.buf / sizeof(float));
            }
            x.ws = carve_vit(h, h->arena + (size_t)l * plan.lane_bytes, x.Bc, plan.split, ntok);
        }
        for (int l = 0; l < nl; ++l) if ((rc = vit_begin(h, L[l]))) return rc;
        for (int i = 0; i < h->vit_depth; ++i)
            for (int l = 0; l < nl; ++l) if ((rc = vit_layer(h, L[l], i))) return rc;
        for (int l = 0; l < nl; ++l) if ((rc = vit_end(h, L[l]))) return rc;
    }
    if (lanes > 1)
        for (int l = 0; l < lanes; ++l) {
            HIPCHK(h, hipEventRecord(h->ev_join[l], h->aux[l]));
            HIPCHK(h, hipStreamWaitEvent(s, h->ev_join[l], 0));
        }
    return KEEP_OK;
}


int similarity_run(keep_handle* h, const float* img, const float* txt, int64_t N, int64_t P, int64_t D, float scale, int mode,
                   void* out, int32_t* argmax_out, hipStream_t s) {
    Scope sc(h, T_SIM, s);
    if (h->tune.sgemv_m > 0 && launch_sim_small(img, txt, (int)N, (int)P, (int)D, scale, mode, out, argmax_out, s) == 0)
        return check_launch(h, "similarity");
    if (h->tune.sgemv_m > 0 && launch_sim_mid(img, txt, (int)N, (int)P, (int)D, scale, mode, out, argmax_out, s) == 0)
        return check_launch(h, "similarity");
    float* logits = (float*)out;
    const bool need_tmp = (mode == KEEP_SIM_ARGMAX && !out) || mode == KEEP_SIM_SOFTMAX_F16 || mode == KEEP_SIM_TOP2SCORE;
    const int nb = (int)((N + 255) / 256);
    if (need_tmp) {
        // scratch lives at the tail end of the arena so that a preceding encode on the same stream
        // (which uses the front) is not disturbed; stream order serialises reuse.
        const size_t bytes = align_up((size_t)N * P * 4) + align_up((size_t)nb * 4) + 256;
        int rc = ensure_arena(h, bytes);
        if (rc) return rc;
        logits = (float*)h->arena;
    }
    SgemmParams g{};
    g.tune = &h->tune;
    g.a = img; g.lda = D; g.b = txt; g.ldb = D; g.out = logits; g.ldo = P; g.bias = nullptr;
    g.M = (int)N; g.N = (int)P; g.K = (int)D; g.act = ACT_NONE;
    g.scale = (mode == KEEP_SIM_RAW || mode == KEEP_SIM_ARGMAX) ? scale : 1.0f;
    if (launch_sgemm_f32(g, s)) return h->fail(KEEP_EUNSUPPORTED, "similarity shape");
    if (mode == KEEP_SIM_ARGMAX) launch_row_argmax(logits, (int)N, (int)P, argmax_out, s);
    else if (mode == KEEP_SIM_SOFTMAX) launch_row_softmax(logits, (int)N, (int)P, scale, logits, s);
    else if (mode == KEEP_SIM_SOFTMAX_F16) launch_row_softmax_f16(logits, (int)N, (int)P, scale, (f16*)out, s);
    else if (mode == KEEP_SIM_TOP2SCORE) {
        float* partial = (float*)(h->arena + align_up((size_t)N * P * 4));
        launch_top2_score(logits, (int)N, (int)P, partial, (float*)out, s);
    }
    return check_launch(h, "similarity");
}


// The options that are one int of the handle (hm) or of its kernel-selection block (tm): keep_set_option and keep_get_option both walk this
// table.  A bool is stored as v ? 1 : 0; anything else must lie in [lo, hi] or the call fails with `msg`.  The options whose domain is a set
// (precision, proj_impl, attn_waves, gemm_impl), the float label_margin, the read-only names and the diagnostics are explicit cases beside it.
enum : unsigned { OPT_REPLAN = 1,       // a prefix shorthand: the whole per-block plan is rewritten from the four of them (a plan set block by block is replaced)
                  OPT_WRITEONLY = 2 };  // keep_get_option answers -1.  TODO: fused_screening and lane_min_tiles can be set but not read back; making them readable changes behaviour
struct Opt { const char* name; int keep_handle::* hm; int KeepTune::* tm; bool is_bool; int lo, hi; const char* msg; unsigned flags; };
constexpr int NO_MAX = 0x7fffffff;
static_assert(SKINNY_MAX_M == 1024, "the gemm_skinny_m message below spells the bound out");
const Opt kOptions[] = {
    {"graphs", &keep_handle::use_graphs, nullptr, true, 0, 0, nullptr, 0},
    {"strict_blocks", &keep_handle::strict_blocks, nullptr, false, 0, NO_MAX, "strict_blocks < 0", 0},
    {"comp_full_blocks", &keep_handle::comp_full_blocks, nullptr, false, 0, NO_MAX, "comp_full_blocks < 0", OPT_REPLAN},
    {"comp_mlp_blocks", &keep_handle::comp_mlp_blocks, nullptr, false, 0, NO_MAX, "comp_mlp_blocks < 0", OPT_REPLAN},
    {"comp_qkv", &keep_handle::comp_qkv, nullptr, true, 0, 0, nullptr, OPT_REPLAN},
    {"comp_qkv_from", &keep_handle::comp_qkv_from, nullptr, false, 0, NO_MAX, "comp_qkv_from < 0", OPT_REPLAN},
    {"comp_min_tiles", &keep_handle::comp_min_tiles, nullptr, false, 24, NO_MAX, "comp_min_tiles must be >= 24 (the compensated product needs the 256x256 kernel)", 0},
    {"fused_screening", &keep_handle::fused_screening, nullptr, false, 0, 2, "fused_screening must be 0..2", OPT_WRITEONLY},
    {"max_tiles", &keep_handle::max_tiles, nullptr, false, 1, NO_MAX, "max_tiles < 1", 0},
    {"max_prompts", &keep_handle::max_prompts, nullptr, false, 1, NO_MAX, "max_prompts < 1", 0},
    {"cls_tail", &keep_handle::cls_tail, nullptr, true, 0, 0, nullptr, 0},
    {"patch_split", &keep_handle::patch_split, nullptr, true, 0, 0, nullptr, 0},
    {"grid_plan", &keep_handle::grid_plan, nullptr, false, 0, 2, "grid_plan must be 0, 1 or 2", 0},
    {"bias_correction", &keep_handle::bias_correction, nullptr, true, 0, 0, nullptr, 0},
    {"streams", &keep_handle::n_streams, nullptr, false, 1, 4, "streams must be 1..4", 0},
    {"lane_min_tiles", &keep_handle::lane_min_tiles, nullptr, false, 6, NO_MAX, "lane_min_tiles must be >= 6", OPT_WRITEONLY},
    {"gemm_persistent", nullptr, &KeepTune::gemm_persistent, false, 0, 1024, "gemm_persistent must be 0..1024", 0},
    {"gemm_splitk_tiles", nullptr, &KeepTune::gemm_splitk_tiles, false, 0, 256, "gemm_splitk_tiles must be 0..256", 0},
    {"sgemv_m", nullptr, &KeepTune::sgemv_m, false, 0, 16, "sgemv_m must be 0..16", 0},
    {"skinny_wide", nullptr, &KeepTune::skinny_wide, true, 0, 0, nullptr, 0},
    {"gemm_skinny_m", nullptr, &KeepTune::gemm_skinny_m, false, 0, SKINNY_MAX_M, "gemm_skinny_m must be 0..1024", 0},
    {"ln_impl", nullptr, &KeepTune::ln_impl, false, 0, 2, "ln_impl must be 0, 1 or 2", 0},
};
const Opt* find_opt(const char* name) {
    for (const Opt& o : kOptions) if (!strcmp(name, o.name)) return &o;
    return nullptr;
}
int& opt_value(keep_handle* h, const Opt& o) { return o.hm ? h->*o.hm : h->tune.*o.tm; }

}  // namespace

// =============================================================================================
extern "C" {

const char* keep_version(void) { return "keep_hip 0.1 (gfx950)"; }

int keep_create(int device_id, keep_handle** out) {
    if (!out) return KEEP_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device_id < 0 || device_id >= n) return KEEP_EHIP;
    DevGuard guard(device_id);
    if (!guard.ok) return KEEP_EHIP;
    keep_handle* h = new keep_handle();
    h->device = device_id;
    if (hipMalloc(&h->err_flag, 4 * sizeof(int)) != hipSuccess) { delete h; return KEEP_ENOMEM; }     // [0] sticky error bits, [2..3] load-time weight statistics
    hipMemset(h->err_flag, 0, 4 * sizeof(int));
    *out = h;
    return KEEP_OK;
}

int keep_destroy(keep_handle* h) {
    if (!h) return KEEP_OK;
    DevGuard guard(h->device);
    hipDeviceSynchronize();
    h->prof_collect();
    for (auto& e : h->pool) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
    for (auto& kv : h->w) { if (kv.second.f32) hipFree(kv.second.f32); if (kv.second.hi) hipFree(kv.second.hi); if (kv.second.lo) hipFree(kv.second.lo);
                            if (kv.second.q) hipFree(kv.second.q); if (kv.second.sc) hipFree(kv.second.sc); }
    if (h->tune.dbg) hipFree(h->tune.dbg);
    for (float* v : h->owned_vecs) hipFree(v);
    h->free_cal();
    h->drop_pos_cache();
    for (auto& l : h->blayers) { if (l.qkv.hi) hipFree(l.qkv.hi); if (l.qkv.lo) hipFree(l.qkv.lo); if (l.qkv_b) hipFree(l.qkv_b); }
    drop_graphs(h);
    if (h->cap_stream) hipStreamDestroy(h->cap_stream);
    if (h->arena) hipFree(h->arena);
    if (h->cls_buf) hipFree(h->cls_buf);
    if (h->err_flag) hipFree(h->err_flag);
    for (int l = 0; l < 4; ++l) { if (h->aux[l]) hipStreamDestroy(h->aux[l]); if (h->ev_join[l]) hipEventDestroy(h->ev_join[l]); }
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    delete h;
    return KEEP_OK;
}

const char* keep_last_error(keep_handle* h) { return h ? h->err.c_str() : "null handle"; }

int keep_set_option(keep_handle* h, const char* name, double value) {
    if (!h || !name) return KEEP_EINVAL;
    const std::string n(name);
    const int v = (int)value;
    ++h->opt_epoch;               // captured graphs bake kernel selection and precision in: drop them lazily (whatever becomes of this call)
    KeepTune& t = h->tune;
    if (const Opt* o = find_opt(name)) {
        if (!o->is_bool && (v < o->lo || v > o->hi)) return h->fail(KEEP_EINVAL, "%s", o->msg);
        opt_value(h, *o) = o->is_bool ? (v ? 1 : 0) : v;
        if (o->flags & OPT_REPLAN) h->plan_from_prefix();
        // (the mean-input biases of the last block were averaged under the other setting: recalibrate)
        if (o->hm == &keep_handle::cls_tail && h->bias_ready && h->cal_cls_tail != h->cls_tail) h->bias_ready = false;
    }
    else if (n == "label_margin") { if (!(value >= 0.0) || value > 2.0) return h->fail(KEEP_EINVAL, "label_margin must be in [0, 2]"); h->label_margin = (float)value; }
    else if (n == "precision") { if (v != KEEP_PREC_FP16 && v != KEEP_PREC_STRICT && v != KEEP_PREC_COMP) return h->fail(KEEP_EINVAL, "precision %d", v); h->precision = v; }
    else if (n == "proj_impl") { if (v != 0 && v != 2128) return h->fail(KEEP_EINVAL, "proj_impl must be 0 or 2128"); h->proj_impl = v; }
    else if (n == "attn_waves") { if (v != 4 && v != 8 && v != 16) return h->fail(KEEP_EINVAL, "attn_waves must be 4, 8 or 16 (16: persistent double-buffered kernel for the image tower)"); t.attn_waves = v; }
    else if (n == "gemm_impl") { if (v != 0 && v != 128 && v != 256) return h->fail(KEEP_EINVAL, "gemm_impl %d (0, 128, 256)", v); t.gemm_impl = v; }
#ifdef KEEP_DIAGNOSTICS
    // result-changing / timing diagnostics exist only in -DKEEP_DIAGNOSTICS builds (tools/gemm_timeline.py, tools/attn_timeline.py)
    else if (n == "gemm_ablate") { t.gemm_ablate = v; }
    else if (n == "gemm_dbg") {
        if (v && !t.dbg) { HIPCHK(h, hipMalloc(&t.dbg, (size_t)65536 * 4 * sizeof(long long))); HIPCHK(h, hipMemset(t.dbg, 0, (size_t)65536 * 4 * sizeof(long long))); }
        if (!v && t.dbg) { hipFree(t.dbg); t.dbg = nullptr; }
    }
#endif
    else return h->fail(KEEP_EINVAL, "unknown option %s", name);
    return KEEP_OK;
}
double keep_get_option(keep_handle* h, const char* name) {
    if (!h || !name) return -1;
    const std::string n(name);
    if (const Opt* o = find_opt(name)) return (o->flags & OPT_WRITEONLY) ? -1 : opt_value(h, *o);
    if (n == "label_margin") return h->label_margin;
    if (n == "precision") return h->precision;
    if (n == "proj_impl") return h->proj_impl;
    if (n == "attn_waves") return h->tune.attn_waves;
    if (n == "gemm_impl") return h->tune.gemm_impl;
    if (n == "plan_custom") return h->plan_custom ? 1 : 0;      // the two read-only names
    if (n == "bias_ready") return h->bias_ready ? 1 : 0;
    if (n == "graph_count") return (double)h->graphs.size();     // read-only as well: the captured graphs the handle holds (stale ones are dropped lazily)
    return -1;
}

int keep_set_block_precision(keep_handle* h, int block, int attn_mode, int mlp_mode) {
    if (!h) return KEEP_EINVAL;
    if (block < 0 || block >= keep_handle::MAX_BLOCKS) return h->fail(KEEP_EINVAL, "block %d outside 0..%d", block, keep_handle::MAX_BLOCKS - 1);
    if (attn_mode > KEEP_ATTN_COMPQKV_PROJ_CLS || mlp_mode > KEEP_MLP_CLS) return h->fail(KEEP_EINVAL, "attn_mode %d (0..5) / mlp_mode %d (0..4); negative = leave", attn_mode, mlp_mode);
    ++h->opt_epoch;               // captured graphs bake the plan in
    if (attn_mode >= 0) h->attn_mode[block] = (unsigned char)attn_mode;
    if (mlp_mode >= 0) h->mlp_mode[block] = (unsigned char)mlp_mode;
    h->plan_custom = true;
    return KEEP_OK;
}
int keep_get_block_precision(keep_handle* h, int block, int* attn_mode, int* mlp_mode) {
    if (!h) return KEEP_EINVAL;
    if (block < 0 || block >= keep_handle::MAX_BLOCKS) return h->fail(KEEP_EINVAL, "block %d outside 0..%d", block, keep_handle::MAX_BLOCKS - 1);
    if (attn_mode) *attn_mode = h->attn_mode[block];
    if (mlp_mode) *mlp_mode = h->mlp_mode[block];
    return KEEP_OK;
}

int keep_reserve(keep_handle* h, int64_t tiles, int64_t prompts, int64_t seq) {
    if (!h || !h->finalized) return h ? h->fail(KEEP_ESTATE, "weights not finalised") : KEEP_EINVAL;
    KEEP_ON_DEVICE(h);
    // (an image call is sized for the 14 x 14 grid and, where it would be graph-replayed, for fp32 pixels: the widest staging)
    size_t need = 0;
    if (tiles > 0 && h->vit_depth) need = vit_plan(h, tiles, 197, (size_t)3 * 224 * 224 * 4, tiles * 197 <= SKINNY_MAX_M).total;
    if (prompts > 0 && seq > 0 && h->bert_layers) need = std::max(need, txt_plan(h, prompts, seq, prompts * seq <= TXT_GRAPH_ROWS).total);
    return ensure_arena(h, need);
}
int64_t keep_workspace_bytes(keep_handle* h) { return h ? (int64_t)h->arena_bytes : 0; }

int keep_encode_image(keep_handle* h, const void* pixels, int pix_dtype, int64_t B, float* out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!h->finalized || !h->vit_depth) return h->fail(KEEP_ESTATE, "image tower not loaded / finalised");
    if (!pixels || !out || B < 0) return h->fail(KEEP_EINVAL, "null pointer or negative batch");
    if (pix_dtype < KEEP_PIX_F32 || pix_dtype > KEEP_PIX_U8_HWC) return h->fail(KEEP_EINVAL, "pixel dtype %d", pix_dtype);
    if (B == 0) return KEEP_OK;
    KEEP_ON_DEVICE(h);
    return encode_image_run(h, pixels, pix_dtype, B, out, (hipStream_t)stream);
}

int keep_encode_image_hw(keep_handle* h, const void* pixels, int pix_dtype, int64_t B, int64_t H, int64_t W, float* out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!h->finalized || !h->vit_depth) return h->fail(KEEP_ESTATE, "image tower not loaded / finalised");
    if (!pixels || !out || B < 0) return h->fail(KEEP_EINVAL, "null pointer or negative batch");
    if (pix_dtype < KEEP_PIX_F32 || pix_dtype > KEEP_PIX_U8_HWC) return h->fail(KEEP_EINVAL, "pixel dtype %d", pix_dtype);
    if (H < 16 || W < 16 || H % 16 || W % 16) return h->fail(KEEP_EINVAL, "image size %lldx%lld: H and W must be positive multiples of 16", (long long)H, (long long)W);
    const int64_t gh = H / 16, gw = W / 16;
    // 32-bit offsets of the kernels: the qkv rows of one tile (launch_attention_long) and a tile's pixels
    if (gh * gw + 1 > 65536) return h->fail(KEEP_EUNSUPPORTED, "image size %lldx%lld: more than 65536 patches", (long long)H, (long long)W);
    if (B == 0) return KEEP_OK;
    KEEP_ON_DEVICE(h);
    // the compensated plan is calibrated on 197-token tiles: outside the band its tolerance was measured in, the grid runs strict
    const int prec = h->precision;
    if (!(gh == 14 && gw == 14) && !h->grid_keeps_plan((int)(gh * gw + 1)) && prec == KEEP_PREC_COMP) h->precision = KEEP_PREC_STRICT;
    const int rc = encode_image_run(h, pixels, pix_dtype, B, out, (hipStream_t)stream, (int)gh, (int)gw);
    h->precision = prec;
    return rc;
}

int keep_encode_image_attn(keep_handle* h, const void* pixels, int pix_dtype, int64_t B, int64_t H, int64_t W, int block, float* out,
                           float* attn_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!h->finalized || !h->vit_depth) return h->fail(KEEP_ESTATE, "image tower not loaded / finalised");
    if (!pixels || !out || !attn_out || B < 0) return h->fail(KEEP_EINVAL, "null pointer or negative batch");
    if (pix_dtype < KEEP_PIX_F32 || pix_dtype > KEEP_PIX_U8_HWC) return h->fail(KEEP_EINVAL, "pixel dtype %d", pix_dtype);
    if (H < 16 || W < 16 || H % 16 || W % 16) return h->fail(KEEP_EINVAL, "image size %lldx%lld: H and W must be positive multiples of 16", (long long)H, (long long)W);
    if (block < -h->vit_depth || block >= h->vit_depth) return h->fail(KEEP_EINVAL, "block %d outside [-%d, %d)", block, h->vit_depth, h->vit_depth);
    const int64_t gh = H / 16, gw = W / 16;
    if (gh * gw + 1 > 65536) return h->fail(KEEP_EUNSUPPORTED, "image size %lldx%lld: more than 65536 patches", (long long)H, (long long)W);
    if (B == 0) return KEEP_OK;
    KEEP_ON_DEVICE(h);
    const int prec = h->precision;                       // the grid rule of keep_encode_image_hw
    if (!(gh == 14 && gw == 14) && !h->grid_keeps_plan((int)(gh * gw + 1)) && prec == KEEP_PREC_COMP) h->precision = KEEP_PREC_STRICT;
    const int rc = encode_image_run(h, pixels, pix_dtype, B, out, (hipStream_t)stream, (int)gh, (int)gw, block < 0 ? block + h->vit_depth : block, attn_out);
    h->precision = prec;
    return rc;
}

// the argument rules keep_encode_image_rollout and keep_rollout_scratch_bytes share with keep_encode_image_attn
static int rollout_grid(keep_handle* h, int64_t B, int64_t H, int64_t W, int64_t* gh, int64_t* gw) {
    if (!h->finalized || !h->vit_depth) return h->fail(KEEP_ESTATE, "image tower not loaded / finalised");
    if (B < 0) return h->fail(KEEP_EINVAL, "negative batch");
    if (H < 16 || W < 16 || H % 16 || W % 16) return h->fail(KEEP_EINVAL, "image size %lldx%lld: H and W must be positive multiples of 16", (long long)H, (long long)W);
    *gh = H / 16; *gw = W / 16;
    if (*gh * *gw + 1 > ROLLOUT_MAX_TOKENS)
        return h->fail(KEEP_EUNSUPPORTED, "image size %lldx%lld: %lld tokens, the rollout covers at most %d", (long long)H, (long long)W, (long long)(*gh * *gw + 1), ROLLOUT_MAX_TOKENS);
    return KEEP_OK;
}

int keep_rollout_scratch_bytes(keep_handle* h, int64_t B, int64_t H, int64_t W, int64_t* bytes) {
    if (!h) return KEEP_EINVAL;
    if (!bytes) return h->fail(KEEP_EINVAL, "null pointer");
    int64_t gh = 0, gw = 0;
    const int rc = rollout_grid(h, B, H, W, &gh, &gw);
    if (rc) return rc;
    const int ntok = (int)(gh * gw + 1);
    *bytes = B ? (int64_t)rollout_scratch(B, ntok, vit_plan(h, B, ntok, 0, false)).total : 0;
    return KEEP_OK;
}

int keep_encode_image_rollout(keep_handle* h, const void* pixels, int pix_dtype, int64_t B, int64_t H, int64_t W, int start_block, float residual,
                              float* out, float* rollout_out, void* scratch, int64_t scratch_bytes, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!h->finalized || !h->vit_depth) return h->fail(KEEP_ESTATE, "image tower not loaded / finalised");
    if (!pixels || !out || !rollout_out || B < 0) return h->fail(KEEP_EINVAL, "null pointer or negative batch");
    if (pix_dtype < KEEP_PIX_F32 || pix_dtype > KEEP_PIX_U8_HWC) return h->fail(KEEP_EINVAL, "pixel dtype %d", pix_dtype);
    if (start_block < -h->vit_depth || start_block >= h->vit_depth)
        return h->fail(KEEP_EINVAL, "start_block %d outside [-%d, %d)", start_block, h->vit_depth, h->vit_depth);
    if (!(residual >= 0.f && residual < 1.f)) return h->fail(KEEP_EINVAL, "residual %g outside [0, 1)", (double)residual);
    int64_t gh = 0, gw = 0;
    int rc = rollout_grid(h, B, H, W, &gh, &gw);
    if (rc) return rc;
    if (B == 0) return KEEP_OK;
    if (!scratch || scratch_bytes < 0) return h->fail(KEEP_EINVAL, "rollout scratch missing (keep_rollout_scratch_bytes)");
    KEEP_ON_DEVICE(h);
    const int prec = h->precision;                       // the grid rule of keep_encode_image_hw
    if (!(gh == 14 && gw == 14) && !h->grid_keeps_plan((int)(gh * gw + 1)) && prec == KEEP_PREC_COMP) h->precision = KEEP_PREC_STRICT;
    const RollArgs roll{start_block < 0 ? start_block + h->vit_depth : start_block, residual, rollout_out, (char*)scratch, scratch_bytes};
    rc = encode_image_run(h, pixels, pix_dtype, B, out, (hipStream_t)stream, (int)gh, (int)gw, -1, nullptr, &roll);
    h->precision = prec;
    return rc;
}

int keep_vit_pos_embed(keep_handle* h, int gh, int gw, float* out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!h->finalized || !h->vit_depth) return h->fail(KEEP_ESTATE, "image tower not loaded / finalised");
    if (!out || gh < 1 || gw < 1 || (int64_t)gh * gw + 1 > 65536) return h->fail(KEEP_EINVAL, "bad position-table arguments (grid %dx%d)", gh, gw);
    KEEP_ON_DEVICE(h);
    const float* pos = nullptr;
    const int rc = vit_pos_table(h, gh, gw, &pos);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(out, pos, (size_t)(gh * gw + 1) * h->vit_D * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return KEEP_OK;
}

int keep_encode_text(keep_handle* h, const int64_t* ids, const int64_t* types, const int64_t* mask, int64_t P, int64_t T,
                     float* out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!h->finalized || !h->bert_layers) return h->fail(KEEP_ESTATE, "text tower not loaded / finalised");
    if (!ids || !out || P < 0 || T < 1) return h->fail(KEEP_EINVAL, "null pointer or bad shape");
    if (T > h->bert_maxpos) return h->fail(KEEP_EINVAL, "sequence length %lld exceeds max_position_embeddings %d", (long long)T, h->bert_maxpos);
    if (T > 512) return h->fail(KEEP_EUNSUPPORTED, "sequence length %lld unsupported (the attention kernels cover 512 tokens, BertModel's max_position_embeddings)", (long long)T);
    if (P == 0) return KEEP_OK;
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    const bool graph = h->use_graphs && !h->prof_mode && P * T <= TXT_GRAPH_ROWS && P <= h->max_prompts;
    const TxtPlan plan = txt_plan(h, P, T, graph);
    const int64_t pc_max = plan.pc;
    int rc = ensure_arena(h, plan.total);
    if (rc) return rc;
    if (graph) {
        // launch-bound size: stage the caller's tensors into fixed buffers and replay the whole tower as one graph
        const size_t nb = (size_t)P * T * sizeof(int64_t), ob = (size_t)P * h->bert_H * sizeof(float);
        int64_t* st_ids = (int64_t*)(h->arena + plan.o_ids);
        int64_t* st_types = (int64_t*)(h->arena + plan.o_types);
        int64_t* st_mask = (int64_t*)(h->arena + plan.o_mask);
        float* st_out = (float*)(h->arena + plan.o_out);
        HIPCHK(h, hipMemcpyAsync(st_ids, ids, nb, hipMemcpyDeviceToDevice, s));
        if (types) HIPCHK(h, hipMemcpyAsync(st_types, types, nb, hipMemcpyDeviceToDevice, s));
        if (mask) HIPCHK(h, hipMemcpyAsync(st_mask, mask, nb, hipMemcpyDeviceToDevice, s));
        char key[96];
        snprintf(key, sizeof key, "txt|%lld|%lld|%d|%d", (long long)P, (long long)T, types ? 1 : 0, mask ? 1 : 0);
        // (the token-range flag is sticky: set by the embedding kernel, cleared only by keep_token_error once the host has seen it --
        // so nothing has to be reset per call, and no memset node is captured: one replayed with a stale value on ROCm 7.2)
        rc = graph_run(h, key, s, [&](hipStream_t cs) {
            return txt_chunk(h, st_ids, types ? st_types : nullptr, mask ? st_mask : nullptr, (int)P, (int)T, st_out, cs);
        });
        if (rc) return rc;
        HIPCHK(h, hipMemcpyAsync(out, st_out, ob, hipMemcpyDeviceToDevice, s));
        return KEEP_OK;
    }
    for (int64_t p0 = 0; p0 < P; p0 += pc_max) {
        const int pc = (int)((P - p0) < pc_max ? (P - p0) : pc_max);
        rc = txt_chunk(h, ids + p0 * T, types ? types + p0 * T : nullptr, mask ? mask + p0 * T : nullptr, pc, (int)T,
                       out + p0 * h->bert_H, s);
        if (rc) return rc;
    }
    return KEEP_OK;
}

/* keep_calibrate_bias (include/keep_hip.h): mean-input compensation of the weight-rounding error, measured on the caller's tiles. */
int keep_calibrate_bias(keep_handle* h, const void* pixels, int pix_dtype, int64_t B, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!h->finalized || !h->vit_depth) return h->fail(KEEP_ESTATE, "image tower not loaded / finalised");
    if (pix_dtype < KEEP_PIX_F32 || pix_dtype > KEEP_PIX_U8_HWC) return h->fail(KEEP_EINVAL, "pixel dtype %d", pix_dtype);
    if (B == 0) { h->bias_ready = false; ++h->opt_epoch; return KEEP_OK; }           // zero tiles: forget the calibration
    if (!pixels || B < 8) return h->fail(KEEP_EINVAL, "bias calibration needs at least 8 tiles");
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    ++h->opt_epoch;
    const int D = h->vit_D, F = h->vit_F;
    const int widths[4] = {D, D, D, F}, outs[4] = {3 * D, D, F, D};
    h->bias_ready = false;
    if ((int)h->cal.size() != h->vit_depth) {
        h->free_cal();
        h->cal.resize(h->vit_depth);
        bool ok = true;
        for (auto& c : h->cal)
            for (int k = 0; k < 4 && ok; ++k)
                ok = hipMalloc(&c.sum[k], widths[k] * sizeof(float)) == hipSuccess && hipMalloc(&c.bias[k], outs[k] * sizeof(float)) == hipSuccess;
        if (!ok) {                                   // never leave a half-allocated table behind: the next call would skip the allocation
            (void)hipGetLastError();
            h->free_cal();
            return h->fail(KEEP_ENOMEM, "bias calibration: out of device memory");
        }
    }
    for (auto& c : h->cal)
        for (int k = 0; k < 4; ++k) {
            if (hipMemsetAsync(c.sum[k], 0, widths[k] * sizeof(float), s) != hipSuccess) { (void)hipGetLastError(); h->free_cal(); return h->fail(KEEP_EHIP, "bias calibration: memset failed"); }
            c.rows[k] = 0;
        }
    h->cal_cls_tail = h->cls_tail;                   // the last block's sites 1-3 average the CLS rows only when cls_tail is on: the biases belong to that setting
    float* scratch = nullptr;
    HIPCHK(h, hipMalloc(&scratch, (size_t)B * h->proj_dim * sizeof(float)));
    // one lane, no graph replay: every site is visited once per sub-batch, on ONE stream, so the sums accumulate in a fixed order
    const int streams_was = h->n_streams, graphs_was = h->use_graphs, prec_was = h->precision;
    h->n_streams = 1; h->use_graphs = 0; h->precision = KEEP_PREC_STRICT; h->capture = true;      // split products: the cleanest activations to average
    int rc = encode_image_run(h, pixels, pix_dtype, B, scratch, s);
    h->n_streams = streams_was; h->use_graphs = graphs_was; h->precision = prec_was; h->capture = false;
    if (!rc) {
        for (int i = 0; i < h->vit_depth && !rc; ++i) {
            const VitBlock& b = h->vblocks[i];
            const WTensor* w[4] = {b.qkv, b.proj, b.fc1, b.fc2};
            const float* bias[4] = {b.qkv_b, b.proj_b, b.fc1_b, b.fc2_b};
            for (int k = 0; k < 4; ++k) {
                if (!w[k]->lo || !(h->cal[i].rows[k] > 0)) { rc = h->fail(KEEP_ESTATE, "block %d site %d was not visited by the calibration encode", i, k); break; }
                launch_bias_mean_corr(w[k]->lo, h->cal[i].sum[k], (float)(1.0 / h->cal[i].rows[k]), bias[k], h->cal[i].bias[k], outs[k], widths[k], s);
            }
        }
    }
    hipError_t e = hipStreamSynchronize(s);
    (void)hipFree(scratch);
    if (rc) return rc;
    HIPCHK(h, e);
    h->bias_ready = true;
    return check_launch(h, "calibrate_bias");
}

int keep_resize_crop_u8(keep_handle* h, const unsigned char* src, int64_t B, int64_t H, int64_t W, const int32_t* xbounds, const int32_t* xweights,
                        int xksize, int64_t out_w, const int32_t* ybounds, const int32_t* yweights, int yksize, int64_t out_h,
                        int64_t crop_left, int64_t crop_top, int64_t size, unsigned char* out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!src || !xbounds || !xweights || !ybounds || !yweights || !out || B < 0 || H < 1 || W < 1 || xksize < 1 || yksize < 1)
        return h->fail(KEEP_EINVAL, "bad resize arguments");
    if (size < 1 || crop_left < 0 || crop_top < 0 || crop_left + size > out_w || crop_top + size > out_h)
        return h->fail(KEEP_EINVAL, "crop window [%lld+%lld, %lld+%lld] outside the resized image %lldx%lld", (long long)crop_left, (long long)size,
                       (long long)crop_top, (long long)size, (long long)out_w, (long long)out_h);
    if (B == 0) return KEEP_OK;
    KEEP_ON_DEVICE(h);
    // the horizontally resized rows live in the arena; whatever runs next on this stream (e.g. the encode of the cropped tiles) is
    // ordered behind the two kernels, so reusing the arena there is safe
    const size_t tmp_bytes = align_up((size_t)B * H * size * 3);
    int rc = ensure_arena(h, tmp_bytes);
    if (rc) return rc;
    launch_resize_crop_u8(src, (int)B, (int)H, (int)W, xbounds, xweights, xksize, (int)crop_left, (int)size, ybounds, yweights, yksize,
                          (int)crop_top, (int)size, (unsigned char*)h->arena, out, (hipStream_t)stream);
    return check_launch(h, "resize_crop_u8");
}

int keep_token_error(keep_handle* h, void* stream) {
    if (!h) return KEEP_EINVAL;
    KEEP_ON_DEVICE(h);
    int flag = 0;
    HIPCHK(h, hipMemcpyAsync(&flag, h->err_flag, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
    if (flag) HIPCHK(h, hipMemsetAsync(h->err_flag, 0, sizeof(int), (hipStream_t)stream));     // seen by the host: re-arm
    return flag & 7;
}

int keep_token_error_async(keep_handle* h, int32_t* host_flag, void* stream) {
    if (!h || !host_flag) return KEEP_EINVAL;
    KEEP_ON_DEVICE(h);
    HIPCHK(h, hipMemcpyAsync(host_flag, h->err_flag, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    return KEEP_OK;
}

int keep_similarity(keep_handle* h, const float* img, const float* txt, int64_t N, int64_t P, int64_t D, float scale, int mode,
                    void* out, int32_t* argmax_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!img || !txt || N < 0 || P < 1 || D < 16 || D % 16) return h->fail(KEEP_EINVAL, "bad similarity arguments");
    if (mode < KEEP_SIM_RAW || mode > KEEP_SIM_TOP2SCORE) return h->fail(KEEP_EINVAL, "similarity mode %d", mode);
    if (mode == KEEP_SIM_ARGMAX && !argmax_out) return h->fail(KEEP_EINVAL, "argmax_out is null");
    if (mode != KEEP_SIM_ARGMAX && !out) return h->fail(KEEP_EINVAL, "out is null");
    if (N == 0) return KEEP_OK;
    KEEP_ON_DEVICE(h);
    return similarity_run(h, img, txt, N, P, D, scale, mode, out, argmax_out, (hipStream_t)stream);
}

/* keep_classify (include/keep_hip.h): labels with the accuracy of the split-product arithmetic at (nearly) the cost of the default one. */
int keep_classify(keep_handle* h, const void* pixels, int pix_dtype, int64_t B, const float* txt, int64_t P, float scale, float margin,
                  float* feats_out, float* sim_out, int32_t* labels_out, int64_t* n_rechecked, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (n_rechecked) *n_rechecked = 0;
    if (!h->finalized || !h->vit_depth) return h->fail(KEEP_ESTATE, "image tower not loaded / finalised");
    if (!pixels || !txt || !labels_out || B < 0 || P < 1) return h->fail(KEEP_EINVAL, "null pointer or bad shape");
    if (pix_dtype < KEEP_PIX_F32 || pix_dtype > KEEP_PIX_U8_HWC) return h->fail(KEEP_EINVAL, "pixel dtype %d", pix_dtype);
    if (!(scale > 0.f)) return h->fail(KEEP_EINVAL, "classify needs scale > 0 (labels are the argmax of scale * cos)");
    if (((uintptr_t)pixels & 15) != 0) return h->fail(KEEP_EINVAL, "pixels must be 16-byte aligned");
    if (B == 0) return KEEP_OK;
    if (B > (1 << 30)) return h->fail(KEEP_EINVAL, "batch too large");
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    const int D = h->proj_dim;
    if (margin < 0.f) margin = h->label_margin;
    const size_t px = pix_dtype == KEEP_PIX_F32 ? 4 : (pix_dtype == KEEP_PIX_U8_HWC ? 1 : 2);
    const size_t tile_bytes = (size_t)3 * 224 * 224 * px;
    const int64_t stage_tiles = B < 256 ? B : 256;                      // flagged tiles are re-encoded in sub-batches of at most 256
    size_t total = 0;
    auto reserve = [&](size_t bytes) { const size_t at = total; total += align_up(bytes); return at; };
    const size_t o_feats = reserve((size_t)B * D * 4), o_sim = reserve((size_t)B * P * 4), o_flags = reserve((size_t)B * 4),
                 o_list = reserve((size_t)B * 4), o_count = reserve(256), o_stage = reserve((size_t)stage_tiles * tile_bytes),
                 o_f2 = reserve((size_t)stage_tiles * D * 4);
    if (total > h->cls_bytes) {
        HIPCHK(h, hipStreamSynchronize(s));
        if (h->cls_buf) HIPCHK(h, hipFree(h->cls_buf));
        h->cls_buf = nullptr; h->cls_bytes = 0;
        HIPCHK(h, hipMalloc(&h->cls_buf, total));
        h->cls_bytes = total;
    }
    char* b = h->cls_buf;
    float* feats = feats_out ? feats_out : (float*)(b + o_feats);
    float* sim = sim_out ? sim_out : (float*)(b + o_sim);
    int* list = (int*)(b + o_list);
    int rc = encode_image_run(h, pixels, pix_dtype, B, feats, s);
    if (rc) return rc;
    rc = similarity_run(h, feats, txt, B, P, D, scale, KEEP_SIM_ARGMAX, sim, labels_out, s);
    if (rc) return rc;
    if (margin == 0.f || P == 1 || h->precision == KEEP_PREC_STRICT) return check_launch(h, "classify");
    launch_top2_margin_flags(sim, (int)B, (int)P, margin * scale, (int*)(b + o_flags), list, (int*)(b + o_count), s);
    int count = 0;
    HIPCHK(h, hipMemcpyAsync(&count, b + o_count, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));                                 // the one host round trip of the call: how many tiles to look at again
    if (n_rechecked) *n_rechecked = count;
    if (count == 0) return check_launch(h, "classify");
    const int saved = h->precision;
    h->precision = KEEP_PREC_STRICT;                                    // per call, no option epoch: graph keys carry the precision
    // equal sub-batches (272 flagged tiles: 136 + 136, not 256 + 16 -- a 16-tile encode is latency-bound and costs a third of a 256-tile one)
    const int64_t parts = (count + stage_tiles - 1) / stage_tiles, per = (count + parts - 1) / parts;
    for (int64_t c0 = 0; c0 < count && !rc; c0 += per) {
        const int n = (int)((count - c0) < per ? (count - c0) : per);
        launch_gather_tiles(pixels, (int64_t)tile_bytes, list + c0, n, b + o_stage, s);
        rc = encode_image_run(h, b + o_stage, pix_dtype, n, (float*)(b + o_f2), s);
        if (!rc) launch_scatter_rows((const float*)(b + o_f2), list + c0, n, D, feats, s);
    }
    h->precision = saved;
    if (rc) return rc;
    rc = similarity_run(h, feats, txt, B, P, D, scale, KEEP_SIM_ARGMAX, sim, labels_out, s);
    if (rc) return rc;
    return check_launch(h, "classify");
}

int keep_prompt_scores(keep_handle* h, const float* feats, const float* bank, int64_t N, int64_t K, int64_t C, int64_t D,
                       float* scores_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!feats || !bank || !scores_out || N < 1 || K < 1 || C < 2 || D < 16 || D % 16) return h->fail(KEEP_EINVAL, "bad prompt_scores arguments");
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    Scope sc(h, T_SIM, s);
    const int64_t KC = K * C;
    if ((C == 2 || C == 4) && D % 128 == 0 && D >= 256 && h->fused_screening) {
        // Fused path: ONE compensated GEMM [N,D] x [D,K*C] whose epilogue takes the per-(tile, classifier)
        // top-2 score in the accumulator registers and sums it over the tile's rows; no logit reaches HBM.
        const int64_t KCp = (KC + 255) / 256 * 256, nslots = (N + 255) / 256 * 2, kpad = KCp / C;
        const bool comp = h->fused_screening == 1;                      // 1: fp16 + MX-fp4 corrections; 2: three fp16 passes
        size_t total = 0;
        auto reserve = [&](size_t bytes) { const size_t at = total; total += align_up(bytes); return at; };     // offsets first: the arena may move
        const size_t o_ahi = reserve(blk_elems(N, D) * sizeof(f16));
        const size_t o_alo = reserve(comp ? 0 : blk_elems(N, D) * sizeof(f16));
        const size_t o_aq = reserve(keepk::q4_data_bytes(N, D));
        const size_t o_asc = reserve(keepk::q4_scale_bytes(N, D));
        const size_t o_whi = reserve(blk_elems(KCp, D) * sizeof(f16));
        const size_t o_wlo = reserve(blk_elems(KCp, D) * sizeof(f16));
        const size_t o_wq = reserve(keepk::q4_data_bytes(KCp, D));
        const size_t o_wsc = reserve(keepk::q4_scale_bytes(KCp, D));
        const size_t o_part = reserve((size_t)nslots * kpad * sizeof(float));
        int rc = ensure_arena(h, total);
        if (rc) return rc;
        char* a = h->arena;
        launch_quant_blockify(feats, (f16*)(a + o_ahi), comp ? nullptr : (f16*)(a + o_alo), (unsigned char*)(a + o_aq), (unsigned char*)(a + o_asc), (int)N, (int)D, s);
        launch_quant_blockify(bank, (f16*)(a + o_whi), (f16*)(a + o_wlo), (unsigned char*)(a + o_wq), (unsigned char*)(a + o_wsc), (int)KC, (int)D, s);
        // (rows KC..KCp of the bank planes are zero-filled by the blockify kernel: their scores land beyond K and are never read)
        GemmParams p{};
        p.tune = &h->tune;
        p.a_hi = (f16*)(a + o_ahi); p.a_lo = (f16*)(a + o_alo); p.w_hi = (f16*)(a + o_whi); p.w_lo = (f16*)(a + o_wlo);
        p.M = (int)N; p.N = (int)KCp; p.K = (int)D; p.nseg = comp ? 1 : 3; p.patches_per_img = 196;
        if (comp) { p.comp = 2; p.a_q = (unsigned char*)(a + o_aq); p.a_sc = (unsigned char*)(a + o_asc); p.w_q = (unsigned char*)(a + o_wq); p.w_sc = (unsigned char*)(a + o_wsc); }
        p.top2_c = (int)C; p.top2_partial = (float*)(a + o_part); p.top2_kpad = (int)kpad;
        h->prof_add_flops(T_SIM, 2.0 * N * (double)KC * D);
        if (launch_gemm_f16(p, EPI_TOP2, s) < 0) return h->fail(KEEP_EUNSUPPORTED, "fused prompt screening launch failed");
        launch_top2_slots_reduce((float*)(a + o_part), (int)nslots, (int)kpad, (int)K, 1.0f / (float)N, scores_out, s);
        return check_launch(h, "prompt_scores");
    }
    int64_t chunk = ((int64_t)256 << 20) / (KC * 4);          // <= 256 MiB of logits alive at a time
    if (chunk < 256) chunk = 256;
    if (chunk > N) chunk = N;
    const int max_rb = 64;
    const size_t b_logits = align_up((size_t)chunk * KC * 4), b_part = align_up((size_t)max_rb * K * 4), b_sums = align_up((size_t)K * 4);
    int rc = ensure_arena(h, b_logits + b_part + b_sums);
    if (rc) return rc;
    float* logits = (float*)h->arena;
    float* partial = (float*)(h->arena + b_logits);
    float* sums = (float*)(h->arena + b_logits + b_part);
    HIPCHK(h, hipMemsetAsync(sums, 0, (size_t)K * 4, s));
    for (int64_t r0 = 0; r0 < N; r0 += chunk) {
        const int64_t n = (N - r0) < chunk ? (N - r0) : chunk;
        SgemmParams g{};
        g.tune = &h->tune;
        g.a = feats + r0 * D; g.lda = D; g.b = bank; g.ldb = D; g.out = logits; g.ldo = KC; g.bias = nullptr;
        g.M = (int)n; g.N = (int)KC; g.K = (int)D; g.scale = 1.0f; g.act = ACT_NONE;
        if (launch_sgemm_f32(g, s)) return h->fail(KEEP_EUNSUPPORTED, "prompt_scores shape");
        launch_group_top2(logits, (int)n, (int)K, (int)C, partial, max_rb, sums, s);
    }
    launch_scale_vec(sums, (int)K, 1.0f / (float)N, scores_out, s);
    return check_launch(h, "prompt_scores");
}

int keep_group_argmax(keep_handle* h, const float* feats, const float* bank, int64_t N, int64_t K, int64_t C, int64_t D,
                      int32_t* labels_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!feats || !bank || !labels_out || N < 1 || K < 1 || C < 1 || D < 16 || D % 16) return h->fail(KEEP_EINVAL, "bad group_argmax arguments");
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    Scope sc(h, T_SIM, s);
    const int64_t KC = K * C;
    int64_t chunk = ((int64_t)256 << 20) / (KC * 4);
    if (chunk < 256) chunk = 256;
    if (chunk > N) chunk = N;
    int rc = ensure_arena(h, align_up((size_t)chunk * KC * 4));
    if (rc) return rc;
    float* logits = (float*)h->arena;
    for (int64_t r0 = 0; r0 < N; r0 += chunk) {
        const int64_t n = (N - r0) < chunk ? (N - r0) : chunk;
        SgemmParams g{};
        g.tune = &h->tune;
        g.a = feats + r0 * D; g.lda = D; g.b = bank; g.ldb = D; g.out = logits; g.ldo = KC; g.bias = nullptr;
        g.M = (int)n; g.N = (int)KC; g.K = (int)D; g.scale = 1.0f; g.act = ACT_NONE;
        if (launch_sgemm_f32(g, s)) return h->fail(KEEP_EUNSUPPORTED, "group_argmax shape");
        // [n][K][C] is contiguous: one argmax per (tile, round) row of C scores, first maximum wins (numpy.argmax)
        launch_row_argmax(logits, (int)(n * K), (int)C, labels_out + r0 * K, s);
    }
    return check_launch(h, "group_argmax");
}

int keep_retrieval_rank(keep_handle* h, const float* txt, const float* img, int64_t P, int64_t N, int64_t D,
                        const int32_t* target, int32_t* rank_out, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!txt || !img || !rank_out || P < 1 || N < 1 || D < 16 || D % 16 || (!target && P > N)) return h->fail(KEEP_EINVAL, "bad retrieval_rank arguments");
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    Scope sc(h, T_SIM, s);
    int64_t chunk = ((int64_t)256 << 20) / (N * 4);
    if (chunk < 64) chunk = 64;
    if (chunk > P) chunk = P;
    int rc = ensure_arena(h, align_up((size_t)chunk * N * 4));
    if (rc) return rc;
    float* sim = (float*)h->arena;
    for (int64_t r0 = 0; r0 < P; r0 += chunk) {
        const int64_t n = (P - r0) < chunk ? (P - r0) : chunk;
        SgemmParams g{};
        g.tune = &h->tune;
        g.a = txt + r0 * D; g.lda = D; g.b = img; g.ldb = D; g.out = sim; g.ldo = N; g.bias = nullptr;
        g.M = (int)n; g.N = (int)N; g.K = (int)D; g.scale = 1.0f; g.act = ACT_NONE;
        if (launch_sgemm_f32(g, s)) return h->fail(KEEP_EUNSUPPORTED, "retrieval_rank shape");
        launch_diag_rank(sim, (int)n, (int)N, target, (int)r0, rank_out, s);
    }
    return check_launch(h, "retrieval_rank");
}

int keep_refine(keep_handle* h, const float* probs, const int64_t* coords, int64_t N, int64_t C, int64_t patch, int overlap,
                float* out_mean, int32_t* is_first, void* stream) {
    if (!h) return KEEP_EINVAL;
    if (!probs || !coords || !out_mean || !is_first || N < 1 || C < 1 || N > (1 << 29)) return h->fail(KEEP_EINVAL, "bad refine arguments");
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    unsigned size = 1024;
    while ((int64_t)size < 2 * N) size <<= 1;
    const size_t b_keys = align_up((size_t)size * 8), b_first = align_up((size_t)size * 4);
    int rc = ensure_arena(h, b_keys + b_first);
    if (rc) return rc;
    launch_refine(probs, (const long long*)coords, (int)N, (int)C, (long long)patch, overlap,
                  (unsigned long long*)h->arena, (int*)(h->arena + b_keys), size, out_mean, (int*)is_first, s);
    return check_launch(h, "refine");
}

int keep_profile_enable(keep_handle* h, const char* tag) {
    if (!h) return KEEP_EINVAL;
    if (!tag) { h->prof_mode = 2; return KEEP_OK; }
    if (!*tag) { h->prof_mode = 0; return KEEP_OK; }
    // one tag, or several separated by commas ("vit.proj,vit.fc2")
    unsigned long long mask = 0;
    std::string names(tag);
    size_t a = 0;
    while (a <= names.size()) {
        const size_t b = names.find(',', a);
        const std::string one = names.substr(a, b == std::string::npos ? std::string::npos : b - a);
        const int t = tag_by_name(one.c_str());
        if (t < 0) return h->fail(KEEP_EINVAL, "unknown profile tag %s", one.c_str());
        mask |= 1ull << t;
        if (b == std::string::npos) break;
        a = b + 1;
    }
    h->prof_mode = 1; h->prof_mask = mask;
    return KEEP_OK;
}
int keep_profile_read(keep_handle* h, const char* tag, double* total_ms, int64_t* launches, double* flops) {
    if (!h || !tag) return KEEP_EINVAL;
    const int t = tag_by_name(tag);
    if (t < 0) return h->fail(KEEP_EINVAL, "unknown profile tag %s", tag);
    DevGuard guard(h->device);
    h->prof_collect();
    if (total_ms) *total_ms = h->prof_ms[t];
    if (launches) *launches = h->prof_n[t];
    if (flops) *flops = h->prof_flops[t];
    return KEEP_OK;
}
int keep_profile_reset(keep_handle* h) {
    if (!h) return KEEP_EINVAL;
    DevGuard guard(h->device);
    h->prof_collect();
    for (int i = 0; i < T_COUNT; ++i) { h->prof_ms[i] = 0; h->prof_n[i] = 0; h->prof_flops[i] = 0; }
    return KEEP_OK;
}

}  // extern "C"
