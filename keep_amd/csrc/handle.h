// The engine handle: what keep_create returns and every extern "C" entry point receives.  engine.hip owns it (arena, towers,
// graphs, options, profile); weights.hip fills its weight store and block tables; op_api.hip borrows its device and kernel
// selection; slide_api.hip uses its device, error text, arena and error flag.  The image tower's precision plan, what it means for a
// block (resolve_block) and the profile tags are block_plan.h, which has no HIP in it.
#pragma once
#include "common.h"
#include "block_plan.h"

#include <cstdarg>
#include <cstdio>
#include <map>
#include <string>
#include <utility>
#include <vector>

#define HIPCHK(h, expr)                                                                      \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) return (h)->fail(KEEP_EHIP, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// Every entry point runs on the handle's device and puts the caller's current device back (torch keeps its own notion of
// the current device per thread; changing it behind its back redirects the caller's next allocation).
struct DevGuard {
    int prev = -1; bool ok = true;
    explicit DevGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess; else prev = -1;
    }
    ~DevGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
#define KEEP_ON_DEVICE(h) DevGuard _guard((h)->device); if (!_guard.ok) return (h)->fail(KEEP_EHIP, "hipSetDevice(%d) failed", (h)->device)

struct WTensor {
    std::vector<int64_t> shape;
    int64_t numel = 0;
    float* f32 = nullptr;     // kept for vectors / embeddings / head / pooler
    f16* hi = nullptr;        // GEMM weights: fp16 planes
    f16* lo = nullptr;
    unsigned char* q = nullptr;   // MX-fp4 side planes of (hi, lo) and their scales (quant4.h); K % 128 == 0 weights only
    unsigned char* sc = nullptr;
    float prescale = 1.f;     // the planes hold prescale * W (a power of two; proj / fc2 of the image tower only): folded back through LayerScale and bias at finalize
};

struct VitBlock {
    const float *n1w, *n1b, *n2w, *n2b, *qkv_b, *proj_b, *fc1_b, *fc2_b, *ls1, *ls2;
    const WTensor *qkv, *proj, *fc1, *fc2;
};
struct BertLayer {
    WTensor qkv;                 // fused [3H, H]
    float* qkv_b = nullptr;      // fused [3H]
    const float *o_b, *ln1w, *ln1b, *i_b, *d_b, *ln2w, *ln2b;
    const WTensor *o, *i, *d;
};

struct keep_handle : PrecisionPlan {      // (the precision plan of the image tower and its queries: block_plan.h)
    int device = 0;
    std::string err;
    std::string load_warnings;   // '\n'-separated notes of keep_load_tensor calls (a weight the fp16 planes resolve poorly); read and cleared by keep_load_warnings
    std::map<std::string, WTensor> w;
    bool finalized = false;

    // dims (filled at finalize)
    int vit_D = 0, vit_heads = 0, vit_F = 0, proj_dim = 0;
    int bert_layers = 0, bert_H = 0, bert_heads = 0, bert_F = 0, bert_vocab = 0, bert_maxpos = 0, bert_types = 0;
    std::vector<VitBlock> vblocks;
    std::vector<BertLayer> blayers;
    std::vector<float*> owned_vecs;   // LayerScale / bias vectors re-derived for pre-scaled weights (finalize_vit)

    // options
    KeepTune tune;               // kernel selection (travels in the launch parameter blocks; nothing is process-wide)
    int fused_screening = 1;     // keep_prompt_scores: 1 fused compensated GEMM (default) | 2 fused 3-pass split GEMM | 0 logits through HBM (any C)
    // keep_classify: tiles whose top-2 cosine margin is below this are re-encoded in KEEP_PREC_STRICT before their label is taken.
    // Default = 2 x the north-star tolerance (both cosines of a pair can move by 1e-4 in opposite directions) + 25 %.
    float label_margin = 2.5e-4f;
    char* cls_buf = nullptr; size_t cls_bytes = 0;     // keep_classify scratch (features, similarity, flags, staged tiles): outside the arena, which the encodes carve
    int max_tiles = 256;
    int max_prompts = 64;
    // Mean-input compensation of the weight-rounding error (keep_calibrate_bias).  A plain fp16 GEMM computes A_hi W_hi^T: the W_lo A_hi term it drops has
    // a part that is the SAME for every row -- W_lo a_mean, a_mean = the mean input row of that GEMM (GELU outputs are positive, LayerNorm outputs carry their
    // bias, attention outputs are averages) -- which no amount of averaging over tiles removes.  It is a constant vector per GEMM: folded into the bias the plain
    // launches use.  cal[i].sum[site]: column sums of the site's input over the calibration tiles; cal[i].bias[site]: bias + W_lo a_mean.
    struct SiteCal { float* sum[4] = {nullptr, nullptr, nullptr, nullptr}; float* bias[4] = {nullptr, nullptr, nullptr, nullptr}; double rows[4] = {0, 0, 0, 0}; };
    std::vector<SiteCal> cal;    // per ViT block; sites: 0 qkv, 1 proj, 2 fc1, 3 fc2
    bool capture = false;        // the running encode accumulates cal[i].sum
    bool bias_ready = false;     // cal[i].bias hold corrected biases for the loaded weights
    int cal_cls_tail = 1;        // cls_tail at the time of the calibration (switching it afterwards invalidates the last block's averages)
    int bias_correction = 1;     // plain launches use them (0: the checkpoint's own biases)
    void free_cal() {
        for (auto& c : cal) for (int k = 0; k < 4; ++k) { if (c.sum[k]) (void)hipFree(c.sum[k]); if (c.bias[k]) (void)hipFree(c.bias[k]); }
        cal.clear(); bias_ready = false;
    }
    // Patch grids other than 14 x 14 (keep_encode_image_hw): the position table resampled to each grid (timm resample_abs_pos_embed), fp32
    // [gh gw + 1][D] on the device, built outside any graph capture on first use; at most POS_CACHE grids, the oldest dropped first (with
    // the captured graphs, which bake its address in); dropped whenever the image tower's weights are (re)finalised or pos_embed is reloaded.
    struct PosSlot { int gh, gw; float* buf; };
    static constexpr int POS_CACHE = 8;
    std::vector<PosSlot> pos_cache;
    void drop_pos_cache() {
        if (pos_cache.empty()) return;
        (void)hipDeviceSynchronize();
        for (auto& e : pos_cache) (void)hipFree(e.buf);
        pos_cache.clear();
        ++opt_epoch;
    }
    // KEEP_PREC_COMP at grids other than 14 x 14: the per-block plan is calibrated on 197-token tiles.  Measured against strict on the bench weights
    // (tools/grid_precision.py, 2 000 tiles per family) it stays at the 224 figure from 257 to 1025 tokens (worst 6.7e-5) and gets
    // worse below 197 (7.1e-5 at 101 tokens, 8.1e-5 at 50).  1 (default): the plan for 197 <= tokens <= 1025, KEEP_PREC_STRICT outside that band;
    // 0: every grid but 14 x 14 strict; 2: the plan at every grid (measurements only).
    int grid_plan = 1;
    bool grid_keeps_plan(int ntok) const { return grid_plan == 2 || (grid_plan == 1 && ntok >= 197 && ntok <= 1025); }
    int patch_split = 1;         // 0: the patch-embedding GEMM as one fp16 pass (experiments; measured in profiles/r05_patch_embed_plain.txt)
    // 2128 (default): the plain proj GEMMs of the image tower on the 256x128 / 4-wave / two-workgroups-per-CU kernel (GemmParams.impl_hint) -- proj is the one GEMM whose
    // tile is 40 % fp32 residual read-modify-write epilogue, and with two workgroups on a CU one's epilogue runs under the other's K loop: -8.5 % on the proj launches,
    // +0.57 % end to end in a six-round rotated A/B on the round-5 plan (profiles/r05_ab_two_workgroups_per_cu.txt; qkv / fc1 / fc2 on the same kernel lose 1.6-4.3 %:
    // 1.5 x the operand bytes per FLOP).  0: the persistent 256x256 kernel.  Bit-identical results either way (same K order per output).
    int proj_impl = 2128;
    // hipGraph replay of launch-bound calls (one prompt / one tile: ~100 dependent kernels of a few us each)
    struct GraphSlot { hipGraphExec_t exec; unsigned long long epoch; char* arena; };
    std::map<std::string, GraphSlot> graphs;
    int use_graphs = 1;
    unsigned long long opt_epoch = 0;   // bumped by keep_set_option / keep_finalize_weights: graphs captured under an older epoch are dropped
    hipStream_t cap_stream = nullptr;
    int lane_min_tiles = 16;     // a lane is only opened for at least this many tiles (32 tiles: 7.09 -> 6.50 ms as 2 x 16; 16 tiles as 2 x 8 loses)
    int n_streams = 2;           // concurrent sub-batches inside keep_encode_image (1 = everything on the caller's stream)
    hipStream_t aux[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[4] = {nullptr, nullptr, nullptr, nullptr};

    // workspace arena
    char* arena = nullptr;
    size_t arena_bytes = 0;
    int* err_flag = nullptr;     // device int, sticky: bit 0 out-of-range token ids, bit 1 non-finite output features (fp16 range exceeded), bit 2 (value 4) a tissue-labelling loop hit its cap

    // profiling
    int prof_mode = 0;           // 0 off, 1 the tags of prof_mask, 2 all
    unsigned long long prof_mask = 0;
    struct Rec { hipEvent_t a, b; int tag; };
    std::vector<Rec> recs;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    double prof_ms[T_COUNT] = {0};
    int64_t prof_n[T_COUNT] = {0};
    double prof_flops[T_COUNT] = {0};      // executed FLOPs (2*M*N*K) of the profiled GEMM launches

    int fail(int code, const char* fmt, ...) {
        char buf[1024];
        va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
        err = buf;
        return code;
    }
    bool prof_on(int tag) const { return prof_mode == 2 || (prof_mode == 1 && ((prof_mask >> tag) & 1ull)); }
    void prof_add_flops(int tag, double f) { if (prof_on(tag)) prof_flops[tag] += f; }
    void prof_begin(int tag, hipStream_t s) {
        if (!prof_on(tag)) return;
        Rec r; r.tag = tag;
        if (!pool.empty()) { r.a = pool.back().first; r.b = pool.back().second; pool.pop_back(); }
        else { hipEventCreate(&r.a); hipEventCreate(&r.b); }
        hipEventRecord(r.a, s);
        recs.push_back(r);
    }
    void prof_end(int tag, hipStream_t s) {
        if (!prof_on(tag)) return;
        hipEventRecord(recs.back().b, s);
    }
    void prof_collect() {
        for (auto& r : recs) {
            hipEventSynchronize(r.b);
            float ms = 0.f;
            hipEventElapsedTime(&ms, r.a, r.b);
            prof_ms[r.tag] += ms; prof_n[r.tag] += 1;
            pool.push_back({r.a, r.b});
        }
        recs.clear();
    }
};

// defined in engine.hip
int ensure_arena(keep_handle* h, size_t bytes);            // grows the workspace arena to at least `bytes` (synchronises the device when it has to)
int check_launch(keep_handle* h, const char* what);        // hipGetLastError after a launch, as a KEEP_E* code with the handle's error text set

inline const WTensor* find_weight(const keep_handle* h, const std::string& k) {
    auto it = h->w.find(k);
    return it == h->w.end() ? nullptr : &it->second;
}

// temp device buffers of one call (op entry points, position-table resample): freed on return; a failed allocation clears `ok`
struct Tmp {
    std::vector<void*> ptrs; bool ok = true;
    ~Tmp() { for (auto p : ptrs) hipFree(p); }
    template <typename T> T* get(size_t n) { void* p = nullptr; if (hipMalloc(&p, (n ? n : 1) * sizeof(T)) != hipSuccess) { ok = false; return nullptr; } ptrs.push_back(p); return (T*)p; }
};

// The launch parameter blocks as the towers and the op entry points fill them: the fields every site sets; outputs and epilogue inputs are the site's own.
inline GemmParams gemm_params(const keep_handle* h, const f16* a_hi, const f16* a_lo, const f16* w_hi, const f16* w_lo, int M, int N, int K, bool split, const float* bias) {
    GemmParams p{};
    p.tune = &h->tune;
    p.a_hi = a_hi; p.a_lo = a_lo; p.w_hi = w_hi; p.w_lo = w_lo;
    p.M = M; p.N = N; p.K = K;
    p.nseg = split ? 3 : 1;
    p.bias = bias;
    p.patches_per_img = 196;
    return p;
}
inline GemmParams gemm_params(const keep_handle* h, const f16* a_hi, const f16* a_lo, const WTensor* w, int M, bool split, const float* bias) {
    return gemm_params(h, a_hi, a_lo, w->hi, w->lo, M, (int)w->shape[0], (int)(w->numel / w->shape[0]), split, bias);
}
inline LnParams ln_params(const keep_handle* h, const float* x, int64_t x_stride, int rows, int D, float eps) {
    LnParams p{};
    p.tune = &h->tune;
    p.x = x; p.x_stride = x_stride; p.rows = rows; p.D = D; p.eps = eps;
    return p;
}
inline AttnParams attn_params(const keep_handle* h, const f16* qkv_hi, const f16* qkv_lo, f16* out_hi, f16* out_lo, int batch, int ntok, int heads, int split, int out_kt) {
    AttnParams a{};
    a.tune = &h->tune;
    a.qkv_hi = qkv_hi; a.qkv_lo = qkv_lo; a.out_hi = out_hi; a.out_lo = out_lo;
    a.batch = batch; a.ntok = ntok; a.heads = heads; a.split = split; a.scale = 0.125f; a.out_kt = out_kt;
    return a;
}
// offer the LayerNorm that follows a residual GEMM to the GEMM itself (taken only on the small-M split-K path)
inline void offer_ln(GemmParams& p, const LnParams& ln) {
    p.ln_gamma = ln.gamma; p.ln_beta = ln.beta; p.ln_eps = ln.eps;
    p.ln_out_hi = ln.out_hi; p.ln_out_lo = ln.out_lo; p.ln_out_f32 = ln.out_f32;
}
