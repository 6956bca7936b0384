// Weight ingestion of libkeep_hip: one state_dict entry at a time into the handle's weight store (release key layout, fp16 hi / lo planes for
// the GEMM weights, MX-fp4 side planes where the compensated product needs them), then keep_finalize_weights, which checks the key set
// (strict semantics) and builds the per-block tables the towers in engine.hip run on.
#include "handle.h"
#include "quant4.h"

#include <cmath>
#include <cstring>

namespace {

bool starts_with(const std::string& s, const char* p) { return s.rfind(p, 0) == 0; }
bool ends_with(const std::string& s, const char* p) {
    const size_t n = strlen(p);
    return s.size() >= n && s.compare(s.size() - n, n, p) == 0;
}

// GEMM weights are stored as fp16 planes only; everything else keeps fp32.
bool is_gemm_weight(const std::string& k) {
    if (k == "visual.patch_embed.proj.weight") return true;
    if (starts_with(k, "visual.blocks.") && ends_with(k, ".weight") &&
        (k.find(".attn.qkv.") != std::string::npos || k.find(".attn.proj.") != std::string::npos ||
         k.find(".mlp.fc1.") != std::string::npos || k.find(".mlp.fc2.") != std::string::npos)) return true;
    if (starts_with(k, "text.encoder.layer.") && ends_with(k, ".weight") && k.find("LayerNorm") == std::string::npos) return true;
    return false;
}

int64_t numel_of(const std::vector<int64_t>& s) { int64_t n = 1; for (auto d : s) n *= d; return n; }

// store one state_dict entry
int store_tensor(keep_handle* h, const std::string& key, const float* dev, const std::vector<int64_t>& shape) {
    WTensor t; t.shape = shape; t.numel = numel_of(shape);
    if (t.numel <= 0) return h->fail(KEEP_EINVAL, "%s: empty tensor", key.c_str());
    if (is_gemm_weight(key)) {
        // fp16 hi/lo planes in blk layout; rows (out features) must fill whole 256-row tiles
        const int64_t n = t.shape[0], k = t.numel / t.shape[0];
        if (n % 256 || k % 32) return h->fail(KEEP_EUNSUPPORTED, "%s: [%lld,%lld] is not tileable (rows %% 256, cols %% 32)", key.c_str(), (long long)n, (long long)k);
        // The GEMM operand planes are fp16: 11 significant bits between 6.1e-5 and 65504, fewer below (subnormals), none above.  A weight whose
        // entries sit above that window cannot be represented at all: refused.  (Below it: see the warning further down.)
        {
            float host[2] = {0.f, 0.f};
            HIPCHK(h, hipMemsetAsync(h->err_flag + 2, 0, 2 * sizeof(float), nullptr));
            launch_weight_stats(dev, t.numel, reinterpret_cast<float*>(h->err_flag + 2), nullptr);
            HIPCHK(h, hipMemcpy(host, h->err_flag + 2, sizeof host, hipMemcpyDeviceToHost));
            const double rms = sqrt((double)host[1] / (double)t.numel);
            if (!(host[0] <= 6.0e4f)) return h->fail(KEEP_EUNSUPPORTED, "%s: max |w| = %g does not fit the fp16 operand planes (65504) or is not finite", key.c_str(), (double)host[0]);
            // A weight far below fp16's normal range (a projection whose magnitude lives in its LayerScale, a pruned or dead layer) still loads, as it
            // does in the reference.  proj / fc2 of the image tower are pre-scaled by a power of two into the window -- exact: their epilogue is
            // ls * (acc + bias), and finalize_vit hands it ls / 2^k and bias * 2^k -- any other weight keeps its entries (they fall into fp16
            // subnormals and lose RELATIVE precision; what such a layer adds to the stream is as small as the layer) and the caller is told.
            if (rms > 0.0 && rms < 2.5e-4) {
                const bool foldable = starts_with(key, "visual.blocks.") && (key.find(".attn.proj.weight") != std::string::npos || key.find(".mlp.fc2.weight") != std::string::npos);
                char buf[512];
                if (foldable && t.numel < (1ll << 31)) {
                    float k2 = exp2f(roundf(log2f(0.02f / (float)rms)));
                    while (host[0] * k2 > 3.0e4f) k2 *= 0.5f;
                    t.prescale = k2;
                    snprintf(buf, sizeof buf, "%s: rms %g is below fp16's normal range; stored as 2^%d * W with LayerScale / bias adjusted (exact)", key.c_str(), rms, (int)log2f(k2));
                } else {
                    snprintf(buf, sizeof buf, "%s: rms %g is below what the fp16 operand planes resolve with 11 bits (entries fall into fp16 subnormals): "
                                              "this layer's products carry fewer significant bits than the error budget assumes", key.c_str(), rms);
                }
                h->load_warnings += (h->load_warnings.empty() ? "" : "\n") + std::string(buf);
            }
        }
        float* scaled = nullptr;
        if (t.prescale != 1.f) {
            HIPCHK(h, hipMalloc(&scaled, t.numel * sizeof(float)));
            launch_scale_vec(dev, (int)t.numel, t.prescale, scaled, nullptr);
            dev = scaled;
        }
        HIPCHK(h, hipMalloc(&t.hi, t.numel * sizeof(f16)));
        HIPCHK(h, hipMalloc(&t.lo, t.numel * sizeof(f16)));
        // the MLP weights of the image tower also get the MX-fp4 side planes of the compensated product (quant4.h)
        if ((key.find(".mlp.fc") != std::string::npos || key.find(".attn.qkv.") != std::string::npos) && starts_with(key, "visual.") && k % 128 == 0 && k >= 256) {
            HIPCHK(h, hipMalloc(&t.q, keepk::q4_data_bytes(n, k)));
            HIPCHK(h, hipMalloc(&t.sc, keepk::q4_scale_bytes(n, k)));
            launch_quant_blockify(dev, t.hi, t.lo, t.q, t.sc, (int)n, (int)k, nullptr);
        } else {
            launch_split_blockify(dev, t.hi, t.lo, (int)n, (int)k, nullptr);
        }
        HIPCHK(h, hipStreamSynchronize(nullptr));
        if (scaled) (void)hipFree(scaled);
    } else {
        const size_t bytes = (size_t)(t.numel > 4 ? t.numel : 4) * sizeof(float);
        HIPCHK(h, hipMalloc(&t.f32, bytes));
        HIPCHK(h, hipMemcpy(t.f32, dev, t.numel * sizeof(float), hipMemcpyDeviceToDevice));
    }
    auto it = h->w.find(key);
    if (it != h->w.end()) {
        if (it->second.f32) hipFree(it->second.f32);
        if (it->second.hi) hipFree(it->second.hi);
        if (it->second.lo) hipFree(it->second.lo);
        if (it->second.q) hipFree(it->second.q);
        if (it->second.sc) hipFree(it->second.sc);
    }
    h->w[key] = t;
    h->finalized = false;
    return KEEP_OK;
}

const float* need_vec(keep_handle* h, const std::string& key, int64_t n, std::string& missing) {
    const WTensor* t = find_weight(h, key);
    if (!t || !t->f32 || t->numel != n) { missing += (missing.empty() ? "" : ", ") + key; return nullptr; }
    return t->f32;
}
const WTensor* need_mat(keep_handle* h, const std::string& key, int64_t n, int64_t k, std::string& missing) {
    const WTensor* t = find_weight(h, key);
    if (!t || !t->hi || t->shape.empty() || t->shape[0] != n || t->numel != n * k) {
        missing += (missing.empty() ? "" : ", ") + key; return nullptr;
    }
    return t;
}

int finalize_vit(keep_handle* h) {
    h->vblocks.clear(); h->vit_depth = 0;
    h->free_cal();               // corrected biases belong to the weights they were calibrated on
    h->drop_pos_cache();         // so do the resampled position tables
    for (float* v : h->owned_vecs) (void)hipFree(v);
    h->owned_vecs.clear();
    const WTensor* pe = find_weight(h, "visual.patch_embed.proj.weight");
    if (!pe) {
        for (auto& kv : h->w) if (starts_with(kv.first, "visual")) return h->fail(KEEP_EKEY, "missing key visual.patch_embed.proj.weight");
        return KEEP_OK;     // image tower not loaded
    }
    if (pe->shape.size() != 4 || pe->shape[1] != 3 || pe->shape[2] != 16 || pe->shape[3] != 16)
        return h->fail(KEEP_EUNSUPPORTED, "patch_embed.proj.weight must be [D,3,16,16]");
    const int64_t D = pe->shape[0];
    if (D % 256 || D > 1024) return h->fail(KEEP_EUNSUPPORTED, "embed dim %lld unsupported", (long long)D);
    int depth = 0;
    while (find_weight(h, "visual.blocks." + std::to_string(depth) + ".attn.qkv.weight")) ++depth;
    if (!depth) return h->fail(KEEP_EKEY, "missing key visual.blocks.0.attn.qkv.weight");
    const WTensor* fc1 = find_weight(h, "visual.blocks.0.mlp.fc1.weight");
    if (!fc1) return h->fail(KEEP_EKEY, "missing key visual.blocks.0.mlp.fc1.weight");
    const int64_t F = fc1->shape[0];
    const WTensor* h0 = find_weight(h, "visual_head.0.weight");
    if (!h0 || h0->shape.size() != 2 || h0->shape[1] != D) return h->fail(KEEP_EKEY, "missing or mis-shaped key visual_head.0.weight");
    const int64_t PJ = h0->shape[0];
    std::string miss;
    need_vec(h, "visual.cls_token", D, miss);
    need_vec(h, "visual.pos_embed", 197 * D, miss);
    need_vec(h, "visual.patch_embed.proj.bias", D, miss);
    need_vec(h, "visual.norm.weight", D, miss);
    need_vec(h, "visual.norm.bias", D, miss);
    need_vec(h, "visual_head.0.bias", PJ, miss);
    need_vec(h, "visual_head.2.weight", PJ * PJ, miss);
    need_vec(h, "visual_head.2.bias", PJ, miss);
    for (int i = 0; i < depth; ++i) {
        const std::string p = "visual.blocks." + std::to_string(i) + ".";
        VitBlock b{};
        b.n1w = need_vec(h, p + "norm1.weight", D, miss); b.n1b = need_vec(h, p + "norm1.bias", D, miss);
        b.n2w = need_vec(h, p + "norm2.weight", D, miss); b.n2b = need_vec(h, p + "norm2.bias", D, miss);
        b.qkv = need_mat(h, p + "attn.qkv.weight", 3 * D, D, miss); b.qkv_b = need_vec(h, p + "attn.qkv.bias", 3 * D, miss);
        b.proj = need_mat(h, p + "attn.proj.weight", D, D, miss);   b.proj_b = need_vec(h, p + "attn.proj.bias", D, miss);
        b.fc1 = need_mat(h, p + "mlp.fc1.weight", F, D, miss);      b.fc1_b = need_vec(h, p + "mlp.fc1.bias", F, miss);
        b.fc2 = need_mat(h, p + "mlp.fc2.weight", D, F, miss);      b.fc2_b = need_vec(h, p + "mlp.fc2.bias", D, miss);
        b.ls1 = need_vec(h, p + "ls1.gamma", D, miss);              b.ls2 = need_vec(h, p + "ls2.gamma", D, miss);
        h->vblocks.push_back(b);
    }
    if (!miss.empty()) return h->fail(KEEP_EKEY, "missing or mis-shaped key(s): %s", miss.c_str());
    if (F % 256 || D % 256 || PJ % 16) return h->fail(KEEP_EUNSUPPORTED, "ViT dims not tileable");
    // pre-scaled proj / fc2 planes (store_tensor): ls * (acc + b) with acc = 2^k * (a . w)  ->  (ls / 2^k) * (acc + 2^k * b), exact in fp32
    auto rescaled = [&](const float* v, float f) -> const float* {
        float* o = nullptr;
        if (hipMalloc(&o, D * sizeof(float)) != hipSuccess) return nullptr;
        launch_scale_vec(v, (int)D, f, o, nullptr);
        h->owned_vecs.push_back(o);
        return o;
    };
    for (auto& b : h->vblocks) {
        if (b.proj->prescale != 1.f) { b.ls1 = rescaled(b.ls1, 1.f / b.proj->prescale); b.proj_b = rescaled(b.proj_b, b.proj->prescale); }
        if (b.fc2->prescale != 1.f) { b.ls2 = rescaled(b.ls2, 1.f / b.fc2->prescale); b.fc2_b = rescaled(b.fc2_b, b.fc2->prescale); }
        if (!b.ls1 || !b.proj_b || !b.ls2 || !b.fc2_b) return h->fail(KEEP_EHIP, "hipMalloc failed for a rescaled LayerScale / bias vector");
    }
    HIPCHK(h, hipStreamSynchronize(nullptr));
    h->vit_has_q = true;
    for (auto& b : h->vblocks) if (!b.fc1->q || !b.fc2->q) h->vit_has_q = false;
    if (depth > keep_handle::MAX_BLOCKS) return h->fail(KEEP_EUNSUPPORTED, "image tower of %d blocks (the per-block precision plan holds %d)", depth, keep_handle::MAX_BLOCKS);
    h->vit_depth = depth; h->vit_D = (int)D; h->vit_heads = (int)(D / 64); h->vit_F = (int)F; h->proj_dim = (int)PJ;
    return KEEP_OK;
}

int finalize_bert(keep_handle* h) {
    for (auto& l : h->blayers) { if (l.qkv.hi) hipFree(l.qkv.hi); if (l.qkv.lo) hipFree(l.qkv.lo); if (l.qkv_b) hipFree(l.qkv_b); }
    h->blayers.clear(); h->bert_layers = 0;
    const WTensor* we = find_weight(h, "text.embeddings.word_embeddings.weight");
    if (!we) {
        for (auto& kv : h->w) if (starts_with(kv.first, "text.")) return h->fail(KEEP_EKEY, "missing key text.embeddings.word_embeddings.weight");
        return KEEP_OK;
    }
    if (we->shape.size() != 2) return h->fail(KEEP_EINVAL, "word_embeddings must be 2-D");
    const int64_t V = we->shape[0], H = we->shape[1];
    if (H != 768 && H != 1024) return h->fail(KEEP_EUNSUPPORTED, "hidden size %lld unsupported (768 or 1024)", (long long)H);
    int L = 0;
    while (find_weight(h, "text.encoder.layer." + std::to_string(L) + ".attention.self.query.weight")) ++L;
    if (!L) return h->fail(KEEP_EKEY, "missing key text.encoder.layer.0.attention.self.query.weight");
    const WTensor* iw = find_weight(h, "text.encoder.layer.0.intermediate.dense.weight");
    if (!iw) return h->fail(KEEP_EKEY, "missing key text.encoder.layer.0.intermediate.dense.weight");
    const int64_t F = iw->shape[0];
    const WTensor* pos = find_weight(h, "text.embeddings.position_embeddings.weight");
    const WTensor* typ = find_weight(h, "text.embeddings.token_type_embeddings.weight");
    if (!pos || !typ || pos->shape.size() != 2 || typ->shape.size() != 2 || pos->shape[1] != H || typ->shape[1] != H)
        return h->fail(KEEP_EKEY, "missing or mis-shaped position/token_type embeddings");
    std::string miss;
    need_vec(h, "text.embeddings.LayerNorm.weight", H, miss);
    need_vec(h, "text.embeddings.LayerNorm.bias", H, miss);
    need_vec(h, "text.pooler.dense.weight", H * H, miss);
    need_vec(h, "text.pooler.dense.bias", H, miss);
    h->blayers.resize(L);
    for (int l = 0; l < L; ++l) {
        const std::string p = "text.encoder.layer." + std::to_string(l) + ".";
        BertLayer& b = h->blayers[l];
        const WTensor* q = need_mat(h, p + "attention.self.query.weight", H, H, miss);
        const WTensor* k = need_mat(h, p + "attention.self.key.weight", H, H, miss);
        const WTensor* v = need_mat(h, p + "attention.self.value.weight", H, H, miss);
        const float* qb = need_vec(h, p + "attention.self.query.bias", H, miss);
        const float* kb = need_vec(h, p + "attention.self.key.bias", H, miss);
        const float* vb = need_vec(h, p + "attention.self.value.bias", H, miss);
        b.o = need_mat(h, p + "attention.output.dense.weight", H, H, miss);
        b.o_b = need_vec(h, p + "attention.output.dense.bias", H, miss);
        b.ln1w = need_vec(h, p + "attention.output.LayerNorm.weight", H, miss);
        b.ln1b = need_vec(h, p + "attention.output.LayerNorm.bias", H, miss);
        b.i = need_mat(h, p + "intermediate.dense.weight", F, H, miss);
        b.i_b = need_vec(h, p + "intermediate.dense.bias", F, miss);
        b.d = need_mat(h, p + "output.dense.weight", H, F, miss);
        b.d_b = need_vec(h, p + "output.dense.bias", H, miss);
        b.ln2w = need_vec(h, p + "output.LayerNorm.weight", H, miss);
        b.ln2b = need_vec(h, p + "output.LayerNorm.bias", H, miss);
        if (!miss.empty()) continue;
        // fuse q|k|v into one [3H,H] weight so the layer needs a single projection GEMM
        b.qkv.shape = {3 * H, H}; b.qkv.numel = 3 * H * H;
        HIPCHK(h, hipMalloc(&b.qkv.hi, b.qkv.numel * sizeof(f16)));
        HIPCHK(h, hipMalloc(&b.qkv.lo, b.qkv.numel * sizeof(f16)));
        HIPCHK(h, hipMalloc(&b.qkv_b, 3 * H * sizeof(float)));
        const WTensor* parts[3] = {q, k, v};
        const float* bparts[3] = {qb, kb, vb};
        for (int j = 0; j < 3; ++j) {
            HIPCHK(h, hipMemcpy(b.qkv.hi + (size_t)j * H * H, parts[j]->hi, H * H * sizeof(f16), hipMemcpyDeviceToDevice));
            HIPCHK(h, hipMemcpy(b.qkv.lo + (size_t)j * H * H, parts[j]->lo, H * H * sizeof(f16), hipMemcpyDeviceToDevice));
            HIPCHK(h, hipMemcpy(b.qkv_b + (size_t)j * H, bparts[j], H * sizeof(float), hipMemcpyDeviceToDevice));
        }
    }
    if (!miss.empty()) { h->blayers.clear(); return h->fail(KEEP_EKEY, "missing or mis-shaped key(s): %s", miss.c_str()); }
    if (F % 256 || H % 256) return h->fail(KEEP_EUNSUPPORTED, "BERT dims not tileable");
    h->bert_layers = L; h->bert_H = (int)H; h->bert_heads = (int)(H / 64); h->bert_F = (int)F;
    h->bert_vocab = (int)V; h->bert_maxpos = (int)pos->shape[0]; h->bert_types = (int)typ->shape[0];
    return KEEP_OK;
}

bool known_key(const std::string& k) {
    static const char* exact[] = {"logit_scale", "visual.cls_token", "visual.pos_embed", "visual.patch_embed.proj.weight",
        "visual.patch_embed.proj.bias", "visual.norm.weight", "visual.norm.bias", "visual_head.0.weight", "visual_head.0.bias",
        "visual_head.2.weight", "visual_head.2.bias", "text.embeddings.word_embeddings.weight",
        "text.embeddings.position_embeddings.weight", "text.embeddings.token_type_embeddings.weight",
        "text.embeddings.LayerNorm.weight", "text.embeddings.LayerNorm.bias", "text.pooler.dense.weight", "text.pooler.dense.bias"};
    for (auto e : exact) if (k == e) return true;
    static const char* vsuf[] = {"norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
        "ls1.gamma", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias", "ls2.gamma"};
    static const char* tsuf[] = {"attention.self.query.weight", "attention.self.query.bias", "attention.self.key.weight",
        "attention.self.key.bias", "attention.self.value.weight", "attention.self.value.bias", "attention.output.dense.weight",
        "attention.output.dense.bias", "attention.output.LayerNorm.weight", "attention.output.LayerNorm.bias",
        "intermediate.dense.weight", "intermediate.dense.bias", "output.dense.weight", "output.dense.bias",
        "output.LayerNorm.weight", "output.LayerNorm.bias"};
    auto layered = [&](const char* prefix, const char* const* suf, size_t n) {
        if (!starts_with(k, prefix)) return false;
        size_t i = strlen(prefix), j = i;
        while (j < k.size() && k[j] >= '0' && k[j] <= '9') ++j;
        if (j == i || j >= k.size() || k[j] != '.') return false;
        const std::string rest = k.substr(j + 1);
        for (size_t q = 0; q < n; ++q) if (rest == suf[q]) return true;
        return false;
    };
    return layered("visual.blocks.", vsuf, sizeof vsuf / sizeof *vsuf) || layered("text.encoder.layer.", tsuf, sizeof tsuf / sizeof *tsuf);
}

}  // namespace

extern "C" {

const char* keep_load_warnings(keep_handle* h) {
    if (!h) return "";
    static thread_local std::string out;
    out.swap(h->load_warnings);
    h->load_warnings.clear();
    return out.c_str();
}

int keep_load_tensor(keep_handle* h, const char* key, const float* data, int ndim, const int64_t* shape, int on_device) {
    if (!h || !key || !data || ndim < 0 || ndim > 8) return KEEP_EINVAL;
    KEEP_ON_DEVICE(h);
    const std::string k(key);
    if (k == "text.embeddings.position_ids" || k == "text.embeddings.token_type_ids") return KEEP_OK;   // buffers of older checkpoints
    if (!known_key(k)) return h->fail(KEEP_EKEY, "unexpected key %s", key);
    if (k == "visual.pos_embed") h->drop_pos_cache();
    std::vector<int64_t> shp(shape, shape + ndim);
    if (ndim == 0) shp = {1};
    const int64_t n = numel_of(shp);
    if (n <= 0) return h->fail(KEEP_EINVAL, "%s: bad shape", key);
    if (on_device) {
        // the repack below runs on the null stream; whatever produced `data` (e.g. a dtype conversion on the caller's
        // stream) must have finished first, and this entry point takes no stream: load time, so simply drain the device
        HIPCHK(h, hipDeviceSynchronize());
        return store_tensor(h, k, data, shp);
    }
    float* tmp = nullptr;
    HIPCHK(h, hipMalloc(&tmp, n * sizeof(float)));
    hipError_t e = hipMemcpy(tmp, data, n * sizeof(float), hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? store_tensor(h, k, tmp, shp) : h->fail(KEEP_EHIP, "H2D copy of %s failed", key);
    hipFree(tmp);
    return rc;
}

int keep_finalize_weights(keep_handle* h) {
    if (!h) return KEEP_EINVAL;
    KEEP_ON_DEVICE(h);
    ++h->opt_epoch;
    int rc = finalize_vit(h);
    if (rc) return rc;
    rc = finalize_bert(h);
    if (rc) return rc;
    if (!h->vit_depth && !h->bert_layers) return h->fail(KEEP_EKEY, "no tower loaded");
    HIPCHK(h, hipDeviceSynchronize());
    h->finalized = true;
    return KEEP_OK;
}

int keep_vit_depth(keep_handle* h) { return h && h->finalized ? h->vit_depth : 0; }
int keep_bert_layers(keep_handle* h) { return h && h->finalized ? h->bert_layers : 0; }

}  // extern "C"
