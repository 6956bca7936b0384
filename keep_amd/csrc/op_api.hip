// Single-operator entry points (keep_op_*) and hardware probes of libkeep_hip: the kernels of the towers, one at a time, on fp32 tensors of the
// caller.  They are the test surface of the kernels (tests/test_ops_gpu.py, tests/test_small_m_gpu.py, tests/test_front_ops_gpu.py): each packs its operands the way the
// towers hold them (hi / lo planes, blk layout, MX-fp4 side planes), fills the launch parameters with the helpers the towers use (handle.h),
// launches, and unpacks the result.  Temporaries are allocated per call; nothing here touches the arena.
#include "handle.h"
#include "quant4.h"

namespace {

// one wave: shader-clock cycles (s_memtime) against the constant 100 MHz counter (s_memrealtime) over ~`spin_us` microseconds
__global__ void clock_probe_kernel(long long* out, int spin_ticks) {
    if (threadIdx.x != 0) return;
    const long long r0 = (long long)__builtin_amdgcn_s_memrealtime(), c0 = (long long)__builtin_readcyclecounter();
    long long r1 = r0;
    while (r1 - r0 < spin_ticks) { __builtin_amdgcn_s_sleep(32); r1 = (long long)__builtin_amdgcn_s_memrealtime(); }
    const long long c1 = (long long)__builtin_readcyclecounter();
    out[0] = c1 - c0; out[1] = r1 - r0;
}

__global__ void f16_planes_to_f32_kernel(const f16* hi, const f16* lo, float* out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = (float)hi[i] + (lo ? (float)lo[i] : 0.f);
}
void planes_to_f32(const f16* hi, const f16* lo, float* out, int64_t n, hipStream_t s) {
    int blocks = (int)((n + 255) / 256); if (blocks > 4096) blocks = 4096; if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(f16_planes_to_f32_kernel, dim3(blocks), dim3(256), 0, s, hi, lo, out, n);
}

// an operand of the op entry points: fp32 [rows][K] of the caller as hi + lo planes in blk layout, with the MX-fp4 side planes where asked for
struct Planes { f16 *hi, *lo; unsigned char *q, *sc; };
Planes alloc_planes(Tmp& t, int64_t rows, int64_t K, bool fp4) {
    Planes p{t.get<f16>(blk_elems(rows, K)), t.get<f16>(blk_elems(rows, K)), nullptr, nullptr};
    if (fp4) { p.q = t.get<unsigned char>(keepk::q4_data_bytes(rows, K)); p.sc = t.get<unsigned char>(keepk::q4_scale_bytes(rows, K)); }
    return p;
}
void with_splitk(GemmParams& p, float* ws) { p.splitk_ws = ws; p.splitk_bytes = SKINNY_WS_BYTES; }   // auto mode may take a split-K path (small or mid-size M), as the towers do
void with_fp4(GemmParams& p, int comp, const Planes& a, const Planes& w) { p.comp = comp; p.a_q = a.q; p.a_sc = a.sc; p.w_q = w.q; p.w_sc = w.sc; }

// The three attention ops are this one body.  What they do differently, as they always did: the plain op takes a key mask and leaves rows it does
// not compute alone (it computes all); the CLS op zero-fills the output (rows past q_rows read back as 0) and the compact [B, D] CLS operand of
// KEEP_ATTN_PROJ_CLS; the long op zero-fills the output, runs the key-blocked kernel and allocates no two-window state.
enum AttnOp { ATTN_OP_PLAIN, ATTN_OP_CLS, ATTN_OP_LONG };
constexpr int ATTN_REFUSED = 1;      // the launcher took no kernel for the shape: the wrapper words its own message
int attention_op(keep_handle* h, AttnOp kind, const char* what, const float* qkv, const int64_t* mask, int64_t B, int64_t T, int heads, int split,
                 int q_rows, float* out, float* cls_out, hipStream_t s) {
    const int64_t M = B * T, D = (int64_t)heads * 64;
    // the towers write the attention output in blk layout when the width allows it (D % 32 == 0 always holds)
    const size_t oe = blk_elems(M, D), ce = blk_elems(B, D);
    Tmp t;
    f16* q_hi = t.get<f16>(M * 3 * D); f16* q_lo = t.get<f16>(M * 3 * D);
    f16* o_hi = t.get<f16>(oe); f16* o_lo = t.get<f16>(oe);
    f16 *c_hi = nullptr, *c_lo = nullptr;
    if (kind == ATTN_OP_CLS) { c_hi = t.get<f16>(ce); c_lo = t.get<f16>(ce); }
    AttnParams a = attn_params(h, q_hi, q_lo, o_hi, split ? o_lo : nullptr, (int)B, (int)T, heads, split, (int)(D / 32));
    a.mask = mask; a.q_rows = q_rows;
    if (kind != ATTN_OP_LONG && split && T > 256) {
        a.part_bytes = (size_t)B * heads * T * ATT_PART_FLOATS * sizeof(float);
        a.part_ws = t.get<float>(a.part_bytes / sizeof(float));
    }
    if (!t.ok) return h->fail(KEEP_ENOMEM, "temp alloc");
    if (kind != ATTN_OP_PLAIN) {
        HIPCHK(h, hipMemsetAsync(o_hi, 0, oe * sizeof(f16), s));
        HIPCHK(h, hipMemsetAsync(o_lo, 0, oe * sizeof(f16), s));
    }
    if (kind == ATTN_OP_CLS) {
        HIPCHK(h, hipMemsetAsync(c_hi, 0, ce * sizeof(f16), s));
        HIPCHK(h, hipMemsetAsync(c_lo, 0, ce * sizeof(f16), s));
    }
    launch_split_f16(qkv, q_hi, q_lo, M * 3 * D, s);
    if (cls_out) { a.cls_hi = c_hi; a.cls_lo = c_lo; }           // (split: launch_attention refuses the planes -- reported, not worked round)
    if (kind == ATTN_OP_LONG ? launch_attention_long(a, s) : launch_attention(a, s)) return ATTN_REFUSED;
    launch_unblockify_f32(o_hi, split ? o_lo : nullptr, out, (int)M, (int)D, s);
    if (cls_out) launch_unblockify_f32(c_hi, c_lo, cls_out, (int)B, (int)D, s);
    HIPCHK(h, hipStreamSynchronize(s));
    return check_launch(h, what);
}

}  // namespace

extern "C" {

int keep_op_linear(keep_handle* h, const float* a, const float* w, const float* bias, const float* ls, const float* resid,
                   int64_t M, int64_t N, int64_t K, int epi, int split, float* out, void* stream) {
    if (!h || !a || !w || !bias || !out) return h ? h->fail(KEEP_EINVAL, "null pointer") : KEEP_EINVAL;
    // K = 32 is a single K step: the LDS-DMA kernels take it, the small-M split-K kernels need two -- so only on a handle that has them switched off
    if (M < 1 || N % 128 || N < 128 || K < 32 || (K < 64 && h->tune.gemm_skinny_m > 0) || K % 32) return h->fail(KEEP_EUNSUPPORTED, "linear needs N%%128==0 and K%%32==0");
    if (epi != EPI_F16 && epi != EPI_GELU_F16 && epi != EPI_RESID_LS && epi != EPI_RESID_F32) return h->fail(KEEP_EINVAL, "epilogue %d", epi);
    if ((epi == EPI_RESID_LS && (!ls || !resid)) || (epi == EPI_RESID_F32 && !resid)) return h->fail(KEEP_EINVAL, "missing ls/resid");
    const bool comp = split == 2 || split == 3;          // 3: the W_lo term only (K >= 512)
    if (comp && (N % 256 || K % 128 || K < (split == 3 ? 512 : 256) || epi == EPI_RESID_F32)) return h->fail(KEEP_EUNSUPPORTED, "compensated linear needs N%%256==0, K%%128==0, K>=256 (512 for the one-term form) and epilogue 0/1/2");
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    Tmp t;
    const Planes A = alloc_planes(t, M, K, comp), W = alloc_planes(t, N, K, comp), O = alloc_planes(t, M, N, false);
    float* ws = t.get<float>(SKINNY_WS_BYTES / 4);
    if (!t.ok) return h->fail(KEEP_ENOMEM, "temp alloc");
    if (comp) { launch_quant_blockify(a, A.hi, A.lo, A.q, A.sc, (int)M, (int)K, s); launch_quant_blockify(w, W.hi, W.lo, W.q, W.sc, (int)N, (int)K, s); }
    else { launch_split_blockify(a, A.hi, A.lo, (int)M, (int)K, s); launch_split_blockify(w, W.hi, W.lo, (int)N, (int)K, s); }
    GemmParams p = gemm_params(h, A.hi, A.lo, W.hi, W.lo, (int)M, (int)N, (int)K, split == 1, bias);
    p.ls = ls;
    if (comp) with_fp4(p, split == 3 ? 1 : 2, A, W);
    with_splitk(p, ws);
    int launch_rc = 0;
    if (epi == EPI_F16 || epi == EPI_GELU_F16) {
        p.out_hi = O.hi; p.out_lo = split ? O.lo : nullptr;       // (split 3 too: what is read back is the accumulator to 2^-22, as the header says, not its fp16 rounding)
        // as in the towers: the GELU output feeds another GEMM (blk layout), the plain one feeds attention (row-major)
        p.out_kt = (epi == EPI_GELU_F16) ? (int)(N / 32) : 0;
        launch_rc = launch_gemm_f16(p, epi, s);
        if (p.out_kt) launch_unblockify_f32(O.hi, p.out_lo, out, (int)M, (int)N, s);
        else planes_to_f32(O.hi, p.out_lo, out, M * N, s);
    } else if (epi == EPI_RESID_LS) {
        HIPCHK(h, hipMemcpyAsync(out, resid, M * N * sizeof(float), hipMemcpyDeviceToDevice, s));
        p.resid = out;
        p.impl_hint = h->proj_impl;      // as the image tower's proj: option proj_impl picks the 256 x 128 kernel where the launcher admits it
        launch_rc = launch_gemm_f16(p, epi, s);
    } else {
        p.resid = const_cast<float*>(resid); p.out_f32 = out;
        launch_rc = launch_gemm_f16(p, epi, s);
    }
    HIPCHK(h, hipStreamSynchronize(s));
    if (launch_rc < 0) return h->fail(KEEP_EUNSUPPORTED, "op_linear: no kernel for this shape / mode");
    return check_launch(h, "op_linear");
}

int keep_op_linear_ln(keep_handle* h, const float* a, const float* w, const float* bias, const float* ls, const float* resid,
                      const float* ln_gamma, const float* ln_beta, float ln_eps, int64_t M, int64_t N, int64_t K, int epi, int split,
                      float* out, float* ln_out, float* ln_hi, int* did_ln, void* stream) {
    if (!h || !a || !w || !bias || !resid || !ln_gamma || !ln_beta || !out || !ln_out || !did_ln) return h ? h->fail(KEEP_EINVAL, "null pointer") : KEEP_EINVAL;
    if (M < 1 || (split != 0 && split != 1)) return h->fail(KEEP_EINVAL, "linear_ln needs M >= 1 and split 0 / 1");
    if (epi != EPI_RESID_LS && epi != EPI_RESID_F32) return h->fail(KEEP_EINVAL, "epilogue %d (linear_ln takes the residual epilogues 2 and 4)", epi);
    if (epi == EPI_RESID_LS && !ls) return h->fail(KEEP_EINVAL, "missing ls");
    if ((N != 768 && N != 1024) || K < 64 || K % 32) return h->fail(KEEP_EUNSUPPORTED, "linear_ln needs N in {768, 1024} and K%%32==0");
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    Tmp t;
    const Planes A = alloc_planes(t, M, K, false), W = alloc_planes(t, N, K, false), Nn = alloc_planes(t, M, N, false);
    float* ws = t.get<float>(SKINNY_WS_BYTES / 4);
    if (!t.ok) return h->fail(KEEP_ENOMEM, "temp alloc");
    launch_split_blockify(a, A.hi, A.lo, (int)M, (int)K, s); launch_split_blockify(w, W.hi, W.lo, (int)N, (int)K, s);
    // as in the towers: the residual stream is updated in place (ViT: resid += ...; BERT: out_f32 == resid), the LayerNorm that follows reads it there
    HIPCHK(h, hipMemcpyAsync(out, resid, M * N * sizeof(float), hipMemcpyDeviceToDevice, s));
    LnParams ln = ln_params(h, out, N, (int)M, (int)N, ln_eps);
    ln.gamma = ln_gamma; ln.beta = ln_beta;
    ln.out_hi = Nn.hi; ln.out_lo = split ? Nn.lo : nullptr; ln.out_kt = (int)(N / 32);
    if (epi == EPI_RESID_F32) { ln.out_f32 = out; ln.out_f32_stride = N; }      // BERT: the normalised row replaces the sum
    GemmParams p = gemm_params(h, A.hi, A.lo, W.hi, W.lo, (int)M, (int)N, (int)K, split != 0, bias);
    p.ls = ls; p.resid = out;
    with_splitk(p, ws);
    if (epi == EPI_RESID_F32) p.out_f32 = out;
    offer_ln(p, ln);
    const int rc = launch_gemm_f16(p, epi, s);
    if (rc < 0) return h->fail(KEEP_EUNSUPPORTED, "op_linear_ln: no kernel for this shape / mode");
    if (!(rc & GEMM_DID_LN) && launch_layernorm(ln, s)) return h->fail(KEEP_EUNSUPPORTED, "layernorm width %lld", (long long)N);
    launch_unblockify_f32(Nn.hi, ln.out_lo, ln_out, (int)M, (int)N, s);
    if (ln_hi) launch_unblockify_f32(Nn.hi, nullptr, ln_hi, (int)M, (int)N, s);      // the hi plane on its own: hi + lo does not tell the two planes apart
    HIPCHK(h, hipStreamSynchronize(s));
    *did_ln = (rc & GEMM_DID_LN) ? 1 : 0;
    return check_launch(h, "op_linear_ln");
}

int keep_op_mlp(keep_handle* h, const float* x, const float* ln_w, const float* ln_b, const float* fc1_w, const float* fc1_b,
                const float* fc2_w, const float* fc2_b, const float* ls, int64_t M, int64_t D, int64_t F, int mode, float* out, void* stream) {
    if (!h || !x || !ln_w || !ln_b || !fc1_w || !fc1_b || !fc2_w || !fc2_b || !ls || !out) return h ? h->fail(KEEP_EINVAL, "null pointer") : KEEP_EINVAL;
    if (M < 1 || (D != 768 && D != 1024) || F % 256 || F < 256 || mode < 0 || mode > 3) return h->fail(KEEP_EUNSUPPORTED, "op_mlp: D in {768, 1024}, F %% 256 == 0, mode 0..3");
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    Tmp t;
    const bool lo = mode == 1, q = mode == 2 || mode == 3;
    const int cmode = mode == 3 ? 1 : 2;                 // GemmParams.comp: the W_lo term only | both terms
    const Planes W1 = alloc_planes(t, F, D, true), W2 = alloc_planes(t, D, F, true), X = alloc_planes(t, M, D, true), H1 = alloc_planes(t, M, F, true);
    float* ws = t.get<float>(SKINNY_WS_BYTES / 4);
    if (!t.ok) return h->fail(KEEP_ENOMEM, "temp alloc");
    launch_quant_blockify(fc1_w, W1.hi, W1.lo, W1.q, W1.sc, (int)F, (int)D, s);
    launch_quant_blockify(fc2_w, W2.hi, W2.lo, W2.q, W2.sc, (int)D, (int)F, s);
    HIPCHK(h, hipMemcpyAsync(out, x, M * D * sizeof(float), hipMemcpyDeviceToDevice, s));
    LnParams ln = ln_params(h, x, D, (int)M, (int)D, 1e-6f);
    ln.gamma = ln_w; ln.beta = ln_b;
    ln.out_hi = X.hi; ln.out_lo = lo ? X.lo : nullptr; ln.out_kt = (int)(D / 32); ln.out_q = q ? X.q : nullptr; ln.out_sc = q ? X.sc : nullptr; ln.out_q_hi_only = mode == 3;
    if (launch_layernorm(ln, s)) return h->fail(KEEP_EUNSUPPORTED, "op_mlp: layernorm");
    GemmParams p = gemm_params(h, X.hi, X.lo, W1.hi, W1.lo, (int)M, (int)F, (int)D, lo, fc1_b);
    with_splitk(p, ws);
    p.out_hi = H1.hi; p.out_lo = lo ? H1.lo : nullptr; p.out_kt = (int)(F / 32);
    if (q) { with_fp4(p, cmode, X, W1); p.out_q = H1.q; p.out_sc = H1.sc; }
    if (launch_gemm_f16(p, EPI_GELU_F16, s) < 0) return h->fail(KEEP_EUNSUPPORTED, "op_mlp: fc1");
    GemmParams r = gemm_params(h, H1.hi, H1.lo, W2.hi, W2.lo, (int)M, (int)D, (int)F, lo, fc2_b);
    with_splitk(r, ws);
    r.ls = ls; r.resid = out;
    if (q) with_fp4(r, cmode, H1, W2);
    if (launch_gemm_f16(r, EPI_RESID_LS, s) < 0) return h->fail(KEEP_EUNSUPPORTED, "op_mlp: fc2");
    HIPCHK(h, hipStreamSynchronize(s));
    return check_launch(h, "op_mlp");
}

int keep_op_mx_planes(keep_handle* h, int producer, int hi_only, const float* x, const float* w, const float* bias, const float* gamma,
                      const float* beta, float eps, int64_t M, int64_t N, int64_t K, int sentinel, float* hi, float* lo, unsigned char* q,
                      unsigned char* sc, void* stream) {
    if (!h || !x || !hi || !q || !sc) return h ? h->fail(KEEP_EINVAL, "null pointer") : KEEP_EINVAL;
    if (producer < KEEP_MX_BLOCKIFY || producer > KEEP_MX_GELU || sentinel < 0 || sentinel > 255) return h->fail(KEEP_EINVAL, "mx_planes: producer %d, sentinel %d", producer, sentinel);
    if (hi_only ? (lo != nullptr || producer == KEEP_MX_BLOCKIFY) : !lo) return h->fail(KEEP_EINVAL, "mx_planes: lo goes with both planes (the blockify kernel always writes both)");
    if (M < 1 || M > (1 << 24)) return h->fail(KEEP_EINVAL, "mx_planes: M %lld", (long long)M);
    if (producer == KEEP_MX_BLOCKIFY && (K < 32 || K % 32 || K > (1 << 20))) return h->fail(KEEP_EUNSUPPORTED, "mx_planes: blockify needs K%%32==0");
    if (producer == KEEP_MX_LAYERNORM && (!gamma || !beta)) return h->fail(KEEP_EINVAL, "missing gamma/beta");
    if (producer == KEEP_MX_LAYERNORM && K != 768 && K != 1024) return h->fail(KEEP_EUNSUPPORTED, "mx_planes: layernorm width %lld", (long long)K);
    if (producer == KEEP_MX_GELU && (!w || !bias)) return h->fail(KEEP_EINVAL, "missing w/bias");
    if (producer == KEEP_MX_GELU && (N < 256 || N % 256 || N > (1 << 20) || K % 128 || K < (hi_only ? 512 : 256) || K > (1 << 20)))
        return h->fail(KEEP_EUNSUPPORTED, "compensated linear needs N%%256==0, K%%128==0, K>=256 (512 for the one-term form)");
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    const int64_t C = producer == KEEP_MX_GELU ? N : K;             // width of the operand the producer writes (the consumer's K)
    Tmp t;
    const Planes P = alloc_planes(t, M, C, true);
    Planes A{}, W{};
    float* ws = nullptr;
    if (producer == KEEP_MX_GELU) { A = alloc_planes(t, M, K, true); W = alloc_planes(t, N, K, true); ws = t.get<float>(SKINNY_WS_BYTES / 4); }
    if (!t.ok) return h->fail(KEEP_ENOMEM, "temp alloc");
    const size_t qb = keepk::q4_data_bytes(M, C), sb = keepk::q4_scale_bytes(M, C);
    HIPCHK(h, hipMemsetAsync(P.q, sentinel, qb, s));
    HIPCHK(h, hipMemsetAsync(P.sc, sentinel, sb, s));
    if (producer == KEEP_MX_BLOCKIFY) {
        launch_quant_blockify(x, P.hi, P.lo, P.q, P.sc, (int)M, (int)K, s);
    } else if (producer == KEEP_MX_LAYERNORM) {
        LnParams ln = ln_params(h, x, K, (int)M, (int)K, eps);
        ln.gamma = gamma; ln.beta = beta;
        // (the towers leave out_lo null in both compensated modes; it is set here so that the lo plane the quantiser saw can be read back)
        ln.out_hi = P.hi; ln.out_lo = hi_only ? nullptr : P.lo; ln.out_kt = (int)(K / 32); ln.out_q = P.q; ln.out_sc = P.sc; ln.out_q_hi_only = hi_only ? 1 : 0;
        if (launch_layernorm(ln, s)) return h->fail(KEEP_EUNSUPPORTED, "mx_planes: layernorm");
    } else {
        launch_quant_blockify(x, A.hi, A.lo, A.q, A.sc, (int)M, (int)K, s);
        launch_quant_blockify(w, W.hi, W.lo, W.q, W.sc, (int)N, (int)K, s);
        GemmParams p = gemm_params(h, A.hi, A.lo, W.hi, W.lo, (int)M, (int)N, (int)K, false, bias);
        with_fp4(p, hi_only ? 1 : 2, A, W);
        with_splitk(p, ws);
        p.out_hi = P.hi; p.out_lo = hi_only ? nullptr : P.lo; p.out_kt = (int)(N / 32); p.out_q = P.q; p.out_sc = P.sc;
        if (launch_gemm_f16(p, EPI_GELU_F16, s) < 0) return h->fail(KEEP_EUNSUPPORTED, "mx_planes: no kernel for this shape / mode");
    }
    launch_unblockify_f32(P.hi, nullptr, hi, (int)M, (int)C, s);
    if (lo) launch_unblockify_f32(P.lo, nullptr, lo, (int)M, (int)C, s);
    HIPCHK(h, hipMemcpyAsync(q, P.q, qb, hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipMemcpyAsync(sc, P.sc, sb, hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return check_launch(h, "op_mx_planes");
}

int keep_op_attention(keep_handle* h, const float* qkv, const int64_t* mask, int64_t B, int64_t T, int heads, int split,
                      float* out, void* stream) {
    if (!h || !qkv || !out || B < 1 || T < 1 || heads < 1) return h ? h->fail(KEEP_EINVAL, "bad attention arguments") : KEEP_EINVAL;
    KEEP_ON_DEVICE(h);
    const int rc = attention_op(h, ATTN_OP_PLAIN, "op_attention", qkv, mask, B, T, heads, split, 0, out, nullptr, (hipStream_t)stream);
    return rc == ATTN_REFUSED ? h->fail(KEEP_EUNSUPPORTED, "sequence length %lld unsupported", (long long)T) : rc;
}

int keep_op_attention_cls(keep_handle* h, const float* qkv, int64_t B, int64_t T, int heads, int split, int q_rows, float* out, float* cls_out,
                          void* stream) {
    if (!h || !qkv || !out || B < 1 || T < 1 || heads < 1 || q_rows < 0) return h ? h->fail(KEEP_EINVAL, "bad attention arguments") : KEEP_EINVAL;
    KEEP_ON_DEVICE(h);
    const int rc = attention_op(h, ATTN_OP_CLS, "op_attention_cls", qkv, nullptr, B, T, heads, split, q_rows, out, cls_out, (hipStream_t)stream);
    return rc == ATTN_REFUSED ? h->fail(KEEP_EUNSUPPORTED, "attention: T %lld%s unsupported", (long long)T, (cls_out && split) ? " with cls_out in split mode" : "") : rc;
}

int keep_op_attention_long(keep_handle* h, const float* qkv, int64_t B, int64_t T, int heads, int split, int q_rows, float* out, void* stream) {
    if (!h || !qkv || !out || B < 1 || T < 1 || heads < 1 || q_rows < 0) return h ? h->fail(KEEP_EINVAL, "bad attention arguments") : KEEP_EINVAL;
    KEEP_ON_DEVICE(h);
    const int rc = attention_op(h, ATTN_OP_LONG, "op_attention_long", qkv, nullptr, B, T, heads, split, q_rows, out, nullptr, (hipStream_t)stream);
    return rc == ATTN_REFUSED ? h->fail(KEEP_EUNSUPPORTED, "long attention: B %lld, T %lld, heads %d unsupported", (long long)B, (long long)T, heads) : rc;
}

int keep_op_attention_cls_probs(keep_handle* h, const float* qkv, int64_t B, int64_t T, int heads, int split, float* out, void* stream) {
    if (!h || !qkv || !out || B < 1 || T < 1 || heads < 1) return h ? h->fail(KEEP_EINVAL, "bad attention arguments") : KEEP_EINVAL;
    if (B > INT32_MAX || T > INT32_MAX || B * T > INT32_MAX) return h->fail(KEEP_EINVAL, "attention_cls_probs: B %lld, T %lld", (long long)B, (long long)T);
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = B * T * 3 * heads * 64;
    Tmp t;
    f16* q_hi = t.get<f16>(n); f16* q_lo = t.get<f16>(n);
    if (!t.ok) return h->fail(KEEP_ENOMEM, "temp alloc");
    launch_split_f16(qkv, q_hi, q_lo, n, s);           // the planes as keep_op_attention makes them
    if (launch_attention_cls_probs(q_hi, split ? q_lo : nullptr, (int)B, (int)T, heads, 0.125f, out, s))
        return h->fail(KEEP_EUNSUPPORTED, "attention_cls_probs: B %lld, T %lld, heads %d unsupported", (long long)B, (long long)T, heads);
    HIPCHK(h, hipStreamSynchronize(s));
    return check_launch(h, "op_attention_cls_probs");
}

int keep_op_attention_rollout_step(keep_handle* h, const float* qkv, int64_t B, int64_t T, int heads, int split, float residual, const float* r_in, int q_rows,
                                   float* r_out, void* stream) {
    if (!h || !qkv || !r_out || B < 1 || T < 1 || heads < 1) return h ? h->fail(KEEP_EINVAL, "bad attention arguments") : KEEP_EINVAL;
    if (q_rows != 0 && q_rows != 1) return h->fail(KEEP_EINVAL, "attention_rollout_step: q_rows %d (0: every row, 1: the CLS row)", q_rows);
    if (!(residual >= 0.f && residual < 1.f)) return h->fail(KEEP_EINVAL, "attention_rollout_step: residual %g outside [0, 1)", (double)residual);
    if (B > INT32_MAX || T > INT32_MAX || B * T > INT32_MAX) return h->fail(KEEP_EINVAL, "attention_rollout_step: B %lld, T %lld", (long long)B, (long long)T);
    if (T > ROLLOUT_MAX_TOKENS) return h->fail(KEEP_EUNSUPPORTED, "attention_rollout_step: T %lld, at most %d", (long long)T, ROLLOUT_MAX_TOKENS);
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = B * T * 3 * heads * 64;
    Tmp t;
    f16* q_hi = t.get<f16>(n); f16* q_lo = t.get<f16>(n);
    float* a_tmp = r_in ? t.get<float>((size_t)B * (q_rows ? 1 : T) * T) : nullptr;
    if (!t.ok) return h->fail(KEEP_ENOMEM, "temp alloc");
    launch_split_f16(qkv, q_hi, q_lo, n, s);           // the planes as keep_op_attention makes them
    if (launch_attention_rollout_step(q_hi, split ? q_lo : nullptr, (int)B, (int)T, heads, 0.125f, residual, r_in, r_out, q_rows, a_tmp, s))
        return h->fail(KEEP_EUNSUPPORTED, "attention_rollout_step: B %lld, T %lld, heads %d unsupported", (long long)B, (long long)T, heads);
    HIPCHK(h, hipStreamSynchronize(s));
    return check_launch(h, "op_attention_rollout_step");
}

// Matrix-pipe ceiling probe (keep_mfma_probe): no memory traffic inside the loop; every wave holds fragments of the caller's data in registers and issues
// independent MFMAs on a 128 x 64 output tile (the pipe's inputs change with every instruction); one 8-wave workgroup per CU, two waves per SIMD, as the GEMM
// kernels run -- and on the MFMA shape their plain K loops are built with (KEEP_MFMA_SHAPE), so the ceiling is the ceiling of the loop in use.
//   32: 2 A x 4 B fragments, 8 v_mfma_f32_32x32x16_f16 per iteration (all (i, j) pairs)
//   16: 8 A x 4 B fragments (6 of the thread's own, 6 of the thread one wave on), 16 v_mfma_f32_16x16x32_f16 per iteration: the same FLOPs per iteration
__global__ __launch_bounds__(512, 2) void mfma_probe_kernel(const f16x8* __restrict__ src, float* __restrict__ sink, int iters) {
    const int t = blockIdx.x * 512 + threadIdx.x;
    float v = 0.f;
#if KEEP_MFMA_SHAPE == 32
    f16x8 a[2], b[4];
#pragma unroll
    for (int i = 0; i < 2; ++i) a[i] = src[(size_t)t * 6 + i];
#pragma unroll
    for (int i = 0; i < 4; ++i) b[i] = src[(size_t)t * 6 + 2 + i];
    f32x16 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i * 4 + j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i], b[j], acc[i * 4 + j], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) v += acc[i][r];
#else
    f16x8 a[8], b[4];
    const int t2 = (t + 64) % ((int)gridDim.x * 512);
#pragma unroll
    for (int i = 0; i < 6; ++i) a[i] = src[(size_t)t * 6 + i];
#pragma unroll
    for (int i = 0; i < 2; ++i) a[6 + i] = src[(size_t)t2 * 6 + i];
#pragma unroll
    for (int i = 0; i < 4; ++i) b[i] = src[(size_t)t2 * 6 + 2 + i];
    f32x4 acc[32];
#pragma unroll
    for (int i = 0; i < 32; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][r] = 0.f;
    // two iterations per trip: all 8 A fragments against all of B = 32 MFMAs, the FLOPs of 16 of the 32 shape (an odd count runs one iteration more)
    for (int it = 0; it < iters; it += 2) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i * 4 + j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(b[j], a[i], acc[i * 4 + j], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 32; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) v += acc[i][r];
#endif
    sink[t] = v;
}

int keep_op_layernorm(keep_handle* h, const float* x, const float* add, const float* gamma, const float* beta, int64_t rows,
                      int64_t D, float eps, float* out, void* stream) {
    if (!h || !x || !gamma || !beta || !out || rows < 1) return h ? h->fail(KEEP_EINVAL, "bad layernorm arguments") : KEEP_EINVAL;
    KEEP_ON_DEVICE(h);
    LnParams p = ln_params(h, x, D, (int)rows, (int)D, eps);
    p.add = add; p.gamma = gamma; p.beta = beta;
    p.out_f32 = out; p.out_f32_stride = D;
    if (launch_layernorm(p, (hipStream_t)stream)) return h->fail(KEEP_EUNSUPPORTED, "layernorm width %lld", (long long)D);
    return check_launch(h, "op_layernorm");
}

int keep_op_sgemm(keep_handle* h, const float* a, const float* b, const float* bias, int64_t M, int64_t N, int64_t K, float scale,
                  int act, float* out, void* stream) {
    if (!h || !a || !b || !out) return h ? h->fail(KEEP_EINVAL, "null pointer") : KEEP_EINVAL;
    KEEP_ON_DEVICE(h);
    SgemmParams g{};
    g.tune = &h->tune;
    g.a = a; g.lda = K; g.b = b; g.ldb = K; g.out = out; g.ldo = N; g.bias = bias; g.M = (int)M; g.N = (int)N; g.K = (int)K;
    g.scale = scale; g.act = act;
    if (launch_sgemm_f32(g, (hipStream_t)stream)) return h->fail(KEEP_EUNSUPPORTED, "sgemm needs K%%16==0");
    return check_launch(h, "op_sgemm");
}

// ---- the towers' front ends, tails and row movers (tests/test_front_ops_gpu.py) ----

int keep_op_patch_embed(keep_handle* h, const void* pixels, int pix_dtype, int64_t B, int64_t gh, int64_t gw, int64_t D, const float* w,
                        const float* bias, const float* cls, const float* pos, int split, int sentinel, float* resid, float* pat_hi, float* pat_lo,
                        void* stream) {
    if (!h || !pixels || !w || !bias || !cls || !pos || !resid || !pat_hi) return h ? h->fail(KEEP_EINVAL, "null pointer") : KEEP_EINVAL;
    if (pix_dtype < PIX_F32 || pix_dtype > PIX_U8_HWC || (split != 0 && split != 1) || sentinel < 0 || sentinel > 255)
        return h->fail(KEEP_EINVAL, "patch_embed: pixel dtype %d, split %d, sentinel %d", pix_dtype, split, sentinel);
    if (B < 1 || gh < 1 || gw < 1 || gh > 1024 || gw > 1024 || B * gh * gw > (1 << 24)) return h->fail(KEEP_EINVAL, "patch_embed: B %lld, grid %lld x %lld", (long long)B, (long long)gh, (long long)gw);
    if (D < 128 || D % 128 || D > (1 << 16)) return h->fail(KEEP_EUNSUPPORTED, "patch_embed needs D%%128==0");
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    const int64_t P = gh * gw, M = B * P, K = 768;
    Tmp t;
    const Planes A = alloc_planes(t, M, K, false), W = alloc_planes(t, D, K, false);
    float* ws = t.get<float>(SKINNY_WS_BYTES / 4);
    if (!t.ok) return h->fail(KEEP_ENOMEM, "temp alloc");
    HIPCHK(h, hipMemsetAsync(A.lo, sentinel, blk_elems(M, K) * sizeof(f16), s));                  // what still holds the sentinel was not written
    HIPCHK(h, hipMemsetAsync(resid, 0xFF, (size_t)B * (P + 1) * D * sizeof(float), s));           // a NaN pattern: a row nobody wrote shows up
    launch_split_blockify(w, W.hi, W.lo, (int)D, (int)K, s);
    // as vit_begin: im2col + the CLS rows, then the GEMM whose epilogue remaps the rows and adds the position table
    launch_im2col(pixels, pix_dtype, (int)B, (int)gh, (int)gw, A.hi, split ? A.lo : nullptr, cls, pos, resid, (int)D, s);
    GemmParams p = gemm_params(h, A.hi, A.lo, W.hi, W.lo, (int)M, (int)D, (int)K, split != 0, bias);
    p.pos = pos; p.patches_per_img = (int)P;
    p.resid = resid;
    with_splitk(p, ws);
    const int rc = launch_gemm_f16(p, EPI_PATCH, s);
    launch_unblockify_f32(A.hi, nullptr, pat_hi, (int)M, (int)K, s);
    if (pat_lo) launch_unblockify_f32(A.lo, nullptr, pat_lo, (int)M, (int)K, s);
    HIPCHK(h, hipStreamSynchronize(s));
    if (rc < 0) return h->fail(KEEP_EUNSUPPORTED, "op_patch_embed: no kernel for this shape / mode");
    return check_launch(h, "op_patch_embed");
}

int keep_op_bert_embed(keep_handle* h, const int64_t* ids, const int64_t* type_ids, const float* wemb, const float* pemb, const float* temb,
                       const float* gamma, const float* beta, float eps, int64_t P, int64_t T, int64_t H, int64_t vocab, int64_t type_vocab,
                       int64_t max_pos, float* resid, float* hi, float* lo, int* err_word, void* stream) {
    if (!h || !ids || !wemb || !pemb || !temb || !gamma || !beta || !resid || !hi || !err_word) return h ? h->fail(KEEP_EINVAL, "null pointer") : KEEP_EINVAL;
    if (H != 256 && H != 768 && H != 1024) return h->fail(KEEP_EUNSUPPORTED, "bert_embed: width %lld", (long long)H);
    if (P < 1 || T < 1 || T > max_pos || P * T > (1 << 24) || vocab < 1 || vocab > INT32_MAX || type_vocab < 1 || type_vocab > INT32_MAX)
        return h->fail(KEEP_EINVAL, "bert_embed: P %lld, T %lld (position table %lld), vocab %lld, types %lld", (long long)P, (long long)T, (long long)max_pos, (long long)vocab, (long long)type_vocab);
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    const int64_t M = P * T;
    Tmp t;
    const Planes X = alloc_planes(t, M, H, false);
    int* err = t.get<int>(1);                            // an error word of this call: the handle's sticky one is left alone
    if (!t.ok) return h->fail(KEEP_ENOMEM, "temp alloc");
    HIPCHK(h, hipMemsetAsync(err, 0, sizeof(int), s));
    launch_bert_embed_ln(ids, type_ids, wemb, pemb, temb, gamma, beta, eps, (int)P, (int)T, (int)H, (int)vocab, (int)type_vocab, resid, X.hi,
                         lo ? X.lo : nullptr, err, s);
    launch_unblockify_f32(X.hi, nullptr, hi, (int)M, (int)H, s);
    if (lo) launch_unblockify_f32(X.lo, nullptr, lo, (int)M, (int)H, s);
    HIPCHK(h, hipMemcpyAsync(err_word, err, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return check_launch(h, "op_bert_embed");
}

int keep_op_layernorm_rows(keep_handle* h, const float* x, int64_t x_stride, const float* gamma, const float* beta, int64_t rows, int64_t D,
                           float eps, float* out, void* stream) {
    if (!h || !x || !gamma || !beta || !out || rows < 1 || rows > INT32_MAX) return h ? h->fail(KEEP_EINVAL, "bad layernorm arguments") : KEEP_EINVAL;
    if (x_stride < D || x_stride % 4) return h->fail(KEEP_EINVAL, "layernorm_rows: row stride %lld (>= D, a multiple of 4)", (long long)x_stride);
    KEEP_ON_DEVICE(h);
    LnParams p = ln_params(h, x, x_stride, (int)rows, (int)D, eps);      // as vit_end: row r of the output is row r * x_stride / D of the token stream
    p.gamma = gamma; p.beta = beta;
    p.out_f32 = out; p.out_f32_stride = D;
    if (launch_layernorm(p, (hipStream_t)stream)) return h->fail(KEEP_EUNSUPPORTED, "layernorm width %lld", (long long)D);
    return check_launch(h, "op_layernorm_rows");
}

int keep_op_sgemm_ld(keep_handle* h, const float* a, int64_t lda, const float* b, int64_t ldb, const float* bias, int64_t M, int64_t N, int64_t K,
                     float scale, int act, float* out, int64_t ldo, void* stream) {
    if (!h || !a || !b || !out) return h ? h->fail(KEEP_EINVAL, "null pointer") : KEEP_EINVAL;
    if (M < 1 || N < 1 || K < 1 || M > INT32_MAX || N > INT32_MAX || K > INT32_MAX || lda < K || ldb < K || ldo < N)
        return h->fail(KEEP_EINVAL, "sgemm_ld: M %lld, N %lld, K %lld, lda %lld, ldb %lld, ldo %lld", (long long)M, (long long)N, (long long)K, (long long)lda, (long long)ldb, (long long)ldo);
    KEEP_ON_DEVICE(h);
    SgemmParams g{};
    g.tune = &h->tune;
    g.a = a; g.lda = lda; g.b = b; g.ldb = ldb; g.out = out; g.ldo = ldo; g.bias = bias; g.M = (int)M; g.N = (int)N; g.K = (int)K;
    g.scale = scale; g.act = act;
    if (launch_sgemm_f32(g, (hipStream_t)stream)) return h->fail(KEEP_EUNSUPPORTED, "sgemm needs K%%16==0, lda%%4==0 and ldb%%4==0");
    return check_launch(h, "op_sgemm_ld");
}

int keep_op_rows(keep_handle* h, int kind, const float* src, int64_t row_stride, int64_t rows, int64_t D, float* dst, void* stream) {
    if (!h || !src || !dst) return h ? h->fail(KEEP_EINVAL, "null pointer") : KEEP_EINVAL;
    if (kind < KEEP_ROWS_GATHER_F32 || kind > KEEP_ROWS_GATHER_BLK) return h->fail(KEEP_EINVAL, "rows: kind %d", kind);
    if (rows < 1 || row_stride < 1 || D < 1 || D > (1 << 20) || rows * row_stride > (1 << 24)) return h->fail(KEEP_EINVAL, "rows: rows %lld, row stride %lld, D %lld", (long long)rows, (long long)row_stride, (long long)D);
    if (kind == KEEP_ROWS_GATHER_BLK && D % 32) return h->fail(KEEP_EUNSUPPORTED, "rows: the blk layout needs D%%32==0");
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    if (kind == KEEP_ROWS_GATHER_F32) {
        launch_gather_rows_f32(src, row_stride * D, dst, (int)rows, (int)D, s);             // as vit_layer: the stride in elements, ntok * D
    } else if (kind == KEEP_ROWS_SCATTER_F32) {
        launch_scatter_rows_f32(src, dst, row_stride * D, (int)rows, (int)D, s);
    } else {
        const int64_t src_rows = rows * row_stride;
        Tmp t;
        f16* s_hi = t.get<f16>(blk_elems(src_rows, D)); f16* d_hi = t.get<f16>(blk_elems(rows, D));
        if (!t.ok) return h->fail(KEEP_ENOMEM, "temp alloc");
        HIPCHK(h, hipMemsetAsync(d_hi, 0, blk_elems(rows, D) * sizeof(f16), s));
        launch_split_blockify(src, s_hi, nullptr, (int)src_rows, (int)D, s);
        launch_gather_rows_blk(s_hi, (int)row_stride, d_hi, (int)rows, (int)D, s);
        launch_unblockify_f32(d_hi, nullptr, dst, (int)rows, (int)D, s);
        HIPCHK(h, hipStreamSynchronize(s));
    }
    return check_launch(h, "op_rows");
}

int keep_op_bias_corr(keep_handle* h, int step, const float* x, int64_t rows, int64_t K, float* col_sum, float inv_rows, const float* bias,
                      float* out, void* stream) {
    if (!h || !x || !col_sum) return h ? h->fail(KEEP_EINVAL, "null pointer") : KEEP_EINVAL;
    if (step != KEEP_BIAS_COL_SUM && step != KEEP_BIAS_MEAN_CORR) return h->fail(KEEP_EINVAL, "bias_corr: step %d", step);
    if (step == KEEP_BIAS_MEAN_CORR && (!bias || !out)) return h->fail(KEEP_EINVAL, "bias_corr: missing bias / out");
    if (rows < 1 || rows > (1 << 24) || K < 32 || K % 32 || K > (1 << 20)) return h->fail(KEEP_EUNSUPPORTED, "bias_corr needs K%%32==0");
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    Tmp t;
    const Planes X = alloc_planes(t, rows, K, false);
    if (!t.ok) return h->fail(KEEP_ENOMEM, "temp alloc");
    launch_split_blockify(x, X.hi, X.lo, (int)rows, (int)K, s);
    if (step == KEEP_BIAS_COL_SUM) launch_blk_col_sum(X.hi, (int)rows, (int)K, col_sum, s);            // adds: what the site's input summed to so far stays
    else launch_bias_mean_corr(X.lo, col_sum, inv_rows, bias, out, (int)rows, (int)K, s);              // x is a GEMM weight [N][K] here: its lo plane
    HIPCHK(h, hipStreamSynchronize(s));
    return check_launch(h, "op_bias_corr");
}

int keep_debug_read(keep_handle* h, void* host_dst, int64_t bytes) {
    if (!h || !host_dst || !h->tune.dbg || bytes > (int64_t)65536 * 4 * 8) return KEEP_EINVAL;      // diagnostics builds only
    KEEP_ON_DEVICE(h);
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipMemcpy(host_dst, h->tune.dbg, bytes, hipMemcpyDeviceToHost));
    return KEEP_OK;
}

int keep_debug_fill_workspace(keep_handle* h, uint32_t word, int64_t* bytes_out, void* stream) {
    if (!h || !bytes_out) return h ? h->fail(KEEP_EINVAL, "null pointer") : KEEP_EINVAL;
    KEEP_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    const size_t na = h->arena ? h->arena_bytes / 4 : 0, nc = h->cls_buf ? h->cls_bytes / 4 : 0;     // whole words: both sizes are multiples of 256
    if (na) HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)h->arena, (int)word, na, s));
    if (nc) HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)h->cls_buf, (int)word, nc, s));
    *bytes_out = (int64_t)(na + nc) * 4;
    return KEEP_OK;
}

int keep_mfma_probe(keep_handle* h, const void* operands_f16, float* sink, int iters, double* flops_out, void* stream) {
    if (!h || !operands_f16 || !sink || iters < 1 || iters > (1 << 24)) return h ? h->fail(KEEP_EINVAL, "bad mfma_probe arguments") : KEEP_EINVAL;
    KEEP_ON_DEVICE(h);
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess || cus < 1) cus = 256;
    hipLaunchKernelGGL(mfma_probe_kernel, dim3(cus), dim3(512), 0, (hipStream_t)stream, (const f16x8*)operands_f16, sink, iters);
    if (flops_out) *flops_out = (double)cus * 8.0 * iters * 8.0 * 2.0 * 32 * 32 * 16;
    return check_launch(h, "mfma_probe");
}

int keep_clock_probe(keep_handle* h, int spin_us, long long* device_out2, void* stream) {
    if (!h || !device_out2 || spin_us < 1 || spin_us > 100000) return h ? h->fail(KEEP_EINVAL, "bad clock_probe arguments") : KEEP_EINVAL;
    KEEP_ON_DEVICE(h);
    hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, device_out2, spin_us * 100);
    return check_launch(h, "clock_probe");
}

int keep_op_l2norm(keep_handle* h, float* x, int64_t rows, int64_t D, void* stream) {
    if (!h || !x || rows < 1 || D < 1) return h ? h->fail(KEEP_EINVAL, "bad l2norm arguments") : KEEP_EINVAL;
    KEEP_ON_DEVICE(h);
    launch_l2norm_rows(x, (int)rows, (int)D, 1e-12f, (hipStream_t)stream);
    return check_launch(h, "op_l2norm");
}

}  // extern "C"
