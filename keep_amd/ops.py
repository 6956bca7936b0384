"""Single-operator wrappers over the C ABI (keep_op_* in include/keep_hip.h).

Used by the parity tests to check each HIP kernel against a torch fp32/fp64 reference of the same
operator; not needed by users of ``KEEPModel``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from .model import _PIX, _ptr, _stream

EPI_F16, EPI_GELU_F16, EPI_RESID_LS, EPI_RESID_F32 = 0, 1, 2, 4
MX_BLOCKIFY, MX_LAYERNORM, MX_GELU = 0, 1, 2             # keep_op_mx_planes: which producer of the MX-fp4 side planes runs
ROWS_GATHER_F32, ROWS_SCATTER_F32, ROWS_GATHER_BLK = 0, 1, 2   # keep_op_rows
BIAS_COL_SUM, BIAS_MEAN_CORR = 0, 1                      # keep_op_bias_corr


class Ops:
    def __init__(self, device="cuda"):
        lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.KeepHipError("no GPU visible: keep_amd has no CPU execution path")
        device = torch.device(device)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        self._h = C.c_void_p(0)
        rc = lib.keep_create(idx, C.byref(self._h))
        if rc:
            raise _lib.KeepHipError(f"keep_create failed ({rc})")

    def __del__(self):
        try:
            if self._h.value:
                _lib.load().keep_destroy(self._h)
        except Exception:
            pass

    def set_option(self, name: str, value: float):
        _lib.check(self._h, _lib.load().keep_set_option(self._h, name.encode(), float(value)), name)

    def debug_timeline(self, nblocks: int):
        """[nblocks,4] int64 shader-clock stamps of the last GEMM launch (needs option gemm_dbg=1)."""
        import numpy as np
        buf = np.zeros((nblocks, 4), dtype=np.int64)
        rc = _lib.load().keep_debug_read(self._h, buf.ctypes.data_as(C.c_void_p), buf.nbytes)
        _lib.check(self._h, rc, "debug_read")
        return buf

    def _f(self, t: Optional[torch.Tensor]):
        return None if t is None else t.to(self.device, torch.float32).contiguous()

    def linear(self, a, w, bias, epi=EPI_F16, split=False, ls=None, resid=None):
        a, w, bias, ls, resid = map(self._f, (a, w, bias, ls, resid))
        M, K = a.shape
        N = w.shape[0]
        out = torch.empty((M, N), dtype=torch.float32, device=self.device)
        rc = _lib.load().keep_op_linear(self._h, _ptr(a), _ptr(w), _ptr(bias), _ptr(ls), _ptr(resid), M, N, K, epi,
                                        int(split), _ptr(out), _stream(self.device))
        _lib.check(self._h, rc, "op_linear")
        return out

    def linear_ln(self, a, w, bias, ln_gamma, ln_beta, ln_eps, epi=EPI_RESID_LS, split=False, ls=None, resid=None, hi=False):
        """A residual linear (epi 2 / 4) with the LayerNorm that follows offered to the GEMM, as the towers do -> (out, ln_out, did_ln).
        ln_out is read back from the fp16 operand planes (hi + lo when split, else hi); did_ln is 1 when the GEMM's reduce did the LayerNorm.
        hi=True: -> (out, ln_out, did_ln, ln_hi) with the hi plane on its own."""
        a, w, bias, ls, resid, ln_gamma, ln_beta = map(self._f, (a, w, bias, ls, resid, ln_gamma, ln_beta))
        M, K = a.shape
        N = w.shape[0]
        out = torch.empty((M, N), dtype=torch.float32, device=self.device)
        ln_out = torch.empty((M, N), dtype=torch.float32, device=self.device)
        ln_hi = torch.empty((M, N), dtype=torch.float32, device=self.device) if hi else None
        did = C.c_int(-1)
        rc = _lib.load().keep_op_linear_ln(self._h, _ptr(a), _ptr(w), _ptr(bias), _ptr(ls), _ptr(resid), _ptr(ln_gamma), _ptr(ln_beta),
                                           float(ln_eps), M, N, K, int(epi), int(split), _ptr(out), _ptr(ln_out), _ptr(ln_hi), C.byref(did),
                                           _stream(self.device))
        _lib.check(self._h, rc, "op_linear_ln")
        return (out, ln_out, did.value, ln_hi) if hi else (out, ln_out, did.value)

    def mlp(self, x, ln_w, ln_b, fc1_w, fc1_b, fc2_w, fc2_b, ls, mode=0):
        """x + ls * fc2(gelu(fc1(layernorm(x)))) through the tower's kernels; mode 0 fp16, 1 split, 2 compensated."""
        x, ln_w, ln_b, fc1_w, fc1_b, fc2_w, fc2_b, ls = map(self._f, (x, ln_w, ln_b, fc1_w, fc1_b, fc2_w, fc2_b, ls))
        M, D = x.shape
        F = fc1_w.shape[0]
        out = torch.empty_like(x)
        rc = _lib.load().keep_op_mlp(self._h, _ptr(x), _ptr(ln_w), _ptr(ln_b), _ptr(fc1_w), _ptr(fc1_b), _ptr(fc2_w), _ptr(fc2_b),
                                     _ptr(ls), M, D, F, int(mode), _ptr(out), _stream(self.device))
        _lib.check(self._h, rc, "op_mlp")
        return out

    def mx_planes(self, producer, x, w=None, bias=None, gamma=None, beta=None, eps=1e-6, hi_only=False, sentinel=0xFF):
        """One producer of the MX-fp4 side planes on its own (MX_BLOCKIFY: x [M,K]; MX_LAYERNORM: x, gamma, beta, eps; MX_GELU: the compensated
        GEMM gelu(x @ w^T + bias)) -> (hi, lo, q, sc): the fp16 planes it wrote as fp32 [M,C] (lo None with hi_only) and the raw e2m1 / E8M0 bytes
        in device layout, padding rows included, every byte preset to `sentinel`."""
        x, w, bias, gamma, beta = map(self._f, (x, w, bias, gamma, beta))
        M, K = x.shape
        N = w.shape[0] if w is not None else 0
        Cw = N if producer == MX_GELU else K
        Mp = (M + 255) // 256 * 256
        hi = torch.empty((M, Cw), dtype=torch.float32, device=self.device)
        lo = None if hi_only else torch.empty((M, Cw), dtype=torch.float32, device=self.device)
        q = torch.empty(Mp * Cw, dtype=torch.uint8, device=self.device)
        sc = torch.empty(Mp * (Cw // 32) * 2, dtype=torch.uint8, device=self.device)
        rc = _lib.load().keep_op_mx_planes(self._h, int(producer), int(hi_only), _ptr(x), _ptr(w), _ptr(bias), _ptr(gamma), _ptr(beta), float(eps),
                                           M, N, K, int(sentinel), _ptr(hi), _ptr(lo), _ptr(q), _ptr(sc), _stream(self.device))
        _lib.check(self._h, rc, "op_mx_planes")
        return hi, lo, q, sc

    def attention(self, qkv, B, T, heads, mask=None, split=False):
        qkv = self._f(qkv)
        m = None if mask is None else mask.to(self.device, torch.int64).contiguous()
        out = torch.empty((B * T, heads * 64), dtype=torch.float32, device=self.device)
        rc = _lib.load().keep_op_attention(self._h, _ptr(qkv), _ptr(m), B, T, heads, int(split), _ptr(out),
                                           _stream(self.device))
        _lib.check(self._h, rc, "op_attention")
        return out

    def attention_cls(self, qkv, B, T, heads, split=False, q_rows=0, cls=False):
        """Unmasked attention with the image tower's CLS features: q_rows > 0 computes only the first q_rows queries of every sequence
        (other rows 0); cls=True also returns the [B, heads*64] CLS rows as hi + lo of the fp32 accumulators -> out, or (out, cls_out)."""
        qkv = self._f(qkv)
        out = torch.empty((B * T, heads * 64), dtype=torch.float32, device=self.device)
        cls_out = torch.empty((B, heads * 64), dtype=torch.float32, device=self.device) if cls else None
        rc = _lib.load().keep_op_attention_cls(self._h, _ptr(qkv), B, T, heads, int(split), int(q_rows), _ptr(out), _ptr(cls_out),
                                               _stream(self.device))
        _lib.check(self._h, rc, "op_attention_cls")
        return (out, cls_out) if cls else out

    def attention_long(self, qkv, B, T, heads, split=False, q_rows=0):
        """The key-blocked attention kernel the image tower runs beyond 512 tokens (any T; no key mask)."""
        qkv = self._f(qkv)
        out = torch.empty((B * T, heads * 64), dtype=torch.float32, device=self.device)
        rc = _lib.load().keep_op_attention_long(self._h, _ptr(qkv), B, T, heads, int(split), int(q_rows), _ptr(out),
                                                _stream(self.device))
        _lib.check(self._h, rc, "op_attention_long")
        return out

    def attention_cls_probs(self, qkv, B, T, heads, split=False):
        """The CLS query's attention probabilities, fp32 [B, heads, T]: softmax over the keys of q_{b,h,0} . k_{b,h,k} / 8 on the fp16 planes
        of qkv (split: hi + lo), fp32 products and sums; any T >= 1."""
        qkv = self._f(qkv)
        out = torch.empty((B, heads, T), dtype=torch.float32, device=self.device)
        rc = _lib.load().keep_op_attention_cls_probs(self._h, _ptr(qkv), B, T, heads, int(split), _ptr(out), _stream(self.device))
        _lib.check(self._h, rc, "op_attention_cls_probs")
        return out

    def attention_rollout_step(self, qkv, B, T, heads, split=False, residual=0.5, r_in=None, q_rows=0):
        """One block's step of the attention rollout: with A the head mean of softmax(q k^T / 8) over all T query rows (fp16
        planes of qkv, split: hi + lo products; fp32 sums) and At = (1 - residual) A + residual I, returns At @ r_in in fp32, or At when r_in is None
        -> fp32 [B, T, T]; q_rows=1: the CLS row alone, [B, 1, T].  r_in: fp32 [B, T, T].  1 <= T <= keep_amd.attention.ROLLOUT_MAX_TOKENS."""
        qkv = self._f(qkv)
        if r_in is not None:
            r_in = self._f(r_in)
            if tuple(r_in.shape) != (B, T, T):
                raise ValueError(f"r_in must be [B, T, T] = {(B, T, T)}, got {tuple(r_in.shape)}")
        out = torch.empty((B, 1 if q_rows == 1 else T, T), dtype=torch.float32, device=self.device)
        rc = _lib.load().keep_op_attention_rollout_step(self._h, _ptr(qkv), B, T, heads, int(split), float(residual), _ptr(r_in), int(q_rows),
                                                        _ptr(out), _stream(self.device))
        _lib.check(self._h, rc, "op_attention_rollout_step")
        return out

    def layernorm(self, x, gamma, beta, eps, add=None):
        x, gamma, beta, add = map(self._f, (x, gamma, beta, add))
        out = torch.empty_like(x)
        rc = _lib.load().keep_op_layernorm(self._h, _ptr(x), _ptr(add), _ptr(gamma), _ptr(beta), x.shape[0], x.shape[1],
                                           float(eps), _ptr(out), _stream(self.device))
        _lib.check(self._h, rc, "op_layernorm")
        return out

    def sgemm(self, a, b, bias=None, scale=1.0, act=0):
        a, b, bias = map(self._f, (a, b, bias))
        out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=self.device)
        rc = _lib.load().keep_op_sgemm(self._h, _ptr(a), _ptr(b), _ptr(bias), a.shape[0], b.shape[0], a.shape[1],
                                       float(scale), int(act), _ptr(out), _stream(self.device))
        _lib.check(self._h, rc, "op_sgemm")
        return out

    def get_option(self, name: str) -> float:
        return float(_lib.load().keep_get_option(self._h, name.encode()))

    def patch_embed(self, pixels, w, bias, cls, pos, gh, gw, split=True, sentinel=0x3C, lo=True):
        """im2col + the patch-embedding GEMM with its row remap and position add, as the image tower runs them in front of block 0.
        pixels: fp32 / fp16 / bf16 [B,3,16 gh,16 gw] or uint8 [B,16 gh,16 gw,3]; w fp32 [D,768] (or the conv's [D,3,16,16]), pos [gh gw + 1, D]
        -> (resid [B (gh gw + 1), D], pat_hi, pat_lo [B gh gw, 768]): the token stream (preset to NaN) and the two im2col planes as fp32.  With
        split=False im2col is not given the lo plane: pat_lo then holds the preset, fp16 words of twice the byte `sentinel`.  lo=False: pat_lo None."""
        x = pixels.to(self.device).contiguous()
        if x.dtype == torch.uint8:
            code, B, ok = _lib.PIX_U8_HWC, x.shape[0], tuple(x.shape[1:]) == (16 * gh, 16 * gw, 3)
        else:
            code, B, ok = _PIX[x.dtype], x.shape[0], tuple(x.shape[1:]) == (3, 16 * gh, 16 * gw)
        if not ok:
            raise ValueError(f"pixels {tuple(x.shape)} {x.dtype} do not fit a {gh} x {gw} patch grid")
        w, bias, cls, pos = map(self._f, (w, bias, cls, pos))
        D, P = w.shape[0], gh * gw
        if w.numel() != D * 768 or bias.numel() != D or cls.numel() != D or tuple(pos.shape) != (P + 1, D):
            raise ValueError("patch_embed: w [D,768], bias [D], cls [D], pos [gh gw + 1, D]")
        resid = torch.empty((B * (P + 1), D), dtype=torch.float32, device=self.device)
        pat_hi = torch.empty((B * P, 768), dtype=torch.float32, device=self.device)
        pat_lo = torch.empty((B * P, 768), dtype=torch.float32, device=self.device) if lo else None
        rc = _lib.load().keep_op_patch_embed(self._h, _ptr(x), code, B, gh, gw, D, _ptr(w), _ptr(bias), _ptr(cls), _ptr(pos), int(split),
                                             int(sentinel), _ptr(resid), _ptr(pat_hi), _ptr(pat_lo), _stream(self.device))
        _lib.check(self._h, rc, "op_patch_embed")
        return resid, pat_hi, pat_lo

    def bert_embed(self, ids, type_ids, wemb, pemb, temb, gamma, beta, eps=1e-12, lo=True):
        """HF BertEmbeddings through the text tower's kernel: ids, type_ids int64 [P,T] (type_ids None: all 0) -> (resid, hi, lo, err): the fp32
        output [P T, H], the two fp16 operand planes it wrote (as fp32; lo None with lo=False) and the call's own error word (bit 0: an id or a
        type outside its table, clamped)."""
        ids = ids.to(self.device, torch.int64).contiguous()
        ty = None if type_ids is None else type_ids.to(self.device, torch.int64).contiguous()
        wemb, pemb, temb, gamma, beta = map(self._f, (wemb, pemb, temb, gamma, beta))
        P, T = ids.shape
        H = wemb.shape[1]
        if ty is not None and ty.shape != ids.shape:
            raise ValueError("type_ids must have the shape of ids")
        if pemb.shape[1] != H or temb.shape[1] != H or gamma.numel() != H or beta.numel() != H:
            raise ValueError("bert_embed: tables [*, H], gamma / beta [H]")
        resid, hi = (torch.empty((P * T, H), dtype=torch.float32, device=self.device) for _ in range(2))
        lo_t = torch.empty((P * T, H), dtype=torch.float32, device=self.device) if lo else None
        err = C.c_int(-1)
        rc = _lib.load().keep_op_bert_embed(self._h, _ptr(ids), _ptr(ty), _ptr(wemb), _ptr(pemb), _ptr(temb), _ptr(gamma), _ptr(beta), float(eps),
                                            P, T, H, wemb.shape[0], temb.shape[0], pemb.shape[0], _ptr(resid), _ptr(hi), _ptr(lo_t), C.byref(err),
                                            _stream(self.device))
        _lib.check(self._h, rc, "op_bert_embed")
        return resid, hi, lo_t, err.value

    def layernorm_rows(self, x, x_stride, rows, gamma, beta, eps):
        """LayerNorm of the rows that start x_stride elements apart in the flat fp32 buffer x -> dense [rows, D]."""
        x, gamma, beta = map(self._f, (x, gamma, beta))
        D = gamma.numel()
        if x.numel() < (rows - 1) * x_stride + D:
            raise ValueError("layernorm_rows: x is shorter than (rows - 1) x_stride + D")
        out = torch.empty((rows, D), dtype=torch.float32, device=self.device)
        rc = _lib.load().keep_op_layernorm_rows(self._h, _ptr(x), int(x_stride), _ptr(gamma), _ptr(beta), rows, D, float(eps), _ptr(out),
                                                _stream(self.device))
        _lib.check(self._h, rc, "op_layernorm_rows")
        return out

    def sgemm_ld(self, a, b, bias, M, N, K, lda, ldb, out, ldo, scale=1.0, act=0):
        """out[m ldo + n] = act(scale * sum_k a[m lda + k] b[n ldb + k] + bias[n]) on flat fp32 buffers; `out` is the caller's (on the device,
        preset as it likes): the columns N..ldo of its rows are not written."""
        a, b, bias = map(self._f, (a, b, bias))
        if out.device != self.device or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("sgemm_ld: out must be a contiguous fp32 tensor on the handle's device")
        if a.numel() < (M - 1) * lda + K or b.numel() < (N - 1) * ldb + K or out.numel() < (M - 1) * ldo + N:
            raise ValueError("sgemm_ld: a buffer is shorter than its leading dimension asks for")
        rc = _lib.load().keep_op_sgemm_ld(self._h, _ptr(a), int(lda), _ptr(b), int(ldb), _ptr(bias), M, N, K, float(scale), int(act), _ptr(out),
                                          int(ldo), _stream(self.device))
        _lib.check(self._h, rc, "op_sgemm_ld")
        return out

    def gather_rows(self, src, row_stride, rows, blk=False):
        """Rows 0, row_stride, 2 row_stride, ... of src fp32 [rows row_stride, D] -> [rows, D]; blk=True: through fp16 planes in blk layout
        (the result holds fp16 values)."""
        src = self._f(src)
        D = src.shape[1]
        if src.shape[0] != rows * row_stride:
            raise ValueError("gather_rows: src must be [rows row_stride, D]")
        dst = torch.empty((rows, D), dtype=torch.float32, device=self.device)
        rc = _lib.load().keep_op_rows(self._h, ROWS_GATHER_BLK if blk else ROWS_GATHER_F32, _ptr(src), int(row_stride), rows, D, _ptr(dst),
                                      _stream(self.device))
        _lib.check(self._h, rc, "op_rows")
        return dst

    def scatter_rows_(self, src, dst, row_stride):
        """Row r row_stride of dst fp32 [rows row_stride, D] (the caller's, on the device) <- row r of src [rows, D], in place."""
        src = self._f(src)
        rows, D = src.shape
        if dst.device != self.device or dst.dtype != torch.float32 or not dst.is_contiguous() or tuple(dst.shape) != (rows * row_stride, D):
            raise ValueError("scatter_rows_: dst must be a contiguous fp32 [rows row_stride, D] on the handle's device")
        rc = _lib.load().keep_op_rows(self._h, ROWS_SCATTER_F32, _ptr(src), int(row_stride), rows, D, _ptr(dst), _stream(self.device))
        _lib.check(self._h, rc, "op_rows")
        return dst

    def blk_col_sum_(self, x, col_sum):
        """col_sum fp32 [K] (the caller's, on the device) += the column sums of the fp16 hi plane of x [M, K]."""
        x = self._f(x)
        if col_sum.device != self.device or col_sum.dtype != torch.float32 or col_sum.numel() != x.shape[1] or not col_sum.is_contiguous():
            raise ValueError("blk_col_sum_: col_sum must be a contiguous fp32 [K] on the handle's device")
        rc = _lib.load().keep_op_bias_corr(self._h, BIAS_COL_SUM, _ptr(x), x.shape[0], x.shape[1], _ptr(col_sum), 0.0, None, None,
                                           _stream(self.device))
        _lib.check(self._h, rc, "op_bias_corr")
        return col_sum

    def bias_mean_corr(self, w, col_sum, inv_rows, bias):
        """bias[n] + inv_rows * sum_k w_lo[n][k] col_sum[k] on the lo plane of the fp16 split of w [N, K]."""
        w, col_sum, bias = map(self._f, (w, col_sum, bias))
        N, K = w.shape
        if col_sum.numel() != K or bias.numel() != N:
            raise ValueError("bias_mean_corr: col_sum [K], bias [N]")
        out = torch.empty(N, dtype=torch.float32, device=self.device)
        rc = _lib.load().keep_op_bias_corr(self._h, BIAS_MEAN_CORR, _ptr(w), N, K, _ptr(col_sum), float(inv_rows), _ptr(bias), _ptr(out),
                                           _stream(self.device))
        _lib.check(self._h, rc, "op_bias_corr")
        return out

    def l2norm_(self, x):
        rc = _lib.load().keep_op_l2norm(self._h, _ptr(x), x.shape[0], x.shape[1], _stream(self.device))
        _lib.check(self._h, rc, "op_l2norm")
        return x
