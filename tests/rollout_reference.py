"""Host references of the attention rollout, written from the definition: the image tower of
tests/attention_reference.py run through EVERY block with each block's head-mean attention matrix kept, the left-multiplied product of
their identity blends read at the CLS row, and one step of it on the operands the kernel reads.  tests/test_attention_rollout.py holds
these to brute force on the CPU; tests/test_attention_rollout_gpu.py holds the kernels to these."""
import math

import torch

import attention_reference as AR
from oracle import keep_oracle as O


def tower_attention_mats(sd, x, heads=16, dtype=torch.float64, operand_dtype=None, eps=1e-6, prefix="visual.", per_head=False, keep_qkv=False):
    """AR.tower_cls_attention's loop through every block -> a list of depth tensors [B, T, T] in ``dtype``: block l's
    mean over the heads of softmax(q k^T / 8), all T query rows (``per_head``: [B, heads, T, T], the heads kept apart).
    ``keep_qkv``: -> (that list, the blocks' qkv rows [B, T, 3 D], q | k | v and head-major inside each, as the engine lays them out)."""
    depth = O.count_vit_depth(sd)
    g = lambda k: sd[prefix + k].to(dtype)
    x = x.to(dtype)
    B = x.shape[0]
    wpe = sd[prefix + "patch_embed.proj.weight"]
    D, patch = wpe.shape[0], wpe.shape[-1]
    p = AR._lin(O.patchify(x, patch), wpe.reshape(D, -1), sd[prefix + "patch_embed.proj.bias"], dtype, operand_dtype)
    t = torch.cat([g("cls_token").expand(B, -1, -1), p], dim=1) + g("pos_embed")
    N, hd = t.shape[1], D // heads
    mats, qkvs = [], []
    for i in range(depth):
        bp = f"blocks.{i}."
        h = O.layer_norm(t, g(bp + "norm1.weight"), g(bp + "norm1.bias"), eps)
        qkv = AR._lin(h, sd[prefix + bp + "attn.qkv.weight"], sd[prefix + bp + "attn.qkv.bias"], dtype, operand_dtype)
        qkvs.append(qkv)
        q, k, v = qkv.reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
        if operand_dtype is not None:
            q, k, v = (z.to(operand_dtype).to(dtype) for z in (q, k, v))
        s = torch.softmax((q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(hd)), dim=-1)
        mats.append(s if per_head else s.mean(dim=1))
        a = (s @ v).transpose(1, 2).reshape(B, N, D)
        t = t + g(bp + "ls1.gamma") * AR._lin(a, sd[prefix + bp + "attn.proj.weight"], sd[prefix + bp + "attn.proj.bias"], dtype, operand_dtype)
        h = O.layer_norm(t, g(bp + "norm2.weight"), g(bp + "norm2.bias"), eps)
        m = O.gelu_erf(AR._lin(h, sd[prefix + bp + "mlp.fc1.weight"], sd[prefix + bp + "mlp.fc1.bias"], dtype, operand_dtype))
        t = t + g(bp + "ls2.gamma") * AR._lin(m, sd[prefix + bp + "mlp.fc2.weight"], sd[prefix + bp + "mlp.fc2.bias"], dtype, operand_dtype)
    return (mats, qkvs) if keep_qkv else mats


def blend(a, residual):
    """(1 - residual) a + residual I for a [B, T, T]."""
    return (1 - residual) * a + residual * torch.eye(a.shape[-1], dtype=a.dtype)


def rollout(mats, start, residual):
    """Row 0 of blend(mats[L-1]) @ ... @ blend(mats[start]) (later blocks on the left) -> [B, T]; ``start`` may be negative."""
    L = len(mats)
    start = start + L if start < 0 else start
    assert 0 <= start < L
    R = blend(mats[start], residual)
    for l in range(start + 1, L):
        R = blend(mats[l], residual) @ R
    return R[:, 0, :]


def rollout_step_reference(qkv, B, T, heads, split, residual, r_in, q_rows):
    """One step in float64 on the operands the kernel reads (AR.planes64) -> (out [B, T or 1, T], A [B]): with At the identity blend of
    the head mean of softmax(0.125 q k^T), out = At @ r_in (At when r_in is None), its first row alone for q_rows = 1; and
    A = max over heads, query rows and keys of sum_i |q_i| |k_i| per tile, what bounds an fp32 accumulation error of the scores."""
    v = AR.planes64(qkv, split).reshape(B, T, 3, heads, 64)
    q = v[:, :, 0].permute(0, 2, 1, 3)                       # [B, heads, T, 64]
    k = v[:, :, 1].permute(0, 2, 1, 3)
    s = 0.125 * (q @ k.transpose(-1, -2))
    A = (q.abs() @ k.abs().transpose(-1, -2)).amax(dim=(1, 2, 3))
    at = blend(torch.softmax(s, dim=-1).mean(dim=1), residual)
    out = at if r_in is None else at @ r_in.to(torch.float64)
    return (out[:, :1] if q_rows == 1 else out), A
