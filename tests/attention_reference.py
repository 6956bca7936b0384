"""Host references of the CLS attention maps, written from the definitions: the image tower up to one block's
scores restated from oracle/keep_oracle.py's own ``vit_tokens`` (same arithmetic, any dtype, stopped at the softmax of the chosen
block), timm's position-table resample for other tile sizes, and the cell raster as a triple loop over tiles and raster pixels in
Python integers.  tests/test_attention_maps.py holds keep_amd's numpy restatement to the triple loop on the CPU;
tests/test_attention_maps_gpu.py holds the kernels to these."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import keep_oracle as O


def rand(*shape, seed=0, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float32) * std


# ---------------------------------------------------------------------------------------------- the operator
def planes64(x, split):
    """The value the kernel reads for an fp32 operand, as float64: fp16(x), or fp16(x) + fp16(x - fp16(x)) in split mode."""
    hi = x.to(torch.float16)
    v = hi.to(torch.float64)
    if split:
        v = v + (x - hi.to(torch.float32)).to(torch.float16).to(torch.float64)
    return v


def cls_probs_reference(qkv, B, T, heads, split):
    """-> (p float64 [B, heads, T], A float64 [B, heads]): softmax_k(0.125 q_{b,h,0} . k_{b,h,k}) on the rounded operands, and
    A = max_k sum_i |q_i| |k_{k,i}|, what bounds an fp32 accumulation error of the scores."""
    v = planes64(qkv, split).reshape(B, T, 3, heads, 64)
    q0 = v[:, 0, 0]                                          # [B, heads, 64]
    k = v[:, :, 1].permute(0, 2, 1, 3)                       # [B, heads, T, 64]
    s = 0.125 * torch.einsum("bhi,bhki->bhk", q0, k)
    A = torch.einsum("bhi,bhki->bhk", q0.abs(), k.abs()).amax(dim=-1)
    return torch.softmax(s, dim=-1), A


# ---------------------------------------------------------------------------------------------- the tower
def _lin(x, w, b, dtype, operand_dtype):
    if operand_dtype is not None:
        x, w = x.to(operand_dtype), w.to(operand_dtype)
    return x.to(dtype) @ w.to(dtype).t() + b.to(dtype)


def tower_cls_attention(sd, x, block, heads=16, dtype=torch.float64, operand_dtype=None, eps=1e-6, prefix="visual."):
    """softmax(q k^T / 8)[:, :, 0, :] of block ``block`` (0-based, or negative from the end) -> [B, heads, T] in ``dtype``.  The blocks
    before it are oracle.vit_tokens' arithmetic in ``dtype``; ``operand_dtype`` rounds every GEMM operand and q / k / v first, as the
    oracle's operand-rounding model does."""
    depth = O.count_vit_depth(sd)
    block = block + depth if block < 0 else block
    assert 0 <= block < depth
    g = lambda k: sd[prefix + k].to(dtype)
    x = x.to(dtype)
    B = x.shape[0]
    wpe = sd[prefix + "patch_embed.proj.weight"]
    D, patch = wpe.shape[0], wpe.shape[-1]
    p = _lin(O.patchify(x, patch), wpe.reshape(D, -1), sd[prefix + "patch_embed.proj.bias"], dtype, operand_dtype)
    t = torch.cat([g("cls_token").expand(B, -1, -1), p], dim=1) + g("pos_embed")
    N, hd = t.shape[1], D // heads
    for i in range(block + 1):
        bp = f"blocks.{i}."
        h = O.layer_norm(t, g(bp + "norm1.weight"), g(bp + "norm1.bias"), eps)
        qkv = _lin(h, sd[prefix + bp + "attn.qkv.weight"], sd[prefix + bp + "attn.qkv.bias"], dtype, operand_dtype)
        q, k, v = qkv.reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
        if operand_dtype is not None:
            q, k, v = (z.to(operand_dtype).to(dtype) for z in (q, k, v))
        s = torch.softmax((q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(hd)), dim=-1)
        if i == block:
            return s[:, :, 0, :]
        a = (s @ v).transpose(1, 2).reshape(B, N, D)
        t = t + g(bp + "ls1.gamma") * _lin(a, sd[prefix + bp + "attn.proj.weight"], sd[prefix + bp + "attn.proj.bias"], dtype, operand_dtype)
        h = O.layer_norm(t, g(bp + "norm2.weight"), g(bp + "norm2.bias"), eps)
        m = O.gelu_erf(_lin(h, sd[prefix + bp + "mlp.fc1.weight"], sd[prefix + bp + "mlp.fc1.bias"], dtype, operand_dtype))
        t = t + g(bp + "ls2.gamma") * _lin(m, sd[prefix + bp + "mlp.fc2.weight"], sd[prefix + bp + "mlp.fc2.bias"], dtype, operand_dtype)
    raise AssertionError("unreachable")


def max_rel(got, ref):
    """The metric of the tower tests: the largest relative error over all entries."""
    return ((got.double() - ref.double()).abs() / ref.double()).max().item()


def timm_pos_embed(pos, gh, gw, old=(14, 14)):
    """timm.layers.resample_abs_pos_embed(pos, new_size=(gh, gw), old_size=old, num_prefix_tokens=1): unchanged at the old grid, else
    the CLS row as it is and the patch table through F.interpolate(bicubic, antialias=True, align_corners=False) in fp32."""
    if gh * gw + 1 == pos.shape[1] and gh == gw:
        return pos
    D = pos.shape[-1]
    cls, grid = pos[:, :1], pos[:, 1:]
    g = grid.reshape(1, old[0], old[1], D).permute(0, 3, 1, 2).float()
    g = F.interpolate(g, size=(gh, gw), mode="bicubic", antialias=True, align_corners=False)
    return torch.cat([cls, g.permute(0, 2, 3, 1).reshape(1, gh * gw, D).to(pos.dtype)], dim=1)


def sd_at(sd, H, W):
    d = dict(sd)
    d["visual.pos_embed"] = timm_pos_embed(sd["visual.pos_embed"], H // 16, W // 16)
    return d


# ---------------------------------------------------------------------------------------------- the cell raster
def cell_raster_brute(coords, values, grid, patch, d, shape, origin=(0, 0), into=None):
    """Every tile against every raster pixel, Python integers throughout -> int64 [h,w] (bits 0..39 sum of q, bits 40..63 tile count).
    Pixel (X, Y) is in tile (x, y)'s footprint iff floor((x - ox) / d) <= X < floor((x - ox + P) / d), rows likewise; it takes the cell
    under its upper-left corner, clamped into the grid, and adds nothing when that cell is NaN."""
    gh, gw = grid
    h, w = shape
    cw, ch = patch // gw, patch // gh
    acc = [[0] * w for _ in range(h)] if into is None else [[int(v) for v in row] for row in np.asarray(into).view(np.uint64)]
    vals = np.asarray(values, dtype=np.float32).reshape(-1, gh, gw)
    for n, (x, y) in enumerate(np.asarray(coords).reshape(-1, 2).tolist()):
        x, y = int(x) - origin[0], int(y) - origin[1]
        for Y in range(h):
            if not y // d <= Y < (y + patch) // d:
                continue
            cy = min(max((Y * d - y) // ch, 0), gh - 1)
            for X in range(w):
                if not x // d <= X < (x + patch) // d:
                    continue
                v = vals[n, cy, min(max((X * d - x) // cw, 0), gw - 1)]
                if np.isnan(v):
                    continue
                q = int(np.rint(np.clip(v, np.float32(0), np.float32(1)) * np.float32(65535)))
                acc[Y][X] += (1 << 40) | q
    return np.array(acc, dtype=np.uint64).view(np.int64)


def raster_cases():
    """name -> (coords int64 [N,2], values fp32 [N, gh gw], grid, patch, downsample, shape, origin): the cases both test files run."""
    rng = np.random.default_rng(20250919)
    cases = {}

    def vals(n, g):
        return rng.random((n, g[0] * g[1]), dtype=np.float32)

    g14 = (14, 14)
    aligned = np.array([[0, 0], [224, 0], [448, 224], [224, 448]], np.int64)
    for d, shape in ((16, (48, 48)), (4, (180, 176)), (1, (250, 256))):
        c = aligned if d > 1 else np.array([[0, 0], [16, 20]], np.int64)
        cases[f"aligned_d{d}"] = (c, vals(len(c), g14), g14, 224, d, shape, (0, 0))
    c = np.array([[5, 9], [229, 3], [101, 233], [333, 447]], np.int64)
    cases["unaligned_d16"] = (c, vals(4, g14), g14, 224, 16, (44, 40), (0, 0))
    cases["unaligned_d7"] = (c, vals(4, g14), g14, 224, 7, (90, 84), (0, 0))
    c = np.array([[-100, -50], [-230, 10], [500, -3], [560, 590], [-17, 600], [1000, 1000]], np.int64)
    cases["borders_d16"] = (c, vals(6, g14), g14, 224, 16, (42, 40), (0, 0))
    cases["borders_origin_d8"] = (c + 64, vals(6, g14), g14, 224, 8, (80, 84), (64, -32))
    c = np.array([[x, y] for y in range(0, 448, 112) for x in range(0, 448, 112)], np.int64)
    cases["overlap_step112"] = (c, vals(len(c), g14), g14, 224, 16, (44, 44), (0, 0))
    c = np.array([[0, 0], [240, 7], [100, 250], [-60, -90]], np.int64)
    cases["grid3x5_patch240"] = (c, vals(4, (3, 5)), (3, 5), 240, 16, (36, 34), (0, 0))
    c = np.array([[3, 5], [230, 120], [120, 230]], np.int64)
    v = vals(3, g14)
    v[0, ::3] = np.nan
    v[1, :] = np.nan
    v[2, 100:] = np.nan
    cases["nan_cells"] = (c, v, g14, 224, 16, (30, 30), (0, 0))
    c = rng.integers(-200, 3000, size=(200, 2)).astype(np.int64)
    v = vals(200, g14) * 1.4 - 0.2                          # values outside [0, 1] are clipped
    cases["many_tiles"] = (c, v, g14, 224, 16, (200, 200), (0, 0))
    return cases
