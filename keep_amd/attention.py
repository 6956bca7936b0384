"""CLS attention maps: from the probabilities ``KEEPModel.encode_image_attention`` returns to the per-tile map
that is shown to a reader -- which patches of the tile the pooled feature's query attended to in one block.

``attn`` is fp32 ``[B, heads, T]``: row (b, h) is the softmax over the T = gh gw + 1 keys of the CLS query's scores in head h, column 0
the CLS -> CLS weight, columns 1.. the patch tokens in row-major (y, x) order.  :func:`cls_attention_map` is plain elementwise torch
on whatever device ``attn`` lives on; ``KEEPModel.cell_raster`` / ``keep_amd.wsi.attention_heatmap`` put its result on the slide raster.

Attention rollout: ``KEEPModel.encode_image_rollout`` returns the CLS row of the product of every block's
head-mean attention matrix, each blended with the identity, as a ONE-head tensor ``[B, 1, T]`` of the same layout, so everything here
and behind it takes it as it is.  Tiles of more than :data:`ROLLOUT_MAX_TOKENS` tokens are a ValueError there.

Not done here or anywhere in the engine: head fusion by max / min, a discard ratio or gradient weighting in the rollout, rows other than
the CLS query's as output, the text tower."""
from typing import Optional, Sequence, Union

import torch

NORMALIZATIONS = ("tile_max", "sum", "none")
ROLLOUT_MAX_TOKENS = 272        # tokens per tile the rollout kernels cover (17 key tiles of 16 in registers): every tile up to 256 x 256 pixels


def cls_attention_map(attn: torch.Tensor, heads: Optional[Union[int, Sequence[int]]] = None, normalize: str = "tile_max") -> torch.Tensor:
    """``attn`` [B, heads, T] -> the patch map ``[B, T - 1]`` (reshape to ``[B, gh, gw]`` for a picture).

    ``a[b, k] = mean over the chosen heads of attn[b, h, 1 + k]``: ``heads`` None takes all of them, an int that head alone, a sequence
    the mean of those (negative indices count from the end; IndexError-style mistakes are a ValueError).  Then

    * ``"tile_max"``: ``a[b] / max_k a[b, k]`` -- every tile's strongest patch is 1, the usual display; it shows WHERE inside a tile the
      query looked and makes tiles incomparable in absolute terms;
    * ``"sum"``: ``a[b] / sum_k a[b, k]`` -- the distribution over the patches alone, the CLS -> CLS share removed;
    * ``"none"``: ``a`` as it is; a row then sums to ``1 - (mean CLS -> CLS weight)``.

    A tile whose patch weights are all 0 stays 0 under either division.  The result is fp32 (fp64 for fp64 input)."""
    if not isinstance(attn, torch.Tensor) or attn.dim() != 3 or not attn.dtype.is_floating_point:
        raise ValueError(f"attn must be a floating-point [B, heads, T] tensor, got {getattr(attn, 'dtype', type(attn).__name__)} "
                         f"{tuple(getattr(attn, 'shape', ()))}")
    if normalize not in NORMALIZATIONS:
        raise ValueError(f"normalize must be one of {NORMALIZATIONS}, got {normalize!r}")
    B, H, T = attn.shape
    if H < 1 or T < 1:
        raise ValueError(f"attn needs at least one head and one token, got {tuple(attn.shape)}")
    if heads is None:
        pick = list(range(H))
    else:
        pick = list(heads) if isinstance(heads, (list, tuple, range)) else [heads]
        if not pick or any(isinstance(i, bool) or not isinstance(i, int) or not -H <= i < H for i in pick):
            raise ValueError(f"heads must be None, an index or a non-empty sequence of indices in [-{H}, {H}), got {heads!r}")
    a = attn if attn.dtype == torch.float64 else attn.to(torch.float32)
    a = a[:, pick, 1:].mean(dim=1)
    if normalize == "none" or T == 1:
        return a
    div = a.amax(dim=1, keepdim=True) if normalize == "tile_max" else a.sum(dim=1, keepdim=True)
    return a / torch.where(div > 0, div, torch.ones_like(div))
