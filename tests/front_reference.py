"""Host references of what the towers run in front of their first block: the fp16 plane split, the im2col index map of the patch
embedding, the uint8 normalisation and the BERT embeddings.  Plain torch on the CPU, fp64 wherever arithmetic is involved that the kernels
do not perform bit for bit; tests/test_front_ops.py checks these references themselves, tests/test_front_ops_gpu.py holds the kernels
against them."""
import torch

PATCH = 16
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def split_planes(x32):
    """The fp16 operand planes of an fp32 tensor (common.h split_f16): hi = fp16(x), lo = fp16(x - hi) with the difference taken in fp32."""
    assert x32.dtype == torch.float32
    hi = x32.half()
    lo = (x32 - hi.float()).half()
    return hi, lo


def bits16(t):
    """fp16 values (given as fp16, or as the fp32 the op entry points read them back as: exact both ways) as their int16 words: -0 and +0, and
    every subnormal, compare as what they are."""
    return t.half().contiguous().view(torch.int16)


def im2col_patches(x):
    """x [B, 3, 16 gh, 16 gw] -> [B gh gw, 768]: row b gh gw + y gw + x is the 16 x 16 patch (y, x) of image b, its 768 elements in the order of
    a flattened conv weight [3, 16, 16].  nn.Unfold is the definition of that order (a convolution is unfold + matmul)."""
    B = x.shape[0]
    cols = torch.nn.functional.unfold(x, kernel_size=PATCH, stride=PATCH)          # [B, 768, gh gw], patches in row-major (y, x) order
    return cols.transpose(1, 2).reshape(B * cols.shape[2], 3 * PATCH * PATCH)


def normalize_u8(u8):
    """uint8 [B, H, W, 3] -> fp32 [B, 3, H, W]: torchvision's ToTensor + Normalize, (u / 255 - mean) / std, every operation in fp32 with fp32
    tensor operands (a division by a Python scalar may be turned into a multiplication by its reciprocal; a tensor divisor is not)."""
    assert u8.dtype == torch.uint8 and u8.device.type == "cpu"
    x = u8.permute(0, 3, 1, 2).to(torch.float32)
    mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float32).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, dtype=torch.float32).view(1, 3, 1, 1)
    return ((x / torch.tensor(255.0, dtype=torch.float32).view(1, 1, 1, 1)) - mean) / std


def bert_embed_sum(ids, type_ids, wemb, pemb, temb):
    """The fp32 sum HF BertEmbeddings normalises, in its order: (word + token_type) + position.  ids [P, T]; type_ids None: all 0."""
    P, T = ids.shape
    ty = torch.zeros_like(ids) if type_ids is None else type_ids
    pos = torch.arange(T).expand(P, T)
    return ((wemb[ids] + temb[ty]) + pemb[pos]).reshape(P * T, wemb.shape[1])


def bert_embed_ref(ids, type_ids, wemb, pemb, temb, gamma, beta, eps):
    """fp64 LayerNorm of the fp32 sum above -> fp64 [P T, H]"""
    s = bert_embed_sum(ids, type_ids, wemb, pemb, temb).double()
    return torch.nn.functional.layer_norm(s, (s.shape[1],), gamma.double(), beta.double(), eps)


def clamp_ids(ids, vocab):
    return ids.clamp(0, vocab - 1)
