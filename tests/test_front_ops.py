"""The host references of tests/front_reference.py, checked on the CPU against independent formulations (torch's convolution, numpy's fp32
arithmetic, explicit loops), so that tests/test_front_ops_gpu.py holds the kernels against something that has itself been held."""
import numpy as np
import pytest
import torch

import front_reference as R


def rand(*shape, seed=0, std=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32) * std


def test_split_planes_is_the_format_definition():
    x = torch.cat([rand(4096, seed=1), rand(4096, seed=2) * 1e-3, torch.tensor([0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 2.0 ** 15, 65504.0, 1.0 / 3.0])])
    hi, lo = R.split_planes(x)
    assert hi.dtype == torch.float16 and lo.dtype == torch.float16
    # numpy performs the same two roundings
    xn = x.numpy()
    hn = xn.astype(np.float16)
    ln = (xn - hn.astype(np.float32)).astype(np.float16)
    assert np.array_equal(hi.numpy().view(np.int16), hn.view(np.int16)) and np.array_equal(lo.numpy().view(np.int16), ln.view(np.int16))
    # what common.h promises of the pair: |x - hi - lo| <= 2^-22 |x| (2^-25 absolute floor)
    err = (x.double() - hi.double() - lo.double()).abs()
    assert (err <= torch.maximum(2.0 ** -22 * x.double().abs(), torch.tensor(2.0 ** -25, dtype=torch.float64))).all()
    # a value fp16 holds exactly has a +0 lo plane, whatever its sign
    assert R.bits16(R.split_planes(hi.float())[1]).eq(0).all()
    # the sign of zero travels in the hi plane
    assert R.bits16(hi[8192:8194]).tolist() == [0, -32768]


def test_bits16_round_trips_through_fp32():
    words = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    h = words.view(torch.float16)
    finite = torch.isfinite(h.float())
    assert torch.equal(R.bits16(h.float())[finite], words[finite])


@pytest.mark.parametrize("B,gh,gw", [(2, 14, 14), (3, 2, 3), (1, 1, 1), (1, 3, 2)])
def test_im2col_map_is_the_convolution(B, gh, gw):
    """patches @ W.flatten(1).T + b == conv2d(x, W, b, stride=16) in fp64: the index map is the one the patch embedding's weight is laid out for."""
    D = 40
    x = rand(B, 3, 16 * gh, 16 * gw, seed=3).double()
    W, b = rand(D, 3, 16, 16, seed=4, std=0.05).double(), rand(D, seed=5).double()
    pat = R.im2col_patches(x)
    assert pat.shape == (B * gh * gw, 768)
    got = pat @ W.flatten(1).t() + b
    ref = torch.nn.functional.conv2d(x, W, b, stride=16)                      # [B, D, gh, gw]
    ref = ref.permute(0, 2, 3, 1).reshape(B * gh * gw, D)                     # timm PatchEmbed: flatten(2).transpose(1, 2)
    assert (got - ref).abs().max().item() < 1e-12
    # and element by element, with no library call in between: row (b, py, px), column (c, ky, kx)
    g = torch.Generator().manual_seed(6)
    for _ in range(64):
        bi, py, px = (int(torch.randint(n, (1,), generator=g)) for n in (B, gh, gw))
        c, ky, kx = (int(torch.randint(n, (1,), generator=g)) for n in (3, 16, 16))
        assert pat[(bi * gh + py) * gw + px, c * 256 + ky * 16 + kx] == x[bi, c, py * 16 + ky, px * 16 + kx]


def test_im2col_map_tells_gh_from_gw():
    x = rand(1, 3, 32, 48, seed=7)
    a = R.im2col_patches(x)
    b = R.im2col_patches(x.transpose(2, 3).contiguous())
    assert a.shape == b.shape == (6, 768) and not torch.equal(a, b)
    assert torch.equal(a[1], x[0, :, 0:16, 16:32].reshape(768))               # patch (0, 1) of a 2 x 3 grid
    assert torch.equal(a[3], x[0, :, 16:32, 0:16].reshape(768))               # patch (1, 0)


def test_u8_normalisation_is_fp32_in_torchvision_order():
    u = torch.arange(256, dtype=torch.uint8).view(1, 256, 1, 1).expand(1, 256, 1, 3).contiguous()
    got = R.normalize_u8(u)                                                   # [1, 3, 256, 1]
    assert got.dtype == torch.float32 and got.shape == (1, 3, 256, 1)
    v = np.arange(256, dtype=np.float32)
    for c in range(3):
        ref = (v / np.float32(255.0) - np.float32(R.IMAGENET_MEAN[c])) / np.float32(R.IMAGENET_STD[c])
        assert ref.dtype == np.float32
        assert np.array_equal(got[0, c, :, 0].numpy().view(np.int32), ref.view(np.int32))
    # within fp32 rounding of the exact value, and NOT what a multiplication by 1 / 255 gives everywhere (the order and the division matter)
    exact = (torch.arange(256, dtype=torch.float64) / 255.0 - R.IMAGENET_MEAN[0]) / R.IMAGENET_STD[0]
    assert (got[0, 0, :, 0].double() - exact).abs().max().item() < 4e-7
    recip = ((torch.arange(256, dtype=torch.float32) * torch.tensor(1.0 / 255.0, dtype=torch.float32)) - torch.tensor(R.IMAGENET_MEAN[0])) / torch.tensor(R.IMAGENET_STD[0])
    assert not torch.equal(recip, got[0, 0, :, 0])


def test_bert_embedding_reference_matches_an_explicit_loop():
    P, T, H, V = 3, 5, 32, 11
    g = torch.Generator().manual_seed(8)
    ids, ty = torch.randint(V, (P, T), generator=g), torch.randint(2, (P, T), generator=g)
    wemb, pemb, temb = rand(V, H, seed=9), rand(16, H, seed=10), rand(2, H, seed=11)
    gamma, beta = 1 + rand(H, seed=12, std=0.1), rand(H, seed=13, std=0.1)
    s = R.bert_embed_sum(ids, ty, wemb, pemb, temb)
    assert s.dtype == torch.float32 and s.shape == (P * T, H)
    for p in range(P):
        for t in range(T):
            assert torch.equal(s[p * T + t], (wemb[ids[p, t]] + temb[ty[p, t]]) + pemb[t])
    assert torch.equal(R.bert_embed_sum(ids, None, wemb, pemb, temb), R.bert_embed_sum(ids, torch.zeros_like(ids), wemb, pemb, temb))
    # the order is observable in fp32: the other association differs somewhere
    other = (wemb[ids] + (temb[ty] + pemb[torch.arange(T).expand(P, T)])).reshape(P * T, H)
    assert not torch.equal(other, s)
    ref = R.bert_embed_ref(ids, ty, wemb, pemb, temb, gamma, beta, 1e-12)
    d = s.double()
    mu, var = d.mean(1, keepdim=True), d.var(1, unbiased=False, keepdim=True)
    assert (ref - ((d - mu) / (var + 1e-12).sqrt() * gamma.double() + beta.double())).abs().max().item() < 1e-12
    assert torch.equal(R.clamp_ids(torch.tensor([-1, 0, V - 1, V]), V), torch.tensor([0, 0, V - 1, V - 1]))
