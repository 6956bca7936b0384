"""The yardsticks of the attention rollout (tests/rollout_reference.py) held to brute force on the CPU, on a
depth-3 checkpoint and 2 tiles; and what the package exports for it."""
import math
import os

import pytest
import torch

import attention_reference as AR
import rollout_reference as RR
from keep_amd import _lib
from keep_amd.attention import ROLLOUT_MAX_TOKENS
from keep_amd.config import small_shape
from keep_amd.synth import synth_state_dict


@pytest.fixture(scope="module")
def sd():
    return {k: v for k, v in synth_state_dict(small_shape(3, 2), seed=5).items() if k.startswith("visual")}


@pytest.fixture(scope="module")
def x():
    return AR.rand(2, 3, 224, 224, seed=3)


@pytest.fixture(scope="module")
def mats(sd, x):
    with torch.no_grad():
        return RR.tower_attention_mats(sd, x)


def test_forward_product_equals_the_backward_row_recursion(mats):
    assert len(mats) == 3 and mats[0].shape == (2, 197, 197) and mats[0].dtype == torch.float64
    for start in (0, 1, 2, -1, -3):
        for residual in (0.0, 0.5, 0.9):
            got = RR.rollout(mats, start, residual)
            r = torch.zeros(2, 1, 197, dtype=torch.float64)
            r[:, 0, 0] = 1.0                                  # e_0, then r <- r At_l from the last block down
            for l in range(2, start % 3 - 1, -1):
                r = r @ RR.blend(mats[l], residual)
            assert (got - r[:, 0]).abs().max() <= 1e-14, (start, residual)


def test_rows_sum_to_one_and_every_entry_is_positive(mats):
    for m in mats:
        assert (m.sum(-1) - 1).abs().max() <= 1e-13 and (m > 0).all()
    for start, residual in ((0, 0.5), (1, 0.0), (-1, 0.9)):
        r = RR.rollout(mats, start, residual)
        assert r.shape == (2, 197) and (r > 0).all() and (r.sum(-1) - 1).abs().max() <= 1e-13


def test_last_block_without_residual_is_the_head_mean_of_the_cls_map(sd, x, mats):
    with torch.no_grad():
        want = AR.tower_cls_attention(sd, x, -1).mean(1)
    err = (RR.rollout(mats, -1, 0.0) - want).abs().max().item()
    print(f"[rollout start -1, residual 0 against tower_cls_attention(-1).mean(1)] max abs err {err:.1e}")
    assert err <= 1e-15
    with torch.no_grad():                                     # every block, head by head, not only the last
        heads = RR.tower_attention_mats(sd, x, per_head=True)
        for l in range(3):
            assert (heads[l][:, :, 0, :] - AR.tower_cls_attention(sd, x, l)).abs().max() <= 1e-15
            assert torch.equal(heads[l].mean(1), mats[l])


def test_residual_towards_one_tends_to_the_cls_unit_vector(mats):
    e0 = torch.zeros(197, dtype=torch.float64)
    e0[0] = 1.0
    last = None
    for residual in (0.9, 0.99, 0.999, 0.9999):
        d = (RR.rollout(mats, 0, residual) - e0).abs().sum(-1).max().item()
        assert d <= 2 * 3 * (1 - residual) * 1.0001           # each block moves at most (1 - residual) of the mass, L1 distance twice that
        assert last is None or d < last
        last = d


def test_step_reference_against_loops():
    B, T, heads = 2, 5, 2
    qkv = AR.rand(B * T, 3 * heads * 64, seed=9, std=1.5)
    g = torch.Generator().manual_seed(4)
    r_in = torch.softmax(torch.randn(B, T, T, generator=g), dim=-1)
    for split in (False, True):
        v = AR.planes64(qkv, split).reshape(B, T, 3, heads, 64)
        want = torch.zeros(B, T, T, dtype=torch.float64)
        amax = torch.zeros(B, dtype=torch.float64)
        for b in range(B):
            for i in range(T):
                for h in range(heads):
                    s = [0.125 * float((v[b, i, 0, h] * v[b, j, 1, h]).sum()) for j in range(T)]
                    z = sum(math.exp(t - max(s)) for t in s)
                    for j in range(T):
                        want[b, i, j] += math.exp(s[j] - max(s)) / z / heads
                        amax[b] = max(amax[b], float((v[b, i, 0, h].abs() * v[b, j, 1, h].abs()).sum()))
        at = 0.25 * want + 0.75 * torch.eye(T, dtype=torch.float64)
        got, A = RR.rollout_step_reference(qkv, B, T, heads, split, 0.75, None, 0)
        assert (got - at).abs().max() <= 1e-15 and ((A - amax).abs() <= 1e-12 * amax).all()
        got, _ = RR.rollout_step_reference(qkv, B, T, heads, split, 0.75, r_in, 0)
        prod = torch.stack([sum(at[b][:, k:k + 1] * r_in[b].double()[k:k + 1, :] for k in range(T)) for b in range(B)])
        assert got.shape == (B, T, T) and (got - prod).abs().max() <= 1e-15
        row, _ = RR.rollout_step_reference(qkv, B, T, heads, split, 0.75, r_in, 1)
        assert row.shape == (B, 1, T) and torch.equal(row, got[:, :1])


def test_exports():
    assert isinstance(ROLLOUT_MAX_TOKENS, int) and ROLLOUT_MAX_TOKENS >= 257
    for name in ("keep_rollout_scratch_bytes", "keep_encode_image_rollout", "keep_op_attention_rollout_step"):
        assert name in _lib.SIGNATURES, name
    from keep_amd import KEEPModel
    from keep_amd.ops import Ops
    assert callable(KEEPModel.encode_image_rollout) and callable(KEEPModel.encode_region_rollout) and callable(Ops.attention_rollout_step)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "keep_amd", "csrc", "common.h")).read()
    assert f"ROLLOUT_MAX_TOKENS = {ROLLOUT_MAX_TOKENS};" in hdr          # the launcher's limit and the Python layer's are one number
