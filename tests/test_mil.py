"""The host side of attention MIL: the float64 restatements of keep_amd.mil held to central differences, the
packing of the words, the chunk table, every argument check, and the Adam fit of the restatement on the synthetic cohort, which is
what justifies the outcomes test_mil_gpu.py asserts of the device fit.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel, _lib, mil, tile_eval, wsi
from keep_amd.mil import (CHUNK, AttentionMIL, MilSums, adam, check_hidden, check_offsets, check_params, chunk_table, fit_numpy, forward_numpy,
                          init_params, join_words, key_share, objective_numpy, pack, split_words, synthetic_cohort, unpack)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the cohort of both test files: bag sizes around the 64-row workgroup and the chunk, an empty bag, a bag with one NaN row, a bag whose
# rows are all out of range, and a bag labelled -1
BAG_SIZES = (1, 63, 64, 65, CHUNK, CHUNK + 1, 2 * CHUNK + 6, 0, 7, 5, 9)
NAN_BAG, BAD_BAG, UNLABELLED_BAG, EMPTY_BAG = 8, 9, 10, 7
FIT = dict(hidden=16, l2=1e-4, lr=0.01, n_steps=100, seed=0)               # the fit of both test files
FIT_SHARE_FLOAT64 = 1.0                                                     # key_share of the float64 fit below (measured here, on the CPU)
_cohorts = {}


def cohort(D, C, seed=0):
    """-> (x fp32 [N, D], offsets int64, labels int32 [S]): unit rows; row 3 of NAN_BAG holds a NaN, every row of BAD_BAG an element of
    1.5; every class labels some kept bag.  Computed once and shared (never written to)."""
    if (D, C, seed) not in _cohorts:
        g = np.random.default_rng(900 + seed)
        o = np.concatenate([[0], np.cumsum(BAG_SIZES)]).astype(np.int64)
        x = g.standard_normal((int(o[-1]), D))
        x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
        x[o[NAN_BAG] + 3, D // 2] = np.nan
        x[o[BAD_BAG]:o[BAD_BAG + 1], 1] = 1.5
        y = (np.arange(len(BAG_SIZES)) % C).astype(np.int32)
        y[UNLABELLED_BAG] = -1
        for a in (x, o, y):
            a.setflags(write=False)
        _cohorts[(D, C, seed)] = (x, o, y)
    return _cohorts[(D, C, seed)]


def params32(D, L, C, seed):
    """Parameters away from the initial point: a trained model's scale (scores spread over a few units, logits of order 1)."""
    g = np.random.default_rng(700 + seed)
    return ((g.standard_normal((L, D)) * 2.0 / np.sqrt(D)).astype(np.float32), (g.standard_normal(L) * 0.3).astype(np.float32),
            (g.standard_normal(L) * 4.0 / np.sqrt(L)).astype(np.float32), (g.standard_normal((C, D)) * 2.0 / np.sqrt(D)).astype(np.float32),
            (g.standard_normal(C) * 0.25).astype(np.float32))


def test_gradient_matches_central_differences():
    """h = 2^-17: the truncation h^2 |F'''| / 6 is of order 1e-11 |F'''| and the rounding of two float64 objectives over 2 269 rows,
    2 269 x 2^-53 |F| / (2 h) = 1.7e-8; the tolerance 1e-7 covers both."""
    D, L, C = 48, 16, 3
    x, o, y = cohort(D, C)
    cw = np.array([1.0, 0.5, 0.25])
    p = params32(D, L, C, 1)
    th = pack(p)
    f, g = objective_numpy(x, o, y, p, 1e-3, cw)
    gg = pack(g)
    assert gg.shape == th.shape and np.isfinite(f)
    rng = np.random.default_rng(0)
    h = 2.0 ** -17
    dirs = [rng.standard_normal(th.shape) for _ in range(4)]
    ends = np.cumsum((0,) + mil.sizes(L, C, D))
    for a, b in zip(ends[:-1], ends[1:]):                                  # one direction inside every parameter block
        d = np.zeros_like(th)
        d[a:b] = rng.standard_normal(b - a)
        dirs.append(d)
    for d in dirs:
        d = d / np.linalg.norm(d)
        fp, _ = objective_numpy(x, o, y, unpack(th + h * d, L, C, D), 1e-3, cw)
        fm, _ = objective_numpy(x, o, y, unpack(th - h * d, L, C, D), 1e-3, cw)
        assert abs((fp - fm) / (2 * h) - gg @ d) <= 1e-7, ((fp - fm) / (2 * h), gg @ d)


def test_forward_restatement_rules():
    D, L, C = 48, 16, 2
    x, o, y = cohort(D, C)
    f = forward_numpy(x, o, params32(D, L, C, 2))
    assert f["skipped_rows"] == 1 + BAG_SIZES[BAD_BAG] and f["skipped_bags"] == 2
    assert list(np.flatnonzero(f["labels"] < 0)) == [EMPTY_BAG, BAD_BAG]
    assert not f["probs"][[EMPTY_BAG, BAD_BAG]].any() and not f["z"][[EMPTY_BAG, BAD_BAG]].any()
    assert f["a"][o[NAN_BAG] + 3] == 0 and f["s"][o[NAN_BAG] + 3] == -np.inf
    sums = np.add.reduceat(f["a"], o[:-1][np.diff(o) > 0])
    kept = [b for b in range(len(BAG_SIZES)) if BAG_SIZES[b] and b != BAD_BAG]
    assert np.allclose(sums[[i for i, b in enumerate(np.flatnonzero(np.diff(o) > 0)) if b in kept]], 1.0, atol=1e-12)
    assert f["kept_rows"][NAN_BAG] == 6 and f["kept_rows"][BAD_BAG] == 0


def test_words_round_trip():
    L, C, D = 32, 3, 48
    g = np.random.default_rng(4)
    n = L * D + 2 * L + 2 + C * D + 2 * C + 2
    buf = g.integers(-2 ** 62, 2 ** 62, n, dtype=np.int64)
    words = split_words(buf, L, C, D)
    assert words["gV"].shape == (L, D) and words["gbv"].shape == (L,) and words["head"]["grad"].shape == (C, D)
    assert np.array_equal(join_words(words), buf)
    sums = MilSums(L, C, D)
    assert sums.buf.numel() == n
    sums.buf.copy_(torch.from_numpy(buf))
    assert np.array_equal(join_words(sums.host()), buf)
    assert torch.equal(sums.gV, sums.buf[:L * D].view(L, D)) and sums.head.grad.data_ptr() == sums.buf[L * D + 2 * L + 2:].data_ptr()
    sums.claim(5)
    assert sums.bags == 5 and sums.head.tiles == 5
    with pytest.raises(ValueError, match="2\\^16"):
        sums.claim(mil.MAX_BAGS)
    assert sums.zero_().bags == 0 and not sums.buf.any()
    theta = g.standard_normal(sum(mil.sizes(L, C, D)))
    assert np.array_equal(pack(unpack(theta, L, C, D)), theta)


def test_argument_checks():
    with pytest.raises(ValueError, match="non-decreasing"):
        check_offsets(np.array([0, 5, 3, 9]), 9)
    with pytest.raises(ValueError, match="start at 0"):
        check_offsets(np.array([1, 5, 9]), 9)
    with pytest.raises(ValueError, match="end at"):
        check_offsets(np.array([0, 5, 8]), 9)
    with pytest.raises(ValueError, match="integers"):
        check_offsets(np.array([0.0, 9.0]), 9)
    assert check_offsets(torch.tensor([0, 0, 9, 9]), 9).tolist() == [0, 0, 9, 9]
    with pytest.raises(ValueError, match="multiple of 16"):
        check_hidden(24)
    with pytest.raises(ValueError, match="multiple of 16"):
        check_hidden(144)
    D = 32
    V, bv, w, Wc, bc = params32(D, 16, 2, 0)
    assert check_params((V, bv, w, Wc, bc), D) == (16, 2, D)
    with pytest.raises(ValueError, match="multiple of 16"):
        check_params((np.zeros((24, D), np.float32), np.zeros(24, np.float32), np.zeros(24, np.float32), Wc, bc))
    with pytest.raises(ValueError, match="2\\.\\.64"):
        check_params((V, bv, w, Wc[:1], bc[:1]))
    with pytest.raises(ValueError, match="float32"):
        check_params((V.astype(np.float64), bv, w, Wc, bc))
    with pytest.raises(ValueError, match="width"):
        check_params((V, bv, w, Wc, bc), 48)
    with pytest.raises(ValueError, match="finite"):
        check_params((V, bv * np.float32(np.inf), w, Wc, bc))
    big = np.full((2, D), 9.0, np.float32)                                 # 4 x 1 x 288 = 1152 > 1024
    with pytest.raises(ValueError, match="gradient word"):
        check_params((V, bv, w, big, bc))
    assert check_params((V, bv, w, big, bc), values=False) == (16, 2, D)
    with pytest.raises(ValueError, match="gradient word"):
        check_params((V, bv, np.full(16, 40.0, np.float32), np.full((2, D), 0.25, np.float32), bc))
    with pytest.raises(ValueError, match="lr"):
        mil.check_adam(0.0, 10)
    with pytest.raises(ValueError, match="n_steps"):
        mil.check_adam(0.1, -1)


def test_chunk_table():
    o = np.concatenate([[0], np.cumsum([0, 1, CHUNK, CHUNK + 1])])
    t = chunk_table(o)
    assert t.dtype == np.int32
    assert t.tolist() == [[1, 0, 1], [2, 1, CHUNK], [3, CHUNK + 1, CHUNK], [3, 2 * CHUNK + 1, 1]]
    assert chunk_table(np.array([0, 0])).shape == (0, 3)
    t = chunk_table(np.array([0, 10, 10, 17]), 4)
    assert t.tolist() == [[0, 0, 4], [0, 4, 4], [0, 8, 2], [2, 10, 4], [2, 14, 3]]
    x, o, _ = cohort(48, 2)
    t = chunk_table(o)
    assert t[:, 2].sum() == x.shape[0] and (t[:, 2] >= 1).all() and (t[:, 2] <= CHUNK).all()


def test_constants_match_the_header_and_the_surface():
    hdr = open(os.path.join(ROOT, "include", "keep_hip.h")).read()
    assert int(re.search(r"#define KEEP_MIL_CHUNK (\d+)", hdr).group(1)) == CHUNK
    common = open(os.path.join(ROOT, "keep_amd", "csrc", "common.h")).read()
    assert f"MIL_MAX_L = {mil.MAX_L};" in common and "MIL_MAX_BAGS = (int64_t)1 << 16;" in common and mil.MAX_BAGS == 1 << 16
    for name in ("keep_mil_chunk", "keep_mil_workspace_bytes", "keep_mil_forward", "keep_mil_backward"):
        assert name in _lib.SIGNATURES, name
    for name in ("mil_forward", "mil_loss_grad", "mil_predict", "mil_fit", "mil_fit_batches"):
        assert callable(getattr(KEEPModel, name))
    assert callable(wsi.mil_attention_map) and callable(tile_eval.attention_mil)


def test_init_is_a_function_of_the_seed():
    a, b, c = init_params(7, 16, 2, 32), init_params(7, 16, 2, 32), init_params(8, 16, 2, 32)
    assert all(np.array_equal(p, q) for p, q in zip(a, b)) and not np.array_equal(a[0], c[0])
    assert np.abs(a[0]).max() <= 32 ** -0.5 and np.abs(a[2]).max() <= 0.25 and not a[3].any() and not a[1].any()
    assert abs(a[0].mean()) < 0.02 and a[0].std() > 0.08                   # uniform in +-0.177: std 0.102


def test_adam_minimises_a_quadratic():
    res = adam(lambda t: (float(((t - 3.0) ** 2).sum()), 2.0 * (t - 3.0)), np.zeros(4), lr=0.1, n_steps=400)
    assert np.abs(res.theta - 3.0).max() < 1e-3 and len(res.history) == 401 and res.history[-1] < 1e-5 < res.history[0]


def test_float64_fit_meets_the_outcomes_of_the_device_fit():
    """The three outcomes test_mil_gpu.py::test_fit asserts, reached by the float64 restatement with the same arguments."""
    x, o, y, key = synthetic_cohort(0)
    assert len(y) == 64 and x.shape[1] == 64 and 16 <= np.diff(o).min() and np.diff(o).max() <= 128
    per_bag = np.add.reduceat(key.astype(np.int64), o[:-1])
    assert ((per_bag[y == 1] >= 1) & (per_bag[y == 1] <= 3)).all() and not per_bag[y == 0].any()
    params, res = fit_numpy(x, o, y, 2, FIT["hidden"], FIT["l2"], None, FIT["lr"], FIT["n_steps"], FIT["seed"])
    assert res.history[-1] < res.history[0] and len(res.history) == FIT["n_steps"] + 1
    f = forward_numpy(x, o, params)
    assert (f["labels"] == y).all()
    assert key_share(f["a"], o, y, key) == FIT_SHARE_FLOAT64
