"""The host side of tile clustering: the numpy restatements of keep_amd.cluster held to per-tile Python loops,
k-means on planted blobs, and every argument check.  No GPU: the device kernels are held to these restatements in test_cluster_gpu.py."""
import math

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel, cluster, wsi
from keep_amd.cluster import (ONE, ClusterSums, accumulate_numpy, assign_numpy, check_centroids, check_features, check_init, check_k,
                              kmeans_numpy, seed_numpy, update_numpy)


def unit_rows(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def blobs(sizes, d, noise, seed):
    """Unit rows around len(sizes) random unit centres -> (x fp32 [N,d], truth [N]); the blobs are interleaved."""
    g = np.random.default_rng(seed)
    centres = unit_rows(len(sizes), d, seed + 1000).astype(np.float64)
    truth = g.permutation(np.repeat(np.arange(len(sizes)), sizes))
    x = centres[truth] + noise * g.standard_normal((len(truth), d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32), truth


def row_skipped(row):
    return any((not math.isfinite(float(v))) or abs(float(v)) > 1.0 for v in row)


def assign_loop(x, c):
    labels, best, margin = [], [], []
    for row in x:
        if row_skipped(row):
            labels.append(-1); best.append(0.0); margin.append(0.0)
            continue
        s = [math.fsum(float(a) * float(b) for a, b in zip(row, cen)) for cen in c]
        l = 0
        for k in range(1, len(s)):
            if s[k] > s[l]:                                              # strictly: the first maximum stays
                l = k
        rest = [s[k] for k in range(len(s)) if k != l]
        labels.append(l); best.append(s[l]); margin.append(s[l] - max(rest) if rest else 0.0)
    return labels, best, margin


def llrint(v):
    return int(round(float(v) * ONE))                                    # Python's round is half-to-even, and the product is exact


@pytest.mark.parametrize("n,k,seed", [(40, 5, 0), (17, 1, 1), (33, 2, 2)])
def test_assign_matches_a_per_tile_loop(n, k, seed):
    x, c = unit_rows(n, 16, seed), unit_rows(k, 16, seed + 50)
    x[3, 2] = np.nan
    x[5, 0] = np.inf
    x[7, 15] = 1.5
    x[9, 4] = -1.25
    labels, best, margin = assign_numpy(x, c)
    wl, wb, wm = assign_loop(x, c)
    assert labels.dtype == np.int32 and labels.tolist() == wl
    assert np.allclose(best, wb, rtol=0, atol=1e-15) and np.allclose(margin, wm, rtol=0, atol=1e-15)
    assert labels[[3, 5, 7, 9]].tolist() == [-1] * 4 and (best[[3, 5, 7, 9]] == 0).all() and (margin[[3, 5, 7, 9]] == 0).all()
    assert (labels[[0, 1, 2, 4]] >= 0).all()
    if k == 1:
        assert (margin == 0).all()


def test_first_maximum_wins_a_tie():
    x = unit_rows(20, 16, 3)
    c = unit_rows(4, 16, 4)
    c[3] = c[1]                                                          # bit-equal centroids: the lower index is chosen
    c[2] = c[0]
    labels, _, margin = assign_numpy(x, c)
    assert set(labels.tolist()) <= {0, 1}
    assert (margin == 0).all()                                           # the runner-up is the copy
    x[0] = c[1]
    assert assign_numpy(x, c)[0][0] == 1 and abs(assign_numpy(x, c)[1][0] - 1) < 1e-6


def test_accumulate_matches_a_per_tile_loop():
    n, d, k = 40, 16, 5
    x, c = unit_rows(n, d, 5), unit_rows(k, d, 6)
    x[2, 1] = np.nan
    x[11, 3] = 2.0
    x[20] = 0.0
    x[21, 0] = 2.0 ** -31                                                # half of the fixed point's step: rounds to even, 0
    x[22, 0] = 3 * 2.0 ** -31                                            # 1.5 steps: rounds to 2
    labels, best, _ = assign_numpy(x, c)
    prev = np.roll(labels, 1)
    sums, counts, cos_sum, changed, skipped = accumulate_numpy(x, labels, best.astype(np.float32), k, prev)
    ws, wc, wcos, wch = [[0] * d for _ in range(k)], [0] * k, 0, 0
    for r in range(n):
        wch += int(labels[r] != prev[r])
        if labels[r] < 0:
            continue
        for j in range(d):
            ws[labels[r]][j] += llrint(x[r, j])
        wc[labels[r]] += 1
        wcos += llrint(np.float32(best[r]))
    assert sums.dtype == np.int64 and sums.tolist() == ws and counts.tolist() == wc
    assert (cos_sum, changed, skipped) == (wcos, wch, 2)
    assert llrint(x[21, 0]) == 0 and llrint(x[22, 0]) == 2
    # the sums do not depend on the split: two halves added equal the whole
    half = accumulate_numpy(x[:17], labels[:17], best[:17].astype(np.float32), k, prev[:17])
    both = accumulate_numpy(x[17:], labels[17:], best[17:].astype(np.float32), k, prev[17:], into=half)
    assert (both[0] == sums).all() and (both[1] == counts).all() and both[2:] == (cos_sum, changed, skipped)
    assert accumulate_numpy(x, labels, best.astype(np.float32), k)[3] == 0            # no prev: nothing changed


def test_update_matches_a_loop_and_keeps_an_empty_cluster():
    n, d, k = 30, 16, 4
    x, c = unit_rows(n, d, 7), unit_rows(k, d, 8)
    labels, best, _ = assign_numpy(x, c)
    labels[labels == 2] = 0                                              # cluster 2 is emptied
    sums, counts, *_ = accumulate_numpy(x, labels, best, k)
    new, empty = update_numpy(sums, counts, c)
    assert new.dtype == np.float32 and empty.dtype == np.uint8 and empty.tolist() == [0, 0, 1, 0]
    assert new[2].tobytes() == c[2].tobytes()
    for j in (0, 1, 3):
        s = [int(v) / ONE for v in sums[j]]
        norm = math.sqrt(math.fsum(v * v for v in s))
        assert np.allclose(new[j], [v / norm for v in s], rtol=0, atol=2.0 ** -24)
        assert abs(float(np.linalg.norm(new[j].astype(np.float64))) - 1) < 1e-6
    # a cluster whose members cancel has a count and a zero sum: kept too
    sums[1] = 0
    assert update_numpy(sums, counts, c)[1].tolist() == [0, 1, 1, 0]


def seed_loop(x, k):
    keep = [r for r in range(len(x)) if not row_skipped(x[r])]
    d = x.shape[1]
    tot = [sum(llrint(x[r, j]) for r in keep) / ONE for j in range(d)]
    norm = math.sqrt(math.fsum(v * v for v in tot))
    mean = [float(np.float32(v / norm)) for v in tot]
    dot = lambda a, b: math.fsum(float(p) * float(q) for p, q in zip(a, b))
    first = keep[0]
    for r in keep:
        if dot(x[r], mean) > dot(x[first], mean):
            first = r
    out, nearest = [first], {r: -math.inf for r in keep}
    for _ in range(1, k):
        for r in keep:
            nearest[r] = max(nearest[r], dot(x[r], x[out[-1]]))
        pick = keep[0]
        for r in keep:
            if nearest[r] < nearest[pick]:                               # strictly: the lowest index stays
                pick = r
        out.append(pick)
    return out


def test_seeding_order_and_lowest_index_ties():
    x = unit_rows(30, 16, 9)
    x[0, 3] = np.nan                                                     # never a candidate
    x[12] = x[4]                                                         # duplicated rows: every value they have ties
    x[25] = x[4]
    gaps = []
    got = seed_numpy(x, 5, gaps)
    assert got.dtype == np.int64 and got.tolist() == seed_loop(x, 5) and len(gaps) == 5
    assert 0 not in got and 12 not in got and 25 not in got or 4 in got
    # three copies of the direction opposite to the mean are the farthest from the first centre: the lowest of their indices is chosen
    y, _ = blobs([20], 16, 0.05, 10)
    far = -y.astype(np.float64).sum(axis=0)
    far = (far / np.linalg.norm(far)).astype(np.float32)
    y[6] = far
    y[3] = far
    y[17] = far
    assert seed_numpy(y, 2).tolist() == seed_loop(y, 2) and seed_numpy(y, 2)[1] == 3
    assert seed_numpy(np.full((4, 16), np.nan, np.float32), 3).tolist() == [-1, -1, -1]


def test_kmeans_recovers_three_planted_blobs():
    x, truth = blobs([60, 35, 25], 16, 0.05, 11)
    r = kmeans_numpy(x, 3)
    assert r["converged"] and r["changed"] == 0 and 2 <= r["n_iter"] <= 10 and r["skipped"] == 0
    relabel = {int(r["labels"][np.flatnonzero(truth == b)[0]]): b for b in range(3)}
    assert sorted(relabel) == [0, 1, 2]
    assert [relabel[int(l)] for l in r["labels"]] == truth.tolist()
    assert sorted(r["counts"].tolist()) == [25, 35, 60] and not r["empty"].any()
    assert r["mean_cosine"] > 0.95 and r["min_margin"] > 0.1
    assert abs(np.linalg.norm(r["centroids"].astype(np.float64), axis=1) - 1).max() < 1e-6
    # the fixed point: another pass from the result changes nothing, with either kind of init
    again = kmeans_numpy(x, 3, init=r["centroids"])
    assert again["n_iter"] == 2 and again["converged"]           # the first pass counts every tile as changed (from no label)
    assert again["centroids"].tobytes() == r["centroids"].tobytes() and (again["labels"] == r["labels"]).all()
    by_rows = kmeans_numpy(x, 3, init=seed_numpy(x, 3))
    assert (by_rows["labels"] == r["labels"]).all() and by_rows["n_iter"] == r["n_iter"]
    # max_iter too small: not converged, and the labels are those of the final centroids
    short = kmeans_numpy(x, 3, max_iter=1)
    assert not short["converged"] and short["n_iter"] == 1
    assert (assign_numpy(x, short["centroids"])[0] == short["labels"]).all()


def test_cluster_sums_is_one_buffer():
    s = ClusterSums(3, 16)
    assert s.sums.shape == (3, 16) and s.counts.shape == (3,) and s.cos_sum.shape == s.changed.shape == s.skipped.shape == (1,)
    s.sums[1, 2] = 5; s.counts[2] = 7; s.cos_sum[0] = 1; s.changed[0] = 2; s.skipped[0] = 3
    s.claim(10)
    assert s.tiles == 10 and int(s.buf.sum()) == 18
    with pytest.raises(ValueError, match="16777216"):
        s.claim(cluster.MAX_TILES)
    assert s.zero_() is s and s.tiles == 0 and int(s.buf.abs().sum()) == 0
    with pytest.raises(ValueError, match="K = 3, D = 16"):
        s.check(4, 16)
    with pytest.raises(ValueError, match="K = 3, D = 16"):
        s.check(3, 32)


def test_argument_checks_name_the_offending_value():
    x = unit_rows(8, 16, 0)
    for bad_k in (0, 65):
        with pytest.raises(ValueError, match=str(bad_k)):
            check_k(bad_k)
        with pytest.raises(ValueError, match=str(bad_k)):
            kmeans_numpy(x, bad_k)
        with pytest.raises(ValueError, match=str(bad_k)):
            ClusterSums(bad_k, 16)
    with pytest.raises(ValueError, match="2.5"):
        check_k(2.5)
    with pytest.raises(ValueError, match="24"):
        check_features(np.zeros((4, 24), np.float32))
    with pytest.raises(ValueError, match="1040"):
        check_features(np.zeros((4, 1040), np.float32))
    with pytest.raises(ValueError, match="float64"):
        check_features(np.zeros((4, 16)))
    with pytest.raises(ValueError, match="float16"):
        check_features(torch.zeros((4, 16), dtype=torch.float16))
    with pytest.raises(ValueError, match=r"\(4,\)"):
        check_features(np.zeros(4, np.float32))
    with pytest.raises(ValueError, match="got 0"):
        check_features(np.zeros((0, 16), np.float32))
    with pytest.raises(ValueError, match="width 32"):
        check_centroids(np.zeros((2, 32), np.float32), 16)
    with pytest.raises(ValueError, match="65"):
        check_centroids(np.zeros((65, 16), np.float32))
    with pytest.raises(ValueError, match="float64"):
        check_centroids(np.zeros((2, 16)))
    with pytest.raises(ValueError, match=r"\(2, 16\)"):
        check_init(np.zeros((2, 16), np.float32), 3, 8, 16)
    with pytest.raises(ValueError, match=r"\(4,\)"):
        check_init(np.arange(4), 3, 8, 16)
    with pytest.raises(ValueError, match="0..8"):
        check_init(np.array([0, 1, 8]), 3, 8, 16)
    with pytest.raises(ValueError, match="random"):
        check_init("random", 3, 8, 16)
    with pytest.raises(ValueError, match="-1"):
        kmeans_numpy(x, 2, max_iter=-1)
    with pytest.raises(ValueError, match="0.5"):
        kmeans_numpy(x, 2, tol_changed=0.5)
    with pytest.raises(ValueError, match=r"\(7,\)"):
        accumulate_numpy(x, np.zeros(7, np.int32), np.zeros(8, np.float32), 2)


def test_engine_entry_points_check_before_any_device_work():
    """The checks of KEEPModel.cluster_* and wsi.cluster_map run before the device is touched, so they hold without a GPU."""
    m = KEEPModel()
    x = torch.from_numpy(unit_rows(8, 16, 0))
    c = torch.from_numpy(unit_rows(3, 16, 1))
    with pytest.raises(ValueError, match="float64"):
        m.cluster_assign(x.double(), c)
    with pytest.raises(ValueError, match="24"):
        m.cluster_assign(torch.zeros(4, 24), torch.zeros(2, 24))
    with pytest.raises(ValueError, match="width 32"):
        m.cluster_assign(x, torch.zeros(2, 32))
    with pytest.raises(ValueError, match="K = 4, D = 16"):
        m.cluster_assign(x, c, sums=ClusterSums(4, 16))
    with pytest.raises(ValueError, match="K = 3, D = 32"):
        m.cluster_assign(x, c, sums=ClusterSums(3, 32))
    with pytest.raises(ValueError, match="K = 3, D = 32"):
        m.cluster_update(ClusterSums(3, 32), c)
    with pytest.raises(ValueError, match="dict"):
        m.cluster_assign(x, c, sums={})
    with pytest.raises(ValueError, match=r"\(5,\)"):
        m.cluster_assign(x, c, sums=ClusterSums(3, 16), prev=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match="int64"):
        m.cluster_assign(x, c, sums=ClusterSums(3, 16), prev=torch.zeros(8, dtype=torch.int64))
    for bad_k in (0, 65):
        with pytest.raises(ValueError, match=str(bad_k)):
            m.cluster_tiles(x, bad_k)
        with pytest.raises(ValueError, match=str(bad_k)):
            m.cluster_seed(x, bad_k)
        with pytest.raises(ValueError, match=str(bad_k)):
            wsi.cluster_map(x, torch.zeros(8, 2, dtype=torch.int64), bad_k, 16, (8, 8))
    with pytest.raises(ValueError, match=r"\(2, 16\)"):
        m.cluster_tiles(x, 3, init=torch.zeros(2, 16))
    with pytest.raises(ValueError, match=r"\(2,\)"):
        m.cluster_tiles(x, 3, init=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="farthest"):
        m.cluster_fit_batches(lambda: [x], 3, "farthest")
    with pytest.raises(ValueError, match="callable"):
        m.cluster_fit_batches([x], 3, c)
    with pytest.raises(ValueError, match=r"\(7, 2\)"):
        wsi.cluster_map(x, torch.zeros(7, 2, dtype=torch.int64), 3, 16, (8, 8))
    with pytest.raises(ValueError, match="max_iter"):
        wsi.cluster_map(x, torch.zeros(8, 2, dtype=torch.int64), c, 16, (8, 8), max_iter=3)
