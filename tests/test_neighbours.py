"""The numpy restatements of keep_amd.neighbours against per-row Python loops and scikit-learn: the key of a
(score, bank row) pair, the top-k of a score matrix, the merge of two lists and the kNN vote.  No GPU."""
import math
import struct

import numpy as np
import pytest

from keep_amd.neighbours import (knn_vote_numpy, merge_numpy, pack_keys_numpy, topk_numpy, unpack_keys_numpy)
from test_cluster import blobs


def key_loop(s, g):
    """The definition, word by word."""
    s = float(np.float32(s)) + 0.0
    u = struct.unpack("<I", struct.pack("<f", s))[0]
    if s == 0.0:
        u = 0                                                            # -0 folded into +0
    u ^= 0xFFFFFFFF if u >> 31 else 0x80000000
    return (u << 32) | (0xFFFFFFFF - g)


def topk_loop(scores, k, bank_base=0, self_first=None):
    out = []
    for i, row in enumerate(scores):
        cand = [(-float(np.float32(s)), bank_base + c) for c, s in enumerate(row)
                if math.isfinite(float(s)) and (self_first is None or bank_base + c != self_first + i)]
        best = sorted(cand)[:k]
        out.append([key_loop(-s, g) for s, g in best] + [0] * (k - len(best)))
    return np.array(out, dtype=np.uint64)


def vote_loop(index, score, labels, C, mode, T):
    lab_out, probs_out, margin_out, skipped = [], [], [], 0
    for idx, sc in zip(index, score):
        v = [np.float32(0)] * C
        for r in range(len(idx)):
            if idx[r] < 0:
                continue
            c = int(labels[idx[r]])
            if not 0 <= c < C:
                continue
            w = np.float32(1)
            if mode == "softmax":
                z = np.float32(np.float32(sc[r] - sc[0]) / np.float32(T))
                w = np.float32(math.exp(float(z)))
            v[c] = np.float32(v[c] + w)
        tot = np.float32(0)
        for c in range(C):
            tot = np.float32(tot + v[c])
        if not tot > 0:
            lab_out.append(-1); probs_out.append([0.0] * C); margin_out.append(0.0); skipped += 1
            continue
        p = [np.float32(x / tot) for x in v]
        win = max(range(C), key=lambda c: (v[c], -c))
        lab_out.append(win)
        probs_out.append(p)
        margin_out.append(np.float32(p[win] - max(p[c] for c in range(C) if c != win)))
    return np.array(lab_out, np.int32), np.array(probs_out, np.float32), np.array(margin_out, np.float32), skipped


def random_scores(nq, m, seed, ties=True):
    g = np.random.default_rng(seed)
    s = g.uniform(-1, 1, (nq, m)).astype(np.float32)
    if ties:
        s = np.round(s * 8) / 8                                          # many equal scores, both zeros among them
        s[:, ::7] *= -1
    return s.astype(np.float32)


# ------------------------------------------------------------------------------------------------ keys
def test_key_round_trip_and_order():
    scores = np.array([-1.0, -0.5, -1e-30, -0.0, 0.0, 1e-30, 0.25, 1.0, 768.0, -1024.0], np.float32)
    index = np.array([0, 1, 5, 7, 7, 2, (1 << 32) - 2, 3, 0, 9], np.int64)
    keys = pack_keys_numpy(scores, index)
    assert [int(k) for k in keys] == [key_loop(s, int(g)) for s, g in zip(scores, index)]
    assert keys[3] == keys[4]                                            # -0.0 and +0.0 at the same row: one key
    gi, gs = unpack_keys_numpy(keys)
    assert np.array_equal(gi, index)
    assert np.array_equal(gs.view(np.uint32), (scores + np.float32(0)).view(np.uint32))
    assert not np.signbit(gs[3])
    assert (keys > 0).all()                                              # the empty slot is below every key
    # ascending (-score, index) is descending key
    g = np.random.default_rng(0)
    s = np.round(g.uniform(-1, 1, 500) * 4).astype(np.float32) / 4
    i = g.permutation(500).astype(np.int64)
    order = sorted(range(500), key=lambda t: (-float(s[t] + np.float32(0)), int(i[t])))
    assert np.array_equal(np.argsort(pack_keys_numpy(s, i))[::-1], np.array(order))


def test_empty_slots_and_int64_view():
    keys = pack_keys_numpy(np.array([[0.5, 0.0]], np.float32), np.array([[3, -1]], np.int64))
    assert keys[0, 1] == 0
    gi, gs = unpack_keys_numpy(keys.view(np.int64))                      # the bit patterns, as Neighbours.keys holds them
    assert gi.tolist() == [[3, -1]] and gs.tolist() == [[0.5, 0.0]]
    with pytest.raises(ValueError):
        pack_keys_numpy(np.array([np.nan], np.float32), np.array([0]))
    with pytest.raises(ValueError):
        pack_keys_numpy(np.array([0.0], np.float32), np.array([(1 << 32) - 1]))


# ------------------------------------------------------------------------------------------------ top-k and merge
@pytest.mark.parametrize("nq,m,k", [(5, 130, 20), (3, 65, 64), (2, 63, 64), (4, 7, 1), (1, 1, 5)])
def test_topk_matches_loop(nq, m, k):
    s = random_scores(nq, m, nq + m)
    assert np.array_equal(topk_numpy(s, k), topk_loop(s, k))
    assert np.array_equal(topk_numpy(s.astype(np.float64), k, bank_base=1000), topk_loop(s, k, bank_base=1000))
    if nq <= m:
        assert np.array_equal(topk_numpy(s, k, bank_base=3, self_first=4), topk_loop(s, k, bank_base=3, self_first=4))


def test_topk_leaves_non_finite_scores_out():
    s = random_scores(3, 70, 1)
    s[0, 5], s[1, :], s[2, 69] = np.nan, np.inf, -np.inf
    got = topk_numpy(s, 64)
    assert np.array_equal(got, topk_loop(s, 64))
    assert (got[1] == 0).all()
    assert 5 not in unpack_keys_numpy(got[0])[0]


@pytest.mark.parametrize("chunk", [1, 63, 64, 65])
@pytest.mark.parametrize("k", [1, 5, 64])
def test_merge_of_any_split_is_topk_of_the_whole(chunk, k):
    s = random_scores(4, 200, 7)
    whole = topk_numpy(s, k)
    for order in (1, -1):
        acc = np.zeros_like(whole)
        for c0 in list(range(0, 200, chunk))[::order]:
            acc = merge_numpy(acc, topk_numpy(s[:, c0:c0 + chunk], k, bank_base=c0))
        assert np.array_equal(acc, whole)


def test_merge_matches_loop():
    s = random_scores(6, 90, 3)
    a, b = topk_numpy(s[:, :40], 20), topk_numpy(s[:, 40:], 20, bank_base=40)
    want = np.array([sorted([int(x) for x in ra] + [int(x) for x in rb], reverse=True)[:20] for ra, rb in zip(a, b)], dtype=np.uint64)
    assert np.array_equal(merge_numpy(a, b), want)
    assert np.array_equal(merge_numpy(a.view(np.int64), b.view(np.int64)), want)


# ------------------------------------------------------------------------------------------------ vote
@pytest.mark.parametrize("C", [2, 3, 64])
@pytest.mark.parametrize("mode,T", [("uniform", 0.07), ("softmax", 0.07), ("softmax", 1.0)])
def test_vote_matches_loop(C, mode, T):
    g = np.random.default_rng(C)
    s = random_scores(40, 90, C, ties=False)
    index, score = unpack_keys_numpy(topk_numpy(s, 20))
    index[3, 15:], score[3, 15:] = -1, 0                                 # a short list
    labels = g.integers(-1, C, 90).astype(np.int32)
    index[5], index[6] = np.arange(20), np.arange(20, 40)
    labels[:20] = -1                                                     # a query whose neighbours are all unlabelled
    labels[20:22], labels[22:40] = [1, 0], -1                            # a two-way tie of one vote each goes to the lower class
    got = knn_vote_numpy(index, score, labels, C, mode, T)
    want = vote_loop(index, score, labels, C, mode, T)
    for a, b in zip(got[:3], want[:3]):
        assert np.array_equal(a, b)
    assert got[3] == want[3] >= 1 and got[0][5] == -1 and not got[1][5].any()
    if mode == "uniform":
        assert got[0][6] == 0 and got[2][6] == 0


def test_vote_arguments():
    i, s = np.zeros((1, 1), np.int64), np.zeros((1, 1), np.float32)
    for bad in (dict(C=1), dict(C=65), dict(mode="distance"), dict(temperature=0.0), dict(temperature=float("nan"))):
        with pytest.raises(ValueError):
            knn_vote_numpy(i, s, np.zeros(1, np.int32), **{"C": 2, **bad})
    for bad in (0, 65, 2.5, True):
        with pytest.raises(ValueError):
            topk_numpy(np.zeros((1, 4)), bad)
    with pytest.raises(ValueError):
        topk_numpy(np.zeros((1, 4)), 2, bank_base=(1 << 32) - 4)


# ------------------------------------------------------------------------------------------------ scikit-learn
SK_CASES = [([300, 200, 150, 100], 768, 0.05, 0, 20), ([40, 30, 20], 32, 0.3, 1, 5), ([500, 400, 300, 200, 100], 1024, 0.06, 2, 64)]


@pytest.mark.parametrize("sizes,d,noise,seed,k", SK_CASES)
def test_against_scikit_learn(sizes, d, noise, seed, k):
    from sklearn import neighbors
    x, y = blobs(sizes, d, noise, seed)
    h = len(x) // 2
    train, test, ytrain = x[:h].astype(np.float64), x[h:].astype(np.float64), y[:h]
    C = len(sizes)
    index, score = unpack_keys_numpy(topk_numpy(test @ train.T, k))
    labels, probs, _, skipped = knn_vote_numpy(index, score, ytrain, C, "uniform")
    clf = neighbors.KNeighborsClassifier(n_neighbors=k, metric="cosine", algorithm="brute").fit(train, ytrain)
    assert skipped == 0
    assert np.array_equal(clf.predict_proba(test).astype(np.float32), probs)
    assert np.array_equal(clf.predict(test), labels)
    nn = neighbors.NearestNeighbors(n_neighbors=k, metric="cosine", algorithm="brute").fit(train)
    theirs = nn.kneighbors(test, return_distance=False)
    # equal as lists wherever the fp32 scores of a list are distinct (sklearn orders by float64 distance); as sets of rows otherwise
    distinct = (np.diff(score, axis=1) < 0).all(axis=1)
    assert distinct.mean() > 0.9
    assert np.array_equal(theirs[distinct], index[distinct])
