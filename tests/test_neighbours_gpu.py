"""Nearest neighbours on the MI355X: keep_topk / keep_topk_merge / keep_topk_unpack / keep_knn_vote,
KEEPModel.topk / topk_batches / knn_vote, tile_eval.knn_probe, wsi.knn_map and wsi.search_tiles.

The yardsticks: a score is keep_cluster_assign's `best` against a one-row centroid bank, bit for bit; the lists are
keep_amd.neighbours.topk_numpy's over those scores (tests/test_neighbours.py holds the numpy side to per-row loops); against float64
the scores lie within b = D 2^-24 (sum |a b| <= 1 for unit rows), so with t the float64 k-th largest score of a row every returned
row scores >= t - 2b and every row scoring > t + 2b is returned.  Keys are compared with torch.equal."""
import ctypes as C_

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel, _lib, tile_eval, wsi
from keep_amd.classmap import ClassRaster, class_raster_numpy, one_hot_numpy
from keep_amd.config import small_shape
from keep_amd.model import _ptr, _stream
from keep_amd.neighbours import Neighbours, knn_vote_numpy, merge_numpy, topk_numpy, unpack_keys_numpy
from keep_amd.synth import synth_state_dict
from test_cluster import blobs, unit_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def model():
    m = KEEPModel(precision="strict")
    m.load_state_dict(synth_state_dict(small_shape(2, 2), seed=5), strict=True)
    return m.to(DEV).eval()


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                         # a copy: the shared cases are read-only


def bound(D):
    return D * 2.0 ** -24


_cases = {}


def case(D, M, Nq):
    """Random unit queries and bank rows with their float64 scores, computed once and shared (never written to)."""
    key = (D, M, Nq)
    if key not in _cases:
        q, b = unit_rows(Nq, D, 300 + M), unit_rows(M, D, 400 + Nq)
        s64 = q.astype(np.float64) @ b.astype(np.float64).T
        for a in (q, b, s64):
            a.setflags(write=False)
        _cases[key] = (q, b, s64)
    return _cases[key]


def topk(model, q, b, k, **kw):
    kw.setdefault("normalize", False)
    return model.topk(q if isinstance(q, torch.Tensor) else dev(q), b if isinstance(b, torch.Tensor) else dev(b), k, **kw)


def device_scores(model, q, b):
    """Every (query, bank row) score as the device computes it, fp32 [Nq, M], NaN where a row is skipped: the bank offered in chunks of
    at most 64 rows with k = 64, so that every candidate is returned (test 1 pins these scores to cluster_assign's)."""
    q, b = dev(q), dev(b)
    out = np.full((q.shape[0], b.shape[0]), np.nan, np.float32)
    for c0 in range(0, b.shape[0], 64):
        nb = topk(model, q, b[c0:c0 + 64], 64, bank_base=c0)
        idx, sc = nb.index.cpu().numpy(), nb.score.cpu().numpy()
        rows = np.nonzero(idx >= 0)
        out[rows[0], idx[rows]] = sc[rows]
    return out


def check_consistent(nb):
    """index / score / count are the keys unpacked, and the lists descend strictly (score, then ascending index)."""
    keys = nb.keys_numpy()
    idx, sc = unpack_keys_numpy(keys)
    assert np.array_equal(nb.index.cpu().numpy(), idx) and np.array_equal(nb.score.cpu().numpy().view(np.uint32), sc.view(np.uint32))
    assert np.array_equal(nb.count.cpu().numpy(), (keys != 0).sum(axis=1))
    filled = keys[:, 1:] != 0
    assert (keys[:, :-1][filled] > keys[:, 1:][filled]).all()
    assert ((keys[:, :-1] != 0) | (keys[:, 1:] == 0)).all()              # the empty slots are last
    s, i = sc[:, :-1][filled], idx[:, :-1][filled]
    s2, i2 = sc[:, 1:][filled], idx[:, 1:][filled]
    assert ((s > s2) | ((s == s2) & (i < i2))).all()


# ------------------------------------------------------------------------------------------------ 1. the scores
@pytest.mark.parametrize("D,M,Nq,k", [(768, 257, 65, 20), (32, 65, 17, 64), (1024, 64, 1, 5)])
def test_scores_are_cluster_assign_bits(model, D, M, Nq, k):
    q, b, _ = case(D, M, Nq)
    qd, bd = dev(q), dev(b)
    full = np.empty((Nq, M), np.float32)
    for r in range(M):
        _, best, _, _ = model.cluster_assign(qd, bd[r:r + 1], normalize=False)
        full[:, r] = best.cpu().numpy()
    nb = topk(model, qd, bd, k)
    assert np.array_equal(nb.keys_numpy(), topk_numpy(full, k))
    check_consistent(nb)
    assert nb.k == k and nb.n_bank == M and int(nb.query_skipped) == 0 and int(nb.bank_skipped) == 0


# ------------------------------------------------------------------------------------------------ 2. float64
F64_CASES = [(768, 4099, 257, 20), (32, 4099, 65, 64), (1024, 257, 63, 5), (768, 1, 1, 1), (768, 63, 3, 64)]


@pytest.mark.parametrize("D,M,Nq,k", F64_CASES)
def test_lists_against_float64(model, D, M, Nq, k):
    q, b, s64 = case(D, M, Nq)
    nb = topk(model, q, b, k)
    check_consistent(nb)
    idx, sc, cnt = nb.index.cpu().numpy(), nb.score.cpu().numpy(), nb.count.cpu().numpy()
    bd = bound(D)
    kk = min(k, M)
    assert (cnt == kk).all() and (idx[:, :kk] >= 0).all()
    if kk < k:
        assert (idx[:, kk:] == -1).all() and (sc[:, kk:] == 0).all()
        assert (np.sort(idx[:, :kk], axis=1) == np.arange(M)).all()      # every bank row is present
    t = np.sort(s64, axis=1)[:, M - kk]                                  # the float64 k-th largest
    rows = np.arange(Nq)[:, None]
    got64 = s64[rows, idx[:, :kk]]
    assert np.abs(sc[:, :kk].astype(np.float64) - got64).max() <= bd
    assert (got64 >= t[:, None] - 2 * bd).all()
    sure = s64 > t[:, None] + 2 * bd
    hit = np.zeros_like(sure)
    hit[rows, idx[:, :kk]] = True
    assert (hit | ~sure).all()


# ------------------------------------------------------------------------------------------------ 3. split invariance
def chunked(model, q, b, k, chunk, reverse=False, **kw):
    nb = None
    for c0 in list(range(0, b.shape[0], chunk))[::-1 if reverse else 1]:
        nb = topk(model, q, b[c0:c0 + chunk], k, bank_base=c0, into=nb, **kw)
    return nb


@pytest.mark.parametrize("D,M,Nq,k", [(32, 2100, 65, 20), (768, 300, 17, 64)])
def test_split_invariance(model, D, M, Nq, k):
    q, b, _ = case(D, M, Nq)
    qd, bd = dev(q), dev(b)
    whole = topk(model, qd, bd, k)
    for chunk in (63, 64, 65, 1000):
        for reverse in (False, True):
            nb = chunked(model, qd, bd, k, chunk, reverse)
            assert torch.equal(nb.keys, whole.keys), (chunk, reverse)
            assert nb.n_bank == M
        check_consistent(nb)
    for cut in (1, 17, 64):
        if cut < Nq:
            parts = [topk(model, qd[:cut], bd, k), topk(model, qd[cut:], bd, k)]
            assert torch.equal(torch.cat([p.keys for p in parts]), whole.keys), cut
    for segments in (1, 2, 7, 0, 40):                                    # 40 is above the number of bank tiles: empty segments
        assert torch.equal(topk(model, qd, bd, k, segments=segments).keys, whole.keys), segments
    got = model.topk_batches(qd, [bd[c0:c0 + 500] for c0 in range(0, M, 500)], k)
    assert torch.equal(got.keys, model.topk(qd, bd, k).keys) and got.n_bank == M
    check_consistent(got)
    # keep_topk_merge of two halves, through Neighbours.merge and in place through the ABI
    h = M // 2 + 1
    lo, hi = topk(model, qd, bd[:h], k), topk(model, qd, bd[h:], k, bank_base=h)
    merged = lo.merge(hi)
    assert torch.equal(merged.keys, whole.keys) and merged.n_bank == M
    assert np.array_equal(merge_numpy(lo.keys_numpy(), hi.keys_numpy()), whole.keys_numpy())
    a = lo.keys.clone()
    rc = _lib.load().keep_topk_merge(model._handle, _ptr(a), _ptr(hi.keys), Nq, k, _ptr(a), _stream(torch.device(DEV)))
    assert rc == _lib.KEEP_OK and torch.equal(a, whole.keys)


def test_chunks_of_one_row(model):
    q, b, _ = case(32, 70, 17)
    qd, bd = dev(q), dev(b)
    for k in (1, 5, 64):
        whole = topk(model, qd, bd, k)
        assert torch.equal(chunked(model, qd, bd, k, 1).keys, whole.keys)
        assert torch.equal(chunked(model, qd, bd, k, 1, reverse=True).keys, whole.keys)


# ------------------------------------------------------------------------------------------------ 4. planted ties
@pytest.mark.parametrize("k", [1, 5, 64])
def test_planted_ties(model, k):
    q, b, _ = case(32, 300, 3)
    i, j = 10, 150                                                       # different 64-row tiles, chunks and (below) segments
    plant = np.array(b)
    plant[i] = plant[j] = q[0]                                           # the best score of query 0, twice
    runs = {"resident": topk(model, q, plant, k), "chunks": chunked(model, dev(q), dev(plant), k, 64),
            "chunks reversed": chunked(model, dev(q), dev(plant), k, 64, reverse=True), "segments": topk(model, q, plant, k, segments=4)}
    first = runs["resident"]
    check_consistent(first)
    idx, sc = first.index.cpu().numpy(), first.score.cpu().numpy()
    assert idx[0, 0] == i                                                # of equal scores the lower row comes first
    if k > 1:
        assert idx[0, 1] == j and sc[0, 0].view(np.uint32) == sc[0, 1].view(np.uint32)
    else:
        assert j not in idx[0]                                           # the pair straddles rank k: i is kept, j is not
    for name, nb in runs.items():
        assert torch.equal(nb.keys, first.keys), name
    # the pair straddling rank k: a copy of the k-th neighbour at a higher row stays out, and the list is what it was
    base = topk(model, q, b, k)
    bi = base.index.cpu().numpy()
    kth = int(bi[0, k - 1])
    later = [r for r in range(kth + 1, 300) if r not in bi[0]]
    assert later
    plant = np.array(b)
    plant[later[0]] = plant[kth]
    for nb in (topk(model, q, plant, k), chunked(model, dev(q), dev(plant), k, 64), topk(model, q, plant, k, segments=4)):
        assert np.array_equal(nb.keys_numpy()[0], base.keys_numpy()[0])


# ------------------------------------------------------------------------------------------------ 5. the skip rule
def test_skip_rule(model):
    D, M, Nq, k = 32, 200, 20, 20
    q, b, _ = case(D, M, Nq)
    clean = device_scores(model, q, b)
    assert np.isfinite(clean).all()
    bq, bb = np.array(q), np.array(b)
    bq[7, 5] = np.nan
    bb[0, 3], bb[63, 31], bb[64, 0] = np.nan, np.inf, 1.5                # the first and last row of a tile, the first of the next
    bb[128:192, 17] = -1.5                                               # a whole 64-row tile
    bad_rows = [0, 63, 64] + list(range(128, 192))
    want = clean.copy()
    want[:, bad_rows] = np.nan
    want[7] = np.nan
    for kw in ({}, {"segments": 3}):
        nb = topk(model, bq, bb, k, **kw)
        check_consistent(nb)
        assert np.array_equal(nb.keys_numpy(), topk_numpy(want, k))
        assert int(nb.count[7]) == 0 and not np.isin(nb.index.cpu().numpy(), bad_rows).any()
        assert int(nb.query_skipped) == 1 and int(nb.bank_skipped) == len(bad_rows)
    # with into= the bad query's list stays what it was, and the counters run on
    other = unit_rows(70, D, 9)
    before = topk(model, q, other, k, bank_base=1000)
    after = topk(model, bq, bb, k, into=before)
    assert torch.equal(after.keys[7], before.keys[7]) and int(before.count[7]) == k
    rest = np.arange(Nq) != 7
    assert np.array_equal(after.keys_numpy()[rest], merge_numpy(before.keys_numpy(), topk_numpy(want, k))[rest])
    assert int(after.bank_skipped) == len(bad_rows) and after.n_bank == 1070
    chunks = chunked(model, dev(bq), dev(bb), k, 64)
    assert int(chunks.query_skipped) == 1 and int(chunks.bank_skipped) == len(bad_rows) and torch.equal(chunks.keys, nb.keys)
    # every bank row bad
    bb[:, 1] = 2.0
    nb = topk(model, bq, bb, k)
    assert int(nb.keys.ne(0).sum()) == 0 and int(nb.count.sum()) == 0 and (nb.index == -1).all() and (nb.score == 0).all()
    assert int(nb.bank_skipped) == M


# ------------------------------------------------------------------------------------------------ 6. exclude_self
@pytest.mark.parametrize("D,N", [(768, 257), (32, 65)])
def test_exclude_self(model, D, N):
    x = dev(unit_rows(N, D, 77))
    own = np.arange(N)[:, None]
    for k in (1, 20, 64):
        nb = topk(model, x, x, k, exclude_self=True)
        check_consistent(nb)
        assert not (nb.index.cpu().numpy() == own).any()
        assert (nb.count.cpu().numpy() == min(k, N - 1)).all()
        if k + 1 <= 64:
            more = topk(model, x, x, k + 1).keys_numpy()
            idx, _ = unpack_keys_numpy(more)
            want = np.stack([row[i != r][:k] for r, (row, i) in enumerate(zip(more, idx))])
            assert np.array_equal(nb.keys_numpy(), want)
        got = model.topk_batches(x, [x[c0:c0 + 64] for c0 in range(0, N, 64)], k, normalize=False, self_first=0)
        assert torch.equal(got.keys, nb.keys)


# ------------------------------------------------------------------------------------------------ 7. the vote
_lists = {}


def vote_lists(model, D, M, Nq, k):
    key = (D, M, Nq, k)
    if key not in _lists:
        q, b, _ = case(D, M, Nq)
        _lists[key] = topk(model, q, b, k)
    return _lists[key]


@pytest.mark.parametrize("C", [2, 3, 64])
@pytest.mark.parametrize("D,M,Nq,k", F64_CASES[:2])
def test_vote(model, D, M, Nq, k, C):
    nb = vote_lists(model, D, M, Nq, k)
    idx, sc = nb.index.cpu().numpy(), nb.score.cpu().numpy()
    labels = np.random.default_rng(C).integers(-1, C, M).astype(np.int32)
    labels[idx[9, :k // 2]], labels[idx[9, k // 2:]] = 1, 0               # a two-way tie: the lower class wins
    labels[idx[5]] = -1                                                  # a query whose neighbours are all unlabelled
    want = knn_vote_numpy(idx, sc, labels, C, "uniform")
    assert want[0][5] == -1 and want[3] >= 1 and (want[2][want[0] >= 0] == 0).any()
    got = model.knn_vote(nb, labels, C, weights="uniform")
    assert np.array_equal(got[0].cpu().numpy(), want[0])
    assert np.array_equal(got[1].cpu().numpy(), want[1])
    assert np.array_equal(got[2].cpu().numpy(), want[2])
    assert int(got[3]) == want[3]
    if not np.isin(idx[5], idx[9]).any():
        assert want[0][9] == 0 and want[2][9] == 0
    for T in (0.07, 1.0):
        want = knn_vote_numpy(idx, sc, labels, C, "softmax", T)
        got = model.knn_vote(nb, labels, C, weights="softmax", temperature=T)
        gl, gp = got[0].cpu().numpy(), got[1].cpu().numpy()
        assert (np.abs(gp - want[1]) <= 1e-5 * np.abs(want[1]) + 1e-7).all()
        assert np.array_equal(gl < 0, want[0] < 0) and int(got[3]) == want[3]
        clear = want[2] >= 2e-5                                          # the restated lead
        voted = want[0] >= 0
        assert (~clear & voted).sum() <= 0.01 * Nq
        assert np.array_equal(gl[clear & voted], want[0][clear & voted])
        assert (np.abs(got[2].cpu().numpy() - want[2]) <= 2.1e-5)[clear & voted].all()       # two shares, each within the bound above


# ------------------------------------------------------------------------------------------------ 8. the consumers
def test_knn_probe_matches_scikit_learn(model):
    from sklearn.neighbors import KNeighborsClassifier
    x, y = blobs([300, 200, 150, 100], 768, 0.05, 0)
    h = len(x) // 2
    res = tile_eval.knn_probe(model, dev(x[:h]), y[:h], dev(x[h:]), y[h:], 4, k=20, weights="uniform", n_boot=200, seed=3)
    clf = KNeighborsClassifier(n_neighbors=20, metric="cosine", algorithm="brute").fit(x[:h], y[:h])
    pred = clf.predict(x[h:])
    conf = np.bincount(y[h:] * 4 + pred, minlength=16).reshape(4, 4)
    assert np.array_equal(res["confusion"], conf)
    assert isinstance(res["neighbours"], Neighbours) and res["skipped"] == 0
    assert np.array_equal(res["labels"].cpu().numpy(), pred)
    assert res["balanced_accuracy_ci"].estimate == pytest.approx(res["balanced_accuracy"], abs=1e-12)
    assert res["weighted_f1_ci"].estimate == pytest.approx(res["weighted_f1"], abs=1e-12)
    diff = res["balanced_accuracy_ci"].minus(res["weighted_f1_ci"])       # paired by seed
    assert len(diff.values) == 200
    per_class, macro = res["ovr_roc"]
    assert len(per_class) == 4 and 0.5 < macro.estimate <= 1.0
    # training rows labelled -1 take no neighbour slot
    y2 = y[:h].copy()
    y2[::3] = -1
    res2 = tile_eval.knn_probe(model, dev(x[:h]), y2, dev(x[h:]), y[h:], 4, k=20, weights="uniform", n_boot=0)
    assert res2["neighbours"].n_bank == int((y2 >= 0).sum()) and (res2["neighbours"].count == 20).all()
    assert res2["balanced_accuracy_ci"] is None and res2["ovr_roc"] is None


def test_knn_map_and_search_tiles(model):
    gw, gh, P, d = 12, 9, 256, 16
    shape = (gh * P // d, gw * P // d)
    x, truth = blobs([70, 38], 768, 0.02, 17)
    tx, ty = blobs([40, 30], 768, 0.02, 17)                              # the same centres
    x = x.copy()
    x[50, 3] = np.nan
    coords = np.stack([np.arange(gw * gh) % gw * P, np.arange(gw * gh) // gw * P], axis=1).astype(np.int64)
    raster = wsi.knn_map(dev(tx), ty, 2, dev(x), torch.from_numpy(coords), d, shape, patch_size=P, k=5, model=model)
    assert isinstance(raster, ClassRaster) and raster.n_classes == 2 and raster.shape == shape and raster.tiles == gw * gh - 1
    nb = model.topk(dev(x), dev(tx), 5)
    labels, probs, _, _ = model.knn_vote(nb, ty, 2)
    keep = labels.cpu().numpy() >= 0
    assert keep.sum() == gw * gh - 1 and not keep[50]
    want = class_raster_numpy(coords[keep], probs.cpu().numpy()[keep], P, d, shape)
    assert torch.equal(raster.acc.cpu(), torch.from_numpy(want))
    assert (labels.cpu().numpy()[keep] == truth[keep]).all()
    votes = wsi.knn_map(dev(tx), ty, 2, dev(x), torch.from_numpy(coords), d, shape, patch_size=P, k=5, weights="uniform", vote=True, model=model)
    voted = model.knn_vote(nb, ty, 2, weights="uniform")[0].cpu().numpy()
    assert np.array_equal(voted >= 0, keep)
    want = class_raster_numpy(coords[keep], one_hot_numpy(voted[keep], 2), P, d, shape)
    assert torch.equal(votes.acc.cpu(), torch.from_numpy(want))
    assert model.class_map(raster).slide_label(drop_last=False) == 0
    # search: two prompts-like queries and a query with a NaN against the slide's tiles
    queries = np.stack([tx[0], tx[1], x[50]])
    index, score, found = wsi.search_tiles(dev(queries), dev(x), 50, tile_coords=torch.from_numpy(coords), model=model)
    idx = index.cpu().numpy()
    assert tuple(found.shape) == (3, 50, 2) and (idx[2] == -1).all() and (idx[:2] >= 0).all() and 50 not in idx
    want = np.where((idx >= 0)[..., None], coords[np.maximum(idx, 0)], -1)
    assert np.array_equal(found.cpu().numpy(), want)
    index2, _, none = wsi.search_tiles(dev(x[:40]), dev(x[:40]), 64, exclude_self=True, model=model)
    assert none is None and not (index2.cpu().numpy() == np.arange(40)[:, None]).any() and int((index2[:, 39:] >= 0).sum()) == 0


# ------------------------------------------------------------------------------------------------ 9. arguments
def test_abi_errors_launch_nothing(model):
    lib, h, st = _lib.load(), model._handle, _stream(torch.device(DEV))
    Nq, M, D, k = 8, 70, 32, 5
    q, b = dev(unit_rows(Nq, D, 0)), dev(unit_rows(M + 1, D, 1))
    keys = torch.full((Nq, k), 77, dtype=torch.int64, device=DEV)
    qs, bs = (torch.full((1,), 5, dtype=torch.int64, device=DEV) for _ in range(2))
    good = topk(model, q, b[:M], k)
    labels = torch.zeros(M, dtype=torch.int32, device=DEV)
    probs = torch.full((Nq, 3), 7.0, dtype=torch.float32, device=DEV)
    lab = torch.full((Nq,), 77, dtype=torch.int32, device=DEV)
    index = torch.full((Nq, k), 77, dtype=torch.int64, device=DEV)
    null = C_.c_void_p(0)
    off4 = lambda t: C_.c_void_p(t.data_ptr() + 4)

    def search(q_=_ptr(q), nq=Nq, b_=_ptr(b), m=M, d=D, k_=k, base=0, sf=-1, merge=0, keys_=_ptr(keys), segments=0):
        return lib.keep_topk(h, q_, nq, b_, m, d, k_, base, sf, merge, keys_, _ptr(qs), _ptr(bs), segments, st)

    def vote(keys_=_ptr(good.keys), k_=k, y=_ptr(labels), n=M, c=3, mode=1, T=0.07, p=_ptr(probs)):
        return lib.keep_knn_vote(h, keys_, Nq, k_, y, n, c, mode, T, p, _ptr(lab), null, _ptr(qs), st)

    def unpack(keys_=_ptr(good.keys), k_=k, i=_ptr(index)):
        return lib.keep_topk_unpack(h, keys_, Nq, k_, i, null, null, st)

    def merge(a=_ptr(good.keys), b_=_ptr(good.keys), k_=k, out=_ptr(keys)):
        return lib.keep_topk_merge(h, a, b_, Nq, k_, out, st)

    bad = [lambda: search(k_=0), lambda: search(k_=65), lambda: search(d=24), lambda: search(q_=off4(q)), lambda: search(b_=off4(b)),
           lambda: search(keys_=off4(keys)), lambda: search(base=(1 << 32) - M), lambda: search(base=-1), lambda: search(segments=1025),
           lambda: search(segments=-1), lambda: search(nq=0), lambda: search(m=0), lambda: search(m=(1 << 22) + 1), lambda: search(merge=2),
           lambda: search(q_=null), lambda: search(keys_=null),
           lambda: vote(c=1), lambda: vote(c=65), lambda: vote(T=0.0), lambda: vote(mode=2), lambda: vote(k_=0), lambda: vote(y=null),
           lambda: vote(n=int(good.index.max())),                          # a key index >= n_bank
           lambda: vote(keys_=off4(good.keys)), lambda: vote(n=0),
           lambda: unpack(k_=65), lambda: unpack(keys_=null), lambda: unpack(i=off4(index)),
           lambda: merge(k_=0), lambda: merge(a=null), lambda: merge(out=off4(keys))]
    for i, call in enumerate(bad):
        assert call() == _lib.KEEP_EINVAL, f"bad call {i}"
        assert len(lib.keep_last_error(h)) > 10, f"bad call {i}"
    assert lib.keep_topk(None, _ptr(q), Nq, _ptr(b), M, D, k, 0, -1, 0, _ptr(keys), null, null, 0, st) == _lib.KEEP_EINVAL
    torch.cuda.synchronize()
    assert (keys == 77).all() and int(qs) == 5 and int(bs) == 5 and (probs == 7.0).all() and (lab == 77).all() and (index == 77).all()
    # the Python layer says the same before anything is launched
    for call in (lambda: topk(model, q, b, 0), lambda: topk(model, q, b, 65), lambda: topk(model, q, dev(unit_rows(4, 24, 0)), 5),
                 lambda: topk(model, q, b, 5, bank_base=(1 << 32) - 8), lambda: topk(model, q, b, 5, segments=1025),
                 lambda: topk(model, q, b, 5, exclude_self=True), lambda: topk(model, q, b[:M], 6, into=good),
                 lambda: model.knn_vote(good, labels, 1), lambda: model.knn_vote(good, labels, 3, temperature=0.0),
                 lambda: model.knn_vote(good, labels, 3, weights="distance"), lambda: model.knn_vote(good, labels[:M - 1], 3)):
        with pytest.raises(ValueError):
            call()
    # and the same arguments, sound, go through; the largest base the keys can hold too
    assert search() == _lib.KEEP_OK and vote() == _lib.KEEP_OK and unpack() == _lib.KEEP_OK and merge() == _lib.KEEP_OK
    assert search(base=(1 << 32) - 1 - M) == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert int(keys.view(-1)[0]) & 0xFFFFFFFF <= M                       # 0xFFFFFFFF - g with g >= 2^32 - 1 - M
