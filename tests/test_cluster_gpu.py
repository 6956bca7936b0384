"""Tile clustering on the MI355X: keep_cluster_assign / keep_cluster_update / keep_cluster_seed_step,
KEEPModel.cluster_assign / cluster_update / cluster_seed / cluster_tiles / cluster_fit_batches and wsi.cluster_map.

The yardsticks are the restatements of keep_amd.cluster, which tests/test_cluster.py holds to per-tile Python loops.  The scores are
fp32 fma chains of length D over unit vectors, so a score lies within D * 2^-24 of float64 (sum |a b| <= 1) and a difference of two
within twice that: labels are compared where the float64 margin is at least that bound, and every case asserts on the host that at
most 1 % of its tiles fall under it.  The accumulators are integers and are compared exactly."""
import ctypes as C_

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel, _lib, wsi
from keep_amd.classmap import ClassRaster, class_raster_numpy, one_hot_numpy
from keep_amd.cluster import (ClusterSums, TileClusters, accumulate_numpy, assign_numpy, kmeans_numpy, seed_numpy, update_numpy)
from keep_amd.config import small_shape
from keep_amd.model import _ptr, _stream
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


# (D, K, N, seed): the seed is one for which the float64 margins leave at most 1 % of the tiles under the bound (asserted below)
ASSIGN_CASES = [(768, 16, 4099, 0), (768, 64, 257, 0), (768, 17, 65, 1), (768, 3, 64, 0), (768, 1, 63, 0), (768, 2, 1, 0),
                (32, 64, 4099, 0), (32, 3, 65, 0), (32, 1, 1, 0), (1024, 17, 257, 1), (1024, 64, 63, 1), (1024, 2, 64, 0)]
_cases = {}


def assign_case(D, K, N, seed):
    """Random unit rows and centroids with the float64 assign, computed once and shared (never written to)."""
    key = (D, K, N, seed)
    if key not in _cases:
        x, c = unit_rows(N, D, 100 + seed), unit_rows(K, D, 200 + seed)
        want = assign_numpy(x, c)
        for a in (x, c) + want:
            a.setflags(write=False)
        _cases[key] = (x, c) + want
    return _cases[key]


@pytest.mark.parametrize("D,K,N,seed", ASSIGN_CASES)
def test_assign_matches_float64(model, D, K, N, seed):
    x, c, wl, wb, wm = assign_case(D, K, N, seed)
    sure = (wm >= 2 * bound(D)) | (K == 1)
    assert (~sure).sum() <= N // 100, f"{(~sure).sum()} of {N} tiles under the margin bound: choose another seed"
    labels, best, margin, skipped = model.cluster_assign(dev(x), dev(c), normalize=False)
    assert labels.dtype == torch.int32 and best.dtype == margin.dtype == torch.float32 and int(skipped) == 0
    gl, gb, gm = labels.cpu().numpy(), best.cpu().numpy().astype(np.float64), margin.cpu().numpy().astype(np.float64)
    print(f"D={D} K={K} N={N}: left out {(~sure).sum()}, label mismatches {(gl != wl)[sure].sum()}, "
          f"best err {np.abs(gb - wb).max():.3g} (bound {bound(D):.3g}), margin err {np.abs(gm - wm).max():.3g}")
    assert (gl[sure] == wl[sure]).all() and (gl >= 0).all() and (gl < K).all()
    assert np.abs(gb - wb).max() <= bound(D)
    assert np.abs(gm - wm).max() <= 2 * bound(D)
    if K == 1:
        assert (gm == 0).all()


@pytest.mark.parametrize("D,K,N", [(768, 17, 257), (32, 64, 65), (1024, 3, 64)])
def test_planted_ties_go_to_the_lower_index(model, D, K, N):
    x, c = unit_rows(N, D, 1).copy(), unit_rows(K, D, 2).copy()
    pairs = [(0, K - 1)] + ([(1, 2)] if K > 3 else [])                   # centroid j a copy of centroid i < j: no tile may get j
    for i, j in pairs:
        c[j] = c[i]
    x[5] = c[1]                                                          # a row that is a copy of a centroid
    x[N - 1] = c[0]
    labels, best, margin, _ = model.cluster_assign(dev(x), dev(c), normalize=False)
    gl = labels.cpu().numpy()
    assert not np.isin(gl, [j for _, j in pairs]).any()
    assert gl[5] == 1 and gl[N - 1] == 0
    assert abs(float(best[5]) - 1) <= bound(D) and abs(float(best[N - 1]) - 1) <= bound(D)
    twins = np.isin(gl, [i for i, _ in pairs])
    assert (margin.cpu().numpy()[twins] == 0).all()                      # the runner-up of a twin's tile is the bit-equal copy


def spoiled(N, D, seed):
    """Unit rows with a NaN, an inf and a 1.5 planted -> (x, the spoiled rows)."""
    x = unit_rows(N, D, seed).copy()
    bad = sorted({0, N // 3, N // 2, N - 1} if N >= 4 else set())
    for i, r in enumerate(bad):
        x[r, (7 * i) % D] = (np.nan, np.inf, 1.5, -np.inf)[i % 4]
    return x, np.asarray(bad, np.int64)


def test_position_and_split_invariance_is_bit_exact(model):
    N, D, K = 4099, 768, 17
    x, bad = spoiled(N, D, 3)
    c = unit_rows(K, D, 4)
    prev = np.random.default_rng(5).integers(-1, K, N).astype(np.int32)
    xd, cd, pd = dev(x), dev(c), dev(prev)
    whole = ClusterSums(K, D, DEV)
    l1, b1, m1, _ = model.cluster_assign(xd, cd, sums=whole, prev=pd, normalize=False)
    assert whole.tiles == N and int(whole.skipped) == len(bad) and (l1[dev(bad)] == -1).all()
    parts = ClusterSums(K, D, DEV)
    got, at = [], 0
    for n in (1, 63, 1000, 3035):
        got.append(model.cluster_assign(xd[at:at + n], cd, sums=parts, prev=pd[at:at + n], normalize=False))
        at += n
    assert at == N
    for j, one in enumerate((l1, b1, m1)):
        assert torch.equal(torch.cat([g[j] for g in got]), one)
    assert torch.equal(parts.buf, whole.buf)
    lr, br, mr, _ = model.cluster_assign(xd.flip(0).contiguous(), cd, normalize=False)
    assert torch.equal(lr.flip(0), l1) and torch.equal(br.flip(0), b1) and torch.equal(mr.flip(0), m1)
    # the two-launch form adds the same words
    two = ClusterSums(K, D, DEV)
    l2, b2, m2, _ = model.cluster_assign(xd, cd, sums=two, prev=pd, normalize=False, fused=False)
    assert torch.equal(l2, l1) and torch.equal(b2, b1) and torch.equal(m2, m1) and torch.equal(two.buf, whole.buf)


# N = 32771 and 262147 are past the sizes at which a workgroup takes two and four groups of 64 rows; K = 64 takes four from 32768 on
@pytest.mark.parametrize("N,D,K", [(4099, 768, 64), (4099, 768, 1), (32771, 32, 5), (32771, 32, 64), (262147, 16, 3)])
def test_accumulate_is_integer_exact(model, N, D, K):
    x, bad = spoiled(N, D, 6)
    c = unit_rows(K, D, 7)
    prev = np.random.default_rng(8).integers(-1, K, N).astype(np.int32)
    sums = ClusterSums(K, D, DEV)
    labels, best, margin, skipped = model.cluster_assign(dev(x), dev(c), sums=sums, prev=dev(prev), normalize=False)
    gl, gb = labels.cpu().numpy(), best.cpu().numpy()
    assert (gl[bad] == -1).all() and (gb[bad] == 0).all() and (margin.cpu().numpy()[bad] == 0).all()
    assert ((gl == -1).sum(), int(skipped)) == (len(bad), len(bad))
    ws, wc, wcos, wch, wsk = accumulate_numpy(x, gl, gb, K, prev)
    assert torch.equal(sums.sums.cpu(), torch.from_numpy(ws)) and torch.equal(sums.counts.cpu(), torch.from_numpy(wc))
    assert (int(sums.cos_sum), int(sums.changed), int(sums.skipped)) == (wcos, wch, wsk)
    assert int(sums.counts.sum()) == N - len(bad)
    if K == 64 and N == 4099:
        assert (wc > 0).all()                                            # every label in every block: the contended shape
    # the labels themselves, where float64 can vouch for them
    wl, _, wm = assign_numpy(x, c)
    sure = (wm >= 2 * bound(D)) | (wl < 0) | (K == 1)
    assert (~sure).sum() <= N // 100 and (gl[sure] == wl[sure]).all()
    two = ClusterSums(K, D, DEV)
    model.cluster_assign(dev(x), dev(c), sums=two, prev=dev(prev), normalize=False, fused=False)
    assert torch.equal(two.buf, sums.buf)


@pytest.mark.parametrize("N,D,K", [(4099, 768, 16), (65, 32, 64), (257, 1024, 3)])
def test_update_matches_float64_and_keeps_an_empty_cluster(model, N, D, K):
    x, c = unit_rows(N, D, 9), unit_rows(K, D, 10).copy()
    c[K - 1] = c[0]                                                      # a copy of centroid 0 never wins: cluster K - 1 is emptied
    sums = ClusterSums(K, D, DEV)
    model.cluster_assign(dev(x), dev(c), sums=sums, normalize=False)
    cd = dev(c)
    new, empty = model.cluster_update(sums, cd)
    assert torch.equal(cd.cpu(), torch.from_numpy(c))                    # the input is not written
    want, wempty = update_numpy(sums.sums.cpu().numpy(), sums.counts.cpu().numpy(), c)
    assert empty.dtype == torch.uint8 and empty.cpu().numpy().tolist() == wempty.tolist() and wempty[K - 1] == 1
    got = new.cpu().numpy()
    print(f"N={N} D={D} K={K}: update err {np.abs(got.astype(np.float64) - want.astype(np.float64)).max():.3g} (bound {2.0 ** -23:.3g})")
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -23
    for k in np.flatnonzero(wempty):
        assert got[k].tobytes() == c[k].tobytes()


def seed_inputs(which):
    if which == "blobs":                                                 # five blobs and, opposite their mean, three bit-equal rows
        x, _ = blobs([150, 120, 100, 80, 47], 768, 0.02, 12)
        x = x.copy()
        far = -x.astype(np.float64).sum(axis=0)
        x[[40, 200, 333]] = (far / np.linalg.norm(far)).astype(np.float32)
        x[7, 100] = np.nan
        return x, 6
    return unit_rows(65, 32, 13), 4


@pytest.mark.parametrize("which", ["blobs", "small"])
def test_seeding_matches_the_restatement(model, which):
    x, k = seed_inputs(which)
    D = x.shape[1]
    gaps = []
    want = seed_numpy(x, k, gaps)
    assert min(gaps) > 2 * bound(D), f"a float64 gap of {min(gaps):.3g} is under the bound {2 * bound(D):.3g}: choose other inputs"
    got = model.cluster_seed(dev(x), k, normalize=False)
    assert got.dtype == torch.int64 and got.device == torch.device(DEV) and got.cpu().numpy().tolist() == want.tolist()
    if which == "blobs":
        assert 40 in want and 200 not in want and 333 not in want and 7 not in want      # of bit-equal rows the lowest index


_loop = {}


def loop_data():
    """Five planted blobs in D = 768, N = 2000; blobs 0 and 1 have two modes each, which is what k = 7 finds."""
    if not _loop:
        g = np.random.default_rng(14)
        sizes = [500, 450, 400, 350, 300]
        centres = unit_rows(5, 768, 15).astype(np.float64)
        modes = unit_rows(2, 768, 16).astype(np.float64)
        truth = g.permutation(np.repeat(np.arange(5), sizes))
        x = centres[truth] + 0.01 * g.standard_normal((2000, 768))
        for b in (0, 1):
            rows = np.flatnonzero(truth == b)
            x[rows] += 0.45 * modes[b] * np.where(np.arange(len(rows)) % 2 == 0, 1.0, -1.0)[:, None]
        x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
        x.setflags(write=False)
        _loop["x"], _loop["truth"] = x, truth
        for k in (5, 7):
            _loop[k] = kmeans_numpy(x, k)
    return _loop


@pytest.mark.parametrize("k", [5, 7])
def test_the_loop_follows_the_restatement(model, k):
    d = loop_data()
    x, want = d["x"], d[k]
    assert want["min_margin"] > 1e-3 and want["converged"], f"float64 margin {want['min_margin']:.3g} along the trajectory"
    if k == 5:
        assert all(len(set(want["labels"][d["truth"] == b].tolist())) == 1 for b in range(5))
    got = model.cluster_tiles(dev(x), k)
    assert isinstance(got, TileClusters) and got.k == k and got.labels.device == torch.device(DEV)
    assert got.labels.cpu().numpy().tolist() == want["labels"].tolist()
    assert got.counts.cpu().numpy().tolist() == want["counts"].tolist()
    assert (got.n_iter, got.converged, got.changed, got.skipped) == (want["n_iter"], want["converged"], want["changed"], want["skipped"])
    assert not got.empty.any() and got.kept().all()
    print(f"k={k}: n_iter {got.n_iter}, mean cosine {got.mean_cosine:.9f} vs {want['mean_cosine']:.9f}, min margin {want['min_margin']:.3g}")
    assert abs(got.mean_cosine - want["mean_cosine"]) <= bound(768)
    again = model.cluster_tiles(dev(x), k)                               # two runs in one process
    for a, b in ((again.labels, got.labels), (again.centroids, got.centroids), (again.counts, got.counts), (again.best, got.best)):
        assert torch.equal(a, b)
    if k == 5:
        # stopped after one iteration: not converged, and the labels are a last assign against the updated centroids
        short, wshort = model.cluster_tiles(dev(x), k, max_iter=1), kmeans_numpy(x, k, max_iter=1)
        assert (short.n_iter, short.converged, short.changed) == (1, False, wshort["changed"]) and wshort["min_margin"] > 1e-3
        assert short.labels.cpu().numpy().tolist() == wshort["labels"].tolist()
        assert np.abs(short.centroids.cpu().numpy().astype(np.float64) - wshort["centroids"]).max() <= 2.0 ** -23
        # three uneven batches, from the same seeds
        idx = model.cluster_seed(dev(x), k)
        cen0 = model.cluster_tiles(dev(x), k, init=idx, max_iter=0).centroids
        cuts = [0, 1, 700, 2000]
        calls = []

        def batches():
            calls.append(1)
            return [torch.from_numpy(np.array(x[a:b])) for a, b in zip(cuts[:-1], cuts[1:])]
        fit = model.cluster_fit_batches(batches, k, cen0)
        assert len(calls) == fit.n_iter == got.n_iter and fit.converged
        assert torch.equal(fit.labels, got.labels) and torch.equal(fit.centroids, got.centroids) and torch.equal(fit.counts, got.counts)
        assert torch.equal(fit.best, got.best) and fit.mean_cosine == got.mean_cosine


def test_cluster_map_rasterises_the_labels(model):
    gw, gh, P, d = 12, 9, 256, 16
    shape = (gh * P // d, gw * P // d)
    x, truth = blobs([70, 38], 768, 0.02, 17)
    x = x.copy()
    coords = np.stack([np.arange(gw * gh) % gw * P, np.arange(gw * gh) // gw * P], axis=1).astype(np.int64)
    nan_tile = 50
    x[nan_tile, 3] = np.nan
    raster, res = wsi.cluster_map(dev(x), torch.from_numpy(coords), 2, d, shape, patch_size=P, model=model)
    assert isinstance(raster, ClassRaster) and isinstance(res, TileClusters) and raster.n_classes == 2 and raster.shape == shape
    gl = res.labels.cpu().numpy()
    keep = gl >= 0
    assert res.skipped == 1 and not keep[nan_tile] and keep.sum() == gw * gh - 1 and raster.tiles == gw * gh - 1
    want = class_raster_numpy(coords[keep], one_hot_numpy(gl[keep], 2), P, d, shape)
    assert torch.equal(raster.acc.cpu(), torch.from_numpy(want))
    # the tiles of a blob share a label, and the slide's label is the larger blob's
    first = {b: int(gl[np.flatnonzero((truth == b) & keep)[0]]) for b in (0, 1)}
    assert first[0] != first[1] and all((gl[(truth == b) & keep] == first[b]).all() for b in (0, 1))
    cm = model.class_map(raster)
    assert cm.slide_label(drop_last=False) == first[0]
    y0, x0 = coords[nan_tile, 1] // d, coords[nan_tile, 0] // d
    assert int(raster.acc[:, y0:y0 + P // d, x0:x0 + P // d].abs().sum()) == 0
    assert (cm.labels[y0:y0 + P // d, x0:x0 + P // d] == 255).all()
    regions = wsi.subtype_regions(cm, model=model)
    assert sorted(regions) == [0, 1]
    # the centroids of the fit instead of k: the same labels, nothing fitted
    raster2, res2 = wsi.cluster_map(dev(x), torch.from_numpy(coords), res.centroids, d, shape, patch_size=P, model=model)
    assert torch.equal(res2.labels, res.labels) and torch.equal(raster2.acc, raster.acc) and res2.n_iter == 0
    assert torch.equal(res2.counts, res.counts) and res2.skipped == 1


def test_abi_errors_launch_nothing(model):
    lib, h, st = _lib.load(), model._handle, _stream(torch.device(DEV))
    N, D, K = 8, 32, 3
    x, c = dev(unit_rows(N, D, 0)), dev(unit_rows(K, D, 1))
    labels = torch.full((N,), 77, dtype=torch.int32, device=DEV)
    best = torch.full((N,), 7.0, dtype=torch.float32, device=DEV)
    sums = ClusterSums(K, D, DEV)
    sums.buf.fill_(5)
    empty = torch.full((K,), 9, dtype=torch.uint8, device=DEV)
    idx = torch.full((1,), 99, dtype=torch.int64, device=DEV)
    nearest = torch.full((N,), 3.0, dtype=torch.float32, device=DEV)
    null = C_.c_void_p(0)
    cen_before = c.clone()

    def assign(x_=_ptr(x), n=N, d=D, c_=_ptr(c), k=K, l=_ptr(labels), counts=_ptr(sums.counts), changed=null, two=0):
        return lib.keep_cluster_assign(h, x_, n, d, c_, k, l, _ptr(best), null, null, _ptr(sums.skipped), changed, _ptr(sums.sums), counts,
                                       _ptr(sums.cos_sum), two, st)

    def update(s=_ptr(sums.sums), k=K, d=D, c_=_ptr(c)):
        return lib.keep_cluster_update(h, s, _ptr(sums.counts), k, d, c_, _ptr(empty), st)

    def seed(x_=_ptr(x), n=N, d=D, centre=_ptr(c), row=null, first=0, near=_ptr(nearest), out=_ptr(idx)):
        return lib.keep_cluster_seed_step(h, x_, n, d, centre, row, first, near, out, st)

    bad = [lambda: assign(x_=null), lambda: assign(c_=null), lambda: assign(k=65), lambda: assign(k=0), lambda: assign(d=24),
           lambda: assign(d=1040), lambda: assign(n=0), lambda: assign(n=(1 << 22) + 1), lambda: assign(counts=null),
           lambda: assign(changed=_ptr(sums.changed)), lambda: assign(two=2),
           lambda: update(s=null), lambda: update(c_=null), lambda: update(k=65), lambda: update(d=24),
           lambda: seed(x_=null), lambda: seed(out=null), lambda: seed(d=24), lambda: seed(n=0), lambda: seed(centre=null),
           lambda: seed(row=_ptr(idx)), lambda: seed(near=null), lambda: seed(first=2)]
    for i, call in enumerate(bad):
        assert call() == _lib.KEEP_EINVAL, f"bad call {i}"
        assert len(lib.keep_last_error(h)) > 10, f"bad call {i}"
    assert lib.keep_cluster_assign(None, _ptr(x), N, D, _ptr(c), K, _ptr(labels), null, null, null, null, null, null, null, null, 0, st) == _lib.KEEP_EINVAL
    torch.cuda.synchronize()
    assert (labels == 77).all() and (best == 7.0).all() and (sums.buf == 5).all() and (empty == 9).all() and int(idx) == 99
    assert (nearest == 3.0).all() and torch.equal(c, cen_before)
    # and the same arguments, sound, go through
    sums.zero_()
    assert assign() == _lib.KEEP_OK and update() == _lib.KEEP_OK and seed() == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert int(sums.counts.sum()) == N and (labels >= 0).all() and 0 <= int(idx) < N
