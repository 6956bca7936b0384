"""Feature PCA on the MI355X: keep_pca_moments / keep_pca_project / keep_class_render_rgb, KEEPModel.pca_moments /
pca_fit / pca_fit_batches / pca_transform / render_rgb_map and wsi.pca_map.

The yardsticks are the float64 restatements of keep_amd.pca, which tests/test_pca.py holds to scikit-learn.  Every bound is computed
from the exact float64 values of the operands the device read, never from the output under test (u = 2^-24):

* a Gram word: ``|dev 2^-32 - sum a_d a_e| <= sum over chunks [(rows_in_chunk + 1) u sum_i |a_id a_ie| + 2^-33]`` with ``a =
  float64(fp32(x - c))``: the worst case of a length-K fp32 sum of products in any order, plus the one rounding to fixed point;
* the fit: with B the matrix of those bounds, ``|lambda_dev - lambda_ref| <= ||B||_F / (n - 1)`` (Weyl) and ``sin angle(w_dev, w_ref) <=
  2 ||B||_F / ((n - 1) gap)`` (Davis-Kahan), the gap from the float64 spectrum.  The rounding of a itself (at most 2 u sum |a_d a_e| per
  word) and the 2^-31 of a sum word are not in B; they stay under 2 / (rows_in_chunk + 1) of it, inside the room between a worst-case
  chain bound and a real chain (a sequential fp32 emulation sits at 0.02-0.03 of B on these shapes);
* a score: ``|dev - (x - mean) . w| <= (D + 2) u (sum |x w| + |b|)``: D fma roundings, the bias's own rounding and its addition.
"""
import ctypes as C_
import functools

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel, _lib, pca, wsi
from keep_amd.classmap import ClassRaster
from keep_amd.cluster import skipped_numpy
from keep_amd.config import small_shape
from keep_amd.model import _ptr, _stream
from keep_amd.pca import FeaturePCA, PcaSums, fit_numpy, moments_numpy, render_rgb_numpy, synthetic_features
from keep_amd.region import TissueMask
from keep_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
CH = _lib.load().keep_pca_chunk()
SENTINEL = 0x0123456789ABCDE
NS = [1, 3, CH - 1, CH, CH + 1, 2 * CH + 37]
SHAPES = [(n, 48) for n in NS] + [(2 * CH + 37, d) for d in (16, 272)] + [(40, 1024)]


@pytest.fixture(scope="module")
def model():
    m = KEEPModel(precision="strict")
    m.load_state_dict(synth_state_dict(small_shape(2, 2), seed=5), strict=True)
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def feats(n, d, seed=1):
    x = synthetic_features(n, d, seed=seed)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def centre_of(d):
    """A fixed fp32 centre near the features' mean that is no row's own mean: a is never all zero, not even at N = 1."""
    c = feats(2 * CH + 37, d, seed=9).astype(np.float64).mean(axis=0).astype(np.float32)
    c.setflags(write=False)
    return c


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                         # a copy: the shared cases are read-only


def operands(x, c):
    """float64 of the fp32 operands the device forms: a = fp32(x - c), a skipped row zero."""
    a = x if c is None else (x - c[None, :]).astype(np.float32)
    return np.where(skipped_numpy(x)[:, None], 0.0, a.astype(np.float64))


def gram_reference(x, c, calls=None):
    """-> (sum a_d a_e, the bound of a device word) for the rows given to the device in ``calls`` = [(first, rows), ...] (default: one
    call); every call cuts its rows into chunks of CH from its own first row."""
    a = operands(x, c)
    d = x.shape[1]
    ref, bound = np.zeros((d, d)), np.zeros((d, d))
    for first, rows in (calls or [(0, x.shape[0])]):
        for r0 in range(first, first + rows, CH):
            blk = a[r0:min(r0 + CH, first + rows)]
            ref += blk.T @ blk
            bound += (blk.shape[0] + 1) * U * (np.abs(blk).T @ np.abs(blk)) + 2.0 ** -33
    return ref, bound


def written(d):
    """bool [D, D]: the 16 x 16 tiles with tile row <= tile column."""
    t = np.arange(d) // 16
    return t[:, None] <= t[None, :]


def moments(model, x, c=None, groups=0, into=None, sentinel=0):
    """One device call on the rows as they are -> the PcaSums (its gram pre-filled with ``sentinel`` when it is made here)."""
    sums = into
    if sums is None:
        sums = PcaSums(x.shape[1], c, DEV)
        if sentinel:
            sums.gram.fill_(sentinel)
    return model.pca_moments(dev(x), sums, normalize=False, groups=groups)


def words(sums):
    return sums.buf.cpu().numpy().copy()


# ------------------------------------------------------------------------------------------------ 1. moments against float64
@pytest.mark.parametrize("n,d", SHAPES, ids=lambda v: str(v))
def test_moments_against_float64(model, n, d):
    x, c = feats(n, d), centre_of(d)
    sums = moments(model, x, c, sentinel=SENTINEL)
    s, _, cnt, skp = moments_numpy(x, c, CH)
    assert torch.equal(sums.sum.cpu(), torch.from_numpy(s))
    assert int(sums.count) == cnt == n and int(sums.skipped) == skp == 0
    g = sums.gram.cpu().numpy()
    w = written(d)
    assert (g[~w] == SENTINEL).all()                                     # the words below are never touched
    ref, bound = gram_reference(x, c)
    err = np.abs((g - SENTINEL) / 2.0 ** 32 - ref)
    print(f"N={n} D={d}: largest error / bound = {(err[w] / bound[w]).max():.4f}")
    assert (err[w] <= bound[w]).all()
    for t in range(d // 16):                                             # diagonal tiles are written in full and symmetric bit for bit
        tile = g[16 * t:16 * t + 16, 16 * t:16 * t + 16]
        assert np.array_equal(tile, tile.T)
    full = sums.gram_full().cpu().numpy() - SENTINEL
    assert np.array_equal(full, full.T) and np.array_equal(full[w], (g - SENTINEL)[w])


# ------------------------------------------------------------------------------------------------ 2. invariance
@pytest.mark.parametrize("d", [48, 272])
def test_words_do_not_depend_on_the_launch_or_the_split(model, d):
    n = 2 * CH + 37
    x, c = feats(n, d), centre_of(d)
    whole = words(moments(model, x, c))
    assert np.array_equal(words(moments(model, x, c)), whole)            # two runs
    for groups in (1, 2, 4):
        assert np.array_equal(words(moments(model, x, c, groups=groups)), whole), groups
    for cuts in ([CH], [CH, 2 * CH]):
        parts = np.split(x, cuts)
        for order in (parts, parts[::-1]):
            sums = None
            for p in order:
                sums = moments(model, p, c, into=sums)
            assert np.array_equal(words(sums), whole), (cuts, order is parts)
    # a split that is no multiple of the chunk: sum and count are the same words, the Gram another sum of chunks within its own bound
    cut = CH + 7
    sums = moments(model, x[cut:], c, into=moments(model, x[:cut], c))
    assert torch.equal(sums.sum.cpu(), torch.from_numpy(whole[:d])) and int(sums.count) == n
    ref, bound = gram_reference(x, c, [(0, cut), (cut, n - cut)])
    w = written(d)
    assert (np.abs(sums.gram.cpu().numpy() / 2.0 ** 32 - ref)[w] <= bound[w]).all()


def test_fit_batches_equals_fit_on_the_whole(model):
    x = feats(3 * CH + 37, 48)
    parts = np.split(x, [CH, 3 * CH])
    calls = []

    def batches():
        calls.append(1)
        return iter([torch.from_numpy(np.array(p)) for p in parts])
    for two_pass in (True, False):
        calls.clear()
        a, b = model.pca_fit(dev(x), 3, two_pass=two_pass), model.pca_fit_batches(batches, 3, 48, two_pass=two_pass)
        assert len(calls) == (2 if two_pass else 1)
        assert np.array_equal(a.components, b.components) and np.array_equal(a.mean, b.mean)
        assert np.array_equal(a.explained_variance, b.explained_variance) and a.n_rows == b.n_rows == x.shape[0]
    with pytest.raises(ValueError, match="batch 0 holds 100 rows and is not the last"):
        model.pca_fit_batches(lambda: iter([torch.from_numpy(np.array(x[:100])), torch.from_numpy(np.array(x[100:200]))]), 3, 48)


# ------------------------------------------------------------------------------------------------ 3. skipped rows
def test_skipped_rows_are_zero_rows(model):
    n, d = 2 * CH + 37, 48
    c = centre_of(d)
    x = np.array(feats(n, d))
    rows = [0, CH - 1, CH, n - 1]
    for r, v in zip(rows, (np.nan, np.inf, 1.5, -np.inf)):
        x[r, (7 * r) % d] = v
    z = x.copy()
    z[rows] = c                                                          # a = 0 there
    dirty, clean = moments(model, x, c), moments(model, z, c)
    assert torch.equal(dirty.gram, clean.gram)
    z[rows] = 0.0
    assert torch.equal(dirty.sum, moments(model, z, None).sum)           # a zero row adds nothing to the sum
    assert int(dirty.count) == n - 4 and int(dirty.skipped) == 4 and int(clean.count) == n and int(clean.skipped) == 0
    s, g, cnt, skp = moments_numpy(x, c, CH)
    assert torch.equal(dirty.sum.cpu(), torch.from_numpy(s)) and (cnt, skp) == (n - 4, 4)
    bad = np.full((CH + 5, d), np.nan, np.float32)
    sums = moments(model, bad, c, into=moments(model, x, c))
    assert np.array_equal(words(sums)[:-1], words(dirty)[:-1]) and int(sums.skipped) == 4 + CH + 5      # all skipped: nothing is added


# ------------------------------------------------------------------------------------------------ 4. centre, 5. fit against float64
def test_null_centre_is_the_zero_centre(model):
    x = feats(CH + 1, 48)
    assert np.array_equal(words(moments(model, x, None)), words(moments(model, x, np.zeros(48, np.float32))))


def fit_bounds(x, fit):
    """||B||_F / (n - 1) for the device pass that made ``fit`` (its own centre)."""
    _, bound = gram_reference(x, fit.centre)
    return float(np.linalg.norm(bound)) / (fit.n_rows - 1)


@pytest.mark.parametrize("two_pass", [True, False], ids=["two_pass", "one_pass"])
@pytest.mark.parametrize("n,d", [(2 * CH + 37, 48), (2 * CH + 37, 272)], ids=lambda v: str(v))
def test_fit_against_float64(model, n, d, two_pass):
    x = feats(n, d)
    fit, ref = model.pca_fit(dev(x), 3, two_pass=two_pass, normalize=False), fit_numpy(x, 6)
    assert (fit.centre is not None) == two_pass and fit.n_rows == n and fit.skipped == 0
    eps = fit_bounds(x, fit)
    lam = ref.explained_variance
    print(f"N={n} D={d} two_pass={two_pass}: ||B||_F / (n - 1) = {eps:.3e}, eigenvalues {lam[:4]}, "
          f"error {np.abs(fit.explained_variance - lam[:3]).max():.3e}")
    assert np.abs(fit.explained_variance - lam[:3]).max() <= eps                       # Weyl
    assert abs(fit.total_variance - ref.total_variance) <= d * eps                     # the trace: D eigenvalues
    for j in range(3):
        gap = min(lam[j - 1] - lam[j] if j else np.inf, lam[j] - lam[j + 1])
        wd, wr = fit.components[j].astype(np.float64), ref.components[j].astype(np.float64)
        cos = float(wd @ wr) / (np.linalg.norm(wd) * np.linalg.norm(wr))
        assert cos > 0                                                                 # the signs agree
        # Davis-Kahan, plus the two fp32 roundings of the stored unit rows (each moves a unit row by at most sqrt(D) 2^-25)
        assert np.sqrt(max(0.0, 1 - cos * cos)) <= 2 * eps / gap + 2 * np.sqrt(d) * 2.0 ** -25
    assert 0 < fit.explained_variance_ratio.sum() <= 1
    assert np.abs(fit.mean.astype(np.float64) - x.astype(np.float64).mean(axis=0)).max() <= 2.0 ** -25 + 2.0 ** -31


def test_fit_needs_two_kept_rows(model):
    x = np.array(feats(3, 48))
    x[0, 0], x[2, 5] = np.nan, 2.0
    for two_pass in (True, False):
        with pytest.raises(ValueError, match="at least two kept rows, got 1"):
            model.pca_fit(dev(x), 1, two_pass=two_pass, normalize=False)


# ------------------------------------------------------------------------------------------------ 6. projection
@functools.lru_cache(maxsize=None)
def unit_rows(k, d):
    w = np.random.default_rng(17).standard_normal((k, d))
    return (w / np.linalg.norm(w, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("d", [48, 272])
@pytest.mark.parametrize("k", [1, 3, 17, 64])
def test_scores_are_cluster_assign_s_chain(model, k, d):
    x = np.array(feats(300, d))
    x[5, 3], x[299, 0] = np.nan, 1.5
    xd, w = dev(x), dev(unit_rows(k, d))
    out, kept = model._pca_project(xd, w, None, None)
    assert out.shape == (300, k) and kept.dtype == torch.bool
    for j in {0, k - 1}:
        best = model.cluster_assign(xd, w[j:j + 1].contiguous(), normalize=False)[1]
        assert torch.equal(out[:, j], best), j                           # bit for bit, the skipped rows' zeros included
    assert not kept[5] and not kept[299] and int(kept.sum()) == 298 and not out[5].any() and not out[299].any()
    for i in (0, 63, 64, 298):                                           # a row's scores depend on that row alone
        one, k1 = model._pca_project(xd[i:i + 1].contiguous(), w, None, None)
        assert torch.equal(one[0], out[i]) and bool(k1[0])


def test_transform_against_float64(model):
    n, d = 2 * CH + 37, 48
    x = np.array(feats(n, d))
    x[11, 2] = np.inf
    fit = model.pca_fit(dev(x), 3, normalize=False)
    scores, kept = model.pca_transform(fit, dev(x), normalize=False)
    ref, rkept = pca.project_numpy(fit, x)
    assert np.array_equal(kept.cpu().numpy(), rkept) and not scores[11].any()
    w, b = fit.components.astype(np.float64), fit.bias().astype(np.float64)
    x0 = np.where(rkept[:, None], x, 0).astype(np.float64)
    bound = (d + 2) * U * (np.abs(x0) @ np.abs(w).T + np.abs(b)[None, :])
    err = np.abs(scores.cpu().numpy().astype(np.float64) - ref)
    print(f"scores: largest error / bound = {(err[rkept] / bound[rkept]).max():.4f}")
    assert (err[rkept] <= bound[rkept]).all()
    assert torch.equal(model.pca_transform(fit, dev(x), k=2, normalize=False)[0], scores[:, :2].contiguous())
    # whitened: var(s_j) = w^T C w lies within eps + 2 sqrt(D) 2^-25 lambda (the stored row's rounding) of lambda_j, C the float64
    # covariance; the device scores differ from s by at most `bound`, which moves a standard deviation by at most the bound's root mean
    # square; the scale and the product round once each (4 u on a variance, 5 u taken)
    white = model.pca_transform(fit, dev(x), whiten=True, normalize=False)[0].cpu().numpy().astype(np.float64)[rkept]
    var = white.var(axis=0, ddof=1)
    eps = fit_bounds(x, fit)
    lam = fit.explained_variance
    eta = np.sqrt((bound[rkept] ** 2).sum(axis=0) / (rkept.sum() - 1))
    slack = eps + 2 * np.sqrt(d) * 2.0 ** -25 * lam
    lo = (np.sqrt(lam - slack) - eta) ** 2 / lam * (1 - 5 * U)
    hi = (np.sqrt(lam + slack) + eta) ** 2 / lam * (1 + 5 * U)
    print("whitened variances:", var, "bounds", lo, hi)
    assert (var >= lo).all() and (var <= hi).all()


# ------------------------------------------------------------------------------------------------ 7. display
def test_render_rgb_map_matches_the_restatement(model):
    g = np.random.default_rng(30)
    C, h, w = 5, 40, 56
    cnt = g.integers(0, 4, (h, w))
    S = g.integers(0, 65536, (C, h, w)) * cnt[None]
    S[0, 0, :8], S[1, 0, :8] = 0, 65535 * cnt[0, :8]                     # both ends of the range
    acc = (cnt[None].astype(np.int64) << 40) | S.astype(np.int64)
    raster = ClassRaster(torch.from_numpy(acc).to(DEV), 16, 224, model=model)
    mask = g.random((h, w)) < 0.8
    tissue = TissueMask(mask, 16)
    base = torch.from_numpy(g.integers(0, 256, (h, w * 4 + 3), dtype=np.uint8)).to(DEV)
    rgba = base.as_strided((h, w, 4), (w * 4 + 3, 4, 1))                 # RGBA, an odd row stride
    for alpha in (0.0, 0.6, 1.0):
        for planes, th, ti in (((0, 1, 2), rgba, tissue), ((4, 2, 0), None, None), ((3, 3, 1), rgba[..., :3].contiguous(), None)):
            got = model.render_rgb_map(raster, th, planes, alpha, ti, background=(250, 240, 230))
            want = render_rgb_numpy(acc, None if th is None else th.cpu().numpy(), planes, alpha, None if ti is None else mask, (250, 240, 230))
            assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), (alpha, planes)
    with pytest.raises(ValueError, match="three plane indices in 0..4"):
        model.render_rgb_map(raster, planes=(0, 1, 5))


def test_pca_map_of_two_planted_groups(model):
    g = np.random.default_rng(31)
    d, gy, gx = 48, 5, 6
    q, _ = np.linalg.qr(g.standard_normal((d, 3)))
    group = (np.arange(gy * gx) % gx) >= gx // 2                         # the right half of the grid
    x = q[:, 0][None, :] + np.where(group, 0.6, -0.6)[:, None] * q[:, 1][None, :] + 0.05 * g.standard_normal((gy * gx, d))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    x[7, 0] = np.nan                                                     # a skipped tile
    coords = np.stack([(np.arange(gy * gx) % gx) * 256, (np.arange(gy * gx) // gx) * 256], axis=1).astype(np.int64)
    shape = (gy * 16, gx * 16)
    raster, fit = wsi.pca_map(dev(x), coords, 3, 16, shape, model=model)
    assert isinstance(fit, FeaturePCA) and fit.skipped == 1 and fit.n_rows == gy * gx - 1 and raster.n_classes == 3
    acc = raster.acc.cpu().numpy()
    cnt = acc[0] >> 40
    ty, tx = 7 // gx, 7 % gx
    assert (cnt[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] == 0).all() and int((cnt == 0).sum()) == 256   # the skipped tile alone
    red = model.render_rgb_map(raster, alpha=1.0)[..., 0].cpu().numpy().astype(np.int64)
    on = cnt > 0
    left, right = np.zeros(shape, bool), np.zeros(shape, bool)
    left[:, :gx // 2 * 16], right[:, gx // 2 * 16:] = True, True
    a, b = red[left & on], red[right & on]
    assert a.max() < b.min() or b.max() < a.min()                        # the two groups differ in channel 0
    again, same_fit = wsi.pca_map(dev(x), coords, fit, 16, shape, model=model)
    assert same_fit is fit and torch.equal(again.acc, raster.acc)
    lin, _ = wsi.pca_map(dev(x), coords, fit, 16, shape, scale=((-1, -1, -1), (1, 1, 1)), model=model)
    assert torch.equal(lin.acc >> 40, raster.acc >> 40)
    with pytest.raises(ValueError, match="three component indices in 0..2"):
        wsi.pca_map(dev(x), coords, fit, 16, shape, components=(0, 1, 3), model=model)


# ------------------------------------------------------------------------------------------------ 8. arguments
def test_every_einval_leaves_the_outputs_untouched(model):
    lib, h, s = _lib.load(), model._handle, _stream(model._device)
    n, d, k = 40, 48, 3
    x, w = dev(feats(n, d)), dev(unit_rows(k, d))
    c = dev(centre_of(d))
    acc = torch.full((d + d * d + 2,), 77, dtype=torch.int64, device=DEV)
    sm, gr, cn, sk = acc[:d], acc[d:d + d * d], acc[d + d * d:d + d * d + 1], acc[d + d * d + 1:]
    p = lambda t, off=0: C_.c_void_p(0 if t is None else t.data_ptr() + off)

    def mom(x_=x, n_=n, d_=d, c_=c, sm_=sm, cn_=cn, gr_=gr, sk_=sk, groups=0, off=0):
        return lib.keep_pca_moments(h, p(x_, off), n_, d_, p(c_), p(sm_), p(cn_), p(gr_), p(sk_), groups, s)
    bad = [mom(n_=0), mom(n_=(1 << 22) + 1), mom(d_=24), mom(d_=1040), mom(d_=0), mom(x_=None), mom(off=4), mom(sm_=None), mom(cn_=None),
           mom(groups=-1), mom(groups=65),
           lib.keep_pca_moments(h, p(x), n, d, p(c, 4), p(sm), p(cn), p(gr), p(sk), 0, s),
           lib.keep_pca_moments(h, p(x), n, d, p(c), p(sm, 4), p(cn), p(gr), p(sk), 0, s),
           lib.keep_pca_moments(h, p(x), n, d, p(c), p(sm), p(cn), p(gr, 4), p(sk), 0, s)]
    assert all(rc == _lib.KEEP_EINVAL for rc in bad), bad
    torch.cuda.synchronize()
    assert bool((acc == 77).all())
    out = torch.full((n, k), 7.0, dtype=torch.float32, device=DEV)
    kept = torch.full((n,), 9, dtype=torch.uint8, device=DEV)

    def proj(x_=x, n_=n, d_=d, w_=w, k_=k, out_=out, off=0, woff=0):
        return lib.keep_pca_project(h, p(x_, off), n_, d_, p(w_, woff), k_, p(None), p(None), p(out_), p(kept), p(sk), s)
    bad = [proj(n_=0), proj(d_=24), proj(k_=0), proj(k_=65), proj(x_=None), proj(w_=None), proj(out_=None), proj(off=4), proj(woff=8)]
    assert all(rc == _lib.KEEP_EINVAL for rc in bad), bad
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((kept == 9).all()) and bool((acc == 77).all())
    ras = torch.zeros((3, 4, 5), dtype=torch.int64, device=DEV)
    img = torch.full((4, 5, 3), 3, dtype=torch.uint8, device=DEV)
    planes = lambda *v: (C_.c_int * 3)(*v)

    def ren(acc_=ras, C=3, H=4, W=5, pl=planes(0, 1, 2), thumb=None, row=0, ps=3, bg=0xFFFFFF, alpha=128, out_=img, off=0):
        return lib.keep_class_render_rgb(h, p(acc_, off), C, H, W, pl, p(thumb), row, ps, bg, p(None), alpha, p(out_), s)
    bad = [ren(acc_=None), ren(off=4), ren(C=0), ren(C=65), ren(H=0), ren(pl=planes(0, 1, 3)), ren(pl=planes(-1, 1, 2)), ren(pl=None),
           ren(out_=None), ren(alpha=257), ren(alpha=-1), ren(bg=0x1000000), ren(thumb=img, row=15, ps=2), ren(thumb=img, row=14, ps=3)]
    assert all(rc == _lib.KEEP_EINVAL for rc in bad), bad
    torch.cuda.synchronize()
    assert bool((img == 3).all())
    assert mom() == _lib.KEEP_OK and proj() == _lib.KEEP_OK and ren() == _lib.KEEP_OK      # the valid forms of the same calls
    torch.cuda.synchronize()
    assert int(cn) == 77 + n and bool((kept == 1).all()) and bool((img == 255).all())       # no tile covers a pixel: the background


def test_python_argument_checks(model):
    x = dev(feats(40, 48))
    with pytest.raises(ValueError, match="sums must be a PcaSums"):
        model.pca_moments(x, None)
    with pytest.raises(ValueError, match="accumulators are for D = 16"):
        model.pca_moments(x, PcaSums(16, None, DEV))
    with pytest.raises(ValueError, match="components must be in 1..64, got 65"):
        model.pca_fit(x, 65)
    with pytest.raises(ValueError, match="multiple of 16 in 16..1024, got 24"):
        model.pca_fit(torch.zeros((4, 24), device=DEV), 2)
    with pytest.raises(ValueError, match="pca must be a FeaturePCA"):
        model.pca_transform(None, x)
    with pytest.raises(ValueError, match="groups must be 0"):
        model.pca_moments(x, PcaSums(48, None, DEV), groups=65)
