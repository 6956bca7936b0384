"""Feature PCA on the host: the float64 restatements of keep_amd.pca against independent yardsticks
(scikit-learn's full-SVD PCA, a per-pixel Python loop), the integer moments' invariances, the skip rule and the argument checks.
No GPU; tests/test_pca_gpu.py holds the device to these restatements."""
import numpy as np
import pytest

from keep_amd import pca
from keep_amd.heatmap import Q_ONE
from keep_amd.pca import (CHUNK, PcaSums, check_batch_rows, components_from_covariance, covariance_from_sums, fit_numpy, moments_numpy,
                          project_numpy, render_rgb_numpy, synthetic_features)

SHAPES = [(1061, 48), (700, 16)]


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def case(request):
    n, d = request.param
    x = synthetic_features(n, d, seed=1)
    x.setflags(write=False)
    return x


def test_synthetic_features_are_unit_rows_with_the_planted_spectrum():
    x = synthetic_features(1061, 48, seed=1)
    assert x.dtype == np.float32 and x.shape == (1061, 48)
    assert np.abs(np.linalg.norm(x.astype(np.float64), axis=1) - 1).max() < 1e-6
    lam = fit_numpy(x, 6).explained_variance
    assert (np.diff(lam[:4]) < -0.014).all()                             # the first four are well apart: their vectors are comparable


def test_fit_numpy_matches_scikit_learn(case):
    sk = pytest.importorskip("sklearn.decomposition")
    ref = sk.PCA(n_components=3, svd_solver="full").fit(case.astype(np.float64))
    fit = fit_numpy(case, 3)
    for mine, theirs in ((fit.explained_variance, ref.explained_variance_), (fit.explained_variance_ratio, ref.explained_variance_ratio_)):
        rel = np.abs(mine - theirs) / np.abs(theirs)
        print("relative difference to scikit-learn:", rel)
        assert rel.max() <= 1e-12
    assert np.abs(fit.components.astype(np.float64) - ref.components_).max() <= 1e-7   # fp32 storage of unit rows: 2^-24
    x64 = case.astype(np.float64)                                        # fit_numpy's own path, before its fp32 storage
    a = x64 - fit.centre.astype(np.float64)
    _, cov = covariance_from_sums(x64.sum(axis=0) * pca.SUM_ONE, (a.T @ a) * pca.GRAM_ONE, case.shape[0], fit.centre)
    _, w = components_from_covariance(cov, 3)
    print("component difference, sign included:", np.abs(w - ref.components_).max())
    assert np.abs(w - ref.components_).max() <= 1e-9
    assert np.abs(fit.mean.astype(np.float64) - ref.mean_).max() <= 2.0 ** -24
    assert fit.n_rows == case.shape[0] and fit.skipped == 0
    assert abs(np.linalg.norm(fit.components.astype(np.float64), axis=1) - 1).max() < 1e-6
    big = np.abs(fit.components).argmax(axis=1)
    assert (fit.components[np.arange(3), big] > 0).all()


def test_one_pass_fit_agrees_in_float64(case):
    two, one = fit_numpy(case, 3, two_pass=True), fit_numpy(case, 3, two_pass=False)
    assert one.centre is None and two.centre is not None
    assert np.abs(one.explained_variance - two.explained_variance).max() <= 1e-12
    assert 0 < two.explained_variance_ratio.sum() <= 1


def test_shifted_data_formula_for_any_centre(case):
    x = case.astype(np.float64)
    n, d = x.shape
    rng = np.random.default_rng(3)
    s = x.sum(axis=0) * pca.SUM_ONE
    _, cov0 = covariance_from_sums(s, (x.T @ x) * pca.GRAM_ONE, n, None)
    for c in (rng.uniform(-1, 1, d).astype(np.float32), (x.mean(axis=0)).astype(np.float32)):
        a = x - c.astype(np.float64)
        mu, cov = covariance_from_sums(s, (a.T @ a) * pca.GRAM_ONE, n, c)
        # float64 rounding of sums of n products of magnitude <= 4, divided by n - 1: n 4 2^-53 n / (n - 1) per word with room
        assert np.abs(cov - cov0).max() <= 8 * n * 2.0 ** -53
        assert np.abs(mu - x.mean(axis=0)).max() <= 1e-15
    assert np.abs(cov0 - np.cov(x, rowvar=False)).max() <= 8 * n * 2.0 ** -53


def test_moment_words_do_not_depend_on_the_split_at_chunk_multiples(case):
    c = fit_numpy(case, 1).centre
    for chunk in (CHUNK, 64):
        whole = moments_numpy(case, c, chunk)
        for cuts in ((chunk,), (2 * chunk,), (chunk, 3 * chunk)):
            cuts = [k for k in cuts if k < case.shape[0]]
            parts, acc = np.split(case, cuts), None
            for part in parts[::-1]:                                     # the order of the calls plays no part either
                acc = moments_numpy(part, c, chunk, into=acc)
            assert all(np.array_equal(a, b) for a, b in zip(acc, whole))
    g = moments_numpy(case, c, CHUNK)[1]
    assert np.array_equal(g, g.T)


def test_sum_words_do_not_depend_on_the_order_of_the_rows(case):
    perm = np.random.default_rng(5).permutation(case.shape[0])
    a, b = moments_numpy(case, None), moments_numpy(case[perm], None)
    assert np.array_equal(a[0], b[0]) and a[2] == b[2] and a[3] == b[3]
    odd = moments_numpy(case[:CHUNK + 7], None, into=moments_numpy(case[CHUNK + 7:], None))      # any split: sum and count
    assert np.array_equal(a[0], odd[0]) and a[2] == odd[2]


def test_moments_against_float64(case):
    c = fit_numpy(case, 1).centre
    s, g, n, skipped = moments_numpy(case, c)
    a = (case - c).astype(np.float32).astype(np.float64)
    chunks = -(-case.shape[0] // CHUNK)
    assert np.abs(g / pca.GRAM_ONE - a.T @ a).max() <= chunks * 2.0 ** -33 + 1e-12
    assert np.abs(s / pca.SUM_ONE - case.astype(np.float64).sum(axis=0)).max() <= case.shape[0] * 2.0 ** -31
    assert (n, skipped) == (case.shape[0], 0)


def test_skipped_rows_change_nothing_but_skipped(case):
    bad = np.array(case[:3])
    bad[0, 1], bad[1, 2], bad[2, 0] = np.nan, np.inf, 1.5
    x = np.concatenate([case[:100], bad[:1], case[100:600], bad[1:], case[600:]])
    c = fit_numpy(case, 1).centre
    # the chunks of x hold other rows than those of `case`: compare against `case` with zero rows where the bad ones are
    z = x.copy()
    z[[100, 601, 602]] = c
    clean, dirty = moments_numpy(z, c), moments_numpy(x, c)
    assert np.array_equal(clean[1], dirty[1])
    assert np.array_equal(moments_numpy(case, c)[0], dirty[0])
    assert dirty[2] == case.shape[0] and dirty[3] == 3 and clean[3] == 0
    a, b = fit_numpy(case, 3), fit_numpy(x, 3)
    assert b.skipped == 3 and b.n_rows == a.n_rows
    assert np.abs(a.explained_variance - b.explained_variance).max() <= 1e-15 and np.array_equal(a.mean, b.mean)
    scores, kept = project_numpy(a, x)
    assert not kept[[100, 601, 602]].any() and kept.sum() == case.shape[0] and not scores[~kept].any()


def test_project_numpy_and_whitening(case):
    fit = fit_numpy(case, 3)
    scores, kept = project_numpy(fit, case)
    assert kept.all()
    assert np.abs(scores.var(axis=0, ddof=1) - fit.explained_variance).max() <= 1e-7       # fp32 storage of mean and components
    white, _ = project_numpy(fit, case, whiten=True)
    assert np.abs(white.var(axis=0, ddof=1) - 1).max() <= 1e-5
    assert np.array_equal(project_numpy(fit, case, k=2)[0], scores[:, :2])
    assert np.allclose(fit.bias(), -(fit.components.astype(np.float64) @ fit.mean.astype(np.float64)), rtol=0, atol=1e-7)


def test_render_rgb_numpy_against_a_pixel_loop():
    rng = np.random.default_rng(11)
    C, h, w = 4, 9, 7
    cnt = rng.integers(1, 5, (h, w))
    cnt[2, 3] = 0                                                        # a pixel no tile covers
    S = rng.integers(0, Q_ONE + 1, (C, h, w)) * cnt[None]                 # every tile adds at most 65535
    S[:, cnt == 0] = 0
    S[1, 0, 0], S[2, 0, 1] = 0, Q_ONE * cnt[0, 1]                        # the ends of the range
    acc = (cnt[None].astype(np.int64) << 40) | S.astype(np.int64)
    mask = np.ones((h, w), np.uint8)
    mask[5, 5] = 0                                                       # a masked pixel
    thumb = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    for planes, alpha, th in (((0, 1, 2), 0.6, thumb), ((3, 1, 0), 1.0, None), ((2, 2, 2), 0.0, thumb[..., :3])):
        got = render_rgb_numpy(acc, th, planes, alpha, mask, background=(250, 240, 230))
        a = int(round(256 * alpha))
        for y in range(h):
            for x in range(w):
                for ch in range(3):
                    under = (250, 240, 230)[ch] if th is None else int(th[y, x, ch])
                    want = under
                    c = int(cnt[y, x])
                    if c > 0 and mask[y, x]:
                        v = min(255, (2 * 255 * int(S[planes[ch], y, x]) + 65535 * c) // (2 * 65535 * c))
                        want = (a * v + (256 - a) * under + 128) >> 8
                    assert got[y, x, ch] == want, (planes, alpha, y, x, ch)
    full = render_rgb_numpy(acc, None, (2, 2, 2), 1.0)
    assert full[0, 1].tolist() == [255, 255, 255] and render_rgb_numpy(acc, None, (1, 1, 1), 1.0)[0, 0].tolist() == [0, 0, 0]


def test_pca_sums_views_share_one_buffer():
    s = PcaSums(32)
    assert s.sum.shape == (32,) and s.gram.shape == (32, 32) and s.count.shape == (1,) and s.skipped.shape == (1,)
    s.gram[0, 17], s.gram[17, 0], s.gram[3, 2], s.gram[2, 3] = 5, 99, 7, 8           # (17, 0) lies below the written triangle
    full = s.gram_full()
    assert full[0, 17] == 5 and full[17, 0] == 5 and full[3, 2] == 8 and full[2, 3] == 8
    s.claim(1 << 24)
    with pytest.raises(ValueError, match="at most 2\\^24"):
        s.claim(1)
    s.zero_()
    assert s.rows == 0 and not s.buf.any()


def test_argument_checks():
    x = synthetic_features(40, 16, seed=2)
    with pytest.raises(ValueError, match="multiple of 16 in 16..1024, got 24"):
        moments_numpy(np.zeros((4, 24), np.float32))
    with pytest.raises(ValueError, match="multiple of 16 in 16..1024, got 24"):
        PcaSums(24)
    with pytest.raises(ValueError, match="components must be in 1..64, got 65"):
        fit_numpy(synthetic_features(80, 80, seed=2), 65)
    with pytest.raises(ValueError, match="must not exceed the feature width 16, got 17"):
        fit_numpy(x, 17)
    c = np.zeros(16, np.float32)
    c[3] = 1.5
    with pytest.raises(ValueError, match="every element within 1 in magnitude"):
        PcaSums(16, c)
    with pytest.raises(ValueError, match="every element within 1 in magnitude"):
        moments_numpy(x, c)
    with pytest.raises(ValueError, match="centre must be \\[16\\]"):
        PcaSums(16, np.zeros(8, np.float32))
    with pytest.raises(ValueError, match="batch 0 holds 100 rows and is not the last"):
        check_batch_rows(100, 0, CHUNK)
    check_batch_rows(2 * CHUNK, 0, CHUNK)
    one = np.array(x[:3])
    one[0, 0], one[2, 5] = np.nan, 2.0
    for two_pass in (True, False):
        with pytest.raises(ValueError, match="at least two kept rows, got 1"):
            fit_numpy(one, 1, two_pass=two_pass)
    with pytest.raises(ValueError, match="groups must be 0"):
        pca.check_groups(65)
    with pytest.raises(ValueError, match="three plane indices in 0..3"):
        render_rgb_numpy(np.zeros((4, 2, 2), np.int64), planes=(0, 1, 4))
    with pytest.raises(ValueError, match="features must be float32"):
        moments_numpy(x.astype(np.float64))
