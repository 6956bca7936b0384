"""The float64 restatements of keep_amd.tsne against scikit-learn, and the argument checks.  No GPU.

Tolerances:

* ``conditional_numpy`` against ``sklearn.manifold._utils._binary_search_perplexity`` on the same squared distances: 5e-5 of the row's
  largest probability.  scikit-learn stops its search once the entropy is within 1e-5 of ``log(perplexity)``, the restatement runs to
  the float64 root, so the two differ by what 1e-5 of entropy moves a probability: ``dp / p = -(d - <d>) dbeta`` with ``dbeta = dH / (beta
  var d)``, a few 1e-6 to 1e-5 of the largest probability on these rows (7.5e-6 at N = 300, k = 60, perplexity 20); 5e-5 leaves room
  for a row whose search ends at the edge of scikit-learn's tolerance and is still 200 times under a wrong beta's effect.
* ``gradient_numpy`` against ``sklearn.manifold._t_sne._kl_divergence``: the same float64 formulas summed in another order, 1e-12
  relative (1.4e-15 measured).
"""
import numpy as np
import pytest
from scipy.spatial.distance import squareform

from keep_amd import tsne
from keep_amd.tsne import (conditional_numpy, distances_numpy, fit_numpy, gradient_numpy, joint_numpy, knn_purity, perplexity_numpy, step_numpy,
                           synthetic_blobs)


def neighbour_lists(x, k):
    """The k nearest rows of every row by cosine, the row itself left out -> (index int64 [N, k], score fp32 [N, k]), best first."""
    s = (x.astype(np.float64) @ x.astype(np.float64).T).astype(np.float32)
    np.fill_diagonal(s, -np.inf)
    index = np.argsort(-s, axis=1, kind="stable")[:, :k]
    return index.astype(np.int64), np.take_along_axis(s, index, axis=1)


@pytest.fixture(scope="module")
def blobs():
    x, labels = synthetic_blobs(300, 48, 4, 0.7, 0)
    index, score = neighbour_lists(x, 60)
    p = conditional_numpy(score, np.full(300, 60), 20.0, index)
    return x, labels, index, score, p, joint_numpy(index, p)


# ------------------------------------------------------------------------------------------------ 1. affinities
@pytest.mark.parametrize("perplexity,k", [(20.0, 60), (5.0, 15), (2.0, 6), (21.0, 64)])
def test_conditional_against_sklearn(blobs, perplexity, k):
    from sklearn.manifold._utils import _binary_search_perplexity
    index, score = neighbour_lists(blobs[0], k)
    d, _ = distances_numpy(score, np.full(300, k))
    ref = _binary_search_perplexity(d.astype(np.float32), perplexity, 0)
    p = conditional_numpy(score, np.full(300, k), perplexity, index)
    err = np.abs(p - ref).max(axis=1) / ref.max(axis=1)
    print(f"perplexity {perplexity}, k {k}: largest |p - sklearn| / max p = {err.max():.2e}")
    assert err.max() <= 5e-5
    assert np.abs(p.sum(axis=1) - 1).max() <= 1e-12
    assert np.abs(perplexity_numpy(p) / perplexity - 1).max() <= 1e-9


def test_conditional_edge_rows():
    score = np.zeros((4, 8), np.float32)
    score[0] = 0.5                                                       # equidistant: uniform
    score[1] = np.linspace(0.9, 0.1, 8)
    score[2] = [0.99] + [0.1] * 7                                        # one neighbour far closer than the rest
    score[3] = np.linspace(0.9, 0.1, 8)
    count = np.array([8, 5, 8, 1])
    index = np.tile(np.arange(8), (4, 1))
    p = conditional_numpy(score, count, 3.0, index)
    assert np.allclose(p[0], 1 / 8, rtol=0, atol=1e-15)
    assert (p[1, 5:] == 0).all() and abs(p[1].sum() - 1) < 1e-12 and abs(perplexity_numpy(p[1:2])[0] - 3) < 1e-9
    assert p[2, 0] > 0.3 and abs(perplexity_numpy(p[2:3])[0] - 3) < 1e-9
    assert (p[3] == 0).all()                                             # fewer than two neighbours: a zero row
    index[1, 2] = -1                                                     # an empty slot inside the count is no neighbour
    assert conditional_numpy(score, count, 3.0, index)[1, 2] == 0


# ------------------------------------------------------------------------------------------------ 2. the joint graph
def test_joint_graph(blobs):
    _, _, index, _, p, g = blobs
    keys = g.keys()
    assert (np.diff(keys) > 0).all()                                     # strictly ascending: sorted, and equal keys merged
    assert abs(g.val.sum() - 1) <= 1e-12
    P = g.dense()
    assert np.array_equal(P, P.T) and (np.diag(P) == 0).all()
    directed = np.zeros((300, 300))
    directed[np.arange(300)[:, None], index] = p
    assert np.abs(P - (directed + directed.T) / 600).max() <= 1e-18
    mutual = (directed > 0) & (directed.T > 0)
    assert mutual.any() and (~mutual & (directed > 0)).any()             # both kinds of edge are there
    assert g.nnz == int(((directed + directed.T) > 0).sum())             # a mutual pair is one entry per direction, not two
    assert g.row_ptr[0] == 0 and g.row_ptr[-1] == g.nnz and g.row_ptr.dtype == np.int32 and g.col.dtype == np.int32


def test_joint_graph_compacts_dropped_rows():
    index = np.array([[1, 2], [0, 2], [-1, -1], [0, 1]], np.int64)       # row 2 is skipped; nobody may name it
    index[0, 1] = 3
    index[1, 1] = 3
    p = np.array([[0.5, 0.5], [0.25, 0.75], [0, 0], [0.5, 0.5]])
    g = joint_numpy(index, p)
    assert g.n == 3 and abs(g.val.sum() - 1) < 1e-15
    P = g.dense()
    assert P[0, 1] == 0.5 / 6 + 0.25 / 6 and P[0, 2] == 0.5 / 6 + 0.5 / 6 and P[1, 2] == 0.75 / 6 + 0.5 / 6    # each edge weighted, then merged


# ------------------------------------------------------------------------------------------------ 3. the gradient
@pytest.mark.parametrize("scale", [1e-4, 1.0, 30.0])
def test_gradient_against_sklearn(blobs, scale):
    from sklearn.manifold._t_sne import _kl_divergence
    g = blobs[5]
    P = g.dense()
    y = np.random.default_rng(3).standard_normal((300, 2)) * scale
    kl_ref, grad_ref = _kl_divergence(y.ravel(), squareform(P), 1.0, 300, 2)
    for given in (g, P):                                                 # a CSR or a dense P
        kl, grad, Z = gradient_numpy(y, given)
        assert abs(kl - kl_ref) <= 1e-12 * abs(kl_ref)
        assert np.abs(grad.ravel() - grad_ref).max() <= 1e-12 * np.abs(grad_ref).max()
    d2 = ((y[:, None] - y[None]) ** 2).sum(axis=2)
    assert abs(Z - ((1 / (1 + d2)).sum() - 300)) <= 1e-12 * Z


def test_gradient_is_the_derivative_of_the_divergence(blobs):
    g = blobs[5]
    P = g.dense()
    y = np.random.default_rng(4).standard_normal((300, 2))
    _, grad, _ = gradient_numpy(y, P)
    h = 1e-5
    for i, c in ((0, 0), (17, 1), (299, 0)):
        e = np.zeros_like(y)
        e[i, c] = h
        fd = (gradient_numpy(y + e, P)[0] - gradient_numpy(y - e, P)[0]) / (2 * h)
        assert abs(fd - grad[i, c]) <= 1e-6 * max(abs(grad[i, c]), np.abs(grad).max() * 1e-2), (i, c, fd, grad[i, c])
    kl, grad12, _ = gradient_numpy(y, P, 12.0)                           # exaggeration scales the attraction alone; KL stays that of P
    assert kl == gradient_numpy(y, P)[0]
    _, grad0, _ = gradient_numpy(y, np.zeros_like(P))                    # the repulsion alone
    assert np.abs((grad12 - grad0) - 12 * (grad - grad0)).max() <= 1e-12 * np.abs(grad12).max()


# ------------------------------------------------------------------------------------------------ 4. the update and the fit
def test_step_rule():
    y = np.zeros((4, 2))
    update = np.array([[1.0, -1.0], [1.0, 0.0], [-1.0, 1.0], [1.0, 1.0]])
    grad = np.array([[-1.0, 1.0], [1.0, 1.0], [-1.0, 0.0], [1.0, 1.0]])
    gains = np.array([[1.0, 1.0], [1.0, 1.0], [1.0, 1.0], [0.0110, 0.0126]])
    y2, u2, g2 = step_numpy(y, update, gains, grad, 0.5, 10.0)
    assert np.array_equal(g2[:3], [[1.2, 1.2], [0.8, 0.8], [0.8, 0.8]])  # opposite signs: + 0.2; the same sign or a zero: x 0.8
    assert g2[3, 0] == 0.01 and g2[3, 1] == 0.0126 * 0.8                 # the floor
    assert np.array_equal(u2, 0.5 * update - 10.0 * (g2 * grad)) and np.array_equal(y2, u2)


def test_fit_separates_blobs(blobs):
    from sklearn.manifold import trustworthiness
    x, labels, _, _, _, g = blobs
    y0 = tsne.random_init(300, 0)
    assert np.array_equal(y0, tsne.random_init(300, 0)) and not np.array_equal(y0, tsne.random_init(300, 1))
    assert 0.8e-4 < y0.std() < 1.2e-4
    y, iters, kls, kl, n_iter, reason = fit_numpy(g, y0, n_iter=500, check_every=50)
    assert (n_iter, reason) == (500, "n_iter") and list(iters) == list(range(49, 500, 50))
    assert knn_purity(y, labels, 10) >= 0.98
    assert trustworthiness(x, y, n_neighbors=10) >= 0.92
    after = kls[iters >= 250]
    assert (np.diff(after) <= 0.03 * after[:-1]).all() and kl <= after[-1] * 1.03
    assert 0.7 < kl < 0.9                                                # 0.776 .. 0.789 over seeds 0 .. 2 at perplexity 20


def test_fit_stops_on_a_small_gradient(blobs):
    g = blobs[5]
    out = fit_numpy(g, tsne.random_init(300, 0), n_iter=400, exaggeration_iter=100, check_every=50, min_grad_norm=1e3)
    assert out[4] == 150 and out[5] == "min_grad_norm"                   # the first check after the exaggeration


# ------------------------------------------------------------------------------------------------ 5. argument checks
def test_argument_checks():
    assert tsne.check_perplexity(20) == (20.0, 60) and tsne.check_perplexity(21) == (21.0, 63)
    assert tsne.check_perplexity(30, 64) == (30.0, 64) and tsne.check_perplexity(2.5) == (2.5, 8)
    for bad in (1.9, 0, -3, float("nan"), float("inf"), "many", True):
        with pytest.raises(ValueError):
            tsne.check_perplexity(bad)
    with pytest.raises(ValueError, match="64"):
        tsne.check_perplexity(22)                                        # 3 x 22 > 64
    for perp, k in ((20, 39), (5, 65), (5, 1), (5, 2.5)):
        with pytest.raises(ValueError):
            tsne.check_perplexity(perp, k)
    for n in (0, 1, 2, (1 << 20) + 1):
        with pytest.raises(ValueError):
            tsne.check_rows(n)
    assert tsne.check_rows(3) == 3
    for init in (np.zeros((299, 2), np.float32), np.zeros((300, 3), np.float32), np.zeros((300, 2), np.float64), "spectral"):
        with pytest.raises(ValueError):
            tsne.check_init(init, 300)
    assert tsne.check_init("pca", 300) == "pca" and tsne.check_init(np.ones((300, 2), np.float32), 300).shape == (300, 2)
    for bad in ((0, 0, 50, 300), (100, 101, 50, 300), (100, 50, 0, 300), (100, 50, 50, 0), (100.0, 50, 50, 300)):
        with pytest.raises(ValueError):
            tsne.check_iterations(*bad)
    assert tsne.check_iterations(1000, 250, 50, 300) == (1000, 250, 50, 300)
    for bad in (0.5, 33.0, float("nan")):
        with pytest.raises(ValueError):
            tsne.check_exaggeration(bad)
    assert tsne.check_learning_rate("auto", 300, 12.0) == 50.0 and tsne.check_learning_rate("auto", 48000, 12.0) == 1000.0
    for bad in ("fast", 0, -1.0, float("inf")):
        with pytest.raises(ValueError):
            tsne.check_learning_rate(bad, 300, 12.0)


def test_scatter_coords():
    y = np.array([[0.0, 10.0], [1.0, 20.0], [np.nan, 0.0], [0.5, 15.0]], np.float32)
    coords, shown = tsne.scatter_coords_numpy(y, (101, 201), 1)
    assert list(shown) == [True, True, False, True]
    assert coords[shown].tolist() == [[0, 0], [200, 100], [100, 50]]
