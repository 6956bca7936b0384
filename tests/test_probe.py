"""The host side of the linear probe: the numpy restatements of keep_amd.probe held to per-row Python loops and
central differences, the L-BFGS held to scipy's optimum and sklearn's objective, the rounding of the integer sums, and every argument
check.  No GPU: the device kernel is held to these restatements in test_probe_gpu.py."""
import math

import numpy as np
import pytest
import torch
from scipy.optimize import minimize

from keep_amd import KEEPModel, probe, wsi
from keep_amd.probe import (GRAD_ONE, LOSS_ONE, LinearProbe, ProbeSums, check_class_weight, check_fit, check_init, check_n_classes,
                            check_weights, forward_numpy, kept_numpy, lbfgs, loss_grad_numpy, loss_noise, objective_from_words,
                            objective_numpy)
from test_cluster import row_skipped, unit_rows


def fit_problem(n, d, c, sep, seed):
    """Class means N(0,1)^d times sep plus N(0,1) noise, rows normalised -> (x fp32 [n,d], y int32 [n]); every class occurs."""
    g = np.random.default_rng(seed)
    means = g.standard_normal((c, d)) * sep
    y = g.permutation(np.arange(n) % c).astype(np.int32)
    x = means[y] + g.standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32), y


def params(c, d, seed, scale=2.0):
    g = np.random.default_rng(seed)
    return (g.standard_normal((c, d)) * scale / math.sqrt(d)).astype(np.float32), (g.standard_normal(c) * 0.5).astype(np.float32)


def theta_fun(x, y, c, l2, cw=None):
    d = x.shape[1]

    def fun(theta):
        f, gw, gb = objective_numpy(x, y, theta[:c * d].reshape(c, d), theta[c * d:], l2, cw)
        return f, np.concatenate([gw.ravel(), gb])
    return fun


def scipy_optimum(x, y, c, l2, cw=None):
    """scipy's L-BFGS-B optimum of objective_numpy at gtol = 1e-9 -> (W [c,d], b [c] with mean 0)."""
    d = x.shape[1]
    res = minimize(theta_fun(x, y, c, l2, cw), np.zeros(c * d + c), jac=True, method="L-BFGS-B",
                   options=dict(gtol=1e-9, ftol=1e-15, maxiter=5000, maxfun=20000, maxcor=10))
    w, b = res.x[:c * d].reshape(c, d), res.x[c * d:]
    return w, b - b.mean()


def forward_loop(x, w, b):
    probs, labels = [], []
    for row in x:
        if row_skipped(row):
            probs.append([0.0] * len(b)); labels.append(-1)
            continue
        z = [math.fsum(float(a) * float(v) for a, v in zip(row, wc)) + float(bc) for wc, bc in zip(w, b)]
        m = max(z)
        e = [math.exp(v - m) for v in z]
        s = math.fsum(e)
        probs.append([v / s for v in e])
        l = 0
        for k in range(1, len(z)):
            if z[k] > z[l]:
                l = k
        labels.append(l)
    return np.array(probs), np.array(labels)


@pytest.mark.parametrize("n,c,seed", [(40, 5, 0), (17, 2, 1), (33, 17, 2)])
def test_forward_and_objective_match_a_per_row_loop(n, c, seed):
    x = unit_rows(n, 16, seed)
    w, b = params(c, 16, seed + 10)
    y = np.random.default_rng(seed).integers(-1, c, n).astype(np.int32)
    x[3, 2], x[5, 0], x[7, 15] = np.nan, np.inf, 1.5
    p, labels, best, margin, _ = forward_numpy(x, w, b)
    wp, wl = forward_loop(x, w, b)
    assert (labels == wl).all() and np.abs(p - wp).max() < 1e-14
    assert (labels[[3, 5, 7]] == -1).all() and (p[[3, 5, 7]] == 0).all() and (best[[3, 5, 7]] == 0).all() and (margin[[3, 5, 7]] == 0).all()
    ok = labels >= 0
    srt = np.sort(wp[ok], axis=1)
    assert np.abs(best[ok] - srt[:, -1]).max() < 1e-14 and np.abs(margin[ok] - (srt[:, -1] - srt[:, -2])).max() < 1e-14
    cw = np.random.default_rng(seed + 1).uniform(0.2, 1.0, c)
    l2 = 0.01
    f, _, _ = objective_numpy(x, y, w, b, l2, cw)
    num = den = 0.0
    for i in range(n):
        if wl[i] < 0 or y[i] < 0:
            continue
        num += cw[y[i]] * -math.log(wp[i, y[i]])
        den += cw[y[i]]
    want = num / den + 0.5 * l2 * float((w.astype(np.float64) ** 2).sum())
    assert abs(f - want) < 1e-12
    assert kept_numpy(x, y).sum() == sum(1 for i in range(n) if wl[i] >= 0 and y[i] >= 0)


def test_gradient_matches_central_differences():
    n, d, c = 50, 16, 4
    x, y = fit_problem(n, d, c, 0.5, 0)
    y[4] = -1
    x[6, 1] = 1.5
    w, b = params(c, d, 1)
    cw = np.array([1.0, 0.5, 0.25, 0.8])
    fun = theta_fun(x, y, c, 0.01, cw)
    theta = np.concatenate([w.ravel().astype(np.float64), b.astype(np.float64)])
    _, g = fun(theta)
    h = 1e-6
    for k in list(range(0, c * d, 7)) + list(range(c * d, c * d + c)):
        e = np.zeros_like(theta)
        e[k] = h
        num = (fun(theta + e)[0] - fun(theta - e)[0]) / (2 * h)
        assert abs(num - g[k]) < 1e-8, (k, num, g[k])


@pytest.mark.parametrize("n,d,c,sep", [(300, 48, 3, 0.6), (65, 16, 2, 1.0), (120, 32, 5, 0.5)])
def test_lbfgs_reaches_scipys_optimum(n, d, c, sep):
    x, y = fit_problem(n, d, c, sep, 0)
    l2 = 1e-3
    ws, bs = scipy_optimum(x, y, c, l2)
    res = lbfgs(theta_fun(x, y, c, l2), np.zeros(c * d + c), gtol=1e-8, max_iter=5000)
    assert res.converged and res.stop_reason == "converged" and np.abs(res.g).max() <= 1e-8
    w, b = res.theta[:c * d].reshape(c, d), res.theta[c * d:]
    b = b - b.mean()
    f_s = objective_numpy(x, y, ws, bs, l2)[0]
    print(f"n={n} d={d} c={c}: {res.n_iter} iterations, {res.n_eval} evaluations, f - f_scipy = {res.f - f_s:.3g}, "
          f"max|dW| {np.abs(w - ws).max():.3g}, max|db| {np.abs(b - bs).max():.3g}")
    # F is l2-strongly convex in W: |W - W*| <= |g| / l2; both optimisers stop at |g|inf <= 1e-8 .. 1e-9, the bias follows the curvature
    assert abs(res.f - f_s) < 1e-10
    assert np.abs(w - ws).max() < 1e-4 and np.abs(b - bs).max() < 1e-4


def test_objective_equals_sklearns_for_three_classes():
    from sklearn.linear_model import LogisticRegression
    n, d, c, l2 = 300, 48, 3, 1e-3
    x, y = fit_problem(n, d, c, 0.6, 0)
    clf = LogisticRegression(C=1.0 / (l2 * n), tol=1e-10, max_iter=10000).fit(x.astype(np.float64), y)
    f_sk = objective_numpy(x, y, clf.coef_, clf.intercept_, l2)[0]
    res = lbfgs(theta_fun(x, y, c, l2), np.zeros(c * d + c), gtol=1e-8, max_iter=5000)
    w = res.theta[:c * d].reshape(c, d)
    print(f"objective {res.f:.15g} against sklearn's {f_sk:.15g}; max|dW| {np.abs(w - clf.coef_).max():.3g}")
    assert abs(res.f - f_sk) < 1e-9
    assert np.abs(w - clf.coef_).max() < 1e-3


def test_lbfgs_noise_rule_and_stall():
    n, d, c, l2 = 120, 32, 5, 1e-3
    x, y = fit_problem(n, d, c, 0.5, 0)
    exact = theta_fun(x, y, c, l2)
    g = np.random.default_rng(0)

    def noisy(theta):                                                    # a loss that jitters by 1e-6, an exact gradient
        f, gr = exact(theta)
        return f + 1e-6 * g.uniform(-1, 1), gr
    res = lbfgs(noisy, np.zeros(c * d + c), gtol=1e-6, max_iter=2000, noise=2e-6)
    assert res.converged, res.stop_reason                                # the decisions rest on the gradient once the decrease is in the noise

    def noisy_grad(theta):
        f, gr = exact(theta)
        return f, gr + 1e-5 * g.uniform(-1, 1, gr.shape)
    res = lbfgs(noisy_grad, np.zeros(c * d + c), gtol=1e-9, max_iter=2000)
    assert not res.converged and res.stop_reason in ("stalled", "max_iter")
    res = lbfgs(exact, np.zeros(c * d + c), gtol=1e-12, max_iter=3)
    assert not res.converged and res.stop_reason == "max_iter" and res.n_iter == 3


@pytest.mark.parametrize("n,d,c,seed", [(257, 48, 3, 0), (1000, 272, 17, 1), (300, 768, 8, 2)])
def test_integer_sums_round_within_their_bound(n, d, c, seed):
    x = unit_rows(n, d, seed)
    w, b = params(c, d, seed + 5)
    y = np.random.default_rng(seed).integers(0, c, n).astype(np.int32)
    cw = check_class_weight(np.random.default_rng(seed + 1).uniform(0.2, 1.0, c), c)
    p64, _, _, _, z = forward_numpy(x, w, b)
    p32 = p64.astype(np.float32)
    row_loss = (np.log(np.exp(z - z.max(1, keepdims=True)).sum(1)) + z.max(1) - z[np.arange(n), y]).astype(np.float32)
    words = loss_grad_numpy(x, y, p32, cw, row_loss)
    # the float64 sums of the SAME residuals: r from the fp32 probabilities, products and sums in float64
    onehot = np.zeros((n, c))
    onehot[np.arange(n), y] = 1.0
    r = (cw[y][:, None] * (p32 - onehot.astype(np.float32))).astype(np.float64)
    bound = n * (2.0 ** -24 + 2.0 ** -31)
    err_g = np.abs(words["grad"] / GRAD_ONE - r.T @ x.astype(np.float64)).max()
    err_b = np.abs(words["gbias"] / GRAD_ONE - r.sum(0)).max()
    err_l = abs(words["loss"] / LOSS_ONE - float((cw[y].astype(np.float64) * row_loss).sum()))
    print(f"n={n} d={d} c={c}: grad {err_g:.3g}, gbias {err_b:.3g} (bound {bound:.3g}); loss {err_l:.3g}")
    assert err_g <= bound and err_b <= bound
    assert err_l <= n * (2.0 ** -24 * float(np.abs(row_loss).max()) + 2.0 ** -25)
    assert (words["counts"] == np.bincount(y, minlength=c)).all() and words["skipped"] == 0
    f, gw, gb = objective_from_words(words, cw, w, b, 0.01)
    f64, gw64, gb64 = objective_numpy(x, y, w, b, 0.01, cw)
    assert abs(f - f64) < 1e-6 and np.abs(gw - gw64).max() < 1e-6 and np.abs(gb - gb64).max() < 1e-6


def test_sums_leave_out_skipped_and_unlabelled_rows_and_add_over_splits():
    n, d, c = 70, 16, 3
    x = unit_rows(n, d, 0)
    w, b = params(c, d, 1)
    y = (np.arange(n) % c).astype(np.int32)
    x[3, 2], x[5, 0], x[7, 15] = np.nan, -np.inf, 1.5
    y[[9, 11]] = -1
    p = forward_numpy(x, w, b)[0].astype(np.float32)
    rl = np.ones(n, np.float32)
    words = loss_grad_numpy(x, y, p, None, rl)
    assert words["skipped"] == 3 and words["counts"].sum() == n - 5 and words["loss"] == (n - 5) * LOSS_ONE
    keep = kept_numpy(x, y)
    only = loss_grad_numpy(x[keep], y[keep], p[keep], None, rl[keep])
    assert (only["grad"] == words["grad"]).all() and (only["gbias"] == words["gbias"]).all()
    parts = loss_grad_numpy(x[:1], y[:1], p[:1], None, rl[:1])
    parts = loss_grad_numpy(x[1:], y[1:], p[1:], None, rl[1:], into=parts)
    for k in words:
        assert np.array_equal(parts[k], words[k]), k
    # all rows of one class: the gradient rows sum to zero over the classes up to one rounding per term
    y1 = np.full(n, 1, np.int32)
    one = loss_grad_numpy(x, y1, p, None)
    assert one["counts"].tolist() == [0, n - 3, 0] and abs(int(one["gbias"].sum())) <= n


def test_class_weight():
    assert check_class_weight(None, 3).tolist() == [1, 1, 1]
    w = check_class_weight([2.0, 4.0, 1.0], 3)
    assert w.dtype == np.float32 and w.tolist() == [0.5, 1.0, 0.25]
    bal = check_class_weight("balanced", 3, np.array([10, 20, 40]))
    want = 70 / (3 * np.array([10.0, 20.0, 40.0]))
    assert np.allclose(bal, want / want.max()) and bal.max() == 1.0
    # a balanced fit weights every class alike: the weighted objective of a constant predictor is log C whatever the class sizes
    x, y = fit_problem(90, 16, 3, 0.5, 0)
    y[:45] = 0
    cw = check_class_weight("balanced", 3, np.bincount(y, minlength=3))
    f, _, _ = objective_numpy(x, y, np.zeros((3, 16)), np.zeros(3), 0.0, cw)
    assert abs(f - math.log(3)) < 1e-12
    for bad in ("even", [1.0, 2.0], [1.0, 0.0, 2.0], [1.0, -1.0, 2.0], [1.0, np.nan, 2.0], [1.0, 1e-60, 1.0]):
        with pytest.raises(ValueError):
            check_class_weight(bad, 3)
    with pytest.raises(ValueError):
        check_class_weight("balanced", 3)
    with pytest.raises(ValueError):
        check_class_weight("balanced", 3, np.array([4, 0, 2]))


def test_probe_sums_views_and_claims():
    s = ProbeSums(3, 16)
    assert s.grad.shape == (3, 16) and s.gbias.shape == (3,) and s.loss.shape == (1,) and s.counts.shape == (3,) and s.skipped.shape == (1,)
    assert s.buf.numel() == 3 * 16 + 3 + 1 + 3 + 1
    s.buf.copy_(torch.arange(s.buf.numel()))
    h = s.host()
    assert h["grad"][2, 15] == 47 and h["gbias"].tolist() == [48, 49, 50] and h["loss"] == 51 and h["counts"].tolist() == [52, 53, 54]
    assert h["skipped"] == 55
    s.claim(1 << 24)
    with pytest.raises(ValueError):
        s.claim(1)
    assert s.zero_().tiles == 0 and int(s.buf.abs().sum()) == 0
    with pytest.raises(ValueError):
        s.check(4, 16)
    with pytest.raises(ValueError):
        ProbeSums(1, 16)
    with pytest.raises(ValueError):
        ProbeSums(3, 24)


def test_argument_checks():
    for bad in (1, 65, 2.0, True, "3"):
        with pytest.raises(ValueError):
            check_n_classes(bad)
    w, b = params(3, 16, 0)
    assert check_weights(w, b, 16) == (3, 16)
    assert check_weights(torch.from_numpy(w), torch.from_numpy(b)) == (3, 16)
    for bw, bb in ((w[0], b), (w.astype(np.float64), b), (w, b.astype(np.float64)), (w, b[:2]), (w[:1], b[:1]), (w[:, :8], b),
                   (np.full((3, 16), np.nan, np.float32), b), (w * 1e5, b), (w, b + 9000)):
        with pytest.raises(ValueError):
            check_weights(bw, bb)
    with pytest.raises(ValueError):
        check_weights(w, b, 32)
    for bad in (dict(l2=-1.0), dict(l2=float("nan")), dict(l2="1"), dict(gtol=0.0), dict(gtol=float("inf")), dict(max_iter=-1), dict(max_iter=1.5)):
        with pytest.raises(ValueError):
            check_fit(**{**dict(l2=1e-3, gtol=1e-4, max_iter=10), **bad})
    assert check_fit(0, 1e-4, 0) == (0.0, 1e-4, 0)
    w0, b0 = check_init(None, 3, 16)
    assert w0.shape == (3, 16) and not w0.any() and not b0.any()
    assert check_init((w, b), 3, 16)[0].dtype == np.float64
    for bad in ((w,), (w, b[:2]), "zeros", (w[:2], b[:2])):
        with pytest.raises(ValueError):
            check_init(bad, 3, 16)
    x = unit_rows(10, 16, 0)
    y = np.zeros(10, np.int32)
    p = np.full((10, 3), 1 / 3, np.float32)
    for bx, by, bp in ((x, y.astype(np.int64), p), (x, y[:9], p), (x, y, p.astype(np.float64)), (x, y, p[:9]), (x, y + 3, p), (x, y - 2, p)):
        with pytest.raises(ValueError):
            loss_grad_numpy(bx, by, bp)
    with pytest.raises(ValueError):
        loss_grad_numpy(x, y, p, np.array([2.0, 1.0, 1.0], np.float32))
    with pytest.raises(ValueError):
        loss_grad_numpy(x, y, p, None, np.ones(10))
    with pytest.raises(ValueError):
        objective_numpy(x, np.full(10, -1, np.int32), w, b)
    with pytest.raises(ValueError):
        objective_numpy(x, y, w[:, :8], b)
    with pytest.raises(ValueError):
        objective_from_words(dict(loss=0, grad=np.zeros((3, 16), np.int64), gbias=np.zeros(3, np.int64), counts=np.zeros(3, np.int64)),
                             np.ones(3, np.float32), w, b, 0.0)
    assert loss_noise(np.zeros((3, 16)), np.zeros(3)) == 2.0 ** -20 * (math.log(3) + 1)


def test_engine_methods_check_their_arguments_before_any_device_work():
    m = KEEPModel()
    x = unit_rows(10, 16, 0)
    y = np.zeros(10, np.int32)
    w, b = params(3, 16, 0)
    with pytest.raises(ValueError):
        m.probe_predict((w, b), x[:, :8])
    with pytest.raises(ValueError):
        m.probe_predict((w[:1], b[:1]), x)
    with pytest.raises(ValueError):
        m.probe_loss_grad(x, y.astype(np.int64), w, b, ProbeSums(3, 16))
    with pytest.raises(ValueError):
        m.probe_loss_grad(x, y, w, b, None)
    with pytest.raises(ValueError):
        m.probe_loss_grad(x, y, w, b, ProbeSums(4, 16))
    with pytest.raises(ValueError):
        m.probe_loss_grad(x, y, w, b, ProbeSums(3, 16), class_weight=np.ones(3))
    with pytest.raises(ValueError):
        m.probe_fit(x, y, 1)
    with pytest.raises(ValueError):
        m.probe_fit(x, y, 3, l2=-1)
    with pytest.raises(ValueError):
        m.probe_fit(x, y, 3, classes=("a", "b"))
    with pytest.raises(ValueError):
        m.probe_fit_batches([(x, y)], 3, 16)
    with pytest.raises(ValueError):
        wsi.probe_map((w, b), x, np.zeros((9, 2), np.int64), 16, (8, 8), model=m)
