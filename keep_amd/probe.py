"""Linear probe: multinomial logistic regression with L2 on unit feature rows, its integer accumulators, the
host restatements the device kernel is held to, and the L-BFGS that drives the fit.

The device side is ``KEEPModel.probe_loss_grad`` / ``probe_predict`` / ``probe_fit`` / ``probe_fit_batches`` (``keep_amd.slide``),
``wsi.probe_map`` and ``tile_eval.linear_probe``; this file has no device code.  What both sides share:

* the objective ``F(W, b) = (1/S) sum_i w[y_i] loss_i + (l2/2) |W|^2`` with ``loss_i = logsumexp(z_i) - z_i[y_i]``, ``z_i = W x_i + b``
  and ``S = sum_i w[y_i]`` over the kept rows; the bias is not penalised;
* a row is *skipped* when it holds a non-finite value or an element with ``|x| > 1`` (label -1, a zero row of probabilities, in no
  sum); a row with label -1 is *unlabelled*: in no sum, still predicted;
* the label is the first maximum of the logits, ``margin`` the lead of its probability over the runner-up's;
* the sums are integers: with ``r_ic = fp32(w[y_i]) * (p_ic - [c = y_i])`` in fp32, ``grad[c,d] += rint(fp32(r_ic x_id) 2^30)``,
  ``gbias[c] += rint(r_ic 2^30)``, ``loss += rint(fp32(w[y_i] loss_i) 2^24)``.  Every term is rounded before it is added, so the words do
  not depend on the order of the rows or on their split over calls.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Sequence, Tuple

import numpy as np
import torch

from .cluster import MAX_TILES, _is_f32, check_dim, check_features, skipped_numpy

MAX_C = 64
GRAD_ONE = 1 << 30
LOSS_ONE = 1 << 24
MAX_LOGIT = 8192.0                  # max_c(|w_c| + |b_c|): loss_i <= 2 max|z| + log C < 2^15 keeps the loss word exact
MEMORY = 10


# ------------------------------------------------------------------------------------------------ argument checks
def check_n_classes(c) -> int:
    if isinstance(c, bool) or not isinstance(c, (int, np.integer)):
        raise ValueError(f"the number of classes must be an integer, got {c!r}")
    if c < 2 or c > MAX_C:
        raise ValueError(f"the number of classes must be in 2..{MAX_C}, got {int(c)}")
    return int(c)


def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def check_weights(weight, bias, dim: Optional[int] = None, values: bool = True) -> Tuple[int, int]:
    """``weight`` fp32 ``[C, D]`` and ``bias`` fp32 ``[C]``, numpy or torch, finite, ``max_c(|w_c| + |b_c|) <= 8192`` -> (C, D).
    ``values=False`` checks shapes and types only (no copy of device tensors to the host: the forward skips a row whose logits are
    not finite, and only the loss word needs the limit)."""
    ws, bs = tuple(weight.shape), tuple(bias.shape)
    if len(ws) != 2:
        raise ValueError(f"weight must be [C, D], got shape {ws}")
    if not _is_f32(weight.dtype) or not _is_f32(bias.dtype):
        raise ValueError(f"weight and bias must be float32, got {weight.dtype} and {bias.dtype}")
    c, d = check_n_classes(int(ws[0])), check_dim(ws[1])
    if bs != (c,):
        raise ValueError(f"bias must be [{c}] beside weight {ws}, got shape {bs}")
    if dim is not None and d != dim:
        raise ValueError(f"weight has width {d}, the features {dim}")
    if not values:
        return c, d
    w, b = _host(weight).astype(np.float64), _host(bias).astype(np.float64)
    size = np.sqrt((w * w).sum(axis=1)) + np.abs(b)
    if not np.isfinite(size).all():
        raise ValueError("weight and bias must be finite")
    if size.max() > MAX_LOGIT:
        raise ValueError(f"max_c(|w_c| + |b_c|) = {size.max():.6g} is above {MAX_LOGIT:g}: the loss word would not hold a row's loss")
    return c, d


def check_labels(labels, n: int) -> None:
    """int32 ``[n]``; the values (-1 .. C - 1) are checked where they are used: on the device by the launch, here by the restatements."""
    shape = tuple(labels.shape)
    if shape != (n,):
        raise ValueError(f"labels must hold one label per row, [{n}], got shape {shape}")
    if not (labels.dtype == torch.int32 if isinstance(labels.dtype, torch.dtype) else np.dtype(labels.dtype) == np.int32):
        raise ValueError(f"labels must be int32, got {labels.dtype}")


def check_label_values(labels: np.ndarray, c: int) -> None:
    if labels.size and (labels.min() < -1 or labels.max() >= c):
        raise ValueError(f"labels must lie in -1..{c - 1}, got {int(labels.min())}..{int(labels.max())}")


def check_class_weight(class_weight, c: int, counts=None) -> np.ndarray:
    """``None`` (all 1), ``"balanced"`` (``n / (C count_c)`` of the labelled rows, ``counts`` int ``[C]`` required) or ``[C]`` positive
    finite numbers -> fp32 ``[C]`` divided by its maximum, so every weight lies in (0, 1]."""
    if class_weight is None:
        return np.ones(c, np.float32)
    if isinstance(class_weight, str):
        if class_weight != "balanced":
            raise ValueError(f'class_weight must be None, "balanced" or [C] numbers, got {class_weight!r}')
        if counts is None:
            raise ValueError('class_weight="balanced" needs the labels\' class counts')
        n = np.asarray(_host(counts), np.float64)
        if n.shape != (c,) or (n <= 0).any():
            raise ValueError(f'class_weight="balanced" needs at least one labelled row of each of the {c} classes, got counts {n.tolist()}')
        w = n.sum() / (c * n)
    else:
        w = np.asarray(_host(class_weight), np.float64)
        if w.shape != (c,):
            raise ValueError(f"class_weight must be [{c}], got shape {w.shape}")
        if not np.isfinite(w).all() or (w <= 0).any():
            raise ValueError("class_weight must be finite and positive")
    out = (w / w.max()).astype(np.float32)
    if (out <= 0).any():
        raise ValueError("a class weight is 0 in float32 beside the largest: the range of class_weight is too wide")
    return out


def check_fit(l2, gtol, max_iter) -> Tuple[float, float, int]:
    if isinstance(l2, bool) or not isinstance(l2, (int, float, np.integer, np.floating)) or not np.isfinite(l2) or l2 < 0:
        raise ValueError(f"l2 must be a finite number >= 0, got {l2!r}")
    if isinstance(gtol, bool) or not isinstance(gtol, (int, float, np.integer, np.floating)) or not gtol > 0 or not np.isfinite(gtol):
        raise ValueError(f"gtol must be a finite number > 0, got {gtol!r}")
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 0:
        raise ValueError(f"max_iter must be an integer >= 0, got {max_iter!r}")
    return float(l2), float(gtol), int(max_iter)


def check_init(init, c: int, d: int) -> Tuple[np.ndarray, np.ndarray]:
    """``None`` (zeros), a ``LinearProbe`` or a ``(weight [C, D], bias [C])`` pair -> float64 copies on the host."""
    if init is None:
        return np.zeros((c, d)), np.zeros(c)
    if isinstance(init, LinearProbe):
        init = (init.weight, init.bias)
    if not isinstance(init, (tuple, list)) or len(init) != 2:
        raise ValueError(f"init must be None, a LinearProbe or a (weight, bias) pair, got {type(init).__name__}")
    w, b = (np.array(_host(a), np.float64) for a in init)
    if w.shape != (c, d) or b.shape != (c,):
        raise ValueError(f"init must be weight [{c}, {d}] and bias [{c}], got {w.shape} and {b.shape}")
    return w, b


# ------------------------------------------------------------------------------------------------ results
class ProbeSums:
    """The integer accumulators of one loss + gradient evaluation as one object: ``grad`` int64 ``[C, D]`` and ``gbias`` int64 ``[C]``
    (2^30 fixed point), ``loss`` int64 ``[1]`` (2^24 fixed point), ``counts`` int64 ``[C]`` (kept rows per class) and ``skipped`` int64
    ``[1]``.  All views share one buffer, so :meth:`zero_` is one fill and one copy brings everything to the host.  ``tiles`` counts the
    rows added since the last :meth:`zero_` (at most 2^24)."""

    def __init__(self, n_classes: int, dim: int, device="cpu"):
        self.c, self.dim = check_n_classes(n_classes), check_dim(dim)
        cd, c = self.c * self.dim, self.c
        self.buf = torch.zeros(cd + 2 * c + 2, dtype=torch.int64, device=device)
        self.grad = self.buf[:cd].view(c, self.dim)
        self.gbias = self.buf[cd:cd + c]
        self.loss = self.buf[cd + c:cd + c + 1]
        self.counts = self.buf[cd + c + 1:cd + 2 * c + 1]
        self.skipped = self.buf[cd + 2 * c + 1:cd + 2 * c + 2]
        self.tiles = 0

    def zero_(self) -> "ProbeSums":
        self.buf.zero_()
        self.tiles = 0
        return self

    def check(self, n_classes: int, dim: int) -> None:
        if (self.c, self.dim) != (n_classes, dim):
            raise ValueError(f"the accumulators are for C = {self.c}, D = {self.dim}; the call has C = {n_classes}, D = {dim}")

    def claim(self, n: int) -> None:
        if self.tiles + n > MAX_TILES:
            raise ValueError(f"accumulators take at most 2^24 = {MAX_TILES} rows in all, got {self.tiles} + {n}")
        self.tiles += n

    def host(self) -> dict:
        """One copy -> ``dict(grad, gbias, loss, counts, skipped)`` as numpy int64 arrays / Python ints."""
        return split_words(self.buf.cpu().numpy(), self.c, self.dim)


def split_words(buf: np.ndarray, c: int, d: int) -> dict:
    cd = c * d
    return dict(grad=buf[:cd].reshape(c, d), gbias=buf[cd:cd + c], loss=int(buf[cd + c]), counts=buf[cd + c + 1:cd + 2 * c + 1],
                skipped=int(buf[cd + 2 * c + 1]))


@dataclass
class LinearProbe:
    """A fitted probe: ``weight`` fp32 ``[C, D]`` and ``bias`` fp32 ``[C]`` (the point the last evaluation was made at), ``l2``,
    ``class_weight`` fp32 ``[C]`` in (0, 1] (numpy), ``classes`` (names or None), ``n_iter`` / ``n_eval`` (L-BFGS iterations and
    loss + gradient evaluations), ``converged`` (``grad_norm <= gtol`` was reached), ``stop_reason`` (``"converged"``, ``"stalled"``:
    the line search found no acceptable step, which is what the fp32 evaluation noise does to a ``gtol`` below it, or
    ``"max_iter"``), ``loss`` (the objective), ``grad_norm`` (its gradient's largest magnitude), ``counts`` int64 ``[C]`` (the kept
    rows of each class) and ``skipped`` (rows the skip rule left out)."""
    weight: torch.Tensor
    bias: torch.Tensor
    l2: float
    class_weight: np.ndarray
    classes: Optional[Sequence[str]]
    n_iter: int
    n_eval: int
    converged: bool
    stop_reason: str
    loss: float
    grad_norm: float
    counts: torch.Tensor
    skipped: int

    @property
    def n_classes(self) -> int:
        return int(self.weight.shape[0])


# ------------------------------------------------------------------------------------------------ host restatements
def forward_numpy(x: np.ndarray, weight: np.ndarray, bias: np.ndarray):
    """The forward restated in float64 -> (probs [N, C], labels int32 [N], best [N], margin [N], logits [N, C]).  A skipped row has a
    zero row of probabilities, label -1 and best = margin = 0."""
    n, d = check_features(x)
    c, _ = check_weights(weight, bias, d)
    skip = skipped_numpy(x)
    z = np.where(skip[:, None], 0.0, x.astype(np.float64)) @ weight.astype(np.float64).T + bias.astype(np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    labels = z.argmax(axis=1).astype(np.int32)                           # the first maximum
    best = p[np.arange(n), labels]
    rest = p.copy()
    rest[np.arange(n), labels] = -np.inf
    margin = best - rest.max(axis=1)
    p[skip], labels[skip], best[skip], margin[skip] = 0.0, -1, 0.0, 0.0
    return p, labels, best, margin, z


def kept_numpy(x: np.ndarray, labels: np.ndarray) -> np.ndarray:
    """bool [N]: the rows that enter the sums (not skipped, label >= 0)."""
    return ~skipped_numpy(x) & (labels >= 0)


def loss_grad_numpy(x: np.ndarray, labels: np.ndarray, probs: np.ndarray, class_weight: Optional[np.ndarray] = None,
                    row_loss: Optional[np.ndarray] = None, into: Optional[dict] = None) -> dict:
    """The integer sums from given fp32 probabilities ``[N, C]``, rounded as the device rounds them -> ``dict(grad int64 [C, D], gbias
    int64 [C], loss, counts int64 [C], skipped)``.  ``row_loss``: the rows' ``logsumexp(z) - z[y]`` in fp32 (``loss`` is 0 without it: it
    does not follow from rounded probabilities); ``into`` (such a dict) is added to."""
    n, d = check_features(x)
    if probs.ndim != 2 or probs.shape[0] != n or np.dtype(probs.dtype) != np.float32:
        raise ValueError(f"probs must be float32 [{n}, C], got {probs.dtype} {probs.shape}")
    c = check_n_classes(int(probs.shape[1]))
    check_labels(labels, n)
    check_label_values(labels, c)
    w = check_class_weight(class_weight, c)
    if class_weight is not None and not np.array_equal(w, np.asarray(class_weight, np.float32)):
        raise ValueError("class_weight must be float32 in (0, 1] with a largest weight of 1 here (check_class_weight makes it so)")
    kept = kept_numpy(x, labels)
    xk, yk, pk = x[kept], labels[kept], probs[kept]
    onehot = np.zeros_like(pk)
    onehot[np.arange(len(yk)), yk] = 1.0
    r = w[yk][:, None] * (pk - onehot)                                   # fp32: the subtraction, then the product
    grad = np.zeros((c, d), np.int64)
    for k in range(c):
        grad[k] = np.rint((r[:, k:k + 1] * xk).astype(np.float64) * GRAD_ONE).astype(np.int64).sum(axis=0)
    out = dict(grad=grad, gbias=np.rint(r.astype(np.float64) * GRAD_ONE).astype(np.int64).sum(axis=0),
               loss=0, counts=np.bincount(yk, minlength=c).astype(np.int64), skipped=int(skipped_numpy(x).sum()))
    if row_loss is not None:
        if row_loss.shape != (n,) or np.dtype(row_loss.dtype) != np.float32:
            raise ValueError(f"row_loss must be float32 [{n}], got {row_loss.dtype} {row_loss.shape}")
        out["loss"] = int(np.rint((w[yk] * row_loss[kept]).astype(np.float64) * LOSS_ONE).astype(np.int64).sum())
    if into is not None:
        out = {k: into[k] + v for k, v in out.items()}
    return out


def objective_numpy(x: np.ndarray, labels: np.ndarray, weight: np.ndarray, bias: np.ndarray, l2: float = 0.0,
                    class_weight: Optional[np.ndarray] = None):
    """The objective and its gradient in float64 -> ``(F, dF/dW [C, D], dF/db [C])``.  ``weight`` / ``bias`` of any float type are
    used as float64; ``class_weight``: ``[C]`` as given (None: all 1)."""
    n, d = check_features(x)
    w64, b64 = np.asarray(weight, np.float64), np.asarray(bias, np.float64)
    c = check_n_classes(int(w64.shape[0]))
    if w64.shape != (c, d) or b64.shape != (c,):
        raise ValueError(f"weight must be [C, {d}] and bias [C], got {w64.shape} and {b64.shape}")
    check_labels(labels, n)
    check_label_values(labels, c)
    cw = np.ones(c) if class_weight is None else np.asarray(class_weight, np.float64)
    kept = kept_numpy(x, labels)
    if not kept.any():
        raise ValueError("no labelled row is kept: the objective is undefined")
    xk, yk = x[kept].astype(np.float64), labels[kept]
    z = xk @ w64.T + b64
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(axis=1, keepdims=True)
    rows = np.arange(len(yk))
    wy = cw[yk]
    S = wy.sum()
    f = float((wy * ((m + np.log(s))[:, 0] - z[rows, yk])).sum() / S + 0.5 * l2 * (w64 * w64).sum())
    r = e / s
    r[rows, yk] -= 1.0
    r *= wy[:, None]
    return f, r.T @ xk / S + l2 * w64, r.sum(axis=0) / S


def objective_from_words(words: dict, class_weight: np.ndarray, weight: np.ndarray, bias: np.ndarray, l2: float):
    """The objective and its gradient from the integer sums of one evaluation -> ``(F, dF/dW, dF/db)`` in float64: the words scaled by
    their fixed point and by ``1 / S``, ``S = sum_c float64(class_weight[c]) counts[c]``, plus the penalty at ``weight``."""
    S = float((np.asarray(class_weight, np.float64) * words["counts"]).sum())
    if not S > 0:
        raise ValueError("no labelled row is kept: the objective is undefined")
    w64 = np.asarray(weight, np.float64)
    f = words["loss"] / LOSS_ONE / S + 0.5 * l2 * float((w64 * w64).sum())
    return f, words["grad"].astype(np.float64) / GRAD_ONE / S + l2 * w64, words["gbias"].astype(np.float64) / GRAD_ONE / S


def loss_noise(weight: np.ndarray, bias: np.ndarray) -> float:
    """What the line search takes as the noise of one evaluated loss: ``2^-20 (2 zmax + log C + 1)`` with ``zmax = max_c(|w_c| + |b_c|)``,
    sixteen times the rounding unit of a row's fp32 loss."""
    w, b = np.asarray(weight, np.float64), np.asarray(bias, np.float64)
    zmax = float((np.sqrt((w * w).sum(axis=1)) + np.abs(b)).max())
    return 2.0 ** -20 * (2.0 * zmax + np.log(w.shape[0]) + 1.0)


# ------------------------------------------------------------------------------------------------ optimiser
@dataclass
class LbfgsResult:
    theta: np.ndarray
    f: float
    g: np.ndarray
    n_iter: int
    n_eval: int
    converged: bool
    stop_reason: str


def lbfgs(fun: Callable, theta0: np.ndarray, gtol: float = 1e-4, max_iter: int = 1000, memory: int = MEMORY, noise=0.0,
          c1: float = 1e-4, c2: float = 0.9, max_ls: int = 30) -> LbfgsResult:
    """L-BFGS (two-loop recursion) for a CONVEX ``fun: theta -> (f, g)`` in numpy float64; stops when ``max|g| <= gtol``.

    The line search brackets the zero of the directional derivative ``g(theta + t d) . d``, which a convex function has increasing in
    t, and accepts a step with ``|g1 . d| <= c2 |g0 . d|``.  The loss enters through one test only, ``f1 <= f0 + c1 t g0 . d + noise``:
    a step that raises the loss by more than the noise went too far.  Once the decrease is under the noise that test always passes
    and the step is accepted on the derivative alone, so no decision rests on a loss difference smaller than ``noise`` (a number, or
    a callable ``theta -> number``).  ``stop_reason``: ``"converged"``, ``"max_iter"`` or ``"stalled"`` (no acceptable step within
    ``max_ls`` evaluations: the gradient's own noise has been reached)."""
    theta = np.array(theta0, np.float64)
    f, g = fun(theta)
    n_eval, mem = 1, []
    for it in range(max_iter + 1):
        if np.abs(g).max() <= gtol:
            return LbfgsResult(theta, f, g, it, n_eval, True, "converged")
        if it == max_iter:
            break
        q, alphas = g.copy(), []
        for s, y, rho in reversed(mem):
            a = rho * (s @ q)
            q -= a * y
            alphas.append(a)
        if mem:
            s, y, _ = mem[-1]
            q *= (s @ y) / (y @ y)
        for (s, y, rho), a in zip(mem, reversed(alphas)):
            q += (a - rho * (y @ q)) * s
        d, gd = -q, -(g @ q)
        if not gd < 0:                                                   # not a descent direction: start over from the gradient
            mem, d, gd = [], -g, -(g @ g)
        t = 1.0 if mem else min(1.0, 1.0 / np.abs(g).sum())
        eps = float(noise(theta)) if callable(noise) else float(noise)
        lo, dlo, hi, dhi, found = 0.0, gd, np.inf, None, False
        for _ in range(max_ls):
            th1 = theta + t * d
            f1, g1 = fun(th1)
            n_eval += 1
            gd1 = g1 @ d
            if f1 > f + c1 * t * gd + eps or gd1 > -c2 * gd:             # too far
                hi, dhi = t, (gd1 if gd1 > 0 else None)
            elif gd1 < c2 * gd:                                          # still going down steeply: not far enough
                lo, dlo = t, gd1
            else:
                found = True
                break
            if np.isinf(hi):
                t = min(max(2.0 * t, t - gd1 * t / (gd1 - gd) if gd1 > gd else 10.0 * t), 10.0 * t)
            else:
                width = hi - lo
                t = lo + width * (-dlo / (dhi - dlo)) if dhi is not None else lo + 0.5 * width
                t = min(max(t, lo + 0.1 * width), hi - 0.1 * width)
                if not width > 1e-16 * max(hi, 1.0):
                    break
        if not found:
            return LbfgsResult(theta, f, g, it, n_eval, False, "stalled")
        s, y = th1 - theta, g1 - g
        if s @ y > 1e-10 * (y @ y):
            mem.append((s, y, 1.0 / (s @ y)))
            mem = mem[-memory:]
        theta, f, g = th1, f1, g1
    return LbfgsResult(theta, f, g, max_iter, n_eval, False, "max_iter")
