"""Attention-based multiple-instance learning: a slide is a bag of unit feature rows, a small network gives every
row a weight, the weighted mean is the slide embedding and a linear head classifies it (Ilse, Tomczak and Welling 2018; CLAM's pooling).
This file has the argument checks, the chunk table, the integer accumulators, the float64 restatements the device kernels are held to
and the Adam that drives the fit; it has no device code.

The device side is ``KEEPModel.mil_forward`` / ``mil_loss_grad`` / ``mil_predict`` / ``mil_fit`` / ``mil_fit_batches`` (``keep_amd.slide``),
``wsi.mil_attention_map`` and ``tile_eval.attention_mil``.  What both sides share:

* features ``x`` fp32 ``[N, D]``, bags the row ranges ``offsets[b] .. offsets[b + 1]`` (int64 ``[S + 1]``, an empty bag allowed), bag labels
  int32 ``[S]`` with -1 for a bag to leave out; parameters ``(V [L, D], bv [L], w [L], Wc [C, D], bc [C])``, L a multiple of 16 in 16..128;
* ``h_i = tanh(V x_i + bv)``, ``s_i = w . h_i``, ``a_i = softmax of s over the bag``, ``z_b = sum_i a_i x_i``, ``logits_b = Wc z_b + bc`` and
  ``F = (1/S_w) sum_b cw[y_b] (logsumexp(logits_b) - logits_b[y_b]) + (l2/2)(|V|^2 + |w|^2 + |Wc|^2)``, ``S_w = sum_b cw[y_b]`` over the kept
  labelled bags; the biases are not penalised;
* a row is *skipped* when it holds a non-finite value or an element with ``|x| > 1``: attention 0, in no sum; a bag without a kept row
  is *skipped*: label -1, a zero row of probabilities, in no sum;
* the head is the linear probe's own evaluation (``keep_amd.probe``) on the pooled rows, its words at 2^30 and 2^24; the attention
  network's words ``gV [L, D]``, ``gbv [L]``, ``gw [L]`` are at 2^36.  A bag's contribution to every word depends on that bag alone, cut
  from its own first row into chunks of ``CHUNK`` rows: the words depend on ``CHUNK`` and on nothing else about the launch.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import bootstrap as _boot
from . import probe as _probe
from .cluster import _is_f32, check_dim, check_features, skipped_numpy

CHUNK = 512                         # KEEP_MIL_CHUNK of include/keep_hip.h: rows of a bag per chunk
MAX_L = 128
MAX_BAGS = 1 << 16                  # per call, and in all into one set of accumulators
POOL_ONE = 1 << 40                  # Z_b and P_b: e_i <= 1 and a bag of <= 2^22 rows stay under 2^62
GRAD_ONE = 1 << 36                  # gV, gbv, gw
MAX_GAIN = 1024.0                   # 4 max(1, |w|_inf) max_c |Wc_c|_1: what one bag can add to a word; 2^16 bags x 2^10 x 2^36 = 2^62
NAMES = ("V", "bv", "w", "Wc", "bc")


# ------------------------------------------------------------------------------------------------ argument checks
def check_hidden(hidden) -> int:
    if isinstance(hidden, bool) or not isinstance(hidden, (int, np.integer)):
        raise ValueError(f"the number of hidden units must be an integer, got {hidden!r}")
    if hidden < 16 or hidden > MAX_L or hidden % 16:
        raise ValueError(f"the number of hidden units must be a multiple of 16 in 16..{MAX_L}, got {int(hidden)}")
    return int(hidden)


def check_offsets(offsets, n: int) -> np.ndarray:
    """Bag offsets ``[S + 1]`` of any integer type, numpy or torch: ``offsets[0] = 0``, non-decreasing, ``offsets[S] = n``, ``1 <= S <= 2^16``
    -> int64 numpy."""
    o = _probe._host(offsets)
    if o.ndim != 1 or o.shape[0] < 2 or o.dtype.kind not in "iu":
        raise ValueError(f"offsets must be integers [S + 1] with S >= 1, got {o.dtype} {o.shape}")
    o = o.astype(np.int64)
    if o.shape[0] - 1 > MAX_BAGS:
        raise ValueError(f"at most 2^16 = {MAX_BAGS} bags per call, got {o.shape[0] - 1}")
    if o[0] != 0 or o[-1] != n:
        raise ValueError(f"offsets must start at 0 and end at the number of rows {n}, got {int(o[0])} .. {int(o[-1])}")
    if (np.diff(o) < 0).any():
        raise ValueError("offsets must be non-decreasing")
    return o


def chunk_table(offsets: np.ndarray, chunk: int = CHUNK) -> np.ndarray:
    """int32 ``[n_chunks, 3]`` of (bag, first row, rows): every bag cut from its own first row into runs of at most ``chunk`` rows; an
    empty bag has no chunk."""
    o = np.asarray(offsets, np.int64)
    sizes = np.diff(o)
    per = (sizes + chunk - 1) // chunk
    bag = np.repeat(np.arange(len(sizes), dtype=np.int64), per)
    k = np.arange(int(per.sum()), dtype=np.int64) - np.repeat(np.cumsum(per) - per, per)          # the chunk's number within its bag
    first = o[bag] + k * chunk
    rows = np.minimum(chunk, o[bag + 1] - first)
    return np.stack([bag, first, rows], axis=1).astype(np.int32).reshape(-1, 3)


def check_params(params, dim: Optional[int] = None, values: bool = True) -> Tuple[int, int, int]:
    """``(V [L, D], bv [L], w [L], Wc [C, D], bc [C])``, float32, numpy or torch -> (L, C, D).  With ``values``: finite, the head within
    the probe's limit, and ``4 max(1, max|w|) max_c |Wc_c|_1 <= 1024``, the bound that keeps the gradient words inside an int64."""
    if not isinstance(params, (tuple, list)) or len(params) != 5:
        raise ValueError("params must be (V, bv, w, Wc, bc)")
    V, bv, w, Wc, bc = params
    for name, a in zip(NAMES, params):
        if not _is_f32(a.dtype):
            raise ValueError(f"{name} must be float32, got {a.dtype}")
    if len(tuple(V.shape)) != 2:
        raise ValueError(f"V must be [L, D], got shape {tuple(V.shape)}")
    L, d = check_hidden(int(V.shape[0])), check_dim(V.shape[1])
    if tuple(bv.shape) != (L,) or tuple(w.shape) != (L,):
        raise ValueError(f"bv and w must be [{L}] beside V {tuple(V.shape)}, got {tuple(bv.shape)} and {tuple(w.shape)}")
    c, dc = _probe.check_weights(Wc, bc, None, values)
    if dc != d or (dim is not None and d != dim):
        raise ValueError(f"V has width {d}, Wc {dc}, the features {d if dim is None else dim}")
    if values:
        v64, bv64, w64, wc64 = (_probe._host(a).astype(np.float64) for a in (V, bv, w, Wc))
        if not (np.isfinite(v64).all() and np.isfinite(bv64).all() and np.isfinite(w64).all()):
            raise ValueError("V, bv and w must be finite")
        gain = 4.0 * max(1.0, float(np.abs(w64).max())) * float(np.abs(wc64).sum(axis=1).max())
        if gain > MAX_GAIN:
            raise ValueError(f"4 max(1, max|w|) max_c |Wc_c|_1 = {gain:.6g} is above {MAX_GAIN:g}: a gradient word would not hold 2^16 bags")
    return L, c, d


def check_adam(lr, n_steps) -> Tuple[float, int]:
    if isinstance(lr, bool) or not isinstance(lr, (int, float, np.integer, np.floating)) or not np.isfinite(lr) or not lr > 0:
        raise ValueError(f"lr must be a finite number > 0, got {lr!r}")
    if isinstance(n_steps, bool) or not isinstance(n_steps, (int, np.integer)) or n_steps < 0:
        raise ValueError(f"n_steps must be an integer >= 0, got {n_steps!r}")
    return float(lr), int(n_steps)


# ------------------------------------------------------------------------------------------------ parameters as one vector
def sizes(L: int, C: int, D: int) -> Tuple[int, ...]:
    return (L * D, L, L, C * D, C)


def pack(params) -> np.ndarray:
    return np.concatenate([np.asarray(_probe._host(a), np.float64).ravel() for a in params])


def unpack(theta: np.ndarray, L: int, C: int, D: int):
    """float64 ``theta`` -> views ``(V [L, D], bv [L], w [L], Wc [C, D], bc [C])``."""
    e = np.cumsum((0,) + sizes(L, C, D))
    return (theta[e[0]:e[1]].reshape(L, D), theta[e[1]:e[2]], theta[e[2]:e[3]], theta[e[3]:e[4]].reshape(C, D), theta[e[4]:e[5]])


def init_params(seed: int, L: int, C: int, D: int):
    """The initial values, float64: ``V`` and ``w`` uniform in ``+-1/sqrt(fan_in)`` from the counter-based generator of
    ``keep_amd.bootstrap`` (tensor t, element j: ``mix64(key(seed, t) + j G)``), the head and the biases zero."""
    seed = _boot.check_seed(seed)

    def uniform(t: int, n: int, bound: float) -> np.ndarray:
        with np.errstate(over="ignore"):
            u = _boot._mix64_np(np.uint64(_boot.key(seed, t)) + np.arange(n, dtype=np.uint64) * np.uint64(_boot.G))
        return ((u >> np.uint64(11)).astype(np.float64) * 2.0 ** -52 - 1.0) * bound
    return (uniform(0, L * D, D ** -0.5).reshape(L, D), np.zeros(L), uniform(1, L, L ** -0.5), np.zeros((C, D)), np.zeros(C))


# ------------------------------------------------------------------------------------------------ results
class MilSums:
    """The integer accumulators of one loss + gradient evaluation as one buffer: ``gV`` int64 ``[L, D]``, ``gbv`` and ``gw`` int64 ``[L]`` (2^36
    fixed point), the head's ``keep_amd.probe.ProbeSums`` (``head``: the gradient of ``Wc`` and ``bc`` at 2^30, the loss at 2^24, the kept
    labelled bags per class) and ``skipped_rows`` / ``skipped_bags`` int64 ``[1]``.  ``bags`` counts the bags added since the last
    :meth:`zero_` (at most 2^16)."""

    def __init__(self, hidden: int, n_classes: int, dim: int, device="cpu"):
        self.L, self.c, self.dim = check_hidden(hidden), _probe.check_n_classes(n_classes), check_dim(dim)
        ld, L = self.L * self.dim, self.L
        self.head = _probe.ProbeSums(self.c, self.dim, device)
        nh = self.head.buf.numel()
        self.buf = torch.zeros(ld + 2 * L + 2 + nh, dtype=torch.int64, device=device)
        self.gV = self.buf[:ld].view(L, self.dim)
        self.gbv = self.buf[ld:ld + L]
        self.gw = self.buf[ld + L:ld + 2 * L]
        self.skipped_rows = self.buf[ld + 2 * L:ld + 2 * L + 1]
        self.skipped_bags = self.buf[ld + 2 * L + 1:ld + 2 * L + 2]
        hb = self.buf[ld + 2 * L + 2:]
        cd, c = self.c * self.dim, self.c                               # the head's views moved into the one buffer
        self.head.buf, self.head.grad, self.head.gbias = hb, hb[:cd].view(c, self.dim), hb[cd:cd + c]
        self.head.loss, self.head.counts, self.head.skipped = hb[cd + c:cd + c + 1], hb[cd + c + 1:cd + 2 * c + 1], hb[cd + 2 * c + 1:cd + 2 * c + 2]
        self.bags = 0

    def zero_(self) -> "MilSums":
        self.buf.zero_()
        self.bags, self.head.tiles = 0, 0
        return self

    def check(self, hidden: int, n_classes: int, dim: int) -> None:
        if (self.L, self.c, self.dim) != (hidden, n_classes, dim):
            raise ValueError(f"the accumulators are for L = {self.L}, C = {self.c}, D = {self.dim}; the call has L = {hidden}, C = {n_classes}, "
                             f"D = {dim}")

    def claim(self, n_bags: int) -> None:
        if self.bags + n_bags > MAX_BAGS:
            raise ValueError(f"accumulators take at most 2^16 = {MAX_BAGS} bags in all, got {self.bags} + {n_bags}")
        self.bags += n_bags
        self.head.claim(n_bags)

    def host(self) -> dict:
        """One copy -> :func:`split_words`'s dict."""
        return split_words(self.buf.cpu().numpy(), self.L, self.c, self.dim)


def split_words(buf: np.ndarray, L: int, c: int, d: int) -> dict:
    """The buffer of a :class:`MilSums` -> ``dict(gV, gbv, gw, skipped_rows, skipped_bags, head)``, ``head`` the probe's ``split_words`` dict."""
    ld = L * d
    return dict(gV=buf[:ld].reshape(L, d), gbv=buf[ld:ld + L], gw=buf[ld + L:ld + 2 * L], skipped_rows=int(buf[ld + 2 * L]),
                skipped_bags=int(buf[ld + 2 * L + 1]), head=_probe.split_words(buf[ld + 2 * L + 2:], c, d))


def join_words(words: dict) -> np.ndarray:
    """The inverse of :func:`split_words`: the int64 buffer of the words."""
    h = words["head"]
    return np.concatenate([np.asarray(words["gV"], np.int64).ravel(), np.asarray(words["gbv"], np.int64), np.asarray(words["gw"], np.int64),
                           np.array([words["skipped_rows"], words["skipped_bags"]], np.int64), np.asarray(h["grad"], np.int64).ravel(),
                           np.asarray(h["gbias"], np.int64), np.array([h["loss"]], np.int64), np.asarray(h["counts"], np.int64),
                           np.array([h["skipped"]], np.int64)])


@dataclass
class AttentionMIL:
    """A fitted model: ``V`` fp32 ``[L, D]``, ``bv`` / ``w`` fp32 ``[L]``, ``Wc`` fp32 ``[C, D]``, ``bc`` fp32 ``[C]`` (the point the last evaluation
    was made at), ``l2``, ``class_weight`` fp32 ``[C]`` in (0, 1] (numpy), ``classes`` (names or None), ``lr`` / ``n_steps`` / ``seed`` (the Adam
    run), ``loss_history`` (the objective at every evaluated point, ``n_steps + 1`` of them), ``loss`` (the last), ``grad_norm`` (the largest
    magnitude of the final gradient), ``counts`` int64 ``[C]`` (the kept labelled bags of each class), ``skipped_rows`` / ``skipped_bags``."""
    V: torch.Tensor
    bv: torch.Tensor
    w: torch.Tensor
    Wc: torch.Tensor
    bc: torch.Tensor
    l2: float
    class_weight: np.ndarray
    classes: Optional[Sequence[str]]
    lr: float
    n_steps: int
    seed: int
    loss_history: List[float] = field(default_factory=list)
    loss: float = float("nan")
    grad_norm: float = float("nan")
    counts: Optional[torch.Tensor] = None
    skipped_rows: int = 0
    skipped_bags: int = 0

    @property
    def params(self):
        return (self.V, self.bv, self.w, self.Wc, self.bc)

    @property
    def n_classes(self) -> int:
        return int(self.Wc.shape[0])

    @property
    def hidden(self) -> int:
        return int(self.V.shape[0])


# ------------------------------------------------------------------------------------------------ host restatements
def _bag_of_rows(offsets: np.ndarray) -> np.ndarray:
    return np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))


def forward_numpy(x: np.ndarray, offsets, params) -> dict:
    """The forward restated in float64 -> ``dict(h [N, L], s [N] (-inf for a skipped row), a [N], z [S, D], logits [S, C], probs [S, C], labels
    int32 [S], kept_rows int64 [S], skipped_rows, skipped_bags)``.  ``params`` of any float type are used as float64.  A skipped bag has
    a zero pooled row, a zero row of probabilities and label -1."""
    n, d = check_features(x)
    o = check_offsets(offsets, n)
    V, bv, w, Wc, bc = (np.asarray(_probe._host(a), np.float64) for a in params)
    S = len(o) - 1
    skip = skipped_numpy(x)
    x64 = np.where(skip[:, None], 0.0, x.astype(np.float64))
    h = np.tanh(x64 @ V.T + bv)
    s = np.where(skip, -np.inf, h @ w)
    bag = _bag_of_rows(o)
    m = np.full(S, -np.inf)
    np.maximum.at(m, bag, s)
    kept_bag = m > -np.inf
    e = np.where(skip, 0.0, np.exp(s - np.where(kept_bag, m, 0.0)[bag]))
    Z = np.zeros(S)
    np.add.at(Z, bag, e)
    a = e / np.where(kept_bag, Z, 1.0)[bag]
    z = np.zeros((S, d))
    np.add.at(z, bag, a[:, None] * x64)
    logits = z @ Wc.T + bc
    p = np.exp(logits - logits.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    labels = logits.argmax(axis=1).astype(np.int32)
    p[~kept_bag], labels[~kept_bag] = 0.0, -1
    kept_rows = np.bincount(bag[~skip], minlength=S).astype(np.int64)
    return dict(h=h, s=s, a=a, z=z, logits=logits, probs=p, labels=labels, kept_rows=kept_rows, skipped_rows=int(skip.sum()),
                skipped_bags=int((~kept_bag).sum()))


def residuals_numpy(x: np.ndarray, offsets, labels: np.ndarray, params, class_weight=None, fwd: Optional[dict] = None) -> dict:
    """The unnormalised sums of the backward in float64 (what the device's words hold before ``1 / S_w`` and the penalty) ->
    ``dict(gV [L, D], gbv [L], gw [L], gWc [C, D], gbc [C], loss, counts int64 [C], r [S, C], dz [S, D], u [S], ds [N], R [N, L])``."""
    n, d = check_features(x)
    o = check_offsets(offsets, n)
    V, bv, w, Wc, bc = (np.asarray(_probe._host(a), np.float64) for a in params)
    c, S = Wc.shape[0], len(o) - 1
    _probe.check_labels(labels, S)
    _probe.check_label_values(labels, c)
    f = forward_numpy(x, o, params) if fwd is None else fwd
    cw = np.ones(c) if class_weight is None else np.asarray(class_weight, np.float64)
    kept = (f["kept_rows"] > 0) & (labels >= 0)
    yk = np.where(kept, labels, 0)
    wy = np.where(kept, cw[yk], 0.0)
    lg = f["logits"]
    mx = lg.max(axis=1)
    lse = mx + np.log(np.exp(lg - mx[:, None]).sum(axis=1))
    loss = float((wy * (lse - lg[np.arange(S), yk])).sum())
    pk = np.exp(lg - lse[:, None])
    r = pk.copy()
    r[np.arange(S), yk] -= 1.0
    r *= wy[:, None]
    skip = skipped_numpy(x)
    x64 = np.where(skip[:, None], 0.0, x.astype(np.float64))
    bag = _bag_of_rows(o)
    dz = r @ Wc
    u = (dz * f["z"]).sum(axis=1)
    da = (dz[bag] * x64).sum(axis=1)
    ds = f["a"] * (da - u[bag])
    R = ds[:, None] * w[None, :] * (1.0 - f["h"] ** 2)
    R[skip] = 0.0
    return dict(gV=R.T @ x64, gbv=R.sum(axis=0), gw=(ds[:, None] * np.where(skip[:, None], 0.0, f["h"])).sum(axis=0), gWc=r.T @ f["z"],
                gbc=r.sum(axis=0), loss=loss, counts=np.bincount(labels[kept], minlength=c).astype(np.int64), r=r, dz=dz, u=u, ds=ds, R=R)


def objective_numpy(x: np.ndarray, offsets, labels: np.ndarray, params, l2: float = 0.0, class_weight=None):
    """The objective and its analytic gradient in float64 -> ``(F, (dV, dbv, dw, dWc, dbc))``."""
    res = residuals_numpy(x, offsets, labels, params, class_weight)
    V, bv, w, Wc, bc = (np.asarray(_probe._host(a), np.float64) for a in params)
    cw = np.ones(Wc.shape[0]) if class_weight is None else np.asarray(class_weight, np.float64)
    S = float((cw * res["counts"]).sum())
    if not S > 0:
        raise ValueError("no labelled bag is kept: the objective is undefined")
    f = res["loss"] / S + 0.5 * l2 * float((V * V).sum() + (w * w).sum() + (Wc * Wc).sum())
    return f, (res["gV"] / S + l2 * V, res["gbv"] / S, res["gw"] / S + l2 * w, res["gWc"] / S + l2 * Wc, res["gbc"] / S)


def objective_from_words(words: dict, class_weight: np.ndarray, params, l2: float):
    """The objective and its gradient from the integer sums of one evaluation -> ``(F, (dV, dbv, dw, dWc, dbc))`` in float64: the words
    scaled by their fixed point and ``1 / S_w`` plus the penalty at ``params`` (float64)."""
    V, bv, w, Wc, bc = (np.asarray(a, np.float64) for a in params)
    f, gWc, gbc = _probe.objective_from_words(words["head"], class_weight, Wc, bc, l2)
    S = float((np.asarray(class_weight, np.float64) * words["head"]["counts"]).sum())
    f += 0.5 * l2 * float((V * V).sum() + (w * w).sum())
    k = 1.0 / GRAD_ONE / S
    return f, (words["gV"].astype(np.float64) * k + l2 * V, words["gbv"].astype(np.float64) * k, words["gw"].astype(np.float64) * k + l2 * w,
               gWc, gbc)


def synthetic_cohort(seed: int = 0, n_bags: int = 64, dim: int = 64, min_tiles: int = 16, max_tiles: int = 128, strength: float = 0.9):
    """A seeded two-class cohort for tests and examples -> ``(x fp32 [N, dim] unit rows, offsets int64 [n_bags + 1], labels int32 [n_bags],
    key bool [N])``.  Every tile is a random unit row; a positive bag (every second one) also holds 1-3 *key* tiles, unit rows near one
    fixed direction (``strength`` of it plus noise).  Negative bags hold none.  The direction depends on ``dim`` alone, so cohorts of
    different seeds share it: one is the training set, another the held-out one."""
    rng = np.random.default_rng(seed)
    direction = np.random.default_rng(0x4B454550).standard_normal(dim)
    direction /= np.linalg.norm(direction)
    sizes_ = rng.integers(min_tiles, max_tiles + 1, n_bags)
    offsets = np.concatenate([[0], np.cumsum(sizes_)]).astype(np.int64)
    labels = (np.arange(n_bags) % 2).astype(np.int32)
    x = rng.standard_normal((int(offsets[-1]), dim))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    key = np.zeros(int(offsets[-1]), bool)
    for b in np.flatnonzero(labels == 1):
        rows = offsets[b] + rng.choice(sizes_[b], int(rng.integers(1, 4)), replace=False)
        key[rows] = True
    x[key] = strength * direction + (1.0 - strength ** 2) ** 0.5 * x[key]
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32), offsets, labels, key


def key_share(attention: np.ndarray, offsets: np.ndarray, labels: np.ndarray, key: np.ndarray) -> float:
    """The share of the positive bags (label 1) whose most-attended tile is a key tile."""
    pos = [b for b in range(len(labels)) if labels[b] == 1 and offsets[b + 1] > offsets[b]]
    hit = sum(bool(key[offsets[b] + int(np.argmax(attention[offsets[b]:offsets[b + 1]]))]) for b in pos)
    return hit / max(len(pos), 1)


# ------------------------------------------------------------------------------------------------ optimiser
@dataclass
class AdamResult:
    theta: np.ndarray
    f: float
    g: np.ndarray
    history: List[float]
    n_steps: int


def adam(fun: Callable, theta0: np.ndarray, lr: float = 0.01, n_steps: int = 300, beta1: float = 0.9, beta2: float = 0.999,
         eps: float = 1e-8) -> AdamResult:
    """Full-batch Adam (Kingma and Ba 2015) for ``fun: theta -> (f, g)`` in numpy float64: ``n_steps`` updates and ``n_steps + 1``
    evaluations, the last one at the returned point.  No random numbers and no decision on a loss difference: the same evaluations give
    the same bits."""
    theta = np.array(theta0, np.float64)
    m, v = np.zeros_like(theta), np.zeros_like(theta)
    f, g = fun(theta)
    history = [float(f)]
    for t in range(1, n_steps + 1):
        m = beta1 * m + (1.0 - beta1) * g
        v = beta2 * v + (1.0 - beta2) * g * g
        theta = theta - lr * (m / (1.0 - beta1 ** t)) / (np.sqrt(v / (1.0 - beta2 ** t)) + eps)
        f, g = fun(theta)
        history.append(float(f))
    return AdamResult(theta, float(f), g, history, n_steps)


def fit_numpy(x: np.ndarray, offsets, labels: np.ndarray, n_classes: int, hidden: int = 64, l2: float = 1e-4, class_weight=None,
              lr: float = 0.01, n_steps: int = 300, seed: int = 0) -> Tuple[tuple, AdamResult]:
    """The fit restated on the host in float64 -> ``((V, bv, w, Wc, bc), AdamResult)``: what ``KEEPModel.mil_fit`` does with the device's
    evaluations replaced by :func:`objective_numpy`.  ``class_weight``: ``[C]`` as given (None: all 1)."""
    n, d = check_features(x)
    L, c = check_hidden(hidden), _probe.check_n_classes(n_classes)

    def fun(theta):
        f, g = objective_numpy(x, offsets, labels, unpack(theta, L, c, d), l2, class_weight)
        return f, pack(g)
    res = adam(fun, pack(init_params(seed, L, c, d)), lr, n_steps)
    return unpack(res.theta, L, c, d), res
