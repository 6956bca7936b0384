"""Exact t-SNE of tile features: the argument checks, the ``TileEmbedding`` result, the graph and state the device
methods pass around, and the float64 restatements the kernels are held to (tests/test_tsne.py holds those to scikit-learn).

The device side is ``KEEPModel.tsne_affinities`` / ``tsne_graph`` / ``tsne_repulsion`` / ``tsne_step`` / ``tsne_gradient`` / ``tsne_fit``
(``keep_amd.slide``) and ``wsi.tsne_map`` / ``wsi.tsne_scatter``; this file has no device code.  What both sides share:

* a neighbour's distance is ``d = max(0, 2 - 2 s)`` of its cosine s (the squared Euclidean distance of unit rows), shifted by the row's
  minimum; ``p_{j|i} ~ exp(-beta_i d_j)`` with beta_i found by bisection so that the row's entropy is ``log(perplexity)``;
* the joint graph: every directed edge ``(i, j, p_{j|i})`` and its mirror ``(j, i, p_{j|i})`` weighted ``1 / (2 N')``, sorted by the key
  ``row << 32 | col``, equal keys merged by one addition, as a CSR whose column order is the key order;
* with ``w_ij = 1 / (1 + |y_i - y_j|^2)``: ``Z = sum_{i != j} w_ij``, ``A_i = sum_j P_ij w_ij (y_i - y_j)``, ``R_i = sum_j w_ij^2 (y_i -
  y_j)``, the gradient ``4 (exaggeration A_i - R_i / Z)`` and ``KL = sum P_ij log(P_ij Z / w_ij)`` (always of the plain P);
* the update of van der Maaten's implementation as scikit-learn's ``_gradient_descent`` has it: the gain is ``+ 0.2`` where the gradient
  and the last update differ in sign and ``x 0.8`` otherwise, floored at 0.01; ``u = momentum u - lr gain g``; ``y += u``; update and
  gains start again from 0 and 1 when the exaggeration ends;
* the fixed points of the device's sums: ``Z_ONE`` (every row's Z_i is rounded to 2^-22 before the integer add), ``KL_ONE``, ``G2_ONE``.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np
import torch

from . import bootstrap as _boot

SEGMENT = 2048                     # KEEP_TSNE_SEGMENT of include/keep_hip.h: columns per partial sum of the repulsion
MAX_ROWS = 1 << 20
MAX_K = 64
MAX_EXAGGERATION = 32.0
Z_ONE = 1 << 22
KL_ONE = 1 << 40
G2_ONE = 1 << 50
MIN_GAIN = 0.01
STOP_REASONS = ("n_iter", "min_grad_norm", "no_progress")


# ------------------------------------------------------------------------------------------------ argument checks
def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_perplexity(perplexity, n_neighbors=None) -> Tuple[float, int]:
    """-> (perplexity, k): ``2 <= perplexity``; without ``n_neighbors`` k is ``ceil(3 perplexity)``, which must not exceed 64; with it
    ``perplexity <= n_neighbors / 2`` and ``2 <= n_neighbors <= 64``."""
    try:
        p = float(perplexity)
    except (TypeError, ValueError):
        raise ValueError(f"perplexity must be a number, got {perplexity!r}") from None
    if isinstance(perplexity, bool) or not np.isfinite(p) or p < 2.0:
        raise ValueError(f"perplexity must be finite and >= 2, got {perplexity!r}")
    if n_neighbors is None:
        if 3.0 * p > MAX_K:
            raise ValueError(f"3 x perplexity = {3.0 * p:g} neighbours exceed the {MAX_K} a neighbour list holds: perplexity <= {MAX_K / 3:.4g}, "
                             f"or give n_neighbors (perplexity <= n_neighbors / 2)")
        return p, int(np.ceil(3.0 * p))
    if not _is_int(n_neighbors) or not 2 <= int(n_neighbors) <= MAX_K:
        raise ValueError(f"n_neighbors must be an integer in 2..{MAX_K}, got {n_neighbors!r}")
    if p > int(n_neighbors) / 2:
        raise ValueError(f"perplexity {p:g} needs more than n_neighbors = {int(n_neighbors)} (perplexity <= n_neighbors / 2)")
    return p, int(n_neighbors)


def check_iterations(n_iter, exaggeration_iter, check_every, n_iter_without_progress) -> Tuple[int, int, int, int]:
    for name, v, lo in (("n_iter", n_iter, 1), ("exaggeration_iter", exaggeration_iter, 0), ("check_every", check_every, 1),
                        ("n_iter_without_progress", n_iter_without_progress, 1)):
        if not _is_int(v) or int(v) < lo or int(v) > 1 << 20:
            raise ValueError(f"{name} must be an integer in {lo}..2^20, got {v!r}")
    if int(exaggeration_iter) > int(n_iter):
        raise ValueError(f"exaggeration_iter = {exaggeration_iter} exceeds n_iter = {n_iter}")
    return int(n_iter), int(exaggeration_iter), int(check_every), int(n_iter_without_progress)


def check_exaggeration(e, name: str = "exaggeration") -> float:
    try:
        v = float(e)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number, got {e!r}") from None
    if not 1.0 <= v <= MAX_EXAGGERATION:
        raise ValueError(f"{name} must be in [1, {MAX_EXAGGERATION:g}] (the squared gradient norm's fixed point), got {e!r}")
    return v


def check_rows(n, what: str = "tiles") -> int:
    if int(n) < 3 or int(n) > MAX_ROWS:
        raise ValueError(f"t-SNE takes 3..2^20 {what}, got {int(n)}")
    return int(n)


def check_learning_rate(learning_rate, n: int, early_exaggeration: float) -> float:
    """``"auto"`` -> ``max(n / early_exaggeration / 4, 50)`` (Belkina et al. 2019, scikit-learn's default)."""
    if isinstance(learning_rate, str):
        if learning_rate != "auto":
            raise ValueError(f'learning_rate must be "auto" or a positive number, got {learning_rate!r}')
        return max(n / early_exaggeration / 4.0, 50.0)
    try:
        v = float(learning_rate)
    except (TypeError, ValueError):
        raise ValueError(f'learning_rate must be "auto" or a positive number, got {learning_rate!r}') from None
    if not (np.isfinite(v) and v > 0):
        raise ValueError(f'learning_rate must be "auto" or a positive number, got {learning_rate!r}')
    return v


def check_min_grad_norm(v) -> float:
    f = float(v)
    if not (np.isfinite(f) and f >= 0):
        raise ValueError(f"min_grad_norm must be finite and >= 0, got {v!r}")
    return f


def check_init(init, n: int):
    """``"pca"`` / ``"random"`` -> the string; an fp32 ``[n, 2]`` array (numpy or torch) -> a finite fp32 numpy copy."""
    if isinstance(init, str):
        if init not in ("pca", "random"):
            raise ValueError(f'init must be "pca", "random" or an fp32 [N, 2] array, got {init!r}')
        return init
    a = init.detach().cpu().numpy() if isinstance(init, torch.Tensor) else np.asarray(init)
    if a.shape != (n, 2):
        raise ValueError(f"init must be [{n}, 2] beside {n} tiles, got shape {a.shape}")
    if a.dtype != np.float32:
        raise ValueError(f"init must be float32, got {a.dtype}")
    return np.array(a, dtype=np.float32, order="C", copy=True)


def check_embedding(y, n: Optional[int] = None) -> int:
    shape = tuple(y.shape)
    if len(shape) != 2 or shape[1] != 2 or (n is not None and shape[0] != n):
        raise ValueError(f"the embedding must be [{'N' if n is None else n}, 2], got shape {shape}")
    if y.dtype not in (torch.float32, np.float32, np.dtype("float32")):
        raise ValueError(f"the embedding must be float32, got {y.dtype}")
    if shape[0] < 1 or shape[0] > MAX_ROWS:
        raise ValueError(f"the embedding must have 1..2^20 rows, got {shape[0]}")
    return int(shape[0])


def n_segments(n: int, segment: int = SEGMENT) -> int:
    return (int(n) + segment - 1) // segment


# ------------------------------------------------------------------------------------------------ what the device methods pass around
@dataclass
class TsneGraph:
    """The joint probabilities as a CSR over the kept tiles: ``row_ptr`` int32 ``[n + 1]``, ``col`` int32 ``[nnz]`` ascending within a
    row, ``val`` ``[nnz]`` (fp32 on the device, float64 from ``joint_numpy``); numpy or torch."""
    row_ptr: object
    col: object
    val: object
    n: int

    @property
    def nnz(self) -> int:
        return int(self.col.shape[0])

    def numpy(self) -> "TsneGraph":
        f = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        return TsneGraph(f(self.row_ptr), f(self.col), f(self.val), self.n)

    def keys(self) -> np.ndarray:
        """int64 ``[nnz]``: ``row << 32 | col`` in stored order."""
        g = self.numpy()
        rows = np.repeat(np.arange(g.n, dtype=np.int64), np.diff(g.row_ptr.astype(np.int64)))
        return (rows << 32) | g.col.astype(np.int64)

    def dense(self) -> np.ndarray:
        """float64 ``[n, n]``."""
        g = self.numpy()
        k = g.keys()
        P = np.zeros((g.n, g.n))
        P[k >> 32, k & 0xFFFFFFFF] = g.val.astype(np.float64)
        return P


class TsneState:
    """What an iteration reads and writes, on one device: ``y`` fp32 ``[n, 2]`` (the embedding), ``update`` (0 at first), ``gains`` (1 at
    first), ``grad`` (the last gradient) and the scratch of the kernels: ``partials`` fp32 ``[n_seg, n, 4]``, ``rz`` fp32 ``[n, 4]`` and
    ``spare`` (the embedding a step writes; it becomes ``y``).  Every word of the scratch is written before it is read."""

    def __init__(self, y: torch.Tensor, segment: int = SEGMENT):
        n = check_embedding(y)
        self.n = n
        self.y = y.detach().clone().contiguous()
        dev = self.y.device
        self.spare = torch.empty_like(self.y)
        self.update = torch.zeros_like(self.y)
        self.gains = torch.ones_like(self.y)
        self.grad = torch.empty_like(self.y)
        self.partials = torch.empty((n_segments(n, segment), n, 4), dtype=torch.float32, device=dev)
        self.rz = torch.empty((n, 4), dtype=torch.float32, device=dev)

    def restart(self) -> None:
        """Update 0 and gains 1: what the end of the exaggeration does."""
        self.update.zero_()
        self.gains.fill_(1.0)


@dataclass
class TileEmbedding:
    """The result of ``KEEPModel.tsne_fit``.  ``embedding``: fp32 ``[N, 2]`` on the device, a NaN row where the skip rule left a tile out;
    ``kept``: bool ``[N]`` on the device; ``kl_iter`` / ``kl_trace``: the iterations (0-based) at which the host read the divergence and
    its values there (of the embedding BEFORE that iteration's update, always of the plain P); ``kl``: the divergence of the returned
    embedding; ``n_iter``: iterations made; ``stop_reason``: one of ``STOP_REASONS``; then the parameters used."""
    embedding: torch.Tensor
    kept: torch.Tensor
    kl_iter: np.ndarray
    kl_trace: np.ndarray
    kl: float
    n_iter: int
    stop_reason: str
    perplexity: float
    n_neighbors: int
    learning_rate: float
    early_exaggeration: float
    exaggeration_iter: int
    init: str
    seed: int
    n_kept: int
    graph: Optional[TsneGraph] = field(default=None, repr=False, compare=False)


# ------------------------------------------------------------------------------------------------ restatements, float64
def distances_numpy(score, count, index=None) -> Tuple[np.ndarray, np.ndarray]:
    """-> (d float64 ``[N, k]``, filled bool ``[N, k]``): ``max(0, 2 - 2 s)`` in fp32 as the device forms it, minus the row's minimum over
    the filled slots (slot j is filled iff ``j < count`` and ``index >= 0``); 0 in an empty slot."""
    s = np.asarray(score, np.float32)
    n, k = s.shape
    on = np.arange(k)[None, :] < np.clip(np.asarray(count).astype(np.int64), 0, k)[:, None]
    if index is not None:
        on &= np.asarray(index) >= 0
    d = np.maximum(np.float32(0), np.float32(2) - np.float32(2) * s)
    dmin = np.where(on, d, np.float32(np.inf)).min(axis=1, initial=np.float32(np.inf))
    d = np.where(on, d - np.where(np.isfinite(dmin), dmin, 0)[:, None].astype(np.float32), np.float32(0))
    return d.astype(np.float64), on


def entropy_numpy(d, on, beta) -> Tuple[np.ndarray, np.ndarray]:
    """-> (H ``[N]``, p ``[N, k]``) of ``p ~ exp(-beta d)`` over the filled slots, float64."""
    P = np.where(on, np.exp(-d * beta[:, None]), 0.0)
    sumP = np.maximum(P.sum(axis=1), 1e-300)
    H = np.log(sumP) + beta * (d * P).sum(axis=1) / sumP
    return H, P / sumP[:, None]


def conditional_numpy(score, count, perplexity, index=None, steps: int = 200, return_beta: bool = False):
    """``keep_tsne_affinities`` restated in float64 -> p float64 ``[N, k]``: the same search (beta from 1, doubled or halved until the
    root is bracketed, then the midpoint) run for ``steps`` steps, so that it ends at the float64 root.  A row with fewer than two filled
    slots is zero.  ``return_beta``: -> ``(p, beta float64 [N])``."""
    d, on = distances_numpy(score, count, index)
    n = d.shape[0]
    target = np.log(float(perplexity))
    beta, lo, hi = np.ones(n), np.full(n, -np.inf), np.full(n, np.inf)
    with np.errstate(over="ignore", invalid="ignore"):
        for _ in range(steps):
            H, _ = entropy_numpy(d, on, beta)
            up = H > target
            lo, hi = np.where(up, beta, lo), np.where(up, hi, beta)
            beta = np.where(up, np.where(np.isinf(hi), beta * 2.0, (beta + hi) * 0.5), np.where(np.isinf(lo), beta * 0.5, (beta + lo) * 0.5))
            beta = np.minimum(beta, 1e300)
        _, p = entropy_numpy(d, on, beta)
    p = np.where((on.sum(axis=1) >= 2)[:, None], p, 0.0)
    return (p, beta) if return_beta else p


def perplexity_numpy(p) -> np.ndarray:
    """The perplexity ``exp(-sum p log p)`` of every row of a float array, float64 (an all-zero row gives 1)."""
    p = np.asarray(p, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.exp(-np.where(p > 0, p * np.log(p), 0.0).sum(axis=1))


def joint_numpy(index, p, kept=None) -> TsneGraph:
    """The joint graph restated in float64 -> ``TsneGraph`` (numpy, ``val`` float64).  ``index`` int64 ``[N, k]`` (-1: empty), ``p`` ``[N,
    k]``; ``kept`` bool ``[N]`` (default: the rows with a positive p): the N' kept rows are renumbered 0..N'-1 in order and edges to or
    from another row are dropped.  Slots with ``p = 0`` are no edges."""
    index, p = np.asarray(index, np.int64), np.asarray(p, np.float64)
    n = index.shape[0]
    kept = (p > 0).any(axis=1) if kept is None else np.asarray(kept, bool)
    new = np.cumsum(kept) - 1
    m = int(kept.sum())
    i = np.broadcast_to(np.arange(n)[:, None], index.shape)
    ok = (index >= 0) & (p > 0) & kept[:, None] & kept[np.clip(index, 0, n - 1)]
    r, c, v = new[i[ok]], new[index[ok]], p[ok] / (2.0 * m)
    keys = np.concatenate([(r << 32) | c, (c << 32) | r])
    uniq, inv = np.unique(keys, return_inverse=True)
    val = np.zeros(uniq.size)
    np.add.at(val, inv, np.concatenate([v, v]))
    row_ptr = np.zeros(m + 1, np.int64)
    np.add.at(row_ptr, (uniq >> 32) + 1, 1)
    return TsneGraph(np.cumsum(row_ptr).astype(np.int32), (uniq & 0xFFFFFFFF).astype(np.int32), val, m)


def _dense(P) -> np.ndarray:
    return P.dense() if isinstance(P, TsneGraph) else np.asarray(P, np.float64)


def gradient_numpy(y, P, exaggeration: float = 1.0) -> Tuple[float, np.ndarray, float]:
    """One evaluation in float64 -> ``(KL, gradient [N, 2], Z)``.  ``P``: a ``TsneGraph`` or a dense ``[N, N]`` array; the divergence is
    that of P itself, the gradient ``4 (exaggeration A - R / Z)``."""
    y, P = np.asarray(y, np.float64), _dense(P)
    d = y[:, None, :] - y[None, :, :]
    w = 1.0 / (1.0 + (d * d).sum(axis=2))
    np.fill_diagonal(w, 0.0)
    Z = float(w.sum())
    A = ((P * w)[:, :, None] * d).sum(axis=1)
    R = ((w * w)[:, :, None] * d).sum(axis=1)
    on = P > 0
    kl = float((P[on] * np.log(P[on] * Z / w[on])).sum())
    return kl, 4.0 * (exaggeration * A - R / Z), Z


def step_numpy(y, update, gains, grad, momentum: float, learning_rate: float):
    """The update in float64 -> ``(y, update, gains)``, new arrays."""
    y, update, gains, grad = (np.asarray(a, np.float64) for a in (y, update, gains, grad))
    gains = np.maximum(np.where(update * grad < 0.0, gains + 0.2, gains * 0.8), MIN_GAIN)
    update = momentum * update - learning_rate * (gains * grad)
    return y + update, update, gains


class Progress:
    """The stop rule both fits share: at a check after the exaggeration, ``"no_progress"`` once the divergence has not improved for more
    than ``n_iter_without_progress`` iterations, ``"min_grad_norm"`` once the gradient's norm is at most ``min_grad_norm``."""

    def __init__(self, exaggeration_iter: int, n_iter_without_progress: int, min_grad_norm: float):
        self.first, self.patience, self.min_grad_norm = exaggeration_iter, n_iter_without_progress, min_grad_norm
        self.best, self.best_iter = np.inf, exaggeration_iter
        self.iters, self.kls = [], []

    def check(self, it: int, kl: float, grad_norm: float) -> Optional[str]:
        self.iters.append(it)
        self.kls.append(kl)
        if it < self.first:
            return None
        if kl < self.best:
            self.best, self.best_iter = kl, it
        elif it - self.best_iter > self.patience:
            return "no_progress"
        return "min_grad_norm" if grad_norm <= self.min_grad_norm else None


def phase(it: int, exaggeration_iter: int, early_exaggeration: float) -> Tuple[float, float]:
    """-> (exaggeration, momentum) of iteration ``it``."""
    return (early_exaggeration, 0.5) if it < exaggeration_iter else (1.0, 0.8)


def fit_numpy(P, y0, n_iter: int = 1000, early_exaggeration: float = 12.0, exaggeration_iter: int = 250, learning_rate="auto",
              min_grad_norm: float = 1e-7, n_iter_without_progress: int = 300, check_every: int = 50, dtype=np.float64):
    """The descent of ``KEEPModel.tsne_fit`` restated -> ``(y [N, 2], kl_iter, kl_trace, kl, n_iter, stop_reason)``.  ``dtype=np.float32``
    rounds y, update and gains to fp32 after every step (the evaluation stays float64): the twin that shows how far two roundings of
    one chaotic descent separate."""
    P = _dense(P)
    n = P.shape[0]
    lr = check_learning_rate(learning_rate, n, early_exaggeration)
    y = np.asarray(y0, dtype)
    update, gains = np.zeros_like(y), np.ones_like(y)
    prog = Progress(exaggeration_iter, n_iter_without_progress, min_grad_norm)
    reason, done = "n_iter", n_iter
    for it in range(n_iter):
        ex, mom = phase(it, exaggeration_iter, early_exaggeration)
        if it == exaggeration_iter:
            update, gains = np.zeros_like(y), np.ones_like(y)
        kl, g, _ = gradient_numpy(y, P, ex)
        y, update, gains = (a.astype(dtype) for a in step_numpy(y, update, gains, g.astype(dtype), mom, lr))
        if (it + 1) % check_every == 0:
            stop = prog.check(it, kl, float(np.sqrt((g * g).sum())))
            if stop is not None:
                reason, done = stop, it + 1
                break
    kl = gradient_numpy(y, P)[0]
    return y, np.asarray(prog.iters, np.int64), np.asarray(prog.kls), kl, done, reason


# ------------------------------------------------------------------------------------------------ initial embeddings and test data
def random_init(n: int, seed: int) -> np.ndarray:
    """fp32 ``[n, 2]``: ``1e-4`` x standard normal by Box-Muller from the counter-based generator of ``keep_amd.bootstrap`` (streams 0
    and 1 of ``seed``; element j reads ``mix64(key(seed, t) + j G)``), the way ``mil_fit`` initialises: the same values on every host."""
    seed = _boot.check_seed(seed)

    def uniform(t: int) -> np.ndarray:
        with np.errstate(over="ignore"):
            u = _boot._mix64_np(np.uint64(_boot.key(seed, t)) + np.arange(2 * n, dtype=np.uint64) * np.uint64(_boot.G))
        return ((u >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53                    # in (0, 1)
    r, phi = np.sqrt(-2.0 * np.log(uniform(0))), 2.0 * np.pi * uniform(1)
    return (1e-4 * r * np.cos(phi)).reshape(n, 2).astype(np.float32)


def pca_init(scores) -> np.ndarray:
    """The first two PCA scores ``[n, 2]`` scaled to a standard deviation of 1e-4 in the first column (scikit-learn's rule) -> fp32."""
    s = np.asarray(scores, np.float64)
    sd = float(np.std(s[:, 0]))
    if not sd > 0:
        raise ValueError('the first principal component of the tiles has no spread: init="pca" cannot start from it (use "random")')
    return (s / sd * 1e-4).astype(np.float32)


def synthetic_blobs(n: int, dim: int, classes: int, noise: float, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """Seeded blobs for tests and examples -> ``(x fp32 [n, dim] unit rows, labels int64 [n])`` with ``label = i % classes``: a unit centre
    per class plus ``noise / sqrt(dim)`` x standard normal per element (a noise vector of length about ``noise``), made unit rows."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((classes, dim))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    labels = np.arange(n, dtype=np.int64) % classes
    x = c[labels] + noise / np.sqrt(dim) * rng.standard_normal((n, dim))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32), labels


def knn_purity(y, labels, k: int = 10) -> float:
    """The share of every point's k nearest neighbours in the embedding that carry its label, float64 on the host (N up to a few
    thousand)."""
    y, labels = np.asarray(y, np.float64), np.asarray(labels)
    d = ((y[:, None, :] - y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    nn = np.argsort(d, axis=1, kind="stable")[:, :k]
    return float((labels[nn] == labels[:, None]).mean())


def scatter_coords_numpy(y, size, point: int) -> Tuple[np.ndarray, np.ndarray]:
    """The affine map of ``wsi.tsne_scatter`` restated -> ``(coords int64 [N, 2] (x, y: a square's top-left corner), shown bool [N])``.
    With lo / hi the fp32 minimum / maximum of a column over the rows without a NaN and ``span = size - point`` pixels: ``c = floor((v -
    lo) / max(hi - lo, tiny) x span + 0.5)`` in float64; column 0 runs along the width, column 1 down the height."""
    y = np.asarray(y, np.float32)
    h, w = int(size[0]), int(size[1])
    shown = ~np.isnan(y).any(axis=1)
    out = np.zeros((y.shape[0], 2), np.int64)
    if shown.any():
        for c, span in ((0, w - point), (1, h - point)):
            v = y[shown, c].astype(np.float64)
            lo, hi = float(v.min()), float(v.max())
            out[shown, c] = np.floor((v - lo) / max(hi - lo, np.finfo(np.float32).tiny) * span + 0.5).astype(np.int64)
    return out, shown
