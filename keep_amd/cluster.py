"""Tile clustering: spherical k-means on unit feature rows, its integer accumulators, and the host restatements
the device kernels are held to.

The device side is ``KEEPModel.cluster_assign`` / ``cluster_update`` / ``cluster_seed`` / ``cluster_tiles`` / ``cluster_fit_batches``
(``keep_amd.slide``) and ``wsi.cluster_map``; this file has no device code.  The arithmetic both sides share:

* a row is *skipped* when it holds a non-finite value or an element with ``|x| > 1``: label -1, ``best = margin = 0``, in no sum;
* the label is the first maximum of the K cosines, ``margin`` the lead over the best of the others (0 when K = 1);
* the sums are integers, ``llrint(x * 2^30)`` per element, so they do not depend on the order of the rows or their split over calls;
* a centroid is its sum, scaled by 2^-30 and divided by its norm in float64, rounded once to fp32; an empty cluster keeps its row.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from .classmap import MAX_CLASSES

MAX_K = MAX_CLASSES                 # every result fits a ClassRaster
MAX_D = 1024
MAX_ROWS = 1 << 22                  # per call
MAX_TILES = 1 << 24                 # into one set of accumulators: 2^30 * 2^24 = 2^54 fits an int64
ONE = 1 << 30


# ------------------------------------------------------------------------------------------------ argument checks
def _is_f32(dtype) -> bool:
    return dtype == torch.float32 if isinstance(dtype, torch.dtype) else np.dtype(dtype) == np.float32


def check_k(k) -> int:
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError(f"the number of clusters must be an integer, got {k!r}")
    if k < 1 or k > MAX_K:
        raise ValueError(f"the number of clusters must be in 1..{MAX_K}, got {int(k)}")
    return int(k)


def check_dim(d) -> int:
    d = int(d)
    if d < 16 or d > MAX_D or d % 16:
        raise ValueError(f"the feature width must be a multiple of 16 in 16..{MAX_D}, got {d}")
    return d


def check_features(x, name: str = "features") -> Tuple[int, int]:
    """fp32 ``[N, D]``, numpy or torch, ``1 <= N <= 2^22``, D a multiple of 16 up to 1024 -> (N, D)."""
    shape = tuple(x.shape)
    if len(shape) != 2:
        raise ValueError(f"{name} must be [N, D], got shape {shape}")
    if not _is_f32(x.dtype):
        raise ValueError(f"{name} must be float32, got {x.dtype}")
    d = check_dim(shape[1])
    if shape[0] < 1 or shape[0] > MAX_ROWS:
        raise ValueError(f"{name} must have 1..2^22 rows per call, got {shape[0]}")
    return int(shape[0]), d


def check_centroids(c, dim: Optional[int] = None) -> Tuple[int, int]:
    """fp32 ``[K, D]``, ``1 <= K <= 64`` -> (K, D); with ``dim`` the width must be that of the features."""
    shape = tuple(c.shape)
    if len(shape) != 2:
        raise ValueError(f"centroids must be [K, D], got shape {shape}")
    if not _is_f32(c.dtype):
        raise ValueError(f"centroids must be float32, got {c.dtype}")
    k, d = check_k(int(shape[0])), check_dim(shape[1])
    if dim is not None and d != dim:
        raise ValueError(f"centroids have width {d}, the features {dim}")
    return k, d


def check_prev(prev, n: int) -> None:
    shape = tuple(prev.shape)
    if shape != (n,):
        raise ValueError(f"prev must hold one label per row, [{n}], got shape {shape}")
    if not (prev.dtype == torch.int32 if isinstance(prev.dtype, torch.dtype) else np.dtype(prev.dtype) == np.int32):
        raise ValueError(f"prev must be int32, got {prev.dtype}")


def check_init(init, k: int, n: int, dim: int) -> str:
    """``init``: "farthest", fp32 centroids ``[k, D]`` or integer row indices ``[k]`` -> "farthest" / "centroids" / "rows"."""
    if isinstance(init, str):
        if init != "farthest":
            raise ValueError(f'init must be "farthest", centroids [k, D] or row indices [k], got {init!r}')
        return "farthest"
    if not hasattr(init, "shape"):
        init = np.asarray(init)
    shape = tuple(init.shape)
    floating = init.dtype.is_floating_point if isinstance(init.dtype, torch.dtype) else np.dtype(init.dtype).kind == "f"
    if floating:
        if shape != (k, dim):
            raise ValueError(f"init centroids must be [{k}, {dim}], got shape {shape}")
        check_centroids(init, dim)
        return "centroids"
    if shape != (k,):
        raise ValueError(f"init row indices must be [{k}], got shape {shape}")
    idx = init.cpu().numpy() if isinstance(init, torch.Tensor) else np.asarray(init)
    if idx.dtype.kind not in "iu":
        raise ValueError(f"init row indices must be integers, got {idx.dtype}")
    if idx.min() < 0 or idx.max() >= n:
        raise ValueError(f"init row indices must lie in 0..{n - 1}, got {int(idx.min())}..{int(idx.max())}")
    return "rows"


def check_fit_args(max_iter, tol_changed) -> Tuple[int, int]:
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 0:
        raise ValueError(f"max_iter must be an integer >= 0, got {max_iter!r}")
    if isinstance(tol_changed, bool) or not isinstance(tol_changed, (int, np.integer)) or tol_changed < 0:
        raise ValueError(f"tol_changed must be an integer >= 0, got {tol_changed!r}")
    return int(max_iter), int(tol_changed)


# ------------------------------------------------------------------------------------------------ results
class ClusterSums:
    """The integer accumulators of one Lloyd iteration as one object: ``sums`` int64 ``[K, D]`` (the rows of each cluster, every element
    as ``llrint(x * 2^30)``), ``counts`` int64 ``[K]``, and the scalars ``cos_sum`` (the winning cosines, same fixed point), ``changed``
    and ``skipped`` (int64 ``[1]`` views).  All views share one buffer, so :meth:`zero_` is one fill.  ``tiles`` counts the rows added
    since the last :meth:`zero_` (at most 2^24).  Integer sums: the same however the rows are ordered or split over calls."""

    def __init__(self, k: int, dim: int, device="cpu"):
        self.k, self.dim = check_k(k), check_dim(dim)
        kd = self.k * self.dim
        self.buf = torch.zeros(kd + self.k + 3, dtype=torch.int64, device=device)
        self.sums = self.buf[:kd].view(self.k, self.dim)
        self.counts = self.buf[kd:kd + self.k]
        self.cos_sum = self.buf[kd + self.k:kd + self.k + 1]
        self.changed = self.buf[kd + self.k + 1:kd + self.k + 2]
        self.skipped = self.buf[kd + self.k + 2:kd + self.k + 3]
        self.tiles = 0

    def zero_(self) -> "ClusterSums":
        self.buf.zero_()
        self.tiles = 0
        return self

    def check(self, k: int, dim: int) -> None:
        if (self.k, self.dim) != (k, dim):
            raise ValueError(f"the accumulators are for K = {self.k}, D = {self.dim}; the call has K = {k}, D = {dim}")

    def claim(self, n: int) -> None:
        if self.tiles + n > MAX_TILES:
            raise ValueError(f"accumulators take at most 2^24 = {MAX_TILES} rows in all, got {self.tiles} + {n}")
        self.tiles += n


@dataclass
class TileClusters:
    """A clustering of N tiles: ``labels`` int32 ``[N]`` (-1 for a skipped tile), ``best`` / ``margin`` fp32 ``[N]`` (the winning cosine
    and its lead over the runner-up), ``centroids`` fp32 ``[K, D]``, ``counts`` int64 ``[K]``, ``skipped`` (tiles left out), ``empty``
    (bool ``[K]``: clusters without a tile), ``n_iter`` (assign passes of the Lloyd loop), ``changed`` (labels that moved in the last
    of them), ``mean_cosine`` (of the kept tiles to their centroids) and ``converged`` (``changed <= tol_changed`` was reached)."""
    labels: torch.Tensor
    best: torch.Tensor
    margin: torch.Tensor
    centroids: torch.Tensor
    counts: torch.Tensor
    skipped: int
    empty: torch.Tensor
    n_iter: int
    changed: int
    mean_cosine: float
    converged: bool

    @property
    def k(self) -> int:
        return int(self.centroids.shape[0])

    def kept(self) -> torch.Tensor:
        """bool ``[N]``: the tiles that got a label."""
        return self.labels >= 0


# ------------------------------------------------------------------------------------------------ host restatements
def skipped_numpy(x: np.ndarray) -> np.ndarray:
    """bool [N]: rows with a non-finite value or an element with |x| > 1."""
    with np.errstate(invalid="ignore"):
        return ~(np.abs(x) <= 1.0).all(axis=1)


def assign_numpy(x: np.ndarray, centroids: np.ndarray):
    """The assign restated with float64 scores -> (labels int32 [N], best float64 [N], margin float64 [N])."""
    n, d = check_features(x)
    k, _ = check_centroids(centroids, d)
    skip = skipped_numpy(x)
    s = np.where(skip[:, None], 0.0, x.astype(np.float64)) @ centroids.astype(np.float64).T
    labels = s.argmax(axis=1).astype(np.int32)                           # the first maximum
    best = s[np.arange(n), labels]
    if k > 1:
        rest = s.copy()
        rest[np.arange(n), labels] = -np.inf
        margin = best - rest.max(axis=1)
    else:
        margin = np.zeros(n)
    labels[skip] = -1
    best[skip] = 0.0
    margin[skip] = 0.0
    return labels, best, margin


def fixed_numpy(x: np.ndarray) -> np.ndarray:
    """llrint(x * 2^30) -> int64 (round half to even, as the device)."""
    return np.rint(np.asarray(x, dtype=np.float64) * ONE).astype(np.int64)


def accumulate_numpy(x: np.ndarray, labels: np.ndarray, best: np.ndarray, k: int, prev: Optional[np.ndarray] = None, into=None):
    """The integer sums of given labels -> (sums int64 [K,D], counts int64 [K], cos_sum, changed, skipped) with Python ints for the
    scalars; ``into`` (such a tuple) is added to.  A row with label -1 is in no sum; ``skipped`` counts the rows the skip rule names."""
    n, d = check_features(x)
    k = check_k(k)
    if labels.shape != (n,) or np.asarray(best).shape != (n,):
        raise ValueError(f"labels and best must be [{n}], got {labels.shape} and {np.asarray(best).shape}")
    sums, counts = np.zeros((k, d), np.int64), np.zeros(k, np.int64)
    kept = labels >= 0
    q = fixed_numpy(np.where(kept[:, None], x, 0.0))
    np.add.at(sums, labels[kept], q[kept])
    np.add.at(counts, labels[kept], 1)
    cos_sum = int(fixed_numpy(np.asarray(best)[kept]).sum())
    changed = 0 if prev is None else int((labels != prev).sum())
    skipped = int(skipped_numpy(x).sum())
    if into is not None:
        return into[0] + sums, into[1] + counts, into[2] + cos_sum, into[3] + changed, into[4] + skipped
    return sums, counts, cos_sum, changed, skipped


def update_numpy(sums: np.ndarray, counts: np.ndarray, centroids: np.ndarray):
    """The update restated in float64 -> (centroids fp32 [K,D], empty uint8 [K]); an empty cluster keeps its row."""
    s = sums.astype(np.float64) / ONE
    norm = np.sqrt((s * s).sum(axis=1))
    empty = (counts == 0) | ~(norm > 0.0)
    out = centroids.astype(np.float32).copy()
    out[~empty] = (s[~empty] / norm[~empty, None]).astype(np.float32)
    return out, empty.astype(np.uint8)


def seed_numpy(x: np.ndarray, k: int, gaps: Optional[list] = None) -> np.ndarray:
    """Farthest-point seeding restated in float64 -> row indices int64 [k].  The first centre is the kept row with the largest cosine
    to the normalised integer mean of the kept rows, every next one the kept row whose largest cosine to the centres so far is the
    smallest; the lowest index wins a tie.  ``gaps`` (a list) receives, per step, the distance from the chosen candidate's value to the
    next DIFFERENT value (inf without one): what a caller needs to know whether fp32 arithmetic must reproduce the choice."""
    n, d = check_features(x)
    k = check_k(k)
    skip = skipped_numpy(x)
    if skip.all():
        return np.full(k, -1, np.int64)
    x64 = np.where(skip[:, None], 0.0, x.astype(np.float64))
    labels = np.where(skip, -1, 0).astype(np.int32)
    sums, counts, *_ = accumulate_numpy(x, labels, np.zeros(n, np.float32), 1)
    mean, _ = update_numpy(sums, counts, np.zeros((1, d), np.float32))

    def pick(values, largest):
        v = np.where(skip, -np.inf if largest else np.inf, values)
        i = int(v.argmax() if largest else v.argmin())
        if gaps is not None:
            other = np.abs(v[~skip] - v[i])
            other = other[other > 0]
            gaps.append(float(other.min()) if other.size else float("inf"))
        return i

    out = [pick(x64 @ mean[0].astype(np.float64), True)]
    nearest = np.full(n, -np.inf)
    for _ in range(1, k):
        nearest = np.maximum(nearest, x64 @ x64[out[-1]])
        out.append(pick(nearest, False))
    return np.asarray(out, np.int64)


def kmeans_numpy(x: np.ndarray, k: int, init="farthest", max_iter: int = 50, tol_changed: int = 0) -> dict:
    """The Lloyd loop of ``KEEPModel.cluster_tiles`` restated: assign in float64, sums and update as above.  Returns a dict with the
    fields of :class:`TileClusters` as numpy / Python values plus ``min_margin``, the smallest float64 margin of a kept row over the
    whole trajectory (the fp32 device arithmetic follows the same trajectory when that is well above its error bound)."""
    n, d = check_features(x)
    k = check_k(k)
    max_iter, tol_changed = check_fit_args(max_iter, tol_changed)
    kind = check_init(init, k, n, d)
    if kind == "farthest":
        init = seed_numpy(x, k)
    cen = np.asarray(init, np.float32).copy() if kind == "centroids" else x[np.asarray(init, np.int64)].copy()
    prev = np.full(n, -1, np.int32)
    min_margin, n_iter, converged = np.inf, 0, False
    acc = None

    def one_pass(prev):
        nonlocal min_margin
        labels, best, margin = assign_numpy(x, cen)
        if k > 1 and (labels >= 0).any():
            min_margin = min(min_margin, float(margin[labels >= 0].min()))
        return labels, best, margin, accumulate_numpy(x, labels, best, k, prev)

    for it in range(1, max_iter + 1):
        labels, best, margin, acc = one_pass(prev)
        n_iter = it
        if acc[3] <= tol_changed:
            converged = True
            break
        cen, _ = update_numpy(acc[0], acc[1], cen)
        prev = labels
    if not converged:
        labels, best, margin, acc = one_pass(prev)
    kept = int(acc[1].sum())
    return dict(labels=labels, best=best, margin=margin, centroids=cen, counts=acc[1], skipped=acc[4], empty=acc[1] == 0, n_iter=n_iter,
                changed=acc[3], mean_cosine=(acc[2] / ONE / kept) if kept else 0.0, converged=converged, min_margin=min_margin)
