"""Feature PCA: the integer moments of unit feature rows, the principal components of their covariance, the
scores of rows on them, the three-component colour picture, and the host restatements the device kernels are held to.

The device side is ``KEEPModel.pca_moments`` / ``pca_fit`` / ``pca_fit_batches`` / ``pca_transform`` / ``render_rgb_map``
(``keep_amd.slide``) and ``wsi.pca_map``; this file has no device code.  The arithmetic both sides share:

* a row is *skipped* when it holds a non-finite value or an element with ``|x| > 1`` (``keep_amd.cluster``'s rule): it is in no sum;
* ``sum`` and ``count`` are integers, ``llrint(x * 2^30)`` per element: the same words for every order and split of the rows;
* ``gram`` is taken over chunks of ``CHUNK`` rows cut from row 0 of every call: per chunk and word the fp32 sum of products of
  ``a = fp32(x - centre)`` is rounded once to ``2^-32`` and added as an integer.  The words depend on ``CHUNK`` and on where the chunk
  boundaries fall, and on nothing else about the launch; the restatement here forms each chunk's sum in float64 instead;
* with ``mu = sum 2^-30 / n`` the covariance is ``(G 2^-32 - n (mu - c)(mu - c)^T) / (n - 1)``: the shifted-data formula, which
  cancels nothing when the centre c is the mean itself (the second pass of a two-pass fit);
* the eigen-decomposition is ``numpy.linalg.eigh`` in float64 on the host; a component's sign makes its largest element positive.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from .classmap import MAX_CLASSES
from .cluster import MAX_TILES, _is_f32, check_dim, check_features, skipped_numpy
from .heatmap import Q_ONE, render_args, unpack_numpy

CHUNK = 512                         # KEEP_PCA_CHUNK of include/keep_hip.h: rows per rounding of a Gram word
MAX_K = 64
SUM_ONE = 1 << 30
GRAM_ONE = 1 << 32
MAX_GROUPS = 64


# ------------------------------------------------------------------------------------------------ argument checks
def check_k(k, dim: Optional[int] = None) -> int:
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError(f"the number of components must be an integer, got {k!r}")
    if k < 1 or k > MAX_K:
        raise ValueError(f"the number of components must be in 1..{MAX_K}, got {int(k)}")
    if dim is not None and k > dim:
        raise ValueError(f"the number of components must not exceed the feature width {dim}, got {int(k)}")
    return int(k)


def check_centre(centre, dim: int) -> Optional[np.ndarray]:
    """``None`` or fp32 ``[D]`` with every ``|c_d| <= 1`` -> a contiguous fp32 numpy copy (or None)."""
    if centre is None:
        return None
    c = centre.detach().cpu().numpy() if isinstance(centre, torch.Tensor) else np.asarray(centre)
    if c.shape != (dim,):
        raise ValueError(f"centre must be [{dim}], got shape {c.shape}")
    if c.dtype != np.float32:
        raise ValueError(f"centre must be float32, got {c.dtype}")
    if not bool((np.abs(c) <= 1.0).all()):
        raise ValueError("centre must be finite with every element within 1 in magnitude (|x - centre| <= 2 bounds the Gram words)")
    return np.array(c, dtype=np.float32, order="C", copy=True)         # the caller's array may change or be read-only: keep our own


def check_groups(groups) -> int:
    if isinstance(groups, bool) or not isinstance(groups, (int, np.integer)) or groups < 0 or groups > MAX_GROUPS:
        raise ValueError(f"groups must be 0 (chosen by the kernel) or 1..{MAX_GROUPS} chunks per workgroup, got {groups!r}")
    return int(groups)


def check_batch_rows(rows: int, index: int, chunk: int = CHUNK) -> None:
    """A batch that another batch follows must hold a multiple of the chunk: the chunk boundaries of the concatenation then fall
    where they fall in the batches."""
    if rows % chunk:
        raise ValueError(f"batch {index} holds {rows} rows and is not the last: every batch but the last must hold a multiple of "
                         f"the chunk ({chunk} rows)")


def check_planes(planes, n_classes: int) -> Tuple[int, int, int]:
    p = tuple(int(v) for v in planes)
    if len(p) != 3 or any(v < 0 or v >= n_classes for v in p):
        raise ValueError(f"planes must be three plane indices in 0..{n_classes - 1} (red, green, blue), got {planes!r}")
    return p


def check_kept_rows(n: int) -> None:
    if n < 2:
        raise ValueError(f"a covariance needs at least two kept rows, got {int(n)}")


# ------------------------------------------------------------------------------------------------ results
class PcaSums:
    """The integer moments as one object: ``sum`` int64 ``[D]`` (``llrint(x * 2^30)`` per kept row), ``gram`` int64 ``[D, D]`` (per
    chunk ``llrint(acc * 2^32)`` of ``a = fp32(x - centre)``; only the 16 x 16 tiles with tile row <= tile column are written),
    ``count`` and ``skipped`` (int64 ``[1]`` views).  All views share one buffer, so :meth:`zero_` is one fill.  ``centre`` (fp32
    ``[D]``, every element within 1 in magnitude, or None for zero) is fixed when the object is made: every call that adds into it
    uses that centre.  ``rows`` counts the rows added since the last :meth:`zero_` (at most 2^24)."""

    def __init__(self, dim: int, centre=None, device="cpu"):
        self.dim = check_dim(dim)
        d = self.dim
        self.centre = check_centre(centre, d)
        self.centre_dev = None if self.centre is None else torch.from_numpy(self.centre).to(device)
        self.buf = torch.zeros(d + d * d + 2, dtype=torch.int64, device=device)
        self.sum = self.buf[:d]
        self.gram = self.buf[d:d + d * d].view(d, d)
        self.count = self.buf[d + d * d:d + d * d + 1]
        self.skipped = self.buf[d + d * d + 1:d + d * d + 2]
        self.rows = 0

    def zero_(self) -> "PcaSums":
        self.buf.zero_()
        self.rows = 0
        return self

    def check(self, dim: int) -> None:
        if self.dim != dim:
            raise ValueError(f"the accumulators are for D = {self.dim}; the call has D = {dim}")

    def claim(self, n: int) -> None:
        if self.rows + n > MAX_TILES:
            raise ValueError(f"accumulators take at most 2^24 = {MAX_TILES} rows in all, got {self.rows} + {n}")
        self.rows += n

    def gram_full(self) -> torch.Tensor:
        """The Gram matrix mirrored -> int64 ``[D, D]``: the words on and above the diagonal and their transposes below."""
        up = torch.triu(self.gram)
        return up + torch.triu(self.gram, 1).t()


@dataclass
class FeaturePCA:
    """A fitted PCA: ``mean`` fp32 ``[D]``, ``components`` fp32 ``[k, D]`` (unit rows, the largest element of each positive),
    ``explained_variance`` float64 ``[k]`` (the eigenvalues of the sample covariance, descending), ``explained_variance_ratio`` (their
    shares of ``total_variance``, the covariance's trace), ``n_rows`` (kept rows), ``skipped`` and ``centre`` (the fp32 centre the Gram
    was taken about, None for zero)."""
    mean: np.ndarray
    components: np.ndarray
    explained_variance: np.ndarray
    explained_variance_ratio: np.ndarray
    total_variance: float
    n_rows: int
    skipped: int
    centre: Optional[np.ndarray] = None

    @property
    def k(self) -> int:
        return int(self.components.shape[0])

    @property
    def dim(self) -> int:
        return int(self.components.shape[1])

    def bias(self, k: Optional[int] = None) -> np.ndarray:
        """fp32 ``[k]``: ``-(mean . w_j)``, the dot in float64, rounded once."""
        k = self.k if k is None else k
        return (-(self.components[:k].astype(np.float64) @ self.mean.astype(np.float64))).astype(np.float32)

    def whiten_scale(self, k: Optional[int] = None) -> np.ndarray:
        """fp32 ``[k]``: ``1 / sqrt(lambda_j)`` (an eigenvalue of 0 gives 0: that score carries nothing)."""
        k = self.k if k is None else k
        lam = self.explained_variance[:k]
        with np.errstate(divide="ignore"):
            return np.where(lam > 0, 1.0 / np.sqrt(lam), 0.0).astype(np.float32)


# ------------------------------------------------------------------------------------------------ host restatements
def covariance_from_sums(sum_words, gram_words, count, centre=None) -> Tuple[np.ndarray, np.ndarray]:
    """The sample covariance from the integer moments, in float64 -> ``(mean float64 [D], cov float64 [D, D])``.  ``gram_words``: the
    mirrored Gram (``PcaSums.gram_full``).  ``mu = sum 2^-30 / n`` and ``cov = (G 2^-32 - n (mu - c)(mu - c)^T) / (n - 1)``."""
    n = int(count)
    check_kept_rows(n)
    s = np.asarray(sum_words).astype(np.float64) / SUM_ONE
    d = s.shape[0]
    g = np.asarray(gram_words).astype(np.float64) / GRAM_ONE
    if g.shape != (d, d):
        raise ValueError(f"gram must be [{d}, {d}] beside sum [{d}], got {g.shape}")
    mu = s / n
    delta = mu - (0.0 if centre is None else np.asarray(centre, np.float64))
    cov = (g - n * np.outer(delta, delta)) / (n - 1)
    return mu, cov


def components_from_covariance(cov: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
    """``numpy.linalg.eigh`` of a symmetric float64 ``[D, D]`` -> ``(eigenvalues float64 [D] descending, below 0 clamped to 0; components
    float64 [k, D])``.  The sign of each row makes its element of largest magnitude positive (scikit-learn's rule)."""
    cov = np.asarray(cov, np.float64)
    k = check_k(k, cov.shape[0])
    lam, vec = np.linalg.eigh((cov + cov.T) * 0.5)
    lam, vec = lam[::-1], vec[:, ::-1]
    w = vec[:, :k].T.copy()
    big = np.abs(w).argmax(axis=1)
    w *= np.where(w[np.arange(k), big] < 0, -1.0, 1.0)[:, None]
    return np.maximum(lam, 0.0), w


def pca_from_sums(sum_words, gram_words, count, skipped, k: int, centre=None) -> FeaturePCA:
    """Moments -> :class:`FeaturePCA`: what the device fit and :func:`fit_numpy` both end in."""
    mu, cov = covariance_from_sums(sum_words, gram_words, count, centre)
    lam, w = components_from_covariance(cov, k)
    total = float(lam.sum())
    ev = lam[:k].copy()
    return FeaturePCA(mu.astype(np.float32), w.astype(np.float32), ev, ev / total if total > 0 else np.zeros_like(ev), total, int(count),
                      int(skipped), None if centre is None else np.asarray(centre, np.float32).copy())


def moments_numpy(x: np.ndarray, centre=None, chunk: int = CHUNK, into=None):
    """The moments restated -> ``(sum int64 [D], gram int64 [D, D] (full, symmetric), count, skipped)`` with Python ints for the
    scalars; ``into`` (such a tuple) is added to.  Each chunk's sum of products of ``a = float64(fp32(x - centre))`` is formed in
    float64 and rounded once to ``2^-32``, where the device forms it in fp32."""
    n, d = check_features(x)
    c = check_centre(centre, d)
    skip = skipped_numpy(x)
    kept = ~skip
    xs = np.where(kept[:, None], x, np.float32(0))
    s = np.rint(xs.astype(np.float64) * SUM_ONE).astype(np.int64).sum(axis=0)
    a = xs if c is None else np.where(kept[:, None], (xs - c[None, :]).astype(np.float32), np.float32(0))
    a = a.astype(np.float64)
    g = np.zeros((d, d), np.int64)
    for r0 in range(0, n, chunk):
        blk = a[r0:r0 + chunk]
        g += np.rint((blk.T @ blk) * GRAM_ONE).astype(np.int64)
    g = np.triu(g) + np.triu(g, 1).T
    out = (s, g, int(kept.sum()), int(skip.sum()))
    if into is not None:
        return into[0] + out[0], into[1] + out[1], into[2] + out[2], into[3] + out[3]
    return out


def fit_numpy(x: np.ndarray, k: int, two_pass: bool = True, chunk: int = CHUNK) -> FeaturePCA:
    """``KEEPModel.pca_fit`` restated in float64, without the fixed points (the yardstick the device fit is held to): pass 1 gives the
    mean, pass 2 the Gram about ``fp32(mean)``, every sum in float64; ``two_pass=False`` is one pass about a zero centre.  ``chunk``
    plays no part here: a float64 sum is not rounded per chunk."""
    n, d = check_features(x)
    k = check_k(k, d)
    kept = ~skipped_numpy(x)
    cnt, skp = int(kept.sum()), int((~kept).sum())
    check_kept_rows(cnt)
    x64 = x[kept].astype(np.float64)
    s = x64.sum(axis=0)
    centre = (s / cnt).astype(np.float32) if two_pass else None
    a = x64 if centre is None else x64 - centre.astype(np.float64)[None, :]
    return pca_from_sums(s * SUM_ONE, (a.T @ a) * GRAM_ONE, cnt, skp, k, centre)


def centre_from_sums(sum_words, count) -> np.ndarray:
    """fp32 ``[D]``: the integer mean rounded once, the centre of a two-pass fit's second pass (within 1 in magnitude as every row is)."""
    return (np.asarray(sum_words).astype(np.float64) / SUM_ONE / int(count)).astype(np.float32)


def project_numpy(pca: FeaturePCA, x: np.ndarray, k: Optional[int] = None, whiten: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """Scores in float64 -> ``(scores float64 [N, k], kept bool [N])``: ``(x - mean) . w_j``, divided by ``sqrt(lambda_j)`` with
    ``whiten``; a skipped row is a zero row."""
    n, d = check_features(x)
    if d != pca.dim:
        raise ValueError(f"the features have width {d}, the PCA {pca.dim}")
    k = pca.k if k is None else check_k(k, pca.k)
    kept = ~skipped_numpy(x)
    xs = np.where(kept[:, None], x, np.float32(0)).astype(np.float64)
    s = (xs - pca.mean.astype(np.float64)[None, :]) @ pca.components[:k].astype(np.float64).T
    if whiten:
        s = s * pca.whiten_scale(k).astype(np.float64)[None, :]
    s[~kept] = 0.0
    return s, kept


def synthetic_features(n: int, dim: int, seed: int = 0, rank: int = 6) -> np.ndarray:
    """Unit rows with a known spectrum -> fp32 ``[n, dim]``: a unit mean direction, plus ``rank`` orthonormal planted directions with
    standard deviations ``0.5 * 0.6^j``, plus 0.02 isotropic noise, every row renormalised."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((dim, rank + 1)))
    mean, planted = q[:, 0], q[:, 1:rank + 1]
    sd = 0.5 * 0.6 ** np.arange(rank)
    x = mean[None, :] + (rng.standard_normal((n, rank)) * sd[None, :]) @ planted.T + 0.02 * rng.standard_normal((n, dim))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


def render_rgb_numpy(acc: np.ndarray, thumbnail: Optional[np.ndarray] = None, planes=(0, 1, 2), alpha: float = 0.6,
                     mask: Optional[np.ndarray] = None, background=(255, 255, 255)) -> np.ndarray:
    """``KEEPModel.render_rgb_map`` restated in the same integers -> uint8 ``[h, w, 3]``.  ``acc``: int64 ``[C, h, w]``; channel ch of a
    pixel with count c > 0 inside ``mask`` is ``v = min(255, (2 255 S + 65535 c) // (2 65535 c))`` of plane ``planes[ch]``, blended as
    ``(a v + (256 - a) under + 128) >> 8`` with ``a = round(256 alpha)``; other pixels keep the thumbnail or the background."""
    a, _, _, _, bg = render_args(alpha, (0.0, 1.0), 0.0, background)
    acc = np.asarray(acc)
    if acc.ndim != 3 or acc.dtype != np.int64:
        raise ValueError(f"acc must be int64 [C, h, w], got {acc.dtype} {acc.shape}")
    C, h, w = acc.shape
    p = check_planes(planes, C)
    if thumbnail is None:
        under = np.empty((h, w, 3), np.int64)
        under[:] = bg
    else:
        if thumbnail.dtype != np.uint8 or thumbnail.ndim != 3 or thumbnail.shape[:2] != (h, w) or thumbnail.shape[2] not in (3, 4):
            raise ValueError(f"thumbnail must be uint8 {(h, w)} x 3|4, got {thumbnail.dtype} {thumbnail.shape}")
        under = thumbnail[..., :3].astype(np.int64)
    out = under.copy()
    for ch in range(3):
        S, c = unpack_numpy(acc[p[ch]])
        c = c.astype(np.int64)
        shown = c > 0
        if mask is not None:
            if mask.shape != (h, w):
                raise ValueError(f"mask must be {(h, w)}, got {mask.shape}")
            shown &= np.asarray(mask) != 0
        v = np.minimum((2 * 255 * S + Q_ONE * c) // (2 * Q_ONE * np.maximum(c, 1)), 255)
        out[..., ch] = np.where(shown, (a * v + (256 - a) * under[..., ch] + 128) >> 8, under[..., ch])
    return out.astype(np.uint8)
