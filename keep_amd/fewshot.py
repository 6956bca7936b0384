"""Few-shot prototypes: SimpleShot with centring and L2 normalisation (CL2N) over many random support sets.
The support sampler's contract, the result classes, the argument checks, the error bounds the tests use and the numpy restatements
the kernels are held to.  No device code lives here: ``KEEPModel.fewshot_sample`` / ``fewshot_prototypes`` / ``fewshot_classify``
(``slide.py``, kernels in ``csrc/fewshot.hip``) do the work.

The sampling, with the bootstrap's generator (``keep_amd.bootstrap``: ``mix64``, ``key``, ``G``).  The labelled training rows are grouped
by class with a stable sort (:func:`class_groups`); ``n_c`` is the size of class ``c``.  For global episode ``e`` and class ``c``::

    k   = key(seed, 64 e + c)
    r_j = (mix64(k + j G) n_c) >> 64          j = 0, 1, 2, ...

and the support of ``(e, c)`` is the first ``shots`` DISTINCT values of ``r_j`` in order of first appearance, each mapped through the class's
row list; with ``n_c <= shots`` it is the whole class in stored order.  The first K distinct values of i.i.d. uniform draws are a uniform
K-subset, and episode ``e`` is the same support set whatever the number of episodes or their split over calls.

The classifier, for one episode with kept support rows ``s_i`` of class ``y_i``: ``mu`` = their mean (0 without centring), ``z_i = (s_i -
mu) / |s_i - mu|`` (a zero row when the norm is 0), ``p_c`` = the mean of class c's ``z_i``; a test row ``x`` gets ``q = (x - mu) / |x - mu|``
and the label ``argmin_c |q - p_c|^2`` over the classes with a kept support row, the first minimum.  Since ``|q| = 1`` that is the argmax of
``s_c = q . p_c - h_c``, ``h_c = |p_c|^2 / 2``, and with ``r = |x - mu| = sqrt(1 - 2 x.mu + |mu|^2)`` of ``t_c = r s_c = (x.p_c - mu.p_c) -
h_c r``: C + 1 dot products per (row, episode) and no division."""
from __future__ import annotations

import operator
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import bootstrap as _boot

MAX_CLASSES = 63                         # an episode's C + 1 bank rows fit one tile of 64
MAX_SHOTS = 256                          # KEEP_FEWSHOT_MAX_SHOTS: per sampled episode
MAX_DRAWS = 1 << 20                      # KEEP_FEWSHOT_MAX_DRAWS
MAX_EPISODES = 1 << 16                   # per call of the C ABI
MAX_ROWS = 1 << 22
U = 2.0 ** -24                           # the unit round-off of fp32


# ------------------------------------------------------------------------------------------------ argument checks
def _index(v, name: str) -> int:
    if isinstance(v, bool):
        raise ValueError(f"{name} must be an integer, got {v!r}")
    try:
        return operator.index(v)
    except TypeError:
        raise ValueError(f"{name} must be an integer, got {v!r}") from None


def check_classes(n_classes) -> int:
    c = _index(n_classes, "n_classes")
    if not 2 <= c <= MAX_CLASSES:
        raise ValueError(f"n_classes must be in 2..{MAX_CLASSES}, got {c}")
    return c


def check_shots(shots, limit: int = MAX_SHOTS) -> int:
    k = _index(shots, "shots")
    if not 1 <= k <= limit:
        raise ValueError(f"shots must be in 1..{limit}, got {k}")
    return k


def check_episodes(n_episodes, first_episode=0) -> Tuple[int, int]:
    e, first = _index(n_episodes, "n_episodes"), _index(first_episode, "first_episode")
    if e < 1:
        raise ValueError(f"n_episodes must be >= 1, got {e}")
    if first < 0 or first + e > 1 << 40:
        raise ValueError(f"first_episode must be >= 0 with first_episode + n_episodes <= 2^40, got {first}")
    return e, first


def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def class_groups(labels, n_classes) -> Tuple[np.ndarray, np.ndarray]:
    """Integer labels ``[M]`` (a label outside ``0 .. C - 1``, such as -1, leaves its row out) -> ``(class_rows int32 [M'], class_offsets
    int64 [C + 1])``: the labelled rows grouped by class by a stable sort, so every class lists its rows in ascending order."""
    c = check_classes(n_classes)
    y = _host(labels)
    if y.ndim != 1 or y.dtype.kind not in "iu":
        raise ValueError(f"labels must be integers [M], got {y.dtype} {y.shape}")
    if len(y) > MAX_ROWS:
        raise ValueError(f"at most 2^22 rows, got {len(y)}")
    y = y.astype(np.int64)
    rows = np.nonzero((y >= 0) & (y < c))[0]
    order = np.argsort(y[rows], kind="stable")
    offsets = np.zeros(c + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(y[rows], minlength=c))
    return rows[order].astype(np.int32), offsets


# ------------------------------------------------------------------------------------------------ the result classes
@dataclass
class SupportSets:
    """``support`` int32 ``[E, C, shots]``: training rows, -1 in an unused slot; episode ``i`` is global episode ``first_episode + i`` of
    ``seed``.  ``class_rows`` / ``class_offsets`` are the grouping it was drawn from (on the host)."""
    support: torch.Tensor
    n_classes: int
    shots: int
    seed: int
    first_episode: int
    class_rows: np.ndarray
    class_offsets: np.ndarray

    @property
    def n_episodes(self) -> int:
        return int(self.support.shape[0])


@dataclass
class Prototypes:
    """``bank`` fp32 ``[E, C + 1, D]`` (``p_0 .. p_{C-1}``, then ``mu``; zero rows for invalid classes), ``consts`` fp32 ``[E, 2 C + 1]``
    (``mu.p_c``, ``h_c``, ``|mu|^2``), ``valid`` uint8 ``[E, C]``, ``support_skipped`` int64 ``[1]`` (sampled rows the skip rule dropped)."""
    bank: torch.Tensor
    consts: torch.Tensor
    valid: torch.Tensor
    support_skipped: torch.Tensor
    centre: bool = True

    @property
    def n_episodes(self) -> int:
        return int(self.bank.shape[0])

    @property
    def n_classes(self) -> int:
        return int(self.bank.shape[1]) - 1

    @property
    def dim(self) -> int:
        return int(self.bank.shape[2])

    def episodes(self, start: int, stop: int) -> "Prototypes":
        """Episodes ``start .. stop - 1`` as a ``Prototypes`` of their own (views)."""
        if not 0 <= start < stop <= self.n_episodes:
            raise ValueError(f"episodes {start}..{stop} of {self.n_episodes}")
        return Prototypes(self.bank[start:stop], self.consts[start:stop], self.valid[start:stop], self.support_skipped, self.centre)


def check_prototypes(protos, dim: Optional[int] = None) -> Tuple[int, int, int]:
    """-> (E, C, D)"""
    if not isinstance(protos, Prototypes):
        raise ValueError(f"protos must be a Prototypes, got {type(protos).__name__}")
    b, k, v = protos.bank, protos.consts, protos.valid
    if b.dim() != 3 or b.dtype != torch.float32:
        raise ValueError(f"bank must be fp32 [E, C + 1, D], got {b.dtype} {tuple(b.shape)}")
    e, c, d = int(b.shape[0]), check_classes(int(b.shape[1]) - 1), int(b.shape[2])
    if e < 1:
        raise ValueError("no episode")
    if tuple(k.shape) != (e, 2 * c + 1) or k.dtype != torch.float32:
        raise ValueError(f"consts must be fp32 [{e}, {2 * c + 1}], got {k.dtype} {tuple(k.shape)}")
    if tuple(v.shape) != (e, c) or v.dtype != torch.uint8:
        raise ValueError(f"valid must be uint8 [{e}, {c}], got {v.dtype} {tuple(v.shape)}")
    if dim is not None and d != dim:
        raise ValueError(f"the prototypes have width {d}, the features {dim}")
    return e, c, d


# ------------------------------------------------------------------------------------------------ the bounds
def dot_bound(dim: int) -> float:
    """|fp32 fma chain of D terms - exact| for two rows of norm <= 1: ``D 2^-24``, as section 28."""
    return dim * U


def r_bound(dim: int, r: float) -> float:
    """|r_device - r|: the argument of the root carries ``2 dot_bound`` and two roundings of values <= 4; a root's error is that over ``r``;
    the root itself rounds once."""
    return (2.0 * dot_bound(dim) + 8.0 * U) / r + 2.0 * U


def t_bound(dim: int, r: float) -> float:
    """|t_c,device - t_c| with ``h_c <= 1/2`` and three roundings of values <= 2."""
    return dot_bound(dim) + 0.5 * r_bound(dim, r) + 6.0 * U


def margin_bound(dim: int, r: float) -> float:
    """The float64 margin ``s_1 - s_2`` (in units of ``t / r``) above which the device's label must be the reference's: two ``t`` errors over
    ``r``."""
    return 2.0 * t_bound(dim, r) / r


def score_bound(dim: int, r: float) -> float:
    """|scores_out - s_c|, ``|s_c| <= 3/2``: the error of t over r, that of r over r, one division."""
    return (t_bound(dim, r) + 1.5 * r_bound(dim, r)) / r + 2.0 * U


def margin_out_bound(dim: int, r: float) -> float:
    return (2.0 * t_bound(dim, r) + 3.0 * r_bound(dim, r)) / r + 4.0 * U


def bank_bound(dim: int, n_support: int, n_class: int, rho: float) -> Tuple[float, float]:
    """``(|mu_d,device - mu_d|, |p_cd,device - p_cd|)`` for an episode of ``n_support`` kept rows, at most ``n_class`` per class, whose
    smallest ``|s_i - mu|`` is ``rho``: a sequential fp32 sum of n terms <= 1 is off by ``n^2 2^-24`` at most, its mean by ``(n + 1) 2^-24``;
    ``v = s - mu`` then by ``a = (n + 3) 2^-24`` per element, the norm by ``a sqrt(D) + (D / 2 + 2) 2^-24 |v|``, ``z = v / |v|`` by ``a / rho +
    a sqrt(D) / rho + (D / 2 + 3) 2^-24`` and the mean of m such rows by ``(m + 1) 2^-24`` more."""
    a = (n_support + 3) * U
    dz = a * (1.0 + np.sqrt(dim)) / rho + (dim / 2.0 + 3.0) * U
    return (n_support + 1) * U, dz + (n_class + 1) * U


def consts_bound(dim: int, dmu: float, dp: float) -> float:
    """|consts_device - consts| for ``mu.p_c``, ``h_c`` and ``|mu|^2``: the chain's ``D 2^-24`` and the rows' own errors, all norms <= 1."""
    return dim * U + 2.0 * np.sqrt(dim) * (dmu + dp)


def end_to_end_margin_bound(dim: int, r: float, dmu: float, dp: float) -> float:
    """:func:`margin_bound` when the reference builds its own prototypes in float64 instead of reading the device's: ``mu`` off by ``dmu``
    per element moves the unit row ``q`` by at most ``2 sqrt(D) dmu / r``, ``p_c`` off by ``dp`` per element moves ``q . p_c - h_c`` by at most
    ``2 sqrt(D) dp`` more; a margin is two scores."""
    return margin_bound(dim, r) + 2.0 * (2.0 * np.sqrt(dim) * dmu / r + 2.0 * np.sqrt(dim) * dp)


# ------------------------------------------------------------------------------------------------ the restatements
def _draws(k: int, j0: int, j1: int, n: int) -> np.ndarray:
    """r_j for j0 <= j < j1 in numpy uint64, as ``keep_amd.bootstrap.draws_numpy``."""
    with np.errstate(over="ignore"):
        x = _boot._mix64_np(np.uint64(k) + np.arange(j0, j1, dtype=np.uint64) * np.uint64(_boot.G))
        hi, lo, nn = x >> np.uint64(32), x & np.uint64(0xFFFFFFFF), np.uint64(n)
        return ((hi * nn + ((lo * nn) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)


def sample_numpy(class_rows, class_offsets, shots, n_episodes, seed=0, first_episode=0) -> np.ndarray:
    """keep_fewshot_sample restated on the host -> int32 ``[E, C, shots]``, unused slots -1."""
    rows, off = np.asarray(class_rows, np.int64), np.asarray(class_offsets, np.int64)
    c = check_classes(len(off) - 1)
    k = check_shots(shots)
    e_n, first = check_episodes(n_episodes, first_episode)
    seed = _boot.check_seed(seed)
    out = np.full((e_n, c, k), -1, np.int32)
    for ci in range(c):
        n = int(off[ci + 1] - off[ci])
        mine = rows[off[ci]:off[ci + 1]]
        if n <= k:
            out[:, ci, :n] = mine
            continue
        for e in range(e_n):
            key = _boot.key(seed, (first + e) * 64 + ci)
            got = np.zeros(0, np.int64)
            j = 0
            while len(got) < k and j < MAX_DRAWS:
                step = min(MAX_DRAWS - j, max(64, 4 * k))
                r = np.concatenate([got, _draws(key, j, j + step, n)])
                _, firsts = np.unique(r, return_index=True)
                got = r[np.sort(firsts)][:k]
                j += step
            out[e, ci, :len(got)] = mine[got]
    return out


def _kept(x: np.ndarray) -> np.ndarray:
    """The skip rule per row: finite and every |x| <= 1."""
    with np.errstate(invalid="ignore"):
        return (np.abs(x) <= 1.0).all(axis=-1)


def prototypes_numpy(train, support, centre=True):
    """keep_fewshot_prototypes in float64 -> ``(bank [E, C + 1, D], consts [E, 2 C + 1], valid uint8 [E, C], skipped, rho)``: ``skipped`` the
    sampled rows the skip rule dropped, ``rho`` the smallest non-zero ``|s_i - mu|`` met (inf when there is none)."""
    x32 = _host(train)
    sup = _host(support).astype(np.int64)
    if x32.ndim != 2 or sup.ndim != 3:
        raise ValueError(f"train must be [M, D] and support [E, C, shots], got {x32.shape} and {sup.shape}")
    m_rows, d = x32.shape
    e_n, c, _ = sup.shape
    ok_row = _kept(x32)
    x = np.where(ok_row[:, None], x32, 0).astype(np.float64)
    bank, consts = np.zeros((e_n, c + 1, d)), np.zeros((e_n, 2 * c + 1))
    valid = np.zeros((e_n, c), np.uint8)
    skipped, rho = 0, np.inf
    for e in range(e_n):
        lists = []
        for ci in range(c):
            s = sup[e, ci]
            s = s[(s >= 0) & (s < m_rows)]
            skipped += int((~ok_row[s]).sum())
            lists.append(s[ok_row[s]])
        allrows = np.concatenate(lists)
        mu = x[allrows].mean(0) if centre and len(allrows) else np.zeros(d)
        bank[e, c] = mu
        consts[e, 2 * c] = mu @ mu
        for ci, s in enumerate(lists):
            if not len(s):
                continue
            v = x[s] - mu
            nrm = np.sqrt((v * v).sum(1))
            if (nrm > 0).any():
                rho = min(rho, float(nrm[nrm > 0].min()))
            z = np.divide(v, nrm[:, None], out=np.zeros_like(v), where=nrm[:, None] > 0)
            p = z.mean(0)
            bank[e, ci], valid[e, ci] = p, 1
            consts[e, ci], consts[e, c + ci] = mu @ p, 0.5 * (p @ p)
    return bank, consts, valid, skipped, rho


def classify_numpy(bank, valid, x, truth=None, consts=None):
    """keep_fewshot_classify in float64 -> ``dict(labels int32 [N, E], scores [N, E, C], margin [N, E], r [N, E], confusion int64 [E, C, C]
    or None, skipped)``.  ``scores`` are ``s_c = q . p_c - h_c`` (-inf for an invalid class), ``margin`` the best minus the runner-up (0
    with one valid class); a skipped row or ``r = 0`` gives label -1, zero scores, margin 0.  With ``consts`` None the direct computation
    from the bank (centre, normalise, dot); with ``consts`` (``[E, 2 C + 1]``, say the device's) the fused form ``((x.p_c - mu.p_c) - h_c r) /
    r`` over those words taken as exact."""
    b = _host(bank).astype(np.float64)
    v = _host(valid).astype(bool)
    x32 = _host(x)
    e_n, c1, d = b.shape
    c = c1 - 1
    n = x32.shape[0]
    ok = _kept(x32)
    xs = np.where(ok[:, None], x32, 0).astype(np.float64)
    labels = np.full((n, e_n), -1, np.int32)
    scores = np.zeros((n, e_n, c))
    margin = np.zeros((n, e_n))
    rr = np.zeros((n, e_n))
    for e in range(e_n):
        p, mu = b[e, :c], b[e, c]
        if consts is None:
            mp, h, mm = p @ mu, 0.5 * (p * p).sum(1), mu @ mu
        else:
            k = _host(consts).astype(np.float64)[e]
            mp, h, mm = k[:c], k[c:2 * c], k[2 * c]
        r = np.sqrt(np.maximum(0.0, 1.0 - 2.0 * (xs @ mu) + mm)) if consts is not None else np.sqrt((((xs - mu) ** 2).sum(1)))
        live = ok & (r > 0) & v[e].any()
        rs = np.where(live, r, 1.0)
        s = ((xs @ p.T - mp) - h * rs[:, None]) / rs[:, None]
        s = np.where(v[e][None, :], s, -np.inf)
        lab = np.argmax(s, axis=1)                                  # the first maximum
        top = np.sort(s, axis=1)
        labels[:, e] = np.where(live, lab, -1)
        scores[:, e] = np.where(live[:, None], s, 0.0)
        with np.errstate(invalid="ignore"):
            margin[:, e] = np.where(live & (v[e].sum() >= 2), top[:, -1] - top[:, -2], 0.0)
        rr[:, e] = np.where(ok, r, 0.0)
    conf = None
    if truth is not None:
        t = _host(truth).astype(np.int64)
        conf = np.zeros((e_n, c, c), np.int64)
        for e in range(e_n):
            on = (t >= 0) & (t < c) & (labels[:, e] >= 0)
            conf[e] = np.bincount(t[on] * c + labels[on, e], minlength=c * c).reshape(c, c)
    return dict(labels=labels, scores=scores, margin=margin, r=rr, confusion=conf, skipped=int((~ok).sum()))


def slide_call_numpy(scores, top: int) -> Tuple[int, np.ndarray]:
    """``wsi.prototype_slide_call`` restated: scores ``[N, C]`` of the kept tiles -> (label, pooled ``[C]``): the mean of each class's ``min(top,
    N)`` largest tile scores, the first maximum."""
    s = np.asarray(scores, np.float64)
    k = min(int(top), s.shape[0])
    pooled = np.sort(s, axis=0)[::-1][:k].mean(0)
    return int(np.argmax(pooled)), pooled
