"""Nearest neighbours: the key of a (score, bank row) pair, the ``Neighbours`` result of
``KEEPModel.topk`` / ``topk_batches`` and the numpy restatements the tests hold the kernels to.

A neighbour is one 64-bit key (``KEEP_TOPK_KEY`` of include/keep_hip.h)::

    ord(s):    u = bits(float32(s) + 0.0);  u ^= 0xFFFFFFFF if u >> 31 else 0x80000000
    key(s, g): ord(s) << 32 | 0xFFFFFFFF - g          g: the row's global bank index, 0 <= g <= 2^32 - 2
    empty:     0

A larger key is a larger score and, of equal scores, the lower index.  A neighbour list is k keys in descending order; the top k of a
union of candidates is the k largest keys of the union, so lists merge exactly whatever the split of the bank."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np
import torch

MAX_K = 64
MAX_SEGMENTS = 1024
MAX_INDEX = (1 << 32) - 2                # the largest global bank index a key can hold
MAX_CLASSES = 64
MODES = {"uniform": 0, "softmax": 1}     # KEEP_KNN_UNIFORM / KEEP_KNN_SOFTMAX


def check_k(k) -> int:
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_K:
        raise ValueError(f"k must be an integer in 1..{MAX_K}, got {k!r}")
    return int(k)


def check_bank_range(bank_base, m: int) -> int:
    if isinstance(bank_base, bool) or not isinstance(bank_base, (int, np.integer)) or int(bank_base) < 0 or int(bank_base) + m > MAX_INDEX + 1:
        raise ValueError(f"bank_base must be an integer >= 0 with bank_base + M <= 2^32 - 1, got {bank_base!r} with M = {m}")
    return int(bank_base)


def check_self_first(self_first) -> int:
    """None -> -1 (no exclusion), else a global row index."""
    if self_first is None:
        return -1
    if isinstance(self_first, bool) or not isinstance(self_first, (int, np.integer)) or not 0 <= int(self_first) <= MAX_INDEX:
        raise ValueError(f"self_first must be None or a global row index in 0..2^32 - 2, got {self_first!r}")
    return int(self_first)


def check_segments(segments) -> int:
    if isinstance(segments, bool) or not isinstance(segments, (int, np.integer)) or not 0 <= int(segments) <= MAX_SEGMENTS:
        raise ValueError(f"segments must be 0 (chosen by the engine) or 1..{MAX_SEGMENTS}, got {segments!r}")
    return int(segments)


def check_vote_args(n_classes, weights, temperature) -> Tuple[int, int, float]:
    if isinstance(n_classes, bool) or not isinstance(n_classes, (int, np.integer)) or not 2 <= int(n_classes) <= MAX_CLASSES:
        raise ValueError(f"n_classes must be an integer in 2..{MAX_CLASSES}, got {n_classes!r}")
    if weights not in MODES:
        raise ValueError(f"weights must be 'uniform' or 'softmax', got {weights!r}")
    t = float(temperature)
    if not (t > 0.0 and np.isfinite(np.float32(t))) or np.float32(t) == 0:
        raise ValueError(f"temperature must be finite and > 0, got {temperature!r}")
    return int(n_classes), MODES[weights], t


# ------------------------------------------------------------------------------------------------ keys
def pack_keys_numpy(score, index) -> np.ndarray:
    """fp32 scores and global bank indices (any equal shapes; an index < 0 is an empty slot) -> uint64 keys."""
    s = np.asarray(score, np.float32) + np.float32(0.0)                  # -0 folded into +0
    g = np.asarray(index, np.int64)
    if s.shape != g.shape:
        raise ValueError(f"score {s.shape} and index {g.shape} differ in shape")
    if g.size and int(g.max()) > MAX_INDEX:
        raise ValueError(f"a bank index above 2^32 - 2: {int(g.max())}")
    if not np.isfinite(s[g >= 0]).all():
        raise ValueError("a key holds a finite score")
    u = s.view(np.uint32).astype(np.uint64)
    u = u ^ np.where(u >> np.uint64(31), np.uint64(0xFFFFFFFF), np.uint64(0x80000000))
    keys = (u << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.where(g >= 0, g, 0).astype(np.uint64))
    return np.where(g >= 0, keys, np.uint64(0))


def unpack_keys_numpy(keys) -> Tuple[np.ndarray, np.ndarray]:
    """uint64 keys (or the int64 bit patterns of ``Neighbours.keys``) -> (index int64, score fp32); an empty slot is (-1, 0)."""
    k = np.ascontiguousarray(keys)
    k = k.view(np.uint64) if k.dtype == np.int64 else k.astype(np.uint64)
    o = (k >> np.uint64(32)).astype(np.uint32)
    bits = np.where(o & np.uint32(0x80000000), o ^ np.uint32(0x80000000), ~o).astype(np.uint32)
    index = np.int64(0xFFFFFFFF) - (k & np.uint64(0xFFFFFFFF)).astype(np.int64)
    filled = k != 0
    return np.where(filled, index, -1), np.where(filled, bits.view(np.float32), np.float32(0))


def topk_numpy(scores, k: int, bank_base: int = 0, self_first: Optional[int] = None) -> np.ndarray:
    """A score matrix ``[Nq, M]`` (any float type, rounded to fp32; a non-finite score is no candidate, as a skipped row's) -> uint64
    ``[Nq, k]``: every row's k largest keys, descending, the tail empty where a row has fewer candidates.  Column c is global bank
    row ``bank_base + c``; with ``self_first`` query row i never takes global row ``self_first + i``."""
    k = check_k(k)
    s = np.asarray(scores).astype(np.float32)
    if s.ndim != 2:
        raise ValueError(f"scores must be [Nq, M], got shape {s.shape}")
    nq, m = s.shape
    bank_base, sf = check_bank_range(bank_base, m), check_self_first(self_first)
    g = np.broadcast_to(bank_base + np.arange(m, dtype=np.int64), s.shape)
    ok = np.isfinite(s)
    if sf >= 0:
        ok = ok & (g != (sf + np.arange(nq, dtype=np.int64))[:, None])
    keys = pack_keys_numpy(np.where(ok, s, np.float32(0)), np.where(ok, g, -1))
    keys = np.sort(keys, axis=1)[:, ::-1]
    out = np.zeros((nq, k), np.uint64)
    out[:, :min(k, m)] = keys[:, :k]
    return out


def merge_numpy(a, b) -> np.ndarray:
    """The k largest keys of two lists of the same queries, uint64 ``[Nq, k]`` each."""
    a, b = (np.ascontiguousarray(x).view(np.uint64) if np.asarray(x).dtype == np.int64 else np.asarray(x, np.uint64) for x in (a, b))
    if a.shape != b.shape or a.ndim != 2:
        raise ValueError(f"the lists must be [Nq, k] both, got {a.shape} and {b.shape}")
    return np.ascontiguousarray(np.sort(np.concatenate([a, b], axis=1), axis=1)[:, ::-1][:, :a.shape[1]])


def knn_vote_numpy(index, score, bank_labels, C: int, mode: str = "uniform", temperature: float = 0.07):
    """The vote of ``keep_knn_vote`` restated -> ``(labels int32 [Nq], probs fp32 [Nq, C], margin fp32 [Nq], skipped)``.  Neighbour r
    (``index[:, r]`` >= 0) votes for ``bank_labels[index]`` when that lies in 0..C-1, with weight 1 or ``exp((s_r - s_0) / T)`` (the
    subtraction and the division in fp32, the exponential in float64, rounded once); the sums are fp32 adds in list order, the total
    in class order."""
    C, m, t = check_vote_args(C, mode, temperature)
    index, score = np.asarray(index, np.int64), np.asarray(score, np.float32)
    y = np.asarray(bank_labels).astype(np.int64)
    nq, k = index.shape
    lab = np.where(index >= 0, y[np.clip(index, 0, len(y) - 1)], -1)
    lab = np.where((lab >= 0) & (lab < C), lab, -1)
    if m == 1:
        z = (score - score[:, :1]) / np.float32(t)
        w = np.exp(z.astype(np.float64)).astype(np.float32)
    else:
        w = np.ones((nq, k), np.float32)
    v = np.zeros((nq, C), np.float32)
    rows = np.arange(nq)
    for r in range(k):
        on = lab[:, r] >= 0
        v[rows[on], lab[on, r]] += w[on, r]
    tot = np.zeros(nq, np.float32)
    for c in range(C):
        tot = tot + v[:, c]
    voted = tot > 0
    probs = np.zeros((nq, C), np.float32)
    probs[voted] = v[voted] / tot[voted, None]
    labels = np.where(voted, v.argmax(axis=1), -1).astype(np.int32)
    rest = probs.copy()
    rest[rows, np.maximum(labels, 0)] = -1
    margin = np.where(voted, probs[rows, np.maximum(labels, 0)] - rest.max(axis=1), 0).astype(np.float32)
    return labels, probs, margin, int((~voted).sum())


# ------------------------------------------------------------------------------------------------ the result
@dataclass
class Neighbours:
    """The k nearest bank rows of every query row, on the device.  ``keys`` int64 ``[Nq, k]``: the bit patterns of the uint64 keys,
    descending; ``index`` int64 ``[Nq, k]``: global bank rows, -1 for an empty slot; ``score`` fp32 ``[Nq, k]``: exactly the fp32 in the
    key, 0 for an empty slot; ``count`` int32 ``[Nq]``: filled slots; ``n_bank``: one more than the largest global row offered so far;
    ``query_skipped`` / ``bank_skipped``: int64 ``[1]`` counts of rows the skip rule left out (a skipped query's list is empty)."""
    keys: torch.Tensor
    index: torch.Tensor
    score: torch.Tensor
    count: torch.Tensor
    k: int
    n_bank: int
    query_skipped: torch.Tensor
    bank_skipped: torch.Tensor
    _ops: object = field(default=None, repr=False, compare=False)

    def keys_numpy(self) -> np.ndarray:
        """The keys as uint64 on the host."""
        return self.keys.cpu().numpy().view(np.uint64)

    def merge(self, other: "Neighbours") -> "Neighbours":
        """The k best of both results (the same queries against two disjoint parts of a bank), merged on the device by keys alone."""
        if not isinstance(other, Neighbours):
            raise ValueError(f"other must be a Neighbours, got {type(other).__name__}")
        if tuple(other.keys.shape) != tuple(self.keys.shape):
            raise ValueError(f"the lists differ in shape: {tuple(self.keys.shape)} and {tuple(other.keys.shape)}")
        if self._ops is None:
            raise ValueError("this Neighbours was not made by an engine; merge host keys with merge_numpy")
        return self._ops._topk_merged(self, other)
