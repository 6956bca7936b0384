"""Macenko stain normalisation in fixed point: the host half and the numpy restatements.

The method is Macenko et al. 2009 as the common float implementations run it: optical density ``OD = -ln((I + 1) / Io)``, pixels
with any channel ``OD < beta`` dropped, the plane of the two leading eigenvectors of the OD covariance, the ``alpha`` /
``100 - alpha`` angle percentiles in that plane as the two stain vectors (haematoxylin first), concentrations by least squares and
their 99th percentiles, rescaling to a target, ``Io exp(-OD)`` back.  Here every pass over pixels is integer arithmetic, so the
device kernels (keep_amd/csrc/stain.hip) and the restatements below agree bit for bit; the dense algebra between the passes (a
3 x 3 ``eigh``, a 3 x 2 ``pinv``, percentiles read off histograms) is float64 on the host and shared by both paths.

Q formats: ``od_q`` Q12, ``V_q`` / ``Minv_q`` / ``T_q`` Q14, concentrations Q26 binned at ``>> 17`` (1 / 512), the transformed OD
Q10 (``>> 16`` of Q26, rounded half up), directions of the angle table Q30.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

OD_BITS, VEC_BITS, DIR_BITS = 12, 14, 30
ANGLE_BINS = 4096                     # equal bins of [-pi, pi)
CONC_BINS, CONC_SHIFT = 4096, 17      # Q26 >> 17: 1 / 512 per bin, 0 .. 8
OUT_SHIFT, OUT_ONE = 16, 1024         # Q26 -> Q10
LUT_LO, LUT_LEN = -72, 6500           # the exp table covers OD -0.07 .. 6.28
T_MAX = 64.0
DEFAULT_HE_REF = ((0.5626, 0.2159), (0.7201, 0.8012), (0.4062, 0.5581))
DEFAULT_MAX_C_REF = (1.9705, 1.0308)
MAX_PIXELS = 1 << 30
STAINS = ("H", "E")


class StainTarget:
    """Where a fit is mapped to: stain vectors ``he_ref`` [3,2] (haematoxylin first), 99th-percentile concentrations ``max_c_ref``
    [2] and the white level ``io``.  The default is the customary Macenko reference."""

    def __init__(self, he_ref=DEFAULT_HE_REF, max_c_ref=DEFAULT_MAX_C_REF, io: float = 240):
        self.he_ref = np.array(he_ref, dtype=np.float64)
        self.max_c_ref = np.array(max_c_ref, dtype=np.float64)
        self.io = check_io(io)
        if self.he_ref.shape != (3, 2) or self.max_c_ref.shape != (2,) or not (np.isfinite(self.he_ref).all() and (self.max_c_ref > 0).all()):
            raise ValueError(f"he_ref must be finite [3,2] and max_c_ref positive [2], got {self.he_ref.shape} and {self.max_c_ref!r}")

    def __repr__(self):
        return f"StainTarget(he_ref={self.he_ref.tolist()}, max_c_ref={self.max_c_ref.tolist()}, io={self.io})"


def check_io(io) -> float:
    if isinstance(io, bool) or not 1 <= float(io) <= 4096:
        raise ValueError(f"io must lie in [1, 4096], got {io!r}")
    return float(io)


def check_fit_args(alpha, beta, io) -> Tuple[float, float, float]:
    if isinstance(alpha, bool) or not 0 <= float(alpha) < 50:
        raise ValueError(f"alpha must lie in [0, 50), got {alpha!r}")
    if isinstance(beta, bool) or not 0 <= float(beta) <= 4:
        raise ValueError(f"beta must lie in [0, 4], got {beta!r}")
    return float(alpha), float(beta), check_io(io)


# ---------------------------------------------------------------------------------------------- host-made tables
def od_table(io: float = 240) -> np.ndarray:
    """``od_q[v] = rint(-ln((v + 1) / io) 2^12)``, int32 [256]."""
    v = np.arange(256, dtype=np.float64)
    return np.rint(-np.log((v + 1.0) / io) * (1 << OD_BITS)).astype(np.int32)


def beta_level(beta: float) -> int:
    return int(np.rint(beta * (1 << OD_BITS)))


_DIRS = None


def angle_dirs() -> np.ndarray:
    """``(rint(2^30 cos), rint(2^30 sin))`` of ``j 2 pi / 4096`` for the first quadrant, int32 [1024,2]."""
    global _DIRS
    if _DIRS is None:
        a = np.arange(ANGLE_BINS // 4, dtype=np.float64) * (2.0 * np.pi / ANGLE_BINS)
        _DIRS = np.rint(np.stack([np.cos(a), np.sin(a)], 1) * (1 << DIR_BITS)).astype(np.int32)
    return _DIRS


def exp_table(io: float = 240, lo: int = LUT_LO, length: int = LUT_LEN) -> np.ndarray:
    """``exp_lut[i] = clip(rint(io exp(-(i + lo) / 1024)), 0, 255)``, uint8 [length]."""
    i = np.arange(length, dtype=np.float64) + lo
    return np.clip(np.rint(io * np.exp(-i / OUT_ONE)), 0, 255).astype(np.uint8)


def quantise(m, bits: int = VEC_BITS) -> np.ndarray:
    return np.rint(np.asarray(m, dtype=np.float64) * (1 << bits)).astype(np.int64).astype(np.int32)


# ---------------------------------------------------------------------------------------------- numpy restatements
def _rgb(image) -> np.ndarray:
    a = image.cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"image must be uint8 [h,w,3] (RGB) or [h,w,4] (RGBA), got {a.dtype} {a.shape}")
    if a.shape[0] * a.shape[1] > MAX_PIXELS:
        raise ValueError(f"image of {a.shape[0]}x{a.shape[1]} pixels: the fit takes h * w <= 2^30")
    return a[..., :3]


def mask_split(tissue):
    """``tissue=``: None or a ``keep_amd.region.TissueMask`` -> (mask tensor or None, downsample)."""
    from .region import TissueMask
    if tissue is None:
        return None, 1
    if not isinstance(tissue, TissueMask):
        raise ValueError(f"tissue must be a TissueMask or None, got {type(tissue).__name__}")
    return tissue.mask, tissue.downsample


def _allowed(h: int, w: int, mask, downsample: int) -> np.ndarray:
    """bool [h,w]: pixel (x, y) reads ``mask[y // downsample, x // downsample]``; outside the mask it is not allowed."""
    if mask is None:
        return np.ones((h, w), bool)
    m = mask.cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
    my, mx = np.arange(h) // downsample, np.arange(w) // downsample
    inside = (my < m.shape[0])[:, None] & (mx < m.shape[1])[None, :]
    return inside & (m[np.minimum(my, m.shape[0] - 1)][:, np.minimum(mx, m.shape[1] - 1)] != 0)


def _od_pixels(image, od_q, mask, downsample, beta_q=None) -> np.ndarray:
    """int64 [n,3]: od_q of the pixels the mask allows and, with ``beta_q``, whose three channels are all >= it; row-major."""
    rgb = _rgb(image)
    od = np.asarray(od_q, dtype=np.int64)[rgb]
    keep = _allowed(rgb.shape[0], rgb.shape[1], mask, downsample)
    if beta_q is not None:
        keep &= (od >= beta_q).all(-1)
    return od[keep]


def stain_moments_numpy(image, od_q, beta_q: int, mask=None, downsample: int = 1) -> np.ndarray:
    """What ``keep_stain_moments`` computes: int64 [10] = n, S_r, S_g, S_b, S_rr, S_rg, S_rb, S_gg, S_gb, S_bb over the kept pixels."""
    od = _od_pixels(image, od_q, mask, downsample, beta_q)
    r, g, b = od[:, 0], od[:, 1], od[:, 2]
    return np.array([len(od), r.sum(), g.sum(), b.sum(), (r * r).sum(), (r * g).sum(), (r * b).sum(), (g * g).sum(), (g * b).sum(), (b * b).sum()],
                    dtype=np.int64)


def angle_bin_numpy(x, y) -> np.ndarray:
    """The bin of ``atan2(y, x)`` among 4096 equal bins of ``[-pi, pi)`` for integer ``|x|, |y| < 2^31``, by integer comparisons only (as
    the device decides it): the quadrant from the signs, an exact rotation into the first quadrant, a binary search of
    :func:`angle_dirs` by the sign of the cross product.  ``(0, 0)`` counts as the angle 0, the angle ``pi`` as ``-pi``."""
    x, y = np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64)
    Q = ANGLE_BINS // 4
    q2, q3, q0, q1 = (x > 0) & (y >= 0), (x <= 0) & (y > 0), (x < 0) & (y <= 0), (x >= 0) & (y < 0)
    base = np.select([q2, q3, q0, q1], [2 * Q, 3 * Q, 0, Q], 2 * Q)
    u = np.select([q2, q3, q0, q1], [x, y, -x, -y], 1)
    w = np.select([q2, q3, q0, q1], [y, -x, -y, x], 0)
    d = angle_dirs().astype(np.int64)
    lo, hi = np.zeros(x.shape, np.int64), np.full(x.shape, Q, np.int64)
    for _ in range(10):                                            # log2(1024) halvings, all lanes in step like the kernel's loop
        mid = (lo + hi) >> 1
        ge = d[mid, 0] * w - d[mid, 1] * u >= 0
        lo, hi = np.where(ge, mid, lo), np.where(ge, hi, mid)
    return (base + lo).astype(np.int64)


def stain_angle_hist_numpy(image, od_q, beta_q: int, v_q, mask=None, downsample: int = 1) -> np.ndarray:
    """What ``keep_stain_angle_hist`` computes: int64 [4096], the histogram of the kept pixels' plane angles."""
    t = _od_pixels(image, od_q, mask, downsample, beta_q) @ np.asarray(v_q, dtype=np.int64).reshape(3, 2)
    return np.bincount(angle_bin_numpy(t[:, 0], t[:, 1]), minlength=ANGLE_BINS).astype(np.int64)


def stain_conc_hist_numpy(image, od_q, minv_q, mask=None, downsample: int = 1) -> np.ndarray:
    """What ``keep_stain_conc_hist`` computes: int64 [2,4096] over every pixel the mask allows (no beta rule)."""
    c = _od_pixels(image, od_q, mask, downsample) @ np.asarray(minv_q, dtype=np.int64).reshape(2, 3).T
    k = np.clip(c >> CONC_SHIFT, 0, CONC_BINS - 1)
    return np.stack([np.bincount(k[:, s], minlength=CONC_BINS) for s in range(2)]).astype(np.int64)


def stain_apply_numpy(pixels, od_q, t_q, exp_lut, lo: int = LUT_LO) -> np.ndarray:
    """What ``keep_stain_apply_u8`` computes on uint8 ``[..., 3]`` pixels: table -> 3 x 3 integer matrix -> table."""
    p = np.asarray(pixels)
    if p.dtype != np.uint8 or p.shape[-1] != 3:
        raise ValueError(f"pixels must be uint8 [..., 3], got {p.dtype} {p.shape}")
    lut = np.asarray(exp_lut, dtype=np.uint8)
    od = np.asarray(od_q, dtype=np.int64)[p]
    o = (od @ np.asarray(t_q, dtype=np.int64).reshape(3, 3).T + (1 << (OUT_SHIFT - 1))) >> OUT_SHIFT
    return lut[np.clip(o - lo, 0, len(lut) - 1)]


# ---------------------------------------------------------------------------------------------- host steps between the passes
def _percentile_bin(hist: np.ndarray, pct: float) -> int:
    """The bin that holds sorted element ``floor(pct / 100 (n - 1))`` (0-based) of the ``n`` counted values."""
    n = int(hist.sum())
    k = int(math.floor(pct / 100.0 * (n - 1)))
    return int(np.searchsorted(np.cumsum(hist), k, side="right"))


def plane_from_moments(moments) -> Tuple[np.ndarray, np.ndarray]:
    """int64 [10] moments -> (V float64 [3,2], V_q int32 [3,2]): the eigenvectors of the second-largest and the largest eigenvalue
    of the OD covariance (in that order, as ``eigvecs[:, 1:3]`` of the float implementations), each signed so that its components
    sum to a positive number.  Raises ValueError with the count on fewer than 2 kept pixels or a degenerate plane."""
    m = [int(v) for v in np.asarray(moments).reshape(-1)]
    n = m[0]
    if n < 2:
        raise ValueError(f"stain fit: {n} pixels survive the mask and the beta threshold; at least 2 are needed")
    s, idx = m[1:4], {(0, 0): 4, (0, 1): 5, (0, 2): 6, (1, 1): 7, (1, 2): 8, (2, 2): 9}
    cov = np.empty((3, 3), dtype=np.float64)
    for (i, j), k in idx.items():                                  # n S_ij - S_i S_j in Python integers: exact before the one division
        cov[i, j] = cov[j, i] = (n * m[k] - s[i] * s[j]) / (n * (n - 1)) / float(1 << (2 * OD_BITS))
    w, vec = np.linalg.eigh(cov)
    if not w[1] > 0:
        raise ValueError(f"stain fit: the {n} kept pixels span no plane (second eigenvalue {w[1]:.3g} <= 0)")
    V = vec[:, 1:3].copy()
    V *= np.where(V.sum(0) < 0, -1.0, 1.0)
    return V, quantise(V)


def vectors_from_angles(angle_hist, v_q, alpha: float) -> Tuple[np.ndarray, np.ndarray]:
    """Angle histogram + the quantised plane -> (HE float64 [3,2] haematoxylin first, Minv_q int32 [2,3] = rint(pinv(HE) 2^14));
    both percentile angles are bin centres."""
    h = np.asarray(angle_hist, dtype=np.int64)
    V = np.asarray(v_q, dtype=np.float64).reshape(3, 2) / (1 << VEC_BITS)
    phi = [-np.pi + (_percentile_bin(h, p) + 0.5) * (2.0 * np.pi / ANGLE_BINS) for p in (alpha, 100.0 - alpha)]
    v_min, v_max = (V @ np.array([np.cos(a), np.sin(a)]) for a in phi)
    he = np.stack([v_min, v_max], 1) if v_min[0] > v_max[0] else np.stack([v_max, v_min], 1)
    return he, quantise(np.linalg.pinv(he))


def max_c_from_hist(conc_hist) -> np.ndarray:
    """Concentration histograms [2,4096] -> their 99th percentiles (bin centres), float64 [2]."""
    h = np.asarray(conc_hist, dtype=np.int64)
    return np.array([(_percentile_bin(h[s], 99.0) + 0.5) * float(1 << CONC_SHIFT) / float(1 << (OD_BITS + VEC_BITS)) for s in range(2)])


class StainFit:
    """A Macenko fit: ``he`` float64 [3,2] (stain vectors, haematoxylin first), ``max_c`` float64 [2] (99th-percentile
    concentrations), ``n`` kept pixels, and what they came from: ``moments`` int64 [10], ``v_q`` int32 [3,2], ``angle_hist`` int64
    [4096], ``minv_q`` int32 [2,3], ``conc_hist`` int64 [2,4096], with ``alpha`` / ``beta`` / ``io``.  ``sources`` are the images (and
    masks) it was accumulated over: the three passes each need the result of the one before over ALL pixels, so a fit continued with
    ``into=`` walks its earlier images again for the two histograms."""

    def __init__(self, alpha: float, beta: float, io: float):
        self.alpha, self.beta, self.io = alpha, beta, io
        self.sources = []
        self.moments = np.zeros(10, dtype=np.int64)
        self.n = 0
        self.v = self.v_q = self.angle_hist = self.he = self.minv_q = self.conc_hist = self.max_c = None

    def __repr__(self):
        return f"StainFit(n={self.n}, he={np.round(self.he, 4).tolist()}, max_c={np.round(self.max_c, 4).tolist()}, io={self.io})"

    def matrix(self, target: Optional[StainTarget] = None, keep: Sequence[str] = STAINS) -> np.ndarray:
        """float64 [3,3] ``T = HERef diag(maxCRef / maxC) pinv(HE)``: source OD -> target OD.  ``keep=("H",)`` / ``("E",)`` zeroes the
        other stain's concentration: the haematoxylin-only or eosin-only image (colour deconvolution) through the same kernel."""
        target = StainTarget() if target is None else target
        if not isinstance(target, StainTarget):
            raise ValueError(f"target must be a StainTarget, got {type(target).__name__}")
        keep = (keep,) if isinstance(keep, str) else tuple(keep)
        if not keep or any(k not in STAINS for k in keep):
            raise ValueError(f"keep must name stains of {STAINS}, got {keep!r}")
        scale = np.array([target.max_c_ref[s] / self.max_c[s] if STAINS[s] in keep else 0.0 for s in range(2)])
        return target.he_ref @ np.diag(scale) @ np.linalg.pinv(self.he)

    def tables(self, target: Optional[StainTarget] = None, keep: Sequence[str] = STAINS) -> dict:
        """The arrays ``keep_stain_apply_u8`` / :func:`stain_apply_numpy` take: ``od_q`` int32 [256] (the fit's ``io``), ``t_q`` int32
        [3,3], ``exp_lut`` uint8 [6500] (the target's ``io``) and ``lo``."""
        T = self.matrix(target, keep)
        if not np.isfinite(T).all() or np.abs(T).max() > T_MAX:
            raise ValueError(f"stain transform has an entry of magnitude {np.abs(T).max():.3g} > {T_MAX:g}")
        io_out = (StainTarget() if target is None else target).io
        return dict(od_q=od_table(self.io), t_q=quantise(T), exp_lut=exp_table(io_out), lo=LUT_LO)


class NumpyPasses:
    """The three pixel passes as the restatements run them; ``KEEPModel`` has the same three on the device."""

    @staticmethod
    def moments(image, mask, downsample, od_q, beta_q, acc):
        return (0 if acc is None else acc) + stain_moments_numpy(image, od_q, beta_q, mask, downsample)

    @staticmethod
    def angle_hist(image, mask, downsample, od_q, beta_q, v_q, acc):
        return (0 if acc is None else acc) + stain_angle_hist_numpy(image, od_q, beta_q, v_q, mask, downsample)

    @staticmethod
    def conc_hist(image, mask, downsample, od_q, minv_q, acc):
        return (0 if acc is None else acc) + stain_conc_hist_numpy(image, od_q, minv_q, mask, downsample)

    @staticmethod
    def to_numpy(acc):
        return np.asarray(acc, dtype=np.int64)


def run_fit(passes, image, tissue, alpha, beta, io, into: Optional[StainFit]) -> StainFit:
    """The whole fit over ``passes`` (numpy or device): pass 1 on the new image only, added to ``into``'s moments; then the two
    histogram passes over every image of the fit, since each needs the step before it finished over all pixels."""
    alpha, beta, io = check_fit_args(alpha, beta, io)
    mask, ds = mask_split(tissue)
    if into is not None:
        if not isinstance(into, StainFit):
            raise ValueError(f"into must be a StainFit, got {type(into).__name__}")
        if (into.alpha, into.beta, into.io) != (alpha, beta, io):
            raise ValueError(f"into was fitted with alpha / beta / io = {(into.alpha, into.beta, into.io)}, this call asks {(alpha, beta, io)}")
    fit = StainFit(alpha, beta, io)
    od_q, beta_q = od_table(io), beta_level(beta)
    fit.sources = (into.sources if into is not None else []) + [(image, mask, ds)]
    fit.moments = (into.moments if into is not None else 0) + passes.to_numpy(passes.moments(image, mask, ds, od_q, beta_q, None))
    fit.n = int(fit.moments[0])
    fit.v, fit.v_q = plane_from_moments(fit.moments)
    acc = None
    for img, m, d in fit.sources:
        acc = passes.angle_hist(img, m, d, od_q, beta_q, fit.v_q, acc)
    fit.angle_hist = passes.to_numpy(acc)
    fit.he, fit.minv_q = vectors_from_angles(fit.angle_hist, fit.v_q, alpha)
    acc = None
    for img, m, d in fit.sources:
        acc = passes.conc_hist(img, m, d, od_q, fit.minv_q, acc)
    fit.conc_hist = passes.to_numpy(acc)
    fit.max_c = max_c_from_hist(fit.conc_hist)
    if not (fit.max_c > 0).all():
        raise ValueError(f"stain fit: degenerate concentrations {fit.max_c.tolist()} over {fit.n} kept pixels")
    return fit


def stain_fit_numpy(image, tissue=None, alpha: float = 1, beta: float = 0.15, io: float = 240, into: Optional[StainFit] = None) -> StainFit:
    """``KEEPModel.stain_fit`` with the pixel passes in numpy: same host steps, same result bit for bit."""
    _rgb(image)
    return run_fit(NumpyPasses, image, tissue, alpha, beta, io, into)


def check_stain(stain, allow_name: bool = False):
    """The ``stain=`` keyword: None, a StainFit (mapped to the default target) or, where a thumbnail is at hand, "macenko"."""
    if stain is None or isinstance(stain, StainFit) or (allow_name and isinstance(stain, str) and stain == "macenko"):
        return stain
    name = ', "macenko"' if allow_name else ""
    raise ValueError(f"stain must be None{name} or a StainFit, got {stain!r}")
