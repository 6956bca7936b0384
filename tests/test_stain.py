"""The fixed-point Macenko stain normalisation, CPU half: keep_amd.stain's numpy restatements, which the
device kernels are held to bit for bit (tests/test_stain_gpu.py), are held here to a plain float64 Macenko written in this file.

Bounds.  The apply is capped at ONE grey level against the float transform of the same fit (the integer OD differs from the float
one by about 1e-3, a quarter of a level at the steepest point of the exponential, and each side rounds once).  The fit bounds are
twice what was measured on the two fixtures (figures in DESIGN.md section 25): stain-vector components within 1.18e-3, maxC within
5.2e-3; their scale is set by the half-widths of the angle bins (pi / 4096 = 7.7e-4) and of the concentration bins (1 / 1024)."""
import os
from fractions import Fraction

import numpy as np
import pytest

from keep_amd import stain as S
from keep_amd.region import TissueMask
from keep_amd.synth import synth_tile_family

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HE_BOUND, MAXC_BOUND = 1.18e-3, 5.2e-3          # 2 x the measured 5.9e-4 (mosaic) / 2.6e-3 (example.tif), the worse fixture of each

_IMAGES = {}


def image(name):
    if name not in _IMAGES:
        if name == "example":
            from PIL import Image
            _IMAGES[name] = np.array(Image.open(os.path.join(ROOT, "tests", "golden", "example.tif")))[..., :3].copy()       # 224 x 298
        elif name == "random":
            _IMAGES[name] = np.random.default_rng(0).integers(0, 256, (512, 512, 3), dtype=np.uint8)
        else:                                                      # 2 x 3 stain_field tiles
            t = synth_tile_family("stain_field", 0, 6, "cpu", seed=7011, unit=8).numpy()
            _IMAGES[name] = np.ascontiguousarray(t.reshape(2, 3, 224, 224, 3).transpose(0, 2, 1, 3, 4).reshape(448, 672, 3))
    return _IMAGES[name]


# ------------------------------------------------------------------------------------------------ the float64 method
def float_od(rgb, io=240.0):
    return -np.log((rgb.reshape(-1, 3).astype(np.float64) + 1.0) / io)


def float_fit(rgb, io=240.0, alpha=1.0, beta=0.15):
    """Macenko et al. 2009 as the common float implementations run it -> (HE [3,2] haematoxylin first, maxC [2])."""
    od = float_od(rgb, io)
    kept = od[~np.any(od < beta, axis=1)]
    _, vec = np.linalg.eigh(np.cov(kept.T))
    V = vec[:, 1:3] * np.where(vec[:, 1:3].sum(0) < 0, -1.0, 1.0)
    t = kept @ V
    phi = np.arctan2(t[:, 1], t[:, 0])
    lo, hi = np.percentile(phi, alpha), np.percentile(phi, 100.0 - alpha)
    v_min, v_max = V @ np.array([np.cos(lo), np.sin(lo)]), V @ np.array([np.cos(hi), np.sin(hi)])
    he = np.stack([v_min, v_max], 1) if v_min[0] > v_max[0] else np.stack([v_max, v_min], 1)
    conc = np.linalg.lstsq(he, od.T, rcond=None)[0]
    return he, np.array([np.percentile(conc[0], 99), np.percentile(conc[1], 99)])


def float_apply(rgb, T, io_in=240.0, io_out=240.0):
    return np.clip(np.rint(io_out * np.exp(-(float_od(rgb, io_in) @ T.T))), 0, 255).astype(np.int64).reshape(rgb.shape)


def float_matrix(he, max_c):
    t = S.StainTarget()
    return t.he_ref @ np.diag(t.max_c_ref / max_c) @ np.linalg.pinv(he)


_FITS = {}


def fits(name):
    if name not in _FITS:
        _FITS[name] = (S.stain_fit_numpy(image(name)), float_fit(image(name)))
    return _FITS[name]


# ------------------------------------------------------------------------------------------------ apply
@pytest.mark.parametrize("name", ["example", "random"])
def test_apply_is_within_one_level_of_the_float_transform(name):
    fit = fits("example")[0]
    px = image(name)
    for keep in (("H", "E"), ("H",), ("E",)):
        tb = fit.tables(keep=keep)
        got = S.stain_apply_numpy(px, tb["od_q"], tb["t_q"], tb["exp_lut"], tb["lo"]).astype(np.int64)
        diff = np.abs(got - float_apply(px, fit.matrix(keep=keep)))
        print(f"apply {name} keep={keep}: max {diff.max()}, share differing {np.mean(diff > 0):.4f}")
        assert got.shape == px.shape and diff.max() <= 1


def test_apply_saturates_at_both_ends_of_the_exp_table():
    od_q, lut = S.od_table(240), S.exp_table(240)
    px = np.array([[0, 0, 0], [255, 255, 255], [17, 200, 3]], dtype=np.uint8)
    dark = S.stain_apply_numpy(px, od_q, S.quantise(np.full((3, 3), 64.0)), lut)
    light = S.stain_apply_numpy(px, od_q, S.quantise(np.full((3, 3), -64.0)), lut)
    assert dark[0].tolist() == [0, 0, 0] and light[0].tolist() == [255, 255, 255]          # OD 5.48 x +-192: past both ends
    assert dark[1].tolist() == [255, 255, 255] and light[1].tolist() == [0, 0, 0]          # OD -0.0645 x +-192 = -+12.4
    assert lut[0] == 255 and lut[-1] == 0 and len(lut) == S.LUT_LEN
    steep = S.StainFit(1.0, 0.15, 240.0)                           # concentrations a thousandth of the target's: |T| > 64
    steep.he, steep.max_c = fits("example")[0].he, fits("example")[0].max_c * 1e-3
    with pytest.raises(ValueError, match="> 64"):
        steep.tables()


# ------------------------------------------------------------------------------------------------ fit
@pytest.mark.parametrize("name", ["example", "mosaic"])
def test_fit_is_close_to_the_float_fit(name):
    fit, (he, max_c) = fits(name)
    d_he, d_c = np.abs(fit.he - he).max(), np.abs(fit.max_c - max_c).max()
    print(f"fit {name}: n {fit.n}, |dHE| {d_he:.3e}, |dmaxC| {d_c:.3e}, HE {fit.he.tolist()}, maxC {fit.max_c.tolist()}")
    assert fit.he[0, 0] > fit.he[0, 1]                             # haematoxylin first
    assert d_he <= HE_BOUND and d_c <= MAXC_BOUND


def test_end_to_end_against_the_float_method():
    px = image("example")
    fit, (he, max_c) = fits("example")
    tb = fit.tables()
    got = S.stain_apply_numpy(px, tb["od_q"], tb["t_q"], tb["exp_lut"], tb["lo"]).astype(np.int64)
    diff = np.abs(got - float_apply(px, float_matrix(he, max_c)))
    print(f"end to end example.tif: max {diff.max()}, share over 1 {np.mean(diff > 1):.6f}, share differing {np.mean(diff > 0):.4f}")
    assert diff.max() <= 2


# ------------------------------------------------------------------------------------------------ angle binning
def exact_bin(x, y):
    """floor((atan2(y, x) + pi) / (2 pi) A) mod A in float64 (|x|, |y| < 2^31 convert exactly and atan2 is good to 1e-15 rad); None
    within 1e-9 rad of a bin edge, where that cannot decide and the 2^-30 rounding of the direction table may (the axes and
    diagonals, which sit ON edges, are checked in closed form instead)."""
    A = S.ANGLE_BINS
    pos = (np.arctan2(float(y), float(x)) + np.pi) / (2 * np.pi) * A
    if abs(pos - round(pos)) * (2 * np.pi / A) < 1e-9:
        return None
    return int(np.floor(pos)) % A


def test_angle_bins_match_exact_arithmetic():
    g = np.random.default_rng(3)
    big = g.integers(-(1 << 31) + 1, 1 << 31, (3000, 2))
    small = g.integers(-40, 41, (1500, 2))
    pts = np.concatenate([big, small])
    got = S.angle_bin_numpy(pts[:, 0], pts[:, 1])
    checked = 0
    for (x, y), b in zip(pts.tolist(), got.tolist()):
        want = exact_bin(x, y)
        if want is not None:
            assert b == want, (x, y, b, want)
            checked += 1
    assert checked > 4000
    # on the axes and the diagonals the bin is known in closed form: multiples of A / 8, the angle pi wrapping to -pi
    A = S.ANGLE_BINS
    for m in (1, 7, 12345, (1 << 31) - 1):
        exact = {(m, 0): A // 2, (m, m): 5 * A // 8, (0, m): 3 * A // 4, (-m, m): 7 * A // 8, (-m, 0): 0, (-m, -m): A // 8, (0, -m): A // 4,
                 (m, -m): 3 * A // 8}
        for (x, y), want in exact.items():
            assert int(S.angle_bin_numpy(x, y)) == want, (x, y)
    assert int(S.angle_bin_numpy(0, 0)) == A // 2
    # the rational check of the table itself: direction j lies within 2^-29 of the true one, in exact fractions of its own length
    d = S.angle_dirs().astype(object)
    for j in (1, 511, 512, 513, 1023):
        assert abs(Fraction(int(d[j][0]) ** 2 + int(d[j][1]) ** 2, 1 << 60) - 1) < Fraction(1, 1 << 28)


def test_histograms_count_what_they_should():
    px = image("example")
    fit = fits("example")[0]
    od = S.od_table(240)[px].astype(np.int64)
    kept = int((od >= S.beta_level(0.15)).all(-1).sum())
    assert fit.n == kept == int(fit.moments[0]) and int(fit.angle_hist.sum()) == kept
    assert fit.conc_hist.sum(1).tolist() == [px.shape[0] * px.shape[1]] * 2
    m = np.zeros((56, 75), np.uint8)
    m[5:40, 10:60] = 1
    allowed = np.kron(m, np.ones((4, 4), np.uint8))[:224, :298].astype(bool)
    masked = S.stain_fit_numpy(px, TissueMask(m, 4))
    assert masked.n == int(((od >= S.beta_level(0.15)).all(-1) & allowed).sum()) and int(masked.angle_hist.sum()) == masked.n
    assert masked.conc_hist.sum(1).tolist() == [int(allowed.sum())] * 2
    # moments against a plain float sum
    sel = od[(od >= S.beta_level(0.15)).all(-1)]
    assert np.array_equal(fit.moments[1:4], sel.sum(0)) and fit.moments[5] == int((sel[:, 0] * sel[:, 1]).sum())


# ------------------------------------------------------------------------------------------------ error paths, keep=, bands
def test_an_all_glass_image_raises():
    glass = np.full((40, 50, 3), 236, np.uint8)
    with pytest.raises(ValueError, match="0 pixels"):
        S.stain_fit_numpy(glass)
    one = glass.copy()
    one[3, 4] = (120, 40, 130)
    with pytest.raises(ValueError, match="1 pixels"):
        S.stain_fit_numpy(one)
    flat = glass.copy()
    flat[:10] = (120, 40, 130)                                     # 500 kept pixels of ONE colour: no plane
    with pytest.raises(ValueError, match="500"):
        S.stain_fit_numpy(flat)
    for bad in (dict(alpha=50), dict(beta=-1), dict(io=0)):
        with pytest.raises(ValueError):
            S.stain_fit_numpy(image("example"), **bad)


def test_single_stain_matrices_sum_to_the_full_one():
    fit = fits("example")[0]
    full, h, e = fit.matrix(), fit.matrix(keep=("H",)), fit.matrix(keep=("E",))
    assert np.allclose(h + e, full, rtol=0, atol=1e-12) and np.abs(h).max() > 0 and np.abs(e).max() > 0
    assert np.linalg.matrix_rank(h) == 1 and np.linalg.matrix_rank(e) == 1
    with pytest.raises(ValueError):
        fit.matrix(keep=("X",))


def test_three_bands_give_the_one_call_fit():
    px = image("example")
    whole = fits("example")[0]
    fit = None
    for band in (px[:70], px[70:71], px[71:]):
        fit = S.stain_fit_numpy(band, into=fit)
    for name in ("moments", "v_q", "angle_hist", "minv_q", "conc_hist", "he", "max_c"):
        assert np.array_equal(getattr(fit, name), getattr(whole, name)), name
    assert fit.n == whole.n
    with pytest.raises(ValueError, match="into"):
        S.stain_fit_numpy(px, beta=0.2, into=whole)
