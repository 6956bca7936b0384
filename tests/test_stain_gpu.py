"""Macenko stain normalisation on the MI355X: keep_stain_moments / keep_stain_angle_hist /
keep_stain_conc_hist / keep_stain_apply_u8, KEEPModel.stain_fit / stain_normalize and the ``stain=`` keyword of the region methods
and of cohort.extract_slide_features.

Everything on the device is integer arithmetic, so every comparison is exact: the yardsticks are keep_amd.stain's numpy
restatements (tests/test_stain.py holds them to a float64 Macenko) and encode_image_uint8 on tiles normalised by hand."""
import os

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel, cohort
from keep_amd import stain as S
from keep_amd.config import small_shape
from keep_amd.region import TissueMask, TissueSegmentation, plan_bands
from keep_amd.synth import _STAIN_E, _STAIN_H, synth_state_dict, synth_tile_family

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OD, BETA = S.od_table(240), S.beta_level(0.15)


@pytest.fixture(scope="module")
def model():
    m = KEEPModel(precision="strict")
    m.load_state_dict(synth_state_dict(small_shape(2, 2), seed=5), strict=True)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def passes(model):
    return model._StainPasses(model)


_CACHE = {}


def example():
    if "example" not in _CACHE:
        from PIL import Image
        _CACHE["example"] = np.array(Image.open(os.path.join(ROOT, "tests", "golden", "example.tif")))[..., :3].copy()      # 224 x 298
    return _CACHE["example"]


def mosaic():
    """2 x 3 stain_field tiles, uint8 [448, 672, 3] (tests/test_stain.py's)."""
    if "mosaic" not in _CACHE:
        t = synth_tile_family("stain_field", 0, 6, "cpu", seed=7011, unit=8).numpy()
        _CACHE["mosaic"] = np.ascontiguousarray(t.reshape(2, 3, 224, 224, 3).transpose(0, 2, 1, 3, 4).reshape(448, 672, 3))
    return _CACHE["mosaic"]


def example_fit():
    if "fit" not in _CACHE:
        _CACHE["fit"] = S.stain_fit_numpy(example())
    return _CACHE["fit"]


def layouts(rgb):
    """The same pixels as: device RGB, and a device RGBA view cut at an odd offset out of a larger image (strided rows)."""
    h, w = rgb.shape[:2]
    yield "rgb", torch.from_numpy(rgb).to(DEV)
    g = torch.Generator().manual_seed(1)
    big = torch.randint(0, 256, (h + 12, w + 9, 4), dtype=torch.uint8, generator=g)
    big[5:5 + h, 3:3 + w, :3] = torch.from_numpy(rgb)
    view = big.to(DEV)[5:5 + h, 3:3 + w]
    assert not view.is_contiguous()
    yield "rgba-view", view


def masks(h, w):
    """No mask; a downsample-4 mask that overhangs the image (4 x 75 = 300 > 298); one that ends inside it (beyond: not allowed)."""
    g = np.random.default_rng(4)
    yield "none", None, 1
    yield "overhang", (g.random(((h + 3) // 4, (w + 3) // 4)) < 0.6).astype(np.uint8), 4
    yield "short", (g.random((h // 4 - 6, w // 4 - 9)) < 0.8).astype(np.uint8), 4


def dev_mask(m):
    return None if m is None else torch.from_numpy(m).to(DEV)


# ------------------------------------------------------------------------------------------------ pass 1: moments
def test_moments_match_the_restatement(passes):
    rgb = example()
    assert rgb.shape == (224, 298, 3)
    for mname, m, ds in masks(224, 298):
        want = S.stain_moments_numpy(rgb, OD, BETA, m, ds)
        assert 2 < want[0] < 224 * 298
        for lname, x in layouts(rgb):
            a = passes.moments(x, dev_mask(m), ds, OD, BETA, None)
            b = passes.moments(x, dev_mask(m), ds, OD, BETA, None)
            assert a.dtype == torch.int64 and np.array_equal(a.cpu().numpy(), want), (mname, lname)
            assert torch.equal(a, b)                               # two runs, the same bits
    # accumulation over bands = the whole, whatever the split
    x = torch.from_numpy(rgb).to(DEV)
    acc = None
    for r0, r1 in ((0, 1), (1, 100), (100, 224)):
        acc = passes.moments(x[r0:r1], None, 1, OD, BETA, acc)
    assert np.array_equal(acc.cpu().numpy(), S.stain_moments_numpy(rgb, OD, BETA))


def test_moments_of_tiny_and_empty_images(model, passes):
    for px in ((120, 40, 130), (240, 240, 240)):
        one = np.array([[px]], dtype=np.uint8)
        got = passes.moments(torch.from_numpy(one).to(DEV), None, 1, OD, BETA, None).cpu().numpy()
        assert np.array_equal(got, S.stain_moments_numpy(one, OD, BETA)) and got[0] == (px[0] == 120)
    glass = (236 + np.random.default_rng(1).integers(-2, 3, (61, 83, 3))).astype(np.uint8)
    got = passes.moments(torch.from_numpy(glass).to(DEV), None, 1, OD, BETA, None).cpu().numpy()
    assert not got.any()                                           # nothing survives beta: n = 0 and every sum 0
    with pytest.raises(ValueError, match="0 pixels"):
        model.stain_fit(glass)
    # a negative sum: od_q < 0 above level 239, kept once beta is low enough
    bright = np.full((9, 7, 3), 250, np.uint8)
    got = passes.moments(torch.from_numpy(bright).to(DEV), None, 1, OD, -1000, None).cpu().numpy()
    assert np.array_equal(got, S.stain_moments_numpy(bright, OD, -1000)) and got[1] < 0 < got[4]


# ------------------------------------------------------------------------------------------------ pass 2: the angle histogram
def test_angle_hist_in_all_quadrants_on_the_axes_and_at_zero(passes):
    """V_q = [[1, 0], [0, 1], [-1, -1]] 2^14: t = 2^14 (od_r - od_b, od_g - od_b), so grey pixels give (0, 0), g == b the x axis,
    r == b the y axis, and random colours all four quadrants.  beta_q = -1000 keeps every pixel."""
    v_q = np.array([[1 << 14, 0], [0, 1 << 14], [-(1 << 14), -(1 << 14)]], dtype=np.int32)
    g = np.random.default_rng(2)
    rgb = g.integers(0, 256, (97, 131, 3), dtype=np.uint8)
    rgb[0, :40] = g.integers(0, 256, (40, 1))                      # grey: t = (0, 0)
    rgb[1, :, 1] = rgb[1, :, 2]                                    # t1 = 0, t0 of either sign
    rgb[2, :, 0] = rgb[2, :, 2]                                    # t0 = 0
    rgb[3, :, 0] = rgb[3, :, 1]                                    # the diagonal t0 = t1
    od = OD[rgb].astype(np.int64)
    t0, t1 = (od[..., 0] - od[..., 2]).ravel(), (od[..., 1] - od[..., 2]).ravel()
    for cond in ((t0 > 0) & (t1 > 0), (t0 < 0) & (t1 > 0), (t0 < 0) & (t1 < 0), (t0 > 0) & (t1 < 0), (t0 == 0) & (t1 == 0),
                 (t0 > 0) & (t1 == 0), (t0 < 0) & (t1 == 0), (t0 == 0) & (t1 > 0), (t0 == 0) & (t1 < 0), (t0 == t1) & (t0 != 0)):
        assert cond.any()
    want = S.stain_angle_hist_numpy(rgb, OD, -1000, v_q)
    assert want.sum() == 97 * 131 and want[S.ANGLE_BINS // 2] >= 40 and want[0] > 0
    for lname, x in layouts(rgb):
        got = passes.angle_hist(x, None, 1, OD, -1000, v_q, None)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), lname
    # added into, in two bands
    x = torch.from_numpy(rgb).to(DEV)
    acc = passes.angle_hist(x[50:], None, 1, OD, -1000, v_q, passes.angle_hist(x[:50], None, 1, OD, -1000, v_q, None))
    assert np.array_equal(acc.cpu().numpy(), want)


def test_angle_and_concentration_hists_of_example_with_its_own_fit(passes):
    rgb, fit = example(), example_fit()
    for mname, m, ds in masks(224, 298):
        want_a = S.stain_angle_hist_numpy(rgb, OD, BETA, fit.v_q, m, ds)
        want_c = S.stain_conc_hist_numpy(rgb, OD, fit.minv_q, m, ds)
        for lname, x in layouts(rgb):
            assert np.array_equal(passes.angle_hist(x, dev_mask(m), ds, OD, BETA, fit.v_q, None).cpu().numpy(), want_a), (mname, lname)
            assert np.array_equal(passes.conc_hist(x, dev_mask(m), ds, OD, fit.minv_q, None).cpu().numpy(), want_c), (mname, lname)
    assert np.array_equal(S.stain_angle_hist_numpy(rgb, OD, BETA, fit.v_q), fit.angle_hist)


# ------------------------------------------------------------------------------------------------ pass 3: concentrations
def test_conc_hist_clamps_at_both_ends(passes):
    """c_0 = 2^20 od_r: bin 8 od_r, past the last bin from od_r = 512 (level <= 211) and below 0 above level 239; c_1 = -c_0."""
    minv_q = np.array([[1 << 20, 0, 0], [-(1 << 20), 0, 0]], dtype=np.int32)
    rgb = np.random.default_rng(6).integers(0, 256, (53, 77, 3), dtype=np.uint8)
    c = OD[rgb[..., 0]].astype(np.int64) << 20 >> S.CONC_SHIFT
    assert (c < 0).any() and (c > S.CONC_BINS - 1).any() and ((c > 0) & (c < S.CONC_BINS - 1)).any()
    want = S.stain_conc_hist_numpy(rgb, OD, minv_q)
    assert want.sum(1).tolist() == [53 * 77] * 2 and want[0, -1] == (c >= S.CONC_BINS - 1).sum() and want[0, 0] == (c <= 0).sum()
    for lname, x in layouts(rgb):
        got = passes.conc_hist(x, None, 1, OD, minv_q, None)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), lname


# ------------------------------------------------------------------------------------------------ the fit as a whole
def test_stain_fit_equals_the_numpy_fit(model):
    rgb = example()
    m = next(mm for name, mm, _ in masks(224, 298) if name == "overhang")
    for tissue in (None, TissueMask(m, 4)):
        want = S.stain_fit_numpy(rgb, tissue)
        for x in (rgb, torch.from_numpy(rgb).to(DEV)):
            got = model.stain_fit(x, tissue)
            for name in ("moments", "v_q", "angle_hist", "minv_q", "conc_hist", "he", "max_c"):
                assert np.array_equal(getattr(got, name), getattr(want, name)), name
    fit = None
    for band in (rgb[:70], rgb[70:71], rgb[71:]):
        fit = model.stain_fit(band, into=fit)
    assert np.array_equal(fit.he, example_fit().he) and np.array_equal(fit.max_c, example_fit().max_c) and fit.n == example_fit().n


# ------------------------------------------------------------------------------------------------ apply
def apply_want(px, tb):
    return S.stain_apply_numpy(px, tb["od_q"], tb["t_q"], tb["exp_lut"], tb["lo"])


def test_apply_small_counts_and_tails(model):
    fit = example_fit()
    tb = fit.tables()
    g = np.random.default_rng(8)
    for n in (1, 3, 4, 5, 4 * 1024 + 1):
        px = g.integers(0, 256, (n, 3), dtype=np.uint8)
        x = torch.from_numpy(px).to(DEV)
        got = model.stain_normalize(x, fit)
        assert got.shape == x.shape and got.device == x.device and np.array_equal(got.cpu().numpy(), apply_want(px, tb)), n
        assert np.array_equal(x.cpu().numpy(), px)                 # out of place: the input is untouched
        # a view that starts 3 bytes into an allocation: not dword aligned, the byte path
        pad = torch.zeros((n + 1, 3), dtype=torch.uint8, device=DEV)
        pad[1:] = x
        out = torch.empty((n, 3), dtype=torch.uint8, device=DEV)
        model._stain_apply(pad[1:], out, model._stain_plan(fit))
        assert np.array_equal(out.cpu().numpy(), apply_want(px, tb)), n
    assert model.stain_normalize(np.zeros((0, 3), np.uint8), fit).shape == (0, 3)


def test_apply_block_in_place_out_of_place_and_single_stains(model):
    fit = example_fit()
    px = np.random.default_rng(9).integers(0, 256, (256, 256, 3), dtype=np.uint8)
    px[0, 0], px[0, 1] = 0, 255
    for keep in (("H", "E"), ("H",), ("E",)):
        want = apply_want(px, fit.tables(keep=keep))
        x = torch.from_numpy(px).to(DEV)
        assert np.array_equal(model.stain_normalize(x, fit, keep=keep).cpu().numpy(), want), keep
        host = model.stain_normalize(px, fit, keep=keep)           # numpy in, numpy out
        assert isinstance(host, np.ndarray) and np.array_equal(host, want)
        out = torch.empty_like(x)
        assert model.stain_normalize(x, fit, keep=keep, out=out) is out and np.array_equal(out.cpu().numpy(), want)
        assert model.stain_normalize(x, fit, keep=keep, out=x) is x and np.array_equal(x.cpu().numpy(), want)          # in place
    rgba = np.concatenate([px, np.full((256, 256, 1), 77, np.uint8)], -1)
    assert np.array_equal(model.stain_normalize(torch.from_numpy(rgba).to(DEV), fit).cpu().numpy(), apply_want(px, fit.tables()))
    other = S.StainTarget(he_ref=[[0.6, 0.1], [0.7, 0.9], [0.3, 0.2]], max_c_ref=[1.5, 1.2], io=255)
    assert np.array_equal(model.stain_normalize(px, fit, target=other), apply_want(px, fit.tables(other)))
    for bad in (px.astype(np.int32), px[..., :2], 3):
        with pytest.raises(ValueError):
            model.stain_normalize(bad, fit)
    with pytest.raises(ValueError):
        model.stain_normalize(px, fit, out=torch.empty((5, 3), dtype=torch.uint8, device=DEV))


def test_apply_saturates_and_refuses_a_steep_matrix(model):
    px = np.random.default_rng(10).integers(0, 256, (333, 3), dtype=np.uint8)
    px[0], px[1] = 0, 255
    x = torch.from_numpy(px).to(DEV)
    od = torch.from_numpy(OD).to(DEV)
    lut_np = S.exp_table(240)
    lut = torch.from_numpy(lut_np).to(DEV)
    for T in (np.full((3, 3), 64.0), np.full((3, 3), -64.0), np.diag([64.0, -64.0, 1.0])):
        t_q = S.quantise(T)
        want = S.stain_apply_numpy(px, OD, t_q, lut_np)
        assert want.min() == 0 and want.max() == 255               # both ends of the exp table
        out = torch.empty_like(x)
        model._stain_apply(x, out, (od, np.ascontiguousarray(t_q), lut, len(lut_np), S.LUT_LO))
        assert np.array_equal(out.cpu().numpy(), want)
    steep = S.quantise(np.diag([1.0, 1.0, 1.0]))
    steep[1, 2] = (64 << 14) + 1
    with pytest.raises(ValueError, match="64"):
        model._stain_apply(x, torch.empty_like(x), (od, steep, lut, len(lut_np), S.LUT_LO))
    with pytest.raises(ValueError, match="overlap"):
        both = torch.zeros((20, 3), dtype=torch.uint8, device=DEV)
        model._stain_apply(both[:12], both[4:16], (od, S.quantise(np.eye(3)), lut, len(lut_np), S.LUT_LO))


def test_apply_one_batch_of_256_tiles(model):
    fit = example_fit()
    tb = fit.tables()
    g = torch.Generator().manual_seed(12)
    tiles = torch.randint(0, 256, (256, 224, 224, 3), dtype=torch.uint8, generator=g)
    got = model.stain_normalize(tiles.to(DEV), fit)
    want_sum, want_weighted = 0, 0
    host = tiles.numpy()
    for i in range(0, 256, 32):                                    # the restatement of the whole batch, 32 tiles at a time
        w = apply_want(host[i:i + 32], tb).astype(np.int64)
        want_sum += int(w.sum())
        want_weighted += int((w.reshape(32, -1).sum(1) * np.arange(i + 1, i + 33)).sum())
    per_tile = got.view(256, -1).sum(1, dtype=torch.int64)
    assert int(per_tile.sum()) == want_sum
    assert int((per_tile * torch.arange(1, 257, device=DEV)).sum()) == want_weighted
    n = 256 * 224 * 224
    idx = torch.arange(0, n, n // (1 << 16))[:1 << 16]             # a strided sample of 2^16 pixels
    sample = got.view(-1, 3)[idx.to(DEV)].cpu().numpy()
    assert np.array_equal(sample, apply_want(host.reshape(-1, 3)[idx.numpy()], tb))


# ------------------------------------------------------------------------------------------------ the flow
FAMILIES = ("he_crops", "stain_field", "background")


@pytest.fixture(scope="module")
def slide():
    """5 x 4 tiles of 224: he_crops / stain_field tiles with a row and a corner of plain glass."""
    g = np.random.default_rng(11)
    pools = {f: synth_tile_family(f, 0, 20, DEV, seed=7011).cpu().numpy() for f in FAMILIES[:2]}
    glass = (236 + g.integers(-2, 3, (224, 224, 3))).astype(np.uint8)
    s = np.zeros((5 * 224, 4 * 224, 3), np.uint8)
    for r in range(5):
        for c in range(4):
            tile = glass if r == 2 or (r == 4 and c < 2) else pools[FAMILIES[(r + c) % 2]][r * 4 + c]
            s[r * 224:(r + 1) * 224, c * 224:(c + 1) * 224] = tile
    return s


DS = 16
SEG = TissueSegmentation(min_area=30, min_hole=16)


def test_encode_region_with_a_stain_fit(model, slide):
    region = torch.from_numpy(slide).to(DEV)
    thumbnail = np.ascontiguousarray(slide[::DS, ::DS])
    mask = model.tissue_mask(thumbnail, DS, SEG)
    fit = model.stain_fit(thumbnail, TissueMask(mask.mask, 1))
    for patch, step in ((224, None), (256, 200)):
        feats, coords = model.encode_region(region, patch, step, tissue=mask, stain=fit)
        plain, coords0 = model.encode_region(region, patch, step, tissue=mask)
        assert torch.equal(coords, coords0) and 0 < len(coords) < 20
        tiles = model.region_patches_uint8(region, coords, patch)
        normalised = model.stain_normalize(tiles, fit)
        assert not torch.equal(normalised, tiles)
        assert torch.equal(feats, model.encode_image_uint8(normalised))
        assert torch.equal(model.region_patches_uint8(region, coords, patch, stain=fit), normalised)
        assert not torch.equal(feats, plain)
        # stain=None is the call without the keyword
        none, coords1 = model.encode_region(region, patch, step, tissue=mask, stain=None)
        assert torch.equal(none, plain) and torch.equal(coords1, coords0)
        assert torch.equal(model.region_patches_uint8(region, coords, patch, stain=None), tiles)
    # attention and rollout: at patch 224 the tiles are cut unresized, so normalising them equals cutting them from the normalised region
    normalised_region = model.stain_normalize(region, fit)
    for method in (model.encode_region_attention, model.encode_region_rollout):
        got = method(region, 224, tissue=mask, stain=fit)
        want = method(normalised_region, 224, tissue=mask)
        plain = method(region, 224, tissue=mask)
        assert all(torch.equal(g, w) for g, w in zip(got, want)) and len(got) == 3
        assert not torch.equal(got[0], plain[0]) and not torch.equal(got[2], plain[2])
        assert all(torch.equal(g, w) for g, w in zip(method(region, 224, tissue=mask, stain=None), plain))
    with pytest.raises(ValueError, match="stain"):
        model.encode_region(region, 224, stain="macenko")


def test_extract_slide_features_with_macenko(model, slide, tmp_path):
    H, W = slide.shape[:2]
    thumbnail = np.ascontiguousarray(slide[::DS, ::DS])

    def read_region(x, y, w, h):
        return slide[y:y + h, x:x + w]

    path = cohort.extract_slide_features(read_region, W, H, "slide_s", str(tmp_path), patch_size=224, band_rows=2, model=model,
                                         thumbnail=thumbnail, thumbnail_downsample=DS, segmentation=SEG, stain="macenko")
    mask = model.tissue_mask(thumbnail, DS, SEG)
    fit = model.stain_fit(thumbnail, TissueMask(mask.mask, 1))
    want, coords = model.encode_region(torch.from_numpy(slide).to(DEV), 224, tissue=mask, stain=fit)
    assert len(coords) > 0 and torch.equal(torch.load(path), want.cpu())
    plain = cohort.extract_slide_features(read_region, W, H, "slide_p", str(tmp_path), patch_size=224, band_rows=2, model=model,
                                          thumbnail=thumbnail, thumbnail_downsample=DS, segmentation=SEG)
    assert torch.equal(torch.load(plain), model.encode_region(torch.from_numpy(slide).to(DEV), 224, tissue=mask)[0].cpu())
    # without a mask: the bands go through encode_region(stain=fit)
    banded = cohort.extract_slide_features(read_region, W, H, "slide_b", str(tmp_path), patch_size=224, band_rows=2, model=model, stain=fit)
    per_band = [model.encode_region(slide[y0:y0 + h], 224, stain=fit, origin=(0, y0))[0] for _, _, y0, h in plan_bands(W, H, 224, None, 2)]
    assert torch.equal(torch.load(banded), torch.cat(per_band))
    unnormalised = cohort.extract_slide_features(read_region, W, H, "slide_u", str(tmp_path), patch_size=224, band_rows=2, model=model)
    assert not torch.equal(torch.load(banded), torch.load(unnormalised))
    with pytest.raises(ValueError, match="thumbnail"):
        cohort.extract_slide_features(read_region, W, H, "slide_x", str(tmp_path), patch_size=224, model=model, stain="macenko")


# ------------------------------------------------------------------------------------------------ what the feature is for
def restain(rgb, scale_h, scale_e):
    """The same tissue stained differently: the concentrations along the generator's two stain vectors scaled in OD space (host)."""
    he = np.stack([np.array(_STAIN_H) / np.linalg.norm(_STAIN_H), np.array(_STAIN_E) / np.linalg.norm(_STAIN_E)], 1)
    od = -np.log((rgb.reshape(-1, 3).astype(np.float64) + 1.0) / 240.0)
    conc = np.linalg.pinv(he) @ od.T
    od = od + (he @ (conc * np.array([[scale_h - 1.0], [scale_e - 1.0]]))).T
    return np.clip(np.rint(240.0 * np.exp(-od) - 1.0), 0, 255).astype(np.uint8).reshape(rgb.shape)


def test_normalisation_removes_a_stain_shift(model):
    """Measured: mean |difference| 14.55 grey levels before, 3.31 after: ratio 0.228.  The bound 1/2 is the floor for "it
    normalises at all", not a quality claim."""
    a = mosaic()
    b = restain(a, 0.6, 1.4)
    before = np.abs(a.astype(np.int64) - b).mean()
    na, nb = (model.stain_normalize(x, model.stain_fit(x)).astype(np.int64) for x in (a, b))
    after = np.abs(na - nb).mean()
    print(f"stain shift: mean |difference| {before:.3f} -> {after:.3f}, ratio {after / before:.4f}")
    assert before > 5 and after < 0.5 * before
