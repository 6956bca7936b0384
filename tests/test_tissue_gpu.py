"""The thumbnail tissue segmentation and the grid on a mask on the MI355X: keep_tissue_median_hist /
keep_tissue_mask / keep_region_grid_mask, KEEPModel.tissue_mask, region_grid / encode_region with a TissueMask and the masked
cohort.extract_slide_features.

Everything is integer arithmetic, so every comparison is exact: the yardsticks are keep_amd.region.tissue_mask_numpy and
mask_grid_numpy (tests/test_tissue.py holds them to scipy and to plain loops), closed-form masks for the shapes that break naive
component labelling, and encode_image_uint8 on host-planned tiles."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel, _lib, cohort
from keep_amd.config import small_shape
from keep_amd.model import _ptr, _stream
from keep_amd.region import (MASK_MODES, TissueMask, TissueRule, TissueSegmentation, grid_shape, mask_grid_numpy, plan_bands, region_grid_numpy,
                             tissue_mask_numpy, tissue_params)
from keep_amd.synth import synth_state_dict, synth_thumbnail, synth_tile_family
from test_tissue import serpentine, spiral

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    m = KEEPModel(precision="strict")
    m.load_state_dict(synth_state_dict(small_shape(2, 2), seed=5), strict=True)
    return m.to(DEV).eval()


_THUMBS = {}


def thumb(name):
    if name not in _THUMBS:
        if name == "synthetic":
            _THUMBS[name] = synth_thumbnail()                    # 384 x 512
        else:
            from PIL import Image
            _THUMBS[name] = np.array(Image.open(os.path.join(ROOT, "tests", "golden", "example.tif")))[..., :3].copy()
    return _THUMBS[name]


_RESTATED = {}


def restated(name, p):
    """tissue_mask_numpy of a fixture, once per parameter set -> (mask, threshold, stages)."""
    key = (name, p)
    if key not in _RESTATED:
        st = {}
        mask, t = tissue_mask_numpy(thumb(name), p, st)
        _RESTATED[key] = (mask, t, st)
    return _RESTATED[key]


AREAS = [(16, 100), (200, 400), (64, 400)]
PARAMS = [TissueSegmentation(mthresh=k, use_otsu=o, close=c, min_hole=mh, min_area=ma)
          for k, o, c, (mh, ma) in itertools.product((1, 3, 7, 15), (False, True), (0, 3, 4), AREAS)]


def pid(p):
    return f"k{p.mthresh}-{'otsu' if p.use_otsu else 'fixed'}-c{p.close}-h{p.min_hole}-a{p.min_area}"


def layouts(rgb):
    """The same pixels as: device RGB, host RGB, and a device RGBA view cut at an odd offset out of a larger image (strided rows)."""
    h, w = rgb.shape[:2]
    yield "device-rgb", torch.from_numpy(rgb).to(DEV)
    yield "host-rgb", rgb
    g = torch.Generator().manual_seed(1)
    big = torch.randint(0, 256, (h + 12, w + 9, 4), dtype=torch.uint8, generator=g)
    big[5:5 + h, 3:3 + w, :3] = torch.from_numpy(rgb)
    view = big.to(DEV)[5:5 + h, 3:3 + w]
    assert not view.is_contiguous()
    yield "device-rgba-view", view
    yield "host-rgba-view", big.numpy()[5:5 + h, 3:3 + w]


# ------------------------------------------------------------------------------------------------ the segmentation
@pytest.mark.parametrize("name", ["synthetic", "example"])
@pytest.mark.parametrize("p", PARAMS, ids=pid)
def test_mask_matches_the_restatement(model, name, p):
    want, t, st = restated(name, p)
    for layout, x in layouts(thumb(name)):
        got = model.tissue_mask(x, 16, p)
        assert isinstance(got, TissueMask) and got.mask.device.type == "cuda" and got.mask.dtype == torch.uint8
        assert (got.downsample, got.mode) == (16, "four_pt")
        assert np.array_equal(model.last_tissue_median.cpu().numpy(), st["median"]), layout
        assert np.array_equal(model.last_tissue_hist.cpu().numpy().astype(np.int64), st["hist"]), layout
        assert got.threshold == t, layout
        assert np.array_equal(got.mask.cpu().numpy(), want), layout
    model.check_errors(wait=True)


def test_every_stage_changes_something_on_the_fixtures():
    """Keeps the test above from passing vacuously: over its parametrisation the median, the closing, the hole filling (filled AND
    kept in one case) and the area filter (dropped AND kept in one case) all act, and no final mask is trivial."""
    seen = dict(median=False, closing=False, holes=False, components=False)
    for name in ("synthetic", "example"):
        nontrivial = 0
        for p in PARAMS:
            mask, _, st = restated(name, p)
            nontrivial += 0 < mask.sum() < mask.size
            seen["median"] |= bool((st["median"] != st["saturation"]).any())
            seen["closing"] |= bool((st["closed"] != st["thresholded"]).any())
            seen["holes"] |= st["holes_filled"] >= 1 and st["holes_kept"] >= 1
            seen["components"] |= 1 <= st["components_kept"] < st["components"]
        assert nontrivial >= len(PARAMS) // 2, (name, nontrivial)      # (the H & E crop is all tissue at the fixed threshold)
    assert all(seen.values()), seen
    _, t, st = restated("example", TissueSegmentation(use_otsu=True, min_hole=64, min_area=400))
    assert (t, st["holes_filled"], st["components"], st["components_kept"]) == (69, 2, 107, 11)
    _, t, st = restated("synthetic", TissueSegmentation(use_otsu=True, min_hole=200, min_area=400))
    assert (t, st["holes_filled"], st["holes_kept"]) == (54, 3, 2)


def as_thumbnail(pattern):
    """A {0,1} pattern as a thumbnail whose thresholded saturation is the pattern (with the median and the closing off)."""
    rgb = np.full(pattern.shape + (3,), 200, np.uint8)
    rgb[pattern != 0] = (220, 30, 120)
    return rgb


def label_only(min_hole, min_area):
    return TissueSegmentation(mthresh=1, close=0, min_hole=min_hole, min_area=min_area)


def shapes():
    g = np.random.default_rng(0)
    yield "1x1-set", np.ones((1, 1), np.uint8)
    yield "1x1-clear", np.zeros((1, 1), np.uint8)
    yield "1x300", (g.random((1, 300)) < 0.7).astype(np.uint8)
    yield "300x1", (g.random((300, 1)) < 0.7).astype(np.uint8)
    yield "off-tile-noise", (g.random((67, 131)) < 0.55).astype(np.uint8)
    yield "sparse-noise", (g.random((203, 317)) < 0.35).astype(np.uint8)
    yield "all-0", np.zeros((70, 150), np.uint8)
    yield "all-1", np.ones((70, 150), np.uint8)
    yield "checkerboard", (np.indices((130, 197)).sum(0) % 2).astype(np.uint8)
    yield "spiral", spiral(301)
    yield "serpentine", serpentine(257, 1000)
    frame = np.zeros((90, 200), np.uint8)
    frame[3, 3:-3] = frame[-4, 3:-3] = frame[3:-3, 3] = frame[3:-3, -4] = 1
    yield "frame", frame
    rings = np.zeros((140, 140), np.uint8)
    rings[10:130, 10:130] = 1
    rings[30:110, 30:110] = 0                                     # a hole ...
    rings[50:90, 50:90] = 1                                       # ... with an island ...
    rings[62:70, 62:70] = 0                                       # ... that has a hole of its own
    yield "nested-rings", rings
    diag = np.zeros((12, 200), np.uint8)
    diag[0:4, 0:64] = 1                                           # two blocks that meet only at the corner of a 64 x 4 tile
    diag[4:8, 64:128] = 1
    diag[8:12, 0:64] = 1                                          # and one that touches neither (a clear row between would join by 8)
    diag[8, 0:64] = 0
    yield "diagonal-at-tile-corner", diag


@pytest.mark.parametrize("name,pattern", list(shapes()), ids=[n for n, _ in shapes()])
def test_shapes_that_break_naive_labelling(model, name, pattern):
    rgb = as_thumbnail(pattern)
    for min_hole, min_area in ((1, 1), (50, 50), (10 ** 9, 0), (0, 10 ** 9), (3000, 300), (1 << 40, 1 << 40)):
        p = label_only(min_hole, min_area)
        want, _ = tissue_mask_numpy(rgb, p)
        got = model.tissue_mask(torch.from_numpy(rgb).to(DEV), 1, p).mask.cpu().numpy()
        assert np.array_equal(got, want), (name, min_hole, min_area)
    model.check_errors(wait=True)
    # what the restatement must have said, in closed form
    n = int(pattern.sum())
    keep_all, _ = tissue_mask_numpy(rgb, label_only(0, 0))
    assert np.array_equal(keep_all, pattern)
    if name == "checkerboard":                                    # one 8-component; every inner background pixel is a 1-pixel hole
        filled, _ = tissue_mask_numpy(rgb, label_only(1, n - 1))
        inner = np.zeros_like(pattern)
        inner[1:-1, 1:-1] = 1
        assert np.array_equal(filled, pattern | inner)
        assert not tissue_mask_numpy(rgb, label_only(0, n))[0].any()
    if name in ("spiral", "serpentine"):                          # one component however long the path
        assert np.array_equal(tissue_mask_numpy(rgb, label_only(0, n - 1))[0], pattern)
        assert not tissue_mask_numpy(rgb, label_only(0, n))[0].any()
    if name == "frame":                                           # one hole = everything inside
        inside = 82 * 192
        assert tissue_mask_numpy(rgb, label_only(inside, 0))[0].sum() == n + inside
        assert tissue_mask_numpy(rgb, label_only(inside - 1, 0))[0].sum() == n
    if name == "nested-rings":
        ring, island, hole, inner = 120 * 120 - 80 * 80, 40 * 40 - 8 * 8, 80 * 80 - 40 * 40, 8 * 8
        assert tissue_mask_numpy(rgb, label_only(0, island))[0].sum() == ring           # the island with its hole is too small ...
        assert tissue_mask_numpy(rgb, label_only(0, island - 1))[0].sum() == ring + island
        assert tissue_mask_numpy(rgb, label_only(inner, island))[0].sum() == ring + island + inner     # ... but not once it is filled
        assert tissue_mask_numpy(rgb, label_only(inner, island + inner))[0].sum() == ring
        assert tissue_mask_numpy(rgb, label_only(hole, 0))[0].sum() == 120 * 120       # both holes filled
    if name == "diagonal-at-tile-corner":
        assert tissue_mask_numpy(rgb, label_only(0, 2 * 256 - 1))[0].sum() == 2 * 256  # the two blocks are one component of 512
        assert tissue_mask_numpy(rgb, label_only(0, 2 * 256))[0].sum() == 0


def test_4096_square_against_a_closed_form(model):
    """16.8 M pixels: a one-pixel frame around the image (its inside is ONE hole of 16 M pixels, too large to fill), and in every 64 x 64
    cell either a 40 x 40 square with a hole (10 x 10: filled; 20 x 20 in every third column: kept) or a 6 x 6 speck (dropped)."""
    n, cell = 4096, 64
    cy, cx = np.indices((n // cell, n // cell))
    big, wide = (cy + cx) % 2 == 0, cx % 3 == 0
    tile_square = np.zeros((cell, cell), np.uint8)
    tile_square[12:52, 12:52] = 1
    small_hole, wide_hole, speck = tile_square.copy(), tile_square.copy(), np.zeros((cell, cell), np.uint8)
    small_hole[27:37, 27:37] = 0
    wide_hole[22:42, 22:42] = 0
    speck[30:36, 30:36] = 1

    def lay(a, b, c):                                             # per cell: big & ~wide -> a, big & wide -> b, else c
        return (np.kron(big & ~wide, a) + np.kron(big & wide, b) + np.kron(~big, c)).astype(np.uint8)
    pattern, want = lay(small_hole, wide_hole, speck), lay(tile_square, wide_hole, np.zeros_like(speck))
    for img in (pattern, want):
        img[0, :] = img[-1, :] = img[:, 0] = img[:, -1] = 1
    assert (pattern != want).any() and pattern.shape == (n, n)
    x = torch.from_numpy(as_thumbnail(pattern)).to(DEV)
    got = model.tissue_mask(x, 1, label_only(150, 100)).mask
    model.check_errors(wait=True)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert torch.equal(got, model.tissue_mask(x, 1, label_only(150, 100)).mask)


def test_the_same_input_twice_gives_the_same_mask(model):
    x = torch.from_numpy(thumb("synthetic")).to(DEV)
    noise = torch.from_numpy(as_thumbnail((np.random.default_rng(5).random((1500, 1700)) < 0.58).astype(np.uint8))).to(DEV)
    for inp, p in ((x, TissueSegmentation(min_hole=200)), (noise, label_only(40, 200)), (noise, TissueSegmentation(mthresh=3, use_otsu=True))):
        a = model.tissue_mask(inp, 8, p)
        b = model.tissue_mask(inp, 8, p)
        assert torch.equal(a.mask, b.mask) and a.threshold == b.threshold
        assert 0 < int(a.mask.sum()) < a.mask.numel()
    want, _ = tissue_mask_numpy(noise.cpu().numpy(), label_only(40, 200))      # a percolating noise field: thousands of merges per component
    assert np.array_equal(model.tissue_mask(noise, 8, label_only(40, 200)).mask.cpu().numpy(), want)
    model.check_errors(wait=True)


# ------------------------------------------------------------------------------------------------ the grid on a mask
FAMILIES = ("he_crops", "stain_field", "background", "half")


def mosaic(rows, cols, seed=11):
    """tests/test_region_gpu.py's mosaic: uint8 [rows*224, cols*224, 3], a synth_tile_family tile per cell."""
    g = np.random.default_rng(seed)
    fam = g.choice(len(FAMILIES), size=(rows, cols), p=[0.25, 0.25, 0.35, 0.15])
    pools = {f: synth_tile_family(f, 0, rows * cols, DEV, seed=7000 + seed).cpu() for f in FAMILIES}
    out = np.zeros((rows * 224, cols * 224, 3), np.uint8)
    for r in range(rows):
        for c in range(cols):
            out[r * 224:(r + 1) * 224, c * 224:(c + 1) * 224] = pools[FAMILIES[fam[r, c]]][r * cols + c].numpy()
    return out


@pytest.fixture(scope="module")
def slide():
    """10 x 7 tiles of 224; tile rows 4 and 5 and the three left tile columns of rows 6..9 are plain glass (grey, saturation <= 5)."""
    s = mosaic(10, 7)
    glass = (236 + np.random.default_rng(1).integers(-2, 3, (224, 224, 3))).astype(np.uint8)
    for r in range(10):
        for c in range(7):
            if r in (4, 5) or (r >= 6 and c < 3):
                s[r * 224:(r + 1) * 224, c * 224:(c + 1) * 224] = glass
    return s


DS = 16
SEG = TissueSegmentation(min_area=30, min_hole=16)


@pytest.fixture(scope="module")
def slide_mask(model, slide):
    thumbnail = np.ascontiguousarray(slide[::DS, ::DS])           # the slide reduced by an integer factor
    mask = model.tissue_mask(thumbnail, DS, SEG)
    want, _ = tissue_mask_numpy(thumbnail, SEG)
    assert np.array_equal(mask.mask.cpu().numpy(), want) and 0 < want.sum() < want.size
    return mask


@pytest.mark.parametrize("mode", MASK_MODES)
@pytest.mark.parametrize("patch,step", [(224, None), (256, 131), (512, 200), (16, 16)])
def test_region_grid_on_a_mask(model, slide, slide_mask, mode, patch, step):
    H, W = slide.shape[:2]
    mask_np = slide_mask.mask.cpu().numpy()
    region = torch.from_numpy(slide).to(DEV)
    counts = []
    for origin, (y0, x0), scale in (((0, 0), (0, 0), 1), ((448, 224), (224, 448), 4), ((-100, 37), (0, 0), 2)):
        view = region[y0:, x0:]                                   # origin = (x, y) of the view's first pixel in the level
        h, w = view.shape[:2]
        want = (mask_grid_numpy(mask_np, DS, h, w, patch, step, origin, mode) + np.asarray(origin)) * scale
        for tissue in (TissueMask(slide_mask.mask, DS, mode), TissueMask(mask_np.astype(bool), DS, mode),
                       TissueMask(slide_mask.mask.cpu() * 255, DS, mode)):                 # the engine's, and two caller-made ones
            got = model.region_grid(view, patch, step, tissue, origin=origin, coord_scale=scale)
            assert got.device.type == "cuda" and got.dtype == torch.int64
            assert np.array_equal(got.cpu().numpy(), want), (origin, mode)
        host = model.region_grid(slide[y0:, x0:], patch, step, TissueMask(mask_np, DS, mode), origin=origin, coord_scale=scale)
        assert host.device.type == "cpu" and np.array_equal(host.numpy(), want)
        gy, gx = grid_shape(h, w, patch, step or patch)
        counts.append((len(want), gy * gx))
    assert any(0 < n < full for n, full in counts)
    # a mask smaller than the region: the cells beyond it are not tissue
    part = TissueMask(mask_np[:40, :50], DS, mode)
    want = mask_grid_numpy(mask_np[:40, :50], DS, H, W, patch, step, (0, 0), mode)
    assert np.array_equal(model.region_grid(region, patch, step, part).cpu().numpy(), want)
    assert len(want) == 0 or (want[:, 0].max() < 50 * DS and want[:, 1].max() < 40 * DS)


def test_every_earlier_tissue_form_gives_what_it_gave(model, slide):
    region = slide[5:, 3:]
    dev = torch.from_numpy(np.ascontiguousarray(region)).to(DEV)
    rule = TissueRule(sat_min=20, min_fraction=0.25)
    for tissue in (None, False, True, rule, (60, 0.05), [0, 0.9], dict(sat_min=30, min_fraction=0.5)):
        for patch, step in ((224, None), (256, 131)):
            sat_min, min_pixels = tissue_params(tissue, patch)
            want = region_grid_numpy(region, patch, step, sat_min, min_pixels)
            assert np.array_equal(model.region_grid(dev, patch, step, tissue).cpu().numpy(), want), tissue
    for bad in ("four_pt", 3, (1, 2, 3), np.ones((4, 4), bool)):
        with pytest.raises(ValueError):
            model.region_grid(dev, 224, None, bad)


def test_encode_region_on_a_mask(model, slide, slide_mask):
    region = torch.from_numpy(slide).to(DEV)
    for patch, step, origin, scale in ((224, None, (0, 0), 1), (256, 200, (0, 0), 2)):
        feats, coords = model.encode_region(region, patch, step, slide_mask, origin=origin, coord_scale=scale)
        want = (mask_grid_numpy(slide_mask.mask.cpu().numpy(), DS, *slide.shape[:2], patch, step, origin, slide_mask.mode) + np.asarray(origin)) * scale
        assert np.array_equal(coords.cpu().numpy(), want) and 0 < len(want) <= 256       # one batch on both sides
        tiles = model.region_patches_uint8(region, coords, patch, origin=origin, coord_scale=scale)
        assert torch.equal(feats, model.encode_image_uint8(tiles))
        x, y = (int(v) // scale for v in coords[len(coords) // 2])
        if patch == 224:
            assert np.array_equal(tiles[len(coords) // 2].cpu().numpy(), slide[y:y + 224, x:x + 224])


# ------------------------------------------------------------------------------------------------ slide -> feature file, by mask
@pytest.mark.parametrize("how,patch,band_rows", [("mask", 224, 2), ("thumbnail", 224, 2), ("mask", 64, 3)])
def test_extract_slide_features_on_a_mask(model, slide, slide_mask, tmp_path, monkeypatch, how, patch, band_rows):
    """patch 64: several hundred kept cells, so the tiles of many bands are encoded in more than one batch of 256."""
    H, W = slide.shape[:2]
    step, scale = None, 2
    reads = []

    def read_region(x, y, w, h):
        reads.append((x, y, w, h))
        return slide[y:y + h, x:x + w]

    saved = {}
    real_save = cohort.save_slide_features

    def spy(data_source, slide_id, features, coords=None, use_h5=False):
        saved["coords"] = np.asarray(coords)
        return real_save(data_source, slide_id, features, coords, use_h5)

    monkeypatch.setattr(cohort, "save_slide_features", spy)
    kw = dict(tissue=slide_mask) if how == "mask" else \
        dict(thumbnail=np.ascontiguousarray(slide[::DS, ::DS]), thumbnail_downsample=DS, segmentation=SEG)
    path = cohort.extract_slide_features(read_region, W, H, "slide_m", str(tmp_path), patch_size=patch, step=step, band_rows=band_rows,
                                         coord_scale=scale, model=model, **kw)
    feats = torch.load(path)
    f1, c1 = model.encode_region(torch.from_numpy(slide).to(DEV), patch, step, slide_mask, coord_scale=scale)
    assert len(c1) > (256 if patch == 64 else 0) and np.array_equal(saved["coords"], c1.cpu().numpy())
    assert torch.equal(feats, f1.cpu())
    # what was read: per band with kept cells, its rows and the columns [min kept x, max kept x + patch); nothing else
    cells = mask_grid_numpy(slide_mask.mask.cpu().numpy(), DS, H, W, patch, step, (0, 0), slide_mask.mode)
    want_reads, empty = [], 0
    for r0, r1, y0, h in plan_bands(W, H, patch, step, band_rows):
        xs = cells[(cells[:, 1] >= r0 * patch) & (cells[:, 1] < r1 * patch), 0]
        if len(xs):
            want_reads.append((int(xs.min()), y0, int(xs.max()) + patch - int(xs.min()), h))
        else:
            empty += 1
    assert reads == want_reads
    assert empty >= 1 and any(x0 > 0 for x0, _, _, _ in reads) and any(w < W for _, _, w, _ in reads)      # the fixture's conditions
    assert sum(w * h for _, _, w, h in reads) < W * H


# ------------------------------------------------------------------------------------------------ the C ABI's argument checks
def test_abi_rejects_bad_arguments(model):
    lib, h, st = _lib.load(), model._handle, _stream(torch.device(DEV))
    H, W = 60, 80
    thumbnail = torch.zeros((H, W, 4), dtype=torch.uint8, device=DEV)
    med = torch.zeros((H, W), dtype=torch.uint8, device=DEV)
    mask = torch.zeros((H, W), dtype=torch.uint8, device=DEV)
    hist = torch.zeros(256, dtype=torch.int32, device=DEV)
    cells = torch.zeros((4096, 2), dtype=torch.int32, device=DEV)
    n = torch.zeros(1, dtype=torch.int64, device=DEV)
    null = C.c_void_p(0)

    def median(t=_ptr(thumbnail), Hh=H, Ww=W, row=W * 4, ps=4, k=7, med_p=_ptr(med), hist_p=_ptr(hist)):
        return lib.keep_tissue_median_hist(h, t, Hh, Ww, row, ps, k, med_p, hist_p, st)

    assert median() == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert int(hist[0]) == H * W and int(hist.sum()) == H * W
    for kw in [dict(t=null), dict(Hh=0), dict(Ww=0), dict(Hh=1 << 16, Ww=1 << 15), dict(row=W * 4 - 1), dict(ps=3, row=W * 3 - 1), dict(ps=2),
               dict(ps=5), dict(k=0), dict(k=4), dict(k=17), dict(k=-3), dict(med_p=null), dict(hist_p=null)]:
        assert median(**kw) == _lib.KEEP_EINVAL, kw
        assert lib.keep_last_error(h)

    def segment(med_p=_ptr(med), Hh=H, Ww=W, t=8, close=4, min_hole=16, min_area=100, mask_p=_ptr(mask)):
        return lib.keep_tissue_mask(h, med_p, Hh, Ww, t, close, min_hole, min_area, mask_p, st)

    assert segment() == _lib.KEEP_OK
    for kw in [dict(med_p=null), dict(mask_p=null), dict(mask_p=_ptr(med)), dict(Hh=0), dict(Ww=-1), dict(Hh=1 << 16, Ww=1 << 15), dict(t=-1),
               dict(t=256), dict(close=-1), dict(close=32), dict(min_hole=-1), dict(min_area=-1)]:
        assert segment(**kw) == _lib.KEEP_EINVAL, kw
        assert lib.keep_last_error(h)

    def grid(mask_p=_ptr(mask), mh=H, mw=W, ds=16, Hh=H * 16, Ww=W * 16, patch=32, step=32, ox=0, oy=0, mode=0, cell_p=_ptr(cells), n_p=_ptr(n)):
        return lib.keep_region_grid_mask(h, mask_p, mh, mw, ds, Hh, Ww, patch, step, ox, oy, mode, cell_p, n_p, st)

    mask.fill_(1)
    assert grid() == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert int(n.item()) == (H * 16 // 32) * (W * 16 // 32) <= cells.shape[0]
    for kw in [dict(mask_p=null), dict(mh=0), dict(mw=0), dict(ds=0), dict(ds=-4), dict(Hh=0), dict(Ww=0), dict(patch=15), dict(step=0),
               dict(step=-3), dict(mode=-1), dict(mode=3), dict(ox=1 << 41), dict(oy=-(1 << 41)), dict(cell_p=null), dict(n_p=null)]:
        assert grid(**kw) == _lib.KEEP_EINVAL, kw
        assert lib.keep_last_error(h)
    n.fill_(7)
    assert grid(patch=H * 16 + 1) == _lib.KEEP_OK                 # a region smaller than one patch: N = 0, no error
    torch.cuda.synchronize()
    assert int(n.item()) == 0
    for call in (lambda: lib.keep_tissue_median_hist(None, _ptr(thumbnail), H, W, W * 4, 4, 7, _ptr(med), _ptr(hist), st),
                 lambda: lib.keep_tissue_mask(None, _ptr(med), H, W, 8, 4, 16, 100, _ptr(mask), st),
                 lambda: lib.keep_region_grid_mask(None, _ptr(mask), H, W, 16, H * 16, W * 16, 32, 32, 0, 0, 0, _ptr(cells), _ptr(n), st)):
        assert call() == _lib.KEEP_EINVAL
    with pytest.raises(ValueError, match="ksize|mthresh"):
        lib_rc = lib.keep_tissue_median_hist(h, _ptr(thumbnail), H, W, W * 4, 4, 6, _ptr(med), _ptr(hist), st)
        _lib.check(h, lib_rc, "tissue_median_hist")
