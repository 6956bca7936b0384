"""Tile quality control on the MI355X: keep_region_quality / keep_pen_mask, KEEPModel.tile_quality /
region_quality / pen_mask and the ``quality=`` keyword of region_grid / encode_region.

Everything on the device is integer arithmetic, so every comparison is exact: the yardsticks are keep_amd.quality's numpy
restatements (tests/test_quality.py holds them to a per-pixel loop) and encode_image_uint8 on the kept tiles cut by hand."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from keep_amd import KEEPModel, QualityGate, QualityRules, TileQuality
from keep_amd import quality as Q
from keep_amd.config import small_shape
from keep_amd.region import TissueMask, TissueRule
from keep_amd.synth import synth_state_dict, synth_tile_family

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def model():
    m = KEEPModel(precision="strict")
    m.load_state_dict(synth_state_dict(small_shape(2, 2), seed=5), strict=True)
    return m.to(DEV).eval()


def scene(h, w, seed):
    """uint8 [h,w,3]: uniform noise (mostly tissue, some of every other class) with rectangles of glass, dark and the default inks."""
    g = np.random.default_rng(seed)
    a = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
    fills = [lambda n: g.integers(215, 256, (n, 3)), lambda n: g.integers(0, 46, (n, 3)),
             lambda n: np.stack([g.integers(0, 70, n), g.integers(0, 150, n), g.integers(140, 256, n)], 1),        # around the blue boxes
             lambda n: np.stack([g.integers(160, 256, n), g.integers(0, 80, n), g.integers(0, 80, n)], 1),         # around the red box
             lambda n: g.integers(35, 100, (n, 3))]                                                                # around the black box
    for k, fill in enumerate(fills):
        y0, x0 = (k * h) // 7, (k * w) // 6
        hh, ww = max(1, h // 4), max(1, w // 3)
        blk = a[y0:y0 + hh, x0:x0 + ww]
        blk[...] = fill(blk.shape[0] * blk.shape[1]).reshape(blk.shape).astype(np.uint8)
    return a


def layouts(rgb, channels, pad):
    """The pixels on the device as [h,w,channels]: pad = 0 contiguous, else a view cut at (3, 2) out of an image pad columns wider."""
    h, w = rgb.shape[:2]
    g = torch.Generator().manual_seed(3)
    big = torch.randint(0, 256, (h + (7 if pad else 0), w + pad, channels), dtype=torch.uint8, generator=g)
    y, x = (3, 2) if pad else (0, 0)
    big[y:y + h, x:x + w, :3] = torch.from_numpy(rgb)
    view = big.to(DEV)[y:y + h, x:x + w]
    assert view.is_contiguous() == (pad == 0)
    return view


def cells_for(H, W, patch):
    """x offsets 0..3 (every byte alignment of a cell's first pixel), steps of patch / 2 (overlap), flush right and bottom."""
    s = max(1, patch // 2)
    xs = sorted({x for x in (0, 1, 2, 3, s, 2 * s + 1, W - patch) if 0 <= x <= W - patch})
    ys = sorted({y for y in (0, s, H - patch) if 0 <= y <= H - patch})
    return np.array([(x, y) for y in ys for x in xs], np.int64)


# ------------------------------------------------------------------------------------------------ the table
# 3: one interior pixel; 225, 257: tails of the 4-pixel groups; 224 / 225 / 257: 4 / 4 / 5 bands of rows, 16: one band
@pytest.mark.parametrize("patch", [1, 2, 3, 16, 224, 225, 257])
@pytest.mark.parametrize("channels", [3, 4])
def test_table_matches_the_restatement(model, patch, channels):
    H, W = 2 * patch + 5, 2 * patch + 6
    rgb = scene(H, W, 100 + patch)
    cells = cells_for(H, W, patch)
    assert len(cells) >= 6 and (cells[:, 0] + patch == W).any() and (cells[:, 1] + patch == H).any()
    want = Q.tile_quality_numpy(rgb, cells, patch)
    assert (want[:, :7].sum(axis=1) <= patch * patch).all() and want[:, :7].sum() > 0
    if patch >= 16:
        assert (want[:, :7] > 0).any(axis=0).all()            # every class occurs
    for pad in (5, 0, 6):                                       # row strides of 3 (W + 5) bytes (odd: every row has its own alignment), W C, and even
        x = layouts(rgb, channels, pad)
        q = model.region_quality(x, torch.from_numpy(cells), patch)
        assert isinstance(q, TileQuality) and q.patch == patch and q.n == len(cells) and q.table.device.type == "cuda"
        assert np.array_equal(q.to_numpy(), want), (patch, channels, pad)
    assert torch.equal(model.region_quality(x, torch.from_numpy(cells), patch).table, q.table)        # two runs, the same bits


def test_many_cells_one_cell_no_cell(model):
    rgb = scene(100, 120, 7)
    g = np.random.default_rng(8)
    cells = np.stack([g.integers(0, 120 - 16 + 1, 300), g.integers(0, 100 - 16 + 1, 300)], 1)
    x = layouts(rgb, 3, 5)
    rules = QualityRules(sat_min=60, white_min=200, dark_max=60, pen=((2, 0, 90, 0, 255, 0, 255), (0, 50, 200, 100, 255, 0, 255), (0, 0, 255, 0, 30, 0, 255)))
    for r in (None, rules, QualityRules(pen=())):
        want = Q.tile_quality_numpy(rgb, cells, 16, r)
        assert np.array_equal(model.region_quality(x, cells, 16, rules=r).to_numpy(), want)
        assert np.array_equal(model.region_quality(x, cells[:1], 16, rules=r).to_numpy(), want[:1])
    assert want[:, :4].sum() == 0                              # the last rules: ink off
    q = model.region_quality(x, np.zeros((0, 2), np.int64), 16)
    assert q.n == 0 and q.table.shape == (0, 12) and q.focus().shape == (0,)
    # origin and coord_scale as region_patches_uint8 takes them; a coord outside the region is its ValueError
    got = model.region_quality(x, (cells + np.array([40, 30])) * 2, 16, origin=(40, 30), coord_scale=2).to_numpy()
    assert np.array_equal(got, Q.tile_quality_numpy(rgb, cells, 16))
    for bad in ([[120 - 15, 0]], [[0, 100 - 15]], [[-1, 0]], [[2 ** 40, 0]]):
        with pytest.raises(ValueError, match="cell"):
            model.region_quality(x, torch.tensor(bad), 16)
    with pytest.raises(ValueError, match="patch"):
        model.region_quality(x, cells, 1025)


def test_checkerboard_of_1024_is_the_overflow_case(model):
    yy, xx = np.mgrid[0:1024, 0:1024]
    tile = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)[None]
    want = Q.tile_quality_numpy(tile[0], [(0, 0)], 1024)
    assert want[0, 8] == 1022 * 1022 * 1020 * 1020 > 2 ** 39 and want[0, 4] == want[0, 5] == 1024 * 512
    q = model.tile_quality(torch.from_numpy(tile).to(DEV))
    assert np.array_equal(q.to_numpy(), want)
    assert q.focus().item() == pytest.approx(1020.0 ** 2, rel=1e-12)       # the mean of L is 0 on an even interior


def test_all_glass_tile(model):
    q = model.tile_quality(np.full((1, 64, 64, 3), 240, np.uint8))
    t = q.to_numpy()[0]
    assert t[5] == 64 * 64 and t[9] == 0 and not t[[0, 1, 2, 3, 4, 6, 7, 8, 10, 11]].any()
    assert torch.isnan(q.focus(tissue=True)).all() and q.focus().item() == 0.0 and q.glass_fraction().item() == 1.0
    assert not QualityGate(min_focus=1.0).keep(q).item() and QualityGate().keep(q).item()


def test_tile_batch_equals_the_tiles_laid_into_a_region(model):
    tiles = synth_tile_family("he_crops", 0, 5, "cpu", seed=41).numpy()
    tiles[1, 50:120, 30:200] = (20, 40, 220)                    # default-table blue ink
    tiles[3, :100] = 250
    q = model.tile_quality(tiles)
    assert q.n == 5 and q.patch == 224
    region = np.zeros((2 * 224 + 9, 3 * 224 + 2, 3), np.uint8)
    cells = np.array([(1, 0), (225, 3), (450, 9), (2, 230), (300, 233)])
    for t, (x, y) in zip(tiles, cells):
        region[y:y + 224, x:x + 224] = t
    r = model.region_quality(torch.from_numpy(region).to(DEV), cells, 224)
    assert torch.equal(q.table, r.table)
    assert np.array_equal(q.to_numpy(), Q.tile_quality_numpy(tiles.reshape(-1, 224, 3), [(0, 224 * i) for i in range(5)], 224))
    assert q.pen_count("blue")[1].item() >= 70 * 170 and q.pen_fraction()[1] >= q.pen_fraction(0)[1]
    assert q.pen_fraction("blue")[1].item() == q.pen_count(0)[1].item() / 224 ** 2 and q.glass_fraction()[3].item() >= 100 / 224
    # a host tensor and a device tensor give the same table; RGBA tiles too
    rgba = np.concatenate([tiles, np.full(tiles.shape[:3] + (1,), 7, np.uint8)], axis=3)
    assert torch.equal(model.tile_quality(torch.from_numpy(rgba).to(DEV)).table, q.table)
    flat = torch.zeros(1 + rgba.size, dtype=torch.uint8, device=DEV)                       # RGBA pixels that start on an odd address: the byte path
    flat[1:] = torch.from_numpy(rgba).to(DEV).flatten()
    assert flat[1:].data_ptr() % 4 and torch.equal(model.tile_quality(flat[1:].view(rgba.shape)).table, q.table)


@pytest.mark.parametrize("channels", [3, 4])
def test_pen_mask_matches_the_restatement(model, channels):
    rgb = scene(37, 53, 21)
    want = Q.pen_mask_numpy(rgb)
    assert set(np.unique(want)) == set(range(8))
    for pad in (5, 0):
        got = model.pen_mask(layouts(rgb, channels, pad))
        assert got.dtype == torch.uint8 and got.device.type == "cuda" and np.array_equal(got.cpu().numpy(), want), (channels, pad)
    assert np.array_equal(model.pen_mask(rgb), want)            # numpy in, numpy out
    rules = QualityRules(pen=())
    assert np.array_equal(model.pen_mask(rgb, rules), Q.pen_mask_numpy(rgb, rules))
    # out of a tissue mask, on the device
    m = TissueMask(torch.ones((37, 53), dtype=torch.uint8, device=DEV), 4)
    e = Q.exclude(m, model.pen_mask(torch.from_numpy(rgb).to(DEV)), radius=2, model=model)
    assert torch.equal(e.mask.cpu(), Q.exclude(TissueMask(np.ones((37, 53), np.uint8), 4), want, radius=2).mask) and e.downsample == 4


# ------------------------------------------------------------------------------------------------ the gate
_CACHE = {}


def gate_region():
    """3 x 3 cells of 224 of he_crops tiles: cell (1, 0) under blue ink, cell (1, 1) blurred heavily, cell (0, 2) dark."""
    if "region" not in _CACHE:
        t = synth_tile_family("he_crops", 0, 9, "cpu", seed=7011).numpy()
        reg = np.ascontiguousarray(t.reshape(3, 3, 224, 224, 3).transpose(0, 2, 1, 3, 4).reshape(672, 672, 3))
        reg[20:200, 224 + 10:224 + 210] = (20, 40, 220)
        x = torch.from_numpy(reg[224:448, 224:448].copy()).permute(2, 0, 1)[None].float()
        for _ in range(3):
            x = F.avg_pool2d(F.pad(x, (4, 4, 4, 4), mode="replicate"), 9, 1)
        reg[224:448, 224:448] = x.round().clamp(0, 255).to(torch.uint8)[0].permute(1, 2, 0).numpy()
        reg[448:672, 0:224] = np.random.default_rng(5).integers(0, 30, (224, 224, 3))
        _CACHE["region"] = reg
    return _CACHE["region"]


GATE = QualityGate(min_tissue=0.25, max_pen=0.25, max_dark=0.5, min_focus=20.0)
DROPPED = {(224, 0), (224, 224), (0, 448)}


@pytest.mark.parametrize("tissue", [None, TissueRule(20, 0.1), "mask"])
def test_region_grid_with_a_gate(model, tissue):
    reg = gate_region()
    x = torch.from_numpy(reg).to(DEV)
    if tissue == "mask":
        tissue = TissueMask(np.ones((21, 21), np.uint8), 32)
    grid = model.region_grid(x, 224, None, tissue)
    assert torch.equal(grid, model.region_grid(x, 224, None, tissue, quality=None))               # None: today's path, bit for bit
    q = model.region_quality(x, grid, 224, rules=GATE.rules)
    want = grid[GATE.keep(q)]
    got = model.region_grid(x, 224, None, tissue, quality=GATE)
    assert torch.equal(got, want)
    host = Q.tile_quality_numpy(reg, grid.cpu().numpy(), 224)
    assert np.array_equal(q.to_numpy(), host)
    assert torch.equal(GATE.keep(q).cpu(), GATE.keep(TileQuality(torch.from_numpy(host), 224)))
    kept = {tuple(c) for c in got.cpu().tolist()}
    assert len(grid) == 9 and len(kept) == 6 and not (kept & DROPPED)
    # origin and coord_scale go through
    got2 = model.region_grid(x[5:, 3:], 224, 200, None, origin=(64, 32), coord_scale=2, quality=GATE)
    grid2 = model.region_grid(x[5:, 3:], 224, 200, None, origin=(64, 32), coord_scale=2)
    assert torch.equal(got2, grid2[GATE.keep(model.region_quality(x[5:, 3:], grid2, 224, origin=(64, 32), coord_scale=2))])


def test_encode_region_with_a_gate(model):
    x = torch.from_numpy(gate_region()).to(DEV)
    f0, c0 = model.encode_region(x, 224)
    f1, c1 = model.encode_region(x, 224, quality=None)
    assert torch.equal(f0, f1) and torch.equal(c0, c1)
    f, c = model.encode_region(x, 224, quality=GATE)
    assert torch.equal(c, model.region_grid(x, 224, quality=GATE)) and c.shape == (6, 2)
    assert torch.equal(f, model.encode_image_uint8(model.region_patches_uint8(x, c, 224)))        # as tests/test_region_gpu.py: the same bits
    keep = GATE.keep(model.region_quality(x, c0, 224))
    assert torch.equal(c, c0[keep])
    fa, ca, attn = model.encode_region_attention(x, 224, quality=GATE)
    assert torch.equal(ca, c) and fa.shape == f.shape and attn.shape[0] == 6
    # a gate nothing passes
    fe, ce = model.encode_region(x, 224, quality=QualityGate(min_focus=1e9))
    assert fe.shape == (0, 768) and ce.shape == (0, 2)
    with pytest.raises(ValueError, match="QualityGate"):
        model.encode_region(x, 224, quality=True)


def test_extract_slide_features_with_a_gate(model, tmp_path, monkeypatch):
    from keep_amd import cohort
    reg = gate_region()
    saved = {}
    real_save = cohort.save_slide_features

    def spy(data_source, slide_id, features, coords=None, use_h5=False):
        saved["features"], saved["coords"] = features, np.asarray(coords)
        return real_save(data_source, slide_id, features, coords, use_h5)

    monkeypatch.setattr(cohort, "save_slide_features", spy)
    f, c = model.encode_region(torch.from_numpy(reg).to(DEV), 224, quality=GATE)
    for tissue in (None, TissueMask(np.ones((21, 21), np.uint8), 32)):       # whole bands through encode_region; cells decided on a mask first
        cohort.extract_slide_features(lambda x, y, w, h: reg[y:y + h, x:x + w], 672, 672, "s", str(tmp_path), patch_size=224, tissue=tissue,
                                      band_rows=2, model=model, quality=GATE)
        assert np.array_equal(saved["coords"], c.cpu().numpy())
        # across bands the batches differ, so rounding may too (the bound of tests/test_region_gpu.py for the same comparison)
        assert saved["features"].shape == (6, 768) and (saved["features"] - f.cpu()).abs().max().item() < 1e-5


def test_the_methods_check_their_arguments(model):
    ok = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    for bad in (ok[:, :, :7], ok.to(torch.int32), ok.float(), torch.zeros((2, 8, 8, 5), dtype=torch.uint8), torch.zeros((2, 8, 8), dtype=torch.uint8),
                torch.zeros((8, 8, 3), dtype=torch.uint8), torch.zeros((1, 1025, 1025, 3), dtype=torch.uint8), [[0]], None):
        with pytest.raises(ValueError):
            model.tile_quality(bad)
    with pytest.raises(ValueError, match="2\\^31"):              # 2^21 tiles of 1024 rows: checked on the shape, nothing is allocated
        model.tile_quality(torch.zeros((1, 1024, 1024, 3), dtype=torch.uint8).expand(1 << 21, 1024, 1024, 3))
    for rules in ("default", QualityGate(), 3):
        with pytest.raises(ValueError, match="QualityRules"):
            model.tile_quality(ok, rules=rules)
        with pytest.raises(ValueError, match="QualityRules"):
            model.pen_mask(ok[0], rules=rules)
        with pytest.raises(ValueError, match="QualityRules"):
            model.region_quality(ok[0], [[0, 0]], 4, rules=rules)
    region = torch.zeros((32, 40, 3), dtype=torch.uint8, device=DEV)
    for coords in ([0, 0], [[0, 0, 0]], torch.zeros((2, 2, 2), dtype=torch.int64)):
        with pytest.raises(ValueError, match="coords"):
            model.region_quality(region, coords, 16)
    for patch in (0, -1, 1025, 16.5, True, "16"):
        with pytest.raises(ValueError, match="patch"):
            model.region_quality(region, [[0, 0]], patch)
    with pytest.raises(ValueError, match="larger than the region"):
        model.region_quality(region, [[0, 0]], 33)
    for kw in (dict(origin=(0,)), dict(origin=(0.5, 0)), dict(coord_scale=0), dict(coord_scale=1.5)):
        with pytest.raises(ValueError):
            model.region_quality(region, [[0, 0]], 16, **kw)
    for bad in (region.to(torch.int16), region[..., :2], region[0], region.permute(1, 0, 2)[:, :, [2, 1, 0]].permute(2, 0, 1), torch.zeros((0, 4, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            model.region_quality(bad, [[0, 0]], 1)
        with pytest.raises(ValueError):
            model.pen_mask(bad)
    for quality in (True, QualityRules(), "gate"):
        with pytest.raises(ValueError, match="QualityGate"):
            model.region_grid(region, 16, quality=quality)
    with pytest.raises(ValueError, match="patch"):               # a gate measures patches up to 1024
        model.region_grid(torch.zeros((1100, 1100, 3), dtype=torch.uint8, device=DEV), 1025, quality=QualityGate())
    # more sets of rules than the engine keeps on the device: every one still gives its own table
    img = torch.from_numpy(scene(16, 16, 2)).to(DEV)
    for k in range(20):
        r = QualityRules(dark_max=k, white_min=255 - k)
        assert np.array_equal(model.region_quality(img, [[0, 0]], 16, rules=r).to_numpy(), Q.tile_quality_numpy(img.cpu().numpy(), [[0, 0]], 16, r))
    assert len(model._quality_blobs) <= 16
