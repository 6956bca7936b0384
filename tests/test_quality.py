"""Tile quality control, host side: keep_amd.quality's rules, numpy restatements, TileQuality, QualityGate and
exclude.  No GPU: the restatements are held to a per-pixel Python loop written from the definitions, the device kernels to the
restatements (tests/test_quality_gpu.py)."""
import math

import numpy as np
import pytest
import torch

from keep_amd import QualityGate, QualityRules, TileQuality
from keep_amd import quality as Q
from keep_amd.region import TissueMask, TissueRule, region_grid_numpy, tissue_params

RULES = QualityRules(sat_min=40, white_min=200, dark_max=50,
                     pen=((1, 0, 120, 100, 255, 0, 140), (0, 0, 80, 0, 160, 130, 255), (3, 51, 90, 51, 90, 51, 90), (2, 150, 255, 0, 90, 0, 90)))


def pixels(h, w, seed):
    """Noise with every class in it: a third of the pixels are drawn near glass, near dark or as greys."""
    g = np.random.default_rng(seed)
    a = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
    kind = g.integers(0, 6, (h, w))
    a[kind == 0] = g.integers(190, 256, (int((kind == 0).sum()), 3))
    a[kind == 1] = g.integers(0, 70, (int((kind == 1).sum()), 3))
    grey = g.integers(0, 256, (h, w, 1), dtype=np.uint8)
    a[kind == 2] = np.broadcast_to(grey, (h, w, 3))[kind == 2]
    return a


def loop_class(r, g, b, rules):
    """One pixel by the priority list: 0-3 pen, 4 dark, 5 glass, 6 tissue, 7 other."""
    for cls in range(4):
        for k, r0, r1, g0, g1, b0, b1 in rules.pen:
            if k == cls and r0 <= r <= r1 and g0 <= g <= g1 and b0 <= b <= b1:
                return cls
    mx, mn = max(r, g, b), min(r, g, b)
    if mx <= rules.dark_max:
        return 4
    if mn >= rules.white_min:
        return 5
    if mx > 0 and 255 * (mx - mn) >= rules.sat_min * mx:
        return 6
    return 7


def loop_table(tile, rules):
    """One tile, pixel by pixel: the twelve columns and the list of Laplacians."""
    P = tile.shape[0]
    t = [[tuple(int(v) for v in tile[y, x, :3]) for x in range(P)] for y in range(P)]
    cls = [[loop_class(*t[y][x], rules) for x in range(P)] for y in range(P)]
    grey = [[(77 * t[y][x][0] + 150 * t[y][x][1] + 29 * t[y][x][2] + 128) >> 8 for x in range(P)] for y in range(P)]
    row = [0] * 12
    for y in range(P):
        for x in range(P):
            if cls[y][x] < 7:
                row[cls[y][x]] += 1
    laps = []
    for y in range(1, P - 1):
        for x in range(1, P - 1):
            L = 4 * grey[y][x] - grey[y][x - 1] - grey[y][x + 1] - grey[y - 1][x] - grey[y + 1][x]
            laps.append(L)
            row[7] += L
            row[8] += L * L
            if cls[y][x] == 6:
                row[9] += 1
                row[10] += L
                row[11] += L * L
    return row, laps, sum(1 for y in range(P) for x in range(P) if cls[y][x] == 7)


# ------------------------------------------------------------------------------------------------ the restatements
@pytest.mark.parametrize("patch", [1, 2, 3, 5, 9])
@pytest.mark.parametrize("rules", [QualityRules(), RULES])
def test_restatement_against_a_per_pixel_loop(patch, rules):
    region = pixels(2 * patch + 3, 2 * patch + 4, 10 + patch)
    rgba = np.concatenate([region, np.full(region.shape[:2] + (1,), 9, np.uint8)], axis=2)
    cells = [(0, 0), (1, 2), (patch + 4, patch + 3), (2, patch + 3), (patch // 2 + 1, patch // 2)]
    got = Q.tile_quality_numpy(region, cells, patch, rules)
    assert got.dtype == np.int64 and got.shape == (5, 12)
    assert np.array_equal(got, Q.tile_quality_numpy(rgba, np.array(cells), patch, rules))      # the alpha is ignored
    seen = np.zeros(8, np.int64)
    for i, (x, y) in enumerate(cells):
        row, laps, other = loop_table(region[y:y + patch, x:x + patch], rules)
        assert got[i].tolist() == row, (patch, i)
        assert got[i, :7].sum() + other == patch * patch                                         # every pixel has one class
        assert len(laps) == max(patch - 2, 0) ** 2
        seen[:7] += got[i, :7]
        seen[7] += other
    if patch == 9:
        assert (seen > 0).all()
    q = TileQuality(torch.from_numpy(got), patch)
    assert q.n == 5 and q.other_count().tolist() == [patch * patch - int(r[:7].sum()) for r in got]
    assert np.array_equal(q.to_numpy(), got)
    assert np.array_equal(Q.tile_quality_numpy(region, np.zeros((0, 2), np.int64), patch, rules), np.zeros((0, 12), np.int64))


def test_class_mask_and_the_kernel_tables_agree_with_the_loop():
    img = pixels(23, 31, 3)
    for rules in (QualityRules(), RULES, QualityRules(pen=())):
        got = Q.pen_mask_numpy(img, rules)
        want = np.array([[(loop_class(*(int(v) for v in img[y, x]), rules) + 1) % 8 for x in range(31)] for y in range(23)], np.uint8)
        assert got.dtype == np.uint8 and np.array_equal(got, want)
        # the words the kernels read: box masks per channel, the boxes sorted by class
        blob = rules.blob()
        assert blob.dtype == np.int32 and blob.shape == (776,) and blob[:4].tolist() == [rules.sat_min, rules.white_min, rules.dark_max, len(rules.pen)]
        lut = blob[8:].view(np.uint32).reshape(3, 256)
        inside = lut[0][img[..., 0]] & lut[1][img[..., 1]] & lut[2][img[..., 2]]
        lowest = np.array([[(int(v) & -int(v)).bit_length() - 1 for v in r] for r in inside])
        pen = (lowest >= blob[4]).astype(int) + (lowest >= blob[5]) + (lowest >= blob[6])
        assert np.array_equal(inside != 0, (got >= 1) & (got <= 4)) and np.array_equal(pen[inside != 0] + 1, got[inside != 0])
    assert Q.CLASS_NAMES[Q.DARK] == "dark" and Q.CLASS_NAMES[Q.GLASS] == "glass" and Q.CLASS_NAMES[Q.TISSUE] == "tissue"
    assert tuple(n[4:] for n in Q.CLASS_NAMES[1:5]) == Q.PEN_CLASSES


def test_priority_overlapping_boxes_and_ink_off():
    px = np.array([[[30, 120, 200]]], np.uint8)
    two = QualityRules(pen=((2, 0, 50, 100, 140, 150, 255), (1, 20, 40, 0, 255, 0, 255)))
    assert Q.tile_quality_numpy(px, [(0, 0)], 1, two)[0, :7].tolist() == [0, 1, 0, 0, 0, 0, 0]          # the lower id, whatever the order
    assert Q.pen_mask_numpy(px, two)[0, 0] == 2
    off = QualityRules(pen=())
    assert Q.tile_quality_numpy(px, [(0, 0)], 1, off)[0, :7].tolist() == [0, 0, 0, 0, 0, 0, 1]
    assert Q.tile_quality_numpy(pixels(9, 9, 1), [(0, 0)], 9, off)[0, :4].sum() == 0
    # ink before dark before glass before tissue
    both = QualityRules(white_min=10, dark_max=250, sat_min=0, pen=((3, 0, 5, 0, 5, 0, 5),))
    for rgb, want in (((3, 3, 3), 4), ((100, 100, 100), Q.DARK), ((251, 252, 253), Q.GLASS), ((255, 0, 0), Q.TISSUE)):
        assert Q.pen_mask_numpy(np.array([[rgb]], np.uint8), both)[0, 0] == want
    assert Q.pen_mask_numpy(np.array([[(0, 0, 0)]], np.uint8), QualityRules(dark_max=0, sat_min=0, pen=()))[0, 0] == Q.DARK
    # the tissue class is TissueRule's pixel test: a whole-region count decides the grid the same way
    img = pixels(32, 32, 9)
    none = QualityRules(white_min=255, dark_max=0, pen=())
    n = int(Q.tile_quality_numpy(img, [(0, 0)], 32, none)[0, 6]) + int((Q.pen_mask_numpy(img, none) == Q.GLASS).sum())
    sat_min, _ = tissue_params(TissueRule(20, 0.5), 32)
    assert len(region_grid_numpy(img, 32, None, sat_min, n)) == 1 and len(region_grid_numpy(img, 32, None, sat_min, n + 1)) == 0


def test_focus_is_the_variance_of_the_laplacian():
    region = pixels(40, 30, 2)
    cells = [(0, 0), (7, 11), (14, 24)]
    for patch in (3, 4, 16):
        tab = Q.tile_quality_numpy(region, cells, patch, RULES)
        q = TileQuality(torch.from_numpy(tab), patch)
        for i, (x, y) in enumerate(cells):
            t = region[y:y + patch, x:x + patch]
            L = Q.laplacian_numpy(Q.grey_numpy(t))
            assert L.shape == (patch - 2, patch - 2)
            assert q.focus()[i].item() == pytest.approx(np.var(L.astype(np.float64)), rel=1e-12, abs=0)
            tis = Q.pen_mask_numpy(t, RULES)[1:-1, 1:-1] == Q.TISSUE
            if tis.any():
                assert q.focus(tissue=True)[i].item() == pytest.approx(np.var(L[tis].astype(np.float64)), rel=1e-12, abs=0)
            else:
                assert math.isnan(q.focus(tissue=True)[i].item())
    for patch in (1, 2):                                       # no interior pixel
        q = TileQuality(torch.from_numpy(Q.tile_quality_numpy(region, cells, patch)), patch)
        assert torch.isnan(q.focus()).all() and torch.isnan(q.focus(True)).all() and not q.table[:, 7:].any()
    glass = TileQuality(torch.from_numpy(Q.tile_quality_numpy(np.full((8, 8, 3), 240, np.uint8), [(0, 0)], 8)), 8)
    assert glass.focus().item() == 0.0 and math.isnan(glass.focus(True).item()) and glass.glass_fraction().item() == 1.0
    # the largest sums stay exact: a 1024 checkerboard row computed from its closed form
    big = TileQuality(torch.tensor([[0, 0, 0, 0, 1024 * 512, 1024 * 512, 0, 0, 1022 * 1022 * 1020 * 1020, 0, 0, 0]]), 1024)
    assert big.focus().item() == 1020.0 ** 2


def test_a_blur_lowers_the_focus():
    g = np.random.default_rng(64)
    tile = g.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    pad = np.pad(tile.astype(np.int64), ((1, 1), (1, 1), (0, 0)), mode="edge")
    blur = (sum(pad[dy:dy + 64, dx:dx + 64] for dy in range(3) for dx in range(3)) // 9).astype(np.uint8)
    q = TileQuality(torch.from_numpy(Q.tile_quality_numpy(np.stack([tile, blur]).reshape(128, 64, 3), [(0, 0), (0, 64)], 64)), 64)
    sharp, soft = q.focus().tolist()
    assert 0 < soft < sharp / 4


def test_fractions_and_pen_classes():
    tab = torch.tensor([[1, 2, 3, 4, 5, 6, 70, 0, 0, 0, 0, 0]])
    q = TileQuality(tab, 10)
    assert q.pen_fraction().item() == 0.1 and q.pen_fraction("green").item() == 0.02 and q.pen_fraction(3).item() == 0.04
    assert q.dark_fraction().item() == 0.05 and q.glass_fraction().item() == 0.06 and q.tissue_fraction().item() == 0.7
    assert q.other_count().item() == 9 and q.pixels == 100 and q.interior == 64
    for bad in ("pink", 4, -1, 1.0, True):
        with pytest.raises(ValueError):
            q.pen_fraction(bad)


# ------------------------------------------------------------------------------------------------ the gate
def test_gate_at_the_exact_boundary_counts():
    def tile(pen=0, dark=0, tissue=0, lap=(64, 0, 64 * 100), lap_t=(0, 0, 0)):
        return [pen, 0, 0, 0, dark, 0, tissue, lap[1], lap[2], lap_t[0], lap_t[1], lap_t[2]]
    P = 10                                                     # 100 pixels: fractions of a hundredth are whole pixels
    def keep(gate, *rows):
        return gate.keep(TileQuality(torch.tensor(rows, dtype=torch.int64), P)).tolist()
    assert QualityGate().keep(TileQuality(torch.zeros((3, 12), dtype=torch.int64), P)).tolist() == [True] * 3
    assert keep(QualityGate(min_tissue=0.25), tile(tissue=25), tile(tissue=24), tile(tissue=26)) == [True, False, True]
    assert keep(QualityGate(max_pen=0.25), tile(pen=25), tile(pen=26), [10, 5, 5, 5] + [0] * 8, [10, 5, 5, 6] + [0] * 8) == [True, False, True, False]
    assert keep(QualityGate(max_dark=0.5), tile(dark=50), tile(dark=51)) == [True, False]
    assert QualityGate(min_tissue=0.3, max_pen=0.7, max_dark=0.11).limits(10) == (30, 70, 11)
    assert QualityGate(min_tissue=1 / 3, max_pen=1 / 3, max_dark=1 / 3).limits(3) == (3, 3, 3)
    assert QualityGate(min_tissue=0.5, max_pen=0.5).limits(3) == (5, 4, 9)                      # ceil for the floor of tissue, floor for the caps
    # focus: variance 100 over all 64 interior pixels; over 4 tissue pixels with S1 = 4, S2 = 404: 404 / 4 - 1 = 100
    t = tile(lap_t=(4, 4, 404))
    assert keep(QualityGate(min_focus=100.0, focus_on_tissue=False), t) == [True]
    assert keep(QualityGate(min_focus=100.0), t) == [True]
    assert keep(QualityGate(min_focus=math.nextafter(100.0, 200.0)), t) == [False]
    assert keep(QualityGate(min_focus=100.0), tile(lap_t=(4, 4, 403))) == [False]
    nan = tile()                                               # no tissue pixel: the tissue focus is NaN
    assert keep(QualityGate(min_focus=1e-9), nan) == [False] and keep(QualityGate(min_focus=0.0), nan) == [True]
    assert keep(QualityGate(min_focus=1e-9, focus_on_tissue=False), nan) == [True]
    with pytest.raises(ValueError, match="TileQuality"):
        QualityGate().keep(torch.zeros((1, 12), dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ exclude
def test_exclude_against_numpy():
    g = np.random.default_rng(12)
    tissue = (g.random((41, 57)) < 0.8).astype(np.uint8)
    classes = np.full((41, 57), Q.TISSUE, np.uint8)
    classes[g.random((41, 57)) < 0.02] = 1
    classes[5:9, 30:50] = 3
    classes[20, 10] = Q.DARK
    classes[30:33, 5:8] = Q.GLASS
    mask = TissueMask(tissue, 16, "center", 9)
    out = Q.exclude(mask, classes)
    assert isinstance(out, TissueMask) and (out.downsample, out.mode, out.threshold) == (16, "center", 9)
    assert np.array_equal(out.mask.numpy(), tissue & ~np.isin(classes, (1, 2, 3, 4, 5)))
    assert np.array_equal(Q.exclude(mask, torch.from_numpy(classes), drop=(Q.GLASS,)).mask.numpy(), tissue & (classes != Q.GLASS))
    assert np.array_equal(Q.exclude(mask, classes, drop=()).mask.numpy(), tissue)
    yy, xx = np.mgrid[0:41, 0:57]
    for radius, drop in ((1, (1, 2, 3, 4, 5)), (3, (3,)), (5, (1, Q.DARK))):
        dropped = np.isin(classes, drop)
        ys, xs = np.nonzero(dropped)
        d2 = ((yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2).min(axis=2)                  # brute force: every dropped pixel
        got = Q.exclude(mask, classes, drop=drop, radius=radius).mask.numpy()
        assert np.array_equal(got, tissue & ~(d2 <= radius * radius)), radius
        try:
            from scipy.ndimage import distance_transform_edt
        except ImportError:
            continue
        assert np.array_equal(got, tissue & ~(distance_transform_edt(~dropped) <= radius))
    assert np.array_equal(Q.exclude(mask, np.full((41, 57), Q.TISSUE, np.uint8), radius=4).mask.numpy(), tissue)   # nothing dropped


# ------------------------------------------------------------------------------------------------ validation
def test_validation_errors():
    for kw in (dict(sat_min=-1), dict(sat_min=256), dict(white_min=2.5), dict(dark_max=True), dict(dark_max="40"), dict(pen=None), dict(pen=[1, 2]),
               dict(pen=((0, 1, 2, 3, 4, 5),)), dict(pen=((4, 0, 1, 0, 1, 0, 1),)), dict(pen=((-1, 0, 1, 0, 1, 0, 1),)), dict(pen=((0, 0, 256, 0, 1, 0, 1),)),
               dict(pen=((0, 9, 8, 0, 1, 0, 1),)), dict(pen=((0, 0, 1, 0, 1, 0, 1.5),)), dict(pen=((0, 0, 1, 0, 1, 0, 1),) * 33)):
        with pytest.raises(ValueError):
            QualityRules(**kw)
    r = QualityRules(pen=[[0, 0, 1, 0, 1, 0, 1]] * 32)
    assert len(r.pen) == 32 and isinstance(r.pen, tuple) and isinstance(r.pen[0], tuple) and hash(r) == hash(QualityRules(pen=r.pen))
    with pytest.raises(Exception):
        r.sat_min = 3                                          # frozen
    assert QualityRules().pen == Q.DEFAULT_PEN and len(Q.DEFAULT_PEN) <= 8 and {b[0] for b in Q.DEFAULT_PEN} == {0, 1, 2, 3}
    for kw in (dict(rules=QualityGate()), dict(rules="default"), dict(min_tissue=-0.1), dict(min_tissue=1.1), dict(max_pen=2), dict(max_dark="1"),
               dict(max_dark=float("nan")), dict(min_focus=-1), dict(min_focus=float("inf")), dict(min_focus=float("nan")), dict(min_focus=None),
               dict(focus_on_tissue=1), dict(min_tissue=True)):
        with pytest.raises(ValueError):
            QualityGate(**kw)
    assert QualityGate() == QualityGate(QualityRules()) and QualityGate().rules == QualityRules() == QualityGate(rules=None).rules
    for bad in (torch.zeros((2, 11), dtype=torch.int64), torch.zeros((2, 12), dtype=torch.int32), np.zeros((2, 12), np.int64), torch.zeros(12, dtype=torch.int64)):
        with pytest.raises(ValueError):
            TileQuality(bad, 16)
    for patch in (0, 1025, 2.0, True):
        with pytest.raises(ValueError):
            TileQuality(torch.zeros((1, 12), dtype=torch.int64), patch)
    img = np.zeros((8, 8, 3), np.uint8)
    for region, cells, patch, rules in ((img.astype(np.int32), [(0, 0)], 4, None), (img[..., :2], [(0, 0)], 4, None), (img[0], [(0, 0)], 4, None),
                                        (img, [(5, 0)], 4, None), (img, [(0, 5)], 4, None), (img, [(-1, 0)], 4, None), (img, [(0, 0, 0)], 4, None),
                                        (img, [(0.5, 0)], 4, None), (img, [(0, 0)], 0, None), (img, [(0, 0)], 1025, None), (img, [(0, 0)], 4, "rules")):
        with pytest.raises(ValueError):
            Q.tile_quality_numpy(region, cells, patch, rules)
    with pytest.raises(ValueError):
        Q.pen_mask_numpy(img.astype(np.float32))
    with pytest.raises(ValueError):
        Q.pen_mask_numpy(img, rules=QualityGate())
    mask = TissueMask(np.ones((8, 8), np.uint8), 2)
    ok = np.zeros((8, 8), np.uint8)
    for args, kw in (((mask.mask, ok), {}), ((mask, np.zeros((8, 9), np.uint8)), {}), ((mask, ok.astype(np.int32)), {}), ((mask, ok), dict(drop=(256,))),
                     ((mask, ok), dict(drop=(1.5,))), ((mask, ok), dict(radius=-1)), ((mask, ok), dict(radius=1024)), ((mask, ok), dict(radius=1.5))):
        with pytest.raises(ValueError):
            Q.exclude(*args, **kw)
    assert Q.check_gate(None) is None and Q.check_gate(QualityGate()) == QualityGate()
    for bad in (True, "gate", QualityRules()):
        with pytest.raises(ValueError):
            Q.check_gate(bad)
