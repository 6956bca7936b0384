"""Slide regions -> patch grid, tissue rule, coords: the host side, no GPU.

keep_amd.region.region_grid_numpy is the restatement the device kernels are held to (tests/test_region_gpu.py); here it is pinned
to hand-made cases, the band planner to the one-shot grid, and the argument checks to run before any device call."""
import math

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel
from keep_amd.region import TissueRule, check_grid_args, grid_shape, plan_bands, region_grid_numpy, tissue_params


def cells_of(region, patch, step=None, sat_min=0, min_pixels=0):
    return [tuple(c) for c in region_grid_numpy(region, patch, step, sat_min, min_pixels).tolist()]


def filled(h, w, rgb, c=3):
    a = np.zeros((h, w, c), np.uint8)
    a[..., :3] = rgb
    if c == 4:
        a[..., 3] = 255
    return a


def test_tissue_rule_at_its_boundary():
    # 255 (max - min) >= sat_min max: (255, 235, 235) is exactly saturation 20/255, (255, 236, 236) just below
    for rgb, s20, s0 in [((255, 235, 235), True, True), ((255, 236, 236), False, True), ((128, 128, 128), False, True),
                         ((255, 255, 255), False, True), ((0, 0, 0), False, False), ((1, 0, 0), True, True), ((200, 120, 180), True, True)]:
        r = filled(16, 16, rgb)
        assert (cells_of(r, 16, sat_min=20, min_pixels=1) == [(0, 0)]) == s20, rgb
        assert (cells_of(r, 16, sat_min=0, min_pixels=1) == [(0, 0)]) == s0, rgb
    # sat_min 255: only pure primaries / mixes with a zero channel
    assert cells_of(filled(16, 16, (10, 0, 3)), 16, sat_min=255, min_pixels=1) == [(0, 0)]
    assert cells_of(filled(16, 16, (10, 1, 3)), 16, sat_min=255, min_pixels=1) == []


def test_min_pixels_threshold_counts_exactly():
    r = filled(32, 32, (250, 250, 250))
    r[3:8, 5:10] = (200, 50, 120)                   # 25 tissue pixels in cell (0, 0)
    r[20, 20] = (200, 50, 120)                      # 1 in cell (16, 16)
    assert cells_of(r, 16, sat_min=20, min_pixels=25) == [(0, 0)]
    assert cells_of(r, 16, sat_min=20, min_pixels=26) == []
    assert cells_of(r, 16, sat_min=20, min_pixels=1) == [(0, 0), (16, 16)]
    assert cells_of(r, 16) == [(0, 0), (16, 0), (0, 16), (16, 16)]          # rule off: every cell, row-major


def test_cells_touching_the_edge_and_partial_cells():
    assert cells_of(filled(16, 48, 0), 16) == [(0, 0), (16, 0), (32, 0)]
    assert cells_of(filled(16, 47, 0), 16) == [(0, 0), (16, 0)]
    assert cells_of(filled(15, 48, 0), 16) == []
    assert cells_of(filled(33, 33, 0), 16) == [(0, 0), (16, 0), (0, 16), (16, 16)]
    assert grid_shape(15, 100, 16, 16) == (0, 6) and grid_shape(100, 15, 16, 7) == (13, 0)


def test_step_smaller_and_larger_than_the_patch():
    r = filled(40, 40, 0)
    assert cells_of(r, 16, step=12) == [(x, y) for y in (0, 12, 24) for x in (0, 12, 24)]
    assert cells_of(r, 16, step=20) == [(0, 0), (20, 0), (0, 20), (20, 20)]
    assert cells_of(r, 16, step=25) == [(0, 0)]
    # overlapping windows share tissue: only the cells that cover the stained square are kept
    r = filled(40, 40, (240, 240, 240))
    r[12:16, 12:16] = (150, 40, 110)
    assert cells_of(r, 16, step=12, sat_min=20, min_pixels=16) == [(0, 0), (12, 0), (0, 12), (12, 12)]
    assert cells_of(r, 16, step=12, sat_min=20, min_pixels=17) == []


def test_rgba_alpha_is_ignored():
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, (50, 70, 3), dtype=np.uint8)
    rgba = np.concatenate([rgb, rng.integers(0, 256, (50, 70, 1), dtype=np.uint8)], 2)
    assert cells_of(rgb, 16, 7, 60, 100) == cells_of(rgba, 16, 7, 60, 100)


def test_origin_and_coord_scale():
    cells = torch.tensor([[0, 0], [256, 0], [0, 512]], dtype=torch.int32)
    got = KEEPModel._cells_to_coords(cells, (1000, 2000), 4)
    assert got.dtype == torch.int64
    assert got.tolist() == [[4000, 8000], [5024, 8000], [4000, 10048]]
    assert KEEPModel._cells_to_coords(cells, (0, 0), 1).tolist() == cells.tolist()


def test_tissue_params():
    assert tissue_params(None, 224) == (0, 0) and tissue_params(False, 224) == (0, 0)
    assert tissue_params(True, 224) == (TissueRule().sat_min, math.ceil(TissueRule().min_fraction * 224 * 224))
    assert tissue_params((30, 0.5), 256) == (30, 32768)
    assert tissue_params({"sat_min": 8, "min_fraction": 0.1}, 100) == (8, 1000)
    assert tissue_params(TissueRule(0, 1.0), 16) == (0, 256)
    assert tissue_params(TissueRule(5, 1e-9), 16) == (5, 1)
    for bad in [(256, 0.5), (-1, 0.5), (20, 1.5), (20, -0.1), (20.5, 0.5), "yes", (1, 2, 3)]:
        with pytest.raises(ValueError):
            tissue_params(bad, 224)


def band_union(region, patch, step, band_rows, sat_min, min_pixels):
    H, W = region.shape[:2]
    out = []
    for r0, r1, y0, h in plan_bands(W, H, patch, step, band_rows):
        band = region[y0:y0 + h]
        got = region_grid_numpy(band, patch, step, sat_min, min_pixels)
        assert grid_shape(h, W, patch, step or patch)[0] == r1 - r0
        out += [(x, y + y0) for x, y in got.tolist()]
    return out


def test_band_planner_covers_every_cell_once_in_order():
    rng = np.random.default_rng(7)
    for _ in range(60):
        p = int(rng.integers(16, 40))
        step = int(rng.integers(1, 2 * p)) if rng.random() < 0.8 else None
        W, H = int(rng.integers(1, 160)), int(rng.integers(1, 200))
        band_rows = int(rng.integers(1, 9))
        region = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        region[rng.random((H, W)) < 0.5] = 245                           # glass
        for sat_min, frac in ((0, 0.0), (40, 0.3)):
            mp = math.ceil(frac * p * p)
            want = cells_of(region, p, step, sat_min, mp)
            got = band_union(region, p, step, band_rows, sat_min, mp)
            assert got == want, (p, step, W, H, band_rows)
            assert len(set(got)) == len(got)
        bands = plan_bands(W, H, p, step, band_rows)
        s = step or p
        for (r0, r1, y0, h), nxt in zip(bands, bands[1:] + [None]):
            assert y0 == r0 * s and y0 + h == (r1 - 1) * s + p <= H and 0 < r1 - r0 <= band_rows
            if nxt:
                assert nxt[0] == r1


def test_argument_checks_run_before_any_device_call():
    m = KEEPModel()                                         # no handle, no weights: a device call would raise KeepHipError
    r = torch.zeros((64, 64, 3), dtype=torch.uint8)
    bad_calls = [
        lambda: m.region_grid(r, patch_size=15),
        lambda: m.region_grid(r, patch_size=32, step=0),
        lambda: m.region_grid(r, patch_size=32, coord_scale=0),
        lambda: m.region_grid(r, patch_size=32, origin=(1,)),
        lambda: m.region_grid(r, patch_size=32, tissue=(300, 0.5)),
        lambda: m.region_grid(r.float(), patch_size=32),
        lambda: m.region_grid(torch.zeros((64, 64, 2), dtype=torch.uint8), patch_size=32),
        lambda: m.region_grid(torch.zeros((64, 64), dtype=torch.uint8), patch_size=32),
        lambda: m.region_grid(torch.zeros((0, 64, 3), dtype=torch.uint8), patch_size=32),
        lambda: m.region_grid(np.zeros((64, 128, 3), np.uint8)[:, ::2], patch_size=32),       # pixel stride 6
        lambda: m.region_grid(r.permute(1, 0, 2), patch_size=32),                               # pixels a row apart
        lambda: m.region_patches_uint8(r, torch.zeros((3, 3), dtype=torch.int64), 32),
        lambda: m.region_patches_uint8(r, torch.zeros((3, 2), dtype=torch.int64), 8),
        lambda: m.encode_region(r, patch_size=32, batch=0),
        lambda: m.encode_region(r, patch_size=32, step=-2),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        check_grid_args(True, None)
    for args in [(0, 10, 16, 16, 1), (10, 10, 16, 16, 0), (10, 10, 8, None, 1)]:
        with pytest.raises(ValueError):
            plan_bands(*args)


def test_extract_slide_features_checks_before_reading():
    from keep_amd import cohort

    def never(*a):
        raise AssertionError("read_region must not be called")
    for kw in [dict(patch_size=8), dict(step=0), dict(band_rows=0), dict(coord_scale=0)]:
        with pytest.raises(ValueError):
            cohort.extract_slide_features(never, 1000, 1000, "s", "/nonexistent", **kw)
