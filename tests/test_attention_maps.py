"""The host side of the CLS attention maps: keep_amd.heatmap.cell_raster_numpy against a triple loop in Python
integers (attention_reference.cell_raster_brute), keep_amd.attention.cls_attention_map, and the argument checks that need no device."""
import numpy as np
import pytest
import torch

import attention_reference as AR
from keep_amd import KEEPModel
from keep_amd.attention import cls_attention_map
from keep_amd.heatmap import (MAX_TILES, TileRaster, cell_raster_numpy, check_cell_args, check_cells, raster_numpy)

CASES = AR.raster_cases()


# ---------------------------------------------------------------------------------------------- cell_raster_numpy
@pytest.mark.parametrize("name", sorted(CASES))
def test_cell_raster_numpy_equals_the_brute_force(name):
    coords, values, grid, patch, d, shape, origin = CASES[name]
    got = cell_raster_numpy(coords, values, grid, patch, d, shape, origin)
    want = AR.cell_raster_brute(coords, values, grid, patch, d, shape, origin)
    assert got.dtype == np.int64 and got.shape == shape
    assert np.array_equal(got, want)
    assert (got != 0).any() or name == "off_raster"


def test_cell_raster_numpy_cases_cover_what_they_claim():
    """Each family of the list does what its name says: clipped footprints, pixels starting before their tile, overlap, NaN cells."""
    c, v, g, P, d, shape, o = CASES["borders_d16"]
    assert (c < 0).any() and (c[:, 0] + P > shape[1] * d).any() and (c[:, 1] + P > shape[0] * d).any()
    c = CASES["unaligned_d16"][0]
    assert (c % 16 != 0).all()
    acc = cell_raster_numpy(*CASES["overlap_step112"])
    assert (acc >> 40).max() == 4
    c, v, g, P, d, shape, o = CASES["nan_cells"]
    acc = cell_raster_numpy(c, v, g, P, d, shape, o)
    full = cell_raster_numpy(c, np.nan_to_num(v, nan=0.5), g, P, d, shape, o)
    assert ((acc >> 40) < (full >> 40)).any() and ((acc >> 40) <= (full >> 40)).all()
    only_nan = cell_raster_numpy(c[1:2], v[1:2], g, P, d, shape, o)
    assert not only_nan.any()                                 # a tile of NaN cells adds neither sum nor count


def test_cell_raster_numpy_into_adds_and_the_split_does_not_matter():
    coords, values, grid, patch, d, shape, origin = CASES["many_tiles"]
    whole = cell_raster_numpy(coords, values, grid, patch, d, shape, origin)
    acc = None
    for lo, hi in ((0, 70), (70, 71), (71, 200)):
        acc = cell_raster_numpy(coords[lo:hi], values[lo:hi], grid, patch, d, shape, origin, into=acc)
    assert np.array_equal(acc, whole)
    want = AR.cell_raster_brute(coords[:5], values[:5], grid, patch, d, shape, origin)
    want = AR.cell_raster_brute(coords[5:9], values[5:9], grid, patch, d, shape, origin, into=want)
    assert np.array_equal(cell_raster_numpy(coords[:9], values[:9], grid, patch, d, shape, origin), want)
    with pytest.raises(ValueError, match="into must be int64"):
        cell_raster_numpy(coords, values, grid, patch, d, shape, origin, into=np.zeros((3, 3), np.int64))


@pytest.mark.parametrize("name", ["aligned_d16", "aligned_d4", "aligned_d1", "unaligned_d7", "borders_origin_d8", "overlap_step112",
                                  "grid3x5_patch240", "many_tiles"])
def test_constant_tiles_equal_the_tile_raster(name):
    coords, values, grid, patch, d, shape, origin = CASES[name]
    per_tile = values[:, 0].copy()
    per_tile[::5] = np.nan                                    # a NaN tile is skipped by both
    const = np.repeat(per_tile[:, None], grid[0] * grid[1], axis=1)
    assert np.array_equal(cell_raster_numpy(coords, const, grid, patch, d, shape, origin), raster_numpy(coords, per_tile, patch, d, shape, origin))


# ---------------------------------------------------------------------------------------------- cls_attention_map
def _attn(B=3, H=4, T=17, seed=0):
    return torch.softmax(AR.rand(B, H, T, seed=seed, std=2.0).double(), dim=-1).float()


def test_cls_attention_map_normalisations():
    a = _attn()
    patches = a[:, :, 1:].double()
    mean = patches.mean(dim=1)
    none = cls_attention_map(a, normalize="none")
    assert none.shape == (3, 16) and none.dtype == torch.float32
    assert torch.allclose(none.double(), mean, rtol=1e-6, atol=0)
    # a row of the raw map sums to 1 - the mean CLS -> CLS weight
    assert torch.allclose(none.double().sum(1), 1 - a[:, :, 0].double().mean(1), rtol=1e-5)
    tmax = cls_attention_map(a)                               # the default
    assert torch.allclose(tmax.double(), mean / mean.amax(dim=1, keepdim=True), rtol=1e-6)
    assert torch.equal(tmax.amax(dim=1), torch.ones(3))
    s = cls_attention_map(a, normalize="sum")
    assert torch.allclose(s.double(), mean / mean.sum(dim=1, keepdim=True), rtol=1e-6)
    assert torch.allclose(s.sum(1), torch.ones(3), rtol=1e-6)
    zero = torch.zeros(2, 4, 5)
    zero[:, :, 0] = 1.0                                       # all weight on CLS -> CLS: the map stays 0, no NaN
    for mode in ("tile_max", "sum", "none"):
        assert torch.equal(cls_attention_map(zero, normalize=mode), torch.zeros(2, 4))
    assert cls_attention_map(a.double()).dtype == torch.float64
    assert cls_attention_map(a[:, :, :1]).shape == (3, 0)      # a sequence of the CLS token alone


def test_cls_attention_map_head_selection():
    a = _attn(seed=3)
    patches = a[:, :, 1:]
    assert torch.equal(cls_attention_map(a, heads=2, normalize="none"), patches[:, 2])
    assert torch.equal(cls_attention_map(a, heads=-1, normalize="none"), patches[:, 3])
    assert torch.allclose(cls_attention_map(a, heads=[0, 3], normalize="none"), (patches[:, 0] + patches[:, 3]) / 2, rtol=1e-6)
    assert torch.equal(cls_attention_map(a, heads=(1,), normalize="none"), patches[:, 1])
    assert torch.equal(cls_attention_map(a, heads=None), cls_attention_map(a, heads=[0, 1, 2, 3]))
    assert not torch.equal(cls_attention_map(a, heads=0), cls_attention_map(a, heads=1))


def test_cls_attention_map_errors():
    a = _attn()
    for bad in (a[0], a[:, :, :, None], a.to(torch.int32), a.numpy()):
        with pytest.raises(ValueError, match=r"\[B, heads, T\]"):
            cls_attention_map(bad)
    with pytest.raises(ValueError, match="normalize"):
        cls_attention_map(a, normalize="max")
    for bad in (4, -5, [0, 4], [], True, 1.0, [0.0]):
        with pytest.raises(ValueError, match="heads"):
            cls_attention_map(a, heads=bad)


# ---------------------------------------------------------------------------------------------- argument checks without a device
def test_check_cell_args():
    assert check_cell_args((14, 14), 224, 16, (10, 20)) == ((14, 14), 224, 16, (10, 20), (0, 0))
    assert check_cell_args((3, 5), 240, 48, (7, 9), (96, -48)) == ((3, 5), 240, 48, (7, 9), (96, -48))
    with pytest.raises(ValueError, match="multiple of both sides"):
        check_cell_args((14, 14), 225, 1, (10, 10))            # patch % gw
    with pytest.raises(ValueError, match="multiple of both sides"):
        check_cell_args((5, 14), 224, 1, (10, 10))             # patch % gh
    with pytest.raises(ValueError, match=r"cell side = 16"):
        check_cell_args((14, 14), 224, 17, (10, 10))           # downsample > cw
    with pytest.raises(ValueError, match=r"cell side = 48"):
        check_cell_args((3, 5), 240, 49, (10, 10))             # the smaller of the two sides: cw = 48, ch = 80
    with pytest.raises(ValueError, match="downsample"):
        check_cell_args((14, 14), 224, 0, (10, 10))
    for grid in ((14,), (0, 14), (14, -1), (14.5, 14), (1 << 13, 1 << 12)):
        with pytest.raises(ValueError, match="grid"):
            check_cell_args(grid, 1 << 13, 1, (10, 10))
    with pytest.raises(ValueError, match="multiple of downsample"):
        check_cell_args((14, 14), 224, 16, (10, 10), (8, 0))   # what check_raster_args asks of every raster
    with pytest.raises(ValueError, match="shape"):
        check_cell_args((14, 14), 224, 16, (10,))


def test_check_cells_and_cell_raster_argument_errors():
    coords = torch.zeros((4, 2), dtype=torch.int64)
    assert check_cells(coords, torch.zeros(4, 196), (14, 14)) == 4
    for bad in (torch.zeros(4, 195), torch.zeros(4), torch.zeros(4, 14, 14), torch.zeros(3, 196), torch.zeros((4, 196), dtype=torch.int32)):
        with pytest.raises(ValueError):
            check_cells(coords, bad, (14, 14))
    with pytest.raises(ValueError, match="integers"):
        check_cells(coords.float(), torch.zeros(4, 196), (14, 14))
    # KEEPModel.cell_raster raises these before it touches a device (none is visible to the CPU suite)
    m = KEEPModel()
    good = (coords, torch.zeros(4, 196), (14, 14), 224, 16, (10, 10))
    with pytest.raises(ValueError, match="multiple of both sides"):
        m.cell_raster(coords, torch.zeros(4, 196), (14, 14), 225, 16, (10, 10))
    with pytest.raises(ValueError, match="cell side"):
        m.cell_raster(coords, torch.zeros(4, 196), (14, 14), 224, 17, (10, 10))
    with pytest.raises(ValueError, match="gh gw = 196"):
        m.cell_raster(coords, torch.zeros(4, 197), (14, 14), 224, 16, (10, 10))
    with pytest.raises(ValueError, match="must be a TileRaster"):
        m.cell_raster(*good, into=np.zeros((10, 10), np.int64))
    host = TileRaster(torch.zeros((10, 10), dtype=torch.int64), 16, 224, (0, 0), MAX_TILES - 3)
    with pytest.raises(ValueError, match="at most 2\\^24 - 1"):
        m.cell_raster(*good, into=host)                       # the cap counts tiles, and is enforced by claim before any device work
    assert host.tiles == MAX_TILES - 3
    with pytest.raises(ValueError, match="into= raster has patch"):
        m.cell_raster(*good, into=TileRaster(torch.zeros((10, 10), dtype=torch.int64), 8, 224))
