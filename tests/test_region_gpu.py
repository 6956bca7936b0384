"""Slide regions on the MI355X: keep_region_grid / keep_region_patches_u8, KEEPModel.region_grid /
region_patches_uint8 / encode_region and cohort.extract_slide_features.

Yardsticks: keep_amd.region.region_grid_numpy (the grid + tissue rule restated, tests/test_region.py pins it by hand), host-cut
patches, keep_amd.preprocess.resize_bicubic_u8_numpy (Pillow's integer resample restated), encode_image_uint8 on the same tiles in
the same batches, and oracle.keep_oracle.encode_image on the normalised tiles.  Regions are mosaics of synth_tile_family tiles
(he_crops, stain_field, background, half), so the tissue rule has real glass to drop."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from keep_amd import KEEPModel, _lib, cohort, wsi
from keep_amd.config import KEEPShape, small_shape
from keep_amd.model import _ptr, _stream
from keep_amd.preprocess import resize_bicubic_u8_numpy
from keep_amd.region import TissueRule, region_grid_numpy, tissue_params
from keep_amd.synth import normalise_u8, synth_state_dict, synth_tile_family
from keep_amd.wsi_evaluation import segment_utils
from keep_amd.wsi_evaluation.utils import WSI_Classification_Dataset
from oracle import keep_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RULE = TissueRule(sat_min=20, min_fraction=0.25)
FAMILIES = ("he_crops", "stain_field", "background", "half")


def mosaic(rows, cols, seed=11):
    """uint8 [rows*224, cols*224, 3] on the host: tile (r, c) of a family drawn per tile, background over a third of the slide."""
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
    return mosaic(6, 7)                          # 1344 x 1568


@pytest.fixture(scope="module")
def small():
    return synth_state_dict(small_shape(2, 2), seed=5)


def make_model(sd, precision="comp"):
    m = KEEPModel(precision=precision)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def models(small):
    return {p: make_model(small, p) for p in ("comp", "strict")}


@pytest.fixture(scope="module")
def text_bank():
    g = torch.Generator().manual_seed(99)
    return F.normalize(torch.randn(64, 768, generator=g), dim=-1)


def want_coords(region_np, patch, step, tissue, origin=(0, 0), scale=1):
    sat_min, min_pixels = tissue_params(tissue, patch)
    cells = region_grid_numpy(region_np, patch, step, sat_min, min_pixels)
    return (cells + np.asarray(origin, np.int64)) * scale


def host_cut(region_np, xy, patch):
    x, y = int(xy[0]), int(xy[1])
    return region_np[y:y + patch, x:x + patch, :3]


# ------------------------------------------------------------------------------------------------ grid
@pytest.mark.parametrize("patch,step", [(224, None), (256, None), (256, 131), (100, 157), (16, 16), (512, 200)])
@pytest.mark.parametrize("tissue", [None, RULE])
def test_grid_matches_numpy(models, slide, patch, step, tissue):
    m = models["comp"]
    region = slide[5:, 3:]                                   # grid and tiles out of phase
    got = m.region_grid(torch.from_numpy(np.ascontiguousarray(region)).to(DEV), patch, step, tissue)
    assert got.device.type == "cuda" and got.dtype == torch.int64
    want = want_coords(region, patch, step, tissue)
    assert np.array_equal(got.cpu().numpy(), want)
    if tissue is not None and patch == 256 and step is None:
        full = want_coords(region, patch, step, None)
        assert 0 < len(want) < len(full)                    # glass was dropped, tissue kept


def test_grid_strided_view_rgba_origin_scale(models, slide):
    m = models["comp"]
    big = torch.from_numpy(slide).to(DEV)
    view = big[37:37 + 1000, 51:51 + 1300]                  # row stride 1568 * 3 bytes, origin byte-unaligned
    assert not view.is_contiguous()
    region = slide[37:37 + 1000, 51:51 + 1300]
    for tissue in (None, RULE, (0, 0.9), (60, 0.05)):
        want = want_coords(region, 224, 111, tissue, origin=(3000, 4000), scale=4)
        got = m.region_grid(view, 224, 111, tissue, origin=(3000, 4000), coord_scale=4)
        assert np.array_equal(got.cpu().numpy(), want), tissue
        # host input: the same coords, returned on the host
        assert np.array_equal(m.region_grid(region, 224, 111, tissue, origin=(3000, 4000), coord_scale=4).numpy(), want)
    alpha = torch.randint(0, 256, slide.shape[:2] + (1,), dtype=torch.uint8, device=DEV)
    rgba = torch.cat([big, alpha], 2)
    rgba_view = rgba[37:37 + 1000, 51:51 + 1300]
    for tissue in (None, RULE):
        assert torch.equal(m.region_grid(rgba_view, 224, 111, tissue).cpu(), torch.from_numpy(want_coords(region, 224, 111, tissue)))


def test_no_tissue_and_region_smaller_than_a_patch(models):
    m = models["comp"]
    g = torch.Generator(device=DEV).manual_seed(3)
    region = torch.full((672, 896, 3), 240, dtype=torch.int16, device=DEV)       # glass: near-white with per-channel noise ...
    region += torch.randint(-3, 4, region.shape, dtype=torch.int16, device=DEV, generator=g)
    region[:, 300:420] = 128                                                     # ... a flat grey band and a black one
    region[400:500] = 0
    region = region.to(torch.uint8)
    assert m.region_grid(region, 224, None, None).shape == (12, 2)
    for tissue in (RULE, (20, 0.05)):
        c = m.region_grid(region, 224, None, tissue)
        assert c.shape == (0, 2) and c.dtype == torch.int64
        f, c = m.encode_region(region, 224, None, tissue)
        assert f.shape == (0, 768) and c.shape == (0, 2) and f.dtype == torch.float32
    tiny = torch.full((100, 300, 3), 128, dtype=torch.uint8, device=DEV)
    for p in (224, 101):
        assert m.region_grid(tiny, p).shape == (0, 2)
        f, c = m.encode_region(tiny, p)
        assert f.shape == (0, 768) and c.shape == (0, 2)
    assert m.region_grid(tiny, 100).tolist() == [[0, 0], [100, 0], [200, 0]]


# ------------------------------------------------------------------------------------------------ patches
def test_patches_224_are_the_host_cut(models, slide):
    m = models["comp"]
    big = torch.from_numpy(slide).to(DEV)
    view = big[29:29 + 1100, 13:13 + 1400]
    region = slide[29:29 + 1100, 13:13 + 1400]
    alpha = torch.randint(0, 256, slide.shape[:2] + (1,), dtype=torch.uint8, device=DEV)
    rgba_view = torch.cat([big, alpha], 2)[29:29 + 1100, 13:13 + 1400]
    coords = m.region_grid(view, 224, 97, RULE, origin=(10, 20), coord_scale=2)
    assert coords.shape[0] > 8
    want = np.stack([host_cut(region, (x // 2 - 10, y // 2 - 20), 224) for x, y in coords.cpu().tolist()])
    for src in (view, rgba_view, region):
        got = m.region_patches_uint8(src, coords, 224, origin=(10, 20), coord_scale=2)
        assert got.shape == (coords.shape[0], 224, 224, 3) and got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("patch", [256, 448, 512])
def test_patches_resized_match_pil_integer_resample(models, slide, patch):
    m = models["comp"]
    big = torch.from_numpy(slide).to(DEV)
    alpha = torch.randint(0, 256, slide.shape[:2] + (1,), dtype=torch.uint8, device=DEV)
    rgba_view = torch.cat([big, alpha], 2)[7:, 5:]
    region = slide[7:, 5:]
    coords = m.region_grid(rgba_view, patch, patch // 2 + 1, RULE)
    pick = coords[torch.linspace(0, coords.shape[0] - 1, 5).long()]
    got = m.region_patches_uint8(rgba_view, pick, patch)
    assert got.shape == (5, 224, 224, 3)
    for i, (x, y) in enumerate(pick.cpu().tolist()):
        want = resize_bicubic_u8_numpy(host_cut(region, (x, y), patch), 224, 224)
        assert np.array_equal(got[i].cpu().numpy(), want), (patch, x, y)
    # the same as resize_crop_uint8 on the host-cut patches (the existing device path)
    cut = torch.from_numpy(np.stack([host_cut(region, xy, patch) for xy in pick.cpu().tolist()])).to(DEV)
    assert torch.equal(m.resize_crop_uint8(cut), got)


def test_patch_outside_the_region_is_an_error(models, slide):
    m = models["comp"]
    region = torch.from_numpy(slide[:600, :700]).to(DEV)
    for bad in ([[700 - 223, 0]], [[0, 600 - 223]], [[-1, 0]], [[0, -5]], [[2 ** 40, 0]]):
        with pytest.raises(ValueError, match="outside|cell"):
            m.region_patches_uint8(region, torch.tensor(bad), 224)
        with pytest.raises(ValueError):
            m.region_patches_uint8(region, torch.tensor(bad), 256)
    assert m.region_patches_uint8(region, torch.tensor([[700 - 224, 600 - 224]]), 224).shape == (1, 224, 224, 3)


# ------------------------------------------------------------------------------------------------ encode
def batched_reference(m, region, coords, patch, batch, origin=(0, 0), scale=1):
    return torch.cat([m.encode_image_uint8(m.region_patches_uint8(region, coords[i:i + batch], patch, origin, scale))
                      for i in range(0, coords.shape[0], batch)])


@pytest.mark.parametrize("patch,step,batch", [(224, None, 256), (224, 150, 7), (256, None, 5), (300, 260, 16)])
def test_encode_region_is_encode_image_uint8_of_its_patches(models, slide, patch, step, batch):
    for prec in ("comp", "strict"):
        m = models[prec]
        region = torch.from_numpy(slide).to(DEV)[11:, 17:]
        f, c = m.encode_region(region, patch, step, RULE, origin=(100, 200), coord_scale=2, batch=batch)
        assert torch.equal(c, m.region_grid(region, patch, step, RULE, origin=(100, 200), coord_scale=2))
        ref = batched_reference(m, region, c, patch, batch, (100, 200), 2)
        assert f.shape == (c.shape[0], 768) and torch.equal(f, ref), prec


def test_encode_region_depth2_vs_oracle(models, small, slide, text_bank):
    region = torch.from_numpy(slide).to(DEV)
    sd_dev = {k: v.to(DEV) for k, v in small.items() if k.startswith("visual")}
    for patch in (224, 256):
        for prec, tol in (("comp", 1e-4), ("strict", 2e-6)):
            m = models[prec]
            f, c = m.encode_region(region, patch, None, RULE, batch=9)
            tiles = m.region_patches_uint8(region, c, patch)
            with torch.no_grad():
                ref = torch.cat([O.encode_image(sd_dev, normalise_u8(tiles[i:i + 8])) for i in range(0, tiles.shape[0], 8)]).cpu()
            dcos = (f.cpu() @ text_bank.t() - ref @ text_bank.t()).abs().max().item()
            print(f"[region depth 2 p={patch} {prec}] {c.shape[0]} tiles, max|dcos| vs oracle = {dcos:.3e}")
            assert dcos < tol


def test_encode_region_full_depth(slide, text_bank):
    sd = synth_state_dict(KEEPShape(), seed=0)
    m = KEEPModel(KEEPShape())
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    region = torch.from_numpy(slide).to(DEV)[:900, :1200]
    f, c = m.encode_region(region, 256, None, RULE, batch=8)
    assert 4 <= c.shape[0] <= 16
    assert torch.equal(f, batched_reference(m, region, c, 256, 8))
    sd_dev = {k: v.to(DEV) for k, v in sd.items() if k.startswith("visual")}
    with torch.no_grad():
        ref = O.encode_image(sd_dev, normalise_u8(m.region_patches_uint8(region, c, 256))).cpu()
    dcos = (f.cpu() @ text_bank.t() - ref @ text_bank.t()).abs().max().item()
    print(f"[region full depth p=256 comp] {c.shape[0]} tiles, max|dcos| vs oracle = {dcos:.3e}")
    assert dcos < 1e-4


# ------------------------------------------------------------------------------------------------ 64-bit offsets
def test_region_over_2gb_last_row_of_patches(models):
    m = models["comp"]
    W, H = 16384, 44000                                       # 2.16e9 bytes > 2^31
    assert H * W * 3 > 2 ** 31
    region = torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    y_rand = H - 600
    region[y_rand:] = torch.randint(0, 256, (600, W, 3), dtype=torch.uint8, device=DEV, generator=g)
    region[y_rand:, ::3] = 250                                 # some glass between the noise
    ys = (((H - 224) // 224) - 3) * 224                       # the last four grid rows
    tail = region[ys:].cpu().numpy()
    for patch, tissue in ((224, RULE), (256, RULE), (224, None)):
        got = m.region_grid(region, patch, None, tissue).cpu().numpy()
        if tissue is None:
            assert got.shape[0] == (H // patch) * (W // patch)
            continue
        ys_p = ((ys + patch - 1) // patch) * patch              # first grid row at or below ys
        want = region_grid_numpy(tail[ys_p - ys:], patch, None, *tissue_params(tissue, patch)) + np.array([0, ys_p])
        assert got.shape[0] > 0 and np.array_equal(got, want)
        last = got[got[:, 1] == got[:, 1].max()]
        pick = torch.from_numpy(last[np.linspace(0, len(last) - 1, 6).astype(int)])
        tiles = m.region_patches_uint8(region, pick, patch).cpu().numpy()
        for i, (x, y) in enumerate(pick.tolist()):
            cut = tail[y - ys:y - ys + patch, x:x + patch]
            assert np.array_equal(tiles[i], cut if patch == 224 else resize_bicubic_u8_numpy(cut, 224, 224)), (patch, x, y)
    del region
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ slide -> feature file
def test_extract_slide_features(models, slide, tmp_path, monkeypatch):
    m = models["strict"]
    H, W = slide.shape[:2]
    rgba = np.concatenate([slide, np.full((H, W, 1), 255, np.uint8)], 2)
    reads = []

    def read_region(x, y, w, h):
        reads.append((x, y, w, h))
        return rgba[y:y + h, x:x + w]

    saved = {}
    real_save = cohort.save_slide_features

    def spy(data_source, slide_id, features, coords=None, use_h5=False):
        saved["coords"] = np.asarray(coords)
        return real_save(data_source, slide_id, features, coords, use_h5)

    monkeypatch.setattr(cohort, "save_slide_features", spy)
    path = cohort.extract_slide_features(read_region, W, H, "slide_a", str(tmp_path), patch_size=256, step=200, tissue=RULE,
                                         band_rows=4, coord_scale=2, model=m)
    assert path == os.path.join(str(tmp_path), "pt_files", "slide_a.pt") and os.path.exists(path)
    assert len(reads) == 2                                    # 6 grid rows in bands of 4: 4 + 2
    feats = torch.load(path)
    f1, c1 = m.encode_region(torch.from_numpy(slide).to(DEV), 256, 200, RULE, coord_scale=2)
    assert np.array_equal(saved["coords"], c1.cpu().numpy())
    assert feats.shape == f1.shape and feats.dtype == torch.float32
    # per band, the file holds exactly what encode_region gives; across bands the batches differ, so rounding may too
    per_band = torch.cat([m.encode_region(torch.from_numpy(rgba[y:y + h]).to(DEV), 256, 200, RULE, origin=(0, y), coord_scale=2)[0].cpu()
                          for _, y, _, h in reads])
    assert torch.equal(feats, per_band)
    assert (feats - f1.cpu()).abs().max().item() < 1e-5

    # the WSI functions run on what it wrote
    rows = [{"slide_id": "slide_a", "Diagnosis": "tumor"}]
    ds = WSI_Classification_Dataset(rows, str(tmp_path), use_h5=False, label_map={"tumor": 1})
    dl = torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False)
    cls2 = F.normalize(torch.randn(768, 2, generator=torch.Generator().manual_seed(3)), dim=0).to(DEV)
    seg, _ = segment_utils.run(cls2, dl, DEV)
    assert seg["slide_a"].shape == (feats.shape[0], 2)
    probs = wsi.zero_shot_segment_probs(cls2, feats.to(DEV), saved["coords"], patch_size=512, model=m)
    assert len(probs) == feats.shape[0]


# ------------------------------------------------------------------------------------------------ the C ABI's argument checks
def test_abi_rejects_bad_arguments(models):
    m = models["comp"]
    lib, h, st = _lib.load(), m._handle, _stream(torch.device(DEV))
    H, W = 300, 400
    region = torch.zeros((H, W, 4), dtype=torch.uint8, device=DEV)
    cells = torch.zeros((256, 2), dtype=torch.int32, device=DEV)            # >= the 9 x 12 cells of the one valid call
    n = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = torch.empty((1, 224, 224, 3), dtype=torch.uint8, device=DEV)
    from keep_amd.region import resize_tables
    xb, xk, xks = resize_tables(256, m._device)

    def grid(region_p=_ptr(region), Hh=H, Ww=W, row=W * 4, ps=4, patch=32, step=32, sat=0, minp=0, cell_p=_ptr(cells), n_p=_ptr(n)):
        return lib.keep_region_grid(h, region_p, Hh, Ww, row, ps, patch, step, sat, minp, cell_p, n_p, st)

    assert grid() == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert int(n.item()) == ((H - 32) // 32 + 1) * ((W - 32) // 32 + 1) <= cells.shape[0]
    for kw in [dict(patch=15), dict(step=0), dict(step=-3), dict(ps=2), dict(ps=5), dict(row=W * 4 - 1), dict(ps=3, row=W * 3 - 1),
               dict(sat=256), dict(sat=-1), dict(minp=32 * 32 + 1), dict(minp=-1), dict(region_p=C.c_void_p(0)), dict(Hh=0), dict(Ww=0),
               dict(cell_p=C.c_void_p(0)), dict(n_p=C.c_void_p(0))]:
        assert grid(**kw) == _lib.KEEP_EINVAL, kw
        assert lib.keep_last_error(h)
    # a region smaller than one patch: N = 0, no error
    n.fill_(7)
    assert grid(patch=301) == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert int(n.item()) == 0

    def patches(cxy, B=1, patch=224, ps=4, row=W * 4, tables=True):
        c = torch.tensor(cxy, dtype=torch.int32, device=DEV).reshape(-1, 2)
        t = (_ptr(xb), _ptr(xk), xks) if tables else (C.c_void_p(0), C.c_void_p(0), 0)
        return lib.keep_region_patches_u8(h, _ptr(region), H, W, row, ps, _ptr(c), B, patch, *t, *t, _ptr(out), st)

    assert patches([0, 0]) == _lib.KEEP_OK and patches([W - 224, H - 224]) == _lib.KEEP_OK
    assert patches([W - 256, H - 256], patch=256) == _lib.KEEP_OK
    for args, kw in [([W - 223, 0], {}), ([0, H - 223], {}), ([-1, 0], {}), ([0, -1], {}), ([W - 255, 0], dict(patch=256)),
                     ([0, 0], dict(patch=15)), ([0, 0], dict(ps=2)), ([0, 0], dict(row=W * 4 - 1)), ([0, 0], dict(B=-1)),
                     ([0, 0], dict(patch=256, tables=False)), ([0, 0], dict(patch=301))]:
        assert patches(args, **kw) == _lib.KEEP_EINVAL, (args, kw)
        assert lib.keep_last_error(h)
    torch.cuda.synchronize()
