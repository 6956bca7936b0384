"""Region shape on the MI355X: keep_regions_moments / keep_regions_feret, KEEPModel.region_shape and the
isolated-tumour-cell rule of KEEPModel.evaluation_mask / wsi.eval_seg_froc.

Everything the device computes is an integer, so every comparison is exact: the yardstick is keep_amd.morphometry.shape_numpy, which
tests/test_region_shape.py holds to per-pixel loops, to a brute force over every corner and to scipy's convex hull."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel, _lib, wsi
from keep_amd.components import COLUMNS, NCOLS, RegionTable, regions_numpy
from keep_amd.config import small_shape
from keep_amd.lesion import LesionCandidates, froc_numpy, lesion_hits_numpy
from keep_amd.model import _ptr, _stream
from keep_amd.morphometry import RegionShape, shape_numpy
from keep_amd.region import TissueMask, TissueSegmentation, tissue_mask_numpy
from keep_amd.synth import synth_state_dict
from test_regions import MASKS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COL = {name: i for i, name in enumerate(COLUMNS)}


@pytest.fixture(scope="module")
def model():
    m = KEEPModel(precision="strict")
    m.load_state_dict(synth_state_dict(small_shape(2, 2), seed=5), strict=True)
    return m.to(DEV).eval()


def same(t: torch.Tensor, a: np.ndarray) -> bool:
    return t.dtype == torch.from_numpy(a).dtype and tuple(t.shape) == a.shape and torch.equal(t.cpu(), torch.from_numpy(a))


def check_mask(model, img, connectivity=8, min_area=1, feret=True) -> RegionShape:
    """mask_regions + region_shape on the device against regions_numpy + shape_numpy on the host."""
    regs = model.mask_regions(torch.from_numpy(np.ascontiguousarray(img)).to(DEV), connectivity, min_area)
    labels, table = regions_numpy(img, connectivity, min_area)
    assert same(regs.table, table)
    sh = model.region_shape(regs, feret=feret)
    moments, want = shape_numpy(labels, table, feret)
    assert sh.moments.device == torch.device(DEV) and same(sh.moments, moments)
    assert (sh.feret is None and want is None) if not feret else same(sh.feret, want)
    return sh


def callers_table(model, labels: np.ndarray, n: int) -> RegionTable:
    """keep_regions_table on a caller's own label image."""
    lab = torch.from_numpy(labels).to(DEV)
    table = torch.empty((n, NCOLS), dtype=torch.int64, device=DEV)
    model._call("regions_table", _ptr(lab), labels.shape[0], labels.shape[1], n, _ptr(None), _ptr(table))
    return RegionTable(table, lab)


@pytest.mark.parametrize("name,img", MASKS, ids=[n for n, _ in MASKS])
def test_masks_match_the_restatement(model, name, img):
    for connectivity, min_area in itertools.product((4, 8), (1, 50)):
        check_mask(model, img, connectivity, min_area)


def test_the_golden_crop(model, golden_dir):
    Image = pytest.importorskip("PIL.Image")
    rgb = np.asarray(Image.open(golden_dir + "/example.tif"))
    img = tissue_mask_numpy(rgb, TissueSegmentation(use_otsu=True, min_hole=64, min_area=400))[0]
    for connectivity, min_area in itertools.product((4, 8), (1, 50)):
        assert check_mask(model, img, connectivity, min_area).n > 0


def test_odd_shape_75_by_211(model):
    g = np.random.default_rng(75)
    blocks = np.kron(g.random((16, 31)) < 0.55, np.ones((5, 7), np.uint8))[:75, :211].astype(np.uint8)     # neither 4 rows nor 64 columns divide it
    for connectivity in (4, 8):
        assert check_mask(model, blocks, connectivity).n > 3
    check_mask(model, (g.random((75, 211)) < 0.5).astype(np.uint8), 8)


@pytest.mark.parametrize("h,w", [(1, 300), (300, 1)])
def test_one_pixel_wide(model, h, w):
    img = np.ones((h, w), np.uint8)
    img[min(h - 1, 100):min(h, 103), min(w - 1, 100):min(w, 103)] = 0
    sh = check_mask(model, img, 4)
    assert sh.d2.tolist() == [100 * 100 + 1, 197 * 197 + 1]


def test_one_region_over_many_workgroups(model):
    sh = check_mask(model, np.ones((300, 517), np.uint8), 4)
    assert sh.feret.tolist() == [[300 * 300 + 517 * 517, 0, 0, 517, 300]]
    assert sh.moments.tolist() == [[300 * (516 * 517 * 1033 // 6), 517 * (299 * 300 * 599 // 6), (516 * 517 // 2) * (299 * 300 // 2)]]


def test_checkerboard_of_one_pixel_regions(model):
    checker = (np.indices((64, 131)).sum(0) % 2).astype(np.uint8)
    sh = check_mask(model, checker, 4)
    assert sh.n == 64 * 131 // 2 and bool((sh.d2 == 2).all()) and not bool(sh.moments.any())


def test_callers_labels(model):
    """Labels nobody carries, in the middle and at the end, values above n and below 0, and rows of a box that carry nothing."""
    labels = np.zeros((70, 150), np.int32)
    labels[1, 2:90] = labels[2, 40:60] = labels[9, 3:130] = labels[10, 100] = 1      # rows 3..8 of the box carry nothing
    labels[20:60, 15] = labels[20, 16:19] = labels[59, 10:15] = 3                     # label 2 is carried by nobody
    labels[65, 0:9] = 9
    labels[66, 0:9] = -4
    small = np.zeros((6, 9), np.int32)                                                # the trailing labels carried by nobody: 6 and 7 of 7
    small[1, 1:5], small[2, 0:6] = 1, 2
    small[4, 3:9] = small[5, 8] = 5
    tail = callers_table(model, small, 7)
    got, (moments, feret) = model.region_shape(tail), shape_numpy(small, tail.table.cpu().numpy())
    assert same(got.moments, moments) and same(got.feret, feret) and moments[[1, 4]].tolist() == [[55, 0, 0], [80, 1, 5]]
    assert not moments[[2, 3, 5, 6]].any() and not feret[[2, 3, 5, 6]].any()
    regs = callers_table(model, labels, 3)
    sh = model.region_shape(regs)
    moments, feret = shape_numpy(labels, regs.table.cpu().numpy())
    assert same(sh.moments, moments) and same(sh.feret, feret)
    assert sh.moments[1].tolist() == [0, 0, 0] and sh.feret[1].tolist() == [0] * 5
    # the entry points themselves, writing between guard rows: nothing lands outside rows 1..3
    mbuf, fbuf = (torch.full((5, c), 77, dtype=torch.int64, device=DEV) for c in (3, 5))
    model._call("regions_moments", _ptr(regs.labels), 70, 150, 3, _ptr(regs.table), _ptr(mbuf[1:4]))
    model._call("regions_feret", _ptr(regs.labels), 70, 150, 3, _ptr(regs.table), 1 << 30, _ptr(fbuf[1:4]), None)
    assert same(mbuf[1:4], moments) and same(fbuf[1:4], feret)
    assert bool((mbuf[[0, 4]] == 77).all()) and bool((fbuf[[0, 4]] == 77).all())
    assert sh.d2[0].item() == 128 ** 2 + 9 ** 2
    with pytest.raises(ValueError, match="label order"):
        model.region_shape(regs.sort("area"))
    with pytest.raises(ValueError, match="labels"):
        model.region_shape(RegionTable(regs.table))
    model.check_errors()


def test_no_regions(model):
    regs = model.mask_regions(np.zeros((9, 70), np.uint8))
    sh = model.region_shape(regs)
    assert sh.n == 0 and tuple(sh.moments.shape) == (0, 3) and tuple(sh.feret.shape) == (0, 5) and sh.moments.dtype == torch.int64
    assert sh.axis_lengths().shape == (0, 2) and sh.feret_diameter().shape == (0,) and model.region_shape(regs, feret=False).feret is None


def test_wide_mask_beyond_float_and_32_bits(model):
    """40 x 100 000, one full region: sum_uu = 1.3e16 > 2^53 and d2 = 1e10 > 2^32."""
    h, w = 40, 100_000
    regs = model.mask_regions(torch.ones((h, w), dtype=torch.uint8, device=DEV), 4)
    sh = model.region_shape(regs)
    moments, feret = shape_numpy(np.ones((h, w), np.int32), regs.table.cpu().numpy())
    assert same(sh.moments, moments) and same(sh.feret, feret)
    assert sh.moments.tolist() == [[h * ((w - 1) * w * (2 * w - 1) // 6), w * ((h - 1) * h * (2 * h - 1) // 6), ((w - 1) * w // 2) * ((h - 1) * h // 2)]]
    assert sh.feret.tolist() == [[w * w + h * h, 0, 0, w, h]] and moments[0, 0] > 1 << 53 and feret[0, 0] > 1 << 32


def comb(teeth: int, tooth: int) -> np.ndarray:
    img = np.zeros((tooth + 3, 4 * teeth + 1), np.uint8)
    img[1, :] = 1
    img[1:tooth + 1, ::4] = 1
    img[tooth + 1, 8] = 1                                                      # one tooth is longer: the diameter ends on it
    return img


def spirals(n: int = 129, pitch: float = 12.0) -> np.ndarray:
    """Two interleaved spiral arms round the centre, a gap of pitch / 4 between them."""
    y, x = np.indices((n, n)) - n // 2
    r, theta = np.hypot(x, y), np.arctan2(y, x)
    arm = np.floor(((r / pitch - theta / (2 * np.pi)) % 1.0) * 4).astype(int)
    return (((arm == 0) | (arm == 2)) & (r >= pitch) & (r < n // 2)).astype(np.uint8)


def test_feret_candidate_choice_and_tie_rule(model):
    wide = comb(40, 9)
    assert wide.shape[1] > wide.shape[0]
    for img in (wide, np.ascontiguousarray(wide.T)):                           # the row choice and the column choice
        assert check_mask(model, img, 4).n == 1
    square = np.zeros((40, 90), np.uint8)
    square[3:36, 50:83] = 1
    assert check_mask(model, square, 8).feret.tolist() == [[2 * 33 * 33, 50, 3, 83, 36]]      # not the other diagonal
    line = np.zeros((70, 90), np.uint8)
    line[np.arange(5, 65), np.arange(5, 65) + 7] = 1
    assert check_mask(model, line, 8).feret.tolist() == [[2 * 60 * 60, 12, 5, 72, 65]]
    assert check_mask(model, line, 4).n == 60
    two = spirals()
    sh = check_mask(model, two, 8, 50)                                         # min_area drops the crumbs the rim cuts off the arms
    t = sh.table.numpy()
    assert sh.n == 2 and t[0, COL["x0"]] < t[1, COL["x1"]] and t[1, COL["x0"]] < t[0, COL["x1"]] and t[0, COL["y0"]] < t[1, COL["y1"]]


def test_two_calls_are_equal_and_max_pairs(model):
    g = np.random.default_rng(3)
    img = (g.random((90, 200)) < 0.6).astype(np.uint8)
    regs = model.mask_regions(img, 8)
    a, b = model.region_shape(regs), model.region_shape(regs)
    assert torch.equal(a.moments, b.moments) and torch.equal(a.feret, b.feret)
    lines = torch.minimum(regs.x1 - regs.x0, regs.y1 - regs.y0)
    candidates, pairs = int(4 * lines.sum()), int((8 * lines * lines).sum())
    assert model.last_feret_totals == (candidates, pairs)
    with pytest.raises(ValueError, match="max_pairs"):
        model.region_shape(regs, max_pairs=pairs - 1)
    assert model.last_feret_totals == (candidates, pairs)
    assert torch.equal(model.region_shape(regs, max_pairs=pairs).feret, a.feret)        # the cap itself is allowed, and a following call works
    assert model.region_shape(regs, feret=False, max_pairs=0).feret is None
    model.check_errors()


def test_c_abi_argument_checks(model):
    lib, h, st = _lib.load(), model._handle, _stream(torch.device(DEV))
    H, W = 12, 70
    labels = torch.ones((H, W), dtype=torch.int32, device=DEV)
    table = torch.tensor([[0, 0, H * W, 0, 0, W, H, 0, 0, 1, 0, 0, 0, 0]], dtype=torch.int64, device=DEV)
    moments, feret = torch.zeros((2, 3), dtype=torch.int64, device=DEV), torch.zeros((2, 5), dtype=torch.int64, device=DEV)
    totals, null = (C.c_int64 * 2)(7, 7), C.c_void_p(0)

    def off(t, nbytes):
        return C.c_void_p(t.data_ptr() + nbytes)

    def mom(l=_ptr(labels), Hh=H, Ww=W, n=1, t=_ptr(table), m=_ptr(moments)):
        return lib.keep_regions_moments(h, l, Hh, Ww, n, t, m, st)

    def fer(l=_ptr(labels), Hh=H, Ww=W, n=1, t=_ptr(table), cap=1 << 20, f=_ptr(feret), tot=totals):
        return lib.keep_regions_feret(h, l, Hh, Ww, n, t, cap, f, tot, st)

    assert mom() == _lib.KEEP_OK and fer() == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert moments[0].tolist() == [H * (W - 1) * W * (2 * W - 1) // 6, W * (H - 1) * H * (2 * H - 1) // 6, (W - 1) * W // 2 * ((H - 1) * H // 2)]
    assert feret[0].tolist() == [W * W + H * H, 0, 0, W, H] and list(totals) == [4 * H, 8 * H * H]
    for kw in [dict(l=null), dict(l=off(labels, 2)), dict(t=null), dict(t=off(table, 4)), dict(m=null), dict(m=off(moments, 4)), dict(Hh=0), dict(Ww=-2),
               dict(Hh=1 << 16, Ww=(1 << 14) + 1), dict(n=-1), dict(n=H * W + 1)]:
        assert mom(**kw) == _lib.KEEP_EINVAL, kw
        assert lib.keep_last_error(h)
    for kw in [dict(l=null), dict(t=null), dict(t=off(table, 4)), dict(f=null), dict(f=off(feret, 4)), dict(Hh=0), dict(Hh=1, Ww=1 << 30), dict(n=-1),
               dict(n=H * W + 1), dict(cap=-1), dict(cap=(1 << 50) + 1), dict(cap=8 * H * H - 1)]:
        assert fer(**kw) == _lib.KEEP_EINVAL, kw
        assert lib.keep_last_error(h)
    assert list(totals) == [4 * H, 8 * H * H]                   # the call over max_pairs still reports what it counted
    assert mom(n=0, t=null, m=null) == _lib.KEEP_OK and fer(n=0, t=null, f=null, tot=None) == _lib.KEEP_OK      # nothing to write is no error
    assert fer(cap=8 * H * H, tot=None) == _lib.KEEP_OK
    # a table that is not the labels' own: boxes outside the image have no lines, and a box inside it that the pixels overrun drops them
    bad = torch.tensor([[0, 0, 1, -5, -5, 1 << 40, 3, 0, 0, 0, 0, 0, 0, 0], [0, 0, 1, 10, 2, 20, 6, 0, 0, 0, 0, 0, 0, 0]], dtype=torch.int64, device=DEV)
    labels[:, 35:] = 2
    assert fer(n=2, t=_ptr(bad)) == _lib.KEEP_OK and mom(n=2, t=_ptr(bad)) == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert feret[0].tolist() == [0] * 5 and list(totals) == [16, 128]
    assert moments[0, 1].item() == 35 * (H - 1) * H * (2 * H - 1) // 6      # wrong rows, but sums of an origin held inside the image
    assert lib.keep_regions_moments(None, _ptr(labels), H, W, 1, _ptr(table), _ptr(moments), st) == _lib.KEEP_EINVAL
    assert lib.keep_regions_feret(None, _ptr(labels), H, W, 1, _ptr(table), 1, _ptr(feret), None, st) == _lib.KEEP_EINVAL
    model.check_errors()


# ------------------------------------------------------------------------------------------------ the isolated-tumour-cell rule
D, MARGIN, T = 4, 1.5, 35.0


def lesion_truth() -> np.ndarray:
    """A 3-pixel speck, a long thin lesion (30 x 1: 32 x 3 once dilated, so its box is shorter than T and its major axis longer)
    and a blob."""
    truth = np.zeros((100, 140), np.uint8)
    truth[10, 10:13] = 1
    truth[30, 20:50] = 1
    truth[50:85, 70:110] = 1
    truth[60:70, 80:90] = 0                                                   # a hole, which the evaluation mask fills
    return truth


def host_evaluation_mask(truth):
    ndimage = pytest.importorskip("scipy.ndimage")
    grown = ndimage.distance_transform_edt(truth == 0) < MARGIN
    return ndimage.binary_fill_holes(grown).astype(np.uint8)


def test_evaluation_mask_by_major_axis(model):
    truth = lesion_truth()
    labels, table = regions_numpy(host_evaluation_mask(truth), 8, 1)
    moments, _ = shape_numpy(labels, table, feret=False)
    major = RegionShape(torch.from_numpy(moments), None, RegionTable(torch.from_numpy(table))).axis_lengths()[:, 0]
    by_axis = (major < T).astype(np.uint8)
    by_box = (np.maximum(table[:, COL["x1"]] - table[:, COL["x0"]], table[:, COL["y1"]] - table[:, COL["y0"]]) < T).astype(np.uint8)
    assert by_axis.tolist() == [1, 0, 0] and by_box.tolist() == [1, 1, 0]     # the thin lesion: the two rules differ
    em = model.evaluation_mask(TissueMask(truth, D), MARGIN, ignore_major_axis=T)
    assert em.n == 3 and same(em.labels, labels) and same(em.ignore, by_axis)
    # the bounding-box rule, with no new keyword: the code path as it was (test_the_box_rule_is_what_it_was holds it to the restatement
    # that was there before)
    old = model.evaluation_mask(TissueMask(truth, D), MARGIN, ignore_max_extent=T)
    assert old.n == 3 and same(old.labels, labels) and same(old.ignore, by_box) and same(old.table.table, table)
    none = model.evaluation_mask(TissueMask(truth, D), MARGIN)
    assert none.ignore.tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="not both"):
        model.evaluation_mask(TissueMask(truth, D), MARGIN, ignore_max_extent=T, ignore_major_axis=T)

    # FROC with the rule: detections on a grid, scored by position
    ys, xs = np.meshgrid(np.arange(2, 100, 7), np.arange(2, 140, 7), indexing="ij")
    xy = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.int64) * D + 1
    g = np.random.default_rng(9)
    scores = g.choice(np.array([0.2, 0.55, 0.7, 0.9], np.float32), len(xy))
    want = froc_numpy([lesion_hits_numpy(xy, scores, labels, D, (0, 0), 3, by_axis)])
    cands = LesionCandidates(torch.from_numpy(xy).to(DEV), torch.from_numpy(scores).to(DEV))
    got = wsi.eval_seg_froc([(cands, TissueMask(truth, D))], margin_px=MARGIN, ignore_major_axis=T, model=model)
    assert got == want and want.n_lesions == 2
    boxed = wsi.eval_seg_froc([(cands, TissueMask(truth, D))], margin_px=MARGIN, ignore_max_extent=T, model=model)
    assert boxed == froc_numpy([lesion_hits_numpy(xy, scores, labels, D, (0, 0), 3, by_box)]) and boxed.n_lesions == 1


def test_the_box_rule_is_what_it_was(model):
    """``ignore_max_extent`` and no new keyword: the same call on unchanged code, against the restatement lesion scoring already had.
    keep_amd.lesion holds none of the evaluation mask; the existing one is ``host_evaluation_mask`` of tests/test_lesion_gpu.py (scipy's
    distance transform, hole filling, labelling and ``find_objects``), used here on that file's own slides."""
    import test_lesion_gpu as L
    for k in range(2):
        polys = L.slide_polys(k)
        labels, n, ignore = L.host_evaluation_mask(polys, 8)
        em = model.evaluation_mask(polys, L.MARGIN, ignore_max_extent=8, downsample=L.D, shape=L.SHAPE)
        assert em.n == n and same(em.labels, labels) and same(em.ignore, ignore) and 0 < ignore.sum() < n
