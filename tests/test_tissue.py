"""The thumbnail tissue segmentation and the grid on a mask, host side: keep_amd.region's numpy restatements
(the yardsticks of tests/test_tissue_gpu.py), Otsu's threshold in exact integers, the argument checks and the planner of a masked
extraction.  No GPU.

The restatement is held to an independent scipy composition where scipy is installed; the union-find the connected-components
kernels run (tissue.hip: run starts inside 64-pixel segments, the reduced set of joins, roots = smallest pixel index) is restated
here step by step and held to scipy's labels too, so that the set of joins the kernel skips is proven sufficient before it runs."""
import numpy as np
import pytest
import torch

from keep_amd.region import (MASK_MODES, TissueMask, TissueSegmentation, close_numpy, label_numpy, mask_grid_numpy, median_numpy,
                             otsu_threshold, plan_bands, plan_mask_reads, saturation_numpy, tissue_mask_numpy)
from keep_amd.synth import synth_thumbnail


# ------------------------------------------------------------------------------------------------ the restatement against scipy
def scipy_mask(rgb, p):
    ndi = pytest.importorskip("scipy.ndimage")
    c = rgb[..., :3].astype(np.int64)
    mx, mn = c.max(2), c.min(2)
    s = np.where(mx > 0, (2 * 255 * (mx - mn) + mx) // (2 * np.maximum(mx, 1)), 0).astype(np.uint8)
    m = ndi.median_filter(s, size=p.mthresh, mode="nearest")
    t = otsu_threshold(np.bincount(m.ravel(), minlength=256)) if p.use_otsu else p.sthresh
    b = (m > t).astype(np.uint8)
    if p.close:
        # scipy's window of size c at origin 0 is [x - c // 2, x + c - 1 - c // 2]: the specification's, for even c too
        b = ndi.maximum_filter(b, size=p.close, mode="constant", cval=0)
        b = ndi.minimum_filter(b, size=p.close, mode="constant", cval=1)
    lab, n = ndi.label(b == 0, structure=ndi.generate_binary_structure(2, 1))
    area = np.bincount(lab.ravel(), minlength=n + 1)
    border = np.zeros(n + 1, bool)
    for e in (lab[0], lab[-1], lab[:, 0], lab[:, -1]):
        border[e] = True
    fill = ~border & (area <= p.min_hole)
    fill[0] = False
    b = b | fill[lab]
    lab, n = ndi.label(b, structure=np.ones((3, 3)))
    keep = np.bincount(lab.ravel(), minlength=n + 1) > p.min_area
    keep[0] = False
    return keep[lab].astype(np.uint8), t


CASES = [TissueSegmentation(), TissueSegmentation(use_otsu=True), TissueSegmentation(min_hole=200),
         TissueSegmentation(mthresh=1, close=0, min_hole=0, min_area=0), TissueSegmentation(mthresh=3, close=3, min_hole=64, min_area=400),
         TissueSegmentation(mthresh=15, close=4, min_hole=200, use_otsu=True), TissueSegmentation(mthresh=5, close=7, min_area=0),
         TissueSegmentation(mthresh=7, close=31, min_hole=10 ** 9, min_area=1)]


@pytest.mark.parametrize("p", CASES, ids=lambda p: f"k{p.mthresh}-c{p.close}-o{int(p.use_otsu)}-h{p.min_hole}-a{p.min_area}")
def test_restatement_matches_scipy(p):
    for rgb in (synth_thumbnail(), synth_thumbnail(97, 131, seed=5)):
        want, t_want = scipy_mask(rgb, p)
        got, t = tissue_mask_numpy(rgb, p)
        assert t == t_want
        assert got.dtype == np.uint8 and np.array_equal(got, want)


def test_restatement_on_the_golden_crop(golden_dir):
    Image = pytest.importorskip("PIL.Image")
    rgb = np.asarray(Image.open(golden_dir + "/example.tif"))
    p = TissueSegmentation(use_otsu=True, min_hole=64, min_area=400)
    st = {}
    got, t = tissue_mask_numpy(rgb, p, st)
    want, t_want = scipy_mask(rgb, p)
    assert t == t_want and np.array_equal(got, want)
    assert 0 < st["holes_filled"] and 0 < st["components_kept"] < st["components"] and 0 < got.sum() < got.size


def test_stages_by_hand():
    # saturation: rounded half up, 0 at black
    rgb = np.array([[[0, 0, 0], [255, 0, 0], [200, 100, 150], [3, 2, 3], [10, 10, 10], [1, 0, 0]]], np.uint8)
    want = [0, 255, (510 * 100 + 200) // 400, (510 * 1 + 3) // 6, 0, 255]
    assert saturation_numpy(rgb).tolist() == [want]
    assert saturation_numpy(np.concatenate([rgb, np.full((1, 6, 1), 77, np.uint8)], 2)).tolist() == [want]      # alpha ignored
    # median: border replicated
    img = np.array([[9, 1, 1], [1, 1, 1], [1, 1, 7]], np.uint8)
    assert median_numpy(img, 3).tolist() == [[1, 1, 1], [1, 1, 1], [1, 1, 1]]
    assert median_numpy(np.array([[5, 0, 0, 0, 9]], np.uint8), 3).tolist() == [[5, 0, 0, 0, 9]]
    assert median_numpy(img, 1) is not img and np.array_equal(median_numpy(img, 1), img)
    # closing with an even box is not symmetric: window [x - 1, x] for c = 2
    b = np.zeros((1, 8), np.uint8)
    b[0, [2, 4]] = 1
    assert close_numpy(b, 2).tolist() == [[0, 0, 0, 1, 1, 1, 0, 0]]   # both passes look left: the result moves right by one
    assert close_numpy(b, 3).tolist() == [[0, 0, 1, 1, 1, 0, 0, 0]]
    edge = np.zeros((1, 6), np.uint8)
    edge[0, 1] = 1
    assert close_numpy(edge, 3).tolist() == [[1, 1, 0, 0, 0, 0]]   # dilation reaches the border, erosion sees 1 outside
    assert close_numpy(b, 0).tolist() == b.tolist()


def test_label_numpy_by_hand():
    b = np.array([[1, 0, 1, 1],
                  [0, 1, 0, 0],
                  [0, 0, 0, 1]], np.uint8)
    lab4, a4 = label_numpy(b, conn8=False)
    assert a4[1:].tolist() == [1, 2, 1, 1] and len(np.unique(lab4)) == 5
    lab8, a8 = label_numpy(b, conn8=True)
    assert sorted(a8[1:].tolist()) == [1, 4] and lab8[0, 0] == lab8[1, 1] == lab8[0, 3] != lab8[2, 3]
    lab0, a0 = label_numpy(np.zeros((3, 4), np.uint8), conn8=True)
    assert not lab0.any() and a0.tolist() == [12]


# ------------------------------------------------------------------------------------------------ the kernel's union-find, restated
def kernel_labels(img, fg, conn8, seg=64):
    """tissue.hip's cc_init + cc_merge + cc_compress, sequentially: labels = smallest linear index of the component, -1 elsewhere."""
    h, w = img.shape
    act = (img != 0) == fg
    L = np.full(h * w, -1, np.int64)
    for y in range(h):
        for x in range(w):
            if act[y, x]:
                s = x
                while s % seg and act[y, s - 1]:
                    s -= 1
                L[y * w + x] = y * w + s

    def find(a):
        while L[a] != a:
            a = L[a]
        return a

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            L[max(a, b)] = min(a, b)
    for y in range(h):
        for x in range(w):
            if not act[y, x]:
                continue
            p = y * w + x
            lf = x > 0 and act[y, x - 1]
            if lf and x % seg == 0:
                union(p, p - 1)
            if y == 0:
                continue
            up, ul, ur = act[y - 1, x], x > 0 and act[y - 1, x - 1], x + 1 < w and act[y - 1, x + 1]
            if up and not (lf and ul):
                union(p, p - w)
            if conn8:
                if ul and not up and not lf:
                    union(p, p - w - 1)
                if ur and not up:
                    union(p, p - w + 1)
    return np.array([find(i) if L[i] >= 0 else -1 for i in range(h * w)]).reshape(h, w)


def spiral(n):
    """A one-pixel-wide square spiral in an n x n image (n odd): one long 4-connected path."""
    img = np.zeros((n, n), np.uint8)
    y = x = 0
    dy, dx = 0, 1
    img[0, 0] = 1
    while True:
        ny, nx = y + dy, x + dx
        ahead = 0 <= ny + dy < n and 0 <= nx + dx < n and img[ny + dy, nx + dx]
        if not (0 <= ny < n and 0 <= nx < n) or img[ny, nx] or ahead:
            dy, dx = dx, -dy
            ny, nx = y + dy, x + dx
            if not (0 <= ny < n and 0 <= nx < n) or img[ny, nx] or (0 <= ny + dy < n and 0 <= nx + dx < n and img[ny + dy, nx + dx]):
                break
        y, x = ny, nx
        img[y, x] = 1
    return img


def serpentine(h, w):
    img = np.zeros((h, w), np.uint8)
    img[::2] = 1
    img[1::4, -1] = 1
    img[3::4, 0] = 1
    return img


def hard_shapes():
    g = np.random.default_rng(0)
    yield "noise", (g.random((37, 150)) < 0.55).astype(np.uint8)
    yield "sparse", (g.random((40, 140)) < 0.3).astype(np.uint8)
    yield "checker", (np.indices((21, 133)).sum(0) % 2).astype(np.uint8)
    yield "spiral", spiral(71)
    yield "serpentine", serpentine(23, 131)
    yield "ones", np.ones((9, 130), np.uint8)
    yield "row", (g.random((1, 300)) < 0.7).astype(np.uint8)
    yield "column", (g.random((300, 1)) < 0.7).astype(np.uint8)
    d = np.zeros((6, 130), np.uint8)
    d[2, 63] = d[3, 64] = d[1, 64] = d[4, 63] = 1                # diagonal contacts across a segment border
    yield "diagonal", d


@pytest.mark.parametrize("name,img", list(hard_shapes()), ids=[n for n, _ in hard_shapes()])
def test_kernel_union_find_labels_are_the_components(name, img):
    ndi = pytest.importorskip("scipy.ndimage")
    for fg, conn8 in ((True, True), (False, False), (True, False), (False, True)):
        act = (img != 0) == fg
        lab, n = ndi.label(act, structure=np.ones((3, 3)) if conn8 else ndi.generate_binary_structure(2, 1))
        first = np.full(n + 1, np.iinfo(np.int64).max, np.int64)  # smallest linear index of every scipy component
        np.minimum.at(first, lab.ravel(), np.arange(img.size))
        want = np.where(act, first[lab], -1)
        assert np.array_equal(kernel_labels(img, fg, conn8), want), (name, fg, conn8)
    # and the numpy labelling of the restatement agrees with scipy on the same shapes
    for conn8 in (False, True):
        lab, n = ndi.label(img, structure=np.ones((3, 3)) if conn8 else ndi.generate_binary_structure(2, 1))
        mine, area = label_numpy(img, conn8)
        pairs = np.unique(np.stack([lab.ravel(), mine.ravel()]), axis=1)
        assert len(area) == n + 1 and pairs.shape[1] == len(np.unique(lab)) == len(np.unique(mine))     # a bijection of the labels
        assert np.array_equal(area, np.bincount(mine.ravel(), minlength=n + 1))


def test_spiral_and_serpentine_are_one_component():
    for img in (spiral(71), serpentine(23, 131)):
        _, area = label_numpy(img, conn8=False)
        assert len(area) == 2 and area[1] == img.sum()


# ------------------------------------------------------------------------------------------------ Otsu
def brute_otsu(hist):
    h = np.asarray(hist, np.float64)
    lv = np.arange(256, dtype=np.float64)
    best, bt = -1.0, 0
    for t in range(256):
        w0, w1 = h[:t + 1].sum(), h[t + 1:].sum()
        if w0 == 0 or w1 == 0:
            continue
        m0, m1 = (h[:t + 1] * lv[:t + 1]).sum() / w0, (h[t + 1:] * lv[t + 1:]).sum() / w1
        v = w0 * w1 * (m0 - m1) ** 2
        if v > best:
            best, bt = v, t
    return bt, best


def test_otsu_against_brute_force():
    g = np.random.default_rng(4)
    checked = 0
    for trial in range(40):
        lo, hi = sorted(g.integers(0, 256, 2))
        hist = np.zeros(256, np.int64)
        hist += (2000 * np.exp(-0.5 * ((np.arange(256) - lo) / g.uniform(2, 12)) ** 2)).astype(np.int64)
        hist += (g.integers(200, 3000) * np.exp(-0.5 * ((np.arange(256) - hi) / g.uniform(2, 20)) ** 2)).astype(np.int64)
        hist += g.integers(0, 5, 256)
        bt, best = brute_otsu(hist)
        # only where float64 separates the maximum from every other candidate
        vals = []
        for t in range(256):
            w0, w1 = hist[:t + 1].sum(), hist[t + 1:].sum()
            if w0 and w1:
                h = hist.astype(np.float64)
                m0 = (h[:t + 1] * np.arange(t + 1)).sum() / w0
                m1 = (h[t + 1:] * np.arange(t + 1, 256)).sum() / w1
                vals.append(w0 * w1 * (m0 - m1) ** 2)
        vals = np.sort(np.array(vals))
        if len(vals) > 1 and vals[-1] - vals[-2] <= 1e-9 * vals[-1]:
            continue
        assert otsu_threshold(hist) == bt, trial
        checked += 1
    assert checked >= 30


def test_otsu_degenerate_cases():
    one = [0] * 256
    one[77] = 1000
    assert otsu_threshold(one) == 0
    assert otsu_threshold([0] * 256) == 0
    two = [0] * 256
    two[10], two[200] = 5, 9
    assert otsu_threshold(two) == 10                             # every t in [10, 200) separates the same classes: the smallest
    sym = [0] * 256
    sym[0] = sym[1] = sym[2] = 7                                 # t = 0 and t = 1 tie exactly
    assert otsu_threshold(sym) == 0
    assert otsu_threshold(np.asarray(two, np.int32)) == 10       # a device histogram read back
    big = [0] * 256
    big[3], big[250] = 1 << 30, (1 << 30) - 1                    # products far beyond 64 bits
    assert otsu_threshold(big) == 3
    for bad in ([1] * 255, [-1] + [0] * 255):
        with pytest.raises(ValueError):
            otsu_threshold(bad)


# ------------------------------------------------------------------------------------------------ the grid on a mask
def loop_grid(mask, ds, H, W, p, step, origin, mode):
    out = []
    for y in range(0, H - p + 1, step):
        for x in range(0, W - p + 1, step):
            cx, cy, s = origin[0] + x + p // 2, origin[1] + y + p // 2, p // 4
            pts = [(cx, cy)] if mode == "center" else [(cx - s, cy - s), (cx + s, cy - s), (cx - s, cy + s), (cx + s, cy + s)]
            v = [px >= 0 and py >= 0 and py // ds < mask.shape[0] and px // ds < mask.shape[1] and bool(mask[py // ds, px // ds])
                 for px, py in pts]
            if all(v) if mode == "four_pt_hard" else any(v):
                out.append((x, y))
    return np.asarray(out, np.int64).reshape(-1, 2)


@pytest.mark.parametrize("mode", MASK_MODES)
@pytest.mark.parametrize("ds", [1, 16, 37])
def test_mask_grid_against_a_loop(mode, ds):
    g = np.random.default_rng(ds)
    H, W = 1900, 2300
    counts = []
    for origin in ((0, 0), (311, 97), (-150, -260)):
        # a mask smaller than the region at this origin: the far points fall outside it
        mh, mw = max(1, (origin[1] + H) * 3 // (4 * ds)), max(1, (origin[0] + W) * 3 // (4 * ds))
        blocks = g.random((mh // 8 + 1, mw // 8 + 1)) < 0.5
        mask = np.kron(blocks, np.ones((8, 8), bool))[:mh, :mw] if ds < 37 else g.random((mh, mw)) < 0.5
        for p, step in ((224, None), (256, 131), (512, 200), (16, 16)):
            got = mask_grid_numpy(mask, ds, H, W, p, step, origin, mode)
            want = loop_grid(mask, ds, H, W, p, step or p, origin, mode)
            assert got.dtype == np.int64 and np.array_equal(got, want), (origin, p, step)
            counts.append((len(want), ((H - p) // (step or p) + 1) * ((W - p) // (step or p) + 1)))
    assert any(0 < n < full for n, full in counts)
    assert mask_grid_numpy(np.ones((4, 4), bool), 16, 10, 10, 16, None).shape == (0, 2)       # region smaller than a cell
    with pytest.raises(ValueError):
        mask_grid_numpy(np.ones((4, 4), bool), 16, 100, 100, 16, None, mode="five_pt")


def test_modes_are_nested():
    g = np.random.default_rng(8)
    mask = np.kron(g.random((12, 15)) < 0.5, np.ones((4, 4), bool))
    n = {m: len(mask_grid_numpy(mask, 16, 760, 950, 64, 32, (5, 9), m)) for m in MASK_MODES}
    assert 0 < n["four_pt_hard"] < n["four_pt"] and n["four_pt_hard"] <= n["center"] <= n["four_pt"]


# ------------------------------------------------------------------------------------------------ argument checks
def test_argument_validation():
    for kw in [dict(mthresh=4), dict(mthresh=17), dict(mthresh=0), dict(mthresh=-3), dict(mthresh=True), dict(close=32), dict(close=-1),
               dict(min_area=-1), dict(min_hole=-1), dict(min_area=2.5), dict(sthresh=256), dict(sthresh=-1), dict(mode="five_pt"),
               dict(mode=None)]:
        with pytest.raises(ValueError):
            TissueSegmentation(**kw)
    p = TissueSegmentation()
    assert (p.mthresh, p.sthresh, p.use_otsu, p.close, p.min_area, p.min_hole, p.mode) == (7, 8, False, 4, 100, 16, "four_pt")
    assert TissueSegmentation.from_clam(64) == TissueSegmentation(min_area=100 * 64, min_hole=16 * 64)
    assert TissueSegmentation.from_clam(32, a_t=10, a_h=2, ref_patch_size=256, close=0).min_hole == 2 * 64
    ok = np.ones((5, 6), bool)
    for args in [(ok, 0), (ok, -2), (ok, 1.5), (ok, True), (ok[0], 4), (np.ones((2, 3, 1), np.uint8), 4), (ok.astype(np.float32), 4),
                 (ok.astype(np.int32), 4), (np.ones((0, 4), bool), 4), ([[1, 0]], 4)]:
        with pytest.raises(ValueError):
            TissueMask(*args)
    with pytest.raises(ValueError):
        TissueMask(ok, 4, mode="five_pt")
    m = TissueMask(np.array([[0, 3], [255, 0]], np.uint8), 8, "center")
    assert m.mask.dtype == torch.uint8 and m.mask.tolist() == [[0, 1], [1, 0]] and (m.downsample, m.mode, m.threshold) == (8, "center", None)
    assert TissueMask(torch.ones(3, 4, dtype=torch.bool), 2, threshold=9).threshold == 9
    with pytest.raises(ValueError):
        tissue_mask_numpy(np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError):
        tissue_mask_numpy(np.zeros((4, 4, 3), np.float32))


def test_model_checks_arguments_before_any_device_work():
    from keep_amd import KEEPModel
    m = KEEPModel()
    thumb = np.zeros((8, 8, 3), np.uint8)
    for args in [(thumb, 0), (thumb, 2.5), (thumb[..., 0], 4), (thumb.astype(np.int16), 4), (np.zeros((8, 8, 2), np.uint8), 4),
                 (torch.zeros(8, 8, 4, dtype=torch.uint8)[:, :, :3], 4)]:
        with pytest.raises(ValueError):
            m.tissue_mask(*args)
    with pytest.raises(ValueError):
        m.tissue_mask(thumb, 4, params=dict(mthresh=7))
    from keep_amd import cohort

    def never(*a):
        raise AssertionError("read_region must not be called")
    for kw in [dict(thumbnail_downsample=4), dict(segmentation=TissueSegmentation())]:
        with pytest.raises(ValueError):
            cohort.extract_slide_features(never, 1000, 1000, "s", "/nonexistent", **kw)


# ------------------------------------------------------------------------------------------------ what a masked extraction reads
def test_plan_mask_reads():
    patch, step = 256, 200
    bands = plan_bands(2000, 3000, patch, step, band_rows=4)      # 14 grid rows: bands of 4, 4, 4, 2
    assert [b[:2] for b in bands] == [(0, 4), (4, 8), (8, 12), (12, 14)]
    cells = np.array([[400, 0], [1000, 600], [600, 200],          # band 0: x from 400 to 1000
                      [0, 1600], [1600, 2200],                    # band 2: the full width of the grid
                      [800, 2400]], np.int64)                     # band 3: one cell
    reads = plan_mask_reads(cells, bands, patch, step)
    assert reads == [(400, 0, 1000 + patch - 400, bands[0][3]), (0, 1600, 1600 + patch, bands[2][3]), (800, 2400, patch, bands[3][3])]
    assert all(x0 % step == 0 for x0, _, _, _ in reads)           # a window starts on the grid: its own grid is the slide's
    assert plan_mask_reads(np.zeros((0, 2), np.int64), bands, patch, step) == []
    # with the planner's cells taken from a mask: every kept cell lies in exactly one window, in order
    g = np.random.default_rng(2)
    mask = np.kron(g.random((10, 7)) < 0.3, np.ones((9, 9), bool))
    mask[27:45] = 0                                               # an empty stretch: bands without cells
    cells = mask_grid_numpy(mask, 32, 3000, 2000, patch, step)
    reads = plan_mask_reads(cells, bands, patch, step)
    assert 0 < len(reads) < len(bands) or len(cells) == 0
    seen = []
    for x0, y0, w, h in reads:
        sub = mask_grid_numpy(mask, 32, h, w, patch, step, (x0, y0)) + (x0, y0)
        assert sub[:, 0].min() == x0 and sub[:, 0].max() + patch == x0 + w
        seen.append(sub)
    assert np.array_equal(np.concatenate(seen), cells)
