"""The subtype map's host side (keep_amd/classmap.py): the numpy restatements the device is held to are
themselves held here to independent statements of the rules -- per-pixel Python loops over Python integers for the class
accumulator, the argmax with its thresholds, the confusion and the render -- plus every ValueError.  No GPU."""
import numpy as np
import pytest
import torch

from keep_amd import KEEPModel
from keep_amd import classmap as cmap
from keep_amd.classmap import (ClassRaster, class_argmax_numpy, class_raster_numpy, class_render_numpy, confusion_numpy, one_hot_numpy,
                               overlap_from_confusion, palette)
from keep_amd.heatmap import TileRaster, raster_numpy, render_args, unpack_numpy
from test_heatmap import case, python_quantize, tie_values

M40 = (1 << 40) - 1


def class_values(n, C, seed=0, specials=True):
    """fp32 [n,C] rows that look like probabilities, with the rows the rules turn on: a NaN first, last and in the middle of a row, +-inf,
    -0.0, values outside [0, 1] and the two round-half-to-even ties."""
    g = np.random.default_rng(seed)
    v = g.random((n, C)).astype(np.float32)
    v /= v.sum(axis=1, keepdims=True)
    if specials:
        even, odd = tie_values()
        rows = g.choice(n, 9, replace=False)
        v[rows[0], 0] = np.nan
        v[rows[1], C - 1] = np.nan
        v[rows[2], C // 2] = np.nan
        v[rows[3], 0], v[rows[3], C - 1] = np.inf, -np.inf
        v[rows[4], C // 2] = -0.0
        v[rows[5], 0], v[rows[5], C - 1] = 1.7, -0.3
        v[rows[6], 0], v[rows[6], C - 1] = even, odd
        v[rows[7], :] = 0.5                                                       # an all-equal row
        v[rows[8], :] = 0.0
    return v


def accumulate_by_pixel(coords, values, P, d, shape, origin):
    """For every (tile, pixel, class): membership by Python-integer floor divisions, one add of (1 << 40) | q; a row with a NaN adds
    nothing anywhere -> Python-int lists [C][h][w]."""
    h, w = shape
    C = values.shape[1]
    acc = [[[0] * w for _ in range(h)] for _ in range(C)]
    for n in range(len(coords)):
        q = [python_quantize(v) for v in values[n]]
        if any(x is None for x in q):
            continue
        x0, x1 = (int(coords[n][0]) - origin[0]) // d, (int(coords[n][0]) - origin[0] + P) // d
        y0, y1 = (int(coords[n][1]) - origin[1]) // d, (int(coords[n][1]) - origin[1] + P) // d
        for y in range(max(y0, 0), min(y1, h)):
            for x in range(max(x0, 0), min(x1, w)):
                for c in range(C):
                    acc[c][y][x] += (1 << 40) | q[c]
    return acc


@pytest.mark.parametrize("d,P,C", [(16, 224, 3), (32, 256, 1), (16, 256, 5), (32, 224, 64)])
def test_class_raster_numpy_against_a_per_pixel_loop(d, P, C):
    coords, _, shape, origin = case(d, P)
    values = class_values(len(coords), C, seed=C)
    acc = class_raster_numpy(coords, values, P, d, shape, origin)
    assert acc.dtype == np.int64 and acc.shape == (C,) + shape
    assert np.array_equal(acc, np.array(accumulate_by_pixel(coords, values, P, d, shape, origin), dtype=np.int64))
    S, n = unpack_numpy(acc)
    assert all(np.array_equal(n[c], n[0]) for c in range(C)) and n.max() >= 4    # a NaN skips its tile in every plane
    # the planes are the scalar raster of their column over the rows without NaN
    ok = ~np.isnan(values).any(axis=1)
    assert (~ok).sum() >= (3 if C >= 3 else 1)
    for c in range(C):
        assert np.array_equal(acc[c], raster_numpy(coords[ok], values[ok, c], P, d, shape, origin))
    # any split over calls, and into=
    parts = None
    for idx in np.array_split(np.random.default_rng(1).permutation(len(coords)), 3):
        parts = class_raster_numpy(coords[idx], values[idx], P, d, shape, origin, into=parts)
    assert np.array_equal(parts, acc)


def test_one_hot_labels_make_a_vote_raster():
    coords, _, shape, origin = case(16, 224, seed=4)
    labels = np.random.default_rng(3).integers(0, 4, len(coords))
    acc = class_raster_numpy(coords, one_hot_numpy(labels, 4), 224, 16, shape, origin)
    S, n = unpack_numpy(acc)
    assert np.array_equal(S.sum(axis=0), 65535 * n[0].astype(np.int64))          # every covering tile votes once
    for c in range(4):
        assert np.array_equal(acc[c], raster_numpy(coords, (labels == c).astype(np.float32), 224, 16, shape, origin))


def argmax_by_pixel(acc, mask, min16, margin16):
    C, h, w = acc.shape
    label, top, margin = np.empty((h, w), np.uint8), np.empty((h, w), np.int64), np.empty((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            words = [int(acc[c, y, x]) & ((1 << 64) - 1) for c in range(C)]
            n, S = words[0] >> 40, [wd & M40 for wd in words]
            if n == 0 or (mask is not None and not mask[y, x]):
                label[y, x], top[y, x], margin[y, x] = 255, 0, 0
                continue
            best = 0
            for c in range(1, C):
                if S[c] > S[best]:
                    best = c
            second = max([S[c] for c in range(C) if c != best], default=0)
            undecided = S[best] < min16 * n or S[best] - second < margin16 * n
            label[y, x] = 254 if undecided else best
            top[y, x], margin[y, x] = (n << 40) | S[best], (n << 40) | (S[best] - second)
    return label, top, margin


@pytest.mark.parametrize("C", [1, 2, 5])
def test_class_argmax_numpy_against_a_per_pixel_loop(C):
    coords, _, shape, origin = case(32, 224, seed=C)
    acc = class_raster_numpy(coords, class_values(len(coords), C, seed=10 + C), 224, 32, shape, origin)
    mask = (np.random.default_rng(C).random(shape) < 0.7).astype(np.uint8)
    for m, mv, mm in [(None, 0.0, 0.0), (mask, 0.0, 0.0), (None, 0.3, 0.0), (mask, 0.25, 0.1), (None, 0.0, 0.05), (None, 1.0, 1.0)]:
        got = class_argmax_numpy(acc, m, mv, mm)
        want = argmax_by_pixel(acc, m, *cmap.class_map_args(mv, mm))
        for g, wnt, dt in zip(got, want, (np.uint8, np.int64, np.int64)):
            assert g.dtype == dt and np.array_equal(g, wnt)
    label, top, margin = class_argmax_numpy(acc)
    n = unpack_numpy(acc)[1][0]
    assert (label[n == 0] == 255).all() and (label[n > 0] < C).all() and (n == 0).any() and (n > 1).any()
    assert np.array_equal(unpack_numpy(top)[1], n) and np.array_equal(unpack_numpy(margin)[1], n)
    if C == 1:
        assert np.array_equal(top, margin) and np.array_equal(top, acc[0])        # no runner-up: the margin is the winner's sum


def test_argmax_ties_go_to_the_lowest_class():
    coords = np.array([[0, 0], [16, 0]], np.int64)                                # two overlapping tiles: the sums tie exactly in the overlap
    values = np.array([[0.25, 0.75], [0.75, 0.25]], np.float32)
    acc = class_raster_numpy(coords, values, 32, 16, (2, 3))
    label, top, margin = class_argmax_numpy(acc)
    S, n = unpack_numpy(acc)
    assert n[0, 0, 1] == 2 and S[0, 0, 1] == S[1, 0, 1]
    assert label.tolist() == [[1, 0, 0], [1, 0, 0]]
    assert margin[0, 1] == 2 << 40 and top[0, 1] == (2 << 40) | int(S[0, 0, 1])
    flat = class_raster_numpy(coords[:1], np.full((1, 7), 0.5, np.float32), 32, 16, (2, 3))   # an all-equal row
    label, _, margin = class_argmax_numpy(flat)
    assert label.tolist() == [[0, 0, 255], [0, 0, 255]] and (unpack_numpy(margin)[0] == 0).all()
    assert (class_argmax_numpy(flat, min_margin=1 / 65535)[0][:, :2] == 254).all()


def test_thresholds_exactly_at_and_one_unit_either_side():
    """One tile, so n = 1 and S_top / n, (S_top - S_second) / n are whole units of the fixed point; and two tiles whose sums are odd, so
    that S / n falls between two units."""
    v = np.array([[0.2, 0.7, 0.1]], np.float32)
    q = [python_quantize(x) for x in v[0]]
    acc = class_raster_numpy(np.zeros((1, 2), np.int64), v, 16, 16, (1, 1))
    u = lambda k: np.float32(k / 65535)
    for k, want in [(q[1] - 1, 1), (q[1], 1), (q[1] + 1, 254)]:
        assert cmap.class_map_args(u(k), 0.0) == (k, 0)
        assert class_argmax_numpy(acc, None, u(k), 0.0)[0].item() == want
    gap = q[1] - q[0]
    for k, want in [(gap - 1, 1), (gap, 1), (gap + 1, 254)]:
        assert class_argmax_numpy(acc, None, 0.0, u(k))[0].item() == want
    label, top, margin = class_argmax_numpy(acc, None, u(q[1] + 1), 0.0)
    assert top.item() == (1 << 40) | q[1] and margin.item() == (1 << 40) | gap     # an undecided pixel keeps its numbers
    two = np.array([[u(1000), u(3001)], [u(1001), u(3002)]], np.float32)          # S = (2001, 6003), n = 2
    acc = class_raster_numpy(np.zeros((2, 2), np.int64), two, 16, 16, (1, 1))
    assert unpack_numpy(acc)[0].reshape(-1).tolist() == [2001, 6003]
    assert [class_argmax_numpy(acc, None, u(k), 0.0)[0].item() for k in (3001, 3002)] == [1, 254]       # 6003 >= 6002, 6003 < 6004
    assert [class_argmax_numpy(acc, None, 0.0, u(k))[0].item() for k in (2001, 2002)] == [1, 254]       # 4002 >= 4002, 4002 < 4004


def test_confusion_numpy_against_add_at():
    g = np.random.default_rng(6)
    C, shape = 5, (37, 53)
    a = g.choice(np.array([0, 1, 2, 3, 4, 5, 9, 100, 253, 254, 255], np.uint8), shape)
    b = g.choice(np.array([0, 1, 2, 3, 4, 6, 64, 254, 255], np.uint8), shape)
    within = (g.random(shape) < 0.6).astype(np.uint8)
    for wi in (None, within):
        want = np.zeros((C + 1, C + 1), np.int64)
        keep = np.ones(shape, bool) if wi is None else wi != 0
        np.add.at(want, (np.minimum(a[keep].astype(int), C), np.minimum(b[keep].astype(int), C)), 1)
        got = confusion_numpy(a, b, C, wi)
        assert got.dtype == np.int64 and np.array_equal(got, want) and got.sum() == keep.sum()
    areas = confusion_numpy(a, a, C)
    assert np.array_equal(np.diagonal(areas), [(a == c).sum() for c in range(C)] + [(a >= C).sum()]) and areas.sum() == np.trace(areas)
    o = overlap_from_confusion(confusion_numpy(a, b, C))
    for c in range(C):
        tp, A, B = ((a == c) & (b == c)).sum(), (a == c).sum(), (b == c).sum()
        assert o["dice"][c] == 2 * tp / (A + B) and o["iou"][c] == tp / (A + B - tp) and o["precision"][c] == tp / A and o["recall"][c] == tp / B
    assert np.isnan(overlap_from_confusion(np.zeros((3, 3), np.int64))["dice"]).all()


def render_by_pixel(labels, pal, under, a, strength, lo16, hi16):
    h, w = labels.shape
    out = np.empty((h, w, 3), np.uint8)
    for y in range(h):
        for x in range(w):
            u = [int(v) for v in under[y, x][:3]]
            lab = int(labels[y, x])
            if lab < len(pal):
                ae = a
                if strength is not None:
                    word = int(strength[y, x]) & ((1 << 64) - 1)
                    S, c = word & M40, word >> 40
                    idx = 0 if c == 0 or S <= lo16 * c else min((2 * 255 * (S - lo16 * c) + (hi16 - lo16) * c) // (2 * (hi16 - lo16) * c), 255)
                    ae = (a * idx + 127) // 255
                u = [(ae * int(pal[lab][ch]) + (256 - ae) * u[ch] + 128) >> 8 for ch in range(3)]
            out[y, x] = u
    return out


def test_class_render_numpy_against_a_per_pixel_loop():
    coords, _, shape, origin = case(32, 224, seed=7)
    C = 4
    acc = class_raster_numpy(coords, class_values(len(coords), C, seed=2), 224, 32, shape, origin)
    labels, top, margin = class_argmax_numpy(acc, None, 0.3, 0.0)
    assert (labels == 254).any() and (labels == 255).any() and (labels < C).any()
    g = np.random.default_rng(5)
    h, w = shape
    big = g.integers(0, 256, (h + 5, w + 9, 4), dtype=np.uint8)
    thumb = big[3:3 + h, 4:4 + w]                                             # an RGBA view with strided rows
    own = g.integers(0, 256, (C, 3), dtype=np.uint8)
    for alpha, pal, st, window in [(0.5, None, None, (0.0, 1.0)), (0.0, None, None, (0.0, 1.0)), (1.0, own, None, (0.0, 1.0)), (0.75, None, margin, (0.0, 1.0)),
                                   (1.0, own, top, (0.3, 0.6)), (0.0, None, margin, (0.0, 0.5)), (1.0, None, margin, (0.0, 0.05))]:
        a, lo16, hi16, _, _ = render_args(alpha, window, 0.0, (255, 255, 255))
        got = class_render_numpy(labels, pal, C, thumb, alpha, st, window)
        assert got.dtype == np.uint8 and got.shape == shape + (3,)
        assert np.array_equal(got, render_by_pixel(labels, palette(C) if pal is None else pal, thumb, a, st, lo16, hi16))
    assert np.array_equal(class_render_numpy(labels, None, C, thumb, 0.0), thumb[..., :3])
    full = class_render_numpy(labels, own, None, thumb, 1.0)
    assert np.array_equal(full[labels < C], own[labels[labels < C]]) and np.array_equal(full[labels >= C], thumb[..., :3][labels >= C])
    bg = (10, 200, 30)
    under = np.broadcast_to(np.array(bg, np.uint8), shape + (3,))
    assert np.array_equal(class_render_numpy(labels, None, C, None, 0.4, background=bg), render_by_pixel(labels, palette(C), under, 102, None, 0, 65535))


def test_palette_formula():
    for C in (1, 2, 3, 4, 7, 64):
        p = palette(C)
        assert p.dtype == np.uint8 and p.shape == (C, 3) and len({tuple(r) for r in p.tolist()}) == C
        for c in range(C):
            H = (1530 * c) // C
            s, f = divmod(H, 255)
            assert tuple(p[c]) == [(255, f, 0), (255 - f, 255, 0), (0, 255, f), (0, 255 - f, 255), (f, 0, 255), (255, 0, 255 - f)][s]
    assert palette(3).tolist() == [[255, 0, 0], [0, 255, 0], [0, 0, 255]]


def test_class_raster_views_and_counts():
    acc = torch.from_numpy(class_raster_numpy(*case(16, 224)[:1], class_values(len(case(16, 224)[0]), 3), 224, 16, *case(16, 224)[2:]))
    r = ClassRaster(acc, 16, 224, case(16, 224)[3], tiles=7, classes=["a", "b", "c"])
    assert r.n_classes == 3 and r.shape == tuple(acc.shape[1:]) and r.classes == ("a", "b", "c")
    p = r.plane(1)
    assert isinstance(p, TileRaster) and p.acc.data_ptr() == acc[1].data_ptr() and p.shape == r.shape and p.tiles == 7      # a view, no copy
    assert (p.downsample, p.patch, p.origin) == (r.downsample, r.patch, r.origin)
    r.claim(3)
    assert r.tiles == 10
    with pytest.raises(ValueError, match="2\\^24 - 1"):
        r.claim(1 << 24)
    with pytest.raises(ValueError, match="host"):
        r.smooth(sigma=1.0)


def test_value_errors():
    m = KEEPModel()                                                              # no device is reached: the checks come first
    c, v = np.zeros((5, 2), np.int64), np.zeros((5, 3), np.float32)
    ok = dict(patch_size=224, downsample=16, shape=(10, 12))
    for cc, vv in [(c, np.zeros((5, 0), np.float32)), (c, np.zeros((5, 65), np.float32)), (c, v[:, 0]), (c, v[:4]), (c, v.astype(np.int32)), (c[:, :1], v),
                   (c.astype(np.float32), v), (c, v.reshape(5, 3, 1))]:
        with pytest.raises(ValueError):
            class_raster_numpy(cc, vv, 224, 16, (10, 12))
        with pytest.raises(ValueError):
            m.class_raster(cc, vv, **ok)
    for kw in [dict(downsample=0), dict(downsample=448), dict(shape=(1 << 16, 1 << 15)), dict(origin=(3, 0)), dict(shape=(1 << 15, 1 << 14))]:
        with pytest.raises(ValueError):                                          # the last: 3 planes of 2^29 pixels, C h w > 2^30
            m.class_raster(c, v, **{**ok, **kw})
    with pytest.raises(ValueError, match="C \\* h \\* w"):
        class_raster_numpy(c, v, 224, 16, (1 << 15, 1 << 14))
    with pytest.raises(ValueError, match="C \\* h \\* w"):
        cmap.check_classes(64, (1 << 12, (1 << 12) + 1))
    assert cmap.check_classes(64, (1 << 12, 1 << 12)) == 64
    labels = np.array([0, 1, 2, 1, 0])
    for kw in [dict(values=v, labels=labels), dict(values=None, labels=None), dict(values=None, labels=labels),                  # both, neither, no C
               dict(values=None, labels=labels, n_classes=2), dict(values=None, labels=np.array([0, -1, 2, 1, 0]), n_classes=3),      # label out of range
               dict(values=None, labels=labels.astype(np.float32), n_classes=3), dict(values=None, labels=labels[:4], n_classes=3),
               dict(values=None, labels=labels, n_classes=3, classes=["a", "b"]), dict(values=None, labels=labels, n_classes=65),
               dict(values=v, labels=None, n_classes=4), dict(values=v, labels=None, classes=["a", "b"]), dict(values=v, labels=None, into=np.zeros((3, 10, 12), np.int64)),
               dict(values=v, labels=None, into=TileRaster(torch.zeros((10, 12), dtype=torch.int64), 16, 224))]:
        with pytest.raises(ValueError):
            m.class_raster(c, **{**ok, **kw})
    r = ClassRaster(torch.zeros((3, 10, 12), dtype=torch.int64), 16, 224)
    for kw in [dict(downsample=8), dict(patch_size=256), dict(shape=(12, 10)), dict(origin=(16, 0)), dict(values=np.zeros((5, 4), np.float32))]:
        with pytest.raises(ValueError, match="into="):
            m.class_raster(c, **{**dict(values=v, into=r), **ok, **kw})
    assert r.tiles == 0
    near = ClassRaster(torch.zeros((3, 10, 12), dtype=torch.int64), 16, 224, tiles=(1 << 24) - 3)
    with pytest.raises(ValueError, match="2\\^24 - 1"):
        m.class_raster(c, v, into=near, **ok)
    with pytest.raises(ValueError):
        class_raster_numpy(c, v, 224, 16, (10, 12), into=np.zeros((3, 10, 13), np.int64))
    for acc in (torch.zeros((3, 4, 4), dtype=torch.int32), torch.zeros((4, 4), dtype=torch.int64), torch.zeros((65, 4, 4), dtype=torch.int64),
                torch.zeros((0, 4, 4), dtype=torch.int64), torch.zeros((3, 4, 8), dtype=torch.int64)[:, :, ::2], np.zeros((3, 4, 4), np.int64)):
        with pytest.raises(ValueError):
            ClassRaster(acc, 16, 224)
    with pytest.raises(ValueError):
        ClassRaster(torch.zeros((3, 4, 4), dtype=torch.int64), 16, 224, classes=["a"])
    for bad in (-1, 3, 1.5):
        with pytest.raises(ValueError):
            r.plane(bad)
    # the label map
    from keep_amd.region import TissueMask
    for kw in [dict(min_value=float("nan")), dict(min_margin=float("nan")), dict(tissue=np.ones((10, 12), np.uint8)), dict(tissue=TissueMask(np.ones((10, 12), np.uint8), 8)),
               dict(tissue=TissueMask(np.ones((10, 13), np.uint8), 16))]:
        with pytest.raises(ValueError):
            m.class_map(r, **kw)
    with pytest.raises(ValueError):
        m.class_map(r.plane(0))
    for kw in [dict(acc=np.zeros((3, 4, 4), np.int32)), dict(acc=np.zeros((4, 4), np.int64)), dict(acc=np.zeros((65, 4, 4), np.int64)),
               dict(acc=np.zeros((3, 4, 4), np.int64), mask=np.ones((4, 5), np.uint8)), dict(acc=np.zeros((3, 4, 4), np.int64), min_value=float("nan"))]:
        with pytest.raises(ValueError):
            class_argmax_numpy(**kw)
    # confusion
    a = np.zeros((4, 5), np.uint8)
    for args in [(a, a, 0), (a, a, 65), (a, a[:, :4], 3), (a.astype(np.int32), a, 3), (a, a.reshape(-1), 3), (a, a, 2.5)]:
        with pytest.raises(ValueError):
            confusion_numpy(*args)
        with pytest.raises(ValueError):
            m.label_confusion(*args)
    with pytest.raises(ValueError):
        confusion_numpy(a, a, 3, within=np.ones((4, 4), np.uint8))
    with pytest.raises(ValueError):
        m.label_confusion(a, a, 3, within=np.ones((4, 4), np.uint8))
    for bad in (np.zeros((3, 4), np.int64), np.zeros((3, 3), np.float64), np.zeros((1, 1), np.int64)):
        with pytest.raises(ValueError):
            overlap_from_confusion(bad)
    # render
    top = TileRaster(torch.zeros((10, 12), dtype=torch.int64), 16, 224)
    cm = cmap.ClassMap(torch.zeros((10, 12), dtype=torch.uint8), top, top, r)
    for kw in [dict(palette=np.zeros((4, 3), np.uint8)), dict(palette=np.zeros((3, 4), np.uint8)), dict(palette=np.zeros((3, 3), np.int32)), dict(alpha=-0.1),
               dict(alpha=1.5), dict(window=(0.5, 0.5)), dict(window=(0.5,)), dict(background=(0, 0, 256)), dict(thumbnail=np.zeros((10, 13, 3), np.uint8)),
               dict(thumbnail=np.zeros((10, 12, 3), np.float32)), dict(strength=np.zeros((10, 13), np.int64))]:
        with pytest.raises(ValueError):
            class_render_numpy(np.zeros((10, 12), np.uint8), **{**dict(n_classes=3), **kw})
        if "strength" in kw:
            kw = dict(strength=TileRaster(torch.zeros((10, 13), dtype=torch.int64), 16, 224))
        with pytest.raises(ValueError):
            m.render_class_map(cm, **kw)
    for kw in [dict(strength="bottom"), dict(strength=np.zeros((10, 12), np.int64))]:
        with pytest.raises(ValueError):
            m.render_class_map(cm, **kw)
    with pytest.raises(ValueError):
        m.render_class_map(cm.labels)
    with pytest.raises(ValueError):
        class_render_numpy(np.zeros((10, 12), np.uint8))
    for bad in (-1, 3):
        with pytest.raises(ValueError):
            cm.mask(bad)
    with pytest.raises(ValueError):
        m.annotation_label_map([], 16, (10, 12))
    with pytest.raises(ValueError):
        m.annotation_label_map([np.zeros((4, 2))], 16, (10, 12))
