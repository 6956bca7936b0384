"""The subtype map on the MI355X: keep_heat_accumulate_classes / keep_class_argmax / keep_class_confusion /
keep_class_render, KEEPModel.class_raster / class_map / label_confusion / annotation_label_map / render_class_map, wsi.subtyping_map /
subtype_regions.

Everything is integer arithmetic, so every comparison is exact: the yardsticks are keep_amd.classmap.class_raster_numpy /
class_argmax_numpy / confusion_numpy / class_render_numpy, which tests/test_classmap.py holds to per-pixel Python loops, and the merged
scalar raster KEEPModel.tile_raster."""
import ctypes as C_

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel, _lib, wsi
from keep_amd.annotation import PolygonSet
from keep_amd.classmap import (ClassMap, ClassRaster, class_argmax_numpy, class_raster_numpy, class_render_numpy, confusion_numpy, one_hot_numpy,
                               palette)
from keep_amd.config import small_shape
from keep_amd.heatmap import MAX_TILES, TileRaster, gaussian_taps, render_numpy, smooth_numpy
from keep_amd.model import _ptr, _stream
from keep_amd.region import TissueMask
from keep_amd.synth import synth_state_dict
from test_classmap import class_values
from test_heatmap import case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(16, 224, 1), (16, 224, 3), (16, 256, 5), (16, 224, 64), (3, 224, 2), (3, 256, 3), (1, 224, 2)]


@pytest.fixture(scope="module")
def model():
    m = KEEPModel(precision="strict")
    m.load_state_dict(synth_state_dict(small_shape(2, 2), seed=5), strict=True)
    return m.to(DEV).eval()


def same(t: torch.Tensor, a: np.ndarray) -> bool:
    want = torch.from_numpy(a if a.flags.writeable else a.copy())                # the shared restatements are read-only
    return t.dtype == want.dtype and torch.equal(t.cpu(), want)


_made = {}


def made(d, P, C):
    """One case's tiles and the restated accumulator, computed once and shared (never written to)."""
    if (d, P, C) not in _made:
        coords, _, shape, origin = case(d, P)
        values = class_values(len(coords), C, seed=C)
        want = class_raster_numpy(coords, values, P, d, shape, origin)
        want.setflags(write=False)
        _made[d, P, C] = (coords, values, shape, origin, want)
    return _made[d, P, C]


@pytest.mark.parametrize("d,P,C", CASES)
def test_accumulate_argmax_confusion_and_render_match_the_restatements(model, d, P, C):
    coords, values, shape, origin, want = made(d, P, C)
    r = model.class_raster(torch.from_numpy(coords).to(DEV), torch.from_numpy(values).to(DEV), P, d, shape, origin)
    assert isinstance(r, ClassRaster) and r.acc.device == torch.device(DEV) and r.tiles == len(coords) and r.shape == shape and r.n_classes == C
    assert same(r.acc, want)
    # every plane is the merged scalar raster of its column over the rows without NaN
    ok = ~np.isnan(values).any(axis=1)
    for c in sorted({0, C // 2, C - 1}):
        assert torch.equal(r.plane(c).acc, model.tile_raster(coords[ok], values[ok, c], P, d, shape, origin).acc)
    g = np.random.default_rng(d + P + C)
    tissue = TissueMask(g.random(shape) < 0.7, d)
    mask = tissue.mask.numpy()
    maps = []
    for kw, (m, mv, mm) in [(dict(), (None, 0.0, 0.0)), (dict(tissue=tissue, min_value=0.3, min_margin=0.05), (mask, 0.3, 0.05)),
                            (dict(min_margin=0.2), (None, 0.0, 0.2))]:
        cm = model.class_map(r, **kw)
        label, top, margin = class_argmax_numpy(want, m, mv, mm)
        assert isinstance(cm, ClassMap) and same(cm.labels, label) and same(cm.top.acc, top) and same(cm.margin.acc, margin)
        maps.append((cm, label, top, margin))
    (cm, label, top, margin), (cm2, label2, _, _) = maps[0], maps[1]
    assert (label < C).any() and (label == 255).any() and ((label2 == 254).any() or C == 1)
    # confusion, and the class areas off its diagonal
    assert same(model.label_confusion(cm, cm2, C), confusion_numpy(label, label2, C))
    assert same(model.label_confusion(cm.labels, label2, C, within=tissue), confusion_numpy(label, label2, C, mask))
    areas = [int((label2 == c).sum()) for c in range(C)] + [int((label2 >= C).sum())]
    assert cm2.counts().tolist() == areas and cm2.counts(tissue).tolist()[:C] == areas[:C]
    # render, plain and with the margin / the winner's mean as strength
    thumb = g.integers(0, 256, shape + (3,), dtype=np.uint8)
    own = g.integers(0, 256, (C, 3), dtype=np.uint8)
    assert same(model.render_class_map(cm2, thumb), class_render_numpy(label2, None, C, thumb))
    assert same(model.render_class_map(cm, thumb, alpha=0.8, palette=own, strength="margin", window=(0.0, 0.5)),
                class_render_numpy(label, own, C, thumb, 0.8, margin, (0.0, 0.5)))
    assert same(model.render_class_map(cm, None, alpha=1.0, strength=cm.top, background=(10, 200, 30)),
                class_render_numpy(label, None, C, None, 1.0, top, background=(10, 200, 30)))
    assert same(model.render_class_map(cm, thumb, alpha=0.0), thumb)
    # the confidence maps are rasters: they go through the heatmap's render unchanged
    assert same(model.render_heatmap(cm.margin, thumb, alpha=0.6), render_numpy(margin, thumb, alpha=0.6))
    assert same(model.render_heatmap(cm.top, None, window=(0.2, 0.9)), render_numpy(top, None, window=(0.2, 0.9)))


@pytest.mark.parametrize("d,P,C", [(16, 224, 3), (3, 224, 2)])
def test_one_call_equals_three_and_two_runs_are_equal(model, d, P, C):
    coords, values, shape, origin, want = made(d, P, C)
    c, v = torch.from_numpy(coords).to(DEV), torch.from_numpy(values).to(DEV)
    one = model.class_raster(c, v, P, d, shape, origin)
    again = model.class_raster(c, v, P, d, shape, origin)
    assert torch.equal(one.acc, again.acc)
    order = torch.from_numpy(np.random.default_rng(d).permutation(len(coords))).to(DEV)
    r = None
    for idx in order.tensor_split(3):
        r = model.class_raster(c[idx], v[idx], P, d, shape, origin, into=r)
    assert r.tiles == len(coords) and torch.equal(r.acc, one.acc) and same(r.acc, want)
    near = ClassRaster(torch.zeros((C,) + shape, dtype=torch.int64, device=DEV), d, P, origin, tiles=MAX_TILES - 2, model=model)
    with pytest.raises(ValueError, match="2\\^24 - 1"):
        model.class_raster(c[:3], v[:3], P, d, shape, origin, into=near)
    assert int(near.acc.abs().sum()) == 0 and near.tiles == MAX_TILES - 2    # refused before anything was added


def test_labels_host_device_numpy_torch_and_empty_inputs(model):
    d, P, C = 16, 224, 3
    coords, values, shape, origin, want = made(d, P, C)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    for cc, vv, to in [(coords, values, lambda a: a), (coords, values, torch.from_numpy), (coords.astype(np.int32), values.astype(np.float64), dev)]:
        assert same(model.class_raster(to(cc), to(vv), P, d, shape, origin).acc, class_raster_numpy(cc, vv, P, d, shape, origin))
    assert same(model.class_raster(dev(coords), values, P, d, shape, origin).acc, want)
    wide = np.concatenate([values, values], axis=1)
    strided_v = dev(wide)[:, 1:1 + C]                                            # non-contiguous device views
    strided_c = dev(np.concatenate([coords, coords], axis=1))[:, 1:3]
    assert same(model.class_raster(strided_c, strided_v, P, d, shape, origin).acc,
                class_raster_numpy(np.concatenate([coords, coords], axis=1)[:, 1:3], wide[:, 1:1 + C], P, d, shape, origin))
    labels = np.random.default_rng(2).integers(0, C, len(coords))
    votes = class_raster_numpy(coords, one_hot_numpy(labels, C), P, d, shape, origin)
    for l in (labels, torch.from_numpy(labels), dev(labels), dev(labels.astype(np.int32))):
        rv = model.class_raster(coords, None, P, d, shape, origin, labels=l, n_classes=C)
        assert same(rv.acc, votes)
    assert torch.equal(rv.acc, model.class_raster(coords, one_hot_numpy(labels, C), P, d, shape, origin).acc)
    named = model.class_raster(coords, None, P, d, shape, origin, labels=labels, classes=["a", "b", "c"])
    assert named.classes == ("a", "b", "c") and same(named.acc, votes)
    more = model.class_raster(coords, None, P, d, shape, origin, labels=labels, into=named)           # C from into=
    assert more is named and more.tiles == 2 * len(coords) and same(more.acc, 2 * votes)
    with pytest.raises(ValueError, match="0..2"):
        model.class_raster(coords, None, P, d, shape, origin, labels=dev(labels + 1), n_classes=C)
    none = model.class_raster(np.zeros((0, 2), np.int64), np.zeros((0, C), np.float32), P, d, shape, origin)
    assert none.tiles == 0 and none.acc.shape == (C,) + shape and int(none.acc.abs().sum()) == 0
    none = model.class_raster(np.zeros((0, 2), np.int64), None, P, d, shape, origin, labels=np.zeros(0, np.int64), n_classes=C)
    assert none.tiles == 0 and int(none.acc.abs().sum()) == 0
    empty = model.class_map(none)
    assert int((empty.labels != 255).sum()) == 0 and int(empty.top.acc.abs().sum()) == 0
    # host label maps and masks of both libraries
    cm = model.class_map(model.class_raster(coords, values, P, d, shape, origin))
    label = class_argmax_numpy(want)[0]
    other = np.random.default_rng(3).choice(np.array([0, 1, 2, 3, 200, 254, 255], np.uint8), shape)
    within = np.random.default_rng(4).random(shape) < 0.5
    wantc = confusion_numpy(label, other, C, within)
    for a, b, wi in [(cm, other, within), (label, torch.from_numpy(other), torch.from_numpy(within)), (dev(label), dev(other), dev(within.astype(np.uint8)))]:
        assert same(model.label_confusion(a, b, C, wi), wantc)
    odd = dev(np.concatenate([np.zeros(1, np.uint8), other.reshape(-1)]))[1:].reshape(shape)      # 1-byte aligned: the scalar path
    assert same(model.label_confusion(cm, odd, C), confusion_numpy(label, other, C))
    assert same(model.label_confusion(other, other, 64), confusion_numpy(other, other, 64))


def test_smooth_and_fractions(model):
    d, P, C = 16, 224, 3
    coords, values, shape, origin, want = made(d, P, C)
    r = model.class_raster(coords, values, P, d, shape, origin, classes=["ccRCC", "pRCC", "chRCC"])
    tissue = TissueMask(np.random.default_rng(1).random(shape) < 0.8, d)
    for kw, m in [(dict(sigma=1.5), None), (dict(sigma=2.0, radius=3, tissue=tissue), tissue.mask.numpy())]:
        s = r.smooth(**kw)
        taps = gaussian_taps(kw["sigma"], kw.get("radius"))
        assert isinstance(s, ClassRaster) and s.classes == r.classes and s.tiles == r.tiles and s.shape == r.shape
        for c in range(C):
            assert same(s.plane(c).acc, smooth_numpy(want[c], taps, m))
        label, top, margin = class_argmax_numpy(s.acc.cpu().numpy(), None, 0.0, 0.02)
        cm = model.class_map(s, min_margin=0.02)
        assert same(cm.labels, label) and same(cm.margin.acc, margin)
    n = np.array([(label == c).sum() for c in range(C)], np.float64)
    assert np.array_equal(cm.fractions(), n / n.sum()) and np.array_equal(cm.fractions(drop_last=True), n[:2] / n[:2].sum())
    assert cm.slide_label(drop_last=False) == int(np.argmax(n)) and cm.slide_label() == int(np.argmax(n[:2]))


def test_subtype_regions_equal_mask_regions_on_the_restated_masks(model):
    d, P, C = 16, 224, 3
    coords, values, shape, origin, want = made(d, P, C)
    cm = model.class_map(model.class_raster(coords, values, P, d, shape, origin), min_margin=0.05)
    label = class_argmax_numpy(want, None, 0.0, 0.05)[0]
    tissue = TissueMask(np.random.default_rng(7).random(shape) < 0.9, d)
    for t, tm in ((None, np.ones(shape, bool)), (tissue, tissue.mask.numpy() != 0)):
        tables = wsi.subtype_regions(cm, tissue=t, connectivity=4, min_area=2, model=model)
        assert sorted(tables) == list(range(C))
        for c in range(C):
            plane = TileRaster(torch.from_numpy(want[c].copy()).to(DEV), d, P, origin, model=model)
            ref = model.mask_regions(((label == c) & tm).astype(np.uint8), 4, 2, raster=plane)
            assert tables[c].n == ref.n and torch.equal(tables[c].table, ref.table) and torch.equal(tables[c].labels, ref.labels)
        assert sum(tables[c].n for c in range(C)) > C


def test_annotation_label_map_is_the_where_composition(model):
    d, shape = 16, (40, 50)
    square = lambda x0, y0, x1, y1: np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.int64) * d
    a = PolygonSet(np.concatenate([square(2, 3, 30, 25), square(35, 30, 48, 38)]), np.array([0, 4, 8]))
    b = PolygonSet(np.concatenate([square(20, 10, 45, 35), np.array([[5, 30], [15, 30], [10, 39]], np.int64) * d + 7]), np.array([0, 4, 7]))
    got = model.annotation_label_map([a, b], d, shape)
    ma, mb = (model.annotation_mask(p, d, shape).mask.cpu().numpy() for p in (a, b))
    want = np.where(mb != 0, 1, np.where(ma != 0, 0, 255)).astype(np.uint8)
    assert same(got, want) and ((ma != 0) & (mb != 0)).any() and all((want == v).any() for v in (0, 1, 255))
    back = model.annotation_label_map([b, a], d, shape)
    assert same(back, np.where(ma != 0, 1, np.where(mb != 0, 0, 255)).astype(np.uint8))
    m = model.label_confusion(got, back, 2).cpu().numpy()
    assert m[2, 2] == (want == 255).sum() and m[0, 0] == 0 and m[1, 0] == ((mb != 0) & (ma == 0)).sum()


def flow_case(seed):
    """48 tiles on a lattice of step patch, random unit features and a random [768, 4] classifier."""
    P = 224
    g = torch.Generator().manual_seed(seed)
    feats = torch.nn.functional.normalize(torch.randn(48, 768, generator=g), dim=1)
    classifier = torch.randn(768, 4, generator=g)
    coords = torch.tensor([(x * P, y * P) for y in range(6) for x in range(8)], dtype=torch.int64)
    return P, feats, classifier, coords[torch.randperm(48, generator=g)]


def test_the_flow_on_a_lattice_gives_the_reference_call(model):
    P, feats, classifier, coords = flow_case(0)
    d = 16
    shape = (6 * P // d + 1, 8 * P // d + 2)
    want_label = int(wsi.zero_shot_subtyping(classifier.to(DEV), feats.to(DEV), coords, patch_size=P, overlap=True, model=model))
    votes = wsi.subtyping_map(classifier.to(DEV), feats.to(DEV), coords, d, shape, patch_size=P, overlap=True, vote=True,
                              classes=["ccRCC", "pRCC", "chRCC", "Normal"], model=model)
    assert isinstance(votes, ClassRaster) and votes.n_classes == 4 and votes.tiles == 48 and votes.classes[3] == "Normal"
    rc, mean, _ = wsi.refine(wsi._probs(model, classifier.to(DEV), feats.to(DEV)), coords, P, True, model=model)
    pred = mean.argmax(dim=1).cpu().numpy()
    tiles = np.bincount(pred, minlength=4)
    top_two = np.sort(tiles[:3])[::-1]
    assert top_two[0] != top_two[1], "the seed must give a slide whose two largest tile shares differ"
    cm = model.class_map(votes)
    assert cm.counts().tolist() == list(tiles * (P // d) ** 2) + [shape[0] * shape[1] - 48 * (P // d) ** 2]
    assert cm.slide_label() == want_label == int(np.argmax(tiles[:3]))
    assert same(votes.acc, class_raster_numpy(rc.cpu().numpy(), one_hot_numpy(pred, 4), P, d, shape))
    probs = wsi.subtyping_map(classifier.to(DEV), feats.to(DEV), coords, d, shape, patch_size=P, overlap=True, model=model)
    assert same(probs.acc, class_raster_numpy(rc.cpu().numpy(), mean.cpu().numpy(), P, d, shape))
    assert torch.equal(model.class_map(probs).labels, cm.labels)                  # one tile per pixel: the same call either way
    picture = model.render_class_map(cm, None, strength="top")
    assert same(picture, class_render_numpy(cm.labels.cpu().numpy(), None, 4, None, 0.5, cm.top.acc.cpu().numpy()))


def test_abi_rejects_bad_arguments(model):
    lib, h, st = _lib.load(), model._handle, _stream(torch.device(DEV))
    H, W, N, C = 20, 24, 6, 3
    acc = torch.zeros((C, H, W), dtype=torch.int64, device=DEV)
    coords = torch.zeros((N, 2), dtype=torch.int64, device=DEV)
    values = torch.full((N, C), 0.5, dtype=torch.float32, device=DEV)
    label = torch.zeros((H, W), dtype=torch.uint8, device=DEV)
    top = torch.zeros((H, W), dtype=torch.int64, device=DEV)
    counts = torch.zeros(((C + 1) ** 2,), dtype=torch.int64, device=DEV)
    pal = torch.from_numpy(palette(C)).to(DEV)
    thumb = torch.zeros((H, W, 4), dtype=torch.uint8, device=DEV)
    out = torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV)
    null = C_.c_void_p(0)
    off = lambda t, nbytes: C_.c_void_p(t.data_ptr() + nbytes)

    def accumulate(c=_ptr(coords), v=_ptr(values), n=N, k=C, P=224, d=16, Hh=H, Ww=W, ox=0, oy=0, a=_ptr(acc)):
        return lib.keep_heat_accumulate_classes(h, c, v, n, k, P, d, Hh, Ww, ox, oy, a, st)

    assert accumulate() == _lib.KEEP_OK
    torch.cuda.synchronize()
    assert all(int(acc[c, 0, 0]) == (N << 40) | (N * 32768) for c in range(C)) and int(acc[:, -1, -1].abs().sum()) == 0
    for kw in [dict(c=null), dict(v=null), dict(a=null), dict(a=off(acc, 4)), dict(n=-1), dict(n=1 << 24), dict(k=0), dict(k=65), dict(P=0),
               dict(P=(1 << 30) + 1), dict(d=0), dict(d=225), dict(Hh=0), dict(Ww=-1), dict(Hh=1 << 15, Ww=1 << 14), dict(ox=8), dict(oy=-8), dict(ox=1 << 44)]:
        assert accumulate(**kw) == _lib.KEEP_EINVAL, kw
        assert lib.keep_last_error(h)
    assert accumulate(n=0, c=null, v=null) == _lib.KEEP_OK                        # nothing to add is no error

    def argmax(a=_ptr(acc), k=C, Hh=H, Ww=W, m=null, mn=0, mg=0, l=_ptr(label), t=_ptr(top), g=null):
        return lib.keep_class_argmax(h, a, k, Hh, Ww, m, mn, mg, l, t, g, st)

    assert argmax() == _lib.KEEP_OK and argmax(l=null) == _lib.KEEP_OK
    for kw in [dict(a=null), dict(a=off(acc, 4)), dict(k=0), dict(k=65), dict(Hh=0), dict(Hh=1 << 15, Ww=1 << 14), dict(mn=-1), dict(mn=65536), dict(mg=-1),
               dict(mg=65536), dict(l=null, t=null), dict(t=off(top, 4))]:
        assert argmax(**kw) == _lib.KEEP_EINVAL, kw

    def confusion(a=_ptr(label), b=_ptr(label), wi=null, Hh=H, Ww=W, k=C, o=_ptr(counts)):
        return lib.keep_class_confusion(h, a, b, wi, Hh, Ww, k, o, st)

    assert confusion() == _lib.KEEP_OK
    for kw in [dict(a=null), dict(b=null), dict(Hh=0), dict(Ww=0), dict(k=0), dict(k=65), dict(o=null), dict(o=off(counts, 4))]:
        assert confusion(**kw) == _lib.KEEP_EINVAL, kw

    def render(l=_ptr(label), Hh=H, Ww=W, k=C, t=_ptr(thumb), row=W * 4, ps=4, bg=0xFFFFFF, p=_ptr(pal), alpha=128, s=_ptr(top), lo=0, hi=65535, o=_ptr(out)):
        return lib.keep_class_render(h, l, Hh, Ww, k, t, row, ps, bg, p, alpha, s, lo, hi, o, st)

    assert render() == _lib.KEEP_OK and render(t=null, s=null) == _lib.KEEP_OK
    for kw in [dict(l=null), dict(p=null), dict(o=null), dict(Hh=0), dict(k=0), dict(k=65), dict(ps=2), dict(row=W * 4 - 1), dict(t=null, bg=-1),
               dict(t=null, bg=1 << 24), dict(alpha=-1), dict(alpha=257), dict(s=off(top, 4)), dict(lo=-1), dict(hi=65536), dict(lo=100, hi=100)]:
        assert render(**kw) == _lib.KEEP_EINVAL, kw
        assert lib.keep_last_error(h)
    for call in (lambda: lib.keep_heat_accumulate_classes(None, _ptr(coords), _ptr(values), N, C, 224, 16, H, W, 0, 0, _ptr(acc), st),
                 lambda: lib.keep_class_argmax(None, _ptr(acc), C, H, W, null, 0, 0, _ptr(label), null, null, st),
                 lambda: lib.keep_class_confusion(None, _ptr(label), _ptr(label), null, H, W, C, _ptr(counts), st),
                 lambda: lib.keep_class_render(None, _ptr(label), H, W, C, null, 0, 3, 0, _ptr(pal), 128, null, 0, 65535, _ptr(out), st)):
        assert call() == _lib.KEEP_EINVAL
    torch.cuda.synchronize()
