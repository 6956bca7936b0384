"""Few-shot prototypes on the MI355X: keep_fewshot_sample / keep_fewshot_prototypes / keep_fewshot_classify,
KEEPModel.fewshot_sample / fewshot_prototypes / fewshot_classify / fewshot_fit / fewshot_predict / fewshot_episodes, tile_eval.few_shot,
wsi.prototype_map and wsi.prototype_slide_call.

The yardsticks: a dot is keep_cluster_assign's `best` against a one-row bank, bit for bit; the support sets equal
keep_amd.fewshot.sample_numpy exactly; the bank lies within keep_amd.fewshot.bank_bound of prototypes_numpy in float64; the labels equal
classify_numpy's (float64, over the device's own bank and consts read back) wherever its margin exceeds margin_bound, computed from the
case's own smallest r; everything that must not depend on the launch is compared with torch.equal."""
import ctypes as C_

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel, _lib, tile_eval, wsi
from keep_amd import fewshot as fs
from keep_amd.classmap import ClassRaster, class_raster_numpy, one_hot_numpy
from keep_amd.config import small_shape
from keep_amd.model import _ptr, _stream
from keep_amd.synth import synth_state_dict
from test_cluster import blobs, unit_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP = 0.02                                                              # the share of undecided (row, episode) pairs a case may have


@pytest.fixture(scope="module")
def model():
    m = KEEPModel(precision="strict")
    m.load_state_dict(synth_state_dict(small_shape(2, 2), seed=5), strict=True)
    return m.to(DEV).eval()


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                         # a copy: the shared cases are read-only


def raw_classify(model, x, bank, consts, valid, truth=None, conf=None, labels=None, scores=None, margin=None, dots=None, skipped=None, segments=0,
                 N=None, D=None, E=None, C=None):
    E_, C1, D_ = bank.shape
    return _lib.load().keep_fewshot_classify(model._handle, _ptr(x), x.shape[0] if N is None else N, D_ if D is None else D, _ptr(bank), _ptr(consts),
                                             _ptr(valid), E_ if E is None else E, C1 - 1 if C is None else C, _ptr(truth), _ptr(conf), _ptr(labels),
                                             _ptr(scores), _ptr(margin), _ptr(dots), _ptr(skipped), segments, _stream(torch.device(DEV)))


# ------------------------------------------------------------------------------------------------ 1. the dots are the pinned chain
@pytest.mark.parametrize("N,D,C", [(70, 48, 3), (1, 16, 2), (130, 768, 5)])
def test_dots_are_cluster_assign_scores(model, N, D, C):
    x = dev(unit_rows(N, D, 10 + N))
    bank = dev(0.75 * unit_rows(C + 1, D, 20 + C)).reshape(1, C + 1, D)
    consts = torch.zeros((1, 2 * C + 1), dtype=torch.float32, device=DEV)
    valid = torch.ones((1, C), dtype=torch.uint8, device=DEV)
    dots = torch.full((N, C + 1), 7.0, dtype=torch.float32, device=DEV)
    assert raw_classify(model, x, bank, consts, valid, dots=dots) == _lib.KEEP_OK
    for j in range(C + 1):
        best = model.cluster_assign(x, bank[0, j:j + 1], normalize=False)[1]
        assert torch.equal(dots[:, j].view(torch.int32), best.view(torch.int32)), f"column {j}"


# ------------------------------------------------------------------------------------------------ 2. sampling
def class_sizes(C, shots):
    """Classes of size shots + 1 (the coupon-collector end), 0, below shots, shots and well above, in turn."""
    return [[shots + 1, 0, shots // 2, shots, 3 * shots + 5][c % 5] for c in range(C)]


@pytest.mark.parametrize("C", [2, 5, 63])
@pytest.mark.parametrize("shots", [1, 4, 256])
def test_support_equals_sample_numpy(model, C, shots):
    sizes = class_sizes(C, shots)
    y = np.random.default_rng(C + shots).permutation(np.repeat(np.arange(C), sizes))
    rows, off = fs.class_groups(y, C)
    want = fs.sample_numpy(rows, off, shots, 37, seed=2024)
    whole = model.fewshot_sample(y, C, shots, 37, seed=2024)
    assert whole.support.dtype == torch.int32 and np.array_equal(whole.support.cpu().numpy(), want)
    a, b = model.fewshot_sample(y, C, shots, 5, seed=2024), model.fewshot_sample(y, C, shots, 32, seed=2024, first_episode=5)
    assert torch.equal(torch.cat([a.support, b.support]), whole.support)
    for c, n in enumerate(sizes):
        s = want[:, c]
        assert ((s >= 0).sum(1) == min(n, shots)).all() and (y[s[s >= 0]] == c).all()


# ------------------------------------------------------------------------------------------------ 3. prototypes
def check_bank(protos, train, sup, centre=True):
    """bank / consts / valid against prototypes_numpy in float64, within the bound of the case's own rho."""
    bank, consts, valid, skipped, rho = fs.prototypes_numpy(train, sup, centre)
    C, D = valid.shape[1], train.shape[1]
    per_class = (sup >= 0).sum(2).max()
    dmu, dp = fs.bank_bound(D, int((sup >= 0).sum((1, 2)).max()), int(per_class), rho)
    got = protos.bank.cpu().numpy().astype(np.float64)
    e_mu, e_p = np.abs(got[:, C] - bank[:, C]).max(), np.abs(got[:, :C] - bank[:, :C]).max()
    e_c = np.abs(protos.consts.cpu().numpy() - consts).max()
    print(f"D {D} rho {rho:.3f}: |mu| err {e_mu:.2e} (bound {dmu:.2e}), |p| err {e_p:.2e} (bound {dp:.2e}), consts err {e_c:.2e} "
          f"(bound {fs.consts_bound(D, dmu, dp):.2e})")
    assert e_mu <= dmu and e_p <= dp and e_c <= fs.consts_bound(D, dmu, dp)
    assert np.array_equal(protos.valid.cpu().numpy(), valid) and int(protos.support_skipped) == skipped
    return bank, valid


@pytest.mark.parametrize("sizes,D,noise,shots,E", [([70, 50, 90], 48, 0.25, 4, 23), ([30, 20, 25, 15, 10], 768, 0.06, 16, 3), ([9, 0, 5], 16, 0.4, 6, 4)])
def test_prototypes_against_float64(model, sizes, D, noise, shots, E):
    x, y = blobs(sizes, D, noise, 3)
    sup = model.fewshot_sample(y, len(sizes), shots, E, seed=7)
    for centre in (True, False):
        protos = model.fewshot_prototypes(dev(x), sup, centre=centre, normalize=False)
        bank, valid = check_bank(protos, x, sup.support.cpu().numpy(), centre)
        assert valid.all() == (0 not in sizes)
        if not centre:
            assert not protos.bank[:, len(sizes)].any() and not protos.consts[:, 2 * len(sizes)].any()
    # one episode alone, at the end of the call, and in two calls: the same words
    protos = model.fewshot_prototypes(dev(x), sup, normalize=False)
    alone = model.fewshot_prototypes(dev(x), sup.support[E - 1:], normalize=False)
    head = model.fewshot_prototypes(dev(x), sup.support[:E - 1], normalize=False)
    for name in ("bank", "consts", "valid"):
        whole = getattr(protos, name)
        assert torch.equal(whole[E - 1:], getattr(alone, name)) and torch.equal(whole[:E - 1], getattr(head, name)), name


def test_prototypes_chunked_class_and_dropped_rows(model):
    """300 slots per class (more than one chunk of 256 in the builder); sampled rows holding NaN, inf and 1.5 are dropped and counted."""
    x = unit_rows(700, 16, 8).copy()
    y = np.arange(700) % 2
    sup = np.stack([np.arange(0, 600, 2), np.arange(1, 600, 2)]).reshape(1, 2, 300).astype(np.int32)
    protos = model.fewshot_prototypes(dev(x), dev(sup), normalize=False)
    check_bank(protos, x, sup)
    x[4, 3], x[11, 0], x[298, 15] = np.nan, np.inf, 1.5
    x[650] = 1.5                                                        # not sampled: not counted
    protos = model.fewshot_prototypes(dev(x), dev(sup), normalize=False)
    check_bank(protos, x, sup)
    assert int(protos.support_skipped) == 3
    # shots=None: the same lists.  fewshot_fit makes unit rows first, which turns the row holding 1.5 into a kept one
    fit, same = model.fewshot_fit(dev(x[:600]), y[:600], 2), model.fewshot_prototypes(dev(x[:600]), dev(sup))
    assert torch.equal(fit.bank, same.bank) and torch.equal(fit.consts, same.consts) and int(fit.support_skipped) == int(same.support_skipped) == 2


# ------------------------------------------------------------------------------------------------ 4. classification against float64
NOISE = {16: 0.35, 48: 0.25, 768: 0.06}
_cases = {}


def classify_case(model, C, E, D):
    """Blobs with a common direction (real features' large common mean), the device's prototypes read back and classify_numpy over them
    for 129 test rows: computed once per (C, E, D), shared, never written to."""
    key = (C, E, D)
    if key not in _cases:
        sz = max(5, -(-270 // C))
        x, y = blobs([sz] * C, D, NOISE[D], 40 + C)
        x = x.astype(np.float64) + 1.5 * unit_rows(1, D, 99)[0]
        x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
        train, ytr, test, truth = x[:-129], y[:-129], x[-129:], y[-129:].astype(np.int32)
        protos = model.fewshot_prototypes(dev(train), model.fewshot_sample(ytr, C, 2, E, seed=5), normalize=False)
        ref = fs.classify_numpy(protos.bank.cpu().numpy(), protos.valid.cpu().numpy(), test, truth, consts=protos.consts.cpu().numpy())
        for a in (test, truth):
            a.setflags(write=False)
        _cases[key] = (protos, test, truth, ref)
    return _cases[key]


@pytest.mark.parametrize("D", [16, 48, 768])
@pytest.mark.parametrize("C,E", [(2, 22), (5, 11), (63, 2), (3, 1)])
def test_labels_against_float64(model, C, E, D):
    protos, test, truth, ref = classify_case(model, C, E, D)
    r_min = ref["r"].min()
    bound = fs.margin_bound(D, r_min)
    sure = ref["margin"] > bound
    print(f"C {C} E {E} D {D}: smallest r {r_min:.3f}, margin bound {bound:.2e} ({bound / (D * fs.U):.1f} D u), undecided {1 - sure.mean():.4f}")
    assert bound <= 64 * D * fs.U and 1.0 - sure.mean() <= CAP
    for N in (1, 63, 70, 129):
        conf, labels, skipped = model.fewshot_classify(protos, dev(test[:N]), truth[:N], return_labels=True, normalize=False)
        got = labels.cpu().numpy()
        assert got.shape == (N, E) and int(skipped) == 0
        assert np.array_equal(got[sure[:N]], ref["labels"][:N][sure[:N]])
        assert ((got >= 0) & (got < C)).all()
        on = truth[:N] >= 0
        want = np.stack([np.bincount(truth[:N][on] * C + got[on, e], minlength=C * C).reshape(C, C) for e in range(E)])
        assert np.array_equal(conf.cpu().numpy(), want)
    if E == 1:
        labels, scores, margin, skipped = model.fewshot_predict(protos, dev(test), normalize=False)
        e_s = np.abs(scores.cpu().numpy() - ref["scores"][:, 0]).max()
        e_m = np.abs(margin.cpu().numpy() - ref["margin"][:, 0])[sure[:, 0]].max()
        print(f"scores err {e_s:.2e} (bound {fs.score_bound(D, r_min):.2e}), margin err {e_m:.2e} (bound {fs.margin_out_bound(D, r_min):.2e})")
        assert e_s <= fs.score_bound(D, r_min) and e_m <= fs.margin_out_bound(D, r_min)
        assert np.array_equal(labels.cpu().numpy()[sure[:, 0]], ref["labels"][:, 0][sure[:, 0]])


# ------------------------------------------------------------------------------------------------ 5. invariances
def test_labels_do_not_depend_on_the_launch(model):
    protos, test, truth, _ = classify_case(model, 2, 22, 48)
    x, t = dev(test), dev(truth)
    conf, labels, _ = model.fewshot_classify(protos, x, t, return_labels=True, normalize=False)
    for segments in (1, 2, 7):
        c2, l2, _ = model.fewshot_classify(protos, x, t, return_labels=True, normalize=False, segments=segments)
        assert torch.equal(l2, labels) and torch.equal(c2, conf), segments
    assert torch.equal(model.fewshot_classify(protos, x[5:75], return_labels=True, normalize=False)[1], labels[5:75])
    assert torch.equal(model.fewshot_classify(protos, x[128:], return_labels=True, normalize=False)[1], labels[128:])
    part = model.fewshot_classify(protos.episodes(3, 10), x, return_labels=True, normalize=False)[1]
    assert torch.equal(part, labels[:, 3:10])
    one = model.fewshot_predict(protos.episodes(21, 22), x, normalize=False)[0]
    assert torch.equal(one, labels[:, 21])
    for cut in (1, 64, 65):
        a = model.fewshot_classify(protos, x[:cut], t[:cut], normalize=False)[0]
        b = model.fewshot_classify(protos, x[cut:], t[cut:], normalize=False)[0]
        assert torch.equal(a + b, conf), cut
    lab = labels.cpu().numpy()
    want = np.stack([np.bincount(truth * 2 + lab[:, e], minlength=4).reshape(2, 2) for e in range(22)])
    assert np.array_equal(conf.cpu().numpy(), want)


def test_episodes_do_not_depend_on_the_chunk(model):
    x, y = blobs([70, 50, 90], 48, 0.25, 1)
    args = (dev(x[:105]), y[:105], dev(x[105:]), y[105:], 3, 4)
    whole = model.fewshot_episodes(*args, n_episodes=11, seed=3)
    assert whole.dtype == torch.int64 and tuple(whole.shape) == (11, 3, 3) and (whole.sum((1, 2)) == 105).all()
    for chunk in (1, 5, None):
        assert torch.equal(model.fewshot_episodes(*args, n_episodes=11, seed=3, episode_chunk=chunk), whole), chunk
    assert torch.equal(model.fewshot_episodes(*args, n_episodes=4, seed=3, first_episode=7), whole[7:])


# ------------------------------------------------------------------------------------------------ 6. rules and arguments
def test_rules(model):
    x, y = blobs([40, 0, 30], 32, 0.3, 6)                               # class 1 has no training row: invalid in every episode
    train, ytr, test = x[:40], y[:40], x[40:].copy()
    truth = y[40:].astype(np.int32)
    truth[::4] = -1
    test[3, 5], test[8, 0], test[20, 31] = np.nan, np.inf, 1.5
    protos = model.fewshot_prototypes(dev(train), model.fewshot_sample(ytr, 3, 2, 9, seed=1), normalize=False)
    assert not protos.valid[:, 1].any() and protos.valid[:, [0, 2]].all()
    for segments in (1, 2):
        conf, labels, skipped = model.fewshot_classify(protos, dev(test), truth, return_labels=True, normalize=False, segments=segments)
        lab = labels.cpu().numpy()
        assert (lab[[3, 8, 20]] == -1).all() and int(skipped) == 3
        assert (np.delete(lab, [3, 8, 20], axis=0) >= 0).all() and (lab != 1).all()
        counted = (truth >= 0) & (lab[:, 0] >= 0)
        assert (conf.sum((1, 2)) == int(counted.sum())).all() and not conf[:, :, 1].any() and not conf[:, 1].any()
    # confusion is added into, not overwritten
    acc = conf.clone()
    assert raw_classify(model, dev(test), protos.bank, protos.consts, protos.valid, truth=dev(truth), conf=acc) == _lib.KEEP_OK
    assert torch.equal(acc, 2 * conf)
    # one support row in all: mu is that row, its class's prototype a zero row, the other class invalid.  The test row equal to mu has
    # r = 0 exactly (a one-hot row: every product is exact): label -1, a zero row, in no count
    eye = np.eye(2, 16, dtype=np.float32)
    one = model.fewshot_prototypes(dev(eye), dev(np.array([[[0], [-1]]], np.int32)), normalize=False)
    assert one.valid.tolist() == [[1, 0]] and not one.bank[0, :2].any() and torch.equal(one.bank[0, 2], dev(eye[0]))
    labels, scores, margin, skipped = model.fewshot_predict(one, dev(eye), normalize=False)
    assert labels.tolist() == [-1, 0] and not scores[0].any() and not margin.any() and int(skipped) == 0
    conf = model.fewshot_classify(one, dev(eye), np.array([0, 0]), normalize=False)[0]
    assert conf.tolist() == [[[1, 0], [0, 0]]]


def test_abi_errors_launch_nothing(model):
    lib, h, st = _lib.load(), model._handle, _stream(torch.device(DEV))
    null = C_.c_void_p(0)
    C, D, N, E, shots, M = 3, 32, 8, 2, 4, 20
    x = dev(unit_rows(M, D, 0))
    rows, off = dev(np.arange(M, dtype=np.int32)), dev(np.array([0, 7, 14, 20], np.int64))
    sup = torch.full((E, C, shots), 77, dtype=torch.int32, device=DEV)
    bank = torch.full((E, C + 1, D), 7.0, dtype=torch.float32, device=DEV)
    consts = torch.full((E, 2 * C + 1), 7.0, dtype=torch.float32, device=DEV)
    valid = torch.full((E, C), 7, dtype=torch.uint8, device=DEV)
    labels = torch.full((N, E), 77, dtype=torch.int32, device=DEV)
    conf = torch.full((E, C, C), 5, dtype=torch.int64, device=DEV)
    truth = torch.zeros(N, dtype=torch.int32, device=DEV)
    scores = torch.full((N, C), 7.0, dtype=torch.float32, device=DEV)
    cnt = torch.full((1,), 5, dtype=torch.int64, device=DEV)

    def sample(C=C, shots=shots, first=0, E=E, rows=_ptr(rows), off=_ptr(off), out=_ptr(sup)):
        return lib.keep_fewshot_sample(h, rows, off, C, shots, C_.c_uint64(1), first, E, out, st)

    def build(M=M, D=D, E=E, C=C, shots=shots, centre=1, train=_ptr(x), s=_ptr(sup), b=_ptr(bank), k=_ptr(consts), v=_ptr(valid)):
        return lib.keep_fewshot_prototypes(h, train, M, D, s, E, C, shots, centre, b, k, v, _ptr(cnt), st)

    def classify(N=N, D=D, E=E, C=C, f=_ptr(x), b=_ptr(bank), k=_ptr(consts), v=_ptr(valid), t=_ptr(truth), cf=_ptr(conf), lab=_ptr(labels), sc=null,
                 segments=0):
        return lib.keep_fewshot_classify(h, f, N, D, b, k, v, E, C, t, cf, lab, sc, null, null, _ptr(cnt), segments, st)

    bad = [lambda: sample(C=1), lambda: sample(C=64), lambda: sample(shots=0), lambda: sample(shots=257), lambda: sample(E=0),
           lambda: sample(E=(1 << 16) + 1), lambda: sample(first=-1), lambda: sample(rows=null), lambda: sample(off=null), lambda: sample(out=null),
           lambda: build(C=1), lambda: build(C=64), lambda: build(D=24), lambda: build(D=1040), lambda: build(M=0), lambda: build(shots=0),
           lambda: build(E=0), lambda: build(centre=2), lambda: build(train=null), lambda: build(s=null), lambda: build(b=null), lambda: build(k=null),
           lambda: build(v=null),
           lambda: classify(C=1), lambda: classify(C=64), lambda: classify(D=24), lambda: classify(N=0), lambda: classify(N=(1 << 22) + 1),
           lambda: classify(E=0), lambda: classify(f=null), lambda: classify(b=null), lambda: classify(k=null), lambda: classify(v=null),
           lambda: classify(t=null), lambda: classify(cf=null), lambda: classify(t=null, cf=null, lab=null), lambda: classify(sc=_ptr(scores)),
           lambda: classify(segments=-1), lambda: classify(segments=1025)]
    for i, call in enumerate(bad):
        assert call() == _lib.KEEP_EINVAL, f"bad call {i}"
        assert len(lib.keep_last_error(h)) > 10, f"bad call {i}"
    assert lib.keep_fewshot_sample(None, _ptr(rows), _ptr(off), C, shots, C_.c_uint64(1), 0, E, _ptr(sup), st) == _lib.KEEP_EINVAL
    torch.cuda.synchronize()
    assert (sup == 77).all() and (bank == 7.0).all() and (consts == 7.0).all() and (valid == 7).all() and (labels == 77).all()
    assert (conf == 5).all() and (scores == 7.0).all() and int(cnt) == 5
    model.check_errors()
    # the Python layer refuses the same before any launch
    for call in (lambda: model.fewshot_sample(np.zeros(4, np.int64), 1, 2, 3), lambda: model.fewshot_sample(np.zeros(4, np.int64), 2, 257, 3),
                 lambda: model.fewshot_sample(np.full(4, -1), 2, 2, 3), lambda: model.fewshot_classify(fs.Prototypes(bank, consts, valid, cnt), x[:N])):
        with pytest.raises(ValueError):
            call()
    model.check_errors()


# ------------------------------------------------------------------------------------------------ 7. the layers above
@pytest.fixture(scope="module")
def blob_eval():
    x, y = blobs([120, 80, 100], 48, 0.25, 2)
    x.setflags(write=False)
    return x[:150], y[:150], x[150:], y[150:]


def test_few_shot_protocol(model, blob_eval):
    train, ytr, test, yte = blob_eval
    res = tile_eval.few_shot(model, dev(train), ytr, dev(test), yte, 3, shots=(1, 4), n_episodes=16, seed=4)
    rows, off = fs.class_groups(ytr, 3)
    for k in (1, 4):
        sup = fs.sample_numpy(rows, off, k, 16, seed=4)
        bank, consts, valid, _, rho = fs.prototypes_numpy(train, sup)
        ref = fs.classify_numpy(bank, valid, test, yte)
        dmu, dp = fs.bank_bound(48, 3 * k, k, rho)
        bound = fs.end_to_end_margin_bound(48, ref["r"].min(), dmu, dp)
        undecided = (ref["margin"] <= bound).sum(0)
        conf = res[k]["confusions"]
        print(f"{k} shots: rho {rho:.3f}, bound {bound:.2e}, undecided pairs {int(undecided.sum())}, median balanced accuracy "
              f"{res[k]['balanced_accuracy_median']:.4f}")
        assert undecided.sum() <= CAP * ref["margin"].size
        assert conf.shape == (16, 3, 3) and (conf.sum((1, 2)) == 150).all()
        assert (np.abs(conf - ref["confusion"]).sum((1, 2)) <= 2 * undecided).all()
        from keep_amd import bootstrap
        assert np.array_equal(res[k]["balanced_accuracy"], bootstrap.balanced_accuracy(conf))
        assert np.allclose(res[k]["weighted_f1"], [tile_eval.weighted_f1_from_confusion(c) for c in conf], rtol=0, atol=1e-15)
        q1, med, q3 = np.percentile(res[k]["weighted_f1"], [25, 50, 75])
        assert (res[k]["weighted_f1_q1"], res[k]["weighted_f1_median"], res[k]["weighted_f1_q3"]) == (q1, med, q3)
        assert res[k]["weighted_f1_mean"] == res[k]["weighted_f1"].mean()
    assert res[4]["balanced_accuracy_median"] >= res[1]["balanced_accuracy_median"]


def test_fit_and_predict_against_nearest_centroid(model, blob_eval):
    from sklearn.neighbors import NearestCentroid
    train, ytr, test, yte = blob_eval
    protos = model.fewshot_fit(dev(train), ytr, 3)
    labels, scores, margin, skipped = model.fewshot_predict(protos, dev(test))
    mu = train.astype(np.float64).mean(0)
    z = train.astype(np.float64) - mu
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    q = test.astype(np.float64) - mu
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    want = NearestCentroid().fit(z, ytr).predict(q)
    rows, off = fs.class_groups(ytr, 3)
    sup = np.full((1, 3, int(np.diff(off).max())), -1, np.int32)
    for c in range(3):
        sup[0, c, :off[c + 1] - off[c]] = rows[off[c]:off[c + 1]]
    bank, _, valid, _, rho = fs.prototypes_numpy(train, sup)
    ref = fs.classify_numpy(bank, valid, test)
    dmu, dp = fs.bank_bound(48, 150, sup.shape[2], rho)
    sure = ref["margin"][:, 0] > fs.end_to_end_margin_bound(48, ref["r"].min(), dmu, dp)
    assert 1.0 - sure.mean() <= CAP and int(skipped) == 0
    assert np.array_equal(ref["labels"][sure, 0], want[sure]) and np.array_equal(labels.cpu().numpy()[sure], want[sure])
    assert (labels.cpu().numpy() == yte).mean() > 0.9
    one = model.fewshot_fit(dev(train), ytr, 3, shots=4, seed=9)          # one sampled episode
    assert torch.equal(one.bank, model.fewshot_prototypes(dev(train), model.fewshot_sample(ytr, 3, 4, 1, seed=9)).bank)


def test_prototype_map_and_slide_call(model, blob_eval):
    train, ytr, test, _ = blob_eval
    gw, gh, P, d = 15, 10, 256, 16
    shape = (gh * P // d, gw * P // d)
    x = test.copy()
    x[50, 3] = np.nan
    coords = np.stack([np.arange(gw * gh) % gw * P, np.arange(gw * gh) // gw * P], axis=1).astype(np.int64)
    protos = model.fewshot_fit(dev(train), ytr, 3)
    raster = wsi.prototype_map(protos, dev(x), torch.from_numpy(coords), d, shape, patch_size=P, model=model)
    labels, scores, _, skipped = model.fewshot_predict(protos, dev(x))
    lab = labels.cpu().numpy()
    keep = lab >= 0
    assert isinstance(raster, ClassRaster) and raster.n_classes == 3 and raster.shape == shape and raster.tiles == 149
    assert int(skipped) == 1 and not keep[50] and keep.sum() == 149
    want = class_raster_numpy(coords[keep], one_hot_numpy(lab[keep], 3), P, d, shape)
    assert torch.equal(raster.acc.cpu(), torch.from_numpy(want))
    label, pooled = wsi.prototype_slide_call(protos, dev(x), top=7, model=model)
    want_label, want_pooled = fs.slide_call_numpy(scores.cpu().numpy()[keep], 7)
    assert label == want_label and np.abs(pooled.cpu().numpy() - want_pooled).max() <= 8 * fs.U
    assert wsi.prototype_slide_call(protos, dev(x[:3]), top=7, model=model)[0] in (0, 1, 2)
