"""keep_amd.calibration on a CPU: the rule of ``KEEPModel.calibrate`` against the same rule written out a second time in float64, the variance
shares on a planted additive model, the plan search with a scripted verification, the probe's validation and the report's key set.

Inputs are seeded fp32 tensors: D = 64, P = 8 unit prompts, groups of 16 tiles, f = normalize(ref_f + noise)."""
import math

import numpy as np
import pytest
import torch

from keep_amd import _lib
from keep_amd import calibration as cal

D, P, NT = 64, 8, 16
POPULATION, CONFIDENCE = 1.0e6, 0.99
# probe_statistics reduces fp32 tensors of at most 16 x 64 elements where the float64 restatement below does not: 1024 x 6e-8 = 6e-5
REL = 1e-4


# ------------------------------------------------------------------------------------------------ the rule, a second time (float64)
def _mix_quantile(sig, n, q):
    """x with prod_i (1 - erfc(x / (s_i sqrt 2)))^(n / len) = q (every sigma stands for n / len errors); 0 if no sigma is positive."""
    pos = [s for s in sig if s > 0.0]
    if not pos:
        return 0.0
    lo, hi = 0.0, 50.0 * max(pos)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        log_p = sum(max(n, 1.0) / len(sig) * math.log1p(-min(math.erfc(mid / (s * math.sqrt(2.0))), 1.0 - 1e-300)) for s in pos)
        lo, hi = (mid, hi) if log_p < math.log(q) else (lo, mid)
    return 0.5 * (lo + hi)


def _mix_exceedance(sig, n, x):
    pos = [s for s in sig if s > 0.0]
    return -math.expm1(sum(max(n, 1.0) / len(sig) * math.log1p(-math.erfc(x / (s * math.sqrt(2.0)))) for s in pos)) if pos else 0.0


def _rule(f, ref_f, sim, ref_sim, members, population, confidence, tolerance):
    """The docstring rule of KEEPModel.calibrate, group by group -> ({name: figures}, anisotropy, governing name, prediction)."""
    f, ref_f, sim, ref_sim = (t.double().numpy() for t in (f, ref_f, sim, ref_sim))
    z = _mix_quantile([1.0], population, confidence)
    d2, e2 = (sim - ref_sim) ** 2, ((f - ref_f) ** 2).sum(axis=1) / f.shape[1]
    out = {}
    for name, idx in members:
        i = idx.numpy()
        ms = e2[i].mean()
        se = e2[i].std(ddof=1) / math.sqrt(len(i)) / ms if len(i) > 1 and ms > 0 else 0.0            # two standard errors of the mean squared error
        out[name] = {"max_abs": math.sqrt(d2[i].max()), "rms_bank": math.sqrt(d2[i].mean()), "rms_iso": math.sqrt(ms),
                     "margin": max(cal.PROBE_RMS_MARGIN, math.sqrt(1.0 + 2.0 * se))}
    ratios = [g["rms_bank"] / g["rms_iso"] for g in out.values() if g["rms_iso"] > 0]
    aniso = max(1.0, float(np.median(ratios))) if ratios else 1.0
    for name, idx in members:
        g, tile = out[name], np.sqrt(e2[idx.numpy()])
        allowed = _mix_quantile((tile * aniso).tolist(), len(tile) * sim.shape[1], 0.99)
        g["tail"] = max(1.0, g["max_abs"] / allowed) if allowed > 0 else 1.0
        g["sigmas"] = (tile * aniso * g["margin"] * g["tail"]).tolist()
        g["predicted"] = _mix_quantile(g["sigmas"], population, confidence)
        g["effective_rms"], g["rms"] = g["predicted"] / z, g["rms_iso"] * aniso
        g["exceedance"] = _mix_exceedance(g["sigmas"], population, tolerance)
    gov = max(out, key=lambda k: out[k]["predicted"])
    return out, aniso, gov, out[gov]["predicted"]


def _probe(scales, seed, identical=()):
    """One group of NT tiles per entry of ``scales`` (per-element noise std); groups named in ``identical`` hold NT copies of one tile whose
    error vector points along the first prompt.  -> (f, ref_f, sim, ref_sim, members, bank)"""
    g = torch.Generator().manual_seed(seed)
    n = NT * len(scales)
    bank = torch.nn.functional.normalize(torch.randn(P, D, generator=g), dim=-1)
    ref_f = torch.nn.functional.normalize(torch.randn(n, D, generator=g), dim=-1)
    noise = torch.randn(n, D, generator=g) * torch.tensor(scales).repeat_interleave(NT)[:, None]
    members = [("abcdefgh"[k], torch.arange(k * NT, (k + 1) * NT)) for k in range(len(scales))]
    for name, idx in members:
        if name in identical:
            ref_f[idx] = ref_f[idx[0]].clone()
            noise[idx] = bank[0] * scales[idx[0] // NT] * math.sqrt(D)
    f = torch.nn.functional.normalize(ref_f + noise, dim=-1)
    return f, ref_f, f @ bank.t(), ref_f @ bank.t(), members, bank


def _check_against_rule(inputs, tolerance):
    f, ref_f, sim, ref_sim, members, _ = inputs
    s = cal.probe_statistics(f, ref_f, sim.clone(), ref_sim, members, POPULATION, CONFIDENCE, tolerance)
    want, aniso, gov, pred = _rule(f, ref_f, sim, ref_sim, members, POPULATION, CONFIDENCE, tolerance)
    assert [g.name for g in s.groups] == [name for name, _ in members] and set(s.per_group) == set(want) | {"anisotropy_factor"}
    for g in s.groups:
        w = want[g.name]
        print(g.name, {k: (getattr(g, k), w[k]) for k in ("max_abs", "rms_bank", "rms_iso", "margin", "rms", "tail", "effective_rms")})
        for k in ("max_abs", "rms_bank", "rms_iso", "margin", "rms", "tail", "effective_rms"):
            assert getattr(g, k) == pytest.approx(w[k], rel=REL), (g.name, k)
        assert g.tiles == NT and list(g.sigmas) == pytest.approx(w["sigmas"], rel=REL)
        rep = s.per_group[g.name]
        assert rep["tiles"] == NT and rep["margin"] == round(g.margin, 4) and rep["tail_factor"] == round(g.tail, 3)
        for k, v in (("max_abs_dcos", g.max_abs), ("rms_dcos_vs_bank", g.rms_bank), ("rms_dcos_isotropic", g.rms_iso), ("effective_rms", g.effective_rms)):
            assert rep[k] == float(f"{v:.3e}")                                      # the report's own rounding
        assert rep["hardest_tile_over_rms"] == pytest.approx(max(w["sigmas"]) / (w["rms"] * w["margin"] * w["tail"]), abs=1e-3)
        # the exceedance probability moves ~ z^2 = 30 times as fast as a sigma, and the report keeps 4 significant digits of it
        assert rep["exceedance_probability"] == pytest.approx(w["exceedance"], rel=30 * REL + 5e-4)
    assert s.anisotropy == pytest.approx(aniso, rel=REL) and s.per_group["anisotropy_factor"] == round(s.anisotropy, 4)
    assert s.governing.name == gov and s.predicted == pytest.approx(pred, rel=REL)
    assert s.max_abs == max(g.max_abs for g in s.groups)
    return s, want


def test_equal_noise_reduces_to_rms_times_the_quantile():
    s, want = _check_against_rule(_probe([1e-3, 1e-3], seed=1), tolerance=8e-3)
    z = cal.max_sigmas_quantile(POPULATION, CONFIDENCE)
    assert s.predicted == s.governing.effective_rms * z
    assert all(g.tail == 1.0 for g in s.groups)                                         # exactly: no group's maximum is above what its mixture allows
    # the per-tile errors are nearly equal, so the effective rms is the group's rms x anisotropy x margin, a little above (the hardest tiles count more)
    for g in s.groups:
        assert g.rms * g.margin <= g.effective_rms <= 1.15 * g.rms * g.margin
    assert 0.0 < s.per_group[s.governing.name]["exceedance_probability"] < 1.0 - CONFIDENCE


def test_the_noisier_group_governs():
    s, want = _check_against_rule(_probe([1e-3, 4e-3], seed=2), tolerance=3e-2)
    assert s.governing.name == "b" and s.governing is s.groups[1]
    assert s.groups[1].rms_iso == pytest.approx(4.0 * s.groups[0].rms_iso, rel=0.2) and s.predicted > 3.0 * want["a"]["predicted"]
    flipped, _ = _check_against_rule(_probe([4e-3, 1e-3], seed=2), tolerance=3e-2)
    assert flipped.governing.name == "a"


def test_a_planted_outlier_stretches_the_tail():
    inputs = _probe([1e-3, 1e-3], seed=3)
    inputs[2][NT + 3, 2] += 2e-2                                                          # one cosine of group b, twenty times its rms
    s, want = _check_against_rule(inputs, tolerance=3e-2)
    a, b = s.groups
    assert a.tail == 1.0 and b.tail > 1.0 and s.governing.name == "b"
    tile_rms = ((inputs[0] - inputs[1]).double().pow(2).sum(1) / D).sqrt()[NT:]
    allowed = _mix_quantile((tile_rms * s.anisotropy).tolist(), NT * P, 0.99)
    assert b.tail == pytest.approx(b.max_abs / allowed, rel=REL) and b.max_abs == pytest.approx(2e-2, rel=0.2)


def test_anisotropy_is_the_median_over_the_groups():
    """Group c: 16 copies of one tile with one error vector, along a prompt -- its bank rms is a single draw, far above the isotropic figure."""
    s, want = _check_against_rule(_probe([1e-3, 1e-3, 1e-3], seed=4, identical=("c",)), tolerance=8e-3)
    ratios = sorted(g.rms_bank / g.rms_iso for g in s.groups)
    c = s.groups[2]
    assert c.rms_bank / c.rms_iso == ratios[-1] > 2.0                                    # |e . t| over the bank against |e| / sqrt(D): at least sqrt(D / P)
    assert s.anisotropy == pytest.approx(max(1.0, ratios[1]), rel=REL) and s.anisotropy < 0.7 * ratios[-1]
    assert c.margin == cal.PROBE_RMS_MARGIN                                              # no tile-to-tile spread: the floor of the margin
    assert list(c.sigmas) == pytest.approx([c.sigmas[0]] * NT, rel=1e-6)


def test_zero_error_is_all_zeros_and_accepted():
    _, ref_f, _, ref_sim, members, _ = _probe([0.0, 0.0], seed=5)
    f, sim = ref_f.clone(), ref_sim.clone()
    s = cal.probe_statistics(f, ref_f, sim.clone(), ref_sim, members, POPULATION, CONFIDENCE, 1e-4)
    for g in s.groups:
        assert (g.max_abs, g.rms_bank, g.rms_iso, g.rms, g.effective_rms) == (0.0,) * 5 and set(g.sigmas) == {0.0}
        assert g.margin == cal.PROBE_RMS_MARGIN and g.tail == 1.0
        assert s.per_group[g.name]["exceedance_probability"] == 0.0 and s.per_group[g.name]["hardest_tile_over_rms"] == 0.0
    assert s.predicted == 0.0 and s.max_abs == 0.0 and s.anisotropy == 1.0
    plan = cal.prefix_plan(2, 0, 0)
    assert cal.search([plan], lambda p: s, 1e-4)[0] == plan


@pytest.mark.parametrize("tile", [0, NT + 5])
def test_a_nan_feature_is_never_accepted(tile):
    """Wherever the NaN sits (the first tile of the first group, the middle of the second) the prediction is NaN and no tolerance accepts it."""
    f, ref_f, _, ref_sim, members, bank = _probe([1e-3, 1e-3], seed=6)
    f[tile, 3] = float("nan")
    s = cal.probe_statistics(f, ref_f, f @ bank.t(), ref_sim, members, POPULATION, CONFIDENCE, 1.0)
    assert math.isnan(s.predicted) and math.isnan(s.governing.effective_rms) and s.governing.name == "ab"[tile // NT]
    other = s.groups[1 - tile // NT]
    assert math.isfinite(other.effective_rms) and other.effective_rms > 0                # the clean group keeps its figures
    plans = cal.ladder_candidates(2)
    chosen, stats, tried = cal.search(plans, lambda p: s, 1.0)
    assert chosen is None and stats is None and len(tried) == len(plans) and all(math.isnan(t["predicted_max_abs_dcos"]) for t in tried)


# ------------------------------------------------------------------------------------------------ variance shares
def test_measure_shares_recovers_a_planted_additive_model():
    depth, names = 3, ("x", "y")
    members = [("x", torch.arange(0, 16)), ("y", torch.arange(16, 34))]
    floor = [2e-13, 5e-13]
    attn = [[3.2e-10, 1.1e-10], [4.0e-11, 9.5e-11], [1.5e-11, 2.5e-11]]                   # [block][group]
    mlp = [[2.1e-10, 6.4e-10], [1.3e-10, 3.3e-10], [7.0e-11, 8.0e-11]]
    left_a = {_lib.ATTN_PLAIN: 1.0, _lib.ATTN_SPLIT: 0.0, _lib.ATTN_SPLIT_COMPQKV: 0.0125, _lib.ATTN_COMPQKV: 0.625, _lib.ATTN_COMPQKV_PROJ_CLS: 0.25,
              _lib.ATTN_PROJ_CLS: [0.75, 0.5, 0.375]}                                      # the CLS-row treatments leave another fraction in every block
    left_m = {_lib.MLP_PLAIN: 1.0, _lib.MLP_SPLIT: 0.0, _lib.MLP_COMP: 0.03125, _lib.MLP_COMP_W: 0.4375, _lib.MLP_CLS: [0.0625, 0.015625, 0.0078125]}
    left = lambda table, mode, i: table[mode][i] if isinstance(table[mode], list) else table[mode]
    calls = []

    def iso_var(plan):
        calls.append(list(plan))
        return [floor[g] + sum(attn[i][g] * left(left_a, a, i) + mlp[i][g] * left(left_m, m, i) for i, (a, m) in enumerate(plan)) for g in range(2)]

    sh = cal.measure_shares(iso_var, depth, members)
    # the sweep of the measurement (one encode of the share probe per call -- calibration time is encode time):
    #   the all-split floor; every block's attention side plain, then every block's MLP plain; MLP_CLS in every block; MLP_COMP and MLP_COMP_W
    #   in blocks {0, depth // 2}; the three compensated-qkv attention modes in blocks {0, min(1, depth - 1), depth // 2}; ATTN_PROJ_CLS in every block
    split = (_lib.ATTN_SPLIT, _lib.MLP_SPLIT)
    one = lambda i, mode: [mode if j == i else split for j in range(depth)]
    sampled_m, sampled_a = sorted({0, depth // 2}), sorted({0, min(1, depth - 1), depth // 2})
    want_calls = ([[split] * depth] + [one(i, (_lib.ATTN_PLAIN, _lib.MLP_SPLIT)) for i in range(depth)] + [one(i, (_lib.ATTN_SPLIT, _lib.MLP_PLAIN)) for i in range(depth)]
                  + [one(i, (_lib.ATTN_SPLIT, _lib.MLP_CLS)) for i in range(depth)]
                  + [one(i, (_lib.ATTN_SPLIT, m)) for m in (_lib.MLP_COMP, _lib.MLP_COMP_W) for i in sampled_m]
                  + [one(i, (a, _lib.MLP_SPLIT)) for a in (_lib.ATTN_SPLIT_COMPQKV, _lib.ATTN_COMPQKV, _lib.ATTN_COMPQKV_PROJ_CLS) for i in sampled_a]
                  + [one(i, (_lib.ATTN_PROJ_CLS, _lib.MLP_SPLIT)) for i in range(depth)])
    assert len(want_calls) == 1 + 2 * depth + depth + 2 * len(sampled_m) + 3 * len(sampled_a) + depth == 23
    assert calls == want_calls
    r3, r4 = (lambda v: float(f"{v:.3e}")), (lambda v: float(f"{v:.4f}"))
    for g, name in enumerate(names):
        got = sh["by_group"][name]
        assert got["attn"] == [r3(attn[i][g]) for i in range(depth)] and got["mlp"] == [r3(mlp[i][g]) for i in range(depth)] and got["floor"] == r3(floor[g])
        assert got["residual_mlp"] == {k: ([r4(x) for x in v] if isinstance(v, list) else r4(v)) for k, v in left_m.items()}
        assert got["residual_attn"] == {k: ([r4(x) for x in v] if isinstance(v, list) else r4(v)) for k, v in left_a.items()}
        assert got["probe_tiles"] == (16, 18)[g]
    assert sh["attn"] == [r3(max(a)) for a in attn] and sh["mlp"] == [r3(max(m)) for m in mlp] and sh["floor"] == r3(max(floor))
    assert sh["residual_mlp"] == sh["by_group"]["x"]["residual_mlp"] and sh["residual_attn"] == sh["by_group"]["x"]["residual_attn"]
    assert sh["groups"] == list(names) and sh["probe_tiles"] == 34 and set(sh) == {"attn", "mlp", "floor", "residual_mlp", "residual_attn", "probe_tiles", "groups", "by_group"}
    # the greedy walk reads these shares: from all-plain it ends with every site treated, the worst group's variance falling all the way
    walk = cal.greedy_walk(sh, depth, cal.DEFAULT_KNOBS)
    assert walk[0][0] == [(0, 0)] * depth and walk[0][1] == pytest.approx(max(floor[g] + sum(attn[i][g] + mlp[i][g] for i in range(depth)) for g in range(2)), rel=1e-3)
    # ... to every attention side split (nothing left) and every MLP at the better of MLP_CLS and MLP_COMP: group y's 5e-13 + 6.4e-10 / 32 + 3.3e-10 / 64 + 8e-11 / 128
    best = max(floor[g] + sum(mlp[i][g] * min(left_m[_lib.MLP_CLS][i], left_m[_lib.MLP_COMP]) for i in range(depth)) for g in range(2))
    assert all(b[1] <= a[1] for a, b in zip(walk, walk[1:])) and walk[-1][1] == pytest.approx(best, rel=1e-3) and all(a == _lib.ATTN_SPLIT for a, _ in walk[-1][0])


def test_share_probe_takes_a_sixteenth_of_every_group():
    members = [("a", torch.arange(0, 40)), ("b", torch.arange(40, 340)), ("c", torch.arange(340, 350))]
    sel, sub = cal.share_probe(members)
    assert sel.tolist() == list(range(0, 16)) + list(range(40, 58)) + list(range(340, 350))          # 16 at least, 300 // 16 = 18, all 10 of a small group
    assert [(n, i.tolist()) for n, i in sub] == [("a", list(range(0, 16))), ("b", list(range(16, 34))), ("c", list(range(34, 44)))]


def test_every_mode_has_a_price():
    cost_a, cost_m = cal.knob_costs()
    assert set(cost_a) == set(range(6)) and set(cost_m) == set(range(5)) and cost_a[_lib.ATTN_PLAIN] == cost_m[_lib.MLP_PLAIN] == 0.0
    assert cost_a[_lib.ATTN_SPLIT] == cal.KNOB_COST_MS["attn_split"] and cost_m[_lib.MLP_SPLIT] == 3.0 * cal.KNOB_COST_MS["mlp_comp"]


# ------------------------------------------------------------------------------------------------ the search
def _stats(pred):
    g = cal.GroupStats("g", NT, max_abs=pred / 4, rms_bank=pred / 6, rms_iso=pred / 7, margin=1.02, rms=pred / 7, tail=1.0, sigmas=[pred / 6] * NT, effective_rms=pred / 6)
    return cal.ProbeStats([g], g, 1.0, g.max_abs, pred, {"g": {"rms_dcos_isotropic": float(f"{g.rms_iso:.3e}")}, "anisotropy_factor": 1.0})


def _scripted(predictions):
    """verify(plan) -> the scripted prediction of that plan; .seen = the plans in the order they were verified."""
    seen = []

    def verify(plan):
        seen.append(plan)
        return _stats(predictions[cal.plan_string(plan)])
    verify.seen = seen
    return verify


def test_ladder_stops_at_the_first_rung_that_passes():
    rungs = cal.ladder_candidates(2)
    assert rungs == [cal.prefix_plan(2, *r) for r in ((0, 0), (0, 2), (1, 2), (2, 2))]                 # 16 rungs clip to 4 distinct plans at depth 2
    assert len(cal.ladder_candidates(24)) == len(cal.COMP_LADDER) and cal.ladder_candidates(24)[-1] == cal.prefix_plan(24, 24, 24)
    verify = _scripted(dict(zip(map(cal.plan_string, rungs), (3e-4, 2e-4, 5e-5, 1e-5))))
    chosen, stats, tried = cal.search(rungs, verify, 1e-4)
    assert chosen == rungs[2] and stats.predicted == 5e-5 and verify.seen == rungs[:3]
    assert [(t["comp_full_blocks"], t["comp_mlp_blocks"], t["predicted_max_abs_dcos"]) for t in tried] == [(0, 0, 3e-4), (0, 2, 2e-4), (1, 2, 5e-5)]
    assert set(tried[0]) == {"comp_full_blocks", "comp_mlp_blocks", "plan", "max_abs_dcos", "rms_dcos", "rms_dcos_vs_bank", "rms_dcos_isotropic", "governing_group",
                             "predicted_max_abs_dcos", "isotropic_rms_by_group", "anisotropy_factor"}
    assert tried[2]["plan"] == cal.plan_string(rungs[2]) and tried[2]["governing_group"] == "g" and tried[2]["isotropic_rms_by_group"] == {"g": float(f"{5e-5 / 7:.3e}")}


def test_measured_walks_up_one_knob_at_a_time_without_bisecting():
    depth, tol = 8, 1e-4
    rms_target = tol / (cal.max_sigmas_quantile(POPULATION, CONFIDENCE) * cal.PROBE_RMS_MARGIN)
    plans = [[(_lib.ATTN_PLAIN, _lib.MLP_CLS if i < k else _lib.MLP_PLAIN) for i in range(depth)] for k in range(8)]
    # predicted variances of the walk in units of rms_target^2: step 2 is the first at or under 1.06^2 = 1.1236
    walk = list(zip(plans, (v * rms_target ** 2 for v in (9.0, 1.2, 1.12, 0.9, 0.7, 0.5, 0.3, 0.1))))
    cands = cal.walk_candidates(walk, rms_target)
    assert cands == plans[2:]
    # what verifying finds is NOT monotone along the walk: steps 3, 6 and 7 pass.  Walking up keeps step 3; a bisection of [2, 7] would look at
    # step 4 (fails), go up to 6 (passes), then 5 (fails) and keep step 6
    verify = _scripted(dict(zip(map(cal.plan_string, plans), (5e-4, 4e-4, 1.5e-4, 0.9e-4, 1.2e-4, 1.3e-4, 0.8e-4, 0.5e-4))))
    chosen, stats, tried = cal.search(cands, verify, tol)
    assert chosen == plans[3] and stats.predicted == 0.9e-4 and verify.seen == plans[2:4] and len(tried) == 2
    assert tried[0]["comp_full_blocks"] is None and tried[0]["plan"] == "attn:00000000 mlp:44000000"                # not a prefix plan
    # a walk that never reaches the target is verified at its last step only
    assert cal.walk_candidates(walk[:2], rms_target) == [plans[1]]


def test_nothing_passes_returns_no_plan_and_every_candidate():
    rungs = cal.ladder_candidates(3)
    verify = _scripted({cal.plan_string(p): 2e-4 for p in rungs})
    chosen, stats, tried = cal.search(rungs, verify, 1e-4)
    assert chosen is None and stats is None and [t["plan"] for t in tried] == [cal.plan_string(p) for p in rungs] and verify.seen == rungs


# ------------------------------------------------------------------------------------------------ validation and the default probe
def test_probe_members_validates_and_names_the_groups():
    with pytest.raises(ValueError, match="^groups: one non-negative group index per probe tile$"):
        cal.probe_members(torch.zeros(3, dtype=torch.int64), None, 4, "cpu")
    with pytest.raises(ValueError, match="^groups: one non-negative group index per probe tile$"):
        cal.probe_members(torch.tensor([0, -1, 0, 1]), None, 4, "cpu")
    with pytest.raises(ValueError, match="^group_names: one name per group index$"):
        cal.probe_members(torch.tensor([0, 1, 2, 2]), ("a", "b"), 4, "cpu")
    (name, idx), = cal.probe_members(None, None, 4, "cpu")
    assert name == "group0" and idx.tolist() == [0, 1, 2, 3]
    got = cal.probe_members([0, 2, 0, 2], ("a", "b", "c"), 4, "cpu")                                   # an empty group is left out
    assert [(n, i.tolist()) for n, i in got] == [("a", [0, 2]), ("c", [1, 3])]
    assert cal.probe_members(None, ("only",), 0, "cpu") == []


def test_default_probe_is_the_mixture_or_gaussian_pixels(monkeypatch):
    from keep_amd import synth
    with pytest.raises(ValueError, match="^probe must be 'mixture' or 'gaussian'$"):
        cal.default_probe("he_crops", 16, "cpu", 5)
    # default_probe("mixture", 16, "cpu", seed) IS calibration_probe(4, "cpu", seed) -- 16 tiles over the four families.  The generator draws whole
    # 256-tile units of every structured family (seconds on a CPU; tests/test_tile_families.py runs it for real and checks that it is deterministic),
    # so here a recording stand-in takes its place
    made = []

    def recorded(n_per_family, device, seed=None):
        made.append((n_per_family, device, seed))
        return torch.full((n_per_family * 4,), float(seed)), torch.arange(4).repeat_interleave(n_per_family), synth.PROBE_FAMILIES
    monkeypatch.setattr(synth, "calibration_probe", recorded)
    tiles, groups, names = cal.default_probe("mixture", 16, "cpu", 5)
    assert made == [(4, "cpu", 5)] and tiles.tolist() == [5.0] * 16 and groups.tolist() == [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4 and names == synth.PROBE_FAMILIES
    assert cal.default_probe("mixture", 3, "cpu", 6)[0].numel() == 4 and made[-1] == (1, "cpu", 6)              # at least one tile of every family
    tiles, groups, names = cal.default_probe("gaussian", 3, "cpu", 5)
    assert tuple(tiles.shape) == (3, 3, 224, 224) and tiles.dtype == torch.bfloat16 and groups is None and names == ("gaussian",)
    assert torch.equal(tiles, cal.default_probe("gaussian", 3, "cpu", 5)[0])


# ------------------------------------------------------------------------------------------------ the report
BASE_KEYS = {"precision", "comp_full_blocks", "comp_mlp_blocks", "plan", "budget", "population", "confidence", "max_sigmas_quantile", "expected_max_sigmas",
             "target_rms_dcos", "strict_blocks", "probe", "probe_distribution", "probe_groups", "tried", "bias_correction"}
CHOSEN_KEYS = {"probe_max_abs_dcos", "probe_rms_dcos", "tail_factor", "rms_margin", "governing_group", "per_group", "predicted_max_abs_dcos", "exceedance_probability",
               "label_margin", "label_margin_per_unit_prompt_distance", "label_population"}


def test_report_has_the_keys_calibrate_always_wrote():
    s = _stats(8e-5)
    common = dict(tried=[{"plan": "x"}], budget="measured", population=float(cal.CALIBRATION_POPULATION), confidence=0.99, tolerance=1e-4, strict_blocks=1,
                  probe_tiles=40, prompts=7, probe_name="caller's tiles", group_names=["g"], bias_correction=False)
    unit, n_margins = cal.label_margin_unit(s.governing.sigmas, float(cal.CALIBRATION_POPULATION), None, 0.99)
    assert n_margins == 100_000.0 and unit == cal.mixture_max_quantile(s.governing.sigmas, 100_000.0, 0.99)
    assert cal.label_margin_unit([1e-5], 5e6, None, 0.99)[1] == 5e6 and cal.label_margin_unit([1e-5], 5e6, 1234, 0.99)[1] == 1234.0
    plan = [(_lib.ATTN_PROJ_CLS, _lib.MLP_CLS), (_lib.ATTN_PLAIN, _lib.MLP_CLS)]
    rep = cal.calibration_report(chosen=plan, stats=s, shares={"attn": []}, label_unit=unit, label_population=n_margins, **common)
    assert set(rep) == BASE_KEYS | CHOSEN_KEYS | {"variance_shares"}
    z = cal.max_sigmas_quantile(cal.CALIBRATION_POPULATION, 0.99)
    assert rep["precision"] == "comp" and rep["plan"] == "attn:40 mlp:44" and rep["comp_full_blocks"] is None and rep["comp_mlp_blocks"] is None
    assert rep["probe"] == "40 tiles x 7 prompts vs the split-product arithmetic" and rep["probe_distribution"] == "caller's tiles" and rep["probe_groups"] == ["g"]
    assert rep["max_sigmas_quantile"] == round(z, 3) and rep["target_rms_dcos"] == float(f"{1e-4 / (z * cal.PROBE_RMS_MARGIN):.3e}") and rep["strict_blocks"] == 1
    assert rep["predicted_max_abs_dcos"] == 8e-5 and rep["governing_group"] == "g" and rep["rms_margin"] == 1.02 and rep["tail_factor"] == 1.0
    assert rep["label_margin_per_unit_prompt_distance"] == float(f"{unit:.3e}") and rep["label_margin"] == float(f"{math.sqrt(2.0) * unit:.3e}")
    assert rep["exceedance_probability"] == float(f"{cal.mixture_exceedance(s.governing.sigmas, cal.CALIBRATION_POPULATION, 1e-4):.3e}")
    assert rep["tried"] is common["tried"] and rep["per_group"] is s.per_group and rep["label_population"] == 100_000.0
    # a prefix plan is reported as its shorthand too; nothing chosen: the strict record, without the figures of a plan
    assert cal.calibration_report(chosen=cal.prefix_plan(2, 1, 2), stats=s, shares=None, **common)["comp_full_blocks"] == 1
    none = cal.calibration_report(chosen=None, stats=None, shares=None, **common)
    assert set(none) == BASE_KEYS and none["precision"] == "strict" and none["plan"] is None
