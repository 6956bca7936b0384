"""How the 'comp' mode's per-block precision plan is chosen: the extreme-value rule, the probe statistics, the variance shares and the plan search.

Pure functions over tensors (on any device, the CPU included), floats and dicts: no ctypes and no engine handle -- ``_lib`` is imported for the mode
constants only.  ``KEEPModel.calibrate`` (keep_amd.model) is the driver: it encodes the probe and hands the results to ``probe_statistics``,
``measure_shares`` and ``search`` through small callbacks, then stores ``calibration_report``.  ``keep_amd.model`` re-exports the public names.
"""
from __future__ import annotations

import math
from typing import Callable, Iterable, List, Mapping, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib

# 'comp' spends its precision budget block by block (keep_set_block_precision): a PLAN is one (attention-side mode, MLP mode) pair per ViT block,
# modes as in include/keep_hip.h (KEEP_ATTN_*, KEEP_MLP_*).  The prefix shorthand (comp_full_blocks, comp_mlp_blocks) = the first blocks' attention
# side as split products / the first blocks' MLP GEMMs with both MX-fp4 correction terms is one family of plans; calibrate() walks it from the
# cheapest rung up (budget="ladder") or builds a plan from variance shares measured on the loaded weights (budget="measured").
COMP_LADDER = ((0, 0), (0, 4), (1, 4), (1, 6), (1, 8), (2, 8), (1, 10), (2, 10), (1, 12), (2, 12), (2, 14), (2, 16), (2, 24), (4, 24), (8, 24), (24, 24))
# calibrate() keeps the cheapest plan whose probe statistics predict, with probability CONFIDENCE, a worst cosine error inside TOLERANCE over the
# POPULATION the model will be used on (tiles x distinct prompts): rms x max_sigmas_quantile(population, CONFIDENCE) x tail factor <= TOLERANCE.
CALIBRATION_POPULATION = 100_000 * 264      # BASELINE config 4: a 100 000-tile slide against the 264 distinct prompt strings of the RCC bank
TOLERANCE = 1e-4
CONFIDENCE = 0.99
# The probe's rms is itself an estimate: 256 tiles x 64 prompts are 16 384 cosines, >= 4 096 effective samples once the correlation of one tile's
# cosines is allowed for, i.e. a relative standard error <= 1.1 %.  The rule holds the tolerance against rms x this factor (two standard errors).
PROBE_RMS_MARGIN = 1.02
# Milliseconds a knob adds to a 256-tile encode step on an MI355X (two lanes; tools/precision_budget.py measures them, profiles/r05_precision_budget.md):
# what the greedy of budget="measured" divides a knob's variance share by.  Only the RATIOS matter.
KNOB_COST_MS = {"attn_split": 0.92, "attn_split_compqkv": 0.56, "attn_compqkv": 0.22, "attn_proj_cls": 0.012, "attn_compqkv_proj_cls": 0.18, "mlp_comp": 0.52, "mlp_comp_w": 0.29, "mlp_cls": 0.07}
# Share of a site's rounding variance that survives a treatment when it is not measured on the loaded weights (same tool, bench weights): both
# MX-fp4 correction terms remove ~96 % of an MLP's share, the W_lo term alone 40-55 %; a compensated qkv inside a split attention side leaves 1-2 %
MLP_RESIDUAL = {_lib.MLP_PLAIN: 1.0, _lib.MLP_CLS: 0.1, _lib.MLP_COMP_W: 0.55, _lib.MLP_COMP: 0.04, _lib.MLP_SPLIT: 0.0}
ATTN_RESIDUAL = {_lib.ATTN_PLAIN: 1.0, _lib.ATTN_COMPQKV: 0.6, _lib.ATTN_PROJ_CLS: 0.55, _lib.ATTN_COMPQKV_PROJ_CLS: 0.25, _lib.ATTN_SPLIT_COMPQKV: 0.015, _lib.ATTN_SPLIT: 0.0}
# The treatments the greedy of budget="measured" may use.  Measured on the bench weights (profiles/r05_precision_budget.md): the W_lo-only MLP form
# removes ~45 % of a block's MLP share for 57 % of the cost of both terms, and a compensated qkv alone ~35 % of an attention side's share at 1 ms per
# percent of variance against 0.45 for MLP blocks -- neither ever wins a greedy step, so they are off by default (``knobs=`` switches them on).
# KEEP_MLP_CLS (every row plain, the CLS row of every tile again as split products) is the cheap one: the feature is pooled from the CLS rows, whose
# own rounding errors reach it directly while the other 196 rows' only arrive through attention averages -- what it leaves of a block's MLP share is
# measured per block (0.5-2 % on the bench weights).
# KEEP_ATTN_PROJ_CLS (round 6) is the attention side's counterpart: on spatially correlated tiles ~70 % of an attention side's rounding error is its proj
# GEMM's (tools/attn_site_study.py), and redoing the CLS row's proj as a split product on its fp32-grade attention output removes what a full CLS-row
# treatment of the attention side would -- for one more small GEMM in the CLS-row chain (measured per block and tile group, like KEEP_MLP_CLS).
DEFAULT_KNOBS = {"attn": (_lib.ATTN_PROJ_CLS, _lib.ATTN_COMPQKV_PROJ_CLS, _lib.ATTN_SPLIT_COMPQKV, _lib.ATTN_SPLIT), "mlp": (_lib.MLP_CLS, _lib.MLP_COMP)}

Plan = List[Tuple[int, int]]
Members = List[Tuple[str, torch.Tensor]]      # [(group name, indices of the group's tiles in the probe)]


def prefix_plan(depth: int, full_blocks: int, mlp_blocks: int) -> Plan:
    """The plan the (comp_full_blocks, comp_mlp_blocks) shorthand stands for."""
    return [(_lib.ATTN_SPLIT if i < full_blocks else _lib.ATTN_PLAIN, _lib.MLP_COMP if i < mlp_blocks else _lib.MLP_PLAIN) for i in range(depth)]


def plan_string(plan: Plan) -> str:
    """'attn:1000... mlp:2222...' -- one digit per block (KEEP_ATTN_* / KEEP_MLP_*)."""
    return "attn:" + "".join(str(a) for a, _ in plan) + " mlp:" + "".join(str(m) for _, m in plan)


def plan_prefix(plan: Plan) -> Optional[Tuple[int, int]]:
    """(comp_full_blocks, comp_mlp_blocks) if the plan is one of the prefix family, else None."""
    full = sum(1 for a, _ in plan if a == _lib.ATTN_SPLIT)
    mlp = sum(1 for _, m in plan if m == _lib.MLP_COMP)
    return (full, mlp) if plan == prefix_plan(len(plan), full, mlp) else None


def max_sigmas_gumbel(n: float) -> Tuple[float, float]:
    """(a, b) of the extreme-value (Gumbel) law of M = max_i |x_i| / sigma over n independent N(0, sigma) samples (2n one-sided samples):
    P(M <= z) ~ exp(-exp(-a (z - b))).  b is the LOCATION (the mode; M exceeds it 63 % of the time), the mean is b + 0.5772 / a."""
    n2 = 2.0 * max(float(n), 2.0)
    a = math.sqrt(2.0 * math.log(n2))
    return a, a - (math.log(math.log(n2)) + math.log(4.0 * math.pi)) / (2.0 * a)


def expected_max_sigmas(n: float) -> float:
    """LOCATION b_n of the maximum of n |N(0, sigma)| samples in units of sigma -- the value the worst of n cosine errors exceeds about 63 % of
    the time (NOT its mean, which is 0.58 / a_n higher, and not a bound): 16 384 -> 4.03, 262 144 -> 4.63, 6.4e6 -> 5.26, 2.6e7 -> 5.51.
    Measured max / rms sits 1-5 % below it at every size (bench.py configs.c4).  A tolerance has to be held against a QUANTILE of the maximum:
    ``max_sigmas_quantile``."""
    return max_sigmas_gumbel(n)[1]


def max_sigmas_quantile(n: float, q: float = CONFIDENCE) -> float:
    """z with P(max_i |x_i| <= z sigma) = q over n independent N(0, sigma) samples, exactly: erfc(z / sqrt 2) = 1 - q^(1/n).  q = 0.99:
    2.64e7 -> 6.26 (the location of the maximum is 5.51), 262 144 -> 5.50, 16 384 -> 4.99; the extreme-value asymptote b_n - ln(-ln q) / a_n is
    0.02-0.05 higher.  Cosine errors of one tile against different prompts are positively correlated (one error vector, projected on the
    prompts), which only lowers the maximum: treating them as independent is the conservative side."""
    n = max(float(n), 1.0)
    q = min(max(q, 1e-300), 1.0 - 1e-15)
    p = -math.expm1(math.log(q) / n)          # 1 - q^(1/n), accurate for tiny values
    lo, hi = 0.0, 40.0
    for _ in range(200):                      # erfc is monotone: bisection to the last bit
        mid = 0.5 * (lo + hi)
        if math.erfc(mid / math.sqrt(2.0)) > p:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def exceedance_probability(rms: float, n: float, tolerance: float = TOLERANCE) -> float:
    """P(at least one of n independent N(0, rms) cosine errors exceeds ``tolerance``) = 1 - (1 - erfc(tolerance / (rms sqrt 2)))^n."""
    if not rms > 0.0:
        return 0.0
    tail = math.erfc(tolerance / (rms * math.sqrt(2.0)))
    if tail >= 1.0:
        return 1.0
    return float(-math.expm1(max(float(n), 1.0) * math.log1p(-tail)))


def mixture_exceedance(sigmas: Sequence[float], n: float, x: float) -> float:
    """P(at least one of n independent zero-mean Gaussian errors exceeds x in magnitude) when the errors' standard deviations are spread like
    ``sigmas`` (each value standing for n / len(sigmas) samples): 1 - prod_i (1 - erfc(x / (sigma_i sqrt 2)))^(n / len).  Tiles are not equally hard
    (a tile with more texture carries a larger error vector): the worst of a population is set by its hardest tiles, not by the rms over all."""
    sig = [s for s in sigmas if s > 0.0]
    if not sig:
        return 0.0
    w = max(float(n), 1.0) / len(sigmas)
    acc = 0.0
    for s in sig:
        tail = math.erfc(x / (s * math.sqrt(2.0)))
        if tail >= 1.0:
            return 1.0
        acc += w * math.log1p(-tail)
    return float(-math.expm1(acc))


def mixture_max_quantile(sigmas: Sequence[float], n: float, q: float = CONFIDENCE) -> float:
    """x with P(max of the n errors <= x) = q under the mixture of ``mixture_exceedance`` (bisection); for equal sigmas this is
    sigma x max_sigmas_quantile(n, q)."""
    top = max(sigmas) if len(sigmas) else 0.0
    if not top > 0.0:
        return 0.0
    lo, hi = 0.0, 40.0 * top
    for _ in range(100):
        mid = 0.5 * (lo + hi)
        if mixture_exceedance(sigmas, n, mid) > 1.0 - q:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


# ------------------------------------------------------------------ the probe
def default_probe(name: str, n_tiles: int, device, seed: int):
    """(tiles, groups, group_names) of the probe ``calibrate`` / ``calibrate_bias`` use when the caller passes no tiles: "gaussian" = N(0,1) pixels,
    one group; "mixture" = ``keep_amd.synth.calibration_probe``, N(0,1) pixels and the structured families in equal parts, one group each."""
    if name == "gaussian":
        g = torch.Generator(device=device).manual_seed(seed)
        return torch.randn(n_tiles, 3, 224, 224, device=device, generator=g, dtype=torch.float32).to(torch.bfloat16), None, ("gaussian",)
    if name == "mixture":
        from .synth import PROBE_FAMILIES, calibration_probe
        return calibration_probe(max(n_tiles // len(PROBE_FAMILIES), 1), device, seed=seed)
    raise ValueError("probe must be 'mixture' or 'gaussian'")


def probe_members(groups, group_names: Optional[Sequence[str]], n_tiles: int, device) -> Members:
    """[(name, indices of the group's tiles on ``device``)] of the non-empty groups; ``groups`` = one group index per probe tile (None: one group)."""
    if groups is None:
        groups = torch.zeros(n_tiles, dtype=torch.int64)
    groups = torch.as_tensor(groups, dtype=torch.int64).cpu()
    if groups.numel() != n_tiles or (n_tiles and int(groups.min()) < 0):
        raise ValueError("groups: one non-negative group index per probe tile")
    n_groups = int(groups.max()) + 1 if n_tiles else 1
    names = tuple(group_names) if group_names is not None else tuple(f"group{i}" for i in range(n_groups))
    if len(names) < n_groups:
        raise ValueError("group_names: one name per group index")
    members = [(names[gi], torch.nonzero(groups == gi).flatten().to(device)) for gi in range(n_groups)]
    return [(name, idx) for name, idx in members if idx.numel() > 0]


def share_probe(members: Members) -> Tuple[torch.Tensor, Members]:
    """The part of the probe the variance shares are measured on -- they only rank the knobs: a sixteenth of every group, at least 16 tiles.
    -> (indices into the probe, the groups' members within that selection)."""
    heads = [idx[:max(16, int(idx.numel()) // 16)] for _, idx in members]
    sub, at = [], 0
    for (name, _), head in zip(members, heads):
        sub.append((name, torch.arange(at, at + int(head.numel()), device=head.device)))
        at += int(head.numel())
    return torch.cat(heads), sub


# ------------------------------------------------------------------ the rule on one encode of the probe
class GroupStats(NamedTuple):
    """One tile group of the probe under one plan."""
    name: str
    tiles: int
    max_abs: float              # largest |cosine error| against the probe's prompt bank
    rms_bank: float             # rms cosine error against the bank
    rms_iso: float              # isotropic rms: |feature error| / sqrt(D)
    margin: float               # two standard errors of the group's mean squared error, at least PROBE_RMS_MARGIN
    rms: float = 0.0            # rms_iso x the plan's anisotropy factor
    tail: float = 1.0           # > 1 when the group's maximum is larger than its per-tile mixture allows the probe
    sigmas: Sequence[float] = ()        # per tile: isotropic error x anisotropy x margin x tail
    effective_rms: float = 0.0  # the homoscedastic rms that predicts the same population maximum as ``sigmas``


class ProbeStats(NamedTuple):
    """What one encode of the probe under a plan predicts for the population."""
    groups: List[GroupStats]
    governing: GroupStats       # the group with the largest prediction: the plan is held to it
    anisotropy: float           # median over the groups of bank rms / isotropic rms, at least 1
    max_abs: float              # largest |cosine error| of the whole probe
    predicted: float            # predicted worst |cosine error| over the population at the confidence (NaN: a group with non-finite errors)
    per_group: dict             # the report: rounded figures by group name, plus "anisotropy_factor"


def probe_statistics(f: torch.Tensor, ref_f: torch.Tensor, sim: torch.Tensor, ref_sim: torch.Tensor, members: Members, population: float,
                     confidence: float, tolerance: float) -> ProbeStats:
    """The rule of ``KEEPModel.calibrate`` on one encode of the probe: ``f`` [n,D] features under the plan, ``ref_f`` the split-product ones, ``sim`` /
    ``ref_sim`` [n,P] their cosines against the prompt bank.  Per group: max, isotropic and bank rms, margin, tail -> the governing group's figures."""
    z_pop = max_sigmas_quantile(population, confidence)
    d2 = (sim - ref_sim).pow_(2)                                      # [n, P] squared cosine errors
    e2 = (f - ref_f).pow(2).sum(dim=1).div_(f.shape[1])               # [n] isotropic squared error per tile
    rows = []
    for name, idx in members:
        dg, eg = d2[idx], e2[idx]
        nt = int(idx.numel())
        ms_iso = float(eg.mean())
        # relative standard error of the group's mean squared error from its tile-to-tile spread (one tile's cosines share ONE error vector:
        # the tile is the sample); the rule holds the plan to two of them, at least PROBE_RMS_MARGIN
        se = float(eg.std()) / math.sqrt(nt) / ms_iso if nt > 1 and ms_iso > 0 else 0.0
        rows.append(GroupStats(name, nt, max_abs=float(dg.max().sqrt()), rms_bank=math.sqrt(float(dg.mean())), rms_iso=math.sqrt(ms_iso),
                               margin=max(PROBE_RMS_MARGIN, math.sqrt(1.0 + 2.0 * se))))
    # error vectors are not isotropic: against a bank of real prompts the rms can sit 5-10 % above (or below) the isotropic figure.  ONE
    # factor for the plan, the MEDIAN over the groups of bank rms / isotropic rms, at least 1: a group of near-identical tiles (glass) has
    # near-identical error vectors, and against a bank of similar prompts its bank rms is a single random draw, not an rms
    ratios = sorted(r.rms_bank / r.rms_iso for r in rows if r.rms_iso > 0)
    aniso = max(1.0, 0.5 * (ratios[(len(ratios) - 1) // 2] + ratios[len(ratios) // 2])) if ratios else 1.0
    groups, per_group, worst = [], {}, None
    for r, (_, idx) in zip(rows, members):
        tile_rms = e2[idx].double().sqrt()
        # heavier tails than the model assumes show as a probe maximum above what the SAME per-tile mixture allows a sample of the probe's
        # size at 99 %: then every sigma is stretched by the ratio (measured against the isotropic per-tile figures, not against the
        # group's bank rms -- for a group of near-identical tiles that is a single random draw)
        allowed = mixture_max_quantile((tile_rms * aniso).tolist(), r.tiles * sim.shape[1], 0.99)
        tail = max(1.0, r.max_abs / allowed) if allowed > 0 else 1.0
        # the group's tiles are not equally hard: the population maximum is predicted from the per-tile spread (mixture_max_quantile),
        # every tile's isotropic error standing for population / nt cosines; `eff` = the homoscedastic rms that predicts the same maximum.
        # (A group with a non-finite error predicts NaN, which no tolerance accepts: the mixture would leave a NaN sigma out of the count.)
        sig = (tile_rms * (aniso * r.margin * tail)).tolist()
        eff = mixture_max_quantile(sig, population, confidence) / z_pop if math.isfinite(r.max_abs) and math.isfinite(r.rms_iso) else math.nan
        g = r._replace(rms=r.rms_iso * aniso, tail=tail, sigmas=sig, effective_rms=eff)
        groups.append(g)
        per_group[g.name] = {"max_abs_dcos": _r3(g.max_abs), "rms_dcos_vs_bank": _r3(g.rms_bank), "rms_dcos_isotropic": _r3(g.rms_iso),
                             "margin": round(g.margin, 4), "tail_factor": round(tail, 3), "effective_rms": _r3(eff),
                             "hardest_tile_over_rms": round(max(sig) / (g.rms * g.margin * tail), 3) if g.rms > 0 else 0.0, "tiles": g.tiles,
                             "exceedance_probability": _r3(mixture_exceedance(sig, population, tolerance))}
        if worst is None or eff > worst.effective_rms or (math.isnan(eff) and not math.isnan(worst.effective_rms)):
            worst = g
    per_group["anisotropy_factor"] = round(aniso, 4)
    return ProbeStats(groups, worst, aniso, max(g.max_abs for g in groups), worst.effective_rms * z_pop, per_group)


def _r3(v: float) -> float:
    return float(f"{v:.3e}")


def _r4(v: float) -> float:
    return float(f"{v:.4f}")


# ------------------------------------------------------------------ budget="measured": variance shares and the greedy walk
def measure_shares(iso_var: Callable[[Plan], List[float]], depth: int, members: Members) -> dict:
    """Cosine-error variance each block's attention side / MLP contributes when it alone runs single fp16 passes and everything else split
    products (so the figure is that site's own rounding error, not the re-drawn rounding of everything downstream), plus what is left of a
    site's share under the cheaper treatments -- per tile group (``members``: [(name, indices into the share probe)]).  ``iso_var(plan)`` encodes
    the share probe under ``plan`` and returns the isotropic variance per group -- |feature error|^2 / D, the mean squared cosine error over
    random prompt directions -- which ranks the knobs independently of any prompt bank.  One encode per call: the sweep below IS the cost of
    the measurement.  Top-level ``attn`` / ``mlp`` / ``floor`` / ``residual_*`` hold the worst group's value per entry; ``by_group`` everything."""
    split = [(_lib.ATTN_SPLIT, _lib.MLP_SPLIT)] * depth
    G = len(members)

    def var_of(i, mode):
        return iso_var(split[:i] + [mode] + split[i + 1:])

    def minus_floor(v):
        return [max(v[g] - floor[g], 0.0) for g in range(G)]

    def ratio(v, base):
        return [min(v[g] / base[g], 1.0) if base[g] > 0 else 0.0 for g in range(G)]

    floor = iso_var(split)
    attn = [minus_floor(var_of(i, (_lib.ATTN_PLAIN, _lib.MLP_SPLIT))) for i in range(depth)]          # [depth][G]
    mlp = [minus_floor(var_of(i, (_lib.ATTN_SPLIT, _lib.MLP_PLAIN))) for i in range(depth)]
    res_m = {k: [v] * G for k, v in MLP_RESIDUAL.items()}
    res_a = {k: [v] * G for k, v in ATTN_RESIDUAL.items()}
    # what the CLS-rows-only treatment leaves differs from block to block (most in the first, where every row's error is amplified by all the
    # attention layers that follow) and from group to group (on correlated tiles the other rows carry the SAME error): measured for every block
    cls_left = [ratio(minus_floor(var_of(i, (_lib.ATTN_SPLIT, _lib.MLP_CLS))), mlp[i]) for i in range(depth)]
    for mode in (_lib.MLP_COMP, _lib.MLP_COMP_W):
        fr = [ratio(minus_floor(var_of(i, (_lib.ATTN_SPLIT, mode))), mlp[i]) for i in sorted({0, depth // 2})]
        res_m[mode] = [sum(f[g] for f in fr) / len(fr) for g in range(G)]
    for mode in (_lib.ATTN_SPLIT_COMPQKV, _lib.ATTN_COMPQKV, _lib.ATTN_COMPQKV_PROJ_CLS):
        fr = [ratio(minus_floor(var_of(i, (mode, _lib.MLP_SPLIT))), attn[i]) for i in sorted({0, min(1, depth - 1), depth // 2})]
        res_a[mode] = [max(f[g] for f in fr) for g in range(G)]
    # ... and so does what the CLS-row proj leaves of an attention side (nearly all of it in block 0 of N(0,1) tiles, under half on correlated tiles)
    pcls_left = [ratio(minus_floor(var_of(i, (_lib.ATTN_PROJ_CLS, _lib.MLP_SPLIT))), attn[i]) for i in range(depth)]
    by_group = {}
    for g, (name, idx) in enumerate(members):
        rm = {int(k): _r4(v[g]) for k, v in res_m.items()}
        rm[int(_lib.MLP_CLS)] = [_r4(cls_left[i][g]) for i in range(depth)]
        ra = {int(k): _r4(v[g]) for k, v in res_a.items()}
        ra[int(_lib.ATTN_PROJ_CLS)] = [_r4(pcls_left[i][g]) for i in range(depth)]
        by_group[name] = {"attn": [_r3(attn[i][g]) for i in range(depth)], "mlp": [_r3(mlp[i][g]) for i in range(depth)], "floor": _r3(floor[g]),
                          "residual_mlp": rm, "residual_attn": ra, "probe_tiles": int(idx.numel())}
    worst_m = {int(k): _r4(max(v)) for k, v in res_m.items()}
    worst_m[int(_lib.MLP_CLS)] = [_r4(max(cls_left[i])) for i in range(depth)]
    worst_a = {int(k): _r4(max(v)) for k, v in res_a.items()}
    worst_a[int(_lib.ATTN_PROJ_CLS)] = [_r4(max(pcls_left[i])) for i in range(depth)]
    return {"attn": [_r3(max(attn[i])) for i in range(depth)], "mlp": [_r3(max(mlp[i])) for i in range(depth)], "floor": _r3(max(floor)),
            "residual_mlp": worst_m, "residual_attn": worst_a, "probe_tiles": sum(int(idx.numel()) for _, idx in members),
            "groups": [name for name, _ in members], "by_group": by_group}


def knob_costs() -> Tuple[dict, dict]:
    """(price of every attention-side mode, price of every MLP mode) in the milliseconds of ``KNOB_COST_MS``."""
    cost_a = {_lib.ATTN_PLAIN: 0.0, _lib.ATTN_PROJ_CLS: KNOB_COST_MS["attn_proj_cls"], _lib.ATTN_COMPQKV: KNOB_COST_MS["attn_compqkv"],
              _lib.ATTN_COMPQKV_PROJ_CLS: KNOB_COST_MS["attn_compqkv_proj_cls"],
              _lib.ATTN_SPLIT_COMPQKV: KNOB_COST_MS["attn_split_compqkv"], _lib.ATTN_SPLIT: KNOB_COST_MS["attn_split"]}
    cost_m = {_lib.MLP_PLAIN: 0.0, _lib.MLP_CLS: KNOB_COST_MS["mlp_cls"], _lib.MLP_COMP_W: KNOB_COST_MS["mlp_comp_w"], _lib.MLP_COMP: KNOB_COST_MS["mlp_comp"],
              _lib.MLP_SPLIT: 3.0 * KNOB_COST_MS["mlp_comp"]}
    return cost_a, cost_m


def greedy_walk(shares: dict, depth: int, knobs: Mapping) -> List[Tuple[Plan, float]]:
    """[(plan, predicted cosine-error variance of the WORST tile group)] from the all-plain plan upwards: every step takes the ONE upgrade (a
    block's attention side or MLP to one of the allowed treatments) that lowers the worst group's predicted variance most per millisecond
    (KNOB_COST_MS); when no upgrade moves the worst group any more, the one with the largest summed reduction.  The last entry has every site
    at its best allowed treatment.  ``shares`` without ``by_group`` (one group) are read from the top level."""
    groups = list(shares["by_group"].values()) if shares.get("by_group") else [shares]
    G = len(groups)
    res_a = [{int(k): v for k, v in g["residual_attn"].items()} for g in groups]
    res_m = [{int(k): v for k, v in g["residual_mlp"].items()} for g in groups]
    left_m = lambda g, i, mode: (res_m[g][mode][i] if isinstance(res_m[g][mode], (list, tuple)) else res_m[g][mode])
    left_a = lambda g, i, mode: (res_a[g][mode][i] if isinstance(res_a[g][mode], (list, tuple)) else res_a[g][mode])
    cost_a, cost_m = knob_costs()
    am, mm = [_lib.ATTN_PLAIN] * depth, [_lib.MLP_PLAIN] * depth

    def predicted():
        return [groups[g]["floor"] + sum(groups[g]["attn"][i] * left_a(g, i, am[i]) + groups[g]["mlp"][i] * left_m(g, i, mm[i]) for i in range(depth))
                for g in range(G)]

    cur = predicted()
    walk = [(list(zip(am, mm)), max(cur))]
    while True:
        best, gain, best_sum, gain_sum = None, 0.0, None, 0.0
        top = max(cur)
        for i in range(depth):
            cands = [(am, a, cost_a[a] - cost_a[am[i]], [groups[g]["attn"][i] * (left_a(g, i, am[i]) - left_a(g, i, a)) for g in range(G)]) for a in knobs.get("attn", ())
                     if a in res_a[0]]
            cands += [(mm, m, cost_m[m] - cost_m[mm[i]], [groups[g]["mlp"][i] * (left_m(g, i, mm[i]) - left_m(g, i, m)) for g in range(G)]) for m in knobs.get("mlp", ())]
            for target, mode, dc, dv in cands:
                if dc <= 0:
                    continue
                drop = top - max(cur[g] - dv[g] for g in range(G))
                if drop > 0 and drop / dc > gain:
                    best, gain = (target, i, mode), drop / dc
                if sum(dv) > 0 and sum(dv) / dc > gain_sum:
                    best_sum, gain_sum = (target, i, mode), sum(dv) / dc
        best = best or best_sum
        if best is None:
            break
        best[0][best[1]] = best[2]
        cur = predicted()
        walk.append((list(zip(am, mm)), max(cur)))
    return walk


# ------------------------------------------------------------------ the search
def ladder_candidates(depth: int) -> List[Plan]:
    """budget="ladder": the prefix plans of COMP_LADDER from the cheapest rung up, clipped to ``depth`` (rungs that clip to the same plan once)."""
    return [prefix_plan(depth, full, mlp) for full, mlp in dict.fromkeys((min(a, depth), min(b, depth)) for a, b in COMP_LADDER)]


def walk_candidates(walk: Sequence[Tuple[Plan, float]], rms_target: float) -> List[Plan]:
    """budget="measured": the plans of a ``greedy_walk`` that are worth verifying.  The sum of measured shares over-predicts the rms of a plan by
    3-11 % (variances of neighbouring sites do not quite add): start the verification a little before the predicted crossing."""
    start = next((i for i, (_, v) in enumerate(walk) if v <= (1.06 * rms_target) ** 2), len(walk) - 1)
    return [plan for plan, _ in walk[start:]]


def search(candidates: Iterable[Plan], verify: Callable[[Plan], ProbeStats], tolerance: float):
    """-> (the first candidate whose verified prediction is inside ``tolerance``, its ProbeStats, the ``tried`` records); (None, None, tried) if
    none is.  Candidates are verified in order, ONE at a time, until a plan passes.  (Not by bisection: along a greedy walk the prediction is not
    monotone -- the anisotropy factor moves between 1.0 and 2.0 once the isotropic error is small -- and a bisection that lands in that region
    keeps a plan several times dearer than the first one that verifies: round 6 saw 47.8 instead of 35.4 ms per step.)"""
    tried = []
    for plan in candidates:
        s = verify(plan)
        gov, pre = s.governing, plan_prefix(plan)
        tried.append({"comp_full_blocks": pre[0] if pre else None, "comp_mlp_blocks": pre[1] if pre else None, "plan": plan_string(plan),
                      "max_abs_dcos": _r3(s.max_abs), "rms_dcos": _r3(gov.rms), "rms_dcos_vs_bank": _r3(gov.rms_bank),
                      "rms_dcos_isotropic": _r3(gov.rms_iso), "governing_group": gov.name, "predicted_max_abs_dcos": _r3(s.predicted),
                      "isotropic_rms_by_group": {k: v["rms_dcos_isotropic"] for k, v in s.per_group.items() if isinstance(v, dict)},
                      "anisotropy_factor": s.per_group["anisotropy_factor"]})
        if s.predicted <= tolerance:                 # (NaN compares False: falls through to the next candidate)
            return plan, s, tried
    return None, None, tried


# ------------------------------------------------------------------ what calibrate() leaves behind
def label_margin_unit(sig: Sequence[float], population: float, label_population: Optional[float], confidence: float) -> Tuple[float, float]:
    """keep_classify looks a second time at tiles whose top-2 cosine margin could hide a flipped label.  A margin is the difference of two
    cosines of ONE tile, i.e. its error vector projected on t1 - t2: standard deviation |t1 - t2| x rms, and there is ONE margin per tile:
    the quantile is taken over the tiles of the population (``label_population``; default: the 100 000 tiles of the default population, the
    whole population for a caller's own), at the same confidence.  -> (the margin per unit of |t1 - t2|, the number of margins).  |t1 - t2| <= 2
    in general; the engine's default is sqrt 2 (prompts with a non-negative cosine -- every pair of the banks this repository has seen);
    ``classify`` scales the unit by the caller's own bank."""
    n_margins = float(label_population) if label_population else (100_000.0 if population == float(CALIBRATION_POPULATION) else population)
    return mixture_max_quantile(sig, n_margins, confidence), n_margins


def calibration_report(*, chosen: Optional[Plan], stats: Optional[ProbeStats], tried: List[dict], shares: Optional[dict], budget: str, population: float,
                       confidence: float, tolerance: float, strict_blocks: int, probe_tiles: int, prompts: int, probe_name: str,
                       group_names: Sequence[str], bias_correction: bool, label_unit: float = 0.0, label_population: float = 0.0) -> dict:
    """The record ``KEEPModel.calibration`` holds (``chosen`` None: nothing qualified and the engine runs 'strict')."""
    z_pop = max_sigmas_quantile(population, confidence)
    pre = plan_prefix(chosen) if chosen else None
    report = {"precision": "comp" if chosen else "strict", "comp_full_blocks": pre[0] if pre else None,
              "comp_mlp_blocks": pre[1] if pre else None, "plan": plan_string(chosen) if chosen else None, "budget": budget,
              "population": population, "confidence": confidence, "max_sigmas_quantile": round(z_pop, 3),
              "expected_max_sigmas": round(expected_max_sigmas(population), 3),
              "target_rms_dcos": _r3(tolerance / (z_pop * PROBE_RMS_MARGIN)), "strict_blocks": strict_blocks,
              "probe": f"{probe_tiles} tiles x {prompts} prompts vs the split-product arithmetic", "probe_distribution": probe_name,
              "probe_groups": list(group_names), "tried": tried, "bias_correction": bias_correction}
    if chosen:
        gov = stats.governing
        report.update({"probe_max_abs_dcos": _r3(stats.max_abs), "probe_rms_dcos": _r3(gov.rms), "tail_factor": round(gov.tail, 3),
                       "rms_margin": round(gov.margin, 4), "governing_group": gov.name, "per_group": stats.per_group,
                       "predicted_max_abs_dcos": _r3(stats.predicted),
                       "exceedance_probability": _r3(mixture_exceedance(gov.sigmas, population, tolerance)),
                       "label_margin": _r3(math.sqrt(2.0) * label_unit), "label_margin_per_unit_prompt_distance": _r3(label_unit),
                       "label_population": label_population})
    if shares is not None:
        report["variance_shares"] = shares
    return report
