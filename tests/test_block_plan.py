"""The image tower's per-block decision (keep_amd/csrc/block_plan.h: resolve_block) over every combination of its inputs, on the CPU.

tests/block_plan_dump.cpp prints one CSV row per case; every row is checked against the rules as include/keep_hip.h words them (written out
again here, in Python), and against the invariants that make the schedule of a block sound."""
import csv
import io
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

FP16, STRICT, COMP = 0, 1, 2                                                  # KEEP_PREC_*
A_PLAIN, A_SPLIT, A_SPLIT_COMPQKV, A_COMPQKV, A_PROJ_CLS, A_COMPQKV_PROJ_CLS = range(6)      # KEEP_ATTN_*
M_PLAIN, M_SPLIT, M_COMP, M_COMP_W, M_CLS = range(5)                          # KEEP_MLP_*
# the profile tags in the order keep_profile_read numbers them
TAGS = ["vit.im2col", "vit.patch", "vit.ln", "vit.qkv", "vit.attn", "vit.proj", "vit.fc1", "vit.fc2", "vit.head",
        "text.embed", "text.ln", "text.qkv", "text.attn", "text.out", "text.ffn1", "text.ffn2", "text.pool", "sim",
        "vit.qkv.x", "vit.attn.x", "vit.proj.x", "vit.fc1.x", "vit.fc2.x", "vit.tail"]
INPUTS = ["precision", "strict_blocks", "attn_mode", "mlp_mode", "lane_tiles", "comp_min_tiles", "vit_has_q", "cls_tail", "block", "depth",
          "xn_ready", "fp4_planes_available", "c_resid_live"]


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler (g++ or hipcc)")
    exe = str(tmp_path_factory.mktemp("block_plan") / "block_plan_dump")
    r = subprocess.run([CXX, "-std=c++17", "-O1", os.path.join(ROOT, "tests", "block_plan_dump.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = [{k: int(v) for k, v in row.items()} for row in csv.DictReader(io.StringIO(r.stdout))]
    for row in out:
        for site in ("qkv", "proj", "fc1", "fc2"):
            row[site + "_tag"] = TAGS[row[site + "_tag"]]
        row["attn_tag"] = TAGS[row["attn_tag"]]
    return out


def test_the_enumeration_is_complete(rows):
    assert len(rows) == 3 * 2 * 6 * 5 * 2 * 2 * 2 * 3 * 2 * 2 * 2
    assert len({tuple(r[k] for k in INPUTS) for r in rows}) == len(rows)
    assert {r["lane_tiles"] - r["comp_min_tiles"] for r in rows} == {-1, 0} and {r["block"] for r in rows} == {0, 1, 2} and {r["depth"] for r in rows} == {3}


def modes(r, block):
    """(attention mode, MLP mode) block `block` runs: the plan's in KEEP_PREC_COMP, all split in KEEP_PREC_STRICT and in the first strict_blocks
    blocks of any mode, all plain in KEEP_PREC_FP16."""
    if r["precision"] == STRICT or block < r["strict_blocks"]:
        return A_SPLIT, M_SPLIT
    if r["precision"] == FP16:
        return A_PLAIN, M_PLAIN
    return r["attn_mode"], r["mlp_mode"]


def attention_side_is_split(r, block):
    a, _ = modes(r, block)
    big = r["lane_tiles"] >= r["comp_min_tiles"] and r["vit_has_q"]           # "sub-batches with fewer tiles use split products instead of compensated ones"
    return a in (A_SPLIT, A_SPLIT_COMPQKV) or (a in (A_COMPQKV, A_COMPQKV_PROJ_CLS) and not big)


def expected(r):
    a, m = modes(r, r["block"])
    big = bool(r["lane_tiles"] >= r["comp_min_tiles"] and r["vit_has_q"])
    last = r["block"] == r["depth"] - 1
    e = {}
    e["any_split"] = r["precision"] != FP16 or r["strict_blocks"] > 0
    e["any_comp"] = r["precision"] == COMP and r["vit_has_q"] and (r["mlp_mode"] in (M_COMP, M_COMP_W) or r["attn_mode"] in (A_SPLIT_COMPQKV, A_COMPQKV, A_COMPQKV_PROJ_CLS))
    e["txt_split"] = r["precision"] != FP16 or r["block"] < r["strict_blocks"]
    e["cls_only"] = last and r["cls_tail"]                                   # the last block's proj / MLP on the CLS rows only
    sp = e["attn_split"] = attention_side_is_split(r, r["block"])
    # a compensated qkv: asked for, a lane the 256x256 kernel takes, fp4 planes there -- and LayerNorm-1 running in this block (oddity 2 below)
    qc = e["qkv_comp"] = a in (A_SPLIT_COMPQKV, A_COMPQKV, A_COMPQKV_PROJ_CLS) and big and r["fp4_planes_available"] and not r["xn_ready"]
    # the CLS-rows-only tail runs on the small-M kernels (split where compensated is asked for) and is itself the CLS-row half of KEEP_MLP_CLS
    if m in (M_COMP, M_COMP_W) and (not big or e["cls_only"]):
        m = M_SPLIT
    if m == M_CLS and e["cls_only"]:
        m = M_SPLIT
    e["cls_proj"] = a in (A_PROJ_CLS, A_COMPQKV_PROJ_CLS) and not sp and not e["cls_only"]
    e["cls_mlp"] = m == M_CLS
    terms = {M_COMP: 2, M_COMP_W: 1}.get(m, 0)
    tail = e["cls_only"]
    e["qkv_split"], e["qkv_comp_terms"], e["qkv_corrected_bias"] = sp and not qc, 2 if qc else 0, not sp and not qc
    e["qkv_tag"] = "vit.qkv.x" if sp or qc else "vit.qkv"
    e["attn_tag"] = "vit.attn.x" if sp else "vit.attn"
    e["proj_split"], e["proj_comp_terms"], e["proj_corrected_bias"] = sp, 0, not sp
    e["proj_tag"] = "vit.tail" if tail else "vit.proj.x" if sp else "vit.proj"
    for fc in ("fc1", "fc2"):
        e[fc + "_split"], e[fc + "_comp_terms"], e[fc + "_corrected_bias"] = m == M_SPLIT, terms, m in (M_PLAIN, M_CLS)
        e[fc + "_tag"] = "vit.tail" if tail else f"vit.{fc}.x" if m in (M_SPLIT, M_COMP, M_COMP_W) else f"vit.{fc}"
    e["ln1_lo"], e["ln1_fp4"], e["ln1_fp4_hi_only"] = sp and not qc, qc, False
    e["ln2_lo"], e["ln2_fp4"], e["ln2_fp4_hi_only"] = m == M_SPLIT, terms > 0, terms == 1
    e["ln2_to_proj"] = terms == 0                                            # the fused LayerNorm writes no fp4 planes
    e["next_ln1_to_fc2"] = not last and not e["cls_mlp"]
    e["next_ln1_lo"] = e["next_ln1_to_fc2"] and attention_side_is_split(r, r["block"] + 1)
    e["gather_before_proj"] = e["cls_proj"] and not r["c_resid_live"]
    e["gather_before_mlp"] = e["cls_mlp"] and not e["cls_proj"]
    e["scatter_after_proj"] = e["cls_proj"] and not e["cls_mlp"]
    e["scatter_after_fc2"] = e["cls_mlp"]
    e["cls_proj_fuses_ln2"] = e["cls_proj"] and e["cls_mlp"]
    e["c_resid_live_after"] = e["cls_mlp"]
    return e


def test_every_row_follows_the_rules(rows):
    outputs = [k for k in rows[0] if k not in INPUTS]
    for r in rows:
        e = expected(r)
        assert sorted(e) == sorted(outputs)
        bad = {k: (r[k], e[k]) for k in outputs if r[k] != e[k]}
        assert not bad, ({k: r[k] for k in INPUTS}, bad)


def test_the_schedule_of_a_block_is_sound(rows):
    by_input = {tuple(r[k] for k in INPUTS): r for r in rows}
    for r in rows:
        where = {k: r[k] for k in INPUTS}
        # a lo plane is written exactly when a split product reads it
        assert r["ln1_lo"] == r["qkv_split"] and r["ln2_lo"] == r["fc1_split"] == r["fc2_split"], where
        assert r["proj_split"] == r["attn_split"], where                     # (the attention kernel writes proj's lo plane)
        if r["next_ln1_to_fc2"]:        # ... by the LayerNorm-1 that fc2 runs for the next block as well: the block that then finds xn_ready
            nxt = dict(where, block=r["block"] + 1, xn_ready=1)
            for live in (0, 1):
                assert r["next_ln1_lo"] == by_input[tuple(dict(nxt, c_resid_live=live)[k] for k in INPUTS)]["qkv_split"], where
        else:
            assert not r["next_ln1_lo"], where
        # fp4 planes are written exactly when a compensated product reads them (and only by a LayerNorm kernel of its own: the fused one cannot)
        assert r["ln1_fp4"] == (r["qkv_comp_terms"] > 0) == r["qkv_comp"] and not r["ln1_fp4_hi_only"], where
        assert r["ln2_fp4"] == (r["fc1_comp_terms"] > 0) and r["ln2_fp4_hi_only"] == (r["fc1_comp_terms"] == 1) and r["fc1_comp_terms"] == r["fc2_comp_terms"], where
        assert r["proj_comp_terms"] == 0 and not (r["ln2_fp4"] and r["ln2_to_proj"]) and not (r["xn_ready"] and r["qkv_comp"]), where
        assert not r["qkv_comp"] or r["fp4_planes_available"], where
        assert not (r["ln1_lo"] and r["ln1_fp4"]) and not (r["ln2_lo"] and r["ln2_fp4"]), where
        # a site takes the corrected bias only on a plain launch (and every plain launch takes it)
        for site in ("qkv", "proj", "fc1", "fc2"):
            assert r[site + "_corrected_bias"] == (not r[site + "_split"] and r[site + "_comp_terms"] == 0), (site, where)
            assert r[site + "_tag"].endswith(".x") == (not r["cls_only"] or site == "qkv") * (not r[site + "_corrected_bias"]), (site, where)
        assert (r["proj_tag"] == r["fc1_tag"] == r["fc2_tag"] == "vit.tail") == bool(r["cls_only"]), where
        # the compact rows are gathered before every chain that reads them, unless live
        assert r["gather_before_proj"] == (r["cls_proj"] and not r["c_resid_live"]), where
        assert r["gather_before_mlp"] == (r["cls_mlp"] and not r["cls_proj"]), where
        assert not (r["cls_only"] and (r["cls_proj"] or r["cls_mlp"])) and not (r["cls_proj"] and r["attn_split"]), where
        assert r["cls_proj_fuses_ln2"] == (r["cls_proj"] and r["cls_mlp"]), where
        # they are scattered exactly once, behind the last launch that overwrote them
        assert r["scatter_after_proj"] + r["scatter_after_fc2"] == (1 if r["cls_proj"] or r["cls_mlp"] else 0), where
        assert r["scatter_after_fc2"] == r["cls_mlp"] == r["c_resid_live_after"], where
        # the next block's LayerNorm-1 is never offered while CLS rows are still to be replaced (or where there is no next block)
        assert not (r["next_ln1_to_fc2"] and (r["scatter_after_fc2"] or r["cls_only"] or r["block"] == r["depth"] - 1)), where


def test_the_two_known_oddities_are_as_they_are(rows):
    """Both are defects left for a follow-up (a fix changes features); DESIGN.md section 5 states them."""
    seen = [0, 0]
    for r in rows:
        # ADVICE.md (round 6, "proj_cls && !mlp_cls"): the plain proj is offered LayerNorm-2 although the CLS rows it normalises are replaced afterwards
        if r["cls_proj"] and not r["cls_mlp"] and not r["ln2_fp4"]:
            assert r["ln2_to_proj"] and r["scatter_after_proj"]
            seen[0] += 1
        # Not among ADVICE.md's findings: a compensated-qkv-only block on a lane large enough for it, whose LayerNorm-1 the previous fc2 already wrote, runs a
        # PLAIN qkv (corrected bias, plain tag): neither compensated (no fp4 planes from the fused LayerNorm) nor the split product a small lane gets
        planned = r["precision"] == COMP and r["block"] >= r["strict_blocks"]
        if planned and r["attn_mode"] in (A_COMPQKV, A_COMPQKV_PROJ_CLS) and r["lane_tiles"] >= r["comp_min_tiles"] and r["vit_has_q"] and r["xn_ready"]:
            assert not r["qkv_comp"] and not r["qkv_split"] and r["qkv_corrected_bias"] and r["qkv_tag"] == "vit.qkv" and not r["attn_split"]
            seen[1] += 1
    assert seen[0] > 0 and seen[1] > 0
