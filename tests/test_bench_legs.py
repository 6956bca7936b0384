"""bench.py with and without --full: a plain run sets up, times its steps and prints the headline; every other leg runs only with --full."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

FULL_ONLY_KEYS = {"sustained", "parity", "configs", "breakdown_ms_per_step_single_stream", "cpu_baseline", "exchange"}
FULL_ONLY_ROOFLINE_KEYS = {"achieved", "by_operator", "other_kernels_single_stream", "traffic", "clock", "matrix_pipe_ceiling_measured"}


def _line(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "64", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_run_prints_the_headline_and_runs_no_other_leg():
    line = _line()
    assert line["metric"] == "224x224 tiles encoded/sec (whole node)" and line["unit"] == "tiles/s" and line["higher_is_better"] is True
    assert line["dtype"] == "fp16+mxfp4" and line["steps"] == 2
    assert line["ms_per_step"] == pytest.approx(64 * 1e3 / line["value"], rel=1e-3)
    assert not FULL_ONLY_KEYS & set(line)
    roofline = line["roofline"]
    assert not FULL_ONLY_ROOFLINE_KEYS & set(roofline)
    # the figures the timed steps themselves give stay on the plain line
    assert roofline["in_timed_region_two_lane"]["launches"] > 0 and roofline["frac_end_to_end"] > 0


def test_full_run_adds_the_other_legs():
    # configs 3-5 and the CPU baseline take minutes at their stated sizes: they are left out here and run in `bench.py --full` itself
    line = _line("--full", "--no-configs", "--no-cpu-baseline", "--sustain-seconds", "1")
    assert line["sustained"]["steps"] >= 2 and line["sustained"]["value"] > 0
    assert line["breakdown_ms_per_step_single_stream"]["vit.fc2"] > 0
    roofline = line["roofline"]
    assert FULL_ONLY_ROOFLINE_KEYS <= set(roofline)
    assert roofline["launches"] > 0 and roofline["clock"]["samples"] > 0
    assert roofline["matrix_pipe_ceiling_measured"]["random_N01_fp16_operands_TFLOPs"] > 0
