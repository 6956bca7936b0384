"""bench.py --dump-outputs: what the timed path returned in its last step, as .npy files that two builds can be compared on."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# bench.py sets the RCCL environment when it is imported: the dump helper is exercised in a process of its own
_DUMP_LARGE = """
import sys, torch
sys.path.insert(0, {root!r})
import bench
a = torch.arange(40000, dtype=torch.float32)[:, None].expand(40000, 768).contiguous()      # 129 MB in all with b (as float32): past the cap
b = -torch.arange(2000, dtype=torch.float64)[:, None].expand(2000, 768).contiguous()
print(bench.dump_outputs(sys.argv[1], {{"a": a, "b": b}}))
"""


def test_dump_keeps_a_fixed_sample_under_the_cap(tmp_path):
    outs = []
    for run in ("x", "y"):
        r = subprocess.run([sys.executable, "-c", _DUMP_LARGE.format(root=ROOT), str(tmp_path / run)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append({n: np.load(tmp_path / run / f"{n}.npy") for n in ("a", "b", "a_rows", "b_rows")})
    x, y = outs
    assert x["a"].dtype == np.float32 and x["b"].dtype == np.float32
    assert x["a_rows"].dtype == np.float64
    assert x["a"].nbytes + x["b"].nbytes <= 64 << 20
    for n in ("a", "b"):
        rows = x[f"{n}_rows"].astype(np.int64)
        assert len(rows) == x[n].shape[0] and np.all(np.diff(rows) > 0)
        assert np.array_equal(x[n], y[n]) and np.array_equal(rows, y[f"{n}_rows"])          # the same rows on every run
        sign = 1.0 if n == "a" else -1.0
        assert np.array_equal(x[n], np.broadcast_to(sign * rows[:, None], x[n].shape))     # row i of the output is row rows[i] of the input
    assert x["a"].shape[0] > 10 * x["b"].shape[0]                                           # both keep the same share of their rows


def _bench(tmp_path, name, steps):
    out = tmp_path / name
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--batch", "64",
           "--no-cpu-baseline", "--no-breakdown", "--no-configs", "--no-sustained", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), out


@pytest.mark.gpu
def test_dump_outputs_are_the_timed_steps_features(tmp_path):
    line2, d2 = _bench(tmp_path, "two", 2)
    line3, d3 = _bench(tmp_path, "three", 3)
    assert line2["steps"] == 2 and line3["steps"] == 3
    for line in (line2, line3):
        assert line["ms_per_step"] == pytest.approx(64 * 1e3 / line["value"], rel=1e-3)
    assert sorted(os.listdir(d2)) == ["features.npy"]
    f2, f3 = np.load(d2 / "features.npy"), np.load(d3 / "features.npy")
    assert f2.dtype == np.float32 and f2.shape == (64, 768)
    assert np.allclose(np.linalg.norm(f2, axis=1), 1.0, atol=1e-5)
    # same seeded weights and tiles, any number of steps: the same features
    assert np.array_equal(f2, f3)
