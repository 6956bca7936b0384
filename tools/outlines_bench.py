#!/usr/bin/env python3
"""Region outlines, measured.

For masks of 1024^2, 4096^2 and 8192^2 pixels -- the four of tools/regions_bench.py: the synthetic tissue mask (few large regions with
long rings), the raw saturation threshold (many small ones), all ones (one ring of four vertices) and isolated 8 x 8 blocks -- the
median of >= 20 warm runs between device events around each C-ABI call, with the min-max spread, the bytes the call has to move at
the least, the rate that implies and its share of the 8 TB/s HBM peak:

  count    keep_outline_count (4 B read per pixel)
  trace    keep_outline_trace (4 B read per pixel, 8 B written per vertex, 64 B per ring)
  draw     keep_outline_draw, width 2 (4 + 3 B read and 3 B written per pixel)

Beside them, in the same process on the same mask: keep_regions_label + keep_regions_table (the stage that made the labels), the
number of jumping rounds that did work in each of the two passes (ceil(log2(edges of the longest ring)): every later round returns at
once), and keep_amd.outline.outlines_numpy on the host up to --host-max.  Every size runs in a child process under its own time limit,
so one that hangs or runs out of memory ends alone.

    python tools/outlines_bench.py [--sizes 1024,4096,8192] [--reps 20] [--host-max 1024] [--limit 600] [--out profiles/outlines_bench.txt]
"""
import argparse
import math
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from keep_amd import KEEPModel, _lib                                       # noqa: E402
from keep_amd.components import NCOLS as TABLE_COLS                        # noqa: E402
from keep_amd.config import small_shape                                    # noqa: E402
from keep_amd.model import _ptr, _stream                                   # noqa: E402
from keep_amd.outline import NCOLS, outlines_numpy                         # noqa: E402
from keep_amd.synth import synth_state_dict                                # noqa: E402
from regions_bench import HBM_PEAK, event_ms, masks                        # noqa: E402

LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def row(name, t, floor):
    med, lo, hi = t
    rate = floor / (med * 1e-3)
    say(f"    {name:13s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})  floor {floor / 1e6:8.1f} MB -> {rate / 1e9:8.1f} GB/s = "
        f"{100 * rate / HBM_PEAK:5.2f} % of the HBM peak")


def size(m, n, reps, host):
    dev = m._device
    lib, h, st = _lib.load(), m._handle, _stream(dev)
    labels = torch.empty((n, n), dtype=torch.int32, device=dev)
    n_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    r_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    rgb = torch.full((n, n, 3), 200, dtype=torch.uint8, device=dev)
    out = torch.empty_like(rgb)
    say(f"mask {n} x {n} ({n * n / 1e6:.1f} M pixels)")
    for name, mask, conn in masks(m, n):
        def label():
            _lib.check(h, lib.keep_regions_label(h, _ptr(mask), n, n, conn, 1, _ptr(labels), _ptr(n_dev), st), "regions_label")
        label()
        k = int(n_dev.item())
        table = torch.empty((max(k, 1), TABLE_COLS), dtype=torch.int64, device=dev)

        def regions():
            label()
            _lib.check(h, lib.keep_regions_table(h, _ptr(labels), n, n, k, None, _ptr(table), st), "regions_table")

        def count():
            _lib.check(h, lib.keep_outline_count(h, _ptr(labels), n, n, k, conn, _ptr(counts), st), "outline_count")
        count()
        E, V = counts.tolist()
        verts = torch.empty((V, 2), dtype=torch.int32, device=dev)
        rings = torch.empty((V // 4, NCOLS), dtype=torch.int64, device=dev)

        def trace():
            _lib.check(h, lib.keep_outline_trace(h, _ptr(labels), n, n, k, conn, E, V, _ptr(verts), _ptr(rings), V // 4, _ptr(r_dev), st),
                       "outline_trace")
        trace()
        R = int(r_dev.item())
        longest = int(rings[:R, 3].max())
        say(f"  {name}: {k} regions, {conn}-connected, {E} edges, {V} vertices, {R} rings, the longest of {longest} edges: "
            f"{math.ceil(math.log2(longest))} rounds of work in each jumping pass (of {math.ceil(math.log2(E)) + 2} launched); workspace "
            f"{lib.keep_workspace_bytes(h) / 1e6:.0f} MB")
        t_reg = event_ms(regions, reps)
        row("(label+table)", t_reg, 9 * n * n + 8 * TABLE_COLS * k)
        t_count = event_ms(count, reps)
        row("count", t_count, 4 * n * n)
        t_trace = event_ms(trace, reps)
        row("trace", t_trace, 4 * n * n + 8 * V + 8 * NCOLS * R)
        t_draw = event_ms(lambda: _lib.check(h, lib.keep_outline_draw(h, _ptr(labels), n, n, _ptr(rgb), _ptr(out), 0, 2, st), "outline_draw"), reps)
        row("draw", t_draw, 10 * n * n)
        say(f"    (count + trace) / (label + table) = {(t_count[0] + t_trace[0]) / t_reg[0]:.2f}")
        if host:
            lab = labels.cpu().numpy()
            t0 = time.perf_counter()
            want = outlines_numpy(lab, conn, k)
            t1 = time.perf_counter()
            same = bool(np.array_equal(want[0], rings[:R].cpu().numpy())) and bool(np.array_equal(want[1], verts.cpu().numpy()))
            say(f"    outlines_numpy on the host: {1e3 * (t1 - t0):.0f} ms = {(t1 - t0) * 1e3 / (t_count[0] + t_trace[0]):.0f} x count + trace; "
                f"rings and vertices equal: {same}")
        m.check_errors(wait=True)
        del table, verts, rings
    say()


def child(n, reps, host, out):
    dev = torch.device("cuda:0")
    shape = small_shape(2, 2)                           # the outline calls use the handle's arena and stream only
    m = KEEPModel(shape)
    m.load_state_dict(synth_state_dict(shape, seed=0))
    m.to(dev).eval()
    size(m, n, reps, host)
    with open(out, "a") as f:
        f.write("\n".join(LINES) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096,8192")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-max", type=int, default=1024, help="largest side outlines_numpy is timed on")
    ap.add_argument("--limit", type=int, default=600, help="seconds every size may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outlines_bench.txt"))
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("outlines_bench needs the GPU: there is nothing to measure without one")
    if a.child:
        return child(a.child, a.reps, a.child <= a.host_max, a.out)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(f"tools/outlines_bench.py on {torch.cuda.get_device_name(0)} (one box); device-event times, median of {a.reps} warm runs\n\n")
    for n in (int(v) for v in a.sizes.split(",") if v):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), "--reps", str(a.reps), "--host-max", str(a.host_max),
                                 "--out", a.out], timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            rc = "time limit"
        if rc != 0:                                     # nothing more is started on a device that has just failed
            with open(a.out, "a") as f:
                f.write(f"mask {n} x {n}: the child ended with {rc}; stopped here\n")
            sys.exit(f"outlines_bench: size {n} ended with {rc}")


if __name__ == "__main__":
    main()
