#!/usr/bin/env python3
"""Bootstrap resampling, measured.

  roc         keep_boot_roc between device events: N items, B replicates, scores that are all distinct (K = N: above
              KEEP_BOOT_LDS_GROUPS the counters live in global slabs) and the same scores rounded to 1/4000 (K <= 4001: the counters
              live in LDS), so the two paths stand side by side at one size; and KEEPModel.bootstrap_roc as a caller sees it (wall
              clock, its one readback included).
  confusion   keep_boot_confusion between device events at C = 2, 4, 16.
  yardstick   what a caller can do on the device without these kernels: per replicate torch.randint + KEEPModel.tile_roc(scores[idx],
              labels[idx], curve=False), and torch.bincount(truth[idx] * C + pred[idx]).  Timed over --loop replicates between device
              events (wall clock for tile_roc, which reads its scalars back) and SCALED to B: the figure printed is loop time x B / loop.

Shapes: the slide (N = 100 000, B = 1000) and the cohort (N = 1000, B = 10 000).  Device-event times are the median of --reps warm
runs with the min-max spread.  The first replicates of every measured call are compared with keep_amd.bootstrap's restatement.
The measurement runs in a child process under a time limit, so one that hangs ends alone.

    python tools/bootstrap_bench.py [--shapes 100000x1000,1000x10000] [--reps 10] [--loop 50] [--limit 900] [--out profiles/bootstrap_bench.txt]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from keep_amd import KEEPModel, _lib, bootstrap                            # noqa: E402
from keep_amd.config import small_shape                                    # noqa: E402
from keep_amd.model import _ptr, _stream                                   # noqa: E402
from keep_amd.synth import synth_state_dict                                # noqa: E402
from regions_bench import event_ms                                         # noqa: E402

LINES = []
SEED = 7


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def row(name, t, draws=None, scaled=None):
    med, lo, hi = t
    tail = f"  {draws / (med * 1e-3) / 1e9:7.2f} G draws/s" if draws else ""
    if scaled:
        tail += f"  (SCALED from {scaled[0]} replicates to {scaled[1]})"
    say(f"    {name:52s} {med:10.3f} ms (min {lo:.3f}, max {hi:.3f}){tail}")
    return med


def scale(t, f):
    return tuple(v * f for v in t)


def wall_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms)), min(ms), max(ms)


def shape(m, n, B, reps, loop):
    dev, lib, h, st = m._device, _lib.load(), m._handle, _stream(m._device)
    g = torch.Generator().manual_seed(n)
    s = (torch.randperm(n, generator=g).to(torch.float32) + 0.5) / n                     # all distinct
    y = ((s + 0.3 * torch.randn((n,), generator=g)) > 0.5).to(torch.uint8)
    sq = torch.round(s * 4000) / 4000
    say(f"N = {n}, B = {B}: {n * B / 1e6:.0f} M draws per call")
    out = torch.empty((B, 4), dtype=torch.int64, device=dev)
    ours = {}
    for name, sc in (("distinct scores (global slabs)" if n > bootstrap.LDS_GROUPS else "distinct scores (LDS)", s), ("scores on a grid of 1/4000 (LDS)", sq)):
        sd, yd = sc.to(dev), y.to(dev)
        call = lambda: _lib.check(h, lib.keep_boot_roc(h, _ptr(sd), _ptr(yd), n, SEED, 0, B, _ptr(out), st), "boot_roc")      # noqa: E731
        ours[name] = row(f"keep_boot_roc, {name}", event_ms(call, reps), n * B)
        ok = np.array_equal(out[:3].cpu().numpy(), bootstrap.boot_roc_numpy(sc.numpy(), y.numpy(), 3, SEED))
        say(f"        K = {len(torch.unique(sc))}; replicates 0..2 equal the restatement: {ok}")
    row("KEEPModel.bootstrap_roc, wall", wall_ms(lambda: m.bootstrap_roc(sd, yd, B, SEED), reps))
    say(f"        workspace {lib.keep_workspace_bytes(h) / 1e6:.0f} MB")
    sd = s.to(dev)

    def roc_loop():
        for _ in range(loop):
            idx = torch.randint(n, (n,), device=dev)
            m.tile_roc(sd[idx], yd[idx], curve=False)
    base = row("yardstick: randint + tile_roc per replicate", scale(wall_ms(roc_loop, 3), B / loop), scaled=(loop, B))
    for name, ms in ours.items():
        say(f"        one call is {base / ms:.0f} x faster than the loop ({name})")
    for C in (2, 4, 16):
        t = torch.randint(C, (n,), generator=g).to(torch.uint8)
        p = torch.where(torch.rand((n,), generator=g) < 0.7, t, torch.randint(C, (n,), generator=g).to(torch.uint8))
        td, pd = t.to(dev), p.to(dev)
        outc = torch.empty((B, C, C), dtype=torch.int64, device=dev)
        call = lambda: _lib.check(h, lib.keep_boot_confusion(h, _ptr(td), _ptr(pd), n, C, SEED, 0, B, _ptr(outc), st), "boot_confusion")   # noqa: E731
        mine = row(f"keep_boot_confusion, C = {C}", event_ms(call, reps), n * B)
        ok = np.array_equal(outc[:3].cpu().numpy(), bootstrap.boot_confusion_numpy(t.numpy(), p.numpy(), C, 3, SEED))
        code = td.to(torch.int64) * C + pd

        def conf_loop():
            for _ in range(loop):
                torch.bincount(code[torch.randint(n, (n,), device=dev)], minlength=C * C)
        base = row(f"yardstick: randint + bincount per replicate, C = {C}", scale(event_ms(conf_loop, 3), B / loop), scaled=(loop, B))
        say(f"        replicates 0..2 equal the restatement: {ok}; one call is {base / mine:.0f} x faster than the loop")
    say()


def child(a):
    dev = torch.device("cuda:0")
    shp = small_shape(2, 2)                             # the calls use the handle's arena and stream only
    m = KEEPModel(shp)
    m.load_state_dict(synth_state_dict(shp, seed=0))
    m.to(dev).eval()
    for n, B in (tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",") if s):
        shape(m, n, B, a.reps, a.loop)
    m.check_errors(wait=True)
    with open(a.out, "a") as f:
        f.write("\n".join(LINES) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100000x1000,1000x10000", help="N x B, comma separated")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--loop", type=int, default=50, help="replicates of the yardstick loop, scaled to B")
    ap.add_argument("--limit", type=int, default=900, help="seconds the measurement may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bootstrap_bench.txt"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bootstrap_bench needs the GPU: there is nothing to measure without one")
    if a.child:
        return child(a)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(f"tools/bootstrap_bench.py on {torch.cuda.get_device_name(0)} (one box); device-event times, median of {a.reps} warm runs; "
                f"LDS cap {bootstrap.LDS_GROUPS} groups\n\n")
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--shapes", a.shapes, "--reps", str(a.reps), "--loop", str(a.loop),
                             "--out", a.out], timeout=a.limit).returncode
    except subprocess.TimeoutExpired:
        rc = "time limit"
    if rc != 0:
        with open(a.out, "a") as f:
            f.write(f"the child ended with {rc}\n")
        sys.exit(f"bootstrap_bench: the child ended with {rc}")


if __name__ == "__main__":
    main()
