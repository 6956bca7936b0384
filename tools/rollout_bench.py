#!/usr/bin/env python3
"""The attention rollout, measured.  Device-event times, median of >= 20 warm runs with the min-max spread, the
variants taking turns within one process so that a drifting clock moves all of them:

  encode_image                        256 bf16 tiles of the depth-24 synthetic checkpoint, option graphs = 0 (the path a tapped or
                                      rollout call takes): the baseline, measured in the same run
  encode_image_attention, block -1    the single-block tap of section 19
  encode_image_rollout, start 0       a step behind all 24 blocks: 1 without a product, 22 with the T x T product, 1 with the CLS row's
  encode_image_rollout, start 12      12 steps
  encode_image_rollout, start -1      the last block's CLS-row step alone (no product)

The overhead is given in ms and in per cent of the baseline; the cost of one middle block (head-mean kernel + T x T product) follows
from the difference of start 0 and start 12 over the 12 steps between them.

    python tools/rollout_bench.py [--reps 20] [--tiles 256] [--depth 24] [--out profiles/rollout_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keep_amd import KEEPModel                                             # noqa: E402
from keep_amd.config import small_shape                                    # noqa: E402
from keep_amd.synth import synth_state_dict, synth_tiles                   # noqa: E402

LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def event_ms_interleaved(fns, reps):
    """Median, min and max of each fn over `reps` warm runs, the fns taking turns; each run between two device events."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [(float(np.median(m)), min(m), max(m)) for m in ms]


def fmt(t):
    med, lo, hi = t
    return f"{med:9.3f} ms (min {lo:.3f}, max {hi:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tiles", type=int, default=256)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rollout_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    say(f"tools/rollout_bench.py on {torch.cuda.get_device_name(0)} (one box); device-event times, median of {a.reps} warm runs, the variants taking turns")
    say()
    sd = {k: v for k, v in synth_state_dict(small_shape(a.depth, 2), seed=5).items() if k.startswith("visual")}
    m = KEEPModel(towers=("image",))
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).eval()
    m.set_option("graphs", 0)
    x = synth_tiles(a.tiles, seed=3, dtype=torch.bfloat16).to(dev)
    half = a.depth // 2
    names = ["encode_image", "encode_image_attention, block -1", "encode_image_rollout, start 0", f"encode_image_rollout, start {half}",
             "encode_image_rollout, start -1"]
    times = event_ms_interleaved([lambda: m.encode_image(x), lambda: m.encode_image_attention(x, block=-1),
                                  lambda: m.encode_image_rollout(x, start_block=0), lambda: m.encode_image_rollout(x, start_block=half),
                                  lambda: m.encode_image_rollout(x, start_block=-1)], a.reps)
    base = times[0][0]
    say(f"{a.tiles} bf16 tiles, depth {a.depth}, precision comp (the handle's default plan), graphs off, residual 0.5")
    say(f"  {names[0]:36s}{fmt(times[0])}")
    for name, t in zip(names[1:], times[1:]):
        say(f"  {name:36s}{fmt(t)}  median {t[0] - base:+7.3f} ms = {100 * (t[0] - base) / base:+6.2f} % of the step")
    steps = a.depth - half
    if half > 0:
        mid = (times[2][0] - times[3][0]) / half
        say()
        say(f"one middle block's step (head-mean kernel + T x T product): (start 0 - start {half}) / {half} = {1e3 * mid:.1f} us; "
            f"all {a.depth} steps {times[2][0] - base:.3f} ms = {100 * (times[2][0] - base) / base:.1f} % of the step; the {steps} steps from block {half} "
            f"{times[3][0] - base:.3f} ms")
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
