#!/usr/bin/env python3
"""The CLS attention maps, measured.  Device-event times, median of >= 20 warm runs with the min-max spread:

  tap          KEEPModel.encode_image on 256 bf16 tiles of the depth-24 synthetic checkpoint (option graphs = 0, the path a tapped
               call takes) next to KEEPModel.encode_image_attention on the same tiles, block -1 and block 0: what the tap adds to a
               step, the probabilities' kernel and the [256, 16, 197] fp32 output included.  The two are run in alternation, so a
               drifting clock moves both.
  cell raster  keep_heat_accumulate_cells for 100 000 tiles of P = 224 with 14 x 14 cells (a 317 x 316 lattice, shuffled) at
               downsample 16 and 4, next to keep_heat_accumulate on the same tiles and raster: same (tile, pixel) pairs and the same
               8-byte atomic add per pair, plus one 4-byte value read and one division pair per pixel.

    python tools/attention_bench.py [--reps 20] [--tiles 256] [--depth 24] [--out profiles/attention_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keep_amd import KEEPModel, _lib                                       # noqa: E402
from keep_amd.config import small_shape                                    # noqa: E402
from keep_amd.heatmap import footprints_numpy                              # noqa: E402
from keep_amd.model import _ptr, _stream                                   # noqa: E402
from keep_amd.synth import synth_state_dict, synth_tiles                   # noqa: E402

P, NX, NY, GRID = 224, 317, 316, (14, 14)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attention_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    say(f"tools/attention_bench.py on {torch.cuda.get_device_name(0)} (one box); device-event times, median of {a.reps} warm runs")
    say()

    sd = {k: v for k, v in synth_state_dict(small_shape(a.depth, 2), seed=5).items() if k.startswith("visual")}
    m = KEEPModel(towers=("image",))
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).eval()
    m.set_option("graphs", 0)
    x = synth_tiles(a.tiles, seed=3, dtype=torch.bfloat16).to(dev)
    plain, last, first = event_ms_interleaved([lambda: m.encode_image(x), lambda: m.encode_image_attention(x, block=-1),
                                               lambda: m.encode_image_attention(x, block=0)], a.reps)
    say(f"tap: {a.tiles} bf16 tiles, depth {a.depth}, precision comp (the plan calibrate() chose), graphs off")
    say(f"  encode_image                       {fmt(plain)}")
    for name, t in (("block -1", last), ("block  0", first)):
        say(f"  encode_image_attention, {name}   {fmt(t)}  median {1e3 * (t[0] - plain[0]):+8.1f} us = {100 * (t[0] - plain[0]) / plain[0]:+.2f} % of the step")
    say()
    del m, x
    torch.cuda.empty_cache()

    e = KEEPModel()
    e._create(dev)                                                         # the raster kernels need no weights
    lib, h, st = _lib.load(), e._handle, _stream(dev)
    g = np.random.default_rng(0)
    n, G = NX * NY, GRID[0] * GRID[1]
    xs, ys = np.meshgrid(np.arange(NX) * P, np.arange(NY) * P)
    coords = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.int64)[g.permutation(n)]
    cd = torch.from_numpy(coords).to(dev)
    cells = torch.rand((n, G), device=dev)
    values = cells[:, 0].contiguous()
    say(f"cell raster: {n} tiles of P = {P}, {GRID[0]} x {GRID[1]} cells = {n * G / 1e6:.1f} M token cells ({4 * n * G / 1e6:.0f} MB of values)")
    for d in (16, 4):
        H, W = NY * P // d, NX * P // d
        fp = footprints_numpy(coords, P, d, (H, W), (0, 0))
        pairs = int(((fp[:, 1] - fp[:, 0]).clip(0) * (fp[:, 3] - fp[:, 2]).clip(0)).sum())
        acc = torch.zeros((H, W), dtype=torch.int64, device=dev)

        def by_cell(zero=0):
            _lib.check(h, lib.keep_heat_accumulate_cells(h, _ptr(cd), _ptr(cells), n, GRID[0], GRID[1], P, d, H, W, 0, 0, zero, _ptr(acc), st),
                       "heat_accumulate_cells")

        def by_tile(zero=0):
            _lib.check(h, lib.keep_heat_accumulate(h, _ptr(cd), _ptr(values), n, P, d, H, W, 0, 0, zero, _ptr(acc), st), "heat_accumulate")
        t_cell, t_tile = event_ms_interleaved([by_cell, by_tile], a.reps)       # 2 x (3 + reps) tiles per pixel at most: far below the cap
        say(f"  downsample {d:2d}: raster {H} x {W} = {H * W / 1e6:.1f} M pixels, {pairs / 1e6:.1f} M (tile, pixel) pairs = {8 * pairs / 1e6:.0f} MB of atomic adds")
        say(f"    keep_heat_accumulate_cells   {fmt(t_cell)}  {8.0 * pairs / (t_cell[0] * 1e-3) / 1e9:8.1f} GB/s of added bytes")
        say(f"    keep_heat_accumulate         {fmt(t_tile)}  {8.0 * pairs / (t_tile[0] * 1e-3) / 1e9:8.1f} GB/s of added bytes   (cells / tiles = {t_cell[0] / t_tile[0]:.2f} x)")
        del acc
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
