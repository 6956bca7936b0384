#!/usr/bin/env python3
"""The subtype map, measured: 100 000 tiles of P = 224 (a 317 x 316 lattice, shuffled) with C = 4 class
probabilities each, rasterised at downsample 16 (lattice step 224: one tile per pixel) and at downsample 4 (step 112: four tiles per
pixel; at step 224 the four planes would hold more than the 2^30 words a class raster may).  Device-event times, median of >= 20 warm runs with the
min-max spread, around each C-ABI call:

  class accumulate   keep_heat_accumulate_classes into a zeroed [C,h,w] raster that is not zeroed again (the scatter alone)
  C x scalar         C calls of the unchanged keep_heat_accumulate on the same tiles, one per column (the columns laid out
                     contiguously beforehand, outside the timed window), into the same planes; timed in the same loop as the fused
                     call, alternating, and the two accumulators are compared afterwards
  argmax             keep_class_argmax, all three outputs: 8 C B read + 17 B written per pixel, against that floor at the 8 TB/s HBM peak
  confusion          keep_class_confusion of the label map with a shuffled copy, within a mask: 3 B read per pixel
  render             keep_class_render over an RGB thumbnail with the margin as strength: 1 + 8 + 3 B read + 3 B written per pixel

    python tools/classmap_bench.py [--reps 20] [--out profiles/classmap_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keep_amd import KEEPModel, _lib                                       # noqa: E402
from keep_amd.classmap import palette                                      # noqa: E402
from keep_amd.model import _ptr, _stream                                   # noqa: E402

HBM_PEAK = 8.0e12
P, NX, NY, C = 224, 317, 316, 4
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def event_ms(fns, reps):
    """Median, min and max over `reps` warm runs of every fn, each run between two device events, the fns alternating."""
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            ms[k].append(timed(fn))
    return [(float(np.median(m)), min(m), max(m)) for m in ms]


def fmt(t):
    med, lo, hi = t
    return f"{med:9.3f} ms (min {lo:.3f}, max {hi:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classmap_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("classmap_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    m = KEEPModel()
    m._create(dev)                                                         # the slide kernels need no weights
    lib, h, st = _lib.load(), m._handle, _stream(dev)
    g = np.random.default_rng(0)
    n = NX * NY
    values = g.random((n, C)).astype(np.float32)
    values /= values.sum(axis=1, keepdims=True)
    vd = torch.from_numpy(values).to(dev)
    cols = vd.t().contiguous()                                             # [C, n]: what C scalar calls read
    pal = torch.from_numpy(palette(C)).to(dev)
    say(f"tools/classmap_bench.py on {torch.cuda.get_device_name(0)}; {n} tiles of P = {P}, C = {C}; device-event times, median of {a.reps} warm runs")
    say()
    for d, step in ((16, 224), (4, 112)):
        xs, ys = np.meshgrid(np.arange(NX) * step, np.arange(NY) * step)
        cd = torch.from_numpy(np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.int64)[g.permutation(n)]).to(dev)
        H, W = ((NY - 1) * step + P) // d, ((NX - 1) * step + P) // d
        pairs = n * (P // d) ** 2
        fused = torch.zeros((C, H, W), dtype=torch.int64, device=dev)
        scalar = torch.zeros((C, H, W), dtype=torch.int64, device=dev)

        def run_fused():
            _lib.check(h, lib.keep_heat_accumulate_classes(h, _ptr(cd), _ptr(vd), n, C, P, d, H, W, 0, 0, _ptr(fused), st), "heat_accumulate_classes")

        def run_scalar():
            for c in range(C):
                _lib.check(h, lib.keep_heat_accumulate(h, _ptr(cd), _ptr(cols[c]), n, P, d, H, W, 0, 0, 0, _ptr(scalar[c]), st), "heat_accumulate")

        t_fused, t_scalar = event_ms([run_fused, run_scalar], a.reps)      # 23 runs of at most four tiles per pixel each: far below the cap
        equal = bool(torch.equal(fused, scalar))
        rate = 8.0 * C * pairs / (t_fused[0] * 1e-3)
        say(f"downsample {d:2d}, step {step}: raster {C} x {H} x {W} = {C * H * W / 1e6:.1f} M words, {C * pairs / 1e6:.1f} M (tile, pixel, class) adds = "
            f"{8 * C * pairs / 1e6:.0f} MB of atomic adds")
        say(f"  class accumulate (one launch)     {fmt(t_fused)}  {rate / 1e9:8.1f} GB/s of added bytes")
        say(f"  {C} x keep_heat_accumulate          {fmt(t_scalar)}")
        say(f"  fused / scalar = {t_fused[0] / t_scalar[0]:.3f}; the two accumulators are equal: {equal}")
        fused.zero_()
        run_fused()
        label = torch.empty((H, W), dtype=torch.uint8, device=dev)
        top, margin = (torch.empty((H, W), dtype=torch.int64, device=dev) for _ in range(2))
        t_arg, = event_ms([lambda: _lib.check(h, lib.keep_class_argmax(h, _ptr(fused), C, H, W, None, 0, 0, _ptr(label), _ptr(top), _ptr(margin), st),
                                              "class_argmax")], a.reps)
        other = label.flatten()[torch.randperm(H * W, device=dev)].reshape(H, W).contiguous()
        within = (torch.rand((H, W), device=dev) < 0.7).to(torch.uint8)
        counts = torch.empty(((C + 1) ** 2,), dtype=torch.int64, device=dev)
        t_conf, = event_ms([lambda: _lib.check(h, lib.keep_class_confusion(h, _ptr(label), _ptr(other), _ptr(within), H, W, C, _ptr(counts), st),
                                               "class_confusion")], a.reps)
        thumb = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev)
        out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        t_render, = event_ms([lambda: _lib.check(h, lib.keep_class_render(h, _ptr(label), H, W, C, _ptr(thumb), W * 3, 3, 0, _ptr(pal), 128, _ptr(margin),
                                                                          0, 65535, _ptr(out), st), "class_render")], a.reps)
        for name, t, bpp in (("argmax (label, top, margin)", t_arg, 8 * C + 17), ("confusion (within a mask)", t_conf, 3), ("render (thumbnail, margin)", t_render, 15)):
            floor = bpp * H * W / HBM_PEAK * 1e3
            say(f"  {name:33s} {fmt(t)}  floor {bpp} B / pixel = {floor:.4f} ms at 8 TB/s -> {100 * floor / t[0]:.1f} % of the HBM peak")
        say()
        del fused, scalar, label, top, margin, other, within, thumb, out
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
