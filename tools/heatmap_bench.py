#!/usr/bin/env python3
"""The heatmap stage, measured: 100 000 tiles of P = 224 (a 317 x 316 lattice, shuffled), step 224 / 112 / 56
(1 / 4 / 16 tiles per pixel) rasterised at downsample 4 / 16 / 32.  Device-event times, median of >= 20 warm runs with the
min-max spread, around each C-ABI call:

  accumulate   keep_heat_accumulate into a zeroed raster that is not zeroed again (the scatter alone), and with zero_first (the
               memset included): time, atomic bytes per second (8 B x (tile, pixel) pairs) and that rate next to the 1.3 TB/s the
               chip sustains for fp32 atomic adds of one dword per lane -- a comparison with a DIFFERENT instruction (this one is a
               64-bit integer add, two dwords per lane), not a ceiling
  mean         keep_heat_mean, mean + count out: 8 B read + 8 B written per pixel, against that floor at the 8 TB/s HBM peak
  render       keep_heat_render over an RGB thumbnail with a mask: 8 + 3 + 1 B read + 3 B written per pixel, likewise

and the numpy restatement's time on the same input on the host, the only baseline that exists (its mean / render only up to
--host-max-pixels: they allocate several int64 images).  The effective shader clock is sampled after each accumulate case.

    python tools/heatmap_bench.py [--reps 20] [--host-max-pixels 32000000] [--no-host] [--out profiles/heatmap_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keep_amd import KEEPModel, _lib                                       # noqa: E402
from keep_amd.heatmap import (colormap, footprints_numpy, mean_numpy, raster_numpy, render_numpy)      # noqa: E402
from keep_amd.model import _ptr, _stream                                   # noqa: E402

HBM_PEAK = 8.0e12
FP32_ATOMIC_RATE = 1.3e12
P, NX, NY = 224, 317, 316
ENCODE_TILES_PER_S = 7150.0                   # README.md: the image encoder, one MI355X
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def event_ms(fn, reps):
    """Median, min and max over `reps` warm runs of fn(), each between two device events."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms)


def fmt(t):
    med, lo, hi = t
    return f"{med:9.3f} ms (min {lo:.3f}, max {hi:.3f})"


def clock_mhz(m):
    buf = torch.zeros(3, 2, dtype=torch.int64, device=m._device)
    for i in range(3):
        m.clock_probe(buf[i], 300)
    torch.cuda.synchronize()
    return int(np.median([100.0 * a / b for a, b in buf.tolist() if b]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-max-pixels", type=int, default=32_000_000)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heatmap_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("heatmap_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    m = KEEPModel()
    m._create(dev)                                                         # the heatmap kernels need no weights
    lib, h, st = _lib.load(), m._handle, _stream(dev)
    g = np.random.default_rng(0)
    lut = torch.from_numpy(colormap("jet")).to(dev)
    n = NX * NY
    say(f"tools/heatmap_bench.py on {torch.cuda.get_device_name(0)} (one box); {n} tiles of P = {P}; device-event times, median of {a.reps} warm runs")
    say(f"idle effective clock {clock_mhz(m)} MHz")
    say()
    worst = 0.0
    for step in (224, 112, 56):
        xs, ys = np.meshgrid(np.arange(NX) * step, np.arange(NY) * step)
        coords = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.int64)[g.permutation(n)]
        values = g.random(n).astype(np.float32)
        cd, vd = torch.from_numpy(coords).to(dev), torch.from_numpy(values).to(dev)
        for d in (4, 16, 32):
            H, W = ((NY - 1) * step + P) // d, ((NX - 1) * step + P) // d
            fp = footprints_numpy(coords, P, d, (H, W), (0, 0))
            pairs = int(((fp[:, 1] - fp[:, 0]).clip(0) * (fp[:, 3] - fp[:, 2]).clip(0)).sum())
            acc = torch.zeros((H, W), dtype=torch.int64, device=dev)

            def accumulate(zero):
                _lib.check(h, lib.keep_heat_accumulate(h, _ptr(cd), _ptr(vd), n, P, d, H, W, 0, 0, zero, _ptr(acc), st), "heat_accumulate")
            t_add = event_ms(lambda: accumulate(0), a.reps)                # at most 23 x 16 tiles per pixel: far below the cap
            mhz = clock_mhz(m)
            t_zero = event_ms(lambda: accumulate(1), a.reps)
            rate = 8.0 * pairs / (t_add[0] * 1e-3)
            say(f"step {step:3d} ({(P // step) ** 2:2d} tiles / pixel), downsample {d:2d}: raster {H} x {W} = {H * W / 1e6:.1f} M pixels, {pairs / 1e6:.1f} M (tile, pixel) "
                f"pairs = {8 * pairs / 1e6:.0f} MB of atomic adds; effective clock {mhz} MHz")
            say(f"  accumulate (scatter alone)   {fmt(t_add)}  {rate / 1e9:8.1f} GB/s of added bytes = {rate / FP32_ATOMIC_RATE:.2f} x the fp32-add rate "
                f"(1.3 TB/s, a different instruction)")
            say(f"  accumulate (zero_first)      {fmt(t_zero)}")
            mean = torch.empty((H, W), dtype=torch.float32, device=dev)
            count = torch.empty((H, W), dtype=torch.int32, device=dev)
            t_mean = event_ms(lambda: _lib.check(h, lib.keep_heat_mean(h, _ptr(acc), H, W, 0.0, _ptr(mean), _ptr(count), None, st), "heat_mean"), a.reps)
            thumb = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev)
            mask = (torch.rand((H, W), device=dev) < 0.7).to(torch.uint8)
            out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
            t_render = event_ms(lambda: _lib.check(h, lib.keep_heat_render(h, _ptr(acc), H, W, _ptr(thumb), W * 3, 3, 0, _ptr(mask), _ptr(lut), 102, 0,
                                                                            65535, 0, _ptr(out), st), "heat_render"), a.reps)
            for name, t, bpp in (("mean + count", t_mean, 16), ("render (thumbnail, mask)", t_render, 15)):
                floor = bpp * H * W / HBM_PEAK * 1e3
                say(f"  {name:28s} {fmt(t)}  floor {bpp} B / pixel = {floor:.4f} ms at 8 TB/s -> {100 * floor / t[0]:.1f} % of the HBM peak")
            stage = t_zero[0] + t_mean[0] + t_render[0]
            worst = max(worst, stage)
            say(f"  whole stage (zero + accumulate + mean + render) {stage:.3f} ms")
            if not a.no_host:
                t0 = time.perf_counter()
                want = raster_numpy(coords, values, P, d, (H, W))
                t_host = time.perf_counter() - t0
                accumulate(1)
                equal = bool(torch.equal(acc.cpu(), torch.from_numpy(want)))
                line = f"  numpy restatement on the host: accumulate {t_host * 1e3:.0f} ms ({t_host * 1e3 / t_zero[0]:.0f} x), device accumulator equal: {equal}"
                if H * W <= a.host_max_pixels:
                    t0 = time.perf_counter()
                    mean_numpy(want)
                    t_hm = time.perf_counter() - t0
                    t0 = time.perf_counter()
                    render_numpy(want, thumb.cpu().numpy(), 0.4, "jet", mask.cpu().numpy())
                    t_hr = time.perf_counter() - t0
                    line += f"; mean {t_hm * 1e3:.0f} ms, render {t_hr * 1e3:.0f} ms"
                else:
                    line += "; mean / render not measured at this size (--host-max-pixels)"
                say(line)
            say()
            del acc, mean, count, thumb, mask, out
            torch.cuda.empty_cache()
    encode_s = n / ENCODE_TILES_PER_S
    say(f"the slowest whole stage above takes {worst:.2f} ms: {100 * worst * 1e-3 / encode_s:.3f} % of encoding the same {n} tiles ({encode_s:.1f} s at "
        f"{ENCODE_TILES_PER_S:.0f} tiles/s) and {worst / (256 / ENCODE_TILES_PER_S * 1e3):.2f} x one 256-tile step ({256 / ENCODE_TILES_PER_S * 1e3:.1f} ms)")
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
