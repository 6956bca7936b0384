#!/usr/bin/env python3
"""Heatmap percentiles and smoothing, measured.  Device-event times, median of >= 20 warm runs with the
min-max spread, around each C-ABI call, the effective shader clock sampled after each case:

  sort + rank  keep_sort_f32 and keep_rank_f32 (the values among themselves) at M = N = 4 096 (one block), 100 172 (a slide) and
               2^24 - 1 (the cap), next to the bytes a sort cannot avoid (4 B read + 4 B written per value), to the bytes the four
               passes move (per pass 4 B read by the count, 4 B read + 4 B written by the scatter) and to scipy.stats.rankdata and
               the numpy restatement on the host
  smooth       keep_heat_smooth on the rasters of section 12's table (100 172 tiles of P = 224 at step 224 and 112, downsample 16
               and 4) at the radius keep_amd.heatmap.clam_blur gives (14 and 56), next to the byte floor (8 B read + 8 B written
               per pixel, the row pass's planes of 4 + 2 B once each way) and to the number of integer multiply-adds (3 per tap
               and pixel), and the numpy restatement on the host up to --host-max-pixels

Each stage runs in a child process of its own under a time limit; a stage that fails ends the run.

    python tools/heatmap_display_bench.py [--reps 20] [--host-max-pixels 6000000] [--no-host] [--out profiles/heatmap_display_bench.txt]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
P, NX, NY = 224, 317, 316
STAGES = (("sort", 240), ("smooth", 420))      # name, time limit in seconds
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def event_ms(fn, reps):
    """Median, min and max over `reps` warm runs of fn(), each between two device events."""
    import torch
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
    import torch
    buf = torch.zeros(3, 2, dtype=torch.int64, device=m._device)
    for i in range(3):
        m.clock_probe(buf[i], 300)
    torch.cuda.synchronize()
    return int(np.median([100.0 * a / b for a, b in buf.tolist() if b]))


def engine():
    import torch
    from keep_amd import KEEPModel, _lib
    from keep_amd.model import _stream
    if not torch.cuda.is_available():
        sys.exit("heatmap_display_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    m = KEEPModel()
    m._create(dev)                                                         # these kernels need no weights
    return m, _lib.load(), m._handle, _stream(dev), dev


def stage_sort(a):
    import scipy.stats
    import torch
    from keep_amd import _lib
    from keep_amd.heatmap import percentiles_numpy
    from keep_amd.model import _ptr
    m, lib, h, st, dev = engine()
    g = np.random.default_rng(0)
    say(f"sort + rank on {torch.cuda.get_device_name(0)}; idle effective clock {clock_mhz(m)} MHz")
    for M in (4096, NX * NY, (1 << 24) - 1):
        v = g.random(M).astype(np.float32)
        v[g.random(M) < 0.01] = np.float32(0.5)                            # some ties
        vd = torch.from_numpy(v).to(dev)
        out = torch.empty(M, dtype=torch.float32, device=dev)
        n = torch.empty(1, dtype=torch.int64, device=dev)
        pct = torch.empty(M, dtype=torch.float32, device=dev)
        t_sort = event_ms(lambda: _lib.check(h, lib.keep_sort_f32(h, _ptr(vd), M, _ptr(out), _ptr(n), st), "sort_f32"), a.reps)
        t_rank = event_ms(lambda: _lib.check(h, lib.keep_rank_f32(h, _ptr(out), M, _ptr(n), _ptr(vd), M, 1, _ptr(pct), None, None, st), "rank_f32"),
                          a.reps)
        mhz = clock_mhz(m)
        floor, moved = 8.0 * M / HBM_PEAK * 1e3, (48.0 if M > 4096 else 8.0) * M / HBM_PEAK * 1e3
        say(f"M = N = {M}: effective clock {mhz} MHz")
        say(f"  sort   {fmt(t_sort)}  floor 8 B / value = {floor:.4f} ms at 8 TB/s ({100 * floor / t_sort[0]:.2f} % of the HBM peak); the bytes the passes move: "
            f"{moved:.4f} ms ({100 * moved / t_sort[0]:.2f} %)")
        floor = 8.0 * M / HBM_PEAK * 1e3
        say(f"  rank   {fmt(t_rank)}  floor 4 B read + 4 B written / query = {floor:.4f} ms ({100 * floor / t_rank[0]:.2f} %); "
            f"{2 * int(np.ceil(np.log2(M + 1)))} dependent loads per query")
        if not a.no_host:
            t0 = time.perf_counter()
            ranks = scipy.stats.rankdata(v, "average")
            t_scipy = time.perf_counter() - t0
            t0 = time.perf_counter()
            want = percentiles_numpy(v)
            t_numpy = time.perf_counter() - t0
            equal = bool(np.array_equal(pct.cpu().numpy(), want)) and bool(np.array_equal((ranks / M).astype(np.float32), want))
            both = t_sort[0] + t_rank[0]
            say(f"  host: scipy.stats.rankdata {t_scipy * 1e3:.1f} ms ({t_scipy * 1e3 / both:.0f} x sort + rank), numpy restatement {t_numpy * 1e3:.1f} ms "
                f"({t_numpy * 1e3 / both:.0f} x); device percentiles equal to both: {equal}")
        say()


def stage_smooth(a):
    import torch
    from keep_amd import _lib
    from keep_amd.heatmap import clam_blur, gaussian_taps, smooth_numpy
    from keep_amd.model import _ptr
    m, lib, h, st, dev = engine()
    g = np.random.default_rng(1)
    n = NX * NY
    say(f"smooth on {torch.cuda.get_device_name(0)}; idle effective clock {clock_mhz(m)} MHz")
    for step in (224, 112):
        xs, ys = np.meshgrid(np.arange(NX) * step, np.arange(NY) * step)
        keep = g.random(n) < 0.8                                           # a fifth of the lattice is glass
        coords = torch.from_numpy(np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.int64)[keep]).to(dev)
        values = torch.from_numpy(g.random(int(keep.sum())).astype(np.float32)).to(dev)
        for d in (16, 4):
            H, W = ((NY - 1) * step + P) // d, ((NX - 1) * step + P) // d
            sigma, radius = clam_blur(P, d)
            taps = gaussian_taps(sigma, radius)
            td = torch.from_numpy(taps).to(dev)
            raster = m.tile_raster(coords, values, P, d, (H, W))
            mask = (torch.rand((H, W), device=dev) < 0.9).to(torch.uint8)
            out = torch.empty((H, W), dtype=torch.int64, device=dev)

            def smooth(md):
                _lib.check(h, lib.keep_heat_smooth(h, _ptr(raster.acc), H, W, _ptr(md), _ptr(td), radius, _ptr(out), st), "heat_smooth")
            t_plain = event_ms(lambda: smooth(None), a.reps)
            mhz = clock_mhz(m)
            t_mask = event_ms(lambda: smooth(mask), a.reps)
            floor = 28.0 * H * W / HBM_PEAK * 1e3
            macs = 3.0 * (2 * radius + 1) * H * W
            say(f"step {step:3d}, downsample {d:2d}: raster {H} x {W} = {H * W / 1e6:.1f} M pixels, sigma {sigma:.1f}, radius {radius} ({2 * radius + 1} taps); "
                f"effective clock {mhz} MHz")
            say(f"  smooth             {fmt(t_plain)}  floor 28 B / pixel = {floor:.4f} ms at 8 TB/s ({100 * floor / t_plain[0]:.1f} % of the HBM peak); "
                f"{macs / 1e9:.1f} G multiply-adds = {macs / (t_plain[0] * 1e-3) / 1e12:.2f} T / s")
            say(f"  smooth under mask  {fmt(t_mask)}")
            if not a.no_host and H * W <= a.host_max_pixels:
                acc = raster.acc.cpu().numpy()
                t0 = time.perf_counter()
                want = smooth_numpy(acc, taps, mask.cpu().numpy())
                t_host = time.perf_counter() - t0
                say(f"  numpy restatement on the host {t_host * 1e3:.0f} ms ({t_host * 1e3 / t_mask[0]:.0f} x), device accumulator equal: "
                    f"{bool(np.array_equal(out.cpu().numpy(), want))}")
            elif not a.no_host:
                say("  numpy restatement not measured at this size (--host-max-pixels)")
            say()
            del raster, mask, out
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-max-pixels", type=int, default=6_000_000)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heatmap_display_bench.txt"))
    ap.add_argument("--stage", choices=[s for s, _ in STAGES], help="run one stage in this process (what the parent starts)")
    a = ap.parse_args()
    if a.stage:
        {"sort": stage_sort, "smooth": stage_smooth}[a.stage](a)
        return
    say(f"tools/heatmap_display_bench.py (one box); device-event times, median of {a.reps} warm runs")
    say()
    for name, limit in STAGES:
        cmd = [sys.executable, os.path.abspath(__file__), "--stage", name, "--reps", str(a.reps), "--host-max-pixels", str(a.host_max_pixels)]
        try:
            r = subprocess.run(cmd + (["--no-host"] if a.no_host else []), capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"stage {name} ran into its time limit of {limit} s: nothing further is started")
        print(r.stdout, end="", flush=True)
        LINES.extend(r.stdout.splitlines())
        if r.returncode != 0:
            sys.exit(f"stage {name} ended with status {r.returncode}: nothing further is started\n{r.stderr[-2000:]}")
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
