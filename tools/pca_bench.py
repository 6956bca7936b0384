#!/usr/bin/env python3
"""Feature PCA, measured: N = 100 000 unit feature rows of D = 768, and one call of 2^22 rows.  Device-event
times, median of >= 20 warm runs with the min-max spread; the forms alternate inside one loop in one process, so a difference between
them is not a difference between runs:

  moments            keep_pca_moments about a centre into zeroed accumulators (the sums launch and the Gram launch), for groups = 0, 1
                     and 4; the FLOPs counted are the upper triangle's alone (N D (D + 16)), against the 157 TFLOP/s f32 matrix rate;
                     the 64-bit atomic adds counted from the launch geometry: one word per (workgroup, word of its tile pair in the
                     written triangle)
  sums alone         the same call without a Gram (pass 1 of a two-pass fit)
  torch form         what the parent commit offers on the device (the baseline, not the code under test): xc = x - x.mean(0);
                     xc.T @ xc in fp32
  pca_fit            KEEPModel.pca_fit end to end (host clock, the device synchronised), with the host eigh stated apart
  pca_transform      k = 3 and 64, against x @ W.T + b in torch
  pca_map            wsi.pca_map for 100 000 tiles at downsample 16 with a fitted PCA (project, three percentile ranks, class raster)

The chunk length is the library's (keep_pca_chunk): a library built with another KEEP_PCA_CHUNK, loaded through KEEP_HIP_LIB, gives the
times of that value.

    python tools/pca_bench.py [--reps 20] [--big 1] [--out profiles/pca_bench.txt]
"""
import argparse
import datetime
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keep_amd import KEEPModel, _lib, pca as P, wsi                        # noqa: E402

N, D = 100_000, 768
PEAK = 157.3e12
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
    return f"{med:8.3f} ms (min {lo:.3f}, max {hi:.3f})"


def atomic_words(n, d, chunk, groups):
    """Words the Gram launch adds: per workgroup the 16 x 16 tiles of its 128-column slab pair with tile row <= tile column."""
    t16 = d // 16
    per_group = 256 * t16 * (t16 + 1) // 2
    n_chunks = -(-n // chunk)
    if groups == 0:
        slabs = -(-d // 128)
        groups = 4 if n_chunks * slabs * (slabs + 1) // 2 >= 8192 else 1
    return per_group * -(-n_chunks // min(groups, n_chunks))


def moments_block(m, x, centre, reps, label):
    n, d = x.shape
    chunk = int(_lib.load().keep_pca_chunk())
    sums = P.PcaSums(d, centre, x.device)
    flops = float(n) * d * (d + 16)                                      # 2 N x (D / 16)(D / 16 + 1) / 2 tiles of 256 words

    def run(groups, gram=True):
        def fn():
            sums.zero_()
            m._pca_moments(x, sums, gram, groups)
        return fn

    def torch_form():
        xc = x - x.mean(0)
        return xc.T @ xc
    ts = event_ms([run(0), run(1), run(4), run(0, False), torch_form], reps)
    say(f"{label}: N = {n}, D = {d}, {-(-n // chunk)} chunks of {chunk}; upper-triangle FLOPs {flops / 1e9:.1f} G")
    for g, t in zip((0, 1, 4), ts[:3]):
        words = atomic_words(n, d, chunk, g)
        say(f"  moments, groups = {g}          {fmt(t)}  / torch form = {t[0] / ts[4][0]:.3f}; {flops / (t[0] * 1e-3) / 1e12:6.1f} TFLOP/s = "
            f"{100 * flops / (t[0] * 1e-3) / PEAK:4.1f} % of the f32 matrix rate; {words * 8 / 1e6:.1f} MB of atomics, "
            f"{words * 8 / (t[0] * 1e-3) / 1e9:.1f} GB/s over the call")
    say(f"  sums alone (no Gram)         {fmt(ts[3])}  = {n * d * 4 / (ts[3][0] * 1e-3) / 1e12:.2f} TB/s of feature bytes")
    say(f"  torch xc = x - mean; xc.T @ xc {fmt(ts[4])}")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--big", type=int, default=1, help="also measure one call of 2^22 rows (12.9 GB of features)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pca_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    m = KEEPModel()
    m._create(dev)                                                         # the slide kernels need no weights
    chunk = int(_lib.load().keep_pca_chunk())
    say(f"tools/pca_bench.py on {torch.cuda.get_device_name(0)}, {datetime.date.today().isoformat()}; KEEP_PCA_CHUNK = {chunk}; fp32 features; "
        f"device-event times, median of {a.reps} warm runs, the forms alternating in one process")
    say()
    x = torch.from_numpy(P.synthetic_features(N, D, seed=0)).to(dev).contiguous()
    centre = x.mean(0).cpu().numpy().astype(np.float32)
    moments_block(m, x, centre, a.reps, "a slide cohort")

    # the fit end to end, the host eigh apart
    m.pca_fit(x, 3, normalize=False)
    torch.cuda.synchronize()
    for two_pass in (True, False):
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            fit = m.pca_fit(x, 3, two_pass=two_pass, normalize=False)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        say(f"pca_fit(k = 3, two_pass = {two_pass}) end to end   {1e3 * np.median(ts):8.1f} ms (min {1e3 * min(ts):.1f}, max {1e3 * max(ts):.1f}), host clock")
    cov = np.cov(np.random.default_rng(0).standard_normal((2 * D, D)), rowvar=False)
    te = []
    for _ in range(5):
        t0 = time.perf_counter()
        P.components_from_covariance(cov, 3)
        te.append(time.perf_counter() - t0)
    say(f"  of which the host eigh of {D} x {D} in float64   {1e3 * np.median(te):8.1f} ms (min {1e3 * min(te):.1f}, max {1e3 * max(te):.1f})")
    say()

    for k in (3, 64):
        big = m.pca_fit(x, k, normalize=False)
        w = m._on_device(np.ascontiguousarray(big.components, np.float32))
        b = m._on_device(big.bias())
        ts = event_ms([lambda: m._pca_project(x, w, b, None), lambda: x @ w.T + b], a.reps)
        say(f"pca_transform, k = {k:2d}        {fmt(ts[0])}  / torch x @ W.T + b {fmt(ts[1])} = {ts[0][0] / ts[1][0]:.3f}; "
            f"{N * D * 4 / (ts[0][0] * 1e-3) / 1e12:.2f} TB/s of feature bytes")
    say()

    gw, patch, down = 400, 256, 16
    coords = torch.stack([torch.arange(N) % gw * patch, torch.arange(N) // gw * patch], dim=1).to(dev)
    shape = (-(-N // gw) * patch // down, gw * patch // down)
    ts = event_ms([lambda: wsi.pca_map(x, coords, fit, down, shape, patch_size=patch, model=m)], max(5, a.reps // 4))
    say(f"wsi.pca_map, {N} tiles on {shape[0]} x {shape[1]} pixels (downsample {down}, PCA given)   {fmt(ts[0])}")
    rast, _ = wsi.pca_map(x, coords, fit, down, shape, patch_size=patch, model=m)
    ts = event_ms([lambda: m.render_rgb_map(rast)], a.reps)
    say(f"render_rgb_map of that raster   {fmt(ts[0])}")
    say()

    if a.big:
        del rast, coords
        nb = 1 << 22
        xb = torch.empty((nb, D), dtype=torch.float32, device=dev)
        for r0 in range(0, nb, N):                                           # the cohort's rows repeated: 12.9 GB
            xb[r0:r0 + N] = x[:min(N, nb - r0)]
        moments_block(m, xb, centre, max(5, a.reps // 4), "one call of 2^22 rows")
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f_:
            f_.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
