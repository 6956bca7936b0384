#!/usr/bin/env python3
"""The region table, measured.

For masks of 1024^2, 4096^2 and 8192^2 pixels -- the synthetic tissue mask (few large regions), the raw saturation threshold (many
small ones), all ones (one region: every workgroup adds into the same table row) and isolated 8 x 8 blocks -- the median of >= 20
warm runs between device events around each C-ABI call, with the min-max spread, the bytes the call has to move at the least (its
input read once, its output written once), the rate that implies and its share of the 8 TB/s HBM peak:

  label          keep_regions_label: labelling + rank + relabel (1 B read, 4 B written per pixel)
  table          keep_regions_table without a raster (4 B read per pixel, 112 B written per region)
  table+raster   keep_regions_table with an accumulator (4 + 8 B read per pixel)

Yardsticks in the same run: the foreground-labelling stage of keep_tissue_mask (tools/tissue_bench.py's "fragments" row: threshold
pass + the same labelling kernels + the drop pass) on the same mask, and the scipy composition on the host (ndimage.label +
find_objects + three sum_labels; up to --host-max).  The effective shader clock is sampled after each mask.

    python tools/regions_bench.py [--sizes 1024,4096,8192] [--reps 20] [--host-max 4096] [--out profiles/regions_bench.txt]

keep_regions_label is one call, so device events cannot part the labelling from rank + relabel inside it.  A kernel trace can:
`--calls label --masks NAME` runs that call alone on one mask, and tools/regions_kernel_split.py reads the per-kernel summaries
of such runs under `rocprofv3 --kernel-trace --stats` (its docstring has the command).
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
from keep_amd.components import NCOLS                                      # noqa: E402
from keep_amd.config import KEEPShape                                      # noqa: E402
from keep_amd.model import _ptr, _stream                                   # noqa: E402
from keep_amd.region import TissueSegmentation, saturation_numpy           # noqa: E402
from keep_amd.synth import synth_state_dict, synth_thumbnail               # noqa: E402

HBM_PEAK = 8.0e12
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


def clock_mhz(m):
    buf = torch.zeros(3, 2, dtype=torch.int64, device=m._device)
    for i in range(3):
        m.clock_probe(buf[i], 300)
    torch.cuda.synchronize()
    return int(np.median([100.0 * a / b for a, b in buf.tolist() if b]))


def masks(m, n):
    rgb = synth_thumbnail(n, n)
    p = TissueSegmentation(min_area=100 * (n // 512) ** 2, min_hole=16 * (n // 512) ** 2)
    yield "tissue mask", m.tissue_mask(rgb, 16, p).mask, 8
    yield "raw threshold", torch.from_numpy((saturation_numpy(rgb) > 8).astype(np.uint8)).to(m._device), 8
    yield "all ones", torch.ones((n, n), dtype=torch.uint8, device=m._device), 8
    i = torch.arange(n, device=m._device)
    yield "8 x 8 blocks", ((i[:, None] % 16 < 8) & (i[None, :] % 16 < 8)).to(torch.uint8), 4


def row(name, t, floor):
    med, lo, hi = t
    rate = floor / (med * 1e-3)
    say(f"    {name:13s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})  floor {floor / 1e6:8.1f} MB -> {rate / 1e9:8.1f} GB/s = "
        f"{100 * rate / HBM_PEAK:5.2f} % of the HBM peak")


def size(m, n, reps, host, only, calls):
    dev = m._device
    lib, h, st = _lib.load(), m._handle, _stream(dev)
    g = torch.Generator(device="cpu").manual_seed(n)
    acc = ((torch.full((n, n), 4, dtype=torch.int64) << 40) | torch.randint(0, 4 * 65535, (n, n), generator=g)).to(dev)       # 4 tiles per pixel
    labels = torch.empty((n, n), dtype=torch.int32, device=dev)
    dropped = torch.empty((n, n), dtype=torch.uint8, device=dev)
    n_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    say(f"mask {n} x {n} ({n * n / 1e6:.1f} M pixels)")
    for name, mask, conn in masks(m, n):
        if only and not any(o in name for o in only):
            continue

        def label():
            _lib.check(h, lib.keep_regions_label(h, _ptr(mask), n, n, conn, 1, _ptr(labels), _ptr(n_dev), st), "regions_label")
        label()
        k = int(n_dev.item())
        table = torch.empty((max(k, 1), NCOLS), dtype=torch.int64, device=dev)

        def tab(a):
            _lib.check(h, lib.keep_regions_table(h, _ptr(labels), n, n, k, _ptr(a), _ptr(table), st), "regions_table")
        say(f"  {name}: {k} regions, {conn}-connected, foreground {float(mask.float().mean()):.3f}")
        t_label = event_ms(label, reps)
        row("label", t_label, 5 * n * n)
        if calls == "label":                          # the run a kernel trace is taken of: nothing else launches the labelling kernels
            m.check_errors(wait=True)
            continue
        t_tab = event_ms(lambda: tab(None), reps)
        row("table", t_tab, 4 * n * n + 8 * NCOLS * k)
        t_acc = event_ms(lambda: tab(acc), reps)
        row("table+raster", t_acc, 12 * n * n + 8 * NCOLS * k)
        t_frag = event_ms(lambda: _lib.check(h, lib.keep_tissue_mask(h, _ptr(mask), n, n, 0, 0, 0, 1, _ptr(dropped), st), "tissue_mask"), reps)
        row("(fragments)", t_frag, 2 * n * n)
        say(f"    table / label = {t_tab[0] / t_label[0]:.2f}, table+raster / label = {t_acc[0] / t_label[0]:.2f}, label / fragments = "
            f"{t_label[0] / t_frag[0]:.2f}; effective clock {clock_mhz(m)} MHz")
        m.check_errors(wait=True)
        if host:
            from scipy import ndimage as ndi
            img = mask.cpu().numpy()
            t0 = time.perf_counter()
            lab, cnt = ndi.label(img, structure=np.ones((3, 3)) if conn == 8 else None)
            t1 = time.perf_counter()
            ndi.find_objects(lab)
            idx = np.arange(1, cnt + 1)
            ys, xs = np.indices(img.shape)
            area = ndi.sum_labels(img, lab, idx)
            ndi.sum_labels(xs, lab, idx)
            ndi.sum_labels(ys, lab, idx)
            t2 = time.perf_counter()
            same = cnt == k and bool(np.array_equal(lab, labels.cpu().numpy())) and bool(np.array_equal(np.rint(area), table[:k, 2].cpu().numpy()))
            say(f"    scipy on the host: label {1e3 * (t1 - t0):.0f} ms + find_objects / sum_labels {1e3 * (t2 - t1):.0f} ms = "
                f"{(t2 - t0) * 1e3 / (t_label[0] + t_tab[0]):.0f} x label + table; labels and areas equal: {same}")
        del table
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096,8192")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-max", type=int, default=4096, help="largest side the scipy composition is timed on")
    ap.add_argument("--masks", default="", help="comma-separated parts of mask names: only these masks (default: all four)")
    ap.add_argument("--calls", default="all", choices=("all", "label"), help="label: time keep_regions_label alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regions_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("regions_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    m = KEEPModel(KEEPShape(), precision="comp", towers=("image",))
    sd = synth_state_dict(KEEPShape(), seed=0)
    m.load_state_dict({k: v for k, v in sd.items() if k.startswith("visual") or k == "logit_scale"}, strict=True)
    m.to(dev).eval()
    say(f"tools/regions_bench.py on {torch.cuda.get_device_name(0)} (one box); device-event times, median of {a.reps} warm runs")
    say(f"idle effective clock {clock_mhz(m)} MHz")
    say()
    for n in (int(v) for v in a.sizes.split(",") if v):
        size(m, n, a.reps, n <= a.host_max and a.calls == "all", [v for v in a.masks.split(",") if v], a.calls)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
