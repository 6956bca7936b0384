#!/usr/bin/env python3
"""Polygon annotations to masks, measured.

For masks of 1024^2, 4096^2 and 8192^2 pixels at downsample 1, the median of >= 20 warm runs between device events around
keep_poly_fill (its one readback of the crossing count included), with the min-max spread, the bytes the call has to move at the least
(4 B zeroed, 4 B read and 1 B written per pixel, 4 B per crossing), the rate that implies and its share of the 8 TB/s HBM peak, on

  (a) the outlines of the four masks of tools/regions_bench.py taken back (tissue mask: few long rings; raw threshold: many small ones;
      all ones: one ring of four vertices; 8 x 8 blocks), traced on the device by keep_outline_*;
  (b) a rectangle ROI over the middle of the mask: four edges, two of which cross every row they span;
  (c) a circle of 10^5 vertices: most of its edges cross no row.

Beside them keep_amd.annotation.fill_numpy on the host up to --host-max, and keep_mask_tile_counts for 100 000 tiles of 224 pixels at
downsample 16 and 1 (no floor is given: the bytes it reads depend on the cache).  Every size runs in a child process under its own time
limit, so one that hangs or runs out of memory ends alone.

    python tools/annotation_bench.py [--sizes 1024,4096,8192] [--reps 20] [--host-max 1024] [--limit 600] [--out profiles/annotation_bench.txt]
"""
import argparse
import ctypes as C
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
from keep_amd.annotation import PolygonSet, fill_numpy                     # noqa: E402
from keep_amd.config import small_shape                                    # noqa: E402
from keep_amd.model import _ptr, _stream                                   # noqa: E402
from keep_amd.outline import RegionOutlines                                # noqa: E402
from keep_amd.synth import synth_state_dict                                # noqa: E402
from regions_bench import HBM_PEAK, event_ms, masks                        # noqa: E402

LINES = []
TILES, PATCH = 100_000, 224


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def inputs(m, n):
    """(name, PolygonSet, the mask it must give or None)."""
    for name, mask, conn in masks(m, n):
        try:                                                # beyond 2^20 rings or 2^24 vertices there is nothing to fill in one call
            regs = m.mask_regions(mask, conn, max_regions=1 << 20)
            o = m.region_outlines(regs, max_rings=1 << 20)
            polys, want = PolygonSet.from_outlines(RegionOutlines(o.rings, o.vertices, 1, (0, 0), o.n)), (regs.labels > 0).to(torch.uint8)
            del regs, o
        except ValueError as e:
            polys, want = str(e), None
        yield f"{name} taken back", polys, want
    q = n // 8
    roi = np.array([(q, q), (n - q, q), (n - q, n - 2 * q), (q, n - 2 * q)], np.int64)
    yield "rectangle ROI", PolygonSet(roi, [0, 4]), None
    t = np.arange(100_000) * (2 * np.pi / 100_000)
    ring = np.floor(np.stack([n / 2 + 0.45 * n * np.cos(t), n / 2 + 0.45 * n * np.sin(t)], 1) + 0.5).astype(np.int64)
    yield "circle of 10^5 vertices", PolygonSet(ring, [0, len(ring)]), None


def size(m, n, reps, host):
    dev = m._device
    lib, h, st = _lib.load(), m._handle, _stream(dev)
    out = torch.empty((n, n), dtype=torch.uint8, device=dev)
    crossings = C.c_int64(0)
    say(f"mask {n} x {n} ({n * n / 1e6:.1f} M pixels), downsample 1")
    for name, polys, want in inputs(m, n):
        if isinstance(polys, str):
            say(f"  {name}: not filled: {polys}")
            continue
        v, rs, wt = (torch.from_numpy(a).to(dev) for a in (polys.vertices, polys.ring_start, polys.weights("union")))
        V, R = int(v.shape[0]), int(rs.shape[0]) - 1

        def fill():
            _lib.check(h, lib.keep_poly_fill(h, _ptr(v), V, _ptr(rs), R, _ptr(wt), 1, n, n, 0, 0, 0, 1, None, _ptr(out), C.byref(crossings), st),
                       "poly_fill")
        fill()
        ok = "" if want is None else f"; equals the mask it came from: {bool(torch.equal(out, want))}"
        cr = int(crossings.value)
        say(f"  {name}: {R} rings, {V} vertices, {cr} crossings; workspace {lib.keep_workspace_bytes(h) / 1e6:.0f} MB{ok}")
        med, lo, hi = event_ms(fill, reps)
        floor = 9 * n * n + 4 * cr
        rate = floor / (med * 1e-3)
        say(f"    fill          {med:9.3f} ms (min {lo:.3f}, max {hi:.3f})  floor {floor / 1e6:8.1f} MB -> {rate / 1e9:8.1f} GB/s = "
            f"{100 * rate / HBM_PEAK:5.2f} % of the HBM peak")
        if host:
            t0 = time.perf_counter()
            ref = fill_numpy(polys, 1, (n, n))
            t1 = time.perf_counter()
            say(f"    fill_numpy on the host: {1e3 * (t1 - t0):.0f} ms = {(t1 - t0) * 1e3 / med:.0f} x the fill; masks equal: "
                f"{bool(np.array_equal(ref, out.cpu().numpy()))}")
        m.check_errors(wait=True)
        del v, rs, wt
    g = torch.Generator().manual_seed(n)
    mask = (torch.rand((n, n), generator=g) < 0.5).to(torch.uint8).to(dev)
    for d in (16, 1):
        coords = torch.stack([torch.randint(-PATCH, n * d, (TILES,), generator=g), torch.randint(-PATCH, n * d, (TILES,), generator=g)], 1).to(dev)
        counts = torch.empty((TILES, 2), dtype=torch.int32, device=dev)
        med, lo, hi = event_ms(lambda: _lib.check(h, lib.keep_mask_tile_counts(h, _ptr(mask), n, n, d, 0, 0, _ptr(coords), TILES, PATCH, _ptr(counts),
                                                                              st), "mask_tile_counts"), reps)
        say(f"  tile counts, {TILES} tiles of {PATCH} at downsample {d}: {med:9.3f} ms (min {lo:.3f}, max {hi:.3f}); "
            f"{int(counts[:, 0].sum())} pixels visited")
    say()


def child(n, reps, host, out):
    dev = torch.device("cuda:0")
    shape = small_shape(2, 2)                           # the calls use the handle's arena and stream only
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
    ap.add_argument("--host-max", type=int, default=1024, help="largest side fill_numpy is timed on")
    ap.add_argument("--limit", type=int, default=600, help="seconds every size may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "annotation_bench.txt"))
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("annotation_bench needs the GPU: there is nothing to measure without one")
    if a.child:
        return child(a.child, a.reps, a.child <= a.host_max, a.out)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(f"tools/annotation_bench.py on {torch.cuda.get_device_name(0)} (one box); device-event times, median of {a.reps} warm runs\n\n")
    for n in (int(v) for v in a.sizes.split(",") if v):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), "--reps", str(a.reps), "--host-max", str(a.host_max),
                                 "--out", a.out], timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            rc = "time limit"
        if rc != 0:                                     # nothing more is started on a device that has just failed
            with open(a.out, "a") as f:
                f.write(f"mask {n} x {n}: the child ended with {rc}; stopped here\n")
            sys.exit(f"annotation_bench: size {n} ended with {rc}")


if __name__ == "__main__":
    main()
