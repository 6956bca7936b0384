#!/usr/bin/env python3
"""The thumbnail tissue segmentation and the masked extraction, measured.

Part 1, `tissue_mask` per stage on synthetic thumbnails (keep_amd.synth.synth_thumbnail) of 1024^2, 4096^2 and 8192^2: the median of
>= 20 warm runs between device events around each C-ABI call, the bytes the stage has to move at the least (its input read once and
its output written once), the rate that implies and its share of the 8 TB/s HBM peak; next to it the numpy restatement's time on
the same input on the host (the only baseline that exists), and whether the device mask equals it.

  median+hist    keep_tissue_median_hist: RGB in (3 B / pixel), median bytes out (1 B / pixel)
  close          keep_tissue_mask with both area filters off: threshold + the four box passes (1 B in, 1 B out)
  holes          keep_tissue_mask on the closed mask, closing off, min_area 0: background labelling + fill (1 B in, 1 B out)
  fragments      keep_tissue_mask on the filled mask, closing off, min_hole 0: foreground labelling + drop (1 B in, 1 B out)

Part 2, synthetic slides of about --tiles grid cells with about two thirds glass (one compact section; three sections side by side): bytes requested through `read_region` and the wall
time of cohort.extract_slide_features with the per-pixel TissueRule (every band read whole) against the mask path (thumbnail ->
tissue_mask -> only the windows with kept cells).  The slide is never held whole: `read_region` composes each window from a pool
of synthetic tiles, the same way for both paths.

    python tools/tissue_bench.py [--sizes 1024,4096,8192] [--reps 20] [--tiles 100000] [--no-slide] [--out profiles/tissue_bench.txt]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keep_amd import KEEPModel, _lib, cohort                               # noqa: E402
from keep_amd.config import KEEPShape                                      # noqa: E402
from keep_amd.model import _ptr, _stream                                   # noqa: E402
from keep_amd.region import TissueRule, TissueSegmentation, tissue_mask_numpy      # noqa: E402
from keep_amd.synth import synth_state_dict, synth_thumbnail, synth_tile_family    # noqa: E402

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


def stages(m, n, reps, host):
    dev = m._device
    lib, h, st = _lib.load(), m._handle, _stream(dev)
    p = TissueSegmentation(min_area=100 * (n // 512) ** 2, min_hole=16 * (n // 512) ** 2)      # the presets' areas at this scale
    rgb = synth_thumbnail(n, n)
    x = torch.from_numpy(rgb).to(dev)
    med = torch.empty((n, n), dtype=torch.uint8, device=dev)
    hist = torch.empty(256, dtype=torch.int32, device=dev)
    closed, filled, final = (torch.empty((n, n), dtype=torch.uint8, device=dev) for _ in range(3))

    def call(name, *args):
        _lib.check(h, getattr(lib, name)(h, *args, st), name)
    runs = [("median+hist", 4, lambda: call("keep_tissue_median_hist", _ptr(x), n, n, n * 3, 3, p.mthresh, _ptr(med), _ptr(hist))),
            ("close", 2, lambda: call("keep_tissue_mask", _ptr(med), n, n, p.sthresh, p.close, 0, 0, _ptr(closed))),
            ("holes", 2, lambda: call("keep_tissue_mask", _ptr(closed), n, n, 0, 0, p.min_hole, 0, _ptr(filled))),
            ("fragments", 2, lambda: call("keep_tissue_mask", _ptr(filled), n, n, 0, 0, 0, p.min_area, _ptr(final)))]
    say(f"thumbnail {n} x {n} ({n * n / 1e6:.1f} M pixels), k = {p.mthresh}, close = {p.close}, min_hole = {p.min_hole}, min_area = {p.min_area}")
    total = 0.0
    for name, bytes_per_pixel, fn in runs:
        med_ms, lo, hi = event_ms(fn, reps)
        total += med_ms
        floor = bytes_per_pixel * n * n
        rate = floor / (med_ms * 1e-3)
        say(f"  {name:12s} {med_ms:9.3f} ms (min {lo:.3f}, max {hi:.3f}; {reps} runs)  floor {floor / 1e6:8.1f} MB -> {rate / 1e9:8.1f} GB/s = "
            f"{100 * rate / HBM_PEAK:5.2f} % of the HBM peak")
    whole, lo, hi = event_ms(lambda: m.tissue_mask(x, 16, p), reps)
    say(f"  {'sum of stages':12s} {total:9.3f} ms; KEEPModel.tissue_mask end to end {whole:.3f} ms (min {lo:.3f}, max {hi:.3f})")
    m.check_errors(wait=True)
    same = torch.equal(final, m.tissue_mask(x, 16, p).mask)
    say(f"  staged calls and tissue_mask give the same mask: {same}; tissue fraction {float(final.float().mean()):.3f}")
    if host:
        t0 = time.perf_counter()
        want, _ = tissue_mask_numpy(rgb, p)
        t_host = time.perf_counter() - t0
        say(f"  numpy restatement on the host: {t_host * 1e3:.0f} ms ({t_host * 1e3 / whole:.0f} x tissue_mask); device mask equal: "
            f"{bool(np.array_equal(want, final.cpu().numpy()))}")
    else:
        say("  numpy restatement on the host: not measured at this size (--host-max)")
    say()


class SyntheticSlide:
    """rows x cols tiles of 224: cell (r, c) is glass unless it lies in one of the layout's ellipses (about one third of the area); pixels come
    from a pool of stain_field tiles (tissue) or grey noise (glass) by (r, c).  Nothing of slide size is ever allocated; read_region composes the window asked for."""

    LAYOUTS = {"compact": ((0.45, 0.5, 0.33, 0.32),),                                                      # one section
               "scattered": ((0.3, 0.3, 0.22, 0.2), (0.7, 0.62, 0.2, 0.27), (0.25, 0.8, 0.1, 0.08))}     # three, side by side

    def __init__(self, rows, cols, dev, layout, pool=64, seed=9):
        self.rows, self.cols = rows, cols
        self.height, self.width = rows * 224, cols * 224
        g = np.random.default_rng(seed)
        yy, xx = np.mgrid[:rows, :cols]
        tissue = np.zeros((rows, cols), bool)
        for cy, cx, ry, rx in self.LAYOUTS[layout]:
            tissue |= ((yy / rows - cy) / ry) ** 2 + ((xx / cols - cx) / rx) ** 2 < 1
        self.tissue = tissue
        self.pick = g.integers(0, pool, (rows, cols))
        self.stain = synth_tile_family("stain_field", 0, pool, dev, seed=31).cpu().numpy()
        self.glass = (236 + g.integers(-2, 3, (pool, 224, 224, 3))).astype(np.uint8)        # plain grey glass: saturation <= 5
        self.bytes_read = self.calls = 0

    def tile(self, r, c):
        return (self.stain if self.tissue[r, c] else self.glass)[self.pick[r, c]]

    def read_region(self, x, y, w, h):
        self.bytes_read += w * h * 3
        self.calls += 1
        out = np.empty((h, w, 3), np.uint8)
        for r in range(y // 224, (y + h - 1) // 224 + 1):
            for c in range(x // 224, (x + w - 1) // 224 + 1):
                y0, y1, x0, x1 = max(y, r * 224), min(y + h, (r + 1) * 224), max(x, c * 224), min(x + w, (c + 1) * 224)
                out[y0 - y:y1 - y, x0 - x:x1 - x] = self.tile(r, c)[y0 - r * 224:y1 - r * 224, x0 - c * 224:x1 - c * 224]
        return out

    def thumbnail(self, ds):
        """Every ds-th pixel of the slide (224 % ds == 0), tile by tile."""
        k = 224 // ds
        out = np.empty((self.rows * k, self.cols * k, 3), np.uint8)
        for r in range(self.rows):
            for c in range(self.cols):
                out[r * k:(r + 1) * k, c * k:(c + 1) * k] = self.tile(r, c)[::ds, ::ds]
        return out


def slide_part(m, tiles, layout):
    side = int(round(tiles ** 0.5))
    s = SyntheticSlide(side, side, m._device, layout)
    say(f"synthetic slide, layout '{layout}': {s.height} x {s.width} pixels = {side * side} cells of 224, {100 * s.tissue.mean():.1f} % of them tissue "
        f"({s.height * s.width * 3 / 1e9:.1f} GB of RGB at the level being tiled)")
    out = tempfile.mkdtemp(prefix="tissue_bench_")
    res = {}
    for name, kw in (("TissueRule (per pixel, every band read)", dict(tissue=TissueRule())),
                     ("thumbnail mask (ds 16)", dict(thumbnail="make", thumbnail_downsample=16,
                                                     segmentation=TissueSegmentation(mthresh=7, min_area=100, min_hole=16)))):
        s.bytes_read = s.calls = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if "thumbnail" in kw:
            kw["thumbnail"] = s.thumbnail(16)                     # reading the thumbnail is part of the mask path's cost
            thumb_bytes = kw["thumbnail"].nbytes
        else:
            thumb_bytes = 0
        path = cohort.extract_slide_features(s.read_region, s.width, s.height, "bench", out, patch_size=224, band_rows=8, model=m, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        n = int(torch.load(path).shape[0])
        res[name] = (s.bytes_read + thumb_bytes, dt, n)
        say(f"  {name:42s} {n:6d} tiles kept, {s.calls:4d} read_region calls, {(s.bytes_read + thumb_bytes) / 1e9:7.3f} GB requested "
            f"({100 * (s.bytes_read + thumb_bytes) / (s.height * s.width * 3):5.1f} % of the slide), {dt:7.1f} s wall")
    (b0, t0, n0), (b1, t1, n1) = res.values()
    say(f"  mask path / rule path: {b1 / b0:.3f} of the bytes, {t1 / t0:.3f} of the wall time, {n1 / max(n0, 1):.3f} of the tiles "
        f"(the two rules do not keep the same cells: the tile count says how far apart they are)")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096,8192")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-max", type=int, default=4096, help="largest thumbnail side the numpy restatement is timed on")
    ap.add_argument("--tiles", type=int, default=100000)
    ap.add_argument("--no-slide", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tissue_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tissue_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    m = KEEPModel(KEEPShape(), precision="comp", towers=("image",))
    sd = synth_state_dict(KEEPShape(), seed=0)
    m.load_state_dict({k: v for k, v in sd.items() if k.startswith("visual") or k == "logit_scale"}, strict=True)
    m.to(dev).eval()
    say(f"tools/tissue_bench.py on {torch.cuda.get_device_name(0)}; device-event times, median of {a.reps} warm runs")
    say()
    for n in (int(v) for v in a.sizes.split(",") if v):
        stages(m, n, a.reps, host=n <= a.host_max)
    if not a.no_slide:
        for layout in SyntheticSlide.LAYOUTS:
            slide_part(m, a.tiles, layout)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
