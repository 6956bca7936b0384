#!/usr/bin/env python3
"""Tile quality control, measured.

Part 1, `keep_region_quality` (through `KEEPModel._quality_table`: the cell check with its read-back, the memset of the table and the
kernel) in three settings: (a) 256 contiguous tiles of 224, (b) --tiles tiles' worth of pixels, contiguous, (c) a grid of about
--tiles cells of 224 at step 112 over one region (every pixel lies in up to four cells).  Each on stain_field tiles and on uniformly
random colours (the pen boxes are looked up in LDS tables, so the two bracket the bank conflicts): the median of warm runs between
device events, the bytes the cells hold (N P^2 C) per second and their share of the 8 TB/s HBM peak.  Yardsticks in the same process: a
plain device read of the same bytes (an int64 sum) and a plain copy (which also writes them); and, on the 256 tiles, the same twelve
columns from torch ops on the device, which is what a caller had before this kernel.  A sample of tiles is compared with the numpy
restatement.

Part 2, `keep_pen_mask` on a 4096 x 6144 thumbnail.

Part 3, `encode_region` over 256 tiles of 224 with `quality=None` and with a gate that keeps every tile, alternating.

    python tools/quality_bench.py [--tiles 100000] [--reps 20] [--no-encode] [--out profiles/quality_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keep_amd import KEEPModel, QualityGate, QualityRules                  # noqa: E402
from keep_amd import quality as Q                                          # noqa: E402
from keep_amd.config import KEEPShape                                      # noqa: E402
from keep_amd.synth import synth_state_dict, synth_tile_family             # noqa: E402

HBM_PEAK = 8.0e12
P = 224
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def event_ms(fn, reps, warm=3):
    """Median, min and max over `reps` warm runs of fn(), each between two device events."""
    for _ in range(warm):
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


def rate_line(name, ms, lo, hi, reps, nbytes):
    rate = nbytes / (ms * 1e-3)
    say(f"  {name:40s} {ms:10.3f} ms (min {lo:.3f}, max {hi:.3f}; {reps} runs)  {nbytes / 1e9:8.3f} GB -> {rate / 1e9:8.1f} GB/s = "
        f"{100 * rate / HBM_PEAK:5.2f} % of the HBM peak")
    return rate


def torch_table(tiles, rules):
    """The twelve columns from torch ops on the device: uint8 [N,S,S,3] -> int64 [N,12]."""
    c = tiles.to(torch.int32)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    mx, mn = c.amax(dim=3), c.amin(dim=3)
    cls = torch.zeros_like(mx)
    cls[(mx > 0) & (255 * (mx - mn) >= rules.sat_min * mx)] = Q.TISSUE
    cls[mn >= rules.white_min] = Q.GLASS
    cls[mx <= rules.dark_max] = Q.DARK
    for k in reversed(range(4)):
        for kk, r0, r1, g0, g1, b0, b1 in rules.pen:
            if kk == k:
                cls[(r >= r0) & (r <= r1) & (g >= g0) & (g <= g1) & (b >= b0) & (b <= b1)] = k + 1
    out = torch.zeros((tiles.shape[0], Q.NCOLS), dtype=torch.int64, device=tiles.device)
    for k in range(1, 8):
        out[:, k - 1] = (cls == k).sum(dim=(1, 2))
    grey = (77 * r + 150 * g + 29 * b + 128) >> 8
    L = (4 * grey[:, 1:-1, 1:-1] - grey[:, 1:-1, :-2] - grey[:, 1:-1, 2:] - grey[:, :-2, 1:-1] - grey[:, 2:, 1:-1]).to(torch.int64)
    t = (cls[:, 1:-1, 1:-1] == Q.TISSUE).to(torch.int64)
    out[:, 7], out[:, 8] = L.sum(dim=(1, 2)), (L * L).sum(dim=(1, 2))
    out[:, 9], out[:, 10], out[:, 11] = t.sum(dim=(1, 2)), (L * t).sum(dim=(1, 2)), (L * L * t).sum(dim=(1, 2))
    return out


def sample_equal(region_view, cells, table, rules, k=4):
    """The table rows of k cells spread over the list against the numpy restatement."""
    idx = np.linspace(0, len(cells) - 1, k).astype(np.int64)
    ok = True
    for i in idx:
        x, y = int(cells[i, 0]), int(cells[i, 1])
        want = Q.tile_quality_numpy(region_view[y:y + P, x:x + P].cpu().numpy(), [(0, 0)], P, rules)[0]
        ok = ok and bool(np.array_equal(table[i].cpu().numpy(), want))
    return ok


def yardsticks(x, nbytes_cells, reps):
    """A plain read and a plain copy of the bytes of x (the unique bytes of the setting)."""
    flat = x.reshape(-1)
    n8 = flat.numel() // 8 * 8
    words = flat[:n8].view(torch.int64)
    ms, lo, hi = event_ms(lambda: words.sum(), reps, warm=1)
    say(f"  {'torch int64 sum over its bytes (a read)':40s} {ms:10.3f} ms (min {lo:.3f}, max {hi:.3f}; {reps} runs)  {n8 / 1e9:8.3f} GB -> "
        f"{n8 / (ms * 1e-3) / 1e9:8.1f} GB/s")
    dst = torch.empty_like(flat)
    cms, clo, chi = event_ms(lambda: dst.copy_(flat), reps, warm=1)
    say(f"  {'torch copy of its bytes (read + write)':40s} {cms:10.3f} ms (min {clo:.3f}, max {chi:.3f}; {reps} runs)  {flat.numel() / 1e9:8.3f} GB read "
        f"-> {flat.numel() / (cms * 1e-3) / 1e9:8.1f} GB/s read (+ as much written)")
    del dst
    return ms, cms


def table_part(m, tiles, reps):
    dev = m._device
    rules = QualityRules()
    g = torch.Generator(device=dev).manual_seed(1)
    kinds = (("stain_field tiles", synth_tile_family("stain_field", 0, 256, dev, seed=35).contiguous()),
             ("uniformly random colours", torch.randint(0, 256, (256, P, P, 3), dtype=torch.uint8, device=dev, generator=g)))
    say(f"keep_region_quality, patch {P}, the default rules ({len(rules.pen)} pen boxes); times include the cell check (a launch, a 4-byte read-back "
        f"and its synchronisation) and the memset of the table")
    for kind, block in kinds:
        say(f" {kind}")

        def contiguous(n):
            x = torch.empty((n, P, P, 3), dtype=torch.uint8, device=dev)
            for i in range(0, n, 256):
                x[i:i + 256] = block[:min(256, n - i)]
            cells = torch.zeros((n, 2), dtype=torch.int32, device=dev)
            cells[:, 1] = torch.arange(n, dtype=torch.int32, device=dev) * P
            return x.view(n * P, P, 3), cells

        # (a) 256 contiguous tiles
        x, cells = contiguous(256)
        run = lambda: m._quality_table(x, x.shape[0], x.shape[1], 3, x.shape[1] * 3, cells, P, rules)
        ms, lo, hi = event_ms(run, reps)
        rate_line("(a) 256 contiguous tiles", ms, lo, hi, reps, 256 * P * P * 3)
        say(f"  equals the numpy restatement on a sample of 4 tiles: {sample_equal(x, cells.cpu().numpy(), run(), rules)}")
        tms, tlo, thi = event_ms(lambda: torch_table(block, rules), max(3, reps // 4), warm=1)
        say(f"  {'torch ops, the same twelve columns':40s} {tms:10.3f} ms (min {tlo:.3f}, max {thi:.3f}): {tms / ms:.1f} x the kernel; equal to it: "
            f"{bool(torch.equal(torch_table(block, rules), run()))}")
        yardsticks(x, 256 * P * P * 3, reps)
        # (b) --tiles tiles' worth of pixels
        r = max(3, reps // 4)
        x, cells = contiguous(tiles)
        run = lambda: m._quality_table(x, x.shape[0], x.shape[1], 3, x.shape[1] * 3, cells, P, rules)
        ms, lo, hi = event_ms(run, r, warm=1)
        rate_line(f"(b) {tiles} contiguous tiles", ms, lo, hi, r, tiles * P * P * 3)
        say(f"  equals the numpy restatement on a sample of 4 tiles: {sample_equal(x, cells.cpu().numpy(), run(), rules)}")
        rms, cms = yardsticks(x, tiles * P * P * 3, r)
        say(f"  the kernel takes {ms / rms:.2f} x the plain read's time and {ms / cms:.2f} x the copy's")
        del x, cells
        # (c) a grid at step P / 2 over one region
        side = int(np.ceil(np.sqrt(tiles)))
        gx, gy = side, -(-tiles // side)
        W, H = (gx - 1) * (P // 2) + P, (gy - 1) * (P // 2) + P
        rows, cols = -(-H // P), -(-W // P)
        pick = torch.from_numpy(np.random.default_rng(5).integers(0, 256, rows * cols)).to(dev)
        region = block[pick].view(rows, cols, P, P, 3).permute(0, 2, 1, 3, 4).reshape(rows * P, cols * P, 3)[:H, :W].contiguous()
        yy, xx = torch.meshgrid(torch.arange(gy, device=dev) * (P // 2), torch.arange(gx, device=dev) * (P // 2), indexing="ij")
        cells = torch.stack([xx.reshape(-1), yy.reshape(-1)], 1).to(torch.int32).contiguous()
        n = int(cells.shape[0])
        run = lambda: m._quality_table(region, H, W, 3, W * 3, cells, P, rules)
        ms, lo, hi = event_ms(run, r, warm=1)
        rate_line(f"(c) {n} cells, step {P // 2}, {H} x {W} region", ms, lo, hi, r, n * P * P * 3)
        say(f"  the region itself holds {H * W * 3 / 1e9:.3f} GB: {H * W * 3 / (ms * 1e-3) / 1e9:.1f} GB/s of unique bytes")
        say(f"  equals the numpy restatement on a sample of 4 cells: {sample_equal(region, cells.cpu().numpy(), run(), rules)}")
        yardsticks(region, n * P * P * 3, r)
        del region, cells
    say()


def pen_mask_part(m, reps, h=4096, w=6144):
    dev = m._device
    pool = synth_tile_family("stain_field", 0, 64, dev, seed=31)
    rows, cols = -(-h // P), -(-w // P)
    pick = torch.from_numpy(np.random.default_rng(5).integers(0, 64, rows * cols)).to(dev)
    thumb = pool[pick].view(rows, cols, P, P, 3).permute(0, 2, 1, 3, 4).reshape(rows * P, cols * P, 3)[:h, :w].contiguous()
    ms, lo, hi = event_ms(lambda: m.pen_mask(thumb), reps)
    say(f"keep_pen_mask on a {h} x {w} thumbnail: 3 bytes read and 1 written per pixel")
    rate_line("class mask", ms, lo, hi, reps, 4 * h * w)
    got = m.pen_mask(thumb[:300, :400])
    say(f"  equals the numpy restatement on a 300 x 400 corner: {bool(np.array_equal(got.cpu().numpy(), Q.pen_mask_numpy(thumb[:300, :400].cpu().numpy())))}")
    say()


def encode_part(m, reps):
    dev = m._device
    tiles = synth_tile_family("stain_field", 0, 256, dev, seed=33)
    region = tiles.view(16, 16, P, P, 3).permute(0, 2, 1, 3, 4).reshape(16 * P, 16 * P, 3).contiguous()
    gate = QualityGate()
    assert m.region_grid(region, P, quality=gate).shape[0] == 256
    runs = {"quality=None": lambda: m.encode_region(region, P), "quality=gate": lambda: m.encode_region(region, P, quality=gate)}
    for fn in runs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(reps):                                         # alternating, so that drift hits both alike
        for k, fn in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    say("encode_region over 256 tiles of 224 (grid, [measure, gate,] cut, encode), a gate that keeps every tile, alternating runs")
    for k, v in ms.items():
        say(f"  {k:13s} median {np.median(v):9.3f} ms (min {min(v):.3f}, max {max(v):.3f}; {reps} runs)")
    d = float(np.median(ms["quality=gate"]) - np.median(ms["quality=None"]))
    say(f"  difference of the medians {d:+.3f} ms = {100 * d / float(np.median(ms['quality=None'])):+.2f} % of the step")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-encode", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quality_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("quality_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    m = KEEPModel(KEEPShape(), precision="comp", towers=("image",))
    sd = synth_state_dict(KEEPShape(), seed=0)
    m.load_state_dict({k: v for k, v in sd.items() if k.startswith("visual") or k == "logit_scale"}, strict=True)
    m.to(dev).eval()
    say(f"tools/quality_bench.py on {torch.cuda.get_device_name(0)}; device-event times, median of warm runs")
    say()
    table_part(m, a.tiles, a.reps)
    pen_mask_part(m, a.reps)
    if not a.no_encode:
        encode_part(m, a.reps)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
