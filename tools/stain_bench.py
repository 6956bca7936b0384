#!/usr/bin/env python3
"""The Macenko stain normalisation, measured.

Part 1, `keep_stain_apply_u8` on 256 tiles and on --tiles tiles' worth of pixels (stain_field tiles, then uniformly random colours): the median of warm runs between device
events, the bytes it has to move (3 read + 3 written per pixel), the rate and its share of the 8 TB/s HBM peak; whether the result
equals the numpy restatement (a strided sample); a plain device copy of the same bytes as the yardstick of what HBM gives a
read + write stream; and, on the 256 tiles, what the device offered before this kernel: the same
transform in torch float ops (log, matmul, exp, round, clamp) in the same process.

Part 2, the three fit passes and `KEEPModel.stain_fit` end to end on a 4096 x 6144 thumbnail of stain_field tiles.

Part 3, `encode_region` over 256 tiles of 224 with and without `stain=`, alternating.

    python tools/stain_bench.py [--tiles 100000] [--reps 20] [--no-encode] [--out profiles/stain_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keep_amd import KEEPModel                                            # noqa: E402
from keep_amd import stain as S                                            # noqa: E402
from keep_amd.config import KEEPShape                                      # noqa: E402
from keep_amd.synth import synth_state_dict, synth_tile_family             # noqa: E402

HBM_PEAK = 8.0e12
TILE_PIXELS = 224 * 224
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


def rate_line(name, ms, lo, hi, reps, n_pixels):
    moved = 6 * n_pixels
    rate = moved / (ms * 1e-3)
    say(f"  {name:34s} {ms:10.3f} ms (min {lo:.3f}, max {hi:.3f}; {reps} runs)  {moved / 1e9:8.3f} GB read + written -> {rate / 1e9:8.1f} GB/s = "
        f"{100 * rate / HBM_PEAK:5.2f} % of the HBM peak")


def torch_float_transform(x, T, io):
    """The same transform with what the device offered before: float ops on the same pixels."""
    od = -torch.log((x.to(torch.float32) + 1.0) / io)
    return (io * torch.exp(-(od @ T.t()))).round().clamp(0, 255).to(torch.uint8)


def apply_part(m, fit, tiles, reps):
    dev = m._device
    plan, tb = m._stain_plan(fit), fit.tables()
    g = torch.Generator(device=dev).manual_seed(1)
    L = 256 * TILE_PIXELS
    kinds = (("stain_field tiles", synth_tile_family("stain_field", 0, 256, dev, seed=35).reshape(L, 3).contiguous()),
             ("uniformly random colours", torch.randint(0, 256, (L, 3), dtype=torch.uint8, device=dev, generator=g)))
    say(f"keep_stain_apply_u8, |T|max = {np.abs(fit.matrix()).max():.3f}; both tables are looked up in LDS, so neighbouring pixels of like colour "
        f"(an image) share banks and addresses, random colours do not: the two inputs bracket the bank conflicts")
    T = torch.from_numpy(fit.matrix()).to(dev, torch.float32)
    for kind, block in kinds:
        say(f" {kind}")
        out = torch.empty_like(block)
        ms, lo, hi = event_ms(lambda: m._stain_apply(block, out, plan), reps)
        rate_line("256 tiles, out of place", ms, lo, hi, reps, L)
        idx = torch.arange(0, L, 997, device=dev)
        want = S.stain_apply_numpy(block[idx].cpu().numpy(), tb["od_q"], tb["t_q"], tb["exp_lut"], tb["lo"])
        say(f"  equals the numpy restatement on a sample of {len(idx)} pixels: {bool(np.array_equal(out[idx].cpu().numpy(), want))}")
        fms, flo, fhi = event_ms(lambda: torch_float_transform(block, T, 240.0), reps)
        say(f"  {'torch float ops, same pixels':34s} {fms:10.3f} ms (min {flo:.3f}, max {fhi:.3f}; {reps} runs): {fms / ms:.1f} x the kernel; "
            f"values that differ from the kernel's by more than 1 level: "
            f"{int(((torch_float_transform(block, T, 240.0).to(torch.int16) - out.to(torch.int16)).abs() > 1).sum())}")
        ims, ilo, ihi = event_ms(lambda: m._stain_apply(out, out, plan), reps)
        rate_line("256 tiles, in place", ims, ilo, ihi, reps, L)
        del out
        n = tiles * TILE_PIXELS
        big = torch.empty((n, 3), dtype=torch.uint8, device=dev)
        for i in range(0, n, L):                                   # the 256 tiles over and over
            big[i:i + L] = block[:min(L, n - i)]
        dst = torch.empty_like(big)
        r = max(3, reps // 4)
        ms, lo, hi = event_ms(lambda: m._stain_apply(big, dst, plan), r, warm=1)
        rate_line(f"{tiles} tiles, out of place", ms, lo, hi, r, n)
        cms, clo, chi = event_ms(lambda: dst.copy_(big), r, warm=1)
        say(f"  {'torch copy of the same bytes':34s} {cms:10.3f} ms (min {clo:.3f}, max {chi:.3f}; {r} runs)  -> {6 * n / (cms * 1e-3) / 1e9:8.1f} GB/s: "
            f"the kernel runs at {cms / ms:.2f} of a plain copy's rate")
        m._stain_apply(big, dst, plan)
        idx = torch.arange(0, n, 1000003, device=dev)
        want = S.stain_apply_numpy(big[idx].cpu().numpy(), tb["od_q"], tb["t_q"], tb["exp_lut"], tb["lo"])
        say(f"  equals the numpy restatement on a sample of {len(idx)} pixels: {bool(np.array_equal(dst[idx].cpu().numpy(), want))}")
        del big, dst
    say()


def fit_part(m, reps, h=4096, w=6144):
    dev = m._device
    pool = synth_tile_family("stain_field", 0, 64, dev, seed=31)
    rows, cols = -(-h // 224), -(-w // 224)
    pick = torch.from_numpy(np.random.default_rng(5).integers(0, 64, rows * cols)).to(dev)
    thumb = pool[pick].view(rows, cols, 224, 224, 3).permute(0, 2, 1, 3, 4).reshape(rows * 224, cols * 224, 3)[:h, :w].contiguous()
    fit = m.stain_fit(thumb)
    p = m._StainPasses(m)
    od, beta = S.od_table(240), S.beta_level(0.15)
    acc = [p.moments(thumb, None, 1, od, beta, None), p.angle_hist(thumb, None, 1, od, beta, fit.v_q, None),
           p.conc_hist(thumb, None, 1, od, fit.minv_q, None)]
    say(f"stain fit on a {h} x {w} thumbnail ({h * w / 1e6:.1f} M pixels, {fit.n / (h * w):.3f} of them kept), 3 bytes read per pixel and pass")
    runs = [("moments", lambda: p.moments(thumb, None, 1, od, beta, acc[0])),
            ("angle histogram", lambda: p.angle_hist(thumb, None, 1, od, beta, fit.v_q, acc[1])),
            ("concentration histograms", lambda: p.conc_hist(thumb, None, 1, od, fit.minv_q, acc[2]))]
    total = 0.0
    for name, fn in runs:
        ms, lo, hi = event_ms(fn, reps)
        total += ms
        rate = 3 * h * w / (ms * 1e-3)
        say(f"  {name:26s} {ms:9.3f} ms (min {lo:.3f}, max {hi:.3f}; {reps} runs)  {rate / 1e9:8.1f} GB/s = {100 * rate / HBM_PEAK:5.2f} % of the HBM peak")
    ms, lo, hi = event_ms(lambda: m.stain_fit(thumb), reps)
    say(f"  sum of the passes {total:.3f} ms; KEEPModel.stain_fit end to end (host algebra and read-backs included) {ms:.3f} ms (min {lo:.3f}, max {hi:.3f})")
    say()
    return fit


def encode_part(m, reps):
    dev = m._device
    tiles = synth_tile_family("stain_field", 0, 256, dev, seed=33)
    region = tiles.view(16, 16, 224, 224, 3).permute(0, 2, 1, 3, 4).reshape(16 * 224, 16 * 224, 3).contiguous()
    fit = m.stain_fit(region)
    runs = {"stain=None": lambda: m.encode_region(region, 224), "stain=fit": lambda: m.encode_region(region, 224, stain=fit)}
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
    say("encode_region over 256 tiles of 224 (grid, cut, encode), alternating runs")
    for k, v in ms.items():
        say(f"  {k:12s} median {np.median(v):9.3f} ms (min {min(v):.3f}, max {max(v):.3f}; {reps} runs)")
    d = float(np.median(ms["stain=fit"]) - np.median(ms["stain=None"]))
    say(f"  difference of the medians {d:+.3f} ms = {100 * d / float(np.median(ms['stain=None'])):+.2f} % of the step")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-encode", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stain_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stain_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    m = KEEPModel(KEEPShape(), precision="comp", towers=("image",))
    sd = synth_state_dict(KEEPShape(), seed=0)
    m.load_state_dict({k: v for k, v in sd.items() if k.startswith("visual") or k == "logit_scale"}, strict=True)
    m.to(dev).eval()
    say(f"tools/stain_bench.py on {torch.cuda.get_device_name(0)}; device-event times, median of warm runs")
    say()
    fit = fit_part(m, a.reps)
    apply_part(m, fit, a.tiles, a.reps)
    if not a.no_encode:
        encode_part(m, a.reps)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
