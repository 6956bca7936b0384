#!/usr/bin/env python3
"""Nearest neighbours, measured: KEEPModel.topk at D = 768 on the four shapes its users bring.
Device-event times, median of the warm runs with the min-max spread; the new call and the yardstick alternate inside one loop in one
process, so a difference between them is not a difference between runs.

  topk         keep_topk: scores, selection and (for few queries) the merge of the bank segments, plus the unpack launch
  yardstick    what the parent commit offers on the device (the baseline, not the code under test): similarity(mode="raw") over
               bank chunks whose [Nq, chunk] matrix fits in 1 GiB, a torch.topk per chunk, and a torch.topk over the chunk winners

The binding peak: with few queries the floor is one read of the bank from HBM (8 TB/s); with many it is the 2 Nq M D FLOP of the
scores at the fp32 matrix rate (157 TFLOP/s).  The share of both is printed, the binding one named.

    python tools/topk_bench.py [--reps 20] [--big-reps 5] [--out profiles/topk_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keep_amd import KEEPModel                                             # noqa: E402

HBM_PEAK, F32_MATRIX_PEAK = 8.0e12, 157.0e12
D = 768
SHAPES = [(1, 100_000, 50, False, "one prompt or tile against a slide"), (264, 100_000, 50, False, "a prompt bank"),
          (10_000, 100_000, 20, False, "a kNN probe"), (100_000, 100_000, 20, True, "a slide's neighbour graph")]
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
    for _ in range(2):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ms[i].append(timed(fn))
    return [(float(np.median(m)), min(m), max(m)) for m in ms]


def fmt(t):
    med, lo, hi = t
    return f"{med:9.3f} ms (min {lo:.3f}, max {hi:.3f})"


def segments_chosen(nq, m, cus):
    """topk_segments of neighbours.hip."""
    qblocks, ntiles = (nq + 63) // 64, (m + 63) // 64
    if qblocks >= cus:
        return 1
    s = max(1, min(3 * cus // qblocks, 1024))
    tps = (ntiles + s - 1) // s
    return (ntiles + tps - 1) // tps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--big-reps", type=int, default=5, help="repeats of the shapes with 10 000 queries and more")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("topk_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    m = KEEPModel()
    m._create(dev)                                                         # the slide kernels need no weights
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    g = torch.Generator(device="cpu").manual_seed(0)
    bank = torch.nn.functional.normalize(torch.randn(100_000, D, generator=g), dim=1).to(dev).contiguous()
    fresh = torch.nn.functional.normalize(torch.randn(10_000, D, generator=g), dim=1).to(dev).contiguous()
    say(f"tools/topk_bench.py on {torch.cuda.get_device_name(0)} ({cus} CUs); D = {D} fp32, unit rows; device-event times, median of the warm "
        f"runs, topk and the yardstick alternating in one process")
    say()
    for nq, M, k, self_, use in SHAPES:
        q = bank[:nq] if self_ else fresh[:nq]
        b = bank[:M]
        chunk = max(1, min(M, (1 << 28) // nq))                          # [nq, chunk] fp32 within 1 GiB
        own = torch.arange(nq, device=dev)

        def new():
            return m.topk(q, b, k, normalize=False, exclude_self=self_)

        def yardstick():
            vals, idx = [], []
            for c0 in range(0, M, chunk):
                s = m.similarity(q, b[c0:c0 + chunk], mode="raw")
                if self_:
                    inside = (own >= c0) & (own < c0 + s.shape[1])
                    s[own[inside], own[inside] - c0] = -float("inf")
                v, i = torch.topk(s, min(k, s.shape[1]), dim=1)
                vals.append(v)
                idx.append(i + c0)
            v, i = torch.cat(vals, dim=1), torch.cat(idx, dim=1)
            top, pos = torch.topk(v, k, dim=1)
            return top, i.gather(1, pos)

        reps = a.reps if nq < 10_000 else a.big_reps
        t_new, t_old = event_ms([new, yardstick], reps)
        nb, (_, old_idx) = new(), yardstick()
        same = float((nb.index.sort(dim=1).values == old_idx.sort(dim=1).values).all(dim=1).float().mean())
        sec = t_new[0] * 1e-3
        flops, bytes_ = 2.0 * nq * M * D, M * D * 4.0
        share_f, share_b = flops / sec / F32_MATRIX_PEAK, bytes_ / sec / HBM_PEAK
        binding = "the 157 TFLOP/s f32 matrix rate" if nq >= 10_000 else "8 TB/s, one read of the bank"
        say(f"{nq} x {M}, k = {k}{', exclude_self' if self_ else ''} ({use}); segments chosen: {segments_chosen(nq, M, cus)}; "
            f"{reps} repeats; the yardstick in chunks of {chunk} bank rows")
        say(f"  topk        {fmt(t_new)}")
        say(f"  yardstick   {fmt(t_old)}   topk / yardstick = {t_new[0] / t_old[0]:.3f}")
        say(f"  {flops / sec / 1e12:7.2f} TFLOP/s = {100 * share_f:5.1f} % of the f32 matrix rate; {bytes_ / sec / 1e12:6.3f} TB/s of bank = "
            f"{100 * share_b:5.1f} % of 8 TB/s; binding: {binding}")
        say(f"  rows whose k indices equal the yardstick's as sets: {100 * same:.2f} % (the yardstick's scores are another fp32 sum)")
        say()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
