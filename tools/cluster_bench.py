#!/usr/bin/env python3
"""Tile clustering, measured: one Lloyd iteration's assign step over N = 100 000 unit feature rows of D = 768
against K = 4, 16 and 64 centroids.  Device-event times, median of >= 20 warm runs with the min-max spread; the forms alternate inside
one loop in one process, so a difference between them is not a difference between runs:

  fused          keep_cluster_assign with the accumulators: labels, best, margin and the integer sums in one launch
  two launches   the same call with two_launch = 1: the assign, then an accumulate over the labels it wrote (the same words)
  assign alone   keep_cluster_assign without accumulators
  host path      what the parent commit offers (the baseline, not the code under test): KEEPModel.similarity(mode="argmax"), which
                 writes the [N,K] matrix, then torch index_add_ of the rows into [K,D] fp32 sums and a normalise

Bytes: the assign reads N D 4 B of features once (the centroids stay in cache), against the 8 TB/s HBM figure; the accumulate adds one
64-bit word per (label present in a workgroup's rows, column), counted here from the labels and the launch geometry.

    python tools/cluster_bench.py [--reps 20] [--out profiles/cluster_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keep_amd import KEEPModel                                             # noqa: E402
from keep_amd.cluster import ClusterSums                                   # noqa: E402

HBM_PEAK = 8.0e12
N, D = 100_000, 768
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


def rows_per_workgroup(n, k):
    """cluster_groups of cluster.hip for a launch that accumulates: 64 rows per group."""
    return 64 * (1 if n < 1 << 15 else 4 if (n >= 1 << 18 or k > 32) else 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cluster_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    m = KEEPModel()
    m._create(dev)                                                         # the slide kernels need no weights
    g = torch.Generator(device="cpu").manual_seed(0)
    # a slide has structure: 24 morphologies with noise, so that the labels of neighbouring rows repeat as they do in a scan
    centres = torch.nn.functional.normalize(torch.randn(24, D, generator=g), dim=1)
    x = centres[torch.randint(0, 24, (N,), generator=g)] + 0.03 * torch.randn(N, D, generator=g)
    x = torch.nn.functional.normalize(x, dim=1).to(dev).contiguous()
    say(f"tools/cluster_bench.py on {torch.cuda.get_device_name(0)}; N = {N}, D = {D} fp32 ({N * D * 4 / 1e6:.0f} MB of features); "
        f"device-event times, median of {a.reps} warm runs, the forms alternating in one process")
    say()
    for K in (4, 16, 64):
        cen = x[torch.randperm(N, generator=g)[:K].to(dev)].contiguous()
        sums_f, sums_t = ClusterSums(K, D, dev), ClusterSums(K, D, dev)
        labels = torch.empty(N, dtype=torch.int32, device=dev)
        best, margin = (torch.empty(N, dtype=torch.float32, device=dev) for _ in range(2))
        host_sums = torch.zeros((K, D), dtype=torch.float32, device=dev)

        def fused():
            m._cluster_assign(x, cen, labels, best, margin, None, sums_f.skipped, sums_f)

        def two_launches():
            m._cluster_assign(x, cen, labels, best, margin, None, sums_t.skipped, sums_t, fused=False)

        def alone():
            m._cluster_assign(x, cen, labels, best, margin, None, None, None)

        def host_path():
            _, lab = m.similarity(x, cen, mode="argmax")
            host_sums.zero_()
            host_sums.index_add_(0, lab.to(torch.int64), x)
            torch.nn.functional.normalize(host_sums, dim=1)

        t_fused, t_two, t_alone, t_host = event_ms([fused, two_launches, alone, host_path], a.reps)
        same = bool(torch.equal(sums_f.buf, sums_t.buf))                   # both ran the same number of times from zero
        lab = labels.cpu().numpy()
        rpw = rows_per_workgroup(N, K)
        present = sum(len(np.unique(lab[i:i + rpw])) for i in range(0, N, rpw))
        atomic_bytes = present * D * 8
        t_acc = max(t_fused[0] - t_alone[0], 1e-6)
        say(f"K = {K}: {present} (workgroup, label) pairs of {rpw} rows -> {atomic_bytes / 1e6:.1f} MB of 64-bit atomic adds "
            f"(one per (row, column) would be {N * D * 8 / 1e6:.0f} MB)")
        say(f"  fused assign + accumulate   {fmt(t_fused)}  {N * D * 4 / (t_fused[0] * 1e-3) / 1e12:6.2f} TB/s of features = "
            f"{100 * N * D * 4 / (t_fused[0] * 1e-3) / HBM_PEAK:.1f} % of the 8 TB/s HBM peak")
        say(f"  two launches                {fmt(t_two)}  fused / two launches = {t_fused[0] / t_two[0]:.3f}; the accumulators are equal: {same}")
        say(f"  assign alone                {fmt(t_alone)}  {N * D * 4 / (t_alone[0] * 1e-3) / 1e12:6.2f} TB/s of features = "
            f"{100 * N * D * 4 / (t_alone[0] * 1e-3) / HBM_PEAK:.1f} % of the HBM peak")
        say(f"  accumulate (fused - alone)  {t_acc:8.3f} ms                          {atomic_bytes / (t_acc * 1e-3) / 1e9:8.1f} GB/s of added bytes")
        say(f"  host path (the baseline)    {fmt(t_host)}  fused / host path = {t_fused[0] / t_host[0]:.3f}")
        say()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
