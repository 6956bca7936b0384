#!/usr/bin/env python3
"""Exact t-SNE, measured: N = 10 000 and 100 000 unit feature rows of D = 384 in 10 blobs, perplexity 20 (60
neighbours).  Device-event times, median of the warm runs with the min-max spread; the forms alternate inside one loop in one process,
so a difference between them is not a difference between runs:

  repulsion          keep_tsne_repulsion alone: N (N - 1) pairs, counted as 10 fp32 VALU issue slots each (8 instructions and a
                     reciprocal that issues at half rate) against the vector unit's 78.6 T lane-instructions/s (157.3 TFLOP/s of fma)
  step               keep_tsne_step alone (the reduction of the partials and the update, with and without the KL / gradient-norm sums)
  iteration          both, as tsne_fit issues them
  torch form         the same iteration in torch ops on the device (the baseline, not the code under test: the parent commit offers
                     nothing else): the all-pairs part in row chunks, cdist-style, the attraction by index_add_
  setup              topk, affinities, graph: host clock, the device synchronised (the graph reads two counts back)
  fit                KEEPModel.tsne_fit, 1000 iterations, init="random", end to end on the host clock

    python tools/tsne_bench.py [--reps 20] [--sizes 10000,100000] [--out profiles/tsne_bench.txt]
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
from keep_amd import KEEPModel, _lib, tsne as T                             # noqa: E402
from keep_amd.model import _ptr                                            # noqa: E402

D, PERPLEXITY, K = 384, 20.0, 60
SLOTS_PER_PAIR = 10
LANE_RATE = 256 * 4 * 32 * 2.4e9                                           # CUs x SIMDs x lanes per clock x the clock
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
    for _ in range(2):
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
    return f"{med:9.3f} ms (min {lo:.3f}, max {hi:.3f})"


def host_ms(fn, reps=3):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return out, (float(np.median(ts)), min(ts), max(ts))


def torch_iteration(y, update, gains, rows, cols, val, ex, mom, lr, chunk):
    """One iteration in torch ops: what a user of the parent commit would write on the device."""
    n = y.shape[0]
    R = torch.empty_like(y)
    Z = torch.zeros((), dtype=torch.float32, device=y.device)
    for r0 in range(0, n, chunk):
        r1 = min(r0 + chunk, n)
        d = y[r0:r1, None, :] - y[None, :, :]
        w = 1.0 / (1.0 + (d * d).sum(dim=2))
        i = torch.arange(r1 - r0, device=y.device)
        w[i, r0 + i] = 0.0
        Z += w.sum()
        R[r0:r1] = ((w * w).unsqueeze(2) * d).sum(dim=1)
    d = y[rows] - y[cols]
    w = val / (1.0 + (d * d).sum(dim=1))
    A = torch.zeros_like(y).index_add_(0, rows, w.unsqueeze(1) * d)
    g = 4.0 * (ex * A - R / Z)
    gains = torch.where(update * g < 0, gains + 0.2, gains * 0.8).clamp_(min=0.01)
    update = mom * update - lr * gains * g
    return y + update, update, gains


def one_size(m, n, reps):
    x, _ = T.synthetic_blobs(n, D, 10, 0.7, 0)
    xd = torch.from_numpy(x).to(m._device)
    say(f"N = {n}: {n * (n - 1) / 1e9:.3f} G pairs, {T.n_segments(n, int(_lib.load().keep_tsne_segment()))} segments")
    nb, t = host_ms(lambda: m.topk(xd, xd, K, normalize=False, exclude_self=True))
    say(f"  setup: topk (k = {K}, D = {D})         {fmt(t)}")
    p, t = host_ms(lambda: m.tsne_affinities(nb, PERPLEXITY))
    say(f"  setup: affinities                    {fmt(t)}")
    (graph, kept), t = host_ms(lambda: m.tsne_graph(nb, p))
    say(f"  setup: graph ({graph.nnz} entries)      {fmt(t)}")
    st = T.TsneState(torch.from_numpy(T.random_init(n, 0)).to(m._device))
    for _ in range(300):                                                   # off the 1e-4 start: a spread a descent spends its time at
        m._tsne_step(st, graph, 12.0, 0.5, T.check_learning_rate("auto", n, 12.0), torch.zeros(3, dtype=torch.int64, device=m._device), False, True)
    sums = torch.zeros(3, dtype=torch.int64, device=m._device)
    lr = T.check_learning_rate("auto", n, 12.0)

    def repulsion():
        m._call("tsne_repulsion", _ptr(st.y), n, _ptr(st.partials))

    def step(stats):
        def fn():
            sums.zero_()
            m._call("tsne_step", _ptr(st.y), n, _ptr(st.partials), _ptr(graph.row_ptr), _ptr(graph.col), _ptr(graph.val), graph.nnz, 1.0, 0.8, lr,
                    stats, _ptr(sums), _ptr(st.rz), _ptr(st.grad), _ptr(st.update), _ptr(st.gains), _ptr(st.spare))
        return fn

    def iteration():
        sums.zero_()
        m._tsne_step(st, graph, 1.0, 0.8, lr, sums, False, True)

    rows = torch.repeat_interleave(torch.arange(n, device=m._device), torch.diff(graph.row_ptr.long()))
    cols = graph.col.long()
    ty, tu, tg = st.y.clone(), st.update.clone(), st.gains.clone()
    chunk = max(256, min(4096, (1 << 27) // n))

    def torch_form():
        torch_iteration(ty, tu, tg, rows, cols, graph.val, 1.0, 0.8, lr, chunk)

    ts = event_ms([repulsion, step(0), step(1), iteration, torch_form], reps)
    pairs = n * (n - 1)
    say(f"  repulsion                            {fmt(ts[0])}  = {pairs / (ts[0][0] * 1e-3) / 1e12:.3f} T pairs/s; at {SLOTS_PER_PAIR} issue slots a pair "
        f"{100 * pairs * SLOTS_PER_PAIR / (ts[0][0] * 1e-3) / LANE_RATE:.1f} % of the fp32 vector issue rate")
    say(f"  step (reduce + update)               {fmt(ts[1])}")
    say(f"  step with the KL / gradient sums     {fmt(ts[2])}")
    say(f"  iteration (repulsion + step)         {fmt(ts[3])}")
    say(f"  torch form (row chunks of {chunk:4d})      {fmt(ts[4])}  ; the kernels' iteration / torch form = {ts[3][0] / ts[4][0]:.4f}")
    del rows, cols, ty, tu, tg, st
    emb, t = host_ms(lambda: m.tsne_fit(neighbours=nb, perplexity=PERPLEXITY, n_iter=1000, init="random"), reps=1)
    say(f"  tsne_fit, 1000 iterations (lists given) {fmt(t)}, host clock; {emb.n_iter} iterations, stop_reason {emb.stop_reason!r}, KL {emb.kl:.4f}")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="10000,100000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsne_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tsne_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    m = KEEPModel()
    m._create(dev)                                                         # the slide kernels need no weights
    say(f"tools/tsne_bench.py on {torch.cuda.get_device_name(0)}, {datetime.date.today().isoformat()}; KEEP_TSNE_SEGMENT = "
        f"{int(_lib.load().keep_tsne_segment())}; D = {D}, perplexity {PERPLEXITY:g}; device-event times, median of {a.reps} warm runs, the forms "
        f"alternating in one process")
    say()
    for n in (int(v) for v in a.sizes.split(",")):
        one_size(m, n, a.reps if n <= 20000 else max(5, a.reps // 4))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f_:
            f_.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
