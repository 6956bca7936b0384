#!/usr/bin/env python3
"""The linear probe, measured: N = 100 000 unit feature rows of D = 768 against C = 2, 8 and 64 classes.
Device-event times, median of >= 20 warm runs with the min-max spread; the forms alternate inside one loop in one process, so a
difference between them is not a difference between runs:

  loss + gradient   keep_probe_loss_grad: the label check (one launch, a 4-byte read-back), then softmax, residuals and the integer sums
                    in one pass over the features; also with each rows-per-workgroup choice the launcher can be given
  forward alone     keep_probe_forward writing labels, probabilities and margins
  torch form        what the parent commit offers on the device (the baseline, not the code under test): x @ W.T + b, softmax,
                    the mean loss and (p - onehot).T @ x in fp32
  fit               a whole KEEPModel.probe_fit (host clock around it, the device synchronised), and the same L-BFGS driven by the
                    torch form

Bytes: an evaluation reads N D 4 B of features from HBM once (the class chunks' re-reads come from L2), against the 8 TB/s figure; the
gradient adds one 64-bit word per (workgroup, class, column), counted here from the launch geometry.

    python tools/probe_bench.py [--reps 20] [--out profiles/probe_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keep_amd import KEEPModel, probe as P                                 # noqa: E402
from keep_amd.slide import _ptr                                            # noqa: E402

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


def groups_chosen(n, c):
    """probe_groups of probe.hip for a gradient launch."""
    return 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("probe_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    m = KEEPModel()
    m._create(dev)                                                         # the slide kernels need no weights
    g = torch.Generator(device="cpu").manual_seed(0)
    say(f"tools/probe_bench.py on {torch.cuda.get_device_name(0)}; N = {N}, D = {D} fp32 ({N * D * 4 / 1e6:.0f} MB of features); "
        f"device-event times, median of {a.reps} warm runs, the forms alternating in one process")
    say()
    for C in (2, 8, 64):
        means = torch.randn(C, D, generator=g) * 0.3
        y = torch.randint(0, C, (N,), generator=g)
        x = torch.nn.functional.normalize(means[y] + torch.randn(N, D, generator=g), dim=1).to(dev).contiguous()
        y32, y64 = y.to(dev, torch.int32), y.to(dev)
        w = (torch.randn(C, D, generator=g) * 0.05).to(dev)
        b = (torch.randn(C, generator=g) * 0.1).to(dev)
        sums = P.ProbeSums(C, D, dev)
        labels = torch.empty(N, dtype=torch.int32, device=dev)
        probs = torch.empty((N, C), dtype=torch.float32, device=dev)
        margin = torch.empty(N, dtype=torch.float32, device=dev)
        onehot = torch.nn.functional.one_hot(y64, C).to(torch.float32)

        def grad(groups=0):
            sums.zero_()
            m._call("probe_loss_grad", _ptr(x), N, D, _ptr(y32), _ptr(w), _ptr(b), C, _ptr(None), _ptr(sums.grad), _ptr(sums.gbias), _ptr(sums.loss),
                    _ptr(sums.counts), _ptr(sums.skipped), _ptr(None), _ptr(None), _ptr(None), _ptr(None), groups)

        def forward():
            m._call("probe_forward", _ptr(x), N, D, _ptr(w), _ptr(b), C, _ptr(probs), _ptr(labels), _ptr(None), _ptr(margin), _ptr(None), 0)

        def torch_form(w_=w, b_=b):
            z = x @ w_.T + b_
            p = torch.softmax(z, dim=1)
            loss = (torch.logsumexp(z, dim=1) - z.gather(1, y64[:, None])[:, 0]).mean()
            r = p - onehot
            return loss, r.T @ x / N, r.mean(dim=0)

        allowed = [G for G in (1, 2, 4) if G * ((C + 15) // 16) <= 8]
        ts = event_ms([grad, forward, torch_form] + [lambda G=G: grad(G) for G in allowed], a.reps)
        t_grad, t_fwd, t_torch, t_groups = ts[0], ts[1], ts[2], ts[3:]
        G = groups_chosen(N, C)
        blocks = (N + 64 * G - 1) // (64 * G)
        atomic_bytes = blocks * C * D * 8
        t_acc = max(t_grad[0] - t_fwd[0], 1e-6)
        say(f"C = {C}: {blocks} workgroups of {64 * G} rows -> {atomic_bytes / 1e6:.1f} MB of 64-bit atomic adds for the gradient")
        say(f"  loss + gradient             {fmt(t_grad)}  {N * D * 4 / (t_grad[0] * 1e-3) / 1e12:6.2f} TB/s of features = "
            f"{100 * N * D * 4 / (t_grad[0] * 1e-3) / HBM_PEAK:.1f} % of the 8 TB/s HBM peak")
        for G_, t in zip(allowed, t_groups):
            say(f"    with {64 * G_:3d} rows per workgroup {fmt(t)}")
        say(f"  forward alone               {fmt(t_fwd)}  {N * D * 4 / (t_fwd[0] * 1e-3) / 1e12:6.2f} TB/s of features = "
            f"{100 * N * D * 4 / (t_fwd[0] * 1e-3) / HBM_PEAK:.1f} % of the HBM peak")
        say(f"  gradient (call - forward)   {t_acc:8.3f} ms                          {atomic_bytes / (t_acc * 1e-3) / 1e9:8.1f} GB/s of added bytes")
        say(f"  torch form (the baseline)   {fmt(t_torch)}  loss + gradient / torch form = {t_grad[0] / t_torch[0]:.3f}")

        # a whole fit, and the same optimiser over the torch form
        def fit_engine():
            return m.probe_fit(x, y32, C, l2=1e-3)

        def fit_torch():
            def fun(theta):
                w_ = torch.from_numpy(theta[:C * D].reshape(C, D).astype(np.float32)).to(dev)
                b_ = torch.from_numpy(theta[C * D:].astype(np.float32)).to(dev)
                loss, gw, gb = torch_form(w_, b_)
                w64 = theta[:C * D]
                f = float(loss) + 0.5e-3 * float(w64 @ w64)
                return f, np.concatenate([gw.double().cpu().numpy().ravel() + 1e-3 * w64, gb.double().cpu().numpy()])
            return P.lbfgs(fun, np.zeros(C * D + C), 1e-4, 1000, noise=lambda th: P.loss_noise(th[:C * D].reshape(C, D), th[C * D:]))

        fit_engine(), fit_torch()
        torch.cuda.synchronize()
        te, tt = [], []
        for _ in range(3):
            t0 = time.perf_counter(); pe = fit_engine(); torch.cuda.synchronize(); te.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); pt = fit_torch(); torch.cuda.synchronize(); tt.append(time.perf_counter() - t0)
        say(f"  probe_fit (l2 1e-3, gtol 1e-4) {1e3 * np.median(te):8.1f} ms: {pe.n_iter} iterations, {pe.n_eval} evaluations, {pe.stop_reason}, "
            f"|grad|inf {pe.grad_norm:.3g} -> {1e3 * np.median(te) / pe.n_eval:.3f} ms per evaluation with its transfers")
        say(f"  the same L-BFGS, torch form    {1e3 * np.median(tt):8.1f} ms: {pt.n_iter} iterations, {pt.n_eval} evaluations, {pt.stop_reason}")
        say()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
