#!/usr/bin/env python3
"""Attention MIL, measured: N = 100 000 unit feature rows of D = 768 in 1, 10 and 1 000 bags, L = 64 and 128
hidden units, C = 2.  Device-event times, median of >= 20 warm runs with the min-max spread; the forms alternate inside one loop in one
process, so a difference between them is not a difference between runs:

  loss + gradient   one evaluation as KEEPModel.mil_fit makes it: keep_mil_forward, the head (keep_probe_loss_grad on the pooled rows)
                    and keep_mil_backward, each with its 4-byte check read-back, into zeroed accumulators
  forward alone     keep_mil_forward writing scores, attention and pooled rows (and the hidden units the backward reads)
  backward alone    keep_mil_backward: dz and u, ds, and the V-gradient launch
  V gradient        the mil_gradv_kernel launches alone, from the kernel records of torch.profiler (n/a where it records none), with
                    the 64-bit atomic adds counted from the launch geometry: one word per (chunk, hidden unit, column)
  torch forms       what the parent commit offers on the device (the baseline, not the code under test): x @ V.T, tanh, a segment
                    softmax with scatter_reduce / index_add_, the head, and R.T @ x, in fp32
  fit               a whole KEEPModel.mil_fit of 20 Adam steps (host clock around it, the device synchronised), and the same Adam
                    driven by the torch forms

The chunk length is the library's (keep_mil_chunk): a library built with another KEEP_MIL_CHUNK, loaded through KEEP_HIP_LIB, gives the
times of that value.

    python tools/mil_bench.py [--reps 20] [--out profiles/mil_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keep_amd import KEEPModel, _lib, mil as M                             # noqa: E402
from keep_amd.slide import _ptr                                            # noqa: E402

N, D, C = 100_000, 768, 2
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


def gradv_kernel_ms(fn, runs=7):
    """The median device time of one evaluation's mil_gradv_kernel launches, from torch.profiler's kernel records; None without any."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(runs):
                fn()
            torch.cuda.synchronize()
        us = [e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total for e in prof.events() if "mil_gradv" in e.name]
        return float(np.median(us)) / 1e3 if us else None
    except Exception as e:                                                 # noqa: BLE001 -- a measurement aid: its absence is reported, not fatal
        say(f"  (torch.profiler gave no kernel records: {type(e).__name__})")
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mil_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mil_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    m = KEEPModel()
    m._create(dev)                                                         # the slide kernels need no weights
    chunk = int(_lib.load().keep_mil_chunk())
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1).to(dev).contiguous()
    say(f"tools/mil_bench.py on {torch.cuda.get_device_name(0)}; KEEP_MIL_CHUNK = {chunk}; N = {N}, D = {D} fp32 ({N * D * 4 / 1e6:.0f} MB of "
        f"features), C = {C}; device-event times, median of {a.reps} warm runs, the forms alternating in one process")
    say()
    for S in (1, 10, 1000):
        o = np.linspace(0, N, S + 1).astype(np.int64)
        y = torch.arange(S, dtype=torch.int32) % C
        bags = m._mil_bags(x, o, False)
        chunks = bags[2]
        yd, y64 = y.to(dev), y.to(dev, torch.int64)
        bag = torch.repeat_interleave(torch.arange(S, device=dev), torch.from_numpy(np.diff(o)).to(dev))
        onehot = torch.nn.functional.one_hot(y64, C).to(torch.float32)
        for L in (64, 128):
            p64 = M.init_params(1, L, C, D)
            p64 = (p64[0] * 3.0, p64[1], p64[2] * 4.0, np.random.default_rng(2).standard_normal((C, D)) * 0.05, p64[4])
            dp = tuple(torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(dev) for q in p64)
            V, bv, w, Wc, bc = dp
            sums = M.MilSums(L, C, D, dev)
            f = m._mil_forward(bags, yd, dp, L, True, sums.skipped_rows, sums.skipped_bags)
            probs = torch.full((S, C), 1.0 / C, device=dev)
            ws = bags[3]

            def evaluate():
                sums.zero_()
                m._mil_eval(bags, yd, dp, L, C, None, sums)

            def forward():
                m._mil_forward(bags, yd, dp, L, True, sums.skipped_rows, sums.skipped_bags)

            def backward():
                m._call("mil_backward", _ptr(x), N, D, _ptr(chunks), chunks.shape[0], S, _ptr(f["head_labels"]), _ptr(probs), _ptr(Wc), C, _ptr(None),
                        _ptr(w), L, _ptr(f["scores"]), _ptr(f["attention"]), _ptr(f["pooled"]), _ptr(f["hidden"]), _ptr(sums.gV), _ptr(sums.gbv),
                        _ptr(sums.gw), _ptr(None), _ptr(ws), ws.numel())

            def torch_forward(V_=V, bv_=bv, w_=w, Wc_=Wc, bc_=bc):
                h = torch.tanh(x @ V_.T + bv_)
                s = h @ w_
                mx = torch.full((S,), float("-inf"), device=dev).scatter_reduce(0, bag, s, "amax")
                e = torch.exp(s - mx[bag])
                att = e / torch.zeros(S, device=dev).index_add_(0, bag, e)[bag]
                z = torch.zeros((S, D), device=dev).index_add_(0, bag, att[:, None] * x)
                return h, att, z, z @ Wc_.T + bc_

            def torch_form(V_=V, bv_=bv, w_=w, Wc_=Wc, bc_=bc):
                h, att, z, logits = torch_forward(V_, bv_, w_, Wc_, bc_)
                loss = (torch.logsumexp(logits, dim=1) - logits.gather(1, y64[:, None])[:, 0]).mean()
                r = (torch.softmax(logits, dim=1) - onehot) / S
                dz = r @ Wc_
                ds = att * ((dz[bag] * x).sum(dim=1) - (dz * z).sum(dim=1)[bag])
                R = ds[:, None] * w_ * (1.0 - h * h)
                return loss, (R.T @ x, R.sum(dim=0), (ds[:, None] * h).sum(dim=0), r.T @ z, r.sum(dim=0))

            def torch_gradv():
                return R0.T @ x

            R0 = torch.randn(N, L, device=dev) * 1e-3
            ts = event_ms([evaluate, forward, backward, torch_form, torch_forward, torch_gradv], a.reps)
            t_eval, t_fwd, t_bwd, t_torch, t_tfwd, t_tgv = ts
            n_chunks = int(chunks.shape[0])
            atomic_bytes = n_chunks * L * D * 8
            say(f"S = {S} bags, L = {L}: {n_chunks} chunks -> {atomic_bytes / 1e6:.1f} MB of 64-bit atomic adds for the V gradient")
            say(f"  loss + gradient             {fmt(t_eval)}  / torch form {fmt(t_torch)} = {t_eval[0] / t_torch[0]:.3f}")
            say(f"  forward alone               {fmt(t_fwd)}  / torch form {fmt(t_tfwd)} = {t_fwd[0] / t_tfwd[0]:.3f}")
            say(f"  backward alone              {fmt(t_bwd)}")
            gv = gradv_kernel_ms(backward)
            if gv is None:
                say(f"  V gradient launch           n/a (no kernel records)         torch R.T @ x {fmt(t_tgv)}")
            else:
                say(f"  V gradient launch           {gv:8.3f} ms (kernel records)   / torch R.T @ x {fmt(t_tgv)} = {gv / t_tgv[0]:.3f}; "
                    f"{atomic_bytes / (gv * 1e-3) / 1e9:.1f} GB/s of added bytes, {2.0 * N * L * D / (gv * 1e-3) / 1e12:.1f} TFLOP/s")
            if L == 128:
                steps = 20

                def fit_engine():
                    return m._mil_fit(lambda: ((bags, yd),), L, C, D, 1e-4, np.ones(C, np.float32), 0.01, steps, 0, None, None)

                def fit_torch():
                    def fun(theta):
                        q = tuple(torch.from_numpy(np.ascontiguousarray(t, np.float32)).to(dev) for t in M.unpack(theta, L, C, D))
                        loss, grads = torch_form(*q)
                        pen = np.concatenate([t if k in (0, 2, 3) else 0.0 * t for k, t in enumerate(M.unpack(theta, L, C, D))], axis=None)
                        return (float(loss) + 0.5e-4 * float(pen @ pen),
                                np.concatenate([t.double().cpu().numpy().ravel() for t in grads]) + 1e-4 * pen)
                    return M.adam(fun, M.pack(M.init_params(0, L, C, D)), 0.01, steps)

                fit_engine(), fit_torch()
                torch.cuda.synchronize()
                te, tt = [], []
                for _ in range(3):
                    t0 = time.perf_counter(); fe = fit_engine(); torch.cuda.synchronize(); te.append(time.perf_counter() - t0)
                    t0 = time.perf_counter(); ft = fit_torch(); torch.cuda.synchronize(); tt.append(time.perf_counter() - t0)
                say(f"  mil_fit, {steps} Adam steps        {1e3 * np.median(te):8.1f} ms = {1e3 * np.median(te) / (steps + 1):.3f} ms per evaluation with its "
                    f"transfers; loss {fe.loss_history[0]:.4f} -> {fe.loss:.4f}")
                say(f"  the same Adam, torch forms   {1e3 * np.median(tt):8.1f} ms; loss {ft.history[0]:.4f} -> {ft.f:.4f}")
            say()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f_:
            f_.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
