#!/usr/bin/env python3
"""Few-shot prototypes, measured: KEEPModel.fewshot_classify at 100 000 test tiles x 768 on the shapes its users
bring, the sampler and the prototype builder at 16 shots, and a whole fewshot_episodes.  Device-event times, median of the warm runs
with the min-max spread; the new call and the yardsticks alternate inside one loop in one process, so a difference between them is not
a difference between runs.

  classify      keep_fewshot_classify with truth: the products, the per-episode epilogue and the confusion counts, one launch
  torch loop    what the parent commit offers on the device (the baseline, not the code under test): per episode, centre, normalise,
                x @ P.T, argmax and a bincount in torch; timed over at most 50 episodes and scaled to E, as the bootstrap bench does
  group_argmax  keep_group_argmax over the same bank cut into groups of C + 1 rows: the engine's existing fused product + argmax, which
                materialises its [N, E (C + 1)] logits; it cannot apply the per-episode epilogue, so this is the cost of the product and
                a plain argmax alone, with a torch bincount per episode on top

The binding peak is the 2 N E (C + 1) D FLOP of the products at the fp32 matrix rate (157 TFLOP/s); the padding columns of a tile
(64 - floor(64 / (C + 1)) (C + 1) of 64) are computed and not counted.

    python tools/fewshot_bench.py [--reps 5] [--out profiles/fewshot_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keep_amd import KEEPModel, _lib                                       # noqa: E402
from keep_amd.model import _ptr, _stream                                   # noqa: E402

F32_MATRIX_PEAK = 157.0e12
N, M, D, SHOTS = 100_000, 50_000, 768, 16
SHAPES = [(1000, 8, "the protocol: 1 000 episodes, 8 classes"), (1000, 2, "1 000 episodes, 2 classes"), (100, 32, "100 episodes, 32 classes"),
          (1, 8, "one fitted classifier applied to a slide")]
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
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ms[i].append(timed(fn))
    return [(float(np.median(m)), min(m), max(m)) for m in ms]


def fmt(t, scale=1.0):
    med, lo, hi = (v * scale for v in t)
    return f"{med:10.3f} ms (min {lo:.3f}, max {hi:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fewshot_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fewshot_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    m = KEEPModel()
    m._create(dev)                                                         # the slide kernels need no weights
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    g = torch.Generator(device="cpu").manual_seed(0)
    common = torch.nn.functional.normalize(torch.randn(1, D, generator=g), dim=1)
    test = torch.nn.functional.normalize(torch.randn(N, D, generator=g) / D ** 0.5 + common, dim=1).to(dev).contiguous()
    train = torch.nn.functional.normalize(torch.randn(M, D, generator=g) / D ** 0.5 + common, dim=1).to(dev).contiguous()
    say(f"tools/fewshot_bench.py on {torch.cuda.get_device_name(0)} ({cus} CUs); {N} test tiles and {M} training tiles x {D} fp32, unit rows "
        f"with a common mean; device-event times, median of {a.reps} warm runs, the forms alternating in one process")
    say()
    for E, C, use in SHAPES:
        ytr = (torch.arange(M) % C).numpy()
        truth = (torch.arange(N, device=dev) % C).to(torch.int32)
        sup = m.fewshot_sample(ytr, C, SHOTS, E, seed=1)
        protos = m.fewshot_prototypes(train, sup, normalize=False)
        ne = min(E, 50)
        bank, mu = protos.bank[:, :C], protos.bank[:, C]
        groups = protos.bank.reshape(E * (C + 1), D).contiguous()
        glabels = torch.empty((N, E), dtype=torch.int32, device=dev)
        t64 = truth.to(torch.int64)

        def new():
            return m.fewshot_classify(protos, test, truth, normalize=False)[0]

        def torch_loop():
            out = []
            for e in range(ne):
                q = torch.nn.functional.normalize(test - mu[e], dim=1)
                s = q @ bank[e].T - 0.5 * (bank[e] * bank[e]).sum(1)
                out.append(torch.bincount(t64 * C + s.argmax(1), minlength=C * C))
            return torch.stack(out).reshape(ne, C, C)

        def group_argmax():
            rc = _lib.load().keep_group_argmax(m._handle, _ptr(test), _ptr(groups), N, E, C + 1, D, _ptr(glabels), _stream(dev))
            _lib.check(m._handle, rc, "group_argmax")
            lab = glabels.to(torch.int64).clamp_(max=C - 1)
            return torch.stack([torch.bincount(t64 * C + lab[:, e], minlength=C * C) for e in range(min(E, 50))])

        t_new, t_loop, t_grp = event_ms([new, torch_loop, group_argmax], a.reps)
        conf, ref = new(), torch_loop()
        agree = float((conf[:ne] == ref).all(dim=(1, 2)).float().mean())
        diff = int((conf[:ne] - ref).abs().sum())
        sec = t_new[0] * 1e-3
        flops = 2.0 * N * E * (C + 1) * D
        ept = 64 // (C + 1)
        say(f"E = {E}, C = {C} ({use}): {E * (C + 1)} bank rows in {-(-E // ept)} tiles of {ept} episodes; {a.reps} repeats")
        say(f"  classify      {fmt(t_new)}   {flops / sec / 1e12:7.2f} TFLOP/s = {100 * flops / sec / F32_MATRIX_PEAK:5.1f} % of the f32 matrix rate")
        say(f"  torch loop    {fmt(t_loop, E / ne)}   ({ne} episodes timed, scaled to {E}); classify / torch loop = {t_new[0] / (t_loop[0] * E / ne):.4f}")
        say(f"  group_argmax  {fmt(t_grp)}   (its bincounts over {min(E, 50)} episodes only); classify / group_argmax = {t_new[0] / t_grp[0]:.4f}")
        say(f"  episodes whose confusion equals the torch loop's word for word: {100 * agree:.1f} % of {ne} (|difference| summed: {diff}; the torch "
            f"loop's sums have another order)")
        say()
    # the sampler, the builder and the whole protocol at the protocol's shape
    E, C = 1000, 8
    ytr = (torch.arange(M) % C).numpy()
    yte = (torch.arange(N) % C).numpy()
    sup = m.fewshot_sample(ytr, C, SHOTS, E, seed=1)
    t_s, t_p, t_all = event_ms([lambda: m.fewshot_sample(ytr, C, SHOTS, E, seed=1), lambda: m.fewshot_prototypes(train, sup, normalize=False),
                                lambda: m.fewshot_episodes(train, ytr, test, yte, C, SHOTS, E, seed=1)], a.reps)
    say(f"E = {E}, C = {C}, {SHOTS} shots:")
    say(f"  fewshot_sample      {fmt(t_s)}   (the host's stable sort of the labels and two uploads included)")
    say(f"  fewshot_prototypes  {fmt(t_p)}   (one workgroup per episode)")
    say(f"  fewshot_episodes    {fmt(t_all)}   (both feature sets normalised, sampled, built and classified)")
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
