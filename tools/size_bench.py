#!/usr/bin/env python3
"""encode_image throughput by tile size (dynamic_img_size): ms/step, tiles/s and TFLOP/s at a fixed token budget per step, plus the
attention kernels' share of the step from the profile tags (a separate, profiled pass: event scopes around every phase, no graphs).

Per tile, FLOPs = depth (2 T (4 D^2 + 2 D F) + 4 T^2 D) + 2 (T - 1) 768 D   (D = 1024, F = 4096, depth = 24, T = (H/16)(W/16) + 1):
the blocks at T tokens plus the patch embedding; the head and the skipped rows of the CLS-only last block are not subtracted.

    python tools/size_bench.py [--sizes 224,256,384,512] [--budget-tiles 256] [--steps 20] [--warmup 5] [--precision comp]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keep_amd import KEEPModel                                            # noqa: E402
from keep_amd.config import KEEPShape                                     # noqa: E402
from keep_amd.synth import synth_state_dict                               # noqa: E402

D, F, DEPTH = 1024, 4096, 24
VIT_TAGS = ("vit.im2col", "vit.patch", "vit.ln", "vit.qkv", "vit.attn", "vit.proj", "vit.fc1", "vit.fc2", "vit.head",
            "vit.qkv.x", "vit.attn.x", "vit.proj.x", "vit.fc1.x", "vit.fc2.x", "vit.tail")


def tile_flops(H, W):
    T = (H // 16) * (W // 16) + 1
    return DEPTH * (2 * T * (4 * D * D + 2 * D * F) + 4 * T * T * D) + 2 * (T - 1) * 768 * D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="224,256,384,512")
    ap.add_argument("--budget-tiles", type=int, default=256, help="tokens per step = this many 224 x 224 tiles (197 tokens each)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="comp")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = synth_state_dict(KEEPShape(), seed=0)
    m = KEEPModel(KEEPShape(), precision=a.precision, towers=("image",), dynamic_img_size=True)
    m.load_state_dict({k: v for k, v in sd.items() if k.startswith("visual") or k == "logit_scale"}, strict=True)
    m.to(dev).eval()
    budget = a.budget_tiles * 197
    rows = []
    for s in (int(x) for x in a.sizes.split(",")):
        T = (s // 16) ** 2 + 1
        n = max(budget // T, 1)
        g = torch.Generator(device=dev).manual_seed(s)
        x = torch.randn(n, 3, s, s, device=dev, generator=g).to(torch.bfloat16)
        for _ in range(a.warmup):
            m.encode_image(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            m.encode_image(x)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / a.steps * 1e3
        # attention share: one profiled step (all tags), after one profiled warm-up
        m.profile_enable()
        m.encode_image(x)
        torch.cuda.synchronize()
        m.profile_reset()
        m.encode_image(x)
        torch.cuda.synchronize()
        tag_ms = {t: m.profile_read(t)[0] for t in VIT_TAGS}
        m.profile_disable()
        m.profile_reset()
        total = sum(tag_ms.values())
        attn = tag_ms["vit.attn"] + tag_ms["vit.attn.x"]
        row = {"size": s, "tokens": T, "tiles_per_step": n, "ms_per_step": round(ms, 3), "tiles_per_s": round(n / ms * 1e3, 1),
               "tflops": round(n * tile_flops(s, s) / (ms * 1e-3) / 1e12, 1), "attn_share": round(attn / total, 3) if total else None}
        rows.append(row)
        print(f"{s}x{s}: T={T:5d} {n:4d} tiles/step  {ms:8.2f} ms/step  {row['tiles_per_s']:8.1f} tiles/s  {row['tflops']:6.1f} TFLOP/s  "
              f"attention {100 * (row['attn_share'] or 0):5.1f} % of the profiled step", flush=True)
    res = {"precision": a.precision, "plan": [list(p) for p in m.get_plan()], "token_budget": budget, "rows": rows}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
