#!/usr/bin/env python3
"""encode_region throughput: tiles/s of KEEPModel.encode_region on a synthetic slide region in HBM at
p = 224 and p = 256 (step = p), tissue rule off and on, against encode_image_uint8 on the same tiles pre-cut in HBM (the same
batches, so the difference is the grid + tissue pass, the per-batch cell check and the gather / resize).  Also times the front end
alone (region_grid + region_patches_uint8 of every batch) and checks that both paths give bit-identical features.

    python tools/region_bench.py [--rows 32] [--cols 32] [--batch 256] [--reps 3] [--precision comp] [--out FILE]
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
from keep_amd.region import TissueRule                                    # noqa: E402
from keep_amd.synth import synth_state_dict, synth_tile_family            # noqa: E402


def slide_region(rows, cols, dev):
    """[rows*224, cols*224, 3] uint8 on the device: a 'mixed' synthetic slide (he_crops, stain_field, background, half in turn)."""
    t = synth_tile_family("mixed", 0, rows * cols, dev, seed=4242)
    return t.reshape(rows, cols, 224, 224, 3).permute(0, 2, 1, 3, 4).reshape(rows * 224, cols * 224, 3).contiguous()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--cols", type=int, default=32)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precision", default="comp")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = synth_state_dict(KEEPShape(), seed=0)
    m = KEEPModel(KEEPShape(), precision=a.precision, towers=("image",))
    m.load_state_dict({k: v for k, v in sd.items() if k.startswith("visual") or k == "logit_scale"}, strict=True)
    m.to(dev).eval()
    region = slide_region(a.rows, a.cols, dev)
    rows = []
    for patch in (224, 256):
        for tissue in (None, TissueRule()):
            coords = m.region_grid(region, patch, None, tissue)
            n = int(coords.shape[0])
            tiles = torch.cat([m.region_patches_uint8(region, coords[i:i + a.batch], patch) for i in range(0, n, a.batch)])

            def pre_cut():
                return torch.cat([m.encode_image_uint8(tiles[i:i + a.batch]) for i in range(0, n, a.batch)])

            def front_end():
                c = m.region_grid(region, patch, None, tissue)
                return [m.region_patches_uint8(region, c[i:i + a.batch], patch) for i in range(0, n, a.batch)]

            t_reg, (f_reg, _) = timed(lambda: m.encode_region(region, patch, None, tissue, batch=a.batch), a.reps)
            t_pre, f_pre = timed(pre_cut, a.reps)
            t_fe, _ = timed(front_end, a.reps)
            row = {"patch": patch, "tissue": tissue is not None, "tiles": n, "encode_region_tiles_per_s": round(n / t_reg, 1),
                   "pre_cut_tiles_per_s": round(n / t_pre, 1), "overhead_pct": round(100 * (t_reg / t_pre - 1), 2),
                   "front_end_ms": round(t_fe * 1e3, 2), "bit_identical": bool(torch.equal(f_reg, f_pre))}
            rows.append(row)
            print(f"p={patch} tissue={'on ' if tissue else 'off'} {n:5d} tiles: encode_region {row['encode_region_tiles_per_s']:8.1f} tiles/s, "
                  f"pre-cut encode_image_uint8 {row['pre_cut_tiles_per_s']:8.1f} tiles/s ({row['overhead_pct']:+.2f} %), "
                  f"grid + gather alone {row['front_end_ms']:.2f} ms, bit-identical {row['bit_identical']}", flush=True)
    res = {"precision": a.precision, "region": list(region.shape), "batch": a.batch, "rows": rows}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
