#!/usr/bin/env python3
"""Does the calibrated 'comp' plan hold the 1e-4 cosine tolerance at tile sizes other than 224 x 224?

`KEEPModel.calibrate()` picks the per-block plan on 224 x 224 tiles (197 tokens).  This tool runs the bench weights, calibrated exactly as
`load_state_dict` leaves them, with dynamic_img_size and option grid_plan = 2 (the plan as calibrated, at every grid) against 'strict'
on `--tiles` tiles per family at each `--sizes` entry, and reports the worst |dcos| against 64 unit prompts per size and family.  Tiles of
size S are built from the 224 x 224 family tiles of keep_amd.synth: a 2 x 2 mosaic of four tiles, resized (bicubic, antialiased) to S x S.
The engine's rule (grid_plan = 1: the plan for 197..1025 tokens, 'strict' outside) follows from these numbers: DESIGN.md, "Other tile sizes".

    python tools/grid_precision.py [--tiles 2000] [--sizes 224,256,384,512] [--out grid_precision.json]
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from keep_amd import KEEPModel                                            # noqa: E402
from keep_amd.config import KEEPShape                                     # noqa: E402
from keep_amd.synth import normalise_u8, synth_state_dict, synth_tile_family   # noqa: E402

FAMILIES = ("he_crops", "stain_field", "background", "half")


def sized_tiles(family, a, b, size, dev, seed=7001):
    t = synth_tile_family(family, 4 * a, 4 * b, dev, seed=seed).permute(0, 3, 1, 2).float()
    n = b - a
    t = t.view(n, 4, 3, 224, 224)
    mosaic = torch.cat([torch.cat([t[:, 0], t[:, 1]], 3), torch.cat([t[:, 2], t[:, 3]], 3)], 2)
    if size != 448:
        mosaic = F.interpolate(mosaic, size=(size, size), mode="bicubic", antialias=True, align_corners=False)
    return mosaic.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=2000)
    ap.add_argument("--sizes", default="224,256,384,512")
    ap.add_argument("--chunk", type=int, default=250)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = synth_state_dict(KEEPShape(), seed=0)
    m = KEEPModel(KEEPShape(), dynamic_img_size=True, towers=("image",))
    m.load_state_dict({k: v for k, v in sd.items() if k.startswith("visual") or k == "logit_scale"}, strict=True)
    m.to(dev).eval()
    m.set_option("grid_plan", 2)
    plan = m.get_plan()
    bank = F.normalize(torch.randn(64, 768, generator=torch.Generator().manual_seed(99)), dim=-1).to(dev)
    res = {"tiles_per_family": a.tiles, "plan": [list(p) for p in plan], "worst_abs_dcos": {}}
    for size in (int(s) for s in a.sizes.split(",")):
        row = {}
        t0 = time.time()
        for fam in FAMILIES:
            worst = 0.0
            for lo in range(0, a.tiles, a.chunk):
                hi = min(lo + a.chunk, a.tiles)
                x = normalise_u8(sized_tiles(fam, lo, hi, size, dev))
                m.set_precision("comp")                               # (the precision switch leaves the calibrated plan as it is)
                fc = m.encode_image(x)
                m.set_precision("strict")
                fs = m.encode_image(x)
                worst = max(worst, (fc @ bank.t() - fs @ bank.t()).abs().max().item())
            row[fam] = worst
            print(f"{size}x{size} {fam:12s} worst |dcos| comp vs strict = {worst:.3e}", flush=True)
        row["seconds"] = round(time.time() - t0, 1)
        res["worst_abs_dcos"][f"{size}x{size}"] = row
    res["plan_unchanged"] = m.get_plan() == plan
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
