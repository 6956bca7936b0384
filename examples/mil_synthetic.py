#!/usr/bin/env python3
"""Attention MIL on frozen tile features: fit on slides that carry one label each, score held-out slides with
bootstrap intervals, and paint the learned attention over one slide's tile grid.

    python examples/mil_synthetic.py [--slides 96] [--dim 256] [--hidden 64] [--steps 200]

No dataset or weights exist offline, so the cohort is seeded synthetic data (`keep_amd.mil.synthetic_cohort`): every slide is a bag of
random unit rows, the shape a `cohort.extract_slide_features` file has; a positive slide also holds one to three tiles near one fixed
direction.  The numbers show the flow, not a model.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from keep_amd import KEEPModel, mil, tile_eval, wsi                                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slides", type=int, default=96)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("this example runs the MIL kernels: it needs the GPU")
    dev = torch.device("cuda:0")
    model = KEEPModel()
    model._create(dev)                                                   # the slide kernels need no encoder weights
    x, o, y, key = mil.synthetic_cohort(0, n_bags=a.slides, dim=a.dim, min_tiles=200, max_tiles=1200)
    xt, ot, yt, keyt = mil.synthetic_cohort(1, n_bags=a.slides // 2, dim=a.dim, min_tiles=200, max_tiles=1200)
    y = y.copy()
    y[::17] = -1                                                         # slides nobody labelled: left out of the fit

    res = tile_eval.attention_mil(model, (torch.from_numpy(x).to(dev), o), y, (torch.from_numpy(xt).to(dev), ot), yt, 2, hidden=a.hidden,
                                  class_weight="balanced", n_steps=a.steps, n_boot=1000)
    fit = res["mil"]
    print(f"fit: {len(y)} slides, {x.shape[0]} tiles; {fit.n_steps} Adam steps, objective {fit.loss_history[0]:.4f} -> {fit.loss:.4f}, "
          f"|grad|inf {fit.grad_norm:.2e}; kept {fit.counts.cpu().tolist()} slides per class, skipped {fit.skipped_bags}")
    for name in ("balanced_accuracy", "weighted_f1"):
        lo, hi = res[name + "_ci"].ci(0.95)
        print(f"held-out {name}: {res[name]:.4f}  (95 % bootstrap interval {lo:.4f} .. {hi:.4f})")
    print(f"held-out macro one-vs-rest AUROC: {res['ovr_roc'][1].estimate:.4f}")
    share = mil.key_share(res["attention"].cpu().numpy(), ot, yt, keyt)
    print(f"held-out positive slides whose most-attended tile is a key tile: {100 * share:.1f} %")

    # the attention of one positive held-out slide over its tile grid: 224-pixel tiles, 40 to a row, at downsample 16
    b = int(np.flatnonzero(yt == 1)[0])
    feats = torch.from_numpy(xt[ot[b]:ot[b + 1]]).to(dev)
    n, gw, patch, down = feats.shape[0], 40, 224, 16
    coords = torch.stack([torch.arange(n) % gw * patch, torch.arange(n) // gw * patch], dim=1)
    shape = (((n + gw - 1) // gw) * patch // down, gw * patch // down)
    raster = wsi.mil_attention_map(fit, feats, coords, down, shape, patch_size=patch, model=model)
    mean = raster.mean()
    hot = int((mean > 0.5).sum()) // (patch // down) ** 2
    print(f"slide {b}: {raster.tiles} tiles rasterised on {shape[0]} x {shape[1]} pixels; {hot} tile(s) above half the largest attention "
          f"({int(keyt[ot[b]:ot[b + 1]].sum())} key tiles in the slide)")


if __name__ == "__main__":
    main()
