#!/usr/bin/env python3
"""A linear probe on frozen tile features: fit multinomial logistic regression on labelled tiles, score held-out
tiles with bootstrap intervals, and paint the probe's probabilities over a slide's tile grid.

    python examples/linear_probe_synthetic.py [--tiles 6000] [--classes 4] [--dim 768] [--l2 1e-3]

No dataset or weights exist offline, so the features are seeded synthetic data: class means with noise, made unit rows, the shape a
`cohort.extract_slide_features` file has, and the labels what `annotation_tile_labels` gives.  The numbers show the flow, not a model.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from keep_amd import KEEPModel, tile_eval, wsi                                     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=6000)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--l2", type=float, default=1e-3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("this example runs the probe kernels: it needs the GPU")
    dev = torch.device("cuda:0")
    model = KEEPModel()
    model._create(dev)                                                   # the slide kernels need no encoder weights
    g = torch.Generator().manual_seed(0)
    means = torch.randn(a.classes, a.dim, generator=g) * 0.06      # classes that overlap: a probe with something to get wrong
    y = torch.randint(0, a.classes, (a.tiles,), generator=g)
    x = (means[y] + torch.randn(a.tiles, a.dim, generator=g)).to(dev)
    y[::50] = -1                                                         # tiles nobody labelled: left out of the fit, still predicted
    half = a.tiles // 2
    names = tuple(f"class{c}" for c in range(a.classes))

    res = tile_eval.linear_probe(model, x[:half], y[:half], x[half:], y[half:], a.classes, l2=a.l2, class_weight="balanced", n_boot=1000)
    probe = res["probe"]
    print(f"fit: {probe.n_iter} iterations, {probe.n_eval} evaluations, {probe.stop_reason}; objective {probe.loss:.6f}, "
          f"|grad|inf {probe.grad_norm:.2e}; kept {probe.counts.cpu().tolist()} tiles per class, skipped {probe.skipped}")
    for key in ("balanced_accuracy", "weighted_f1"):
        lo, hi = res[key + "_ci"].ci(0.95)
        print(f"held-out {key}: {res[key]:.4f}  (95 % bootstrap interval {lo:.4f} .. {hi:.4f})")
    print(f"held-out macro one-vs-rest AUROC: {res['ovr_roc'][1].estimate:.4f}")

    # the same probe over a slide: a 60 x 50 grid of 224-pixel tiles at downsample 16
    gw, gh, patch, down = 60, 50, 224, 16
    n = gw * gh
    ys = torch.randint(0, a.classes, (n,), generator=g)
    feats = (means[ys] + torch.randn(n, a.dim, generator=g)).to(dev)
    coords = torch.stack([torch.arange(n) % gw * patch, torch.arange(n) // gw * patch], dim=1)
    raster = wsi.probe_map(probe, feats, coords, down, (gh * patch // down, gw * patch // down), patch_size=patch, classes=names, model=model)
    cmap = model.class_map(raster)
    areas = np.bincount(cmap.labels.cpu().numpy().ravel(), minlength=a.classes)[:a.classes]
    print(f"slide map: {raster.tiles} tiles rasterised; pixels per class {areas.tolist()} (tiles per class {np.bincount(ys.numpy(), minlength=a.classes).tolist()})")


if __name__ == "__main__":
    main()
