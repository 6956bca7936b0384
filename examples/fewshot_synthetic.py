#!/usr/bin/env python3
"""The few-shot prototype protocol on frozen tile features: SimpleShot with centring and L2 normalisation over
many random support sets per shot count, the median and quartiles over the episodes; then one fitted set of prototypes paints a slide's
tile grid and makes the slide-level call.

    python examples/fewshot_synthetic.py [--tiles 6000] [--classes 4] [--dim 768] [--episodes 200]

No dataset or weights exist offline, so the features are seeded synthetic data: class means with noise around a large common mean, the
shape a `cohort.extract_slide_features` file has.  The numbers show the flow, not a model.
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
    ap.add_argument("--episodes", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("this example runs the few-shot kernels: it needs the GPU")
    dev = torch.device("cuda:0")
    model = KEEPModel()
    model._create(dev)                                                   # the slide kernels need no encoder weights
    g = torch.Generator().manual_seed(0)
    common = torch.randn(1, a.dim, generator=g) * 0.2                    # what every tile shares: centring takes it out
    means = torch.randn(a.classes, a.dim, generator=g) * 0.06 + common
    y = torch.randint(0, a.classes, (a.tiles,), generator=g)
    x = (means[y] + torch.randn(a.tiles, a.dim, generator=g)).to(dev)
    y[::50] = -1                                                         # tiles nobody labelled: never sampled, in no count
    half = a.tiles // 2

    res = tile_eval.few_shot(model, x[:half], y[:half], x[half:], y[half:], a.classes, shots=(1, 2, 4, 8, 16, 32), n_episodes=a.episodes)
    print(f"{a.episodes} episodes per shot count, {a.classes} classes, {int((y[half:] >= 0).sum())} labelled test tiles")
    for k, r in res.items():
        print(f"  {k:2d} shots: balanced accuracy median {r['balanced_accuracy_median']:.4f} (Q1 {r['balanced_accuracy_q1']:.4f}, Q3 "
              f"{r['balanced_accuracy_q3']:.4f}), weighted F1 median {r['weighted_f1_median']:.4f}")

    # every labelled tile as support: the nearest-centroid classifier, applied to a 60 x 50 grid of 224-pixel tiles at downsample 16
    protos = model.fewshot_fit(x[:half], y[:half], a.classes)
    labels, scores, margin, skipped = model.fewshot_predict(protos, x[half:])
    on = (y[half:] >= 0).to(dev)
    acc = float((labels[on].cpu() == y[half:][on.cpu()]).float().mean())
    print(f"all {int((y[:half] >= 0).sum())} labelled tiles as support: held-out accuracy {acc:.4f}, median margin {float(margin.median()):.4f}")
    gw, gh, patch, down = 60, 50, 224, 16
    n = gw * gh
    ys = torch.randint(0, a.classes, (n,), generator=g)
    feats = (means[ys] + torch.randn(n, a.dim, generator=g)).to(dev)
    coords = torch.stack([torch.arange(n) % gw * patch, torch.arange(n) // gw * patch], dim=1)
    raster = wsi.prototype_map(protos, feats, coords, down, (gh * patch // down, gw * patch // down), patch_size=patch,
                               classes=tuple(f"class{c}" for c in range(a.classes)), model=model)
    cmap = model.class_map(raster)
    areas = np.bincount(cmap.labels.cpu().numpy().ravel(), minlength=a.classes)[:a.classes]
    print(f"slide map: {raster.tiles} tiles rasterised; pixels per class {areas.tolist()} (tiles per class {np.bincount(ys.numpy(), minlength=a.classes).tolist()})")
    label, pooled = wsi.prototype_slide_call(protos, feats, top=50, model=model)
    print(f"slide call from the 50 best tiles per class: class {label}, pooled scores {[round(float(v), 4) for v in pooled]}")


if __name__ == "__main__":
    main()
