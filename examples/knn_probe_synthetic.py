#!/usr/bin/env python3
"""A kNN probe on frozen tile features, the linear probe's non-parametric twin: every held-out tile's 20 nearest
labelled tiles vote for its class; then the same bank paints a slide's tile grid, and a search lists the tiles most like one example.

    python examples/knn_probe_synthetic.py [--tiles 6000] [--classes 4] [--dim 768] [--k 20]

No dataset or weights exist offline, so the features are seeded synthetic data: class means with noise, the shape a
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
    ap.add_argument("--k", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("this example runs the neighbour kernels: it needs the GPU")
    dev = torch.device("cuda:0")
    model = KEEPModel()
    model._create(dev)                                                   # the slide kernels need no encoder weights
    g = torch.Generator().manual_seed(0)
    means = torch.randn(a.classes, a.dim, generator=g) * 0.06      # classes that overlap: a probe with something to get wrong
    y = torch.randint(0, a.classes, (a.tiles,), generator=g)
    x = (means[y] + torch.randn(a.tiles, a.dim, generator=g)).to(dev)
    y[::50] = -1                                                         # tiles nobody labelled: they take no neighbour slot
    half = a.tiles // 2
    names = tuple(f"class{c}" for c in range(a.classes))

    for weights in ("uniform", "softmax"):
        res = tile_eval.knn_probe(model, x[:half], y[:half], x[half:], y[half:], a.classes, k=a.k, weights=weights, n_boot=1000)
        print(f"k = {a.k}, {weights} votes: bank of {res['neighbours'].n_bank} labelled tiles, {res['skipped']} test tiles without a label")
        for key in ("balanced_accuracy", "weighted_f1"):
            lo, hi = res[key + "_ci"].ci(0.95)
            print(f"  held-out {key}: {res[key]:.4f}  (95 % bootstrap interval {lo:.4f} .. {hi:.4f})")
        print(f"  held-out macro one-vs-rest AUROC of the vote shares: {res['ovr_roc'][1].estimate:.4f}")

    # the same bank over a slide: a 60 x 50 grid of 224-pixel tiles at downsample 16
    gw, gh, patch, down = 60, 50, 224, 16
    n = gw * gh
    ys = torch.randint(0, a.classes, (n,), generator=g)
    feats = (means[ys] + torch.randn(n, a.dim, generator=g)).to(dev)
    coords = torch.stack([torch.arange(n) % gw * patch, torch.arange(n) // gw * patch], dim=1)
    raster = wsi.knn_map(x[:half], y[:half], a.classes, feats, coords, down, (gh * patch // down, gw * patch // down), patch_size=patch, k=a.k,
                         classes=names, model=model)
    cmap = model.class_map(raster)
    areas = np.bincount(cmap.labels.cpu().numpy().ravel(), minlength=a.classes)[:a.classes]
    print(f"slide map: {raster.tiles} tiles rasterised; pixels per class {areas.tolist()} (tiles per class {np.bincount(ys.numpy(), minlength=a.classes).tolist()})")

    # tile search: the 10 tiles of the slide most like tile 0, itself left out, and the slide's neighbour graph
    index, score, found = wsi.search_tiles(feats[:1], feats, 10, tile_coords=coords, model=model)
    print(f"tiles most like tile 0 (class {int(ys[0])}): {index[0, 1:].tolist()} at cosine {[round(float(s), 3) for s in score[0, 1:]]}, "
          f"classes {ys[index[0, 1:].cpu()].tolist()}, first at {found[0, 1].tolist()}")
    graph = model.topk(feats, feats, a.k, exclude_self=True)
    agree = float((ys.to(dev)[graph.index] == ys.to(dev)[:, None]).float().mean())
    print(f"neighbour graph: {n} x {a.k} edges, {100 * agree:.1f} % join tiles of one class")


if __name__ == "__main__":
    main()
