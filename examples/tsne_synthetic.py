#!/usr/bin/env python3
"""The tile-embedding scatter plot on the device: exact t-SNE of frozen tile features, painted as a scatter
picture coloured by class and, back on the slide, as the embedding's geography over the tile grid.

    python examples/tsne_synthetic.py [--tiles 2000] [--dim 64] [--classes 5] [--out tsne_scatter.ppm]

No dataset or weights exist offline, so the features are seeded synthetic blobs (`keep_amd.tsne.synthetic_blobs`): a unit centre per
class plus noise, unit rows.  The numbers show the flow, not a model.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from keep_amd import KEEPModel, tsne, wsi                                           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=2000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("this example runs the t-SNE kernels: it needs the GPU")
    dev = torch.device("cuda:0")
    model = KEEPModel()
    model._create(dev)                                                   # the slide kernels need no encoder weights
    n, gw, patch, down = a.tiles, 50, 224, 16
    x, labels = tsne.synthetic_blobs(n, a.dim, a.classes, 0.7, seed=0)
    x[5, 0] = np.nan                                                     # a tile whose features did not survive: a NaN row of the embedding
    feats = torch.from_numpy(x).to(dev)

    emb = model.tsne_fit(feats, perplexity=20, n_iter=750, normalize=False)
    print(f"fit: {emb.n_kept} of {n} tiles, {emb.n_neighbors} neighbours, learning rate {emb.learning_rate:g}, {emb.n_iter} iterations "
          f"({emb.stop_reason}); KL {emb.kl:.4f}")
    print("KL at the checks:", ", ".join(f"{i + 1}: {v:.3f}" for i, v in zip(emb.kl_iter, emb.kl_trace)))
    kept = emb.kept.cpu().numpy()
    print(f"10-NN label purity of the embedding: {tsne.knn_purity(emb.embedding.cpu().numpy()[kept], labels[kept], 10):.4f}")

    scatter = wsi.tsne_scatter(emb, labels, a.classes, size=(512, 512), point=3, model=model)
    picture = model.render_class_map(model.class_map(scatter), thumbnail=None, alpha=1.0)       # uint8 [512, 512, 3] on the device
    painted = int((picture != 255).any(dim=2).sum())
    print(f"scatter picture {tuple(picture.shape)}: {scatter.tiles} points, {painted} pixels painted")

    coords = torch.stack([torch.arange(n) % gw * patch, torch.arange(n) // gw * patch], dim=1)
    shape = (((n + gw - 1) // gw) * patch // down, gw * patch // down)
    raster, _ = wsi.tsne_map(feats, coords, down, shape, patch_size=patch, model=model, perplexity=20, n_iter=750, normalize=False)
    rgb = model.render_rgb_map(raster, alpha=1.0)
    print(f"t-SNE map {shape[0]} x {shape[1]}: {raster.tiles} tiles; mean colour {[round(float(v), 1) for v in rgb.float().mean(dim=(0, 1))]}")
    if a.out:
        with open(a.out, "wb") as f:
            f.write(b"P6\n512 512\n255\n" + picture.cpu().numpy().tobytes())
        print("wrote", a.out)


if __name__ == "__main__":
    main()
