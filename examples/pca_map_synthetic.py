#!/usr/bin/env python3
"""Feature PCA on frozen tile features: the spectrum of a slide's features, a whitened 8-column projection,
and the PCA colour map -- the first three components as red, green and blue over the tile grid.

    python examples/pca_map_synthetic.py [--tiles 4000] [--dim 256] [--out pca_map.ppm]

No dataset or weights exist offline, so the features are seeded synthetic data (`keep_amd.pca.synthetic_features`): unit rows with a
common mean direction and six planted directions of falling variance, the first of them tied to the tile's position so that the map
shows structure.  The numbers show the flow, not a model.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from keep_amd import KEEPModel, pca, wsi                                           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=4000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("this example runs the PCA kernels: it needs the GPU")
    dev = torch.device("cuda:0")
    model = KEEPModel()
    model._create(dev)                                                   # the slide kernels need no encoder weights
    n, gw, patch, down = a.tiles, 80, 224, 16
    x = pca.synthetic_features(n, a.dim, seed=0)
    order = np.argsort(pca.fit_numpy(x, 1).components[0].astype(np.float64) @ x.T.astype(np.float64))
    x = x[order]                                                         # the first component now runs down the slide
    x[5, 0] = np.nan                                                     # a tile whose features did not survive: skipped everywhere
    feats = torch.from_numpy(x).to(dev)

    fit = model.pca_fit(feats, 8)
    print(f"fit: {fit.n_rows} tiles kept, {fit.skipped} skipped; total variance {fit.total_variance:.5f}")
    print("explained variance ratio of the first 8 components:", np.round(fit.explained_variance_ratio, 4).tolist())
    one = model.pca_fit(feats, 8, two_pass=False)
    print(f"one pass about a zero centre: largest eigenvalue difference {np.abs(one.explained_variance - fit.explained_variance).max():.2e}")
    white, kept = model.pca_transform(fit, feats, whiten=True)
    print(f"whitened scores {tuple(white.shape)}: variances {np.round(white[kept].var(dim=0).cpu().numpy(), 4).tolist()}")

    coords = torch.stack([torch.arange(n) % gw * patch, torch.arange(n) // gw * patch], dim=1)
    shape = (((n + gw - 1) // gw) * patch // down, gw * patch // down)
    raster, _ = wsi.pca_map(feats, coords, fit, down, shape, patch_size=patch, model=model)
    rgb = model.render_rgb_map(raster, alpha=1.0)
    top, bottom = rgb[: shape[0] // 4, :, 0].float().mean(), rgb[-shape[0] // 4:, :, 0].float().mean()
    print(f"PCA map {shape[0]} x {shape[1]}: {raster.tiles} tiles; mean red of the top quarter {float(top):.1f}, of the bottom quarter {float(bottom):.1f}")
    if a.out:
        with open(a.out, "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (shape[1], shape[0]) + rgb.cpu().numpy().tobytes())
        print("wrote", a.out)


if __name__ == "__main__":
    main()
