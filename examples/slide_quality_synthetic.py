#!/usr/bin/env python3
"""Tile quality control on a synthetic slide: the slide of examples/slide_heatmap_synthetic.py with a blue pen
stroke painted across it and one band of rows blurred heavily.  Both pass the tissue mask (ink is strongly saturated, blur keeps the
colour), so without a gate they are encoded and coloured like tissue; with `quality=QualityGate(...)` their cells are measured in the
region and dropped before any tile is cut, and they are gone from the heatmap.  Writes the two heatmaps side by side.

    python examples/slide_quality_synthetic.py [--rows 8] [--cols 10] [--depth 2] [--out slide_quality.png]

No dataset, weights or tokenizer exist offline, so slide, weights and prompts are seeded synthetic data: the picture shows the flow.
"""
import argparse
import os
import sys
import tempfile

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.slide_heatmap_synthetic import DOWNSAMPLE, PATCH, synthetic_slide    # noqa: E402
from keep_amd import KEEPModel, QualityGate, wsi                                   # noqa: E402
from keep_amd import quality as Q                                                  # noqa: E402
from keep_amd.config import KEEPShape, small_shape                                 # noqa: E402
from keep_amd.region import TissueSegmentation                                     # noqa: E402
from keep_amd.synth import synth_prompts, synth_state_dict                         # noqa: E402


def spoil(slide):
    """A diagonal stroke of default-table blue ink, and rows 3 P .. 4 P blurred by three 9 x 9 box filters."""
    H, W = slide.shape[:2]
    yy, xx = torch.meshgrid(torch.arange(H, device=slide.device), torch.arange(W, device=slide.device), indexing="ij")
    slide[((yy - 0.6 * xx - 0.1 * H).abs() < 40) & (xx > W // 4)] = torch.tensor((20, 40, 220), dtype=torch.uint8, device=slide.device)
    band = slide[3 * PATCH:4 * PATCH].permute(2, 0, 1)[None].float()
    for _ in range(3):
        band = F.avg_pool2d(F.pad(band, (4, 4, 4, 4), mode="replicate"), 9, 1)
    slide[3 * PATCH:4 * PATCH] = band.round().clamp(0, 255).to(torch.uint8)[0].permute(1, 2, 0)
    return slide


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--cols", type=int, default=10)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(tempfile.gettempdir(), "slide_quality.png"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    shape = KEEPShape() if a.depth >= 24 else small_shape(a.depth, max(1, a.depth // 2))
    model = KEEPModel(shape)
    model.load_state_dict(synth_state_dict(shape, seed=0))
    model.to(dev).eval()
    slide = spoil(synthetic_slide(a.rows, a.cols, dev))
    thumb = slide[::DOWNSAMPLE, ::DOWNSAMPLE].contiguous()
    txt = model.encode_text({k: v.to(dev) for k, v in synth_prompts(2, 256, seed=5).items()})
    classifier = torch.nn.functional.normalize(txt, dim=-1).t().contiguous()
    tissue = model.tissue_mask(thumb, DOWNSAMPLE, TissueSegmentation(min_area=64, min_hole=16))

    # what the gate will see: every cell of the grid, measured in the region
    grid = model.region_grid(slide, PATCH, PATCH // 2, tissue=tissue)
    q = model.region_quality(slide, grid, PATCH)
    gate = QualityGate(min_tissue=0.25, max_pen=0.05, max_dark=0.5, min_focus=0.25 * float(q.focus(tissue=True).nanmedian()))
    keep = gate.keep(q)
    print(f"{q.n} cells of {PATCH} at step {PATCH // 2}: ink in {int((q.pen_fraction() > gate.max_pen).sum())}, median tissue focus "
          f"{float(q.focus(tissue=True).nanmedian()):.1f}, below {gate.min_focus:.1f} in {int((q.focus(tissue=True) < gate.min_focus).sum())}; "
          f"the gate keeps {int(keep.sum())}")
    # the same on the thumbnail: ink (grown by 2 pixels) and dark taken out of the tissue mask
    classes = model.pen_mask(thumb)
    clean = Q.exclude(tissue, classes, radius=2, model=model)
    print(f"thumbnail: {int(((classes >= 1) & (classes <= 4)).sum())} ink pixels; the tissue mask goes from {int(tissue.mask.sum())} to {int(clean.mask.sum())}")

    pictures = []
    for gate_or_none in (None, gate):
        feats, coords = model.encode_region(slide, PATCH, PATCH // 2, tissue=tissue, quality=gate_or_none)
        raster = wsi.segment_heatmap(classifier, feats, coords, DOWNSAMPLE, tuple(thumb.shape[:2]), patch_size=PATCH, overlap=True, model=model)
        pictures.append(model.render_heatmap(raster, thumb, alpha=0.5, colormap="jet", tissue=tissue))
        print(f"quality={'None' if gate_or_none is None else 'gate'}: {feats.shape[0]} tiles encoded, {int((raster.count > 0).sum())} thumbnail pixels covered")
    from PIL import Image
    Image.fromarray(torch.cat(pictures, dim=1).cpu().numpy()).save(a.out)
    print(f"wrote {a.out}: without the gate (left) and with it (right)")


if __name__ == "__main__":
    main()
