#!/usr/bin/env python3
"""Slide pixels in, heatmap, lesion table and lesion polygons out, on one GPU (DESIGN.md sections 10-15): a synthetic slide and its
thumbnail -> tissue_mask -> encode_region with half-overlapping tiles -> wsi.segment_heatmap -> render_heatmap; wsi.segment_regions ->
the regions above the median score, largest first; region_outlines -> their boundary rings with holes, written as GeoJSON in level-0
pixels (what QuPath or ASAP open as annotations); draw_outlines -> the lesions outlined in black and the tissue in blue on the PNG.
Last the GeoJSON is read back as the ground truth and the heatmap is evaluated against it, as the reference's
eval_seg_auc / eval_seg_coarse do against a mask: tile AUROC, the threshold of the best tpr - fpr, Dice at level 16, the threshold sweep.

    python examples/slide_heatmap_synthetic.py [--rows 8] [--cols 10] [--depth 2] [--out slide_heatmap.png] [--geojson lesions.geojson]

No dataset, weights or tokenizer exist offline, so the slide (stained tiles inside an ellipse, grey glass around it), the weights
and the two prompts are seeded synthetic data: the picture shows the flow, not a tumour.  With --attention the same region is encoded twice
more, once with the last block's CLS attention and once with the attention rollout through every block (DESIGN.md sections 19, 20), and
the two token-resolution heatmaps are written side by side.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from keep_amd import KEEPModel, wsi                                   # noqa: E402
from keep_amd.config import KEEPShape, small_shape                    # noqa: E402
from keep_amd.region import TissueSegmentation                        # noqa: E402
from keep_amd.synth import synth_prompts, synth_state_dict, synth_tile_family    # noqa: E402

PATCH, DOWNSAMPLE = 224, 16


def synthetic_slide(rows, cols, dev):
    """[rows * 224, cols * 224, 3] uint8 on the device: `stain_field` tiles inside an ellipse, plain grey glass elsewhere."""
    g = torch.Generator().manual_seed(7)
    stain = synth_tile_family("stain_field", 0, rows * cols, dev, seed=31)
    glass = (236 + torch.randint(-2, 3, (rows * cols, PATCH, PATCH, 3), generator=g)).to(torch.uint8).to(dev)
    yy, xx = torch.meshgrid(torch.arange(rows), torch.arange(cols), indexing="ij")
    inside = (((yy + 0.5) / rows - 0.5) / 0.36) ** 2 + (((xx + 0.5) / cols - 0.5) / 0.4) ** 2 < 1
    tiles = torch.where(inside.reshape(-1, 1, 1, 1).to(dev), stain, glass)
    return tiles.reshape(rows, cols, PATCH, PATCH, 3).permute(0, 2, 1, 3, 4).reshape(rows * PATCH, cols * PATCH, 3).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--cols", type=int, default=10)
    ap.add_argument("--depth", type=int, default=2, help="ViT/BERT depth (24 = the real model's shape; small for a quick look)")
    ap.add_argument("--out", default=os.path.join(tempfile.gettempdir(), "slide_heatmap.png"))
    ap.add_argument("--attention", default="", help="write the last-block CLS attention map and the rollout map, side by side, to this PNG")
    ap.add_argument("--geojson", default=os.path.join(tempfile.gettempdir(), "slide_lesions.geojson"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    shape = KEEPShape() if a.depth >= 24 else small_shape(a.depth, max(1, a.depth // 2))
    model = KEEPModel(shape)
    model.load_state_dict(synth_state_dict(shape, seed=0))
    model.to(dev).eval()

    slide = synthetic_slide(a.rows, a.cols, dev)
    thumb = slide[::DOWNSAMPLE, ::DOWNSAMPLE].contiguous()               # one thumbnail pixel per 16 x 16 slide pixels
    txt = model.encode_text({k: v.to(dev) for k, v in synth_prompts(2, 256, seed=5).items()})          # "normal", "tumour"
    classifier = torch.nn.functional.normalize(txt, dim=-1).t().contiguous()                             # [D, 2]

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tissue = model.tissue_mask(thumb, DOWNSAMPLE, TissueSegmentation(min_area=64, min_hole=16))
    feats, coords = model.encode_region(slide, PATCH, PATCH // 2, tissue=tissue)
    raster = wsi.segment_heatmap(classifier, feats, coords, DOWNSAMPLE, tuple(thumb.shape[:2]), patch_size=PATCH, overlap=True, model=model)
    lo, hi = (float(v) for v in torch.aminmax(raster.mean()[raster.count > 0]))
    picture = model.render_heatmap(raster, thumb, alpha=0.5, colormap="jet", tissue=tissue, window=(lo, max(hi, lo + 1e-3)))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"{a.rows} x {a.cols} cells of {PATCH}: {int(tissue.mask.sum())} of {tissue.mask.numel()} thumbnail pixels are tissue, {feats.shape[0]} tiles "
          f"encoded (step {PATCH // 2}), {raster}, up to {int(raster.count.max())} tiles per pixel, mean in [{lo:.4f}, {hi:.4f}]; "
          f"heatmap {tuple(picture.shape)} in {dt * 1e3:.1f} ms")
    thd = float(raster.mean()[raster.count > 0].median())
    lesions = wsi.segment_regions(raster, thd, tissue=tissue, min_area=4, model=model)
    tissue_regions = model.mask_regions(tissue)
    print(f"{tissue_regions.n} tissue region(s); {lesions.n} region(s) of >= 4 pixels with mean score > {thd:.4f}:")
    print("   id  area px  area mm2 @0.25um  box level-0 (x0, y0, x1, y1)    centroid level-0      mean    peak  border")
    top = lesions.sort("area")
    l0 = top.to_level0()
    for i in range(min(top.n, 10)):
        box, (cx, cy) = [int(v) for v in l0["box"][i]], l0["centroid"][i]
        print(f"  {int(top.ids[i]):3d}  {int(top.area[i]):7d}  {top.area_mm2(0.25)[i]:16.4f}  {str(tuple(box)):30s}  ({cx:8.1f}, {cy:8.1f})  "
              f"{top.mean_score()[i]:.4f}  {top.peak_score()[i]:.4f}  {int(top.border[i])}")
    outlines = model.region_outlines(lesions)
    holes = outlines.n_holes()
    print(f"{outlines.n_rings} ring(s), {int(outlines.vertices.shape[0])} vertices; {int(holes.sum())} hole(s); the largest region's outer ring has "
          f"{len(outlines.polygons(int(top.ids[0]))[0]) if top.n else 0} vertices and a perimeter of {int(outlines.perimeter().max()) if top.n else 0} pixel sides")
    with open(a.geojson, "w") as f:
        json.dump(outlines.to_geojson(table=lesions, max_n_holes=8, min_hole_area=2), f)
    print(f"wrote {a.geojson}")
    picture = model.draw_outlines(model.draw_outlines(picture, tissue_regions, (0, 0, 255), 1), lesions, (0, 0, 0), 1)
    from PIL import Image
    Image.fromarray(picture.cpu().numpy()).save(a.out)
    print(f"wrote {a.out}")
    if a.attention:                                                       # where inside the tiles the model looked: one block, and all of them
        shape_t = tuple(thumb.shape[:2])
        _, c, attn = model.encode_region_attention(slide, PATCH, tissue=tissue, block=-1)
        _, _, rollout = model.encode_region_rollout(slide, PATCH, tissue=tissue, start_block=0, residual=0.5)
        maps = [wsi.attention_heatmap(model, t, c, (14, 14), PATCH, DOWNSAMPLE, shape_t) for t in (attn, rollout)]
        side = torch.cat([model.render_heatmap(r, thumb, alpha=0.6, colormap="jet", tissue=tissue) for r in maps], dim=1)
        Image.fromarray(side.cpu().numpy()).save(a.attention)
        print(f"wrote {a.attention}: last-block CLS attention (left) and attention rollout from block 0 (right), {c.shape[0]} tiles at token resolution")
    from keep_amd.annotation import PolygonSet
    truth = PolygonSet.from_geojson(a.geojson)                            # the polygons just written: what a pathologist would have drawn
    try:
        roc, overlap, sweep = wsi.segment_evaluate(classifier, feats, coords, truth, patch_size=PATCH, overlap=True,
                                                   shape=tuple(thumb.shape[:2]), sweep=True, model=model)
    except ValueError as e:                                               # every tile on one side of the outlines: no ROC to speak of
        print(f"not evaluated: {e}")
        return
    print(f"against its own outlines: tile AUROC {roc.auc:.4f} over {roc.n_pos} + {roc.n_neg} tiles, best threshold {roc.best_threshold:.4f} "
          f"({len(roc.thresholds)} points, {int(roc.kept.sum())} kept); Dice at level 16 {overlap.dice:.4f}, IoU {overlap.iou:.4f}; "
          f"pixel sweep: best Dice {sweep.best_dice:.4f} at {sweep.best_threshold:.4f}, pixel AUROC {sweep.auc:.4f}")


if __name__ == "__main__":
    main()
