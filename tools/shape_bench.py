"""Two measurements for DESIGN.md section 21, on one GPU:

1. keep_regions_moments against keep_regions_table (without an accumulator) on the same labels, in the same run: both read the label
   image once.  The labels are those of a blocky mask in the thumbnail geometry of a 100 000-tile slide (224-pixel tiles at
   downsample 16: 14 x 14 thumbnail pixels per tile).
2. The Feret pair rate in pairs per second on one large region (a filled square: 4 x side candidates), which sets the default of
   ``max_pairs`` (keep_amd.morphometry.DEFAULT_MAX_PAIRS).

    python tools/shape_bench.py [--reps 20] [--side 32768]

Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from keep_amd import KEEPModel                                   # noqa: E402
from keep_amd.components import NCOLS, RegionTable              # noqa: E402
from keep_amd.config import small_shape                         # noqa: E402
from keep_amd.model import _ptr                                 # noqa: E402
from keep_amd.synth import synth_state_dict                     # noqa: E402


def timed(fn, reps: int) -> float:
    """Median milliseconds of fn() by device events, after two warm-up calls."""
    for _ in range(2):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--side", type=int, default=32768)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model = KEEPModel(precision="strict")
    model.load_state_dict(synth_state_dict(small_shape(2, 2), seed=5), strict=True)
    model = model.to(dev).eval()

    # 1. 100 000 tiles of 14 x 14 thumbnail pixels: 250 x 400 tiles, 55 % of them set
    g = np.random.default_rng(0)
    mask = np.kron(g.random((250, 400)) < 0.55, np.ones((14, 14), np.uint8)).astype(np.uint8)
    regs = model.mask_regions(torch.from_numpy(mask).to(dev), 8)
    h, w, n = mask.shape[0], mask.shape[1], regs.n
    table, moments = torch.empty((n, NCOLS), dtype=torch.int64, device=dev), torch.empty((n, 3), dtype=torch.int64, device=dev)
    t_table = timed(lambda: model._call("regions_table", _ptr(regs.labels), h, w, n, _ptr(None), _ptr(table)), args.reps)
    t_moments = timed(lambda: model._call("regions_moments", _ptr(regs.labels), h, w, n, _ptr(regs.table), _ptr(moments)), args.reps)
    t_feret = timed(lambda: model.region_shape(regs), max(args.reps // 4, 1))
    slide_pairs = model.last_feret_totals[1]

    # 2. one region filling side x side
    s = args.side
    labels = torch.ones((s, s), dtype=torch.int32, device=dev)
    one = torch.empty((1, NCOLS), dtype=torch.int64, device=dev)
    model._call("regions_table", _ptr(labels), s, s, 1, _ptr(None), _ptr(one))
    big = RegionTable(one, labels)
    t_big = timed(lambda: model.region_shape(big, max_pairs=1 << 50), max(args.reps // 4, 1))
    pairs = model.last_feret_totals[1]
    t_small = timed(lambda: model.region_shape(RegionTable(one, labels), feret=False), max(args.reps // 4, 1))
    print(json.dumps({"mask": [h, w], "regions": n, "table_ms": round(t_table, 4), "moments_ms": round(t_moments, 4),
                      "moments_over_table": round(t_moments / t_table, 3), "slide_shape_ms": round(t_feret, 3), "slide_pairs": slide_pairs,
                      "side": s, "pairs": pairs, "shape_ms": round(t_big, 3), "moments_only_ms": round(t_small, 3),
                      "pairs_per_second": round(pairs / ((t_big - t_small) * 1e-3), 0), "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
