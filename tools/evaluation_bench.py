#!/usr/bin/env python3
"""Segmentation evaluation, measured.

  tile_roc       100 000 and 2^24 - 1 tiles (random float32 scores, labels that follow them with noise): keep_eval_roc between device
                 events, scalars only and with the curve, and KEEPModel.tile_roc as a caller sees it (wall clock, its one readback
                 included); beside it the host route for the same input: the copy to the host, then roc_auc_score, roc_curve and
                 thresholds[np.argmax(tpr - fpr)] of scikit-learn as WSI_evaluation/segment_utils.py:113-117 calls them.
  mask_overlap   two masks of 6000 x 6000: keep_eval_mask_counts against the copy to the host + numpy's count_nonzero of the three masks.
  raster_sweep   a 6000 x 6000 raster at downsample 16 of overlapping 224-pixel tiles: keep_eval_raster_hist between device events,
                 KEEPModel.raster_sweep (wall clock) against the copy to the host + raster_hist_numpy + sweep_from_hist_numpy.

Device-event times are the median of --reps warm runs with the min-max spread; host routes run once (--host-reps).  The floor of a
kernel is the bytes it has to read once.  The measurement runs in a child process under a time limit, so one that hangs ends alone.

    python tools/evaluation_bench.py [--tiles 100000,16777215] [--side 6000] [--reps 20] [--limit 900] [--out profiles/evaluation_bench.txt]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from keep_amd import KEEPModel, _lib                                       # noqa: E402
from keep_amd.config import small_shape                                    # noqa: E402
from keep_amd.evaluation import HIST_BINS, mask_counts_numpy, raster_hist_numpy, sweep_from_hist_numpy      # noqa: E402
from keep_amd.model import _ptr, _stream                                   # noqa: E402
from keep_amd.synth import synth_state_dict                                # noqa: E402
from regions_bench import HBM_PEAK, event_ms                               # noqa: E402

LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def row(name, t, floor=None):
    med, lo, hi = t
    tail = ""
    if floor:
        rate = floor / (med * 1e-3)
        tail = f"  floor {floor / 1e6:8.1f} MB -> {rate / 1e9:8.1f} GB/s = {100 * rate / HBM_PEAK:5.2f} % of the HBM peak"
    say(f"    {name:34s} {med:9.3f} ms (min {lo:.3f}, max {hi:.3f}){tail}")


def wall_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms)), min(ms), max(ms)


def roc(m, n, reps, host_reps):
    from sklearn import metrics
    dev, lib, h, st = m._device, _lib.load(), m._handle, _stream(m._device)
    g = torch.Generator().manual_seed(n)
    s = torch.rand((n,), generator=g)
    y = ((s + 0.3 * torch.randn((n,), generator=g)) > 0.5).to(torch.uint8)
    sd, yd = s.to(dev), y.to(dev)
    scalars = torch.empty((8,), dtype=torch.int64, device=dev)
    curve = [torch.empty((n,), dtype=dt, device=dev) for dt in (torch.float32, torch.int32, torch.int32, torch.uint8)]
    say(f"tile_roc, {n} tiles")
    row("keep_eval_roc, scalars only", event_ms(lambda: _lib.check(h, lib.keep_eval_roc(h, _ptr(sd), _ptr(yd), n, _ptr(scalars), None, None, None,
                                                                                          None, st), "eval_roc"), reps), 5 * n)
    row("keep_eval_roc, with the curve", event_ms(lambda: _lib.check(h, lib.keep_eval_roc(h, _ptr(sd), _ptr(yd), n, _ptr(scalars), *map(_ptr, curve),
                                                                                            st), "eval_roc"), reps), 5 * n)
    row("KEEPModel.tile_roc(curve=False), wall", wall_ms(lambda: m.tile_roc(sd, yd, curve=False), reps))
    row("KEEPModel.tile_roc(curve=True), wall", wall_ms(lambda: m.tile_roc(sd, yd), reps))
    got = m.tile_roc(sd, yd)
    say(f"    workspace {lib.keep_workspace_bytes(h) / 1e6:.0f} MB; K = {len(got.thresholds)} points, {int(got.kept.sum())} kept")
    for _ in range(host_reps):
        t0 = time.perf_counter()
        sh, yh = sd.cpu().numpy(), yd.cpu().numpy()
        t1 = time.perf_counter()
        auc = metrics.roc_auc_score(yh, sh)
        fpr, tpr, thresholds = metrics.roc_curve(yh, sh)
        best = thresholds[np.argmax(tpr - fpr)]
        t2 = time.perf_counter()
        say(f"    host route: copy {1e3 * (t1 - t0):.1f} ms + scikit-learn {1e3 * (t2 - t1):.1f} ms; best threshold equal: {bool(best == got.best_threshold)}, "
            f"|auc - roc_auc_score| = {abs(auc - got.auc):.1e}, kept + 1 == len(thresholds): {int(got.kept.sum()) + 1 == len(thresholds)}")
    say()


def masks_and_raster(m, n, reps, host_reps):
    dev, lib, h, st = m._device, _lib.load(), m._handle, _stream(m._device)
    i = torch.arange(n, device=dev, dtype=torch.float32)
    r2 = (i[:, None] - 0.45 * n) ** 2 + (i[None, :] - 0.55 * n) ** 2
    truth = (r2 < (0.3 * n) ** 2).to(torch.uint8) * 255
    d, patch, step = 16, 224, 112
    xs = torch.arange(0, n * d - patch, step, device=dev)
    coords = torch.stack(torch.meshgrid(xs, xs, indexing="xy"), -1).reshape(-1, 2)
    keep = ((coords[:, 0] // step + 3 * (coords[:, 1] // step)) % 11) != 0          # holes: uncovered pixels
    coords = coords[keep]
    c = (coords.to(torch.float32) + patch / 2) / d
    g = torch.Generator().manual_seed(n)
    p = torch.sigmoid(((0.33 * n) ** 2 - (c[:, 1] - 0.5 * n) ** 2 - (c[:, 0] - 0.5 * n) ** 2) / (0.05 * n) ** 2
                      + torch.randn((len(c),), generator=g).to(dev))
    raster = m.tile_raster(coords, p, patch, d, (n, n))
    pred = (raster.mean() > 0.5).to(torch.uint8)
    out4 = torch.empty((4,), dtype=torch.int64, device=dev)
    hist = torch.empty((2, HIST_BINS), dtype=torch.int64, device=dev)
    say(f"masks and raster of {n} x {n} ({n * n / 1e6:.1f} M pixels); the raster holds {len(coords)} tiles of {patch} at downsample {d}")
    row("keep_eval_mask_counts", event_ms(lambda: _lib.check(h, lib.keep_eval_mask_counts(h, _ptr(truth), _ptr(pred), None, n, n, _ptr(out4), st),
                                                              "eval_mask_counts"), reps), 2 * n * n)
    row("KEEPModel.mask_overlap, wall", wall_ms(lambda: m.mask_overlap(truth, pred), reps))
    ov = m.mask_overlap(truth, pred)
    for _ in range(host_reps):
        t0 = time.perf_counter()
        th, ph = truth.cpu().numpy(), pred.cpu().numpy()
        t1 = time.perf_counter()
        counts = (np.count_nonzero(th), np.count_nonzero(ph), np.count_nonzero(th * ph), th.size)
        t2 = time.perf_counter()
        say(f"    host route: copy {1e3 * (t1 - t0):.1f} ms + numpy {1e3 * (t2 - t1):.1f} ms; counts equal: {counts == ov.counts}; dice {ov.dice:.6f}")
    row("keep_eval_raster_hist", event_ms(lambda: _lib.check(h, lib.keep_eval_raster_hist(h, _ptr(raster.acc), _ptr(truth), None, n, n, _ptr(hist), st),
                                                              "eval_raster_hist"), reps), 9 * n * n)
    row("KEEPModel.raster_sweep, wall", wall_ms(lambda: m.raster_sweep(raster, truth), reps))
    sw = m.raster_sweep(raster, truth)
    for _ in range(host_reps):
        t0 = time.perf_counter()
        ah, th = raster.acc.cpu().numpy(), truth.cpu().numpy()
        t1 = time.perf_counter()
        hh = raster_hist_numpy(ah, th)
        t2 = time.perf_counter()
        want = sweep_from_hist_numpy(hh)
        t3 = time.perf_counter()
        say(f"    host route: copy {1e3 * (t1 - t0):.1f} ms + raster_hist_numpy {1e3 * (t2 - t1):.1f} ms + sweep_from_hist_numpy {1e3 * (t3 - t2):.1f} ms; "
            f"histograms equal: {bool(np.array_equal(hh, sw.hist.cpu().numpy()))}; best t16 / u2 equal: "
            f"{(want.best_t16, want.u2) == (sw.best_t16, sw.u2)}")
    say(f"    {sw!r}; occupied bins: {int((sw.hist > 0).sum())}")
    say()


def child(a):
    dev = torch.device("cuda:0")
    shape = small_shape(2, 2)                           # the calls use the handle's arena and stream only
    m = KEEPModel(shape)
    m.load_state_dict(synth_state_dict(shape, seed=0))
    m.to(dev).eval()
    for n in (int(v) for v in a.tiles.split(",") if v):
        roc(m, n, a.reps, a.host_reps)
    masks_and_raster(m, a.side, a.reps, a.host_reps)
    m.check_errors(wait=True)
    with open(a.out, "a") as f:
        f.write("\n".join(LINES) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", default="100000,16777215")
    ap.add_argument("--side", type=int, default=6000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--limit", type=int, default=900, help="seconds the measurement may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluation_bench.txt"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("evaluation_bench needs the GPU: there is nothing to measure without one")
    if a.child:
        return child(a)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(f"tools/evaluation_bench.py on {torch.cuda.get_device_name(0)} (one box); device-event times, median of {a.reps} warm runs\n\n")
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tiles", a.tiles, "--side", str(a.side), "--reps", str(a.reps),
                             "--host-reps", str(a.host_reps), "--out", a.out], timeout=a.limit).returncode
    except subprocess.TimeoutExpired:
        rc = "time limit"
    if rc != 0:
        with open(a.out, "a") as f:
            f.write(f"the child ended with {rc}\n")
        sys.exit(f"evaluation_bench: the child ended with {rc}")


if __name__ == "__main__":
    main()
