#!/usr/bin/env python3
"""Lesion-level scoring, measured.

  mask_distance    a 6000 x 6000 mask (a disc with 2 000 specks beside it): keep_mask_dist2 between device events at R = 5 and R = 64;
                   beside it the host route for the same input: the copy to the host, then scipy's distance_transform_edt.
  raster_peaks     a 6000 x 6000 raster at downsample 16 of 100 000 overlapping 224-pixel tiles: keep_raster_peaks at r = 8 between
                   device events, KEEPModel.raster_peaks as a caller sees it (wall clock, its one readback included); the host route:
                   the copy, the means, then scipy's maximum_filter and the comparison.
  lesion_hits      10^5 candidates against the labelled evaluation mask: keep_lesion_hits; the host route: the copy and numpy indexing
                   with np.maximum.at.
  evaluation_mask  KEEPModel.evaluation_mask in full (dilate by the CAMELYON16 margin, fill holes, label; wall clock); the host route:
                   the copy, distance_transform_edt, binary_fill_holes, label.

Device-event times are the median of --reps warm runs with the min-max spread; host routes run once.  The floor of a kernel is the
bytes it has to read and write once.  The measurement runs in a child process under a time limit, so one that hangs ends alone.

    python tools/lesion_bench.py [--side 6000] [--tiles 100000] [--reps 20] [--limit 900] [--out profiles/lesion_bench.txt]
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
from keep_amd.evaluation import mean16_numpy                               # noqa: E402
from keep_amd.lesion import camelyon16_margin, distance_threshold          # noqa: E402
from keep_amd.model import _ptr, _stream                                   # noqa: E402
from keep_amd.region import TissueMask                                     # noqa: E402
from keep_amd.synth import synth_state_dict                                # noqa: E402
from evaluation_bench import LINES, row, say, wall_ms                      # noqa: E402
from regions_bench import event_ms                                         # noqa: E402


def truth_mask(n, dev):
    i = torch.arange(n, device=dev, dtype=torch.float32)
    disc = ((i[:, None] - 0.45 * n) ** 2 + (i[None, :] - 0.55 * n) ** 2 < (0.2 * n) ** 2) & \
        ~((i[:, None] - 0.5 * n) ** 2 + (i[None, :] - 0.5 * n) ** 2 < (0.05 * n) ** 2)          # a lesion with a hole
    g = torch.Generator().manual_seed(n)
    specks = torch.zeros((n, n), dtype=torch.bool)
    at = torch.randint(0, n - 6, (2000, 2), generator=g)
    for dy in range(6):
        for dx in range(6):
            specks[at[:, 0] + dy, at[:, 1] + dx] = True
    return (disc | specks.to(dev)).to(torch.uint8)


def distance(m, truth, reps):
    from scipy import ndimage
    dev, lib, h, st = m._device, _lib.load(), m._handle, _stream(m._device)
    n = int(truth.shape[0])
    out = torch.empty((n, n), dtype=torch.uint32, device=dev)
    say(f"mask_distance, {n} x {n} ({n * n / 1e6:.1f} M pixels, {int(truth.sum())} set)")
    for R in (5, 64):
        row(f"keep_mask_dist2, R = {R}", event_ms(lambda: _lib.check(h, lib.keep_mask_dist2(h, _ptr(truth), n, n, R, 0, _ptr(out), st), "mask_dist2"),
                                                  reps), 9 * n * n)
        t0 = time.perf_counter()
        th = truth.cpu().numpy()
        t1 = time.perf_counter()
        want = np.minimum(np.rint(ndimage.distance_transform_edt(th == 0) ** 2), R * R + 1).astype(np.uint32)
        t2 = time.perf_counter()
        say(f"    host route: copy {1e3 * (t1 - t0):.1f} ms + distance_transform_edt {1e3 * (t2 - t1):.1f} ms; equal: "
            f"{bool(np.array_equal(want.view(np.int32), out.view(torch.int32).cpu().numpy()))}")
    say()


def evaluation(m, truth, reps):
    from scipy import ndimage
    margin = camelyon16_margin()
    say(f"evaluation_mask, margin {margin:.3f} pixels (R, k = {distance_threshold(margin)})")
    tm = TissueMask(truth, 32)
    row("KEEPModel.evaluation_mask, wall", wall_ms(lambda: m.evaluation_mask(tm, margin), max(reps // 4, 3)))
    em = m.evaluation_mask(tm, margin)
    t0 = time.perf_counter()
    th = truth.cpu().numpy()
    t1 = time.perf_counter()
    grown = ndimage.distance_transform_edt(th == 0) < margin
    t2 = time.perf_counter()
    filled = ndimage.binary_fill_holes(grown)
    t3 = time.perf_counter()
    labels, n = ndimage.label(filled, structure=np.ones((3, 3), int))
    t4 = time.perf_counter()
    say(f"    host route: copy {1e3 * (t1 - t0):.1f} ms + distance_transform_edt {1e3 * (t2 - t1):.1f} ms + binary_fill_holes {1e3 * (t3 - t2):.1f} ms "
        f"+ label {1e3 * (t4 - t3):.1f} ms; {n} lesions, labels equal: {bool(n == em.n and np.array_equal(labels, em.labels.cpu().numpy()))}")
    say()
    return em


def peaks_and_hits(m, em, n, tiles, reps):
    from scipy import ndimage
    dev, lib, h, st = m._device, _lib.load(), m._handle, _stream(m._device)
    d, patch = 16, 224
    g = torch.Generator().manual_seed(tiles)
    coords = torch.randint(0, n * d - patch, (tiles, 2), generator=g).to(dev)
    c = (coords.to(torch.float32) + patch / 2) / d
    p = torch.sigmoid(((0.2 * n) ** 2 - (c[:, 1] - 0.45 * n) ** 2 - (c[:, 0] - 0.55 * n) ** 2) / (0.05 * n) ** 2 + torch.randn((tiles,), generator=g).to(dev))
    raster = m.tile_raster(coords, p, patch, d, (n, n))
    cap = 1 << 20
    peaks = torch.empty((cap, 3), dtype=torch.int64, device=dev)
    n_dev = torch.empty((1,), dtype=torch.int64, device=dev)
    say(f"raster_peaks, {n} x {n} raster of {tiles} tiles of {patch} at downsample {d}, r = 8, min_score 0.5")
    row("keep_raster_peaks", event_ms(lambda: _lib.check(h, lib.keep_raster_peaks(h, _ptr(raster.acc), None, n, n, 8, 32768, cap, _ptr(peaks), _ptr(n_dev),
                                                                                  st), "raster_peaks"), reps), 32 * n * n)
    row("KEEPModel.raster_peaks, wall", wall_ms(lambda: m.raster_peaks(raster, 8, 0.5), reps))
    cand = m.raster_peaks(raster, 8, 0.5)
    t0 = time.perf_counter()
    ah = raster.acc.cpu().numpy()
    t1 = time.perf_counter()
    mean = mean16_numpy(ah)
    key = np.where(mean <= 65535, ((mean + 1) << 32) | (0xFFFFFFFF - np.arange(n * n, dtype=np.int64).reshape(n, n)), 0)
    t2 = time.perf_counter()
    best = ndimage.maximum_filter(key, size=17, mode="constant", cval=0)
    ys, xs = np.nonzero((key != 0) & (key == best) & (mean >= 32768) & (mean <= 65535))
    t3 = time.perf_counter()
    same = len(ys) == len(cand) and np.array_equal(np.stack([xs, ys], 1) * d + d // 2, cand.xy.cpu().numpy())
    say(f"    host route: copy {1e3 * (t1 - t0):.1f} ms + means and keys {1e3 * (t2 - t1):.1f} ms + maximum_filter {1e3 * (t3 - t2):.1f} ms; "
        f"{len(cand)} peaks, equal: {bool(same)}")
    say()

    N = 100000
    xy = torch.randint(0, n * em.downsample, (N, 2), generator=g).to(dev)
    s = torch.rand((N,), generator=g).to(dev)
    hit = torch.empty((N,), dtype=torch.int32, device=dev)
    best_dev = torch.empty((max(em.n, 1),), dtype=torch.float32, device=dev)
    say(f"lesion_hits, {N} candidates against {em.n} lesions")
    row("keep_lesion_hits", event_ms(lambda: _lib.check(h, lib.keep_lesion_hits(h, _ptr(xy), _ptr(s), N, _ptr(em.labels), n, n, em.downsample, 0, 0, em.n,
                                                                                None, _ptr(hit), _ptr(best_dev), st), "lesion_hits"), reps), 24 * N)
    row("KEEPModel.lesion_hits, wall", wall_ms(lambda: m.lesion_hits((xy, s), em), reps))
    got = m.lesion_hits((xy, s), em)
    t0 = time.perf_counter()
    xh, sh, lh = xy.cpu().numpy(), s.cpu().numpy(), em.labels.cpu().numpy()
    t1 = time.perf_counter()
    lab = lh[xh[:, 1] // em.downsample, xh[:, 0] // em.downsample]
    want = np.zeros(em.n + 1, np.float32)
    np.maximum.at(want, lab, sh)
    t2 = time.perf_counter()
    say(f"    host route: copy {1e3 * (t1 - t0):.1f} ms + numpy {1e3 * (t2 - t1):.1f} ms; hits equal: {bool(np.array_equal(lab, got.hit.cpu().numpy()))}, "
        f"maxima equal: {bool(np.array_equal(want[1:], got.lesion_max.cpu().numpy()))}; {int((lab > 0).sum())} candidates on a lesion")
    say()


def child(a):
    dev = torch.device("cuda:0")
    shape = small_shape(2, 2)                           # the calls use the handle's arena and stream only
    m = KEEPModel(shape)
    m.load_state_dict(synth_state_dict(shape, seed=0))
    m.to(dev).eval()
    truth = truth_mask(a.side, dev)
    distance(m, truth, a.reps)
    em = evaluation(m, truth, a.reps)
    peaks_and_hits(m, em, a.side, a.tiles, a.reps)
    m.check_errors(wait=True)
    with open(a.out, "a") as f:
        f.write("\n".join(LINES) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=6000)
    ap.add_argument("--tiles", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=900, help="seconds the measurement may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lesion_bench.txt"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lesion_bench needs the GPU: there is nothing to measure without one")
    if a.child:
        return child(a)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(f"tools/lesion_bench.py on {torch.cuda.get_device_name(0)} (one box); device-event times, median of {a.reps} warm runs\n\n")
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--side", str(a.side), "--tiles", str(a.tiles), "--reps", str(a.reps),
                             "--out", a.out], timeout=a.limit).returncode
    except subprocess.TimeoutExpired:
        rc = "time limit"
    if rc != 0:
        with open(a.out, "a") as f:
            f.write(f"the child ended with {rc}\n")
        sys.exit(f"lesion_bench: the child ended with {rc}")


if __name__ == "__main__":
    main()
