"""Cohort mode: the reference's feature-file dataset and ``run(classifier, dataloader, device)`` loops
 on the GPU similarity kernels.

  * ``WSIClassificationDataset``  <- ``WSI_Classification_Dataset`` (WSI_evaluation/utils.py:11-61):
    one slide per item, CLAM-style feature files ``<data_source>/pt_files/<slide>.pt`` (tensor [N,768])
    or ``<data_source>/h5_files/<slide>.h5`` (datasets ``features`` [N,768] f32, ``coords`` [N,2]).
    h5py is imported lazily: it is not installed in this image, the ``.pt`` path needs nothing.
  * ``run_subtyping`` / ``run_detection`` / ``run_segmentation`` <- the three ``run(classifier, dataloader, device)``
    functions, same arguments and return values (subtyping_utils.py:12-35 raw cosine logits; detection_utils.py:12-36 and
    segment_utils.py:16-42 softmax(10*logits)); ``keep_amd/wsi_evaluation/*_utils.py`` export each of them as ``run``.
  * ``save_slide_features`` writes what ``encode_image`` produced in the same on-disk formats, so feature
    files can be regenerated with this engine instead of the offline CLAM extraction (README.md:74).
  * ``extract_slide_features`` is that extraction: slide pixels in bands -> ``KEEPModel.encode_region`` -> the feature file.
"""
from __future__ import annotations

import os
from typing import Dict, Mapping, Optional, Sequence

import numpy as np
import torch

from .wsi import _engine, _normalized


class WSIClassificationDataset(torch.utils.data.Dataset):
    def __init__(self, df, data_source, target_transform=None, index_col="slide_id", target_col="Diagnosis",
                 use_h5=True, label_map=None):
        self.label_map, self.data_source = label_map, data_source
        self.index_col, self.target_col, self.target_transform = index_col, target_col, target_transform
        self.data, self.use_h5 = df, use_h5

    def __len__(self):
        return len(self.data)

    def _cell(self, idx, col):
        d = self.data
        return d.loc[idx, col] if hasattr(d, "loc") else d[idx][col]

    def get_ids(self, ids):
        return str(self._cell(ids, self.index_col))

    def get_labels(self, ids):
        return self._cell(ids, self.target_col)

    def __getitem__(self, idx):
        slide_id = str(self.get_ids(idx))
        label = self.get_labels(idx)
        if self.label_map is not None:
            label = self.label_map[label]
        if self.target_transform is not None:
            label = self.target_transform(label)
        if self.use_h5:
            try:
                import h5py
            except ImportError as e:            # pragma: no cover - h5py absent in the build image
                raise ImportError("use_h5=True needs h5py; use the pt_files layout (use_h5=False) instead") from e
            with h5py.File(os.path.join(self.data_source, "h5_files", slide_id + ".h5"), "r") as f:
                features = torch.from_numpy(f["features"][:])
                coords = torch.from_numpy(f["coords"][:])
        else:
            features = torch.load(os.path.join(self.data_source, "pt_files", slide_id + ".pt"))
            coords = []
        return {"features": features, "coords": coords, "label": label}


def save_slide_features(data_source: str, slide_id: str, features: torch.Tensor, coords=None, use_h5: bool = False) -> str:
    """Write one slide in the layout ``WSIClassificationDataset`` reads."""
    f = features.detach().to("cpu", torch.float32).contiguous()
    if use_h5:
        import h5py
        os.makedirs(os.path.join(data_source, "h5_files"), exist_ok=True)
        path = os.path.join(data_source, "h5_files", slide_id + ".h5")
        with h5py.File(path, "w") as h:
            h.create_dataset("features", data=f.numpy())
            h.create_dataset("coords", data=np.asarray(coords if coords is not None else np.zeros((f.shape[0], 2), np.int64)))
    else:
        os.makedirs(os.path.join(data_source, "pt_files"), exist_ok=True)
        path = os.path.join(data_source, "pt_files", slide_id + ".pt")
        torch.save(f, path)
    return path


@torch.no_grad()
def extract_slide_features(read_region, width: int, height: int, slide_id: str, data_source: str, patch_size: int = 256,
                           step: Optional[int] = None, tissue=None, band_rows: int = 8, coord_scale: int = 1, use_h5: bool = False,
                           model=None, thumbnail=None, thumbnail_downsample: Optional[int] = None, segmentation=None, stain=None, quality=None) -> str:
    """The feature files the WSI scripts read, made on the device (replaces the CLAM extraction step of README.md:74).

    ``read_region(x, y, w, h)`` returns uint8 [h, w, 3 | 4] pixels of the slide level being tiled, ``width`` x ``height`` pixels
    in all; with openslide, for example::

        ds = int(slide.level_downsamples[level])
        read_region = lambda x, y, w, h: np.asarray(slide.read_region((x * ds, y * ds), level, (w, h)))   # RGBA; alpha is ignored
        extract_slide_features(read_region, *slide.level_dimensions[level], slide_id, out_dir, coord_scale=ds, model=m)

    The slide is walked in horizontal bands of ``band_rows`` grid rows (keep_amd.region.plan_bands); each band goes through
    ``model.encode_region(band, patch_size, step, tissue, origin=(0, y0), coord_scale)``, so every grid cell is encoded exactly once
    and the rows come out in the slide's row-major grid order.  The features (and, with ``use_h5``, the level-0 coords) are
    written by :func:`save_slide_features`; returns its path.

    ``tissue`` may also be a ``keep_amd.region.TissueMask`` (``model.tissue_mask(...)`` or a caller's own mask), or one is made
    first from ``thumbnail`` (uint8 [h,w,3|4] of the whole slide, one pixel = ``thumbnail_downsample`` pixels of the level being
    tiled per side) with ``segmentation`` (a ``TissueSegmentation``)::

        thumb = np.asarray(slide.read_region((0, 0), top, slide.level_dimensions[top]))         # the smallest pyramid level
        extract_slide_features(read_region, ..., thumbnail=thumb,
                               thumbnail_downsample=int(slide.level_downsamples[top] / slide.level_downsamples[level]), model=m)

    With a mask the cells of every band are decided BEFORE ``read_region``: a band with no kept cell is not read at all, of the
    others only the columns ``[min kept x, max kept x + patch_size)`` (keep_amd.region.plan_mask_reads), and that window is cut
    with ``origin=(x0, y0)``.  Rows and coords come out in the same slide row-major order, and the tiles are encoded in the batches
    ``encode_region(whole slide, tissue=mask)`` would form, so the features equal its features exactly.

    ``stain``: a ``keep_amd.stain.StainFit`` (``model.stain_fit(...)``) normalises every batch of cut tiles on the device before it is
    encoded (``encode_region(..., stain=fit)``); ``"macenko"`` fits one first on ``thumbnail`` under the tissue mask
    made from it, and so needs ``thumbnail=``; ``None`` (the default) changes nothing.

    ``quality``: a ``keep_amd.quality.QualityGate``; the cells of every band are measured in the band as read (class counts and focus,
    ``model.region_quality``) and those the gate rejects are neither cut nor encoded nor written; ``None`` (the
    default) changes nothing."""
    from .model import engine_for
    from .region import TissueMask, check_grid_args, plan_bands, plan_mask_reads
    from .quality import check_gate, check_patch
    from .stain import check_stain
    if check_gate(quality) is not None:
        check_patch(patch_size)
    if check_stain(stain, allow_name=True) == "macenko" and thumbnail is None:
        raise ValueError('stain="macenko" fits on the thumbnail: give thumbnail= (or a StainFit of your own)')
    patch, step, _, coord_scale = check_grid_args(patch_size, step, (0, 0), coord_scale)
    bands = plan_bands(width, height, patch, step, band_rows)
    if thumbnail is not None and (tissue is not None or thumbnail_downsample is None):
        raise ValueError("thumbnail= needs thumbnail_downsample= and replaces tissue=: give one of the two")
    if thumbnail is None and (thumbnail_downsample is not None or segmentation is not None):
        raise ValueError("thumbnail_downsample= / segmentation= need thumbnail=")
    m = engine_for(model=model)
    if thumbnail is not None:
        tissue = m.tissue_mask(thumbnail, thumbnail_downsample, segmentation)
        if isinstance(stain, str):                                 # the mask lies on the thumbnail pixel for pixel
            stain = m.stain_fit(thumbnail, TissueMask(tissue.mask, 1))
    feats, coords = [], []
    if isinstance(tissue, TissueMask):
        # every kept cell of the slide, decided on the mask alone; then per band only the window that holds kept cells is read.
        # Tiles are encoded ``batch`` consecutive kept cells at a time ACROSS bands: the batches of one encode_region over the
        # whole slide, so the features equal it bit for bit (and a band with three kept cells does not cost a launch of three)
        m._ready()
        cells = m._mask_cells(tissue, height, width, patch, step, (0, 0)).cpu().numpy().astype(np.int64)
        pending, n_pending, batch = [], 0, 256

        def encode(final):
            nonlocal pending, n_pending
            while n_pending >= batch or (final and n_pending):
                tiles = torch.cat(pending) if len(pending) > 1 else pending[0]
                feats.append(m.encode_image_uint8(tiles[:batch]).cpu())
                pending, n_pending = ([tiles[batch:]], n_pending - batch) if n_pending > batch else ([], 0)
        for x0, y0, w, h in plan_mask_reads(cells, bands, patch, step):
            band = read_region(x0, y0, w, h)
            band = torch.from_numpy(np.ascontiguousarray(band)) if not isinstance(band, torch.Tensor) else band
            if band.dim() != 3 or tuple(band.shape[:2]) != (h, w):
                raise ValueError(f"read_region({x0}, {y0}, {w}, {h}) returned {tuple(band.shape)}, expected [{h}, {w}, 3|4]")
            xy = torch.from_numpy(cells[(cells[:, 1] >= y0) & (cells[:, 1] + patch <= y0 + h)] * coord_scale)
            band = band.to(m._device)
            if quality is not None:
                xy = xy[quality.keep(m.region_quality(band, xy, patch, origin=(x0, y0), coord_scale=coord_scale, rules=quality.rules)).cpu()]
                if len(xy) == 0:
                    continue
            pending.append(m.region_patches_uint8(band, xy, patch, origin=(x0, y0), coord_scale=coord_scale, stain=stain))
            n_pending += len(xy)
            coords.append(xy)
            encode(final=False)
        encode(final=True)
    else:
        for _, _, y0, h in bands:
            band = read_region(0, y0, width, h)
            band = torch.from_numpy(np.ascontiguousarray(band)) if not isinstance(band, torch.Tensor) else band
            if band.dim() != 3 or tuple(band.shape[:2]) != (h, width):
                raise ValueError(f"read_region(0, {y0}, {width}, {h}) returned {tuple(band.shape)}, expected [{h}, {width}, 3|4]")
            f, c = m.encode_region(band, patch, step, tissue, origin=(0, y0), coord_scale=coord_scale, stain=stain, quality=quality)
            feats.append(f.cpu())
            coords.append(c.cpu())
    features = torch.cat(feats) if feats else torch.empty((0, m.config.projection_dim), dtype=torch.float32)
    xy = torch.cat(coords) if coords else torch.empty((0, 2), dtype=torch.int64)
    return save_slide_features(data_source, slide_id, features, xy.numpy(), use_h5=use_h5)


def _loop(model, classifier: torch.Tensor, dataloader, device, softmax: bool, want_targets: bool):
    m = _engine(model, classifier, device=device)
    cls_t = classifier.to(m._device, torch.float32).t().contiguous()          # [C, 768] rows, as keep_similarity wants
    logits_all, coords_all, targets_all = {}, {}, {}
    for idx, data in enumerate(dataloader):                                   # batch size is always 1 slide
        feats = _normalized(m, data["features"])
        coords = data["coords"]
        if not isinstance(coords, list):
            coords = coords.squeeze(0).numpy()
        slide_id = dataloader.dataset.get_ids(idx)
        coords_all[slide_id] = coords
        logits_all[slide_id] = m.similarity(feats, cls_t, scale=10.0 if softmax else 1.0, mode="softmax" if softmax else "raw")
        if want_targets:
            t = data["label"]
            targets_all[slide_id] = t.item() if hasattr(t, "item") else t
    return logits_all, coords_all, targets_all


@torch.no_grad()
def run_subtyping(classifier, dataloader, device, model=None):
    """``run`` of subtyping_utils.py:12-35 -> (raw cosine logits per slide, coords, targets)."""
    return _loop(model, classifier, dataloader, device, softmax=False, want_targets=True)


@torch.no_grad()
def run_detection(classifier, dataloader, device, model=None):
    """``run`` of detection_utils.py:12-36 -> (softmax(10*logits) per slide, coords, targets)."""
    return _loop(model, classifier, dataloader, device, softmax=True, want_targets=True)


@torch.no_grad()
def run_segmentation(classifier, dataloader, device, model=None):
    """``run`` of segment_utils.py:16-42 -> (softmax(10*logits) per slide, coords)."""
    l, c, _ = _loop(model, classifier, dataloader, device, softmax=True, want_targets=False)
    return l, c


def _per_slide(values, targets, what: str):
    """One value and one target per slide, aligned -> two lists.  ``targets``: the ``{slide_id: label}`` a ``run_*`` returns, or a
    sequence; ``values``: a mapping with the same slide ids, or a sequence in the same order.  Every entry is one number."""
    def number(x):
        a = np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x)
        if a.size != 1:
            raise ValueError(f"{what}: one number per slide is needed, got an array of shape {a.shape} (reduce a slide's tiles to its "
                             "call or score first, e.g. with wsi.zero_shot_subtyping / zero_shot_detection)")
        return a.reshape(()).item()
    if isinstance(targets, Mapping):
        ids = list(targets)
        t = [targets[i] for i in ids]
        if isinstance(values, Mapping):
            missing = [i for i in ids if i not in values]
            if missing:
                raise ValueError(f"{what}: no value for slide {missing[0]!r}")
            v = [values[i] for i in ids]
        else:
            v = list(values)
    else:
        t = list(targets)
        v = list(values.values()) if isinstance(values, Mapping) else list(values)
    if len(v) != len(t):
        raise ValueError(f"{what}: {len(v)} values for {len(t)} targets")
    if not t:
        raise ValueError(f"{what}: no slides")
    return [number(x) for x in v], [number(x) for x in t]


def bootstrap_subtyping(preds, targets, n_classes: int, n_boot: int = 1000, seed: int = 0, model=None, device=None):
    """The cohort's balanced accuracy and weighted F1 with bootstrap replicates -> ``{"balanced_accuracy":
    BootstrapResult, "weighted_f1": BootstrapResult}`` (``.estimate``, ``.ci()``), both from the same resamples of the slides.
    ``targets``: what ``run_subtyping`` returns third, ``{slide_id: class index}``; ``preds``: the called class index per slide, a
    mapping with those ids or a sequence in their order."""
    from . import bootstrap
    p, t = _per_slide(preds, targets, "bootstrap_subtyping")
    m = _engine(model, device=device)
    rows, seed, first = m._boot_confusions(np.asarray(t, dtype=np.int64), np.asarray(p, dtype=np.int64), n_classes, n_boot, seed, 0)
    return {name: bootstrap.result_from_confusions(rows, name, seed, first) for name in ("balanced_accuracy", "weighted_f1")}


def bootstrap_detection(scores, targets, n_boot: int = 1000, seed: int = 0, model=None, device=None):
    """The cohort's AUROC with bootstrap replicates -> ``BootstrapResult``.  ``targets``: what ``run_detection`` returns third (non-zero =
    positive); ``scores``: one score per slide, a mapping with those ids or a sequence in their order."""
    s, t = _per_slide(scores, targets, "bootstrap_detection")
    m = _engine(model, device=device)
    return m.bootstrap_roc(np.asarray(s, dtype=np.float64), np.asarray(t, dtype=np.int64) != 0, n_boot, seed)[1]


WSI_Classification_Dataset = WSIClassificationDataset        # the reference's spelling (utils.py:11)
