"""The slide-analysis methods of ``KEEPModel``: patch grid and tiles of a region, tissue mask, heatmap raster, percentiles and
smoothing, region table, outlines, region shape, polygon fill, segmentation evaluation, the subtype map, bootstrap resampling, the linear probe, attention MIL, feature PCA and the t-SNE tile embedding (DESIGN.md sections 10-32).  Thin wrappers of the
entry points in csrc/slide_api.hip; the argument checks and the numpy references live in the feature modules imported below."""
from __future__ import annotations

import ctypes as C
import struct
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, bootstrap
from .annotation import PolygonSet, check_fill_args, check_into, check_tile_args, polygon_arrays
from .classmap import (ClassMap, ClassRaster, check_class_names, check_class_tiles, check_classes, check_label_map, check_labels, check_palette,
                       class_map_args)
from .cluster import (ONE as CLUSTER_ONE, ClusterSums, TileClusters, check_centroids, check_dim, check_features, check_fit_args, check_init, check_k,
                      check_prev)
from .components import NCOLS as REGION_COLS, RegionTable, check_raster, check_region_count, check_regions_args, mask_tensor
from .evaluation import HIST_BINS, MaskOverlap, RocResult, check_mask, check_roc_args, check_same_geometry, plan_label_bands, sweep_from_hist
from .heatmap import (MAX_TILES, ScoreReference, TileRaster, check_cell_args, check_cells, check_raster_args, check_tiles, check_values,
                      colormap as colormap_table, render_args, smooth_taps)
from .heatmap import Q_ONE
from .lesion import (MAX_LABELS, EvaluationMask, LesionCandidates, LesionHits, check_candidates, check_direction, check_peak_args, check_peak_count,
                     check_radius, distance_threshold)
from .morphometry import DEFAULT_MAX_PAIRS, RegionShape, check_shape_args
from .outline import NCOLS as RING_COLS, RegionOutlines, check_draw_args, check_outline_args, check_ring_count, regions_labels, rgb_tensor
from .region import (MASK_MODES, TILE, TissueMask, TissueSegmentation, check_downsample, check_grid_args, grid_shape, otsu_threshold, region_layout,
                     resize_tables, thumbnail_layout, tissue_params)
from . import fewshot as _fs
from . import mil as _mil
from . import neighbours as _nb
from . import pca as _pca
from . import probe as _probe
from . import stain as _stain
from . import tsne as _tsne
from .quality import NCOLS as QUALITY_COLS, MAX_CELLS as QUALITY_MAX_CELLS, QualityGate, TileQuality, check_gate, check_patch, check_rules
from .stain import StainFit, StainTarget, check_stain


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream(device: torch.device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _check_tile_raster(raster) -> None:
    if not isinstance(raster, TileRaster):
        raise ValueError(f"raster must be a TileRaster, got {type(raster).__name__}")


def _check_tissue(tissue, raster) -> None:
    """``tissue=`` beside a raster: a ``TissueMask`` of the raster's downsample and shape."""
    if not isinstance(tissue, TissueMask):
        raise ValueError(f"tissue must be a TissueMask, got {type(tissue).__name__}")
    if tissue.downsample != raster.downsample or tuple(tissue.mask.shape) != raster.shape:
        raise ValueError(f"tissue mask has downsample {tissue.downsample} and shape {tuple(tissue.mask.shape)}, the raster "
                         f"{raster.downsample} and {raster.shape}")


class SlideOps:
    """Base of ``KEEPModel``, which supplies what these methods use of the engine: ``_handle``, ``_device``, ``_ready()``,
    ``_ready_device()``, ``_queue_flag_check()``, ``encode_image_uint8()``, ``_encode_tapped()``, ``_check_block()``, ``_encode_rollout()``, ``_check_rollout()``, ``config`` and
    ``_heat_luts``."""

    def _call(self, name: str, *args) -> None:
        """``keep_<name>(handle, *args, current stream)``; a failure raises with the library's message, labelled ``name``."""
        _lib.check(self._handle, getattr(_lib.load(), "keep_" + name)(self._handle, *args, _stream(self._device)), name)

    def _on_device(self, a, dtype=None) -> torch.Tensor:
        """numpy or torch, host or device -> contiguous on the engine's device, as ``dtype`` if one is given; a bool mask as uint8."""
        t = (torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a).to(self._device, dtype).contiguous()
        return t.view(torch.uint8) if t.dtype == torch.bool else t

    def _raster_here(self, raster) -> None:
        if raster.acc.device != self._device:
            raise ValueError(f"the raster lives on {raster.acc.device}, this engine on {self._device}")

    # ------------------------------------------------------------------ slide regions
    @staticmethod
    def _region_tensor(region) -> torch.Tensor:
        """uint8 [H,W,3|4] tensor or numpy array, checked on the host (shape / dtype / pixel-stride errors before any device work)."""
        x = torch.from_numpy(region) if not isinstance(region, torch.Tensor) else region
        region_layout(x)
        return x

    def _region_on_device(self, x: torch.Tensor) -> Tuple[torch.Tensor, int, int, int, int]:
        """-> (device view, H, W, C, row_stride_bytes); a device region of any row stride is used in place."""
        if x.device != self._device:
            x = x.to(self._device)                                 # a cropped host view arrives contiguous
        H, W, C, row = region_layout(x)
        return x, H, W, C, row

    def _region_cells(self, xd: torch.Tensor, H: int, W: int, C: int, row: int, patch: int, step: int, sat_min: int,
                      min_pixels: int) -> torch.Tensor:
        """keep_region_grid -> the kept cells' (x, y) offsets in the region, int32 [N,2] on the device (reads N back: one sync)."""
        gy, gx = grid_shape(H, W, patch, step)
        if gy * gx == 0:
            return torch.empty((0, 2), dtype=torch.int32, device=self._device)
        cells = torch.empty((gy * gx, 2), dtype=torch.int32, device=self._device)
        n = torch.empty((1,), dtype=torch.int64, device=self._device)
        self._call("region_grid", _ptr(xd), H, W, row, C, patch, step, sat_min, min_pixels, _ptr(cells), _ptr(n))
        return cells[:int(n.item())]

    def _region_tiles(self, xd: torch.Tensor, H: int, W: int, C: int, row: int, cells: torch.Tensor, patch: int) -> torch.Tensor:
        """keep_region_patches_u8: int32 [B,2] cells -> uint8 [B,224,224,3] tiles on the device."""
        cells = cells.to(self._device, torch.int32).contiguous()
        B = int(cells.shape[0])
        out = torch.empty((B, TILE, TILE, 3), dtype=torch.uint8, device=self._device)
        if patch == TILE:
            xb = xk = None
            xks = 0
        else:
            xb, xk, xks = resize_tables(patch, self._device)
        self._call("region_patches_u8", _ptr(xd), H, W, row, C, _ptr(cells), B, patch, _ptr(xb), _ptr(xk), xks, _ptr(xb), _ptr(xk), xks, _ptr(out))
        return out

    def _mask_cells(self, mask, H: int, W: int, patch: int, step: int, origin) -> torch.Tensor:
        """keep_region_grid_mask -> the kept cells' (x, y) offsets in an H x W region at ``origin``, int32 [N,2] on the device (reads N
        back: one sync).  The region's pixels play no part."""
        gy, gx = grid_shape(H, W, patch, step)
        if gy * gx == 0:
            return torch.empty((0, 2), dtype=torch.int32, device=self._device)
        md = mask.mask.to(self._device)
        cells = torch.empty((gy * gx, 2), dtype=torch.int32, device=self._device)
        n = torch.empty((1,), dtype=torch.int64, device=self._device)
        self._call("region_grid_mask", _ptr(md), int(md.shape[0]), int(md.shape[1]), mask.downsample, H, W, patch, step, origin[0], origin[1],
                   MASK_MODES.index(mask.mode), _ptr(cells), _ptr(n))
        return cells[:int(n.item())]

    @torch.no_grad()
    def tissue_mask(self, thumbnail, downsample: int, params=None):
        """Tissue segmentation of a slide thumbnail on the device -> ``keep_amd.region.TissueMask``.

        ``thumbnail``: uint8 [h,w,3] (RGB) or [h,w,4] (RGBA, alpha ignored), host or device, numpy or torch, any row stride,
        ``h w <= 2^30``; one pixel of it covers ``downsample`` x ``downsample`` pixels of the level that will be tiled.  ``params``: a
        ``keep_amd.region.TissueSegmentation`` (default: its defaults).  Stages, after CLAM's ``segmentTissue`` but on the pixel mask
        instead of contour polygons, all in integers and equal to ``keep_amd.region.tissue_mask_numpy`` bit for bit: HSV saturation,
        k x k median, fixed or Otsu threshold (the histogram is made on the device, the 256-candidate choice on the host; the
        threshold used is ``.threshold`` of the result), closing, small holes filled, small fragments dropped.  The mask stays on
        the engine's device; hand the result to ``region_grid`` / ``encode_region`` / ``extract_slide_features`` as ``tissue=``."""
        params = TissueSegmentation() if params is None else params
        if not isinstance(params, TissueSegmentation):
            raise ValueError(f"params must be a TissueSegmentation, got {params!r}")
        downsample = check_downsample(downsample)
        x = torch.from_numpy(thumbnail) if not isinstance(thumbnail, torch.Tensor) else thumbnail
        thumbnail_layout(x)
        self._ready_device()
        if x.device != self._device:
            x = x.to(self._device)
        h, w, C, row = thumbnail_layout(x)
        med = torch.empty((h, w), dtype=torch.uint8, device=self._device)
        hist = torch.empty((256,), dtype=torch.int32, device=self._device)
        self._call("tissue_median_hist", _ptr(x), h, w, row, C, params.mthresh, _ptr(med), _ptr(hist))
        t = otsu_threshold(hist.cpu().tolist()) if params.use_otsu else int(params.sthresh)
        mask = torch.empty((h, w), dtype=torch.uint8, device=self._device)
        self._call("tissue_mask", _ptr(med), h, w, t, params.close, params.min_hole, params.min_area, _ptr(mask))
        self._queue_flag_check(_stream(self._device))
        self.last_tissue_median, self.last_tissue_hist = med, hist                  # the intermediates, for inspection and tests
        return TissueMask(mask, downsample, params.mode, t)

    # ------------------------------------------------------------------ heatmap
    @torch.no_grad()
    def tile_raster(self, coords, values, patch_size: int, downsample: int, shape, origin=(0, 0), into=None):
        """Per-tile values rasterised in slide geometry on the device -> ``keep_amd.heatmap.TileRaster``.

        ``coords``: integers [N,2], level-0 ``(x, y)`` (the convention of ``wsi.refine`` / ``cood2str`` / ``region_grid``); ``values``:
        floating point [N]; both host or device, numpy or torch.  ``patch_size``: a tile's footprint in the units of the coords
        (``patch_size * coord_scale`` of ``encode_region``); one raster pixel covers ``downsample`` x ``downsample`` of them,
        ``1 <= downsample <= patch_size``; ``shape``: the raster's ``(h, w)``, ``h w <= 2^30``; ``origin``: the level-0 position of raster
        pixel (0, 0), a multiple of ``downsample``.  Tile n adds ``rint(clip(float32(v), 0, 1) * 65535)`` and a count of one to the
        columns ``[(x - ox) // d, (x - ox + P) // d)`` and the rows likewise (floor division, clipped to the raster); a NaN value skips
        its tile; duplicate coords each count (pass the output of ``wsi.refine`` for first-occurrence-wins).  Coordinates must stay
        within +-2^62 (they are not read on the host).  ``into``: an earlier raster of the same geometry to add to; the result is the
        same however the tiles are split over calls.  At most 2^24 - 1 tiles go into one raster.  No host synchronisation."""
        patch, d, (h, w), origin = check_raster_args(patch_size, downsample, shape, origin)
        c = coords if isinstance(coords, torch.Tensor) else torch.as_tensor(coords)
        v = values if isinstance(values, torch.Tensor) else torch.as_tensor(values)
        N = check_tiles(c, v)
        into, zero = self._raster_into(N, patch, d, (h, w), origin, into)
        c = c.to(self._device, torch.int64).contiguous()
        v = v.to(self._device, torch.float32).contiguous()
        self._call("heat_accumulate", _ptr(c), _ptr(v), N, patch, d, h, w, origin[0], origin[1], zero, _ptr(into.acc))
        return into

    def _raster_into(self, N: int, patch: int, d: int, shape, origin, into):
        """The raster N more tiles go into -> (raster, zero_first): ``into`` after its geometry and device checks with the tiles claimed
        (ValueError beyond the cap, before any device work), or a new one."""
        if into is not None:
            if not isinstance(into, TileRaster):
                raise ValueError(f"into must be a TileRaster, got {type(into).__name__}")
            into.check_geometry(patch, d, shape, origin)
            into.claim(N)                                           # raises beyond the cap, before any device work
        elif N > MAX_TILES:
            raise ValueError(f"a raster takes at most 2^24 - 1 = {MAX_TILES} tiles in all, got {N}")
        self._ready_device()
        if into is None:
            return TileRaster(torch.empty(shape, dtype=torch.int64, device=self._device), d, patch, origin, N, self), 1
        if into.acc.device != self._device:
            into.tiles -= N
            raise ValueError(f"into= raster lives on {into.acc.device}, this engine on {self._device}")
        return into, 0

    @torch.no_grad()
    def cell_raster(self, coords, cell_values, grid, patch_size: int, downsample: int, shape, origin=(0, 0), into=None):
        """Values on a grid of cells inside every tile rasterised in slide geometry -> ``TileRaster``: the
        token-level counterpart of :meth:`tile_raster`, made for the maps of ``keep_amd.attention.cls_attention_map``.

        ``coords``: integers [N,2] as in :meth:`tile_raster`; ``cell_values``: floating point [N, gh gw], row-major (y, x) over the
        ``grid = (gh, gw)`` cells of a tile, each ``patch_size / gw`` x ``patch_size / gh`` level-0 units (both divisions exact);
        ``1 <= downsample <= min(cell width, cell height)``.  A tile covers exactly the pixels it covers in :meth:`tile_raster`; pixel
        (X, Y) of them takes the cell ``cx = clamp((X d + ox - x) // cw, 0, gw - 1)``, ``cy`` likewise: the cell under the pixel's
        upper-left corner.  It adds ``rint(clip(float32(v), 0, 1) * 65535)`` and a count of ONE, so the count, the cap of 2^24 - 1 and
        ``into=`` are about tiles, as before; a NaN cell adds nothing to its pixels.  Tiles that are constant over their cells give
        :meth:`tile_raster`'s raster bit for bit.  The result goes to ``mean()``, :meth:`render_heatmap`, :meth:`smooth_raster` and
        :meth:`mask_regions` unchanged.  Integer arithmetic, the same however the tiles are split over calls; no host
        synchronisation."""
        (gh, gw), patch, d, (h, w), origin = check_cell_args(grid, patch_size, downsample, shape, origin)
        c = coords if isinstance(coords, torch.Tensor) else torch.as_tensor(coords)
        v = cell_values if isinstance(cell_values, torch.Tensor) else torch.as_tensor(cell_values)
        N = check_cells(c, v, (gh, gw))
        into, zero = self._raster_into(N, patch, d, (h, w), origin, into)
        c = c.to(self._device, torch.int64).contiguous()
        v = v.to(self._device, torch.float32).contiguous()
        self._call("heat_accumulate_cells", _ptr(c), _ptr(v), N, gh, gw, patch, d, h, w, origin[0], origin[1], zero, _ptr(into.acc))
        return into

    def _heat_read(self, raster, uncovered: float, mean: bool, count: bool, pred: bool):
        """keep_heat_mean -> (mean fp32 | None, count int32 | None, pred uint8 | None), each [h,w] on the device."""
        h, w = raster.shape
        outs = [torch.empty((h, w), dtype=dt, device=self._device) if on else None
                for on, dt in ((mean, torch.float32), (count, torch.int32), (pred, torch.uint8))]
        self._call("heat_mean", _ptr(raster.acc), h, w, uncovered, _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]))
        return tuple(outs)

    @torch.no_grad()
    def render_heatmap(self, raster, thumbnail=None, alpha: float = 0.4, colormap="jet", tissue=None, window=(0.0, 1.0),
                       min_value: float = 0.0, background=(255, 255, 255)) -> torch.Tensor:
        """The raster's mean, coloured and blended over the thumbnail -> uint8 [h,w,3] on the device.

        ``thumbnail``: uint8 [h,w,3|4] of the raster's shape (the layout contract of :meth:`tissue_mask`: any row stride, alpha
        ignored; host or device), or None for the constant ``background``.  ``tissue``: a ``TissueMask`` of the raster's downsample
        and shape; pixels outside it are not painted.  ``colormap``: "jet", "gray" or a uint8 [256,3] table
        (``keep_amd.heatmap.colormap``).  ``window``: the values mapped to the ends of the table; ``min_value``: pixels whose mean
        is below it are not painted; ``alpha``: the weight of the colour, used as ``round(256 alpha)``.  All in integers on the
        16-bit fixed-point sums, equal to ``keep_amd.heatmap.render_numpy`` bit for bit.  CLAM's percentile ranks and blur are
        steps made before this one: :meth:`percentiles` on the tile values, :meth:`smooth_raster` on the raster."""
        _check_tile_raster(raster)
        a, lo16, hi16, min16, bg = render_args(alpha, window, min_value, background)
        h, w = raster.shape
        key = colormap if isinstance(colormap, str) else None
        lut_host = colormap_table(colormap)
        x = None
        if thumbnail is not None:
            x = torch.from_numpy(thumbnail) if not isinstance(thumbnail, torch.Tensor) else thumbnail
            if region_layout(x)[:2] != (h, w):
                raise ValueError(f"thumbnail is {tuple(x.shape[:2])}, the raster {(h, w)}")
        if tissue is not None:
            _check_tissue(tissue, raster)
        self._ready_device()
        self._raster_here(raster)
        lut = self._heat_luts.get(key)
        if lut is None or lut.device != self._device:
            lut = torch.from_numpy(lut_host).to(self._device)
            if key is not None:
                self._heat_luts[key] = lut                              # the named tables are uploaded once
        ps, row = 3, 0
        if x is not None:
            if x.device != self._device:
                x = x.to(self._device)
            _, _, ps, row = region_layout(x)
        md = None if tissue is None else tissue.mask.to(self._device)
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=self._device)
        self._call("heat_render", _ptr(raster.acc), h, w, _ptr(x), row, ps, bg[0] | bg[1] << 8 | bg[2] << 16, _ptr(md), _ptr(lut), a, lo16, hi16,
                   min16, _ptr(out))
        return out

    # ------------------------------------------------------------------ heatmap percentiles and smoothing
    def _values_f32(self, values, name: str, least: int) -> torch.Tensor:
        """A population or queries (host or device, numpy or torch, any floating dtype) checked on the host -> fp32 [N] on the device."""
        v = values if isinstance(values, torch.Tensor) else torch.as_tensor(values)
        check_values(v, name, least)
        self._ready_device()
        return v.to(self._device, torch.float32).contiguous()

    @torch.no_grad()
    def score_reference(self, values):
        """A score population sorted on the device -> ``keep_amd.heatmap.ScoreReference``.  ``values``: floating
        point [M], ``1 <= M <= 2^24 - 1``, host or device, numpy or torch, rounded to float32 first.  NaNs are not part of the
        population and -0 counts as +0; equal to ``keep_amd.heatmap.sort_numpy`` bit for bit.  No host synchronisation."""
        v = self._values_f32(values, "values", 1)
        M = int(v.shape[0])
        out = torch.empty((M,), dtype=torch.float32, device=self._device)
        n = torch.empty((1,), dtype=torch.int64, device=self._device)
        self._call("sort_f32", _ptr(v), M, _ptr(out), _ptr(n))
        return ScoreReference(out, n, self)

    def _rank(self, reference, values, self_rank: bool, pct: bool, counts: bool):
        """keep_rank_f32 -> (pct fp32 | None, less int32 | None, eq int32 | None), each [N] on the device."""
        if not isinstance(reference, ScoreReference):
            raise ValueError(f"reference must be a ScoreReference, got {type(reference).__name__}")
        q = self._values_f32(values, "values", 0)
        if reference.sorted.device != self._device:
            raise ValueError(f"the reference lives on {reference.sorted.device}, this engine on {self._device}")
        N = int(q.shape[0])
        outs = [torch.empty((N,), dtype=dt, device=self._device) if on else None
                for on, dt in ((pct, torch.float32), (counts, torch.int32), (counts, torch.int32))]
        if N == 0:
            return tuple(outs)                                          # empty tensors have no address to pass
        self._call("rank_f32", _ptr(reference.sorted), reference.M, _ptr(reference.n), _ptr(q), N, int(self_rank), _ptr(outs[0]), _ptr(outs[1]),
                   _ptr(outs[2]))
        return tuple(outs)

    @torch.no_grad()
    def percentiles(self, values, reference=None) -> torch.Tensor:
        """Rank percentiles on the device -> fp32 [N] in (0, 1].  ``reference=None`` ranks the values among
        themselves: ``(2 less + eq + 1) / (2 n)``, which is ``scipy.stats.rankdata(v, 'average') / n`` over the n values that are not
        NaN.  With a ``ScoreReference`` (:meth:`score_reference`) they are outsiders to that population: ``(2 less + eq) / (2 n)``,
        ``scipy.stats.percentileofscore(ref, v, kind='mean') / 100``.  A NaN stays NaN.  Equal to
        ``keep_amd.heatmap.percentiles_numpy`` bit for bit; no host synchronisation."""
        if reference is None:
            q = self._values_f32(values, "values", 1)
            return self._rank(self.score_reference(q), q, True, True, False)[0]
        return self._rank(reference, values, False, True, False)[0]

    @torch.no_grad()
    def smooth_raster(self, raster, sigma=None, radius=None, taps=None, tissue=None):
        """A raster's mean smoothed by a Gaussian under its support -> a new ``TileRaster`` of the same
        geometry and ``tiles``, whose pixels hold the smoothed mean in 16-bit fixed point with a count of one where the input was
        covered (and inside ``tissue``), nothing elsewhere.  ``sigma`` (and ``radius``, default ``ceil(3 sigma)``) make the taps
        with ``keep_amd.heatmap.gaussian_taps``; or pass ``taps``, an odd number of non-negative integers with a centre >= 1 and a sum
        <= 32768.  ``tissue``: a ``TissueMask`` of the raster's downsample and shape.  A normalised convolution: uncovered and
        masked-out pixels neither give nor receive, a constant region stays constant.  Integer arithmetic, equal to
        ``keep_amd.heatmap.smooth_numpy`` bit for bit.  The input must be a raster as ``tile_raster`` makes it (sum <= 65535 count)."""
        _check_tile_raster(raster)
        t = smooth_taps(sigma, radius, taps)
        h, w = raster.shape
        if tissue is not None:
            _check_tissue(tissue, raster)
        self._ready_device()
        self._raster_here(raster)
        td = torch.from_numpy(t).to(self._device)
        md = None if tissue is None else self._on_device(tissue.mask)
        out = torch.empty((h, w), dtype=torch.int64, device=self._device)
        self._call("heat_smooth", _ptr(raster.acc), h, w, _ptr(md), _ptr(td), t.size // 2, _ptr(out))
        return TileRaster(out, raster.downsample, raster.patch, raster.origin, raster.tiles, self)

    # ------------------------------------------------------------------ subtype map
    @torch.no_grad()
    def class_raster(self, coords, values, patch_size: int, downsample: int, shape, origin=(0, 0), into=None, labels=None, n_classes=None,
                     classes=None):
        """Per-tile class values rasterised in slide geometry, all classes in one launch ->
        ``keep_amd.classmap.ClassRaster``.

        ``coords``: integers [N,2] as in :meth:`tile_raster`; ``values``: floating point [N,C], ``1 <= C <= 64`` (the refined
        probabilities of ``wsi.refine``); the geometry arguments are :meth:`tile_raster`'s, with ``C h w <= 2^30``.  Plane c of the result
        is exactly ``tile_raster(coords, values[:, c], ...)`` over the tiles whose row holds no NaN: a NaN anywhere in a row skips the
        tile in every plane, so all planes count the same tiles.  ``labels``: integers [N] given INSTEAD of ``values`` (``values=None``),
        every one in ``0 .. C - 1`` (checked on the host: one read of their range), expanded to one-hot rows on the device: a vote
        raster.  C is then ``n_classes``, the number of ``classes`` (optional names, kept on the result) or that of ``into``.
        ``into``: an earlier ``ClassRaster`` of the same geometry and C to add to; the result is the same however the tiles are split
        over calls.  At most 2^24 - 1 tiles go into one raster."""
        patch, d, (h, w), origin = check_raster_args(patch_size, downsample, shape, origin)
        if (values is None) == (labels is None):
            raise ValueError("give values= [N,C] or labels= [N], one of the two")
        if into is not None and not isinstance(into, ClassRaster):
            raise ValueError(f"into must be a ClassRaster, got {type(into).__name__}")
        names = check_class_names(classes)
        c = coords if isinstance(coords, torch.Tensor) else torch.as_tensor(coords)
        if values is not None:
            v = values if isinstance(values, torch.Tensor) else torch.as_tensor(values)
            N, C = check_class_tiles(c, v)
            if n_classes is not None and check_classes(n_classes) != C:
                raise ValueError(f"n_classes is {n_classes}, values has {C} columns")
        else:
            given = [k for k in (n_classes, None if names is None else len(names), None if into is None else into.n_classes) if k is not None]
            if not given or any(k != given[0] for k in given):
                raise ValueError("labels= needs the number of classes: n_classes=, classes= or into= (and they must agree)")
            C = check_classes(given[0])
            l = labels if isinstance(labels, torch.Tensor) else torch.as_tensor(labels)
            N = check_labels(c, l, C)
        check_class_names(names, C)
        check_classes(C, (h, w))
        if into is not None:
            into.check_geometry(C, patch, d, (h, w), origin)
            into.claim(N)                                           # raises beyond the cap, before any device work
        elif N > MAX_TILES:
            raise ValueError(f"a raster takes at most 2^24 - 1 = {MAX_TILES} tiles in all, got {N}")
        try:
            self._ready_device()
            if into is not None and into.acc.device != self._device:
                raise ValueError(f"into= raster lives on {into.acc.device}, this engine on {self._device}")
        except Exception:
            if into is not None:
                into.tiles -= N
            raise
        if into is None:
            into = ClassRaster(torch.zeros((C, h, w), dtype=torch.int64, device=self._device), d, patch, origin, N, names, self)
        c = c.to(self._device, torch.int64).contiguous()
        if values is not None:
            v = v.to(self._device, torch.float32).contiguous()
        else:
            v = torch.zeros((N, C), dtype=torch.float32, device=self._device)
            v.scatter_(1, l.to(self._device, torch.int64).reshape(N, 1), 1.0)
        self._call("heat_accumulate_classes", _ptr(c), _ptr(v), N, C, patch, d, h, w, origin[0], origin[1], _ptr(into.acc))
        return into

    @torch.no_grad()
    def class_map(self, raster, tissue=None, min_value: float = 0.0, min_margin: float = 0.0):
        """The per-pixel call of a ``ClassRaster`` -> ``keep_amd.classmap.ClassMap``.

        With n the number of tiles over a pixel and S_c the planes' sums there: the label is the smallest c with the largest S_c (the
        argmax of the means, ties to the lowest class), 255 where n = 0 or outside ``tissue`` (a ``TissueMask`` of the raster's
        geometry), and 254 where the winner's mean is below ``min_value`` or its lead over the runner-up below ``min_margin`` (both in
        16-bit fixed point, compared as ``S < t16 * n``).  ``.top`` and ``.margin`` hold the winner's sum and its lead as
        ``TileRaster``s.  Equal to ``keep_amd.classmap.class_argmax_numpy`` exactly; no host synchronisation."""
        if not isinstance(raster, ClassRaster):
            raise ValueError(f"raster must be a ClassRaster, got {type(raster).__name__}")
        min16, margin16 = class_map_args(min_value, min_margin)
        if tissue is not None:
            _check_tissue(tissue, raster)
        self._ready_device()
        self._raster_here(raster)
        C, (h, w) = raster.n_classes, raster.shape
        md = None if tissue is None else self._on_device(tissue.mask)
        labels = torch.empty((h, w), dtype=torch.uint8, device=self._device)
        top, margin = (torch.empty((h, w), dtype=torch.int64, device=self._device) for _ in range(2))
        self._call("class_argmax", _ptr(raster.acc), C, h, w, _ptr(md), min16, margin16, _ptr(labels), _ptr(top), _ptr(margin))
        as_raster = lambda acc: TileRaster(acc, raster.downsample, raster.patch, raster.origin, raster.tiles, self)
        return ClassMap(labels, as_raster(top), as_raster(margin), raster, self)

    @torch.no_grad()
    def label_confusion(self, a, b, n_classes: int, within=None) -> torch.Tensor:
        """The confusion of two label maps on the device -> int64 ``[C+1, C+1]`` on the device: entry (i, j)
        counts the pixels inside ``within`` with ``a = i`` and ``b = j``; every label ``>= C`` (254 and 255 among them) goes to index C.
        ``a``, ``b``: uint8 ``[h,w]`` of one shape, numpy or torch, host or device, or ``ClassMap``s; ``within``: bool / uint8 ``[h,w]`` or a
        ``TissueMask``.  ``keep_amd.classmap.overlap_from_confusion`` reads Dice, IoU, precision and recall per class off it.  Equal to
        ``keep_amd.classmap.confusion_numpy`` exactly; no host synchronisation."""
        C = check_classes(n_classes)
        a = check_label_map(a, "a")
        shape = (int(a.shape[0]), int(a.shape[1]))
        b = check_label_map(b, "b", shape)
        within = None if within is None else check_mask(within, "within", shape)
        self._ready_device()
        a, b, within = self._on_device(a), self._on_device(b), (None if within is None else self._on_device(within))
        out = torch.empty((C + 1, C + 1), dtype=torch.int64, device=self._device)
        self._call("class_confusion", _ptr(a), _ptr(b), _ptr(within), shape[0], shape[1], C, _ptr(out))
        return out

    @torch.no_grad()
    def annotation_label_map(self, polygon_sets, downsample: int, shape, order=None, rule: str = "union") -> torch.Tensor:
        """One ``PolygonSet`` per class -> a uint8 ``[h,w]`` label map on the device: class c where set c covers the pixel
        (:meth:`annotation_mask` of that set, with the same ``order`` / ``rule``), later sets painted over earlier ones, 255 where no
        set covers it.  What a multi-class ground truth is compared as in :meth:`label_confusion`."""
        sets = list(polygon_sets)
        check_classes(len(sets))
        for p in sets:
            if not isinstance(p, PolygonSet):
                raise ValueError(f"polygon_sets must hold PolygonSets, got {type(p).__name__}")
        check_fill_args(downsample, shape, (0, 0), rule, 1)
        out = None
        for c, p in enumerate(sets):
            m = self.annotation_mask(p, downsample, shape, order, rule).mask
            if out is None:
                out = torch.full_like(m, 255)
            out = torch.where(m != 0, torch.full_like(m, c), out)
        return out

    @torch.no_grad()
    def render_class_map(self, cm, thumbnail=None, alpha: float = 0.5, palette=None, strength=None, window=(0.0, 1.0),
                         background=(255, 255, 255)) -> torch.Tensor:
        """A label map painted with a palette over the thumbnail -> uint8 [h,w,3] on the device.

        ``cm``: a ``ClassMap``; ``thumbnail`` / ``background`` / ``alpha`` as in :meth:`render_heatmap`; ``palette``: uint8 [C,3]
        (default ``keep_amd.classmap.palette(C)``).  Pixels labelled 254 or 255 show the underlay.  ``strength``: ``"margin"`` or
        ``"top"`` (the map's own rasters) or a ``TileRaster`` of its shape: its mean, windowed by ``window`` to 0..255 with
        :meth:`render_heatmap`'s index rule, scales alpha: ``a_eff = (a idx + 127) // 255``, so a confident call is painted stronger.
        Equal to ``keep_amd.classmap.class_render_numpy`` exactly."""
        if not isinstance(cm, ClassMap):
            raise ValueError(f"cm must be a ClassMap, got {type(cm).__name__}")
        a, lo16, hi16, _, bg = render_args(alpha, window, 0.0, background)
        h, w = cm.shape
        pal_host = check_palette(palette, cm.n_classes)
        if isinstance(strength, str):
            if strength not in ("margin", "top"):
                raise ValueError(f"strength must be 'margin', 'top' or a TileRaster, got {strength!r}")
            strength = cm.margin if strength == "margin" else cm.top
        if strength is not None:
            _check_tile_raster(strength)
            if strength.shape != (h, w):
                raise ValueError(f"strength is {strength.shape}, the label map {(h, w)}")
        x = None
        if thumbnail is not None:
            x = torch.from_numpy(thumbnail) if not isinstance(thumbnail, torch.Tensor) else thumbnail
            if region_layout(x)[:2] != (h, w):
                raise ValueError(f"thumbnail is {tuple(x.shape[:2])}, the label map {(h, w)}")
        self._ready_device()
        if strength is not None:
            self._raster_here(strength)
        labels = self._on_device(cm.labels)
        pal = torch.from_numpy(pal_host).to(self._device)
        ps, row = 3, 0
        if x is not None:
            if x.device != self._device:
                x = x.to(self._device)
            _, _, ps, row = region_layout(x)
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=self._device)
        self._call("class_render", _ptr(labels), h, w, cm.n_classes, _ptr(x), row, ps, bg[0] | bg[1] << 8 | bg[2] << 16, _ptr(pal), a,
                   _ptr(None if strength is None else strength.acc), lo16, hi16, _ptr(out))
        return out

    # ------------------------------------------------------------------ tile clustering
    def _cluster_features(self, features, normalize: bool) -> torch.Tensor:
        """fp32 ``[N, D]`` -> contiguous on the engine's device; ``normalize`` divides every row by max(its norm, 1e-12) on the engine
        (keep_op_l2norm, the unit-row path of the WSI functions) in a copy."""
        check_features(features)
        self._ready_device()
        x = self._on_device(features)
        if normalize:
            if isinstance(features, torch.Tensor) and x.data_ptr() == features.data_ptr():
                x = x.clone()
            self._call("op_l2norm", _ptr(x), x.shape[0], x.shape[1])
        return x

    def _cluster_assign(self, x, cen, labels, best, margin, prev, skipped, sums, fused: bool = True) -> None:
        N, D = x.shape
        acc = (None, None, None) if sums is None else (sums.sums, sums.counts, sums.cos_sum)
        self._call("cluster_assign", _ptr(x), N, D, _ptr(cen), cen.shape[0], _ptr(labels), _ptr(best), _ptr(margin), _ptr(prev), _ptr(skipped),
                   _ptr(None if prev is None else sums.changed), _ptr(acc[0]), _ptr(acc[1]), _ptr(acc[2]), 0 if fused else 1)

    @torch.no_grad()
    def cluster_assign(self, features, centroids, sums=None, prev=None, normalize=True, fused=True):
        """Every tile's nearest centroid by cosine, in one pass over the features -> ``(labels, best, margin,
        skipped)`` on the device: int32 ``[N]`` (the first maximum; -1 for a skipped tile), fp32 ``[N]`` twice (the winning cosine and its
        lead over the runner-up, 0 when K = 1) and an int64 ``[1]`` count of skipped tiles.

        ``features``: fp32 ``[N, D]``, ``1 <= N <= 2^22``, D a multiple of 16 up to 1024; ``centroids``: fp32 ``[K, D]`` unit rows, ``1 <= K
        <= 64``.  ``normalize=True`` makes unit rows of the features first (the engine's row kernel); ``False`` takes them as they are.  A
        tile with a non-finite value or an element beyond 1 in magnitude is skipped everywhere.  ``sums``: a
        ``keep_amd.cluster.ClusterSums`` of the same K and D: the same launch adds every kept tile into its centroid's integer sums
        (``skipped`` is then ``sums.skipped``, which keeps counting until ``sums.zero_()``); ``prev``: int32 ``[N]`` earlier labels,
        with ``sums``: the tiles whose label differs are added to ``sums.changed``.  The scores are fp32 fma chains of one fixed order:
        labels, best and margin of a tile do not depend on N, its row or the split over calls, and neither do the integer sums.
        ``fused=False`` runs the accumulate as a second launch (the same words; for measurement).  No host synchronisation."""
        N, D = check_features(features)
        K, _ = check_centroids(centroids, D)
        if sums is not None:
            if not isinstance(sums, ClusterSums):
                raise ValueError(f"sums must be a ClusterSums, got {type(sums).__name__}")
            sums.check(K, D)
        if prev is not None:
            if sums is None:
                raise ValueError("prev= needs sums=: the changed labels are counted in sums.changed")
            check_prev(prev, N)
        x = self._cluster_features(features, normalize)
        if sums is not None:
            if sums.buf.device != self._device:
                raise ValueError(f"the accumulators live on {sums.buf.device}, this engine on {self._device}")
            sums.claim(N)
        cen = self._on_device(centroids)
        labels = torch.empty(N, dtype=torch.int32, device=self._device)
        best, margin = (torch.empty(N, dtype=torch.float32, device=self._device) for _ in range(2))
        skipped = torch.zeros(1, dtype=torch.int64, device=self._device) if sums is None else sums.skipped
        self._cluster_assign(x, cen, labels, best, margin, None if prev is None else self._on_device(prev), skipped, sums, fused)
        return labels, best, margin, skipped

    @torch.no_grad()
    def cluster_update(self, sums, centroids):
        """New centroids from the integer sums -> ``(centroids fp32 [K, D], empty uint8 [K])`` on the device: each
        row its cluster's sum divided by its norm in float64, rounded once; a cluster without tiles (or with a zero sum) keeps its row of
        ``centroids`` bit for bit and is flagged in ``empty``.  ``centroids`` itself is not written.  No host synchronisation."""
        if not isinstance(sums, ClusterSums):
            raise ValueError(f"sums must be a ClusterSums, got {type(sums).__name__}")
        K, D = check_centroids(centroids)
        sums.check(K, D)
        self._ready_device()
        if sums.buf.device != self._device:
            raise ValueError(f"the accumulators live on {sums.buf.device}, this engine on {self._device}")
        out = self._on_device(centroids).clone()
        empty = torch.empty(K, dtype=torch.uint8, device=self._device)
        self._call("cluster_update", _ptr(sums.sums), _ptr(sums.counts), K, D, _ptr(out), _ptr(empty))
        return out, empty

    def _cluster_seed(self, x: torch.Tensor, k: int) -> torch.Tensor:
        N, D = x.shape
        dev = self._device
        sums = ClusterSums(1, D, dev)
        zero = torch.zeros((1, D), dtype=torch.float32, device=dev)
        self._cluster_assign(x, zero, None, None, None, None, None, sums)        # K = 1: the integer mean of the kept rows
        mean, _ = self.cluster_update(sums, zero)
        idx = torch.empty(k, dtype=torch.int64, device=dev)
        nearest = torch.full((N,), float("-inf"), dtype=torch.float32, device=dev)
        self._call("cluster_seed_step", _ptr(x), N, D, _ptr(mean), _ptr(None), 1, _ptr(None), C.c_void_p(idx.data_ptr()))
        for i in range(1, k):
            self._call("cluster_seed_step", _ptr(x), N, D, _ptr(None), C.c_void_p(idx.data_ptr() + 8 * (i - 1)), 0, _ptr(nearest),
                       C.c_void_p(idx.data_ptr() + 8 * i))
        return idx

    @torch.no_grad()
    def cluster_seed(self, features, k: int, normalize=True) -> torch.Tensor:
        """Deterministic farthest-point seeding -> row indices int64 ``[k]`` on the device.  The first is the tile
        with the largest cosine to the normalised integer mean of all tiles, every next one the tile whose largest cosine to the
        centres chosen so far is the smallest; the lowest index wins every tie and skipped tiles are never chosen (-1 when every tile
        is skipped).  No random numbers; k passes over the features, the index chain stays on the device (no host synchronisation)."""
        check_features(features)
        k = check_k(k)
        return self._cluster_seed(self._cluster_features(features, normalize), k)

    def _cluster_lloyd(self, batches, k: int, D: int, cen: torch.Tensor, max_iter: int, tol_changed: int):
        """The Lloyd loop over ``batches()`` (an iterable of prepared device tensors, the same rows in the same order every time it is
        called); ``cen`` fp32 ``[k, D]`` on the device."""
        dev = self._device
        sums = ClusterSums(k, D, dev)
        bufs = []                                                       # per batch: [labels, previous labels, best, margin]

        def one_pass():
            sums.zero_()
            first, seen = not bufs, 0
            for i, x in enumerate(batches()):
                seen += 1
                if i == len(bufs):
                    if not first:
                        raise ValueError(f"batches() returned more than the {len(bufs)} batches of its first call")
                    N = x.shape[0]
                    bufs.append([torch.empty(N, dtype=torch.int32, device=dev), torch.full((N,), -1, dtype=torch.int32, device=dev),
                                 torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.float32, device=dev)])
                b = bufs[i]
                if b[0].shape[0] != x.shape[0]:
                    raise ValueError(f"batch {i} has {x.shape[0]} rows, it had {b[0].shape[0]} in the first pass")
                sums.claim(x.shape[0])
                self._cluster_assign(x, cen, b[0], b[2], b[3], b[1], sums.skipped, sums)
            if not bufs or seen != len(bufs):
                raise ValueError(f"batches() returned {seen} batches, {len(bufs)} in its first call (at least one is needed)")

        n_iter, converged = 0, False
        for it in range(1, max_iter + 1):
            one_pass()
            n_iter = it
            if int(sums.changed.item()) <= tol_changed:                  # the iteration's one host synchronisation
                converged = True
                break
            cen, _ = self.cluster_update(sums, cen)
            for b in bufs:
                b[0], b[1] = b[1], b[0]
        if not converged:
            one_pass()
        tail = sums.buf[k * D:].cpu()
        counts, (cos_sum, changed, skipped) = tail[:k], (int(v) for v in tail[k:])
        kept = int(counts.sum())
        cat = lambda j: bufs[0][j] if len(bufs) == 1 else torch.cat([b[j] for b in bufs])
        return TileClusters(cat(0), cat(2), cat(3), cen, sums.counts.clone(), skipped, sums.counts == 0, n_iter, changed,
                            (cos_sum / CLUSTER_ONE / kept) if kept else 0.0, converged)

    @torch.no_grad()
    def cluster_tiles(self, features, k: int, init="farthest", max_iter: int = 50, tol_changed: int = 0):
        """Spherical k-means of a slide's tiles on the device -> ``keep_amd.cluster.TileClusters``.

        ``features``: fp32 ``[N, D]`` (made unit rows first); ``k`` in 1..64; ``init``: ``"farthest"`` (:meth:`cluster_seed`), fp32
        centroids ``[k, D]`` (taken as they are: unit rows) or integer row indices ``[k]``.  Every iteration is one fused assign +
        accumulate launch and one update launch; the host reads the number of changed labels once per iteration, the only
        synchronisation, and stops when it is ``<= tol_changed`` or after ``max_iter`` iterations (then one more assign gives the labels of
        the final centroids).  An empty cluster keeps its centroid.  No random numbers and integer sums: two runs give the same bits,
        and :meth:`cluster_fit_batches` over any split of the same tiles gives them too.  Equal to ``keep_amd.cluster.kmeans_numpy``
        wherever its float64 margins stay above the fp32 error of a length-D dot product."""
        N, D = check_features(features)
        k = check_k(k)
        max_iter, tol_changed = check_fit_args(max_iter, tol_changed)
        kind = check_init(init, k, N, D)
        x = self._cluster_features(features, True)
        if kind == "centroids":
            cen = self._on_device(init if hasattr(init, "shape") else np.asarray(init, np.float32)).clone()
        else:
            idx = self._cluster_seed(x, k) if kind == "farthest" else self._on_device(torch.as_tensor(init), torch.int64)
            cen = x[idx.clamp(min=0)].contiguous()
        return self._cluster_lloyd(lambda: (x,), k, D, cen, max_iter, tol_changed)

    @torch.no_grad()
    def cluster_fit_batches(self, batches, k: int, init, max_iter: int = 50, tol_changed: int = 0):
        """:meth:`cluster_tiles` for features that are never resident at once (a cohort of feature files) -> ``TileClusters`` over the
        concatenation of the batches.  ``batches``: a callable returning an iterable of fp32 ``[n_i, D]`` tensors, called once per
        iteration and returning the same rows in the same order each time; ``init``: fp32 centroids ``[k, D]`` (unit rows).  One
        ``ClusterSums`` is accumulated over an iteration's batches (at most 2^24 tiles), so the result equals ``cluster_tiles`` on the
        concatenation with the same ``init`` bit for bit."""
        k = check_k(k)
        max_iter, tol_changed = check_fit_args(max_iter, tol_changed)
        if not callable(batches):
            raise ValueError(f"batches must be a callable returning the feature tensors, got {type(batches).__name__}")
        if isinstance(init, str) or not hasattr(init, "shape") or len(tuple(init.shape)) != 2:
            raise ValueError(f"init must be centroids [k, D] here (seed on a resident sample with cluster_seed), got {init!r}")
        D = check_dim(init.shape[1])
        check_init(init, k, 1, D)
        self._ready_device()
        cen = self._on_device(init).clone()

        def prepared():
            for x in batches():
                if check_features(x)[1] != D:
                    raise ValueError(f"a batch has width {x.shape[1]}, the centroids {D}")
                yield self._cluster_features(x, True)
        return self._cluster_lloyd(prepared, k, D, cen, max_iter, tol_changed)

    # ------------------------------------------------------------------ linear probe
    def _probe_params(self, weight, bias, D: int, values: bool = True):
        """fp32 weight ``[C, D]`` / bias ``[C]`` checked on the host (shapes; with ``values`` finite and the norm limit, which reads
        device tensors back) -> (C, device weight, device bias)."""
        C_, _ = _probe.check_weights(weight, bias, D, values)
        return C_, self._on_device(weight), self._on_device(bias)

    @torch.no_grad()
    def probe_loss_grad(self, features, labels, weight, bias, sums, class_weight=None, normalize=True, forward=False, groups=0):
        """One loss + gradient evaluation of the linear probe on the device: every kept row's softmax residual
        is added into ``sums`` (a ``keep_amd.probe.ProbeSums`` of the same C and D) in one pass over the features.

        ``features``: fp32 ``[N, D]`` as in :meth:`cluster_assign` (``normalize=True`` makes unit rows first); ``labels``: int32 ``[N]``,
        -1 for an unlabelled row (in no sum) or ``0 .. C - 1``, anything else is an error the call reports after one 4-byte read-back;
        ``weight`` fp32 ``[C, D]``, ``bias`` fp32 ``[C]``, ``2 <= C <= 64``; ``class_weight``: None or fp32 ``[C]`` in (0, 1]
        (``keep_amd.probe.check_class_weight`` makes one).  The sums are integers, every term rounded before it is added: the same words
        however the rows are split over calls; ``keep_amd.probe.objective_from_words`` turns them into the objective and its gradient.
        ``forward=True`` returns ``(labels, probs, best, margin)`` of the same launch as :meth:`probe_predict` would, otherwise None.
        ``groups``: 0, or 1 / 2 / 4 groups of 64 rows per workgroup (the same words; for measurement)."""
        N, D = check_features(features)
        _probe.check_labels(labels, N)
        C_, w, b = self._probe_params(weight, bias, D)
        if not isinstance(sums, _probe.ProbeSums):
            raise ValueError(f"sums must be a ProbeSums, got {type(sums).__name__}")
        sums.check(C_, D)
        cw = None
        if class_weight is not None:
            cw = class_weight if isinstance(class_weight, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(class_weight))
            if tuple(cw.shape) != (C_,) or cw.dtype != torch.float32:
                raise ValueError(f"class_weight must be float32 [{C_}], got {cw.dtype} {tuple(cw.shape)}")
        x = self._cluster_features(features, normalize)
        if sums.buf.device != self._device:
            raise ValueError(f"the accumulators live on {sums.buf.device}, this engine on {self._device}")
        sums.claim(N)
        y = self._on_device(labels)
        cw = None if cw is None else self._on_device(cw)
        out = (None, None, None, None)
        if forward:
            out = (torch.empty(N, dtype=torch.int32, device=self._device), torch.empty((N, C_), dtype=torch.float32, device=self._device),
                   torch.empty(N, dtype=torch.float32, device=self._device), torch.empty(N, dtype=torch.float32, device=self._device))
        self._call("probe_loss_grad", _ptr(x), N, D, _ptr(y), _ptr(w), _ptr(b), C_, _ptr(cw), _ptr(sums.grad), _ptr(sums.gbias), _ptr(sums.loss),
                   _ptr(sums.counts), _ptr(sums.skipped), _ptr(out[1]), _ptr(out[0]), _ptr(out[2]), _ptr(out[3]), int(groups))
        return out if forward else None

    @torch.no_grad()
    def probe_predict(self, probe, features, normalize=True, groups=0):
        """The linear probe's forward on the device -> ``(labels, probs, margin, skipped)``: int32 ``[N]`` (the
        first maximum of the logits; -1 for a skipped tile), fp32 ``[N, C]`` (softmax; a zero row for a skipped tile), fp32 ``[N]`` (the
        winner's probability minus the runner-up's) and an int64 ``[1]`` count of skipped tiles.  ``probe``: a
        ``keep_amd.probe.LinearProbe`` or a ``(weight fp32 [C, D], bias fp32 [C])`` pair; ``features`` as in :meth:`cluster_assign`.  The
        logits are fp32 fma chains of one fixed order plus the bias: a tile's outputs do not depend on N, its row or the split over
        calls.  No host synchronisation."""
        N, D = check_features(features)
        weight, bias = (probe.weight, probe.bias) if isinstance(probe, _probe.LinearProbe) else probe
        C_, w, b = self._probe_params(weight, bias, D, values=False)
        x = self._cluster_features(features, normalize)
        labels = torch.empty(N, dtype=torch.int32, device=self._device)
        probs = torch.empty((N, C_), dtype=torch.float32, device=self._device)
        margin = torch.empty(N, dtype=torch.float32, device=self._device)
        skipped = torch.zeros(1, dtype=torch.int64, device=self._device)
        self._call("probe_forward", _ptr(x), N, D, _ptr(w), _ptr(b), C_, _ptr(probs), _ptr(labels), _ptr(None), _ptr(margin), _ptr(skipped),
                   int(groups))
        return labels, probs, margin, skipped

    def _probe_fit(self, batches, C_: int, D: int, l2: float, cw: np.ndarray, gtol: float, max_iter: int, init, classes):
        """L-BFGS on the host over ``batches()`` (an iterable of prepared device ``(features, labels)`` pairs, the same rows in the
        same order every time it is called).  Every evaluation streams all batches into one ``ProbeSums`` and reads it back once."""
        dev = self._device
        sums = _probe.ProbeSums(C_, D, dev)
        cwd = torch.from_numpy(cw).to(dev)
        cd = C_ * D
        last = {}

        def split(theta):
            return theta[:cd].reshape(C_, D), theta[cd:]

        def fun(theta):
            w64, b64 = split(theta)
            w32, b32 = w64.astype(np.float32), b64.astype(np.float32)
            _probe.check_weights(w32, b32, D)
            wd, bd = torch.from_numpy(w32).to(dev), torch.from_numpy(b32).to(dev)
            sums.zero_()
            for x, y in batches():
                sums.claim(x.shape[0])
                self._call("probe_loss_grad", _ptr(x), x.shape[0], D, _ptr(y), _ptr(wd), _ptr(bd), C_, _ptr(cwd), _ptr(sums.grad), _ptr(sums.gbias),
                           _ptr(sums.loss), _ptr(sums.counts), _ptr(sums.skipped), _ptr(None), _ptr(None), _ptr(None), _ptr(None), 0)
            if sums.tiles == 0:
                raise ValueError("batches() returned no rows")
            words = sums.host()                                          # the evaluation's one read of the sums
            f, gw, gb = _probe.objective_from_words(words, cw, w64, b64, l2)
            last.update(words=words, weight=wd, bias=bd, theta=theta.copy())
            return f, np.concatenate([gw.ravel(), gb])

        w0, b0 = _probe.check_init(init, C_, D)
        res = _probe.lbfgs(fun, np.concatenate([w0.ravel(), b0]), gtol, max_iter, noise=lambda th: _probe.loss_noise(*split(th)))
        if not np.array_equal(last["theta"], res.theta):                # a stall: the accepted point is not the last one tried
            fun(res.theta)
        words = last["words"]
        return _probe.LinearProbe(last["weight"], last["bias"], l2, cw, classes, res.n_iter, res.n_eval, res.converged, res.stop_reason,
                                  float(res.f), float(np.abs(res.g).max()), torch.from_numpy(words["counts"].copy()).to(dev),
                                  int(words["skipped"]))

    def _probe_labels(self, labels, n: int) -> torch.Tensor:
        """Integer labels ``[n]`` of any integer type, numpy or torch -> int32 on the device."""
        y = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.array(labels))       # a copy: the caller's may be read-only
        if tuple(y.shape) != (n,) or y.dtype.is_floating_point or y.dtype.is_complex or y.dtype == torch.bool:
            raise ValueError(f"labels must be integers [{n}], got {y.dtype} {tuple(y.shape)}")
        return y.to(self._device, torch.int32).contiguous()

    @torch.no_grad()
    def probe_fit(self, features, labels, n_classes: int, l2: float = 1e-3, class_weight=None, gtol: float = 1e-4, max_iter: int = 1000,
                  init=None, classes=None):
        """Fit a linear probe on frozen features -> ``keep_amd.probe.LinearProbe``: multinomial logistic
        regression with L2, ``F = (1/S) sum_i w[y_i] (logsumexp(z_i) - z_i[y_i]) + (l2/2) |W|^2``, the bias not penalised; with
        ``class_weight=None`` and C >= 3 this is sklearn's ``LogisticRegression(C=1 / (l2 n))``.

        ``features``: fp32 ``[N, D]`` (made unit rows first); ``labels``: integers ``[N]``, -1 for a tile to leave out; ``n_classes`` in
        2..64; ``class_weight``: None, ``"balanced"`` or ``[C]`` positive numbers (divided by their maximum).  The parameters live on the
        host in float64 and L-BFGS (memory 10) runs there; every evaluation is one pass over the features on the device and one
        read of the integer sums.  It stops when the gradient's largest magnitude is ``<= gtol``, after ``max_iter`` iterations, or when
        the line search stalls in the fp32 evaluation noise (``stop_reason="stalled"``, not an error).  Integer sums and no random
        numbers: two fits give the same bits, and :meth:`probe_fit_batches` over any split of the same tiles gives them too."""
        N, D = check_features(features)
        C_ = _probe.check_n_classes(n_classes)
        l2, gtol, max_iter = _probe.check_fit(l2, gtol, max_iter)
        classes = check_class_names(classes, C_)
        self._ready_device()
        y = self._probe_labels(labels, N)
        counts = torch.bincount(y[y >= 0].to(torch.int64), minlength=C_)[:C_] if isinstance(class_weight, str) else None
        cw = _probe.check_class_weight(class_weight, C_, counts)
        x = self._cluster_features(features, True)
        return self._probe_fit(lambda: ((x, y),), C_, D, l2, cw, gtol, max_iter, init, classes)

    @torch.no_grad()
    def probe_fit_batches(self, batches, n_classes: int, dim: int, l2: float = 1e-3, class_weight=None, gtol: float = 1e-4,
                          max_iter: int = 1000, init=None, classes=None):
        """:meth:`probe_fit` for features that are never resident at once (a cohort of feature files) -> ``LinearProbe`` over the
        concatenation of the batches.  ``batches``: a callable returning an iterable of ``(features fp32 [n_i, dim], labels [n_i])``
        pairs, called once per evaluation (and once more for ``class_weight="balanced"``) and returning the same rows in the same order
        each time.  One ``ProbeSums`` is accumulated over an evaluation's batches (at most 2^24 tiles); the sums are integers, so the
        result equals ``probe_fit`` on the concatenation bit for bit."""
        C_, D = _probe.check_n_classes(n_classes), check_dim(dim)
        l2, gtol, max_iter = _probe.check_fit(l2, gtol, max_iter)
        classes = check_class_names(classes, C_)
        if not callable(batches):
            raise ValueError(f"batches must be a callable returning (features, labels) pairs, got {type(batches).__name__}")
        self._ready_device()

        def prepared():
            for x, y in batches():
                if check_features(x)[1] != D:
                    raise ValueError(f"a batch has width {x.shape[1]}, dim is {D}")
                yield self._cluster_features(x, True), self._probe_labels(y, x.shape[0])
        counts = None
        if isinstance(class_weight, str):
            counts = torch.zeros(C_, dtype=torch.int64, device=self._device)
            for _, y in batches():
                y = self._probe_labels(y, len(y))
                counts += torch.bincount(y[y >= 0].to(torch.int64), minlength=C_)[:C_]
        cw = _probe.check_class_weight(class_weight, C_, counts)
        return self._probe_fit(prepared, C_, D, l2, cw, gtol, max_iter, init, classes)

    # ------------------------------------------------------------------ attention MIL
    def _mil_bags(self, features, offsets, normalize: bool = True):
        """Checked features and offsets -> (device features, int64 host offsets, device chunk table int32 [n, 3], workspace)."""
        N, D = check_features(features)
        o = _mil.check_offsets(offsets, N)
        self._ready_device()
        x = self._cluster_features(features, normalize)
        lib = _lib.load()
        table = _mil.chunk_table(o, int(lib.keep_mil_chunk()))
        chunks = torch.from_numpy(np.ascontiguousarray(table)).to(self._device)
        need = C.c_int64(0)
        _lib.check(self._handle, lib.keep_mil_workspace_bytes(self._handle, N, D, len(o) - 1, C.byref(need)), "mil_workspace_bytes")
        ws = torch.empty(int(need.value), dtype=torch.uint8, device=self._device)
        return x, o, chunks, ws

    def _mil_params(self, params, D: int, values: bool = True):
        if isinstance(params, _mil.AttentionMIL):
            params = params.params
        L, C_, _ = _mil.check_params(params, D, values)
        return L, C_, tuple(self._on_device(a) for a in params)

    def _mil_forward(self, bags, y, dev_params, L: int, hidden: bool, skipped_rows, skipped_bags) -> dict:
        x, o, chunks, ws = bags
        N, D, S = x.shape[0], x.shape[1], len(o) - 1
        V, bv, w = dev_params[:3]
        dev = self._device
        out = dict(scores=torch.empty(N, dtype=torch.float32, device=dev), attention=torch.empty(N, dtype=torch.float32, device=dev),
                   pooled=torch.empty((S, D), dtype=torch.float32, device=dev), kept_rows=torch.empty(S, dtype=torch.int32, device=dev),
                   hidden=torch.empty((N, L), dtype=torch.float32, device=dev) if hidden else None,
                   head_labels=torch.empty(S, dtype=torch.int32, device=dev))
        self._call("mil_forward", _ptr(x), N, D, _ptr(chunks), chunks.shape[0], S, _ptr(y), _ptr(V), _ptr(bv), _ptr(w), L, _ptr(out["scores"]),
                   _ptr(out["attention"]), _ptr(out["pooled"]), _ptr(out["kept_rows"]), _ptr(out["hidden"]), _ptr(out["head_labels"]),
                   _ptr(skipped_rows), _ptr(skipped_bags), _ptr(ws), ws.numel())
        return out

    @torch.no_grad()
    def mil_forward(self, features, offsets, params, labels=None, normalize=True, hidden=False) -> dict:
        """The attention pooling on the device -> a dict with ``scores`` fp32 ``[N]`` (``s_i``; -inf for a skipped
        row), ``attention`` fp32 ``[N]`` (the softmax of the scores over each bag; 0 for a skipped row), ``pooled`` fp32 ``[S, D]``
        (``z_b``; a zero row for a bag without a kept row), ``kept_rows`` int32 ``[S]``, ``head_labels`` int32 ``[S]`` (``labels[b]``, 0 without
        labels, or -1 for a bag without a kept row), ``hidden`` fp32 ``[N, L]`` (``tanh(V x + bv)``, with ``hidden=True``) and ``skipped``
        int64 ``[2]`` (rows, bags).  ``features`` fp32 ``[N, D]`` as in :meth:`cluster_assign`; ``offsets`` integers ``[S + 1]`` (bag b is the
        rows ``offsets[b] .. offsets[b + 1]``); ``params``: ``(V, bv, w, Wc, bc)`` or an ``AttentionMIL`` (the head is not used here).  A
        row's score and a bag's pooled row depend on that row and that bag alone."""
        bags = self._mil_bags(features, offsets, normalize)
        L, _, dp = self._mil_params(params, bags[0].shape[1], values=False)
        y = None if labels is None else self._probe_labels(labels, len(bags[1]) - 1)
        skipped = torch.zeros(2, dtype=torch.int64, device=self._device)
        out = self._mil_forward(bags, y, dp, L, hidden, skipped[0:1], skipped[1:2])
        out["skipped"] = skipped
        return out

    def _mil_eval(self, bags, y, dp, L: int, C_: int, cwd, sums, forward: bool = False, ds=None):
        """One loss + gradient evaluation of prepared bags into ``sums``: the pooling, the head (the probe's own launch on the pooled
        rows) and the backward -> ``(forward outputs, head probabilities, head labels)``."""
        x, o, chunks, ws = bags
        N, D, S = x.shape[0], x.shape[1], len(o) - 1
        sums.claim(S)
        f = self._mil_forward(bags, y, dp, L, True, sums.skipped_rows, sums.skipped_bags)
        V, bv, w, Wc, bc = dp
        h = sums.head
        probs = torch.empty((S, C_), dtype=torch.float32, device=self._device)
        plab = torch.empty(S, dtype=torch.int32, device=self._device) if forward else None
        self._call("probe_loss_grad", _ptr(f["pooled"]), S, D, _ptr(f["head_labels"]), _ptr(Wc), _ptr(bc), C_, _ptr(cwd), _ptr(h.grad), _ptr(h.gbias),
                   _ptr(h.loss), _ptr(h.counts), _ptr(h.skipped), _ptr(probs), _ptr(plab), _ptr(None), _ptr(None), 0)
        self._call("mil_backward", _ptr(x), N, D, _ptr(chunks), chunks.shape[0], S, _ptr(f["head_labels"]), _ptr(probs), _ptr(Wc), C_, _ptr(cwd),
                   _ptr(w), L, _ptr(f["scores"]), _ptr(f["attention"]), _ptr(f["pooled"]), _ptr(f["hidden"]), _ptr(sums.gV), _ptr(sums.gbv),
                   _ptr(sums.gw), _ptr(ds), _ptr(ws), ws.numel())
        return f, probs, plab

    @staticmethod
    def _mil_mask(f: dict, labels, probs):
        """A bag without a kept row: label -1 and a zero row of probabilities, whatever the head made of its zero pooled row."""
        gone = f["kept_rows"] == 0
        return labels.masked_fill(gone, -1), probs.masked_fill(gone[:, None], 0.0)

    @torch.no_grad()
    def mil_loss_grad(self, features, offsets, labels, params, sums, class_weight=None, normalize=True, forward=False, detail=False):
        """One loss + gradient evaluation of the attention MIL model on the device, added into ``sums`` (a
        ``keep_amd.mil.MilSums`` of the same L, C and D).  ``features`` / ``offsets`` / ``params`` as in :meth:`mil_forward`; ``labels``:
        integers ``[S]``, -1 for a bag to leave out; ``class_weight``: None or fp32 ``[C]`` in (0, 1].  The words are integers and a bag's
        contribution to each depends on that bag alone: the same words for every split of the bags over calls, in any order;
        ``keep_amd.mil.objective_from_words`` turns them into the objective and its gradient.  ``forward=True`` returns
        ``(labels, probs, attention)`` as :meth:`mil_predict` would, otherwise None; ``detail=True`` returns every intermediate instead:
        the dict of :meth:`mil_forward` (with ``hidden``) plus ``probs`` fp32 ``[S, C]`` as the head wrote them and ``ds`` fp32 ``[N]``, the
        derivative of the unnormalised loss by each row's score."""
        bags = self._mil_bags(features, offsets, normalize)
        D, S = bags[0].shape[1], len(bags[1]) - 1
        L, C_, dp = self._mil_params(params, D)
        if not isinstance(sums, _mil.MilSums):
            raise ValueError(f"sums must be a MilSums, got {type(sums).__name__}")
        sums.check(L, C_, D)
        if sums.buf.device != self._device:
            raise ValueError(f"the accumulators live on {sums.buf.device}, this engine on {self._device}")
        cw = None
        if class_weight is not None:
            cw = class_weight if isinstance(class_weight, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(class_weight))
            if tuple(cw.shape) != (C_,) or cw.dtype != torch.float32:
                raise ValueError(f"class_weight must be float32 [{C_}], got {cw.dtype} {tuple(cw.shape)}")
            cw = self._on_device(cw)
        y = self._probe_labels(labels, S)
        ds = torch.empty(bags[0].shape[0], dtype=torch.float32, device=self._device) if detail else None
        f, probs, plab = self._mil_eval(bags, y, dp, L, C_, cw, sums, forward, ds)
        if detail:
            return dict(f, probs=probs, ds=ds)
        return (*self._mil_mask(f, plab, probs), f["attention"]) if forward else None

    @torch.no_grad()
    def mil_predict(self, mil, features, offsets, normalize=True):
        """The attention MIL forward on the device -> ``(labels, probs, attention, skipped)``: int32 ``[S]`` (the
        first maximum of the bag's logits; -1 for a bag without a kept row), fp32 ``[S, C]`` (a zero row for such a bag), fp32 ``[N]`` (the
        tiles' attention within their bag; 0 for a skipped tile) and int64 ``[2]`` (skipped rows, skipped bags).  ``mil``: an
        ``AttentionMIL`` or ``(V, bv, w, Wc, bc)``."""
        bags = self._mil_bags(features, offsets, normalize)
        D, S = bags[0].shape[1], len(bags[1]) - 1
        L, C_, dp = self._mil_params(mil, D, values=False)
        skipped = torch.zeros(2, dtype=torch.int64, device=self._device)
        f = self._mil_forward(bags, None, dp, L, False, skipped[0:1], skipped[1:2])
        labels = torch.empty(S, dtype=torch.int32, device=self._device)
        probs = torch.empty((S, C_), dtype=torch.float32, device=self._device)
        self._call("probe_forward", _ptr(f["pooled"]), S, D, _ptr(dp[3]), _ptr(dp[4]), C_, _ptr(probs), _ptr(labels), _ptr(None), _ptr(None), _ptr(None), 0)
        return (*self._mil_mask(f, labels, probs), f["attention"], skipped)

    def _mil_fit(self, batches, L: int, C_: int, D: int, l2: float, cw: np.ndarray, lr: float, n_steps: int, seed: int, init, classes):
        """Adam on the host over ``batches()`` (an iterable of prepared ``(bags, labels)`` pairs, the same bags every time it is called).
        Every evaluation streams all batches into one ``MilSums`` and reads it back once."""
        dev = self._device
        sums = _mil.MilSums(L, C_, D, dev)
        cwd = torch.from_numpy(cw).to(dev)
        last = {}

        def fun(theta):
            p64 = _mil.unpack(theta, L, C_, D)
            p32 = tuple(np.ascontiguousarray(a, np.float32) for a in p64)
            _mil.check_params(p32, D)
            dp = tuple(torch.from_numpy(a).to(dev) for a in p32)
            sums.zero_()
            for bags, y in batches():
                self._mil_eval(bags, y, dp, L, C_, cwd, sums)
            if sums.bags == 0:
                raise ValueError("batches() returned no bags")
            words = sums.host()                                          # the evaluation's one read of the sums
            f, g = _mil.objective_from_words(words, cw, p64, l2)
            last.update(words=words, params=dp)
            return f, _mil.pack(g)

        theta0 = _mil.pack(_mil.init_params(seed, L, C_, D) if init is None else init)
        if theta0.shape != (sum(_mil.sizes(L, C_, D)),):
            raise ValueError(f"init must be (V [{L}, {D}], bv [{L}], w [{L}], Wc [{C_}, {D}], bc [{C_}])")
        res = _mil.adam(fun, theta0, lr, n_steps)
        words = last["words"]
        return _mil.AttentionMIL(*last["params"], l2, cw, classes, lr, n_steps, seed, res.history, float(res.f), float(np.abs(res.g).max()),
                                 torch.from_numpy(words["head"]["counts"].copy()).to(dev), words["skipped_rows"], words["skipped_bags"])

    @torch.no_grad()
    def mil_fit(self, features, offsets, labels, n_classes: int, hidden: int = 64, l2: float = 1e-4, class_weight=None, lr: float = 0.01,
                n_steps: int = 300, seed: int = 0, init=None, classes=None):
        """Fit attention-based multiple-instance learning on frozen features -> ``keep_amd.mil.AttentionMIL``.

        ``features``: fp32 ``[N, D]`` (made unit rows first); ``offsets``: integers ``[S + 1]``; ``labels``: integers ``[S]``, -1 for a slide
        to leave out; ``n_classes`` in 2..64; ``hidden``: a multiple of 16 in 16..128; ``class_weight``: None, ``"balanced"`` (over the
        labelled bags) or ``[C]`` positive numbers.  The parameters live on the host in float64 and full-batch Adam (``lr``, ``n_steps``)
        runs there from initial values drawn by a counter-based generator of ``seed`` (or from ``init``, an ``AttentionMIL`` or the five
        arrays); every evaluation is one pass on the device and one read of the integer sums.  Two fits give the same bits, and
        :meth:`mil_fit_batches` over any split of the same bags gives them too."""
        C_, L = _probe.check_n_classes(n_classes), _mil.check_hidden(hidden)
        l2, _, _ = _probe.check_fit(l2, 1.0, 0)
        lr, n_steps = _mil.check_adam(lr, n_steps)
        classes = check_class_names(classes, C_)
        bags = self._mil_bags(features, offsets, True)
        y = self._probe_labels(labels, len(bags[1]) - 1)
        counts = torch.bincount(y[y >= 0].to(torch.int64), minlength=C_)[:C_] if isinstance(class_weight, str) else None
        cw = _probe.check_class_weight(class_weight, C_, counts)
        init = init.params if isinstance(init, _mil.AttentionMIL) else init
        return self._mil_fit(lambda: ((bags, y),), L, C_, bags[0].shape[1], l2, cw, lr, n_steps, seed, init, classes)

    @torch.no_grad()
    def mil_fit_batches(self, batches, n_classes: int, dim: int, hidden: int = 64, l2: float = 1e-4, class_weight=None, lr: float = 0.01,
                        n_steps: int = 300, seed: int = 0, init=None, classes=None):
        """:meth:`mil_fit` for a cohort that is never resident at once (feature files) -> ``AttentionMIL`` over all the bags.
        ``batches``: a callable returning an iterable of ``(features fp32 [n_i, dim], offsets [s_i + 1], labels [s_i])`` triples (whole
        bags: a bag is never split over batches), called once per evaluation (and once more for ``class_weight="balanced"``) and
        returning the same bags each time, in any order.  The sums are integers and a bag's contribution depends on that bag alone, so
        the result equals ``mil_fit`` on the concatenation bit for bit."""
        C_, D, L = _probe.check_n_classes(n_classes), check_dim(dim), _mil.check_hidden(hidden)
        l2, _, _ = _probe.check_fit(l2, 1.0, 0)
        lr, n_steps = _mil.check_adam(lr, n_steps)
        classes = check_class_names(classes, C_)
        if not callable(batches):
            raise ValueError(f"batches must be a callable returning (features, offsets, labels) triples, got {type(batches).__name__}")
        self._ready_device()

        def prepared():
            for x, o, y in batches():
                if check_features(x)[1] != D:
                    raise ValueError(f"a batch has width {x.shape[1]}, dim is {D}")
                bags = self._mil_bags(x, o, True)
                yield bags, self._probe_labels(y, len(bags[1]) - 1)
        counts = None
        if isinstance(class_weight, str):
            counts = torch.zeros(C_, dtype=torch.int64, device=self._device)
            for _, _, y in batches():
                y = self._probe_labels(y, len(y))
                counts += torch.bincount(y[y >= 0].to(torch.int64), minlength=C_)[:C_]
        cw = _probe.check_class_weight(class_weight, C_, counts)
        init = init.params if isinstance(init, _mil.AttentionMIL) else init
        return self._mil_fit(prepared, L, C_, D, l2, cw, lr, n_steps, seed, init, classes)

    # ------------------------------------------------------------------ feature PCA
    def _pca_moments(self, x: torch.Tensor, sums, gram: bool = True, groups: int = 0) -> None:
        self._call("pca_moments", _ptr(x), x.shape[0], x.shape[1], _ptr(sums.centre_dev), _ptr(sums.sum), _ptr(sums.count),
                   _ptr(sums.gram if gram else None), _ptr(sums.skipped), groups)

    @torch.no_grad()
    def pca_moments(self, features, sums, normalize=True, groups=0):
        """The integer moments of the tiles' features, added into ``sums`` (a ``keep_amd.pca.PcaSums``) in one call (DESIGN.md section
        30) -> ``sums``.  ``features``: fp32 ``[N, D]``, ``1 <= N <= 2^22``, D a multiple of 16 up to 1024; ``normalize`` as in
        :meth:`cluster_assign`.  ``sums.sum`` and ``sums.count`` are the same words for every order and split of the rows; the words of
        ``sums.gram`` (about ``sums.centre``) depend on where the chunks of ``keep_pca_chunk()`` rows fall, counted from row 0 of every
        call, and on nothing else: not on ``groups`` (the chunks a workgroup walks before its atomics; for measurement), the order
        of the calls or a split at multiples of the chunk.  A tile with a non-finite value or an element beyond 1 in magnitude is
        in no sum and counted in ``sums.skipped``.  No host synchronisation."""
        N, D = check_features(features)
        if not isinstance(sums, _pca.PcaSums):
            raise ValueError(f"sums must be a PcaSums, got {type(sums).__name__}")
        sums.check(D)
        groups = _pca.check_groups(groups)
        x = self._cluster_features(features, normalize)
        if sums.buf.device != self._device:
            raise ValueError(f"the accumulators live on {sums.buf.device}, this engine on {self._device}")
        sums.claim(N)
        self._pca_moments(x, sums, True, groups)
        return sums

    def _pca_fit(self, batches, k: int, D: int, two_pass: bool):
        """``batches()``: an iterable of prepared device tensors, the same rows in the same order every time it is called."""
        chunk = _lib.load().keep_pca_chunk()

        def one_pass(sums, gram):
            prev = None
            for i, x in enumerate(batches()):
                if prev is not None:
                    _pca.check_batch_rows(prev, i - 1, chunk)
                prev = int(x.shape[0])
                sums.claim(prev)
                self._pca_moments(x, sums, gram)
            if prev is None:
                raise ValueError("batches() returned no batch (at least one is needed)")

        centre = None
        if two_pass:
            first = _pca.PcaSums(D, None, self._device)
            one_pass(first, False)
            tail = first.buf.cpu().numpy()                               # the fit's first host synchronisation
            _pca.check_kept_rows(int(tail[-2]))
            centre = _pca.centre_from_sums(tail[:D], int(tail[-2]))
        sums = _pca.PcaSums(D, centre, self._device)
        one_pass(sums, True)
        words = torch.cat([sums.sum, sums.gram_full().reshape(-1), sums.count, sums.skipped]).cpu().numpy()
        return _pca.pca_from_sums(words[:D], words[D:D + D * D].reshape(D, D), int(words[-2]), int(words[-1]), k, centre)

    @torch.no_grad()
    def pca_fit(self, features, k: int, two_pass=True, normalize=True):
        """The principal components of the tiles' features -> ``keep_amd.pca.FeaturePCA``.

        ``features``: fp32 ``[N, D]`` as in :meth:`pca_moments`; ``k`` in 1..64.  With ``two_pass`` the first pass over the features takes
        the integer sum and count alone, the second the Gram about ``fp32(mean)``, so that the shifted-data formula ``(G - n (mu - c)(mu
        - c)^T) / (n - 1)`` cancels nothing; ``two_pass=False`` is one pass about a zero centre, which loses the small eigenvalues to the
        features' common mean.  The D x D ``eigh`` runs on the host in float64.  Integer moments: two runs give the same bits, and
        :meth:`pca_fit_batches` over a split at multiples of ``keep_pca_chunk()`` gives them too.  Fewer than two kept tiles is an
        error."""
        N, D = check_features(features)
        k = _pca.check_k(k, D)
        x = self._cluster_features(features, normalize)
        return self._pca_fit(lambda: (x,), k, D, bool(two_pass))

    @torch.no_grad()
    def pca_fit_batches(self, batches, k: int, dim: int, two_pass=True):
        """:meth:`pca_fit` for features that are never resident at once -> ``FeaturePCA`` over the concatenation of the batches.
        ``batches``: a callable returning a fresh iterable of fp32 ``[n_i, dim]`` tensors (made unit rows here), called twice under
        ``two_pass`` and returning the same rows in the same order each time.  Every batch except the last must hold a multiple of
        ``keep_pca_chunk()`` rows (a ``ValueError`` otherwise): the chunk boundaries then fall where they fall in the concatenation
        and the result equals ``pca_fit`` on it bit for bit."""
        D = check_dim(dim)
        k = _pca.check_k(k, D)
        if not callable(batches):
            raise ValueError(f"batches must be a callable returning the feature tensors, got {type(batches).__name__}")
        self._ready_device()

        def prepared():
            for x in batches():
                if check_features(x)[1] != D:
                    raise ValueError(f"a batch has width {x.shape[1]}, dim is {D}")
                yield self._cluster_features(x, True)
        return self._pca_fit(prepared, k, D, bool(two_pass))

    @torch.no_grad()
    def pca_transform(self, pca, features, k=None, whiten=False, normalize=True):
        """The tiles' scores on the first ``k`` components of a ``FeaturePCA`` -> ``(scores fp32 [N, k], kept bool
        [N])`` on the device.  ``scores[i, j] = fp32(chain_j(x_i) + bias[j])`` with ``chain_j`` the fp32 fma chain of :meth:`cluster_assign`
        on component j and ``bias[j] = fp32(-(mean . w_j))``; ``whiten`` multiplies by ``fp32(1 / sqrt(lambda_j))``.  A tile's scores
        depend on that tile alone; a skipped tile gives a zero row and ``kept = False``.  No host synchronisation."""
        if not isinstance(pca, _pca.FeaturePCA):
            raise ValueError(f"pca must be a FeaturePCA, got {type(pca).__name__}")
        N, D = check_features(features)
        if D != pca.dim:
            raise ValueError(f"the features have width {D}, the PCA {pca.dim}")
        k = pca.k if k is None else _pca.check_k(k, pca.k)
        x = self._cluster_features(features, normalize)
        w = self._on_device(np.ascontiguousarray(pca.components[:k], np.float32))
        bias = self._on_device(pca.bias(k))
        scale = self._on_device(pca.whiten_scale(k)) if whiten else None
        return self._pca_project(x, w, bias, scale)

    def _pca_project(self, x, w, bias, scale):
        N, k = x.shape[0], w.shape[0]
        out = torch.empty((N, k), dtype=torch.float32, device=self._device)
        kept = torch.empty(N, dtype=torch.uint8, device=self._device)
        self._call("pca_project", _ptr(x), N, x.shape[1], _ptr(w), k, _ptr(bias), _ptr(scale), _ptr(out), _ptr(kept), _ptr(None))
        return out, kept.view(torch.bool)

    @torch.no_grad()
    def render_rgb_map(self, class_raster, thumbnail=None, planes=(0, 1, 2), alpha: float = 0.6, tissue=None,
                       background=(255, 255, 255)) -> torch.Tensor:
        """Three planes of a ``ClassRaster`` as one colour picture over the thumbnail -> uint8 [h,w,3] on the
        device: red, green and blue are the exact means of ``planes`` (0..1 mapped to 0..255 by :meth:`render_heatmap`'s integer
        division), blended with ``round(256 alpha)``; pixels no tile covers or outside ``tissue`` keep the thumbnail or
        ``background``.  ``thumbnail`` as in :meth:`render_heatmap`.  Equal to ``keep_amd.pca.render_rgb_numpy`` bit for bit."""
        if not isinstance(class_raster, ClassRaster):
            raise ValueError(f"class_raster must be a ClassRaster, got {type(class_raster).__name__}")
        a, _, _, _, bg = render_args(alpha, (0.0, 1.0), 0.0, background)
        C_, (h, w) = class_raster.n_classes, class_raster.shape
        p = _pca.check_planes(planes, C_)
        x = None
        if thumbnail is not None:
            x = torch.from_numpy(thumbnail) if not isinstance(thumbnail, torch.Tensor) else thumbnail
            if region_layout(x)[:2] != (h, w):
                raise ValueError(f"thumbnail is {tuple(x.shape[:2])}, the raster {(h, w)}")
        if tissue is not None:
            _check_tissue(tissue, class_raster)
        self._ready_device()
        self._raster_here(class_raster)
        ps, row = 3, 0
        if x is not None:
            if x.device != self._device:
                x = x.to(self._device)
            _, _, ps, row = region_layout(x)
        md = None if tissue is None else self._on_device(tissue.mask)
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=self._device)
        self._call("class_render_rgb", _ptr(class_raster.acc), C_, h, w, (C.c_int * 3)(*p), _ptr(x), row, ps, bg[0] | bg[1] << 8 | bg[2] << 16,
                   _ptr(md), a, _ptr(out))
        return out

    # ------------------------------------------------------------------ nearest neighbours
    def _neighbours(self, keys, k: int, n_bank: int, query_skipped, bank_skipped):
        """The ``Neighbours`` of device keys int64 ``[Nq, k]``: one unpack launch."""
        Nq = keys.shape[0]
        index = torch.empty((Nq, k), dtype=torch.int64, device=self._device)
        score = torch.empty((Nq, k), dtype=torch.float32, device=self._device)
        count = torch.empty(Nq, dtype=torch.int32, device=self._device)
        self._call("topk_unpack", _ptr(keys), Nq, k, _ptr(index), _ptr(score), _ptr(count))
        return _nb.Neighbours(keys, index, score, count, k, n_bank, query_skipped, bank_skipped, self)

    def _topk_merged(self, a, b):
        if a.keys.device != self._device or b.keys.device != self._device:
            raise ValueError(f"the lists live on {a.keys.device} and {b.keys.device}, this engine on {self._device}")
        self._ready_device()
        out = torch.empty_like(a.keys)
        self._call("topk_merge", _ptr(a.keys.contiguous()), _ptr(b.keys.contiguous()), a.keys.shape[0], a.k, _ptr(out))
        return self._neighbours(out, a.k, max(a.n_bank, b.n_bank), a.query_skipped.clone(), a.bank_skipped + b.bank_skipped)

    @torch.no_grad()
    def topk(self, queries, bank, k: int, normalize=True, exclude_self=False, into=None, bank_base: int = 0, self_first=None, segments: int = 0):
        """The k bank rows nearest to every query row by cosine, on the device -> ``keep_amd.neighbours.Neighbours``.
        The ``[Nq, M]`` score matrix is never written: one fused launch scores tiles of the bank and keeps every query's k best keys.

        ``queries`` fp32 ``[Nq, D]`` and ``bank`` fp32 ``[M, D]`` as the features of :meth:`cluster_assign` (``normalize=True`` makes unit
        rows of both first); ``k`` in 1..64.  A score is :meth:`cluster_assign`'s fp32 fma chain, so its bits depend on the two rows
        alone; of equal scores the lower bank row comes first.  A row with a non-finite value or an element beyond 1 in magnitude is
        skipped: such a bank row is never returned, such a query's list stays as it was (empty without ``into``).  ``bank_base``: the
        global index of ``bank[0]``; ``into``: an earlier ``Neighbours`` of the same queries against other bank rows, whose lists
        are candidates too (it is not modified); the result does not depend on how a bank is cut into calls or on their order.
        ``exclude_self=True`` (queries and bank are the same rows): no row takes itself; ``self_first``: the same for query row i
        and global row ``self_first + i``.  ``segments``: 0, or 1..1024 cuts of the bank run side by side (the same words; for
        measurement).  No host synchronisation."""
        Nq, D = check_features(queries, "queries")
        M, Db = check_features(bank, "bank")
        if D != Db:
            raise ValueError(f"the queries have width {D}, the bank {Db}")
        k, segments = _nb.check_k(k), _nb.check_segments(segments)
        bank_base = _nb.check_bank_range(bank_base, M)
        if exclude_self:
            if self_first is not None:
                raise ValueError("exclude_self=True is self_first=bank_base: give one of the two")
            if Nq != M:
                raise ValueError(f"exclude_self=True takes queries and bank of the same rows, got {Nq} and {M}")
            self_first = bank_base
        sf = _nb.check_self_first(self_first)
        if into is not None:
            if not isinstance(into, _nb.Neighbours):
                raise ValueError(f"into must be a Neighbours, got {type(into).__name__}")
            if tuple(into.keys.shape) != (Nq, k):
                raise ValueError(f"into holds lists {tuple(into.keys.shape)}, this call [{Nq}, {k}]")
        q = self._cluster_features(queries, normalize)
        b = q if bank is queries else self._cluster_features(bank, normalize)
        if into is None:
            keys = torch.empty((Nq, k), dtype=torch.int64, device=self._device)
            qs, bs = (torch.zeros(1, dtype=torch.int64, device=self._device) for _ in range(2))
            n_bank = bank_base + M
        else:
            if into.keys.device != self._device:
                raise ValueError(f"into lives on {into.keys.device}, this engine on {self._device}")
            keys, qs, bs = into.keys.clone(), into.query_skipped, into.bank_skipped.clone()
            n_bank = max(into.n_bank, bank_base + M)
        # the queries' skip count is that of the first call: the same rows are skipped in every one
        self._call("topk", _ptr(q), Nq, _ptr(b), M, D, k, bank_base, sf, 0 if into is None else 1, _ptr(keys), _ptr(qs if into is None else None),
                   _ptr(bs), segments)
        return self._neighbours(keys, k, n_bank, qs, bs)

    @torch.no_grad()
    def topk_batches(self, queries, batches, k: int, normalize=True, self_first=None):
        """:meth:`topk` against a bank that is never resident at once (a cohort's feature files) -> ``Neighbours`` over the
        concatenation of the batches, equal to the resident call bit for bit.  ``batches``: an iterable of fp32 ``[m_i, D]``; batch i's
        rows take the global indices that follow batch i - 1's.  ``self_first`` as in :meth:`topk`."""
        Nq, D = check_features(queries, "queries")
        k, sf = _nb.check_k(k), _nb.check_self_first(self_first)
        q = self._cluster_features(queries, normalize)
        keys = torch.zeros((Nq, k), dtype=torch.int64, device=self._device)
        qs, bs = (torch.zeros(1, dtype=torch.int64, device=self._device) for _ in range(2))
        base = 0
        for x in batches:
            M, Db = check_features(x, "a batch")
            if Db != D:
                raise ValueError(f"a batch has width {Db}, the queries {D}")
            _nb.check_bank_range(base, M)
            b = self._cluster_features(x, normalize)
            self._call("topk", _ptr(q), Nq, _ptr(b), M, D, k, base, sf, 1, _ptr(keys), _ptr(qs if base == 0 else None), _ptr(bs), 0)
            base += M
        if base == 0:
            raise ValueError("batches is empty")
        return self._neighbours(keys, k, base, qs, bs)

    @torch.no_grad()
    def knn_vote(self, neighbours, bank_labels, n_classes: int, weights: str = "softmax", temperature: float = 0.07):
        """The kNN classifier's vote on the device -> ``(labels, probs, margin, skipped)``: int32 ``[Nq]`` (the
        smallest class with the largest vote; -1 for a query without a voting neighbour), fp32 ``[Nq, C]`` (the vote shares; a zero row
        for such a query), fp32 ``[Nq]`` (the winner's share minus the runner-up's) and an int64 ``[1]`` count of such queries.

        ``neighbours``: a ``Neighbours``; ``bank_labels``: integers ``[n]``, ``n >= neighbours.n_bank``, indexed by global bank row; a
        label outside ``0 .. n_classes - 1`` (such as -1) does not vote.  ``weights="uniform"``: one vote each; ``"softmax"``:
        ``exp((s_r - s_0) / temperature)`` with ``s_0`` the list's best score (DINO's kNN weights up to the common factor).  The votes
        are added in list order in fp32, so the result is the same from run to run.  One 4-byte read-back (the check that every key
        names a row of ``bank_labels``) is the only host synchronisation."""
        if not isinstance(neighbours, _nb.Neighbours):
            raise ValueError(f"neighbours must be a Neighbours, got {type(neighbours).__name__}")
        C_, mode, t = _nb.check_vote_args(n_classes, weights, temperature)
        n = len(bank_labels)
        if n < neighbours.n_bank:
            raise ValueError(f"bank_labels has {n} entries, the bank {neighbours.n_bank} rows")
        self._ready_device()
        if neighbours.keys.device != self._device:
            raise ValueError(f"the lists live on {neighbours.keys.device}, this engine on {self._device}")
        y = self._probe_labels(bank_labels, n)
        Nq = neighbours.keys.shape[0]
        labels = torch.empty(Nq, dtype=torch.int32, device=self._device)
        probs = torch.empty((Nq, C_), dtype=torch.float32, device=self._device)
        margin = torch.empty(Nq, dtype=torch.float32, device=self._device)
        skipped = torch.zeros(1, dtype=torch.int64, device=self._device)
        self._call("knn_vote", _ptr(neighbours.keys.contiguous()), Nq, neighbours.k, _ptr(y), n, C_, mode, t, _ptr(probs), _ptr(labels),
                   _ptr(margin), _ptr(skipped))
        return labels, probs, margin, skipped

    # ------------------------------------------------------------------ few-shot prototypes
    @torch.no_grad()
    def fewshot_sample(self, labels, n_classes: int, shots: int, n_episodes: int, seed: int = 0, first_episode: int = 0):
        """Random support sets on the device -> ``keep_amd.fewshot.SupportSets``: for each of ``n_episodes``
        episodes (at most 2^16 per call) and each class, ``shots`` distinct training rows of that class, uniformly, or the whole class
        when it has no more than ``shots`` rows.  ``labels``: integers ``[M]``, a label outside ``0 .. n_classes - 1`` (such as -1)
        leaves the row out; the grouping by class is a stable sort on the host.  The draws come from the bootstrap's counter-based
        generator: global episode ``first_episode + i`` is the same support set whatever ``n_episodes`` or the split over calls, and
        ``support`` equals ``keep_amd.fewshot.sample_numpy`` exactly.  No host synchronisation after the upload."""
        C_, k = _fs.check_classes(n_classes), _fs.check_shots(shots)
        E, first = _fs.check_episodes(n_episodes, first_episode)
        if E > _fs.MAX_EPISODES:
            raise ValueError(f"at most 2^16 episodes per call, got {E}")
        seed = bootstrap.check_seed(seed)
        rows, offsets = _fs.class_groups(labels, C_)
        if len(rows) == 0:
            raise ValueError("no labelled training row")
        self._ready_device()
        support = torch.empty((E, C_, k), dtype=torch.int32, device=self._device)
        rows_d, offsets_d = self._on_device(rows), self._on_device(offsets)          # both alive until the launch is queued
        self._call("fewshot_sample", _ptr(rows_d), _ptr(offsets_d), C_, k, C.c_uint64(seed), first, E, _ptr(support))
        return _fs.SupportSets(support, C_, k, seed, first, rows, offsets)

    @torch.no_grad()
    def fewshot_prototypes(self, train_x, support, centre: bool = True, normalize: bool = True):
        """The class prototypes of every episode -> ``keep_amd.fewshot.Prototypes``: SimpleShot's CL2N -- the mean
        ``mu`` of an episode's support rows is subtracted, the rows are L2-normalised, and ``p_c`` is the mean of class c's rows.
        ``train_x`` fp32 ``[M, D]`` as the features of :meth:`cluster_assign`; ``support``: a ``SupportSets`` or int32 ``[E, C, shots]``
        row indices (-1 = unused slot; any ``shots`` up to 2^22 here).  A support row with a non-finite value or an element beyond 1
        is left out and counted in ``support_skipped``; a class without a kept row is invalid and never predicted.  One workgroup per
        episode adds the rows in (class, slot) order, so an episode's words depend on its own support list alone.  No host
        synchronisation."""
        M, D = check_features(train_x, "train_x")
        sup = support.support if isinstance(support, _fs.SupportSets) else support
        if not isinstance(sup, torch.Tensor) or sup.dim() != 3 or sup.dtype != torch.int32:
            raise ValueError("support must be a SupportSets or an int32 tensor [E, C, shots]")
        E, C_, k = int(sup.shape[0]), _fs.check_classes(int(sup.shape[1])), _fs.check_shots(int(sup.shape[2]), _fs.MAX_ROWS)
        if not 1 <= E <= _fs.MAX_EPISODES:
            raise ValueError(f"1..2^16 episodes per call, got {E}")
        x = self._cluster_features(train_x, normalize)
        sup = sup.to(self._device).contiguous()
        dev = self._device
        protos = _fs.Prototypes(torch.empty((E, C_ + 1, D), dtype=torch.float32, device=dev), torch.empty((E, 2 * C_ + 1), dtype=torch.float32, device=dev),
                                torch.empty((E, C_), dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int64, device=dev), bool(centre))
        self._call("fewshot_prototypes", _ptr(x), M, D, _ptr(sup), E, C_, k, 1 if centre else 0, _ptr(protos.bank), _ptr(protos.consts),
                   _ptr(protos.valid), _ptr(protos.support_skipped))
        return protos

    def _fewshot_protos(self, protos, D: int):
        E, C_, _ = _fs.check_prototypes(protos, D)
        if E > _fs.MAX_EPISODES:
            raise ValueError(f"at most 2^16 episodes per call, got {E}")
        if protos.bank.device != self._device:
            raise ValueError(f"the prototypes live on {protos.bank.device}, this engine on {self._device}")
        return E, C_, protos.bank.contiguous(), protos.consts.contiguous(), protos.valid.contiguous()

    @torch.no_grad()
    def fewshot_classify(self, protos, x, truth=None, return_labels: bool = False, normalize: bool = True, segments: int = 0):
        """Every test row against every episode's prototypes in one fused launch -> ``(confusion, labels,
        skipped)``: int64 ``[E, C, C]`` (``confusion[e, truth, label]``; None without ``truth``), int32 ``[N, E]`` (None unless
        ``return_labels``) and an int64 ``[1]`` count of skipped test rows.  ``x`` fp32 ``[N, D]`` as the features of
        :meth:`cluster_assign`; ``truth``: integers ``[N]``, -1 leaves a row out of the counts.  The label is the nearest prototype of
        the centred, normalised row among the valid classes, the first of equal ones; -1 for a skipped row or one equal to ``mu``.
        The products are f32 MFMA chains of one fixed order and the counts integers: the words do not depend on N, the grid,
        ``segments`` (0, or 1..1024 cuts of the episodes; for measurement) or the split over calls.  No ``[N, E C]`` matrix is
        written.  No host synchronisation."""
        N, D = check_features(x, "x")
        self._ready_device()
        E, C_, bank, consts, valid = self._fewshot_protos(protos, D)
        segments = _nb.check_segments(segments)
        if truth is None and not return_labels:
            raise ValueError("nothing to return: give truth, return_labels=True or both")
        f = self._cluster_features(x, normalize)
        t = None if truth is None else self._probe_labels(truth, N)
        conf = None if truth is None else torch.zeros((E, C_, C_), dtype=torch.int64, device=self._device)
        labels = torch.empty((N, E), dtype=torch.int32, device=self._device) if return_labels else None
        skipped = torch.zeros(1, dtype=torch.int64, device=self._device)
        self._call("fewshot_classify", _ptr(f), N, D, _ptr(bank), _ptr(consts), _ptr(valid), E, C_, _ptr(t), _ptr(conf), _ptr(labels), _ptr(None),
                   _ptr(None), _ptr(None), _ptr(skipped), segments)
        return conf, labels, skipped

    @torch.no_grad()
    def fewshot_fit(self, train_x, train_y, n_classes: int, shots=None, seed: int = 0, centre: bool = True):
        """A one-episode ``Prototypes``: the nearest-centroid classifier on centred, normalised features.
        ``shots=None``: every labelled row of every class (the builder walks a class's list in chunks, so no limit of 256 applies;
        one workgroup adds all rows in order); otherwise one sampled episode of ``shots`` rows per class."""
        M, _ = check_features(train_x, "train_x")
        if shots is not None:
            return self.fewshot_prototypes(train_x, self.fewshot_sample(train_y, n_classes, shots, 1, seed), centre)
        rows, offsets = _fs.class_groups(train_y, n_classes)
        if len(train_y) != M:
            raise ValueError(f"train_y has {len(train_y)} entries, train_x {M} rows")
        if len(rows) == 0:
            raise ValueError("no labelled training row")
        sizes = np.diff(offsets)
        sup = np.full((1, len(sizes), int(sizes.max())), -1, np.int32)
        for c, n in enumerate(sizes):
            sup[0, c, :n] = rows[offsets[c]:offsets[c + 1]]
        self._ready_device()
        return self.fewshot_prototypes(train_x, self._on_device(sup), centre)

    @torch.no_grad()
    def fewshot_predict(self, protos, x, normalize: bool = True):
        """A one-episode ``Prototypes`` applied to tiles -> ``(labels, scores, margin, skipped)`` as
        :meth:`probe_predict` returns them: int32 ``[N]`` (-1 for a skipped tile), fp32 ``[N, C]`` (``s_c = q . p_c - |p_c|^2 / 2 = 1/2 - |q -
        p_c|^2 / 2`` of the centred, normalised tile ``q``; -inf for an invalid class, a zero row for a skipped tile), fp32 ``[N]`` (the
        winner's score minus the runner-up's) and an int64 ``[1]`` count of skipped tiles."""
        N, D = check_features(x, "x")
        self._ready_device()
        E, C_, bank, consts, valid = self._fewshot_protos(protos, D)
        if E != 1:
            raise ValueError(f"fewshot_predict takes the prototypes of one episode, got {E}")
        f = self._cluster_features(x, normalize)
        labels = torch.empty((N, 1), dtype=torch.int32, device=self._device)
        scores = torch.empty((N, C_), dtype=torch.float32, device=self._device)
        margin = torch.empty(N, dtype=torch.float32, device=self._device)
        skipped = torch.zeros(1, dtype=torch.int64, device=self._device)
        self._call("fewshot_classify", _ptr(f), N, D, _ptr(bank), _ptr(consts), _ptr(valid), 1, C_, _ptr(None), _ptr(None), _ptr(labels), _ptr(scores),
                   _ptr(margin), _ptr(None), _ptr(skipped), 0)
        return labels.reshape(N), scores, margin, skipped

    @torch.no_grad()
    def fewshot_episodes(self, train_x, train_y, test_x, test_y, n_classes: int, shots: int, n_episodes: int = 1000, seed: int = 0,
                         first_episode: int = 0, episode_chunk=None) -> torch.Tensor:
        """The few-shot protocol -> int64 ``[E, C, C]`` on the device, the confusion of the test set under each of
        ``n_episodes`` random support sets of ``shots`` rows per class: :meth:`fewshot_sample`, :meth:`fewshot_prototypes` and
        :meth:`fewshot_classify` over chunks of ``episode_chunk`` episodes (None: 4096).  Episode e is global episode ``first_episode +
        e`` of ``seed``: the words are the same whatever ``episode_chunk``."""
        E, first = _fs.check_episodes(n_episodes, first_episode)
        C_ = _fs.check_classes(n_classes)
        chunk = 4096 if episode_chunk is None else _fs._index(episode_chunk, "episode_chunk")
        if not 1 <= chunk <= _fs.MAX_EPISODES:
            raise ValueError(f"episode_chunk must be in 1..2^16, got {chunk}")
        tx, qx = self._cluster_features(train_x, True), self._cluster_features(test_x, True)
        truth = self._probe_labels(test_y, int(qx.shape[0]))
        out = []
        for e0 in range(0, E, chunk):
            sup = self.fewshot_sample(train_y, C_, shots, min(chunk, E - e0), seed, first + e0)
            protos = self.fewshot_prototypes(tx, sup, True, normalize=False)
            out.append(self.fewshot_classify(protos, qx, truth, normalize=False)[0])
        return torch.cat(out)

    # ------------------------------------------------------------------ t-SNE tile embedding
    def _tsne_neighbours(self, neighbours):
        if not isinstance(neighbours, _nb.Neighbours):
            raise ValueError(f"neighbours must be a Neighbours, got {type(neighbours).__name__}")
        self._ready_device()
        if neighbours.keys.device != self._device:
            raise ValueError(f"the lists live on {neighbours.keys.device}, this engine on {self._device}")

    @torch.no_grad()
    def tsne_affinities(self, neighbours, perplexity) -> torch.Tensor:
        """The conditional probabilities ``p_{j|i}`` of neighbour lists at a perplexity -> fp32 ``[N, k]`` on the
        device, 0 in an empty slot; a row with fewer than two neighbours is zero.  ``neighbours``: a ``Neighbours`` (:meth:`topk` with
        ``exclude_self=True``); ``2 <= perplexity <= k / 2``.  One wave per row, 64 bisection steps, none skipped: a row's bits depend
        on that row alone.  Held to ``keep_amd.tsne.conditional_numpy``; no host synchronisation."""
        self._tsne_neighbours(neighbours)
        perp, k = _tsne.check_perplexity(perplexity, neighbours.k)
        N = _tsne.check_rows(neighbours.index.shape[0])
        p = torch.empty((N, k), dtype=torch.float32, device=self._device)
        self._call("tsne_affinities", _ptr(neighbours.index.contiguous()), _ptr(neighbours.score.contiguous()), _ptr(neighbours.count.contiguous()),
                   N, k, perp, _ptr(p))
        return p

    @torch.no_grad()
    def tsne_graph(self, neighbours, p):
        """The joint graph of :meth:`tsne_affinities`' rows -> ``(keep_amd.tsne.TsneGraph, kept bool [N])`` on the
        device.  A row is kept iff its list is not empty (the skip rule empties a skipped tile's list and never returns it as a
        neighbour); the N' kept rows are renumbered in order.  Edges ``(i, j)`` and ``(j, i)`` carry ``fp32(p_{j|i} / (2 N'))``, are sorted by
        ``row << 32 | col`` and equal keys are merged by one fp32 addition (at most two meet, so the sum has no order).  Torch plumbing,
        once per fit; reads N' and the number of edges back (two host synchronisations)."""
        self._tsne_neighbours(neighbours)
        index = neighbours.index
        N, k = index.shape
        if tuple(p.shape) != (N, k) or p.dtype != torch.float32 or p.device != self._device:
            raise ValueError(f"p must be fp32 [{N}, {k}] on {self._device}, got {p.dtype} {tuple(p.shape)} on {p.device}")
        if neighbours.n_bank > N:
            raise ValueError(f"the lists name bank rows up to {neighbours.n_bank - 1}, the graph has {N} rows: t-SNE takes the tiles' own neighbours")
        kept = neighbours.count > 0
        new = torch.cumsum(kept, 0) - 1
        m = _tsne.check_rows(int(new[-1]) + 1, "kept tiles")
        ok = (index >= 0) & (p > 0)
        ok &= kept[index.clamp(min=0)]
        rows = new[torch.arange(N, device=self._device)].unsqueeze(1).expand(N, k)[ok]
        cols = new[index[ok]]
        v = p[ok] / float(2 * m)
        keys, order = torch.sort(torch.cat([(rows << 32) | cols, (cols << 32) | rows]))
        v = torch.cat([v, v])[order]
        first = torch.ones_like(keys, dtype=torch.bool)
        first[1:] = keys[1:] != keys[:-1]
        twin = torch.zeros_like(v)
        twin[:-1] = torch.where(first[1:], torch.zeros_like(v[1:]), v[1:])        # the mirror edge of a mutual pair, next in key order
        val = (v + twin)[first].contiguous()
        keys = keys[first]
        row_ptr = torch.zeros(m + 1, dtype=torch.int64, device=self._device)
        row_ptr[1:] = torch.cumsum(torch.bincount(keys >> 32, minlength=m), 0)
        graph = _tsne.TsneGraph(row_ptr.to(torch.int32), (keys & 0xFFFFFFFF).to(torch.int32).contiguous(), val, m)
        return graph, kept

    def _tsne_graph_here(self, graph, n: int) -> None:
        if not isinstance(graph, _tsne.TsneGraph):
            raise ValueError(f"graph must be a TsneGraph, got {type(graph).__name__}")
        if graph.n != n:
            raise ValueError(f"the graph has {graph.n} rows, the embedding {n}")
        for a, dt in ((graph.row_ptr, torch.int32), (graph.col, torch.int32), (graph.val, torch.float32)):
            if not isinstance(a, torch.Tensor) or a.dtype != dt or a.device != self._device or not a.is_contiguous():
                raise ValueError(f"the graph's arrays must be contiguous int32 / int32 / fp32 tensors on {self._device} (tsne_graph makes them)")

    @torch.no_grad()
    def tsne_repulsion(self, y, out=None) -> torch.Tensor:
        """The all-pairs repulsion of an embedding in partial sums -> fp32 ``[n_seg, N, 4]`` on the device: for
        row i and segment s of ``keep_tsne_segment()`` columns the sums over the segment's j != i, ascending, of ``w^2 (y_i - y_j)``
        (words 0, 1) and ``w`` (word 2), ``w = 1 / (1 + |y_i - y_j|^2)``; word 3 is 0.  ``y``: fp32 ``[N, 2]``.  The words depend on the
        segment length and on nothing else about the launch or N.  ``out``: a buffer of that shape to write into (every word is
        written).  No host synchronisation."""
        N = _tsne.check_embedding(y)
        self._ready_device()
        yd = self._on_device(y)
        shape = (_tsne.n_segments(N, _lib.load().keep_tsne_segment()), N, 4)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self._device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != self._device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous fp32 {shape} on {self._device}")
        self._call("tsne_repulsion", _ptr(yd), N, _ptr(out))
        return out

    def _tsne_step(self, st, graph, exaggeration: float, momentum: float, lr: float, sums: torch.Tensor, stats: bool, move: bool) -> None:
        self._call("tsne_repulsion", _ptr(st.y), st.n, _ptr(st.partials))
        self._call("tsne_step", _ptr(st.y), st.n, _ptr(st.partials), _ptr(graph.row_ptr), _ptr(graph.col), _ptr(graph.val), graph.nnz,
                   exaggeration, momentum, lr, 1 if stats else 0, _ptr(sums), _ptr(st.rz), _ptr(st.grad), _ptr(st.update if move else None),
                   _ptr(st.gains if move else None), _ptr(st.spare if move else None))
        if move:
            st.y, st.spare = st.spare, st.y

    @staticmethod
    def _tsne_words(sums: torch.Tensor) -> Tuple[float, float, float]:
        """int64 [3] -> (Z, KL, squared gradient norm) as floats (reads them back)."""
        z, kl, g2 = (int(v) for v in sums.cpu())
        return z / _tsne.Z_ONE, kl / _tsne.KL_ONE, g2 / _tsne.G2_ONE

    @torch.no_grad()
    def tsne_step(self, state, graph, exaggeration: float, momentum: float, learning_rate: float, stats: bool = False):
        """One iteration on a ``keep_amd.tsne.TsneState``: the repulsion, Z, the attraction over ``graph``, the
        gradient ``4 (exaggeration A - R / Z)`` (left in ``state.grad``) and van der Maaten's update of ``state.update`` / ``gains`` / ``y``
        -> int64 ``[3]`` on the device: ``Z 2^22``, and with ``stats`` ``KL 2^40`` and ``|g|^2 2^50`` (of the embedding before the update).
        No host synchronisation."""
        if not isinstance(state, _tsne.TsneState):
            raise ValueError(f"state must be a TsneState, got {type(state).__name__}")
        self._ready_device()
        if state.y.device != self._device:
            raise ValueError(f"the state lives on {state.y.device}, this engine on {self._device}")
        self._tsne_graph_here(graph, state.n)
        sums = torch.zeros(3, dtype=torch.int64, device=self._device)
        self._tsne_step(state, graph, float(exaggeration), float(momentum), float(learning_rate), sums, bool(stats), True)
        return sums

    @torch.no_grad()
    def tsne_gradient(self, y, graph, exaggeration: float = 1.0, state=None):
        """One evaluation at an embedding -> ``(grad fp32 [N, 2] on the device, KL, Z)``: the kernels of an
        iteration without the update.  ``y``: fp32 ``[N, 2]``; ``graph``: :meth:`tsne_graph`'s.  KL is that of the plain P whatever the
        ``exaggeration``; Z is the exact value of its fixed-point word (``Z 2^22`` is an integer).  ``state``: a ``TsneState`` of N rows
        whose scratch is used (and whose ``y`` is overwritten by ``y``); one is made otherwise.  One read-back of three words."""
        N = _tsne.check_embedding(y)
        self._ready_device()
        yd = self._on_device(y)
        self._tsne_graph_here(graph, N)
        if state is None:
            state = _tsne.TsneState(yd)
        elif not isinstance(state, _tsne.TsneState) or state.n != N or state.y.device != self._device:
            raise ValueError(f"state must be a TsneState of {N} rows on {self._device}")
        else:
            state.y.copy_(yd)
        sums = torch.zeros(3, dtype=torch.int64, device=self._device)
        self._tsne_step(state, graph, float(exaggeration), 0.0, 0.0, sums, True, False)
        Z, kl, _ = self._tsne_words(sums)
        return state.grad.clone(), kl, Z

    @torch.no_grad()
    def tsne_fit(self, features=None, perplexity=20, n_iter=1000, neighbours=None, n_neighbors=None, init="pca", early_exaggeration=12.0,
                 exaggeration_iter=250, learning_rate="auto", min_grad_norm=1e-7, n_iter_without_progress=300, check_every=50, seed=0,
                 normalize=True):
        """The exact t-SNE embedding of a slide's tiles -> ``keep_amd.tsne.TileEmbedding``.

        ``features``: fp32 ``[N, D]`` as in :meth:`topk`; their ``3 perplexity`` (or ``n_neighbors``) nearest neighbours by cosine are
        taken with ``topk(..., exclude_self=True)`` unless ``neighbours`` (a ``Neighbours`` of the tiles against themselves, from
        :meth:`topk_batches` with ``self_first=0`` for features that are never resident) is given.  ``2 <= perplexity``, ``3 perplexity
        <= 64`` or ``perplexity <= n_neighbors / 2``, and below the neighbours every kept tile has.  ``init``: ``"pca"`` (``pca_fit(k=2)``
        and ``pca_transform``, scaled to a standard deviation of 1e-4 in the first column; needs ``features``), ``"random"`` (1e-4 x
        normal, counter-based from ``seed``) or an fp32 ``[N, 2]`` array.  ``early_exaggeration`` multiplies P for the first
        ``exaggeration_iter`` iterations at momentum 0.5; then momentum 0.8 with update and gains started again.  ``learning_rate="auto"``:
        ``max(N' / early_exaggeration / 4, 50)``.  Every ``check_every`` iterations the host reads the divergence and the gradient's
        norm (the only synchronisations of the descent) and, after the exaggeration, stops when the norm is at most ``min_grad_norm``
        or the divergence has not improved for ``n_iter_without_progress`` iterations.  Tiles the skip rule leaves out are compacted out
        before the fit and come back as NaN rows.  Every sum has a fixed order or is an integer: two fits give the same bits."""
        n_iter, ex_iter, every, patience = _tsne.check_iterations(n_iter, exaggeration_iter, check_every, n_iter_without_progress)
        ex0 = _tsne.check_exaggeration(early_exaggeration, "early_exaggeration")
        gmin = _tsne.check_min_grad_norm(min_grad_norm)
        seed = _tsne._boot.check_seed(seed)
        if neighbours is None:
            if features is None:
                raise ValueError("give features= or neighbours=")
            perp, k = _tsne.check_perplexity(perplexity, n_neighbors)
            N = _tsne.check_rows(check_features(features)[0])
            x = self._cluster_features(features, normalize)
            neighbours = self.topk(x, x, k, normalize=False, exclude_self=True)
        else:
            self._tsne_neighbours(neighbours)
            if n_neighbors is not None and n_neighbors != neighbours.k:
                raise ValueError(f"n_neighbors = {n_neighbors}, the lists hold {neighbours.k}")
            perp, k = _tsne.check_perplexity(perplexity, neighbours.k)
            N = _tsne.check_rows(neighbours.index.shape[0])
            if features is not None and check_features(features)[0] != N:
                raise ValueError(f"features has {features.shape[0]} rows, the lists {N}")
            x = None if features is None else self._cluster_features(features, normalize)
        start = _tsne.check_init(init, N)
        if isinstance(start, str) and start == "pca" and x is None:
            raise ValueError('init="pca" needs features= (give them beside neighbours=, or another init)')
        p = self.tsne_affinities(neighbours, perp)
        graph, kept = self.tsne_graph(neighbours, p)
        m = graph.n
        fewest = int(neighbours.count[kept].min())
        if perp >= fewest:
            raise ValueError(f"perplexity {perp:g} must be below the {fewest} neighbours the sparsest kept tile has")
        lr = _tsne.check_learning_rate(learning_rate, m, ex0)
        if isinstance(start, str) and start == "pca":
            pca = self.pca_fit(x[kept], 2, normalize=False)
            y0 = _tsne.pca_init(self.pca_transform(pca, x[kept], 2, normalize=False)[0].cpu().numpy())
        elif isinstance(start, str):
            y0 = _tsne.random_init(m, seed)
        else:
            y0 = start[kept.cpu().numpy()]
        if not np.isfinite(y0).all():
            raise ValueError("the initial embedding holds a non-finite value")
        st = _tsne.TsneState(self._on_device(y0))
        sums = torch.zeros((n_iter + 1, 3), dtype=torch.int64, device=self._device)      # a row per iteration: nothing to zero on the way
        prog = _tsne.Progress(ex_iter, patience, gmin)
        reason, done = "n_iter", n_iter
        for it in range(n_iter):
            ex, mom = _tsne.phase(it, ex_iter, ex0)
            if it == ex_iter:
                st.restart()
            check = (it + 1) % every == 0
            self._tsne_step(st, graph, ex, mom, lr, sums[it], check, True)
            if check:
                _, kl, g2 = self._tsne_words(sums[it])
                stop = prog.check(it, kl, float(np.sqrt(g2)))
                if stop is not None:
                    reason, done = stop, it + 1
                    break
        self._tsne_step(st, graph, 1.0, 0.0, 0.0, sums[n_iter], True, False)
        kl = self._tsne_words(sums[n_iter])[1]
        emb = torch.full((N, 2), float("nan"), dtype=torch.float32, device=self._device)
        emb[kept] = st.y
        return _tsne.TileEmbedding(emb, kept, np.asarray(prog.iters, np.int64), np.asarray(prog.kls, np.float64), kl, done, reason, perp, k, lr,
                                   ex0, ex_iter, start if isinstance(start, str) else "array", seed, m, graph)

    # ------------------------------------------------------------------ region table
    @torch.no_grad()
    def mask_regions(self, mask, connectivity: int = 8, min_area: int = 1, raster=None, labels: bool = True, max_regions: int = 1 << 20):
        """The connected regions of a mask, numbered, with geometry and scores, on the device ->
        ``keep_amd.components.RegionTable``.

        ``mask``: uint8 / bool [h,w], numpy or torch, host or device, non-zero = foreground, ``h w <= 2^30``; or a ``TissueMask``, which
        brings its ``downsample``.  Components are 4- or 8-connected; one is KEPT iff it holds ``>= min_area`` pixels (``min_area >= 1``;
        note that ``TissueSegmentation.min_area`` DROPS a fragment iff it holds ``<= min_area``).  The kept ones are numbered 1..n in the
        row-major order of their first pixels, which is ``scipy.ndimage.label``'s numbering with the dropped ones removed.
        ``raster``: a ``TileRaster`` of the mask's shape (and downsample, where both have one) whose sums fill the score columns;
        without one they are 0.  ``labels=False`` leaves the int32 [h,w] label image out of the result.  n is read back once to size
        the table (the one host synchronisation); more than ``max_regions`` regions is a ValueError raised before the table is
        allocated.  Everything is integer arithmetic, equal to ``keep_amd.components.regions_numpy`` bit for bit and the same from
        run to run."""
        connectivity, min_area, max_regions = check_regions_args(connectivity, min_area, max_regions)
        m, d = mask_tensor(mask)
        h, w = int(m.shape[0]), int(m.shape[1])
        d = check_raster(raster, (h, w), d)
        self._ready_device()
        if raster is not None:
            self._raster_here(raster)
        m = self._on_device(m)
        lab = torch.empty((h, w), dtype=torch.int32, device=self._device)
        n_dev = torch.empty((1,), dtype=torch.int64, device=self._device)
        self._call("regions_label", _ptr(m), h, w, connectivity, min_area, _ptr(lab), _ptr(n_dev))
        self._queue_flag_check(_stream(self._device))
        n = check_region_count(int(n_dev.item()), max_regions)
        table = torch.empty((n, REGION_COLS), dtype=torch.int64, device=self._device)
        self._call("regions_table", _ptr(lab), h, w, n, _ptr(None if raster is None else raster.acc), _ptr(table))
        return RegionTable(table, lab if labels else None, d, (0, 0) if raster is None else raster.origin, connectivity=connectivity)

    # ------------------------------------------------------------------ region outlines
    @torch.no_grad()
    def region_outlines(self, regions, connectivity: Optional[int] = None, max_rings: int = 1 << 20, n: Optional[int] = None):
        """The boundary rings of the regions, with holes, traced on the device ->
        ``keep_amd.outline.RegionOutlines``: polygons on the corner lattice that ``to_geojson`` hands to a viewer.

        ``regions``: a ``RegionTable`` that kept its labels (``mask_regions`` / ``wsi.segment_regions``), or an int32 [h,w] label image
        (numpy or torch, host or device, ``h w <= 2^28``) with ``n=``: values outside 1..n count as background.  ``connectivity``
        defaults to the one the table was labelled with (8 for a label image); with the labelling's own connectivity every region has
        exactly one outer ring, its first, and every other ring of it is a hole.  Two values are read back: the numbers of edges and
        of vertices, which size the workspace and the result, and the number of rings; more than ``max_rings`` rings is a ValueError
        after that.  No thread walks a ring (pointer jumping: the cost follows the logarithm of the longest ring).  Integer
        arithmetic, equal to ``keep_amd.outline.outlines_numpy`` exactly and the same from run to run."""
        lab, n, conn, d, origin = regions_labels(regions, n, connectivity)
        if n is None:
            raise ValueError("a label image needs n=, the number of regions (labels outside 1..n count as background)")
        connectivity, max_rings = check_outline_args(connectivity if connectivity is not None else (8 if conn is None else conn), max_rings)
        h, w = int(lab.shape[0]), int(lab.shape[1])
        self._ready_device()
        lab = lab.to(self._device).contiguous()
        counts = torch.zeros((2,), dtype=torch.int64, device=self._device)
        if n > 0:
            self._call("outline_count", _ptr(lab), h, w, n, connectivity, _ptr(counts))
        E, V = (int(v) for v in counts.tolist()) if n > 0 else (0, 0)
        vertices = torch.empty((V, 2), dtype=torch.int32, device=self._device)
        if V == 0:
            return RegionOutlines(torch.empty((0, RING_COLS), dtype=torch.int64, device=self._device), vertices, d, origin, n)
        cap = min(V // 4, max_rings)
        rings = torch.empty((cap, RING_COLS), dtype=torch.int64, device=self._device)
        r_dev = torch.empty((1,), dtype=torch.int64, device=self._device)
        self._call("outline_trace", _ptr(lab), h, w, n, connectivity, E, V, _ptr(vertices), _ptr(rings if cap else None), cap, _ptr(r_dev))
        R = check_ring_count(int(r_dev.item()), max_rings)
        return RegionOutlines(rings[:R], vertices, d, origin, n)

    @torch.no_grad()
    def draw_outlines(self, rgb, regions, color=(0, 0, 0), width: int = 1) -> torch.Tensor:
        """The regions' outlines drawn into an image on the device -> a new uint8 [h,w,3] on the device.  ``rgb``: uint8 [h,w,3]
        (``render_heatmap``'s output, a thumbnail), numpy or torch, host or device; ``regions``: a ``RegionTable`` with labels or an
        int32 [h,w] label image.  A pixel takes ``color`` iff it belongs to a region and its ``(2 width + 1)^2`` window leaves the
        image or meets another label: a band of ``width`` pixels on the inside of every region, holes included
        (``1 <= width <= 16``).  Equal to ``keep_amd.outline.draw_numpy`` exactly."""
        packed, width = check_draw_args(color, width)
        lab = regions_labels(regions)[0]
        h, w = int(lab.shape[0]), int(lab.shape[1])
        x = rgb_tensor(rgb, (h, w))
        self._ready_device()
        lab, x = lab.to(self._device).contiguous(), x.to(self._device).contiguous()
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=self._device)
        self._call("outline_draw", _ptr(lab), h, w, _ptr(x), _ptr(out), packed, width)
        return out

    # ------------------------------------------------------------------ region shape
    @torch.no_grad()
    def region_shape(self, regions, feret: bool = True, max_pairs: int = DEFAULT_MAX_PAIRS):
        """The second moments and the exact largest diameter of every region, on the device ->
        ``keep_amd.morphometry.RegionShape``: axis lengths, eccentricity, orientation, Feret diameter with its end points and the
        isolated-cells / micro / macro size class follow from it on the host.

        ``regions``: a ``RegionTable`` that kept its labels, in label order (``mask_regions`` / ``wsi.segment_regions``; not a copy that
        ``sort`` permuted).  ``moments``: ``sum_uu, sum_vv, sum_uv`` over every region's pixels from its box origin, one pass over the
        labels, no host synchronisation.  ``feret=True`` adds ``d2, ax, ay, bx, by``: the largest squared distance between two
        corner-lattice points of the region and the first pair, in lattice row-major order, that reaches it.  Its candidates are the
        corners of the first and last pixel of every row (or column, along the shorter box side): ``4 min(bw, bh)`` per region; the
        candidate total and the pair total (the sum of ``c^2 / 2``) are read back once (the one host synchronisation; left in
        ``last_feret_totals``), and more than ``max_pairs`` pairs is a ValueError.  The label image needs
        ``h w max(h, w)^2 < 3 * 2^63`` and, with ``feret``, ``(h + 1) (w + 1) <= 2^31``.  Integer arithmetic, equal to
        ``keep_amd.morphometry.shape_numpy`` exactly and the same from run to run."""
        if not isinstance(regions, RegionTable):
            raise ValueError(f"regions must be a RegionTable, got {type(regions).__name__}")
        if regions.labels is None:
            raise ValueError("this RegionTable has no labels: call mask_regions with labels=True")
        if not regions.label_order:
            raise ValueError("the table's rows are not in label order (a copy that sort() permuted): pass the table mask_regions returned")
        h, w = int(regions.labels.shape[0]), int(regions.labels.shape[1])
        max_pairs = check_shape_args(h, w, feret, max_pairs)
        n = regions.n
        if n == 0:
            dev = regions.table.device
            return RegionShape(torch.empty((0, 3), dtype=torch.int64, device=dev),
                               torch.empty((0, 5), dtype=torch.int64, device=dev) if feret else None, regions)
        self._ready_device()
        lab, table = self._on_device(regions.labels, torch.int32), self._on_device(regions.table, torch.int64)
        moments = torch.empty((n, 3), dtype=torch.int64, device=self._device)
        self._call("regions_moments", _ptr(lab), h, w, n, _ptr(table), _ptr(moments))
        out = None
        if feret:
            out = torch.empty((n, 5), dtype=torch.int64, device=self._device)
            totals = (C.c_int64 * 2)(0, 0)
            try:
                self._call("regions_feret", _ptr(lab), h, w, n, _ptr(table), max_pairs, _ptr(out), totals)
            finally:                                                    # also when the call raises over max_pairs
                self.last_feret_totals = (int(totals[0]), int(totals[1]))
        return RegionShape(moments, out, regions)

    # ------------------------------------------------------------------ polygon annotations
    @torch.no_grad()
    def fill_polygons(self, polys, downsample: int, shape, origin=(0, 0), rule: str = "union", value: int = 1, into=None) -> torch.Tensor:
        """Polygons on level-0 coordinates filled into a mask in thumbnail geometry on the device -> uint8
        ``[h,w]`` on the device: the inverse of :meth:`region_outlines`.

        ``polys``: a ``keep_amd.annotation.PolygonSet`` (``from_geojson`` / ``from_asap_xml`` / ``from_outlines``; its ring weights follow
        ``rule``), or a tuple ``(vertices int [V,2], ring_start int [R+1], weight int [R] in {-1, 0, 1})`` of numpy / torch arrays, host
        or device (arrays on the device are read back once for the argument checks).  One mask pixel covers ``downsample`` x
        ``downsample`` level-0 pixels (``1..4096``), pixel (0, 0) starts at ``origin``; ``shape = (h, w)`` with ``h (w + 1) <= 2^28``; every
        coordinate within +-2^26.  A pixel is inside iff its CENTRE is: the winding number there is ``> 0`` (``"union"``: overlapping
        features unite, a feature's hole does not punch through another feature, the drawing direction does not matter) or odd
        (``"evenodd"``); a centre exactly on an edge belongs to the polygon on whose left or upper side it lies, so polygons that
        share an edge partition the pixels.  ``out = value`` (0..255) inside, ``into`` (uint8 ``[h,w]``, host or device) or 0 elsewhere:
        ``into`` gives a painter's order across calls and ``value=0`` cuts.  The number of edge / row crossings is read back once (the
        one host synchronisation; it is left in ``last_fill_crossings``); ``>= 2^31`` of them is a ValueError.  Integer arithmetic,
        equal to ``keep_amd.annotation.fill_numpy`` exactly and the same from run to run."""
        d, (h, w), (ox, oy), rule_id, value = check_fill_args(downsample, shape, origin, rule, value)
        vertices, ring_start, weight = polygon_arrays(polys, rule)
        into = check_into(into, (h, w))
        self._ready_device()
        V, R = int(vertices.shape[0]), int(ring_start.shape[0]) - 1
        vd, rd, wd = (torch.from_numpy(a).to(self._device) for a in (vertices, ring_start, weight))
        into = None if into is None else self._on_device(into)
        out = torch.empty((h, w), dtype=torch.uint8, device=self._device)
        crossings = C.c_int64(0)
        self._call("poly_fill", _ptr(vd), V, _ptr(rd), R, _ptr(wd), d, h, w, ox, oy, rule_id, value, _ptr(into), _ptr(out), C.byref(crossings))
        self.last_fill_crossings = int(crossings.value)
        return out

    @torch.no_grad()
    def annotation_mask(self, polys, downsample: int, shape, order=None, rule: str = "union", mode: str = "four_pt"):
        """A ``PolygonSet`` -> a ``keep_amd.region.TissueMask`` on the device, which ``region_grid`` / ``encode_region`` /
        ``extract_slide_features`` take as ``tissue=``, ``mask_regions`` as its mask and ``render_heatmap`` as ``tissue=``.

        Without ``order`` everything is filled with 1 in one call of :meth:`fill_polygons`.  ``order``: a sequence of
        ``(groups, value)`` (``keep_amd.annotation.CAMELYON16_ORDER``: the tumour groups painted 1, then the exclusions painted 0): one
        fill per entry over the features of those groups, each painted into the result of the one before.  The origin is (0, 0), as a
        ``TissueMask`` has none; ``mode`` is how a grid cell is tested against the mask."""
        if not isinstance(polys, PolygonSet):
            raise ValueError(f"polys must be a PolygonSet, got {type(polys).__name__}")
        if mode not in MASK_MODES:
            raise ValueError(f"mode must be one of {MASK_MODES}, got {mode!r}")
        check_fill_args(downsample, shape, (0, 0), rule, 1)
        if order is None:
            mask = self.fill_polygons(polys, downsample, shape, (0, 0), rule, 1)
        else:
            steps = [(tuple([g] if isinstance(g, str) else g), check_fill_args(downsample, shape, (0, 0), rule, v)[4]) for g, v in order]
            if not steps:
                raise ValueError("order is empty")
            mask = None
            for groups, v in steps:
                mask = self.fill_polygons(polys.select(groups=groups), downsample, shape, (0, 0), rule, v, mask)
        return TissueMask(mask, downsample, mode)

    @torch.no_grad()
    def mask_tile_counts(self, mask, coords, patch_size: int, downsample: Optional[int] = None, origin=(0, 0)) -> torch.Tensor:
        """How much of a mask lies under every tile, on the device -> int32 ``[N,2]`` on the device: column 0 the mask pixels whose
        centre lies in the tile ``[x, x + patch_size) x [y, y + patch_size)`` (clipped to the mask), column 1 those of them that are
        non-zero.  ``mask``: uint8 / bool ``[h,w]``, numpy or torch, host or device, with ``downsample=``, or a ``TissueMask``, which brings
        its own; ``coords``: integers ``[N,2]``, level-0 top-left ``(x, y)``, within +-2^60; ``origin``: the level-0 position of mask pixel
        (0, 0).  At ``downsample=1`` and origin 0, ``2 * counts[:, 1] > patch_size ** 2`` is the tile label rule of the reference's
        ``segment_utils.py``.  No host synchronisation; equal to ``keep_amd.annotation.tile_counts_numpy`` exactly."""
        m, c, patch, d, (ox, oy) = check_tile_args(mask, coords, patch_size, downsample, origin)
        self._ready_device()
        m, c = self._on_device(m), self._on_device(c, torch.int64)
        N = int(c.shape[0])
        out = torch.empty((N, 2), dtype=torch.int32, device=self._device)
        self._call("mask_tile_counts", _ptr(m), int(m.shape[0]), int(m.shape[1]), d, ox, oy, _ptr(c), N, patch, _ptr(out))
        return out

    # ------------------------------------------------------------------ segmentation evaluation
    @torch.no_grad()
    def tile_roc(self, scores, labels, curve: bool = True):
        """The tile-level ROC of ``eval_seg_auc`` (``segment_utils.py:105-119``) on the device ->
        ``keep_amd.evaluation.RocResult``: ``auc`` (what ``roc_auc_score`` computes, exact and rounded once), ``best_threshold`` (the
        reference's ``thresholds[np.argmax(tpr - fpr)]``, ``inf`` when no threshold beats chance) and, with ``curve=True``, the whole
        curve as device tensors.  ``scores``: floating point [N], rounded to float32; ``labels``: bool / integers [N], non-zero =
        positive; host or device, numpy or torch; ``1 <= N <= 2^24 - 1``.  A NaN score removes its tile.  One class only (or no tile
        left) is the ``ValueError`` scikit-learn raises.  One read of eight scalars (the one host synchronisation; with ``curve=True``
        it also sizes the curve); equal to ``keep_amd.evaluation.roc_numpy`` exactly."""
        s = scores if isinstance(scores, torch.Tensor) else torch.as_tensor(np.asarray(scores))
        l = labels if isinstance(labels, torch.Tensor) else torch.as_tensor(np.asarray(labels))
        N = check_roc_args(s, l)
        self._ready_device()
        s = s.to(self._device, torch.float32).contiguous()
        l = (l.to(self._device) != 0).to(torch.uint8).contiguous()
        scalars = torch.empty((8,), dtype=torch.int64, device=self._device)
        outs = [torch.empty((N,), dtype=dt, device=self._device) if curve else None for dt in (torch.float32, torch.int32, torch.int32, torch.uint8)]
        self._call("eval_roc", _ptr(s), _ptr(l), N, _ptr(scalars), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]))
        n, P, Nn, u2, K, _, bits, _ = scalars.tolist()
        best = struct.unpack("<f", struct.pack("<I", bits & 0xFFFFFFFF))[0]
        if not curve:
            return RocResult(n, P, Nn, u2, best)
        return RocResult(n, P, Nn, u2, best, outs[0][:K], outs[1][:K], outs[2][:K], outs[3][:K].to(torch.bool))

    # ------------------------------------------------------------------ bootstrap confidence intervals
    def _boot_rows(self, name: str, args: tuple, row_shape: tuple, B: int, seed: int, first: int) -> torch.Tensor:
        """int64 ``[1 + B, *row_shape]`` on the device: the sample's own row (replicate -1), then replicates ``first .. first + B - 1`` of
        ``keep_boot_<name>``.  One launch when the replicates start at 0 (the estimate rides in it), else two."""
        out = torch.empty((1 + B,) + row_shape, dtype=torch.int64, device=self._device)
        if first == 0 and B < bootstrap.MAX_REPLICATES:
            self._call(name, *args, seed, -1, 1 + B, _ptr(out))
        else:
            self._call(name, *args, seed, -1, 1, _ptr(out))
            if B:
                self._call(name, *args, seed, first, B, _ptr(out[1:]))
        return out

    @torch.no_grad()
    def bootstrap_roc(self, scores, labels, n_boot: int = 1000, seed: int = 0, first_replicate: int = 0):
        """``n_boot`` bootstrap replicates of the tile ROC on the device -> ``(counts, result)``: ``counts`` int64
        ``[n_boot, 4]`` on the device, rows ``n, P_b, Nn_b, U2_b`` of replicates ``first_replicate ..``, and the AUROC's
        ``keep_amd.bootstrap.BootstrapResult`` (``estimate``, ``values``, ``ci()``, ``se``, ``minus()``).  Arguments as :meth:`tile_roc`;
        ``seed``: an integer in ``[0, 2^64)``.  A replicate that drew one class only has a NaN value and counts in ``n_undefined``; so
        does the estimate of a one-class sample.  Two score vectors with NaNs in the same places and equal ``seed`` give paired
        replicates.  One sort, then one workgroup per replicate; one read of the counts.  Equal to
        ``keep_amd.bootstrap.boot_roc_numpy`` exactly."""
        s = scores if isinstance(scores, torch.Tensor) else torch.as_tensor(np.asarray(scores))
        l = labels if isinstance(labels, torch.Tensor) else torch.as_tensor(np.asarray(labels))
        N = check_roc_args(s, l)
        seed = bootstrap.check_seed(seed)
        B, first = bootstrap.check_replicates(n_boot, first_replicate)
        if first < 0:
            raise ValueError("first_replicate must be >= 0 here: the sample's own row is the result's estimate")
        self._ready_device()
        s = s.to(self._device, torch.float32).contiguous()
        l = (l.to(self._device) != 0).to(torch.uint8).contiguous()
        rows = self._boot_rows("boot_roc", (_ptr(s), _ptr(l), N), (4,), B, seed, first)
        return rows[1:], bootstrap.result_from_roc_counts(rows, seed, first)

    def _boot_confusions(self, truth, pred, n_classes, n_boot, seed, first_replicate):
        """-> (int64 ``[1 + B, C, C]`` on the device, the sample's confusion first; seed; first replicate)."""
        t = truth if isinstance(truth, torch.Tensor) else torch.as_tensor(np.asarray(truth))
        p = pred if isinstance(pred, torch.Tensor) else torch.as_tensor(np.asarray(pred))
        N, C = bootstrap.check_confusion_args(t, p, n_classes)
        seed = bootstrap.check_seed(seed)
        B, first = bootstrap.check_replicates(n_boot, first_replicate)
        if first < 0:
            raise ValueError("first_replicate must be >= 0 here: the sample's own row is the result's estimate")
        self._ready_device()
        t, p = t.to(self._device, torch.uint8).contiguous(), p.to(self._device, torch.uint8).contiguous()
        return self._boot_rows("boot_confusion", (_ptr(t), _ptr(p), N, C), (C, C), B, seed, first), seed, first

    @torch.no_grad()
    def bootstrap_confusion(self, truth, pred, n_classes: int, n_boot: int = 1000, seed: int = 0, first_replicate: int = 0) -> torch.Tensor:
        """``n_boot`` bootstrap replicates of a confusion matrix on the device -> int64 ``[n_boot, C, C]`` on the device:
        ``counts[r, t, p]`` = the draws of replicate ``first_replicate + r`` that landed on an item with truth ``t`` and prediction
        ``p``; every ``counts[r]`` sums to N.  ``truth`` / ``pred``: bool or integers ``[N]`` with values in ``[0, n_classes)``, host or
        device, numpy or torch; ``2 <= n_classes <= 16``; anything else is a ``ValueError``.  Equal to
        ``keep_amd.bootstrap.boot_confusion_numpy`` exactly."""
        return self._boot_confusions(truth, pred, n_classes, n_boot, seed, first_replicate)[0][1:]

    @torch.no_grad()
    def bootstrap_metric(self, truth, pred, n_classes: int, metric, n_boot: int = 1000, seed: int = 0, first_replicate: int = 0):
        """A metric of the confusion matrix with its bootstrap replicates -> ``keep_amd.bootstrap.BootstrapResult``.  ``metric``:
        ``"accuracy"``, ``"balanced_accuracy"``, ``"weighted_f1"``, for two classes ``"sensitivity"`` / ``"specificity"``, or a callable that
        takes the int64 ``[1 + n_boot, C, C]`` confusions (numpy) and returns one float64 per confusion
        (``lambda m: bootstrap.recall(m, 2)``).  The counts come from one launch of :meth:`bootstrap_confusion`'s kernel; the
        metric runs on the host in float64."""
        fn = bootstrap.resolve_metric(metric)
        rows, seed, first = self._boot_confusions(truth, pred, n_classes, n_boot, seed, first_replicate)
        return bootstrap.result_from_confusions(rows, fn, seed, first)

    @torch.no_grad()
    def bootstrap_ovr_roc(self, probs, labels, n_boot: int = 1000, seed: int = 0, first_replicate: int = 0):
        """One-vs-rest AUROC per class with bootstrap replicates, and their macro mean -> ``(per_class, macro)``: a list of C
        ``BootstrapResult`` and one more.  ``probs``: floating ``[N,C]``; ``labels``: integers ``[N]`` in ``[0, C)``.  A row of ``probs``
        with any NaN is dropped for every class (``class_raster``'s rule), so every class resamples the same items with the same
        draws; a replicate undefined for any class is undefined for the macro mean."""
        p = probs if isinstance(probs, torch.Tensor) else torch.as_tensor(np.asarray(probs))
        l = labels if isinstance(labels, torch.Tensor) else torch.as_tensor(np.asarray(labels))
        if p.ndim != 2 or not p.dtype.is_floating_point or p.shape[1] < 2:
            raise ValueError(f"probs must be floating point [N, C] with C >= 2, got {p.dtype} {tuple(p.shape)}")
        if l.ndim != 1 or l.shape[0] != p.shape[0] or l.dtype.is_floating_point or l.dtype.is_complex:
            raise ValueError(f"labels must be integers [N] beside probs [N, C], got {l.dtype} {tuple(l.shape)}")
        C = int(p.shape[1])
        if l.numel() and (int(l.min()) < 0 or int(l.max()) >= C):
            raise ValueError(f"labels outside [0, {C})")
        self._ready_device()
        p, l = p.to(self._device, torch.float32), l.to(self._device)
        keep = ~torch.isnan(p).any(dim=1)
        p, l = p[keep], l[keep]
        per_class = [self.bootstrap_roc(p[:, c].contiguous(), l == c, n_boot, seed, first_replicate)[1] for c in range(C)]
        return per_class, bootstrap.macro_mean(per_class)

    @torch.no_grad()
    def mask_overlap(self, a, b, within=None):
        """The overlap counts of two masks on the device, the counting of ``eval_seg_coarse`` (``segment_utils.py:130-151``) ->
        ``keep_amd.evaluation.MaskOverlap`` (``.dice``, ``.iou``, ``.confusion`` follow in Python integers).  ``a``, ``b`` and the
        optional ``within``: bool / uint8 ``[h,w]`` of one shape, numpy or torch, host or device, or ``TissueMask``s; non-zero = set;
        only the pixels where ``within`` is set are considered.  One read of four integers; equal to
        ``keep_amd.evaluation.mask_counts_numpy`` exactly."""
        a = check_mask(a, "a")
        shape = (int(a.shape[0]), int(a.shape[1]))
        b = check_mask(b, "b", shape)
        within = None if within is None else check_mask(within, "within", shape)
        self._ready_device()
        a, b, within = self._on_device(a), self._on_device(b), (None if within is None else self._on_device(within))
        out = torch.empty((4,), dtype=torch.int64, device=self._device)
        self._call("eval_mask_counts", _ptr(a), _ptr(b), _ptr(within), shape[0], shape[1], _ptr(out))
        return MaskOverlap(*out.tolist())

    @torch.no_grad()
    def raster_hist(self, raster, truth, within=None) -> torch.Tensor:
        """int64 ``[2, 65537]`` on the device: the raster's pixels (inside ``within``) by truth and by their mean in 16-bit fixed
        point, the uncovered ones in bin 65536.  Arguments as :meth:`raster_sweep`.  No host synchronisation; equal to
        ``keep_amd.evaluation.raster_hist_numpy`` exactly."""
        _check_tile_raster(raster)
        check_same_geometry(raster, truth, "truth")
        check_same_geometry(raster, within, "within")
        truth = check_mask(truth, "truth", raster.shape)
        within = None if within is None else check_mask(within, "within", raster.shape)
        self._ready_device()
        self._raster_here(raster)
        truth, within = self._on_device(truth), (None if within is None else self._on_device(within))
        hist = torch.empty((2, HIST_BINS), dtype=torch.int64, device=self._device)
        h, w = raster.shape
        self._call("eval_raster_hist", _ptr(raster.acc), _ptr(truth), _ptr(within), h, w, _ptr(hist))
        return hist

    @torch.no_grad()
    def raster_sweep(self, raster, truth, within=None):
        """Every threshold of a heatmap against a truth mask at once -> ``keep_amd.evaluation.RasterSweep``:
        TP / FP / FN and Dice of "mean > t" for the 65536 thresholds of the raster's fixed point, the threshold of the best Dice and
        the pixel-level AUROC.  ``raster``: a ``TileRaster`` (``tile_raster`` / ``wsi.segment_heatmap``); ``truth`` / ``within``: bool /
        uint8 ``[h,w]`` of the raster's shape or ``TissueMask``s of its geometry (``fill_polygons`` / ``annotation_mask`` at the raster's
        downsample make one).  One histogram kernel, then cumulative sums with torch on the device."""
        return sweep_from_hist(self.raster_hist(raster, truth, within))

    @torch.no_grad()
    def annotation_tile_labels(self, polys_or_mask, coords, patch_size: int, order=None, rule: str = "union",
                               max_band_bytes: int = 1 << 28) -> torch.Tensor:
        """A label per tile from the ground truth, by the reference's rule (``segment_utils.py:99-103``): 1 iff more than half of the
        tile's level-0 pixels are set -> uint8 ``[N]`` on the device.  ``coords``: integers ``[N,2]``, level-0 top-left ``(x, y)``.

        A ``PolygonSet`` is filled at downsample 1 -- a level-0 mask of a whole slide would not fit, so in horizontal bands of whole
        tile rows over the tiles' x extent, at most ``max_band_bytes`` of mask each (``keep_amd.evaluation.plan_label_bands``), with
        :meth:`mask_tile_counts` per band; no tile is clipped by a band, so the labels do not depend on the banding.  ``order``
        (``keep_amd.annotation.CAMELYON16_ORDER``) paints group after group as :meth:`annotation_mask` does.  A ``TissueMask`` of
        downsample d (origin 0) gives ``2 c1 d^2 > patch_size^2`` with c1 the set mask pixels whose centre lies in the tile: the
        reference's rule at d = 1; a bare bool / uint8 ``[h,w]`` array is a level-0 mask (d = 1).  Pixels outside a mask are not set."""
        if not isinstance(polys_or_mask, PolygonSet):
            mask = polys_or_mask if isinstance(polys_or_mask, TissueMask) else TissueMask(polys_or_mask, 1)
            if order is not None:
                raise ValueError("order= paints the groups of a PolygonSet: a mask has none")
            counts = self.mask_tile_counts(mask, coords, patch_size)
            return (2 * counts[:, 1].to(torch.int64) * mask.downsample ** 2 > int(patch_size) ** 2).to(torch.uint8)
        polys = polys_or_mask
        _, c, patch, _, _ = check_tile_args(np.zeros((1, 1), np.uint8), coords, patch_size, 1)
        steps = [(None, 1)] if order is None else [(tuple([g] if isinstance(g, str) else g), int(v)) for g, v in order]
        if not steps:
            raise ValueError("order is empty")
        self._ready_device()
        c = self._on_device(c, torch.int64)
        labels = torch.zeros((int(c.shape[0]),), dtype=torch.uint8, device=self._device)
        if c.shape[0] == 0:
            return labels
        x0, y_all = int(c[:, 0].min()), c[:, 1]
        x1 = int(c[:, 0].max()) + patch
        sets = [(polys if g is None else polys.select(groups=g), v) for g, v in steps]
        for y_first, y_last in plan_label_bands(y_all.cpu().numpy(), x0, x1, patch, max_band_bytes):
            shape, origin = (y_last + patch - y_first, x1 - x0), (x0, y_first)
            check_fill_args(1, shape, origin, rule, 1)
            mask = None
            for sel, v in sets:
                mask = self.fill_polygons(sel, 1, shape, origin, rule, v, mask)
            rows = torch.nonzero((y_all >= y_first) & (y_all <= y_last)).squeeze(1)
            counts = self.mask_tile_counts(mask, c[rows], patch, 1, origin)
            labels[rows] = (2 * counts[:, 1].to(torch.int64) > patch * patch).to(torch.uint8)
        return labels

    # ------------------------------------------------------------------ lesion-level scoring
    def _mask_dist2(self, m: torch.Tensor, R: int, invert: int) -> torch.Tensor:
        """keep_mask_dist2 on a uint8 [h,w] device tensor -> uint32 [h,w] on the device."""
        h, w = int(m.shape[0]), int(m.shape[1])
        out = torch.empty((h, w), dtype=torch.uint32, device=self._device)
        self._call("mask_dist2", _ptr(m), h, w, R, invert, _ptr(out))
        return out

    @torch.no_grad()
    def mask_distance(self, mask, radius: int, to: str = "foreground") -> torch.Tensor:
        """The squared Euclidean distance transform of a mask, capped at a radius, on the device -> uint32
        ``[h,w]`` on the device: the squared distance in pixels from every pixel to the nearest set pixel (``to="background"``: to the
        nearest zero pixel), exact where it is ``<= radius^2`` and ``radius^2 + 1`` elsewhere, a mask without such a pixel included.
        ``mask``: bool / uint8 ``[h,w]``, numpy or torch, host or device, or a ``TissueMask``; ``1 <= radius <= 1024``.  Pixels outside the
        image do not exist (scipy's behaviour): ``rint(distance_transform_edt(mask == 0) ** 2)`` capped.  No host synchronisation;
        equal to ``keep_amd.lesion.dist2_numpy`` exactly."""
        R, invert = check_radius(radius), check_direction(to)
        m = check_mask(mask, "mask")
        self._ready_device()
        return self._mask_dist2(self._on_device(m), R, invert)

    def _mask_band(self, mask, distance, invert: int):
        R, k = distance_threshold(distance)
        m = check_mask(mask, "mask")
        self._ready_device()
        d2 = self._mask_dist2(self._on_device(m), R, invert).view(torch.int32)          # <= 2^20 + 1: the sign bit is clear
        out = (d2 > k) if invert else (d2 <= k)
        if isinstance(mask, TissueMask):
            return TissueMask(out, mask.downsample, mask.mode, mask.threshold)
        return TissueMask(out, 1)

    @torch.no_grad()
    def dilate_mask(self, mask, distance: float):
        """A mask dilated by a true disc -> ``TissueMask`` of the same geometry (downsample 1 for a bare array): a pixel is taken
        iff its distance to the mask is ``< distance`` pixels, ``0 < distance <= 1024``, a float.  The comparison is scipy's float64
        ``distance_transform_edt(mask == 0) < distance``, done exactly as an integer threshold on :meth:`mask_distance`
        (``keep_amd.lesion.distance_threshold``)."""
        return self._mask_band(mask, distance, 0)

    @torch.no_grad()
    def erode_mask(self, mask, distance: float):
        """A mask eroded by a true disc: a pixel stays iff its distance to the background is ``>= distance`` pixels; the outside of
        the image is not background.  Otherwise as :meth:`dilate_mask`."""
        return self._mask_band(mask, distance, 1)

    @torch.no_grad()
    def evaluation_mask(self, truth, margin_px: float, connectivity: int = 8, fill_holes: bool = True, ignore_max_extent=None,
                        downsample: Optional[int] = None, shape=None, order=None, rule: str = "union", max_regions: int = 1 << 20,
                        ignore_major_axis=None):
        """The labelled lesions a detection may hit, as the CAMELYON16 evaluation describes its mask: the truth dilated by
        ``margin_px`` (``keep_amd.lesion.camelyon16_margin``; 0 = as it is), holes filled, labelled with ``connectivity`` ->
        ``keep_amd.lesion.EvaluationMask``.  ``truth``: a ``TissueMask``, or a ``PolygonSet`` with ``downsample=`` and ``shape=`` (through
        :meth:`annotation_mask` with ``order`` / ``rule``).  Holes are the 4-connected background regions that touch no border.
        ``ignore_major_axis``: lesions of this labelled mask whose major axis length (``RegionShape.axis_lengths()[:, 0]``, from the
        device's integer moments; :meth:`region_shape`) is below it get their ``ignore`` byte set: the challenge's
        isolated-tumour-cell rule, on the mask it is defined on (``keep_amd.morphometry.camelyon16_itc_axis``: 275 um, 35.4 pixels at
        downsample 32).  ``ignore_max_extent``: the same by the longer side of the bounding box, the rule this method had before
        the moments; giving both is a ValueError.  Callers may overwrite ``ignore``.  Parity with the challenge's script and with
        scikit-image is unpinned (neither is available where this is built).  Two labellings, each with its one readback."""
        if isinstance(truth, PolygonSet):
            if downsample is None or shape is None:
                raise ValueError("a PolygonSet needs downsample= and shape=, the geometry of the evaluation mask")
            truth = self.annotation_mask(truth, downsample, shape, order=order, rule=rule)
        if not isinstance(truth, TissueMask):
            raise ValueError(f"truth must be a TissueMask or a PolygonSet, got {type(truth).__name__}")
        if ignore_max_extent is not None and not ignore_max_extent >= 0:
            raise ValueError(f"ignore_max_extent must be >= 0, got {ignore_max_extent!r}")
        if ignore_major_axis is not None:
            if ignore_max_extent is not None:
                raise ValueError("give ignore_major_axis (the challenge's rule) or ignore_max_extent (the bounding-box rule), not both")
            if not ignore_major_axis >= 0:
                raise ValueError(f"ignore_major_axis must be >= 0, got {ignore_major_axis!r}")
        grown = self.dilate_mask(truth, margin_px) if margin_px else TissueMask(self._on_device(truth.mask), truth.downsample, truth.mode)
        mask = grown.mask
        if fill_holes:
            bg = self.mask_regions(mask == 0, 4, max_regions=max_regions)
            hole = torch.cat([torch.zeros((1,), dtype=torch.uint8, device=self._device), (bg.border == 0).to(torch.uint8)])
            mask = mask | hole[bg.labels.to(torch.int64)]
        table = self.mask_regions(TissueMask(mask, truth.downsample, truth.mode), connectivity, max_regions=max_regions)
        ignore = torch.zeros((table.n,), dtype=torch.uint8, device=self._device)
        if ignore_max_extent is not None:
            ignore = (torch.maximum(table.x1 - table.x0, table.y1 - table.y0) < ignore_max_extent).to(torch.uint8)
        if ignore_major_axis is not None:
            major = self.region_shape(table, feret=False).axis_lengths()[:, 0]
            ignore = torch.from_numpy((major < float(ignore_major_axis)).astype(np.uint8)).to(self._device)
        return EvaluationMask(table.labels, table.n, table, ignore, truth.downsample, (0, 0))

    @torch.no_grad()
    def raster_peaks(self, raster, radius: int, min_score: float = 0.5, tissue=None, max_peaks: int = 1 << 20):
        """The local maxima of a heatmap on the device -> ``keep_amd.lesion.LesionCandidates``.  A raster
        pixel is eligible iff a tile covers it (and ``tissue``, a ``TissueMask`` of the raster's geometry, is set there); its value is
        its mean in 16-bit fixed point; an eligible pixel at or above ``quantize(min_score)`` is a peak iff no other eligible pixel of
        its ``(2 radius + 1)^2`` window is larger, or equal with a lower row-major index (``1 <= radius <= 127``).  Candidates come in
        row-major order, the same from run to run.  Their number is read back once; more than ``max_peaks`` is a ValueError that
        reports it.  Equal to ``keep_amd.lesion.peaks_numpy`` / ``candidates_numpy`` exactly."""
        _check_tile_raster(raster)
        r, min16, cap = check_peak_args(radius, min_score, max_peaks)
        if tissue is not None:
            _check_tissue(tissue, raster)
        self._ready_device()
        self._raster_here(raster)
        h, w = raster.shape
        md = None if tissue is None else self._on_device(tissue.mask)
        rows = min(cap, h * w)
        peaks = torch.empty((rows, 3), dtype=torch.int64, device=self._device)
        n_dev = torch.empty((1,), dtype=torch.int64, device=self._device)
        self._call("raster_peaks", _ptr(raster.acc), _ptr(md), h, w, r, min16, rows, _ptr(peaks if rows else None), _ptr(n_dev))
        n = check_peak_count(int(n_dev.item()), cap)
        peaks = peaks[:n]
        d = raster.downsample
        xy = peaks[:, :2] * d + (torch.tensor(raster.origin, dtype=torch.int64, device=self._device) + d // 2)
        return LesionCandidates(xy, (peaks[:, 2].to(torch.float64) / float(Q_ONE)).to(torch.float32), peaks[:, 2].clone())

    @torch.no_grad()
    def lesion_hits(self, candidates, evaluation_mask):
        """Which lesion does every candidate hit, and the best score on every lesion, on the device ->
        ``keep_amd.lesion.LesionHits``.  ``candidates``: a ``LesionCandidates`` or a pair ``(xy integers [N,2] level-0, scores floating
        [N])``, host or device, ``N <= 2^24 - 1``; ``evaluation_mask``: an ``EvaluationMask``.  A candidate reads the label under it
        (floor division by the mask's downsample; outside the mask is background); a NaN score gives ``hit = -1`` and takes no part;
        ``lesion_max`` is the maximum of ``max(score, 0)`` over a lesion's hits and stays 0 for an ignored lesion, whose hits are not
        false positives either.  No host synchronisation but for ``fp_scores``; equal to ``keep_amd.lesion.lesion_hits_numpy`` exactly."""
        if not isinstance(evaluation_mask, EvaluationMask):
            raise ValueError(f"evaluation_mask must be an EvaluationMask, got {type(evaluation_mask).__name__}")
        xy, s = (candidates.xy, candidates.scores) if isinstance(candidates, LesionCandidates) else candidates
        xy = xy if isinstance(xy, torch.Tensor) else torch.as_tensor(np.asarray(xy))
        s = s if isinstance(s, torch.Tensor) else torch.as_tensor(np.asarray(s))
        N = check_candidates(xy, s)
        em = evaluation_mask
        if em.n > MAX_LABELS:
            raise ValueError(f"the evaluation mask has {em.n} lesions, at most 2^20")
        self._ready_device()
        xy, s = self._on_device(xy, torch.int64), self._on_device(s, torch.float32)
        lab, ignore = self._on_device(em.labels, torch.int32), self._on_device(em.ignore, torch.uint8)
        hit = torch.empty((N,), dtype=torch.int32, device=self._device)
        best = torch.empty((em.n,), dtype=torch.float32, device=self._device)
        self._call("lesion_hits", _ptr(xy if N else None), _ptr(s if N else None), N, _ptr(lab), int(lab.shape[0]), int(lab.shape[1]), em.downsample,
                   em.origin[0], em.origin[1], em.n, _ptr(ignore if em.n else None), _ptr(hit if N else None), _ptr(best if em.n else None))
        return LesionHits(hit, best, em.n - int(ignore.sum()), s[hit == 0] + 0.0)

    # ------------------------------------------------------------------ stain normalisation
    def _stain_const(self, key, make) -> torch.Tensor:
        """A host-made table on the device, uploaded once per engine and key."""
        cache = self.__dict__.setdefault("_stain_consts", {})
        if key not in cache:
            cache[key] = torch.from_numpy(make()).to(self._device)
        return cache[key]

    def _stain_view(self, image, mask, ds):
        """-> the arguments the three fit passes share: image view, mask (or null) and downsample."""
        if isinstance(image, np.ndarray):                          # an image of a fit begun with stain_fit_numpy and continued here
            image = torch.from_numpy(np.ascontiguousarray(image))
        image = image.to(self._device)
        H, W, C, row = thumbnail_layout(image)
        md = None if mask is None else mask.to(self._device, torch.uint8).contiguous()
        return (_ptr(image), H, W, row, C, _ptr(md), 0 if md is None else int(md.shape[0]), 0 if md is None else int(md.shape[1]), ds), (image, md)

    class _StainPasses:
        """keep_amd.stain.run_fit's three passes on the device: the accumulators are device tensors, read back by ``to_numpy``."""

        def __init__(self, ops):
            self.ops = ops

        def _acc(self, acc, shape, dtype):
            return (torch.empty(shape, dtype=dtype, device=self.ops._device), 1) if acc is None else (acc, 0)

        def moments(self, image, mask, ds, od_q, beta_q, acc):
            o = self.ops
            acc, zero = self._acc(acc, (10,), torch.int64)
            view, _md = o._stain_view(image, mask, ds)
            o._call("stain_moments", *view, _ptr(o._stain_const(("od", od_q.tobytes()), lambda: od_q)), beta_q, zero, _ptr(acc))
            return acc

        def angle_hist(self, image, mask, ds, od_q, beta_q, v_q, acc):
            o = self.ops
            acc, zero = self._acc(acc, (_stain.ANGLE_BINS,), torch.int32)
            view, _md = o._stain_view(image, mask, ds)
            v = np.ascontiguousarray(v_q, dtype=np.int32)
            o._call("stain_angle_hist", *view, _ptr(o._stain_const(("od", od_q.tobytes()), lambda: od_q)), beta_q, v.ctypes.data_as(C.c_void_p),
                    _ptr(o._stain_const("dirs", _stain.angle_dirs)), zero, _ptr(acc))
            return acc

        def conc_hist(self, image, mask, ds, od_q, minv_q, acc):
            o = self.ops
            acc, zero = self._acc(acc, (2, _stain.CONC_BINS), torch.int32)
            view, _md = o._stain_view(image, mask, ds)
            m = np.ascontiguousarray(minv_q, dtype=np.int32)
            o._call("stain_conc_hist", *view, _ptr(o._stain_const(("od", od_q.tobytes()), lambda: od_q)), m.ctypes.data_as(C.c_void_p), zero,
                    _ptr(acc))
            return acc

        @staticmethod
        def to_numpy(acc):
            return acc.cpu().numpy().astype(np.int64)

    @torch.no_grad()
    def stain_fit(self, image, tissue=None, alpha: float = 1, beta: float = 0.15, io: float = 240, into: Optional[StainFit] = None) -> StainFit:
        """Macenko fit of the H & E stain of ``image`` on the device -> ``keep_amd.stain.StainFit``.

        ``image``: a thumbnail or region, uint8 [h,w,3] (RGB) or [h,w,4] (RGBA, alpha ignored), host or device, numpy or torch, any
        row stride, ``h w <= 2^30``.  ``tissue``: a ``TissueMask`` whose pixel covers ``downsample`` x ``downsample`` pixels of ``image``
        (a mask made from this very thumbnail: ``TissueMask(mask.mask, 1)``) or ``None`` (every pixel).  Three integer passes on the
        device (moments of the optical density over pixels with every channel ``OD >= beta``; the histogram of their angles in the
        plane of the two leading eigenvectors; the histograms of the least-squares concentrations over every allowed pixel) with the
        3 x 3 ``eigh``, the 3 x 2 ``pinv`` and the percentiles (``alpha``, ``100 - alpha``, 99) in float64 on the host between them;
        equal to ``keep_amd.stain.stain_fit_numpy`` bit for bit.  ``into``: a fit to continue with this image (bands of a region, slides
        of a cohort); the result is the fit of all its images however they were split.  Fewer than 2 kept pixels, or pixels that span
        no plane, raise ValueError naming the count."""
        x = torch.from_numpy(image) if not isinstance(image, torch.Tensor) else image
        thumbnail_layout(x)
        _stain.mask_split(tissue)
        self._ready_device()
        if x.device != self._device:
            x = x.to(self._device)
        return _stain.run_fit(self._StainPasses(self), x, tissue, alpha, beta, io, into)

    def _stain_plan(self, fit, target=None, keep=_stain.STAINS):
        """A fit (+ target, stains kept) -> what ``keep_stain_apply_u8`` takes: (od_q on the device, t_q on the host, exp table on the
        device, its length, lo)."""
        if not isinstance(fit, StainFit):
            raise ValueError(f"fit must be a StainFit, got {type(fit).__name__}")
        t = fit.tables(target, keep)
        return (self._stain_const(("od", t["od_q"].tobytes()), lambda: t["od_q"]), np.ascontiguousarray(t["t_q"], dtype=np.int32),
                self._stain_const(("exp", t["exp_lut"].tobytes()), lambda: t["exp_lut"]), int(len(t["exp_lut"])), int(t["lo"]))

    def _stain_apply(self, src: torch.Tensor, dst: torch.Tensor, plan) -> None:
        """keep_stain_apply_u8 on contiguous device uint8 [..., 3]; ``dst`` may be ``src``."""
        od, t_q, lut, n_lut, lo = plan
        self._call("stain_apply_u8", _ptr(src), src.numel() // 3, _ptr(od), t_q.ctypes.data_as(C.c_void_p), _ptr(lut), n_lut, lo, _ptr(dst))

    @torch.no_grad()
    def stain_normalize(self, pixels_u8, fit: StainFit, target: Optional[StainTarget] = None, keep=_stain.STAINS, out=None):
        """Map uint8 ``[..., 3]`` pixels (``[..., 4]``: the alpha is dropped, the result is ``[..., 3]``) of the stain ``fit`` describes
        to ``target`` (default: the customary Macenko reference) on the device -> uint8 of the same shape on the input's device, a
        numpy array for a numpy input.  One kernel: table -> 3 x 3 integer matrix -> table per pixel, equal to
        ``keep_amd.stain.stain_apply_numpy`` with ``fit.tables(target, keep)`` bit for bit.  ``keep=("H",)`` / ``("E",)`` gives the
        haematoxylin-only / eosin-only image.  ``out``: a contiguous uint8 tensor of the result's shape on the engine's device; it may
        be ``pixels_u8`` itself (in place)."""
        as_numpy = isinstance(pixels_u8, np.ndarray)
        x = torch.from_numpy(pixels_u8) if as_numpy else pixels_u8
        if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or x.dim() < 1 or x.shape[-1] not in (3, 4):
            raise ValueError(f"pixels must be uint8 [..., 3] or [..., 4], got {getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))}")
        self._ready_device()
        plan = self._stain_plan(fit, target, keep)
        src = x.to(self._device)[..., :3].contiguous()
        if out is None:
            dst = torch.empty_like(src)
        else:
            if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != self._device or out.shape != src.shape \
                    or not out.is_contiguous():
                raise ValueError(f"out must be a contiguous uint8 tensor {tuple(src.shape)} on {self._device}")
            dst = out
        if src.numel():
            self._stain_apply(src, dst, plan)
        if out is not None:
            return out
        return dst.cpu().numpy() if as_numpy else (dst if x.device == self._device else dst.to(x.device))

    # ------------------------------------------------------------------ tile quality control
    def _quality_table(self, xd: torch.Tensor, H: int, W: int, C: int, row: int, cells: torch.Tensor, patch: int, rules) -> torch.Tensor:
        """keep_region_quality: int32 [N,2] cells of a device region -> the int64 [N,12] table on the device (one sync: the cell check)."""
        cells = cells.to(self._device, torch.int32).contiguous()
        N = int(cells.shape[0])
        if N > QUALITY_MAX_CELLS:
            raise ValueError(f"at most 2^24 - 1 cells go into one table, got {N}")
        out = torch.empty((N, QUALITY_COLS), dtype=torch.int64, device=self._device)
        if N:
            self._call("region_quality", _ptr(xd), H, W, C, row, _ptr(cells), N, patch, _ptr(self._quality_blob(rules)), 1, _ptr(out))
        return out

    def _quality_blob(self, rules) -> torch.Tensor:
        """The rules' words on the device, uploaded once per engine and set of rules; the 16 sets used last are kept."""
        cache = self.__dict__.setdefault("_quality_blobs", {})
        blob = cache.pop(rules, None)
        if blob is None or blob.device != self._device:
            blob = torch.from_numpy(rules.blob()).to(self._device)
        cache[rules] = blob                                         # dicts keep insertion order: the first key is the one used longest ago
        while len(cache) > 16:
            del cache[next(iter(cache))]
        return blob

    def _quality_cells(self, xd: torch.Tensor, H: int, W: int, C: int, row: int, cells: torch.Tensor, patch: int, gate: QualityGate) -> torch.Tensor:
        """The cells of a grid that ``gate`` keeps, in grid order (measured in the region at its own resolution)."""
        if cells.shape[0] == 0:
            return cells
        return cells[gate.keep(TileQuality(self._quality_table(xd, H, W, C, row, cells, patch, gate.rules), patch))]

    @torch.no_grad()
    def tile_quality(self, tiles_u8, rules=None) -> TileQuality:
        """Class counts and focus of every tile of a batch on the device -> ``keep_amd.quality.TileQuality``.
        ``tiles_u8``: uint8 ``[N,S,S,3]`` (or ``[N,S,S,4]``, alpha ignored), ``1 <= S <= 1024``, host or device, numpy or torch; ``rules``: a
        ``keep_amd.quality.QualityRules`` (default: its defaults).  The batch is read as a region of height ``N S`` with the cells
        ``(0, i S)``: the kernel, and the numbers, are :meth:`region_quality`'s.  Equal to ``keep_amd.quality.tile_quality_numpy`` exactly."""
        rules = check_rules(rules)
        x = torch.from_numpy(tiles_u8) if isinstance(tiles_u8, np.ndarray) else tiles_u8
        if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or x.dim() != 4 or x.shape[1] != x.shape[2] or x.shape[3] not in (3, 4):
            raise ValueError(f"tiles must be uint8 [N,S,S,3], got {getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))}")
        N, S, C = int(x.shape[0]), int(x.shape[1]), int(x.shape[3])
        check_patch(S)
        if N * S >= 1 << 31:
            raise ValueError(f"{N} tiles of {S} rows: a batch holds fewer than 2^31 rows")
        self._ready_device()
        if N == 0:
            return TileQuality(torch.empty((0, QUALITY_COLS), dtype=torch.int64, device=self._device), S)
        xd = x.to(self._device).contiguous().view(N * S, S, C)
        cells = torch.zeros((N, 2), dtype=torch.int32, device=self._device)
        cells[:, 1] = torch.arange(N, dtype=torch.int32, device=self._device) * S
        return TileQuality(self._quality_table(xd, N * S, S, C, S * C, cells, S, rules), S)

    @torch.no_grad()
    def region_quality(self, region, coords, patch_size: int, origin=(0, 0), coord_scale: int = 1, rules=None) -> TileQuality:
        """Class counts and focus of the tiles of ``coords`` measured IN the region, at its own resolution and before any resize to 224
         -> ``keep_amd.quality.TileQuality`` on the engine's device.  ``region``, ``coords``, ``origin`` and
        ``coord_scale`` as in :meth:`region_patches_uint8` (a coord outside the region is the same ValueError); ``1 <= patch_size <= 1024``;
        overlapping tiles are fine.  Per tile: the pixels of each pen class, of dark, glass and tissue (every pixel has one class;
        ``keep_amd.quality``), and the sums behind the variance of the integer Laplacian over the tile's interior pixels, over all
        of them and over the tissue ones.  Integer arithmetic, equal to ``keep_amd.quality.tile_quality_numpy`` exactly."""
        rules, patch = check_rules(rules), check_patch(patch_size)
        _, _, origin, coord_scale = check_grid_args(TILE, None, origin, coord_scale)
        coords = torch.as_tensor(coords)
        if coords.dim() != 2 or coords.shape[1] != 2:
            raise ValueError(f"coords must be [N,2] (x, y), got {tuple(coords.shape)}")
        x = self._region_tensor(region)
        self._ready_device()
        xd, H, W, C, row = self._region_on_device(x)
        c = coords.to(self._device, torch.int64)
        cells = (torch.div(c, coord_scale, rounding_mode="floor") - torch.tensor(origin, dtype=torch.int64, device=self._device))
        cells = cells.clamp(-(1 << 31), (1 << 31) - 1).to(torch.int32)          # out of int32 range stays outside the region
        return TileQuality(self._quality_table(xd, H, W, C, row, cells, patch, rules), patch)

    @torch.no_grad()
    def pen_mask(self, thumbnail, rules=None):
        """The class of every pixel of a thumbnail on the device -> uint8 ``[h,w]`` on the input's device (a numpy
        array for a numpy input): 0 none, 1-4 pen class + 1 (``keep_amd.quality.PEN_CLASSES``), 5 dark, 6 glass, 7 tissue.
        ``thumbnail``: the layout contract of :meth:`tissue_mask`.  ``keep_amd.quality.exclude`` takes chosen classes out of a
        ``TissueMask`` with it.  Equal to ``keep_amd.quality.pen_mask_numpy`` exactly; no host synchronisation."""
        rules = check_rules(rules)
        as_numpy = isinstance(thumbnail, np.ndarray)
        x = torch.from_numpy(thumbnail) if as_numpy else thumbnail
        thumbnail_layout(x)
        self._ready_device()
        xd = x if x.device == self._device else x.to(self._device)
        h, w, C, row = thumbnail_layout(xd)
        out = torch.empty((h, w), dtype=torch.uint8, device=self._device)
        self._call("pen_mask", _ptr(xd), h, w, C, row, _ptr(self._quality_blob(rules)), _ptr(out))
        return out.cpu().numpy() if as_numpy else (out if x.device == self._device else out.to(x.device))

    @staticmethod
    def _cells_to_coords(cells: torch.Tensor, origin, coord_scale: int) -> torch.Tensor:
        o = torch.tensor(origin, dtype=torch.int64, device=cells.device)
        return (cells.to(torch.int64) + o) * coord_scale

    @torch.no_grad()
    def region_grid(self, region, patch_size: int = 224, step: Optional[int] = None, tissue=None, origin=(0, 0),
                    coord_scale: int = 1, quality: Optional[QualityGate] = None) -> torch.Tensor:
        """Patch grid over a uint8 region [H,W,3] (RGB) or [H,W,4] (RGBA, alpha ignored as PIL's ``convert("RGB")`` drops it), host or
        device, any row stride -> the level-0 coords int64 [N,2] ``(x, y)`` of the kept cells, on the region's device.

        Cells of side ``patch_size`` sit at ``(gx step, gy step)`` (``step`` defaults to ``patch_size``) wherever they lie wholly inside
        the region, in row-major order; coords are ``(origin + cell offset) * coord_scale`` (the convention of refine_seg / cood2str and
        the CLAM .h5 files; ``coord_scale`` for a region read at a downsampled level).  ``tissue`` (default off: every cell) is an exact
        integer rule (keep_amd.region.TissueRule): a pixel is tissue iff ``max(r,g,b) > 0`` and ``255 (max - min) >= sat_min max``, a cell
        is kept iff it holds ``>= ceil(min_fraction patch^2)`` of them.  That rule is deliberately NOT CLAM's contour segmentation;
        a ``keep_amd.region.TissueMask`` (from :meth:`tissue_mask`, or a caller's own) is the other choice: a cell is then tested at
        CLAM's ``four_pt`` / ``four_pt_hard`` / ``center`` points, in level coordinates including ``origin``, against the mask
        (DESIGN.md section 11), and the region's pixels are not read.  ``quality``: a ``keep_amd.quality.QualityGate``; the cells of the
        grid (by rule or by mask) are then measured in the region (:meth:`region_quality`, ``patch_size <= 1024``) and those the gate
        rejects are dropped, the rest staying in grid order; ``None`` changes nothing."""
        patch, step, origin, coord_scale = check_grid_args(patch_size, step, origin, coord_scale)
        if check_gate(quality) is not None:
            check_patch(patch)
        x = self._region_tensor(region)
        if isinstance(tissue, TissueMask):                         # decided by the mask: the region gives its shape, no pixel is read
            self._ready_device()
            H, W, _, _ = region_layout(x)
            cells = self._mask_cells(tissue, H, W, patch, step, origin)
            if quality is not None:
                xd, H, W, C, row = self._region_on_device(x)
        else:
            sat_min, min_pixels = tissue_params(tissue, patch)
            self._ready_device()
            xd, H, W, C, row = self._region_on_device(x)
            cells = self._region_cells(xd, H, W, C, row, patch, step, sat_min, min_pixels)
        if quality is not None:
            cells = self._quality_cells(xd, H, W, C, row, cells, patch, quality)
        coords = self._cells_to_coords(cells, origin, coord_scale)
        return coords if x.device == self._device else coords.to(x.device)

    @torch.no_grad()
    def region_patches_uint8(self, region, coords: torch.Tensor, patch_size: int, origin=(0, 0), coord_scale: int = 1, stain=None) -> torch.Tensor:
        """The tiles of ``coords`` (as :meth:`region_grid` returns them, same ``origin`` / ``coord_scale``) cut from ``region`` on the
        device -> uint8 [N,224,224,3]: the patches themselves at ``patch_size == 224``, else the reference transform's
        ``Resize(224, BICUBIC)`` + ``CenterCrop(224)`` of each patch, bit-identical to PIL.  A coord outside the region is a ValueError.
        ``stain``: a ``StainFit`` (:meth:`stain_fit`) maps the cut tiles to the default stain target (:meth:`stain_normalize`, after
        the resize); ``None`` leaves them as cut."""
        patch, _, origin, coord_scale = check_grid_args(patch_size, None, origin, coord_scale)
        check_stain(stain)
        coords = torch.as_tensor(coords)
        if coords.dim() != 2 or coords.shape[1] != 2:
            raise ValueError(f"coords must be [N,2] (x, y), got {tuple(coords.shape)}")
        x = self._region_tensor(region)
        self._ready_device()
        plan = None if stain is None else self._stain_plan(stain)
        xd, H, W, C, row = self._region_on_device(x)
        c = coords.to(self._device, torch.int64)
        cells = (torch.div(c, coord_scale, rounding_mode="floor") - torch.tensor(origin, dtype=torch.int64, device=self._device))
        cells = cells.clamp(-(1 << 31), (1 << 31) - 1).to(torch.int32)          # out of int32 range stays outside the region
        out = self._region_tiles(xd, H, W, C, row, cells, patch)
        if plan is not None and out.numel():
            self._stain_apply(out, out, plan)
        return out if x.device == self._device else out.to(x.device)

    @torch.no_grad()
    def encode_region(self, region, patch_size: int = 224, step: Optional[int] = None, tissue=None, origin=(0, 0), coord_scale: int = 1,
                      batch: int = 256, stain=None, quality: Optional[QualityGate] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Slide pixels in, what the WSI functions take out: the grid of :meth:`region_grid`, the tiles of
        :meth:`region_patches_uint8` and :meth:`encode_image_uint8`, ``batch`` tiles at a time -> (features fp32 [N,768],
        coords int64 [N,2]) on the region's device; ``[0,768]`` / ``[0,2]`` when no cell is kept.  ``tissue`` as in
        :meth:`region_grid`: off, the per-pixel rule, or a ``TissueMask``.  ``stain``: a ``StainFit`` normalises every batch of cut tiles
        (after the resize to 224, before the encoder) as :meth:`stain_normalize` does; ``None`` changes nothing.  ``quality``: a
        ``QualityGate`` drops the cells it rejects as in :meth:`region_grid`, before any tile is cut or encoded and on the pixels as
        scanned (not stain-normalised); features and coords come back for the kept cells only, in grid order; ``None`` changes nothing."""
        return self._encode_region(region, patch_size, step, tissue, origin, coord_scale, batch, None, stain, quality)[:2]

    @torch.no_grad()
    def encode_region_attention(self, region, patch_size: int = 224, step: Optional[int] = None, tissue=None, origin=(0, 0),
                                coord_scale: int = 1, batch: int = 256, block: int = -1, stain=None,
                                quality: Optional[QualityGate] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """:meth:`encode_region` with the CLS query's attention of block ``block`` for every tile (``encode_image_attention``;
        DESIGN.md section 19) -> (features [N,768], coords [N,2], attn fp32 [N, heads, 197]) on the region's device.  Same grid, same
        tiles; the features equal :meth:`encode_region`'s with option ``graphs`` = 0 bit for bit."""
        self._ready()
        self._check_block(block)
        return self._encode_region(region, patch_size, step, tissue, origin, coord_scale, batch, block, stain, quality)

    @torch.no_grad()
    def encode_region_rollout(self, region, patch_size: int = 224, step: Optional[int] = None, tissue=None, origin=(0, 0), coord_scale: int = 1,
                              batch: int = 256, start_block: int = 0, residual: float = 0.5, stain=None,
                              quality: Optional[QualityGate] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """:meth:`encode_region` with every tile's attention rollout (``encode_image_rollout``) -> (features
        [N,768], coords [N,2], rollout fp32 [N, 1, 197]) on the region's device.  Same grid, same tiles; the features equal
        :meth:`encode_region`'s with option ``graphs`` = 0 bit for bit."""
        self._ready()
        self._check_rollout(start_block, residual, (TILE // 16) ** 2 + 1)
        return self._encode_region(region, patch_size, step, tissue, origin, coord_scale, batch, ("rollout", start_block, residual), stain, quality)

    def _encode_region(self, region, patch_size, step, tissue, origin, coord_scale, batch, block, stain=None, quality=None):
        """The body of :meth:`encode_region`.  ``block`` an int: the tiles go through the tapped encode -> (features, coords, attn
        [N, heads, 197]); ``("rollout", start_block, residual)``: through the rollout encode -> (features, coords, rollout [N, 1, 197])."""
        rollout = isinstance(block, tuple)
        patch, step, origin, coord_scale = check_grid_args(patch_size, step, origin, coord_scale)
        by_mask = isinstance(tissue, TissueMask)
        sat_min, min_pixels = (0, 0) if by_mask else tissue_params(tissue, patch)
        if isinstance(batch, bool) or int(batch) != batch or batch < 1:
            raise ValueError(f"batch must be an integer >= 1, got {batch!r}")
        x = self._region_tensor(region)
        check_stain(stain)
        if check_gate(quality) is not None:
            check_patch(patch)
        self._ready()
        plan = None if stain is None else self._stain_plan(stain)
        xd, H, W, C, row = self._region_on_device(x)
        cells = self._mask_cells(tissue, H, W, patch, step, origin) if by_mask else \
            self._region_cells(xd, H, W, C, row, patch, step, sat_min, min_pixels)
        if quality is not None:
            cells = self._quality_cells(xd, H, W, C, row, cells, patch, quality)
        N = int(cells.shape[0])
        feats = torch.empty((N, self.config.projection_dim), dtype=torch.float32, device=self._device)
        attn = None if block is None else torch.empty((N, 1 if rollout else self.config.vision.num_heads, (TILE // 16) ** 2 + 1),
                                                      dtype=torch.float32, device=self._device)
        for i in range(0, N, int(batch)):
            tiles = self._region_tiles(xd, H, W, C, row, cells[i:i + batch], patch)
            if plan is not None:
                self._stain_apply(tiles, tiles, plan)
            if block is None:
                feats[i:i + batch] = self.encode_image_uint8(tiles)
            elif rollout:
                feats[i:i + batch], attn[i:i + batch] = self._encode_rollout(tiles, _lib.PIX_U8_HWC, TILE, TILE, block[1], block[2], "encode_region_rollout")
            else:
                feats[i:i + batch], attn[i:i + batch] = self._encode_tapped(tiles, _lib.PIX_U8_HWC, TILE, TILE, block, "encode_region_attention")
        coords = self._cells_to_coords(cells, origin, coord_scale)
        out = (feats, coords) if block is None else (feats, coords, attn)
        return out if x.device == self._device else tuple(t.to(x.device) for t in out)
