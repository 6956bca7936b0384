"""Slide regions -> patch grid, tissue rule, coords: the host side of ``KEEPModel.region_grid`` /
``region_patches_uint8`` / ``encode_region`` and of ``cohort.extract_slide_features``.

  * argument checks that run before any device call (``check_grid_args``, ``tissue_params``);
  * the Resize(224, BICUBIC) tables of a patch size, built once per (size, device) (``resize_tables``);
  * the band planner that walks a slide in horizontal bands of whole grid rows (``plan_bands``);
  * a numpy restatement of the grid and the tissue rule, the yardstick of the device kernels (``region_grid_numpy``).

The tissue rule is a per-pixel integer test, NOT CLAM's contour segmentation (median blur + Otsu on saturation + contour
filtering, README.md:74 of the reference): a pixel is tissue iff ``max(r,g,b) > 0`` and ``255 (max - min) >= sat_min max``
(HSV saturation >= sat_min / 255, exact in integers); a cell is kept iff it holds at least ``ceil(min_fraction p^2)`` of them.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch

TILE = 224


@dataclass(frozen=True)
class TissueRule:
    """Keep a grid cell iff at least ``min_fraction`` of its pixels have HSV saturation >= ``sat_min`` (0..255 scale).
    Glass (near-white, grey, black) has saturation near 0; H & E stain well above 20."""
    sat_min: int = 20
    min_fraction: float = 0.25


TissueArg = Union[None, bool, TissueRule, Tuple[int, float], Dict[str, float]]


def tissue_params(tissue: TissueArg, patch: int) -> Tuple[int, int]:
    """-> (sat_min, min_pixels) for the kernel; the rule off is (0, 0): every cell is kept, no pixel is read."""
    if tissue is None or tissue is False:
        return 0, 0
    if tissue is True:
        rule = TissueRule()
    elif isinstance(tissue, TissueRule):
        rule = tissue
    elif isinstance(tissue, dict):
        rule = TissueRule(**tissue)
    elif isinstance(tissue, (tuple, list)) and len(tissue) == 2:
        rule = TissueRule(*tissue)
    else:
        raise ValueError(f"tissue: None, True, a TissueRule, (sat_min, min_fraction) or a dict, got {tissue!r}")
    if int(rule.sat_min) != rule.sat_min or not 0 <= rule.sat_min <= 255:
        raise ValueError(f"tissue sat_min must be an integer in [0, 255], got {rule.sat_min!r}")
    if not 0.0 <= float(rule.min_fraction) <= 1.0:
        raise ValueError(f"tissue min_fraction must lie in [0, 1], got {rule.min_fraction!r}")
    return int(rule.sat_min), int(math.ceil(float(rule.min_fraction) * patch * patch))


def check_grid_args(patch: int, step: Optional[int], origin=(0, 0), coord_scale: int = 1) -> Tuple[int, int, Tuple[int, int], int]:
    """Validate the grid arguments on the host -> (patch, step, origin, coord_scale); ``step=None`` means ``step = patch``."""
    if isinstance(patch, bool) or int(patch) != patch or patch < 16:
        raise ValueError(f"patch_size must be an integer >= 16, got {patch!r}")
    patch = int(patch)
    step = patch if step is None else step
    if isinstance(step, bool) or int(step) != step or step < 1:
        raise ValueError(f"step must be an integer >= 1, got {step!r}")
    if isinstance(coord_scale, bool) or int(coord_scale) != coord_scale or coord_scale < 1:
        raise ValueError(f"coord_scale must be an integer >= 1, got {coord_scale!r}")
    if len(origin) != 2 or any(int(o) != o for o in origin):
        raise ValueError(f"origin must be two integers (x, y), got {origin!r}")
    return patch, int(step), (int(origin[0]), int(origin[1])), int(coord_scale)


def region_layout(region: torch.Tensor) -> Tuple[int, int, int, int]:
    """uint8 [H,W,C], C in (3, 4), channels contiguous and pixels C bytes apart -> (H, W, C, row_stride_bytes)."""
    if region.dtype != torch.uint8 or region.dim() != 3 or region.shape[2] not in (3, 4):
        raise ValueError(f"region must be uint8 [H,W,3] (RGB) or [H,W,4] (RGBA), got {region.dtype} {tuple(region.shape)}")
    H, W, C = (int(v) for v in region.shape)
    if H < 1 or W < 1:
        raise ValueError(f"region is empty: {tuple(region.shape)}")
    s0, s1, s2 = region.stride()
    if (C > 1 and s2 != 1) or (W > 1 and s1 != C):
        raise ValueError(f"region pixels must be {C} contiguous bytes (strides (*, {C}, 1)), got strides {region.stride()}")
    row = s0 if H > 1 else W * C
    if row < W * C:
        raise ValueError(f"region row stride {row} < W * C = {W * C}")
    return H, W, C, row


def grid_shape(H: int, W: int, patch: int, step: int) -> Tuple[int, int]:
    """(rows, columns) of the grid: every cell wholly inside the region."""
    return ((H - patch) // step + 1 if H >= patch else 0), ((W - patch) // step + 1 if W >= patch else 0)


def region_grid_numpy(region: np.ndarray, patch: int, step: Optional[int] = None, sat_min: int = 0, min_pixels: int = 0) -> np.ndarray:
    """The grid + tissue rule restated on the host: uint8 [H,W,3|4] -> kept cells' (x, y) pixel offsets, int64 [N,2], row-major."""
    step = patch if step is None else step
    H, W = region.shape[:2]
    gy, gx = grid_shape(H, W, patch, step)
    if min_pixels > 0 and gy and gx:
        rgb = region[..., :3].astype(np.int64)
        mx, mn = rgb.max(axis=2), rgb.min(axis=2)
        tissue = ((mx > 0) & (255 * (mx - mn) >= sat_min * mx)).astype(np.int64)
        ii = np.zeros((H + 1, W + 1), np.int64)                # summed-area table: exact window counts
        ii[1:, 1:] = tissue.cumsum(0).cumsum(1)
        ys, xs = np.arange(gy) * step, np.arange(gx) * step
        cnt = ii[ys[:, None] + patch, xs[None, :] + patch] - ii[ys[:, None], xs[None, :] + patch] - ii[ys[:, None] + patch, xs[None, :]] \
            + ii[ys[:, None], xs[None, :]]
        keep = cnt >= min_pixels
    else:
        keep = np.ones((gy, gx), bool)
    yy, xx = np.nonzero(keep)                                  # row-major: y outer, x inner
    return np.stack([xx * step, yy * step], axis=1).astype(np.int64).reshape(-1, 2)


def plan_bands(width: int, height: int, patch: int, step: Optional[int] = None, band_rows: int = 8) -> List[Tuple[int, int, int, int]]:
    """Horizontal bands of ``band_rows`` grid rows -> [(r0, r1, y0, h)]: band k holds grid rows [r0, r1) and covers pixel rows
    [y0, y0 + h) = [r0 step, (r1 - 1) step + patch), so every grid cell of the whole slide falls in exactly one band."""
    patch, step, _, _ = check_grid_args(patch, step)
    if isinstance(band_rows, bool) or int(band_rows) != band_rows or band_rows < 1:
        raise ValueError(f"band_rows must be an integer >= 1, got {band_rows!r}")
    if width < 1 or height < 1:
        raise ValueError(f"slide size must be positive, got {width}x{height}")
    gy, _ = grid_shape(height, width, patch, step)
    return [(r0, min(r0 + band_rows, gy), r0 * step, (min(r0 + band_rows, gy) - 1 - r0) * step + patch) for r0 in range(0, gy, band_rows)]


_TABLES: Dict[Tuple[int, str], tuple] = {}


def resize_tables(patch: int, device: torch.device) -> tuple:
    """Pillow's Resize(224, BICUBIC) tables of a square ``patch`` (the same for both axes; CenterCrop(224) is then the
    identity) on ``device`` -> (bounds, weights, ksize); built in float64 by ``pil_bicubic_coeffs`` once per (patch, device)."""
    from .preprocess import pil_bicubic_coeffs
    key = (int(patch), str(device))
    if key not in _TABLES:
        b, k, ks = pil_bicubic_coeffs(int(patch), TILE)
        _TABLES[key] = (torch.from_numpy(b).to(device).contiguous(), torch.from_numpy(k).to(device).contiguous(), ks)
    return _TABLES[key]
