"""Host-side mirror of the reference's model API on top of libkeep_hip.

``KEEPModel`` keeps the surface of ``KEEPModel`` in ``quick_start/keep_inference.py:25-73`` (the
class HF ``AutoModel.from_pretrained('Astaxanthin/KEEP', trust_remote_code=True)`` returns in
``WSI_evaluation/zeroshot_*_WSI.py``): ``encode_image``, ``encode_text``, ``forward``, ``eval``,
``to``, ``load_state_dict``, ``logit_scale`` -- same argument meaning, same output shapes/dtypes,
L2-normalised fp32 features on the caller's device.  Underneath there is no torch module: tensors
are handed to the C ABI as raw device pointers; torch supplies storage, streams and file loading.

There is no CPU execution path.  Inputs that live on the CPU are copied to the engine's GPU and the
result is copied back; without a GPU (or without libkeep_hip.so) every call raises.

How the 'comp' mode's per-block plan is chosen -- the rule, the statistics, the search -- is ``keep_amd.calibration`` (pure functions, testable on a
CPU); ``KEEPModel.calibrate`` only drives it: it encodes the probe and applies what comes back.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
import weakref
from typing import Dict, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
# how the 'comp' plan is chosen lives in keep_amd.calibration; its public names stay importable from here
from .calibration import (ATTN_RESIDUAL, CALIBRATION_POPULATION, COMP_LADDER, CONFIDENCE, DEFAULT_KNOBS, KNOB_COST_MS, MLP_RESIDUAL,  # noqa: F401
                          PROBE_RMS_MARGIN, TOLERANCE, Plan, calibration_report, default_probe, exceedance_probability, expected_max_sigmas,
                          greedy_walk, label_margin_unit, ladder_candidates, max_sigmas_gumbel, max_sigmas_quantile, measure_shares,
                          mixture_exceedance, mixture_max_quantile, plan_prefix, plan_string, prefix_plan, probe_members, probe_statistics,
                          search, share_probe, walk_candidates)
from .config import KEEPShape
from .slide import SlideOps, _ptr, _stream

_PIX = {torch.float32: _lib.PIX_F32, torch.float16: _lib.PIX_F16, torch.bfloat16: _lib.PIX_BF16}
_PRECISIONS = {"fp16": _lib.PREC_FP16, "strict": _lib.PREC_STRICT, "comp": _lib.PREC_COMP}
DEFAULT_PRECISION = "comp"     # the mode that meets the reference tolerance (cosines within 1e-4) at the lowest cost


class KEEPModel(SlideOps):
    """Drop-in for the reference ``KEEPModel`` (inference only)."""

    # engines that own a handle, newest last: the slide-level functions of keep_amd.wsi take no model argument (the reference's are plain
    # torch code, WSI_evaluation/utils.py:107-146) and find the engine of their device here (keep_amd.model.engine_for)
    _live: "List[weakref.ref]" = []

    def __init__(self, config: Optional[Union[KEEPShape, Mapping, str]] = None, precision: str = DEFAULT_PRECISION,
                 towers=("image", "text"), dynamic_img_size: bool = False):
        if config is None:
            config = KEEPShape()
        elif not isinstance(config, KEEPShape):
            config = KEEPShape.from_config_json(config)
        self.config = config
        # timm's dynamic_img_size (keep_inference.py:32-40 builds the ViT with it): True = encode_image / encode_image_uint8 / forward take tiles of
        # any H, W that are multiples of 16 (one size per call; the position embedding is resampled to the patch grid, keep_encode_image_hw).
        # False (default) = 224 x 224 only, as before.  classify, encode_image_raw and the WSI functions stay 224-only either way.
        self.dynamic_img_size = bool(dynamic_img_size)
        # nn.Parameter(torch.ones([]) * log(1/0.04)) -- keep_inference.py:52 (never applied at inference)
        self.logit_scale = torch.tensor(config.logit_scale_init, dtype=torch.float32)
        self.training = False
        self._handle = C.c_void_p(0)
        self._device: Optional[torch.device] = None
        self._heat_luts: Dict[str, torch.Tensor] = {}           # render_heatmap's named colour tables on the device
        self._host_sd: Optional[Dict[str, torch.Tensor]] = None
        self._loaded = False
        self._options = {"precision": _PRECISIONS[precision], "strict_blocks": 0}
        self._plan: Optional[Plan] = None        # per-block plan set through set_plan (re-applied whenever the handle is re-created)
        # load_state_dict(strict=True) demands the keys of every tower named here (the reference's model has both,
        # keep_inference.py:28-52); a single-tower engine -- e.g. an encode_image-only worker -- opts in with towers=("image",)
        self.towers = tuple(towers)
        if not self.towers or any(t not in ("image", "text") for t in self.towers):
            raise ValueError(f"towers must be a non-empty subset of ('image', 'text'), got {towers!r}")
        # out-of-range token ids raise IndexError, as nn.Embedding does.  True: checked before encode_text returns (one host
        # synchronisation per call); "lazy": the flag is copied back asynchronously and the error is raised by the NEXT engine call
        # or by check_errors() -- no synchronisation, which is also how the reference's CUDA path reports it (device-side assert);
        # False: never checked -- and that includes the non-finite-feature bit (an activation beyond the fp16 range of the engine's stores reaches the
        # output as NaN; with False nothing raises, the caller sees the NaNs).  The reference's WSI scripts make thousands of one-prompt calls, so the
        # default is "lazy".
        self.check_token_ids = "lazy"
        self._pending_token_checks = []   # [(pinned int32 flag, event)] in issue order; the device flag is sticky, so none can be lost
        self._flag_pool = []              # pinned buffers are recycled only after their copy has landed
        # load_state_dict on a GPU ends with calibrate(): the cheapest 'comp' setting whose worst cosine error on a seeded probe batch
        # (against the engine's own split-product arithmetic) predicts a worst error inside the tolerance over CALIBRATION_POPULATION cosines.  KEEP_CALIBRATE=0 / auto_calibrate=False: keep the
        # plan a handle starts with (block 0 treated in full, the CLS rows' MLP redone as split products everywhere else), which no measurement on THESE weights backs.
        self.auto_calibrate = os.environ.get("KEEP_CALIBRATE", "1") != "0"
        # "measured": one split-product encode of a 64-tile probe per block and half ranks the knobs for THESE weights, then a greedy plan is verified
        # (about 2 s at load for ViT-L); "ladder": the prefix family COMP_LADDER only (under 1 s, up to 12 % slower plans -- profiles/r05_precision_budget.md)
        self.calibration_budget = os.environ.get("KEEP_CALIBRATION_BUDGET", "measured")
        self.calibration: Optional[dict] = None
        self._label_margin_unit: Optional[float] = None      # calibrate(): classify's second-look margin per unit of prompt distance
        # what calibrate() / calibrate_bias() probe when the caller passes no tiles: "mixture" = N(0,1) pixels AND the structured tile families of
        # keep_amd.synth.calibration_probe, the plan being held to the WORST family; "gaussian" = N(0,1) pixels only (round 5's probe: it does not
        # hold the tolerance on structured tiles -- profiles/r06_offdist_parity_before_repair_gaussian_probe.json)
        self.calibration_probe = os.environ.get("KEEP_CALIBRATION_PROBE", "mixture")
        # load_state_dict on a GPU also runs calibrate_bias(): the mean-input compensation of the weight-rounding error that the plain fp16 launches use
        # (keep_calibrate_bias; KEEP_BIAS_CORRECTION=0 / bias_correction=False: the checkpoint's own biases everywhere)
        # Round 6: OFF by default.  The correction is exact for the mean input row of the tiles it was calibrated on and only for it: calibrated on N(0,1)
        # tiles it adds error on glass background, calibrated on the mixture probe it adds error on N(0,1) tiles, and the plan calibrate() then needs
        # is dearer with it than without (profiles/r06_offdist_parity_*.json).  A caller who knows their tiles opts in: calibrate_bias(tiles=own) + calibrate(tiles=own).
        self.bias_correction = os.environ.get("KEEP_BIAS_CORRECTION", "0") != "0"
        self.trim_padding = True      # encode_text at the longest valid length instead of the padded one (same result)
        self.last_text_length = 0     # T the text tower actually ran at in the last encode_text call

    # ------------------------------------------------------------------ lifetime
    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    def _destroy(self):
        if getattr(self, "_handle", None) is not None and self._handle.value:
            _lib.load().keep_destroy(self._handle)
            self._handle = C.c_void_p(0)
            self._loaded = False

    def _create(self, device: torch.device):
        lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.KeepHipError("no GPU visible: keep_amd has no CPU execution path")
        if device.type != "cuda":
            raise ValueError(f"keep_amd runs on a ROCm GPU ('cuda:N'), not on {device}")
        idx = device.index if device.index is not None else torch.cuda.current_device()
        h = C.c_void_p(0)
        rc = lib.keep_create(idx, C.byref(h))
        if rc != _lib.KEEP_OK:
            raise _lib.KeepHipError(f"keep_create(device={idx}) failed with code {rc}")
        self._handle = h
        self._device = torch.device("cuda", idx)
        KEEPModel._live[:] = [r for r in KEEPModel._live if r() is not None and r() is not self] + [weakref.ref(self)]
        self._apply_options()

    def _apply_options(self):
        """Push the stored options, then the per-block plan (the comp_* shorthands rewrite the plan, so it goes last)."""
        lib, h = _lib.load(), self._handle
        for k, v in self._options.items():
            _lib.check(h, lib.keep_set_option(h, k.encode(), float(v)), k)
        if self._plan is not None:
            for i, (a, m) in enumerate(self._plan):
                _lib.check(h, lib.keep_set_block_precision(h, i, int(a), int(m)), "set_block_precision")

    # ------------------------------------------------------------------ nn.Module-like surface
    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("keep_amd is an inference engine; training is out of scope")
        return self.eval()

    def requires_grad_(self, flag: bool = False):
        return self

    @property
    def device(self) -> torch.device:
        return self._device if self._device is not None else torch.device("cpu")

    def to(self, device=None, *args, **kwargs):
        if device is None:
            return self
        device = torch.device(device)
        if device.type == "cpu":
            if self._loaded:
                raise _lib.KeepHipError("keep_amd has no CPU execution path; the model stays on its GPU")
            return self
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        if self._loaded and self._device == device:
            return self
        if self._loaded and self._host_sd is None:
            raise _lib.KeepHipError("weights were already uploaded and the host copy released; "
                                    "reload the state_dict to move to another GPU")
        self._destroy()
        self._create(device)
        if self._host_sd is not None:
            self._upload(self._host_sd)
            self._host_sd = None
        return self

    cuda = lambda self, device=None: self.to(torch.device("cuda", device) if isinstance(device, int) else (device or "cuda"))

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, state_dict: Mapping[str, torch.Tensor], strict: bool = True):
        """``model.load_state_dict(state_dict, strict=True)`` -- keep_inference.py:83.

        Key layout: SURVEY.md §A.3.  On a model that is already on a GPU the tensors are repacked
        immediately; otherwise they are held (by reference) until ``.to('cuda')``.
        """
        sd = {k: v for k, v in state_dict.items()}
        if "logit_scale" in sd:
            self.logit_scale = sd["logit_scale"].detach().to("cpu", torch.float32).reshape(())
        self._strict = strict
        if self._handle.value:
            self._upload(sd)
        else:
            self._host_sd = sd
        return self

    def _upload(self, sd: Mapping[str, torch.Tensor]):
        lib, h = _lib.load(), self._handle
        errors = []
        for key, t in sd.items():
            if not isinstance(t, torch.Tensor):
                continue
            t = t.detach()
            on_dev = t.device.type == "cuda" and t.device == self._device
            src = t.to(torch.float32).contiguous() if on_dev else t.to("cpu", torch.float32).contiguous()
            shape = (C.c_int64 * max(src.dim(), 1))(*src.shape)
            rc = lib.keep_load_tensor(h, key.encode(), _ptr(src), src.dim(), shape, 1 if on_dev else 0)
            if rc == _lib.KEEP_EKEY:
                if getattr(self, "_strict", True):
                    errors.append(lib.keep_last_error(h).decode())
            else:
                _lib.check(h, rc, key)
        if errors:
            raise RuntimeError("Error(s) in loading state_dict for KEEPModel:\n\t" + "\n\t".join(errors))
        notes = lib.keep_load_warnings(h).decode()
        if notes:
            import warnings
            for line in notes.split("\n"):
                warnings.warn(line, RuntimeWarning, stacklevel=3)
        rc = lib.keep_finalize_weights(h)
        if rc == _lib.KEEP_EKEY:
            raise RuntimeError("Error(s) in loading state_dict for KEEPModel:\n\t" + lib.keep_last_error(h).decode())
        _lib.check(h, rc, "finalize_weights")
        if getattr(self, "_strict", True):
            missing = []
            if "image" in self.towers and lib.keep_vit_depth(h) == 0:
                missing.append("visual.* / visual_head.* (image tower)")
            if "text" in self.towers and lib.keep_bert_layers(h) == 0:
                missing.append("text.* (text tower)")
            if missing:
                raise RuntimeError("Error(s) in loading state_dict for KEEPModel:\n\tMissing key(s) in state_dict: " + ", ".join(missing)
                                   + ' (construct with towers=("image",) / ("text",) for a single-tower engine)')
        self._loaded = True
        self._label_margin_unit = None
        self._weights_epoch = getattr(self, "_weights_epoch", 0) + 1      # invalidates per-model prompt caches (keep_amd.wsi)
        self.calibration = None
        if self.auto_calibrate and lib.keep_vit_depth(h) > 0:
            if self.bias_correction and self._options["precision"] != _lib.PREC_STRICT:
                self.calibrate_bias()
            if self._options["precision"] == _lib.PREC_COMP:
                self.calibrate()

    @classmethod
    def from_pretrained(cls, path: str, precision: str = DEFAULT_PRECISION, **_ignored) -> "KEEPModel":
        """Load a release directory (``config.json`` + ``pytorch_model.bin`` or ``model.safetensors``),
        the local-files equivalent of ``AutoModel.from_pretrained`` at zeroshot_subtyping_WSI.py:44."""
        cfg_path = os.path.join(path, "config.json")
        config = KEEPShape.from_config_json(cfg_path) if os.path.exists(cfg_path) else KEEPShape()
        model = cls(config, precision=precision, towers=_ignored.pop("towers", ("image", "text")),
                    dynamic_img_size=_ignored.pop("dynamic_img_size", False))
        st = os.path.join(path, "model.safetensors")
        pt = os.path.join(path, "pytorch_model.bin")
        if os.path.exists(st):
            from safetensors.torch import load_file
            sd = load_file(st)
        elif os.path.exists(pt):
            sd = torch.load(pt, map_location="cpu")
        else:
            raise FileNotFoundError(f"no model.safetensors / pytorch_model.bin under {path}")
        model.load_state_dict(sd, strict=True)
        return model

    # ------------------------------------------------------------------ options
    def set_precision(self, precision: str = DEFAULT_PRECISION, strict_blocks: int = 0):
        """'comp' (default): fp16 MFMA pass plus the first-order correction terms where the error budget needs them
        (MX-fp4 correction passes in the image tower's MLP GEMMs, split products in its first blocks and in the text
        tower): cosines within 1e-4 of the fp32 reference.  'fp16': single fp16 pass everywhere (fastest; ~1.5e-4, outside
        the tolerance -- opt-in).  'strict': hi/lo split operands, three MFMA passes (4e-7, ~0.4x the speed).
        ``strict_blocks=n`` additionally runs the first n transformer blocks of each tower in split mode."""
        self._options["precision"] = _PRECISIONS[precision]
        self._options["strict_blocks"] = int(strict_blocks)
        if self._handle.value:
            self._apply_options()
        return self

    _PLAN_SHORTHANDS = ("comp_full_blocks", "comp_mlp_blocks", "comp_qkv", "comp_qkv_from")

    def set_option(self, name: str, value: float):
        self._options[name] = value
        if name == "label_margin":
            self._label_margin_unit = None        # an explicit threshold replaces the calibrated, bank-scaled one
        if name in self._PLAN_SHORTHANDS:
            self._plan = None                 # the engine rewrites the whole per-block plan from the shorthands
        if self._handle.value:
            _lib.check(self._handle, _lib.load().keep_set_option(self._handle, name.encode(), float(value)), name)
        return self

    def set_plan(self, plan: Sequence[Tuple[int, int]]):
        """The per-block plan of the 'comp' mode: ``plan[i] = (attention-side mode, MLP mode)`` of ViT block i (``_lib.ATTN_*`` / ``_lib.MLP_*``,
        = KEEP_ATTN_* / KEEP_MLP_* of include/keep_hip.h).  Blocks beyond ``len(plan)`` run plain fp16 passes."""
        plan = [(int(a), int(m)) for a, m in plan]
        if any(not (0 <= a <= 5 and 0 <= m <= 4) for a, m in plan) or len(plan) > 64:
            raise ValueError("a plan holds at most 64 (attn_mode 0..5, mlp_mode 0..4) pairs")
        pre = plan_prefix(plan)
        for k in self._PLAN_SHORTHANDS:
            self._options.pop(k, None)
        if pre is not None:                   # a prefix plan is stored as its shorthand (and reads back through get_option); the handle's qkv
            # variants of the shorthand are reset first, so that what the engine rebuilds from the prefix is exactly `plan`
            self._options["comp_qkv"], self._options["comp_qkv_from"] = 0, 1 << 20
            self._options["comp_full_blocks"], self._options["comp_mlp_blocks"] = pre
            self._plan = None
        else:
            self._options["comp_full_blocks"] = self._options["comp_mlp_blocks"] = 0
            self._plan = plan + [(0, 0)] * (64 - len(plan))
        if self._handle.value:
            self._apply_options()
        return self

    def get_plan(self) -> Plan:
        """What the engine will run per ViT block in the 'comp' mode (read back from the handle)."""
        self._ready_device()
        lib, h = _lib.load(), self._handle
        depth = int(lib.keep_vit_depth(h)) or self.config.vision.depth
        out, a, m = [], C.c_int(0), C.c_int(0)
        for i in range(depth):
            _lib.check(h, lib.keep_get_block_precision(h, i, C.byref(a), C.byref(m)), "get_block_precision")
            out.append((a.value, m.value))
        return out

    @torch.no_grad()
    def calibrate_bias(self, tiles: Optional[torch.Tensor] = None, n_tiles: int = 64, seed: int = 20250936, probe: Optional[str] = None) -> "KEEPModel":
        """Mean-input compensation of the weight-rounding error (``keep_calibrate_bias``): the engine encodes ``tiles`` in split products, averages the
        input rows of every GEMM of the image tower and folds ``W_lo @ mean_input`` into the bias its plain fp16 launches use -- the row-independent
        part of the term a single fp16 pass drops, at no cost per call.  The correction is exact for the MEAN input row of ``tiles`` and only for it:
        pass tiles of the caller's own distribution for a closer mean.  Default (``probe="mixture"``): ``n_tiles`` tiles of
        ``keep_amd.synth.calibration_probe`` (N(0,1) pixels and the structured families in equal parts; round 6 -- calibrated on N(0,1) tiles alone
        (``probe="gaussian"``, what round 5 did) the compensation ADDS error on near-constant background tiles,
        profiles/r06_offdist_parity_before_repair_gaussian_probe.json).  ``calibrate()`` verifies whatever this leaves, family by family.  ``tiles`` of
        zero length forgets the calibration."""
        self._ready()
        dev = self._device
        if tiles is None:
            tiles = default_probe(probe or self.calibration_probe, n_tiles, dev, seed)[0]
        x = tiles.to(dev)
        if x.dtype not in _PIX and x.dtype != torch.uint8:
            x = x.to(torch.float32)
        x = x.contiguous()
        code = _lib.PIX_U8_HWC if x.dtype == torch.uint8 else _PIX[x.dtype]
        self._call("calibrate_bias", _ptr(x) if x.shape[0] else C.c_void_p(0), code, x.shape[0])
        self._weights_epoch = getattr(self, "_weights_epoch", 0)      # (text features do not depend on it: the prompt caches stay valid)
        return self

    @torch.no_grad()
    def calibrate(self, n_tiles: int = 1024, population: Optional[float] = None, tiles: Optional[torch.Tensor] = None,
                  text_features: Optional[torch.Tensor] = None, seed: int = 20250929, tolerance: float = TOLERANCE,
                  confidence: float = CONFIDENCE, budget: Optional[str] = None, knobs: Optional[Mapping] = None,
                  label_population: Optional[float] = None, groups: Optional[torch.Tensor] = None, group_names: Optional[Sequence[str]] = None,
                  probe: Optional[str] = None) -> Optional[dict]:
        """Pick the 'comp' plan for THESE weights and for the population the model will be used on.

        A probe batch is encoded once with split products (the engine's fp32-class arithmetic, ~5e-7 from the fp32 reference) and then with candidate
        plans from the cheapest up.  Kept: the first plan whose cosine errors over probe tiles x prompts predict, with probability ``confidence``
        (0.99), a worst error <= ``tolerance`` (1e-4) over ``population`` cosines (tiles x distinct prompts the caller will compare; default
        ``CALIBRATION_POPULATION`` = a 100 000-tile slide x the 264 distinct prompts of the RCC bank, BASELINE config 4):

            max over tile groups g of  mixture_max_quantile({sigma_t : t in g}, population, confidence) <= tolerance,
            sigma_t = (isotropic error of probe tile t) x anisotropy x margin_g x tail_g

        i.e. the ``confidence`` quantile of the largest of ``population`` Gaussian errors whose standard deviations are spread like the group's
        per-tile errors (tiles are not equally hard; for equal sigmas this is rms x max_sigmas_quantile(population, confidence)).

        The probe: ``tiles`` (with ``groups``, an int64 group index per tile, when they come from several distributions) or, by default
        (``probe="mixture"``), ``n_tiles`` tiles of ``keep_amd.synth.calibration_probe`` -- N(0,1) pixels (BASELINE config 2) and the structured
        families (stain fields, glass background, half / half) in equal parts, one group each.  The plan is held to the WORST group: a slide can be
        all tissue or mostly glass, and rounding errors behave differently there -- on spatially correlated tiles most of the error vector is COMMON
        to the tiles of a family (it does not average out across rows in attention, and the knobs that fix N(0,1) tiles leave it alone; round 6,
        profiles/r06_offdist_parity_*.json).  ``probe="gaussian"`` = round 5's probe.

        ``rms_g`` = the group's ISOTROPIC rms |feature error| / sqrt(D) -- what the rms would be against prompts in random directions -- times one
        anisotropy factor for the plan: the median over the groups of (rms against the probe's prompt bank / isotropic rms), at least 1 (error
        vectors are not isotropic; but the bank rms of a group of near-identical tiles is one random draw, so no single group's ratio is trusted).
        ``margin_g`` >= PROBE_RMS_MARGIN = two standard errors of the group's mean squared error, estimated from its tile-to-tile spread (one tile's
        cosines share ONE error vector).  ``tail_g`` >= 1 only when the group's own maximum is larger than its per-tile mixture allows a sample of the
        probe's size at 99 %.  ``model.calibration`` reports the prediction, the per-group figures and the ``exceedance_probability`` of the chosen plan.
        Candidates: ``budget="ladder"`` walks ``COMP_LADDER`` (prefix plans); ``budget="measured"`` first measures, on these weights and per group,
        the variance share of every block's attention side and MLP (one split-product encode per block and half with that one site downgraded),
        then builds the plan greedily -- each step the upgrade that lowers the worst group's predicted variance most per millisecond
        (``KNOB_COST_MS``) -- and verifies it the same way.  The prompts are ``text_features`` ([P,768] unit rows -- pass the caller's own bank to
        calibrate against it; default: 64 seeded prompts through the loaded text tower, or 64 seeded random unit vectors for an image-only engine,
        a harsher yardstick).  If nothing qualifies the engine switches to 'strict'.  ``label_margin`` (keep_classify's second-look threshold) is set
        from the measured rms.  Non-finite probe features (an activation beyond the fp16 range) raise FloatingPointError.  ``strict_blocks`` is
        kept; on an exception the previous setting is restored.  Returns and stores ``self.calibration``."""
        lib, h = _lib.load(), self._handle
        if not self._loaded and self._host_sd is not None:
            self.to("cuda")
            if self.calibration is not None:
                return self.calibration
        if not h.value or lib.keep_vit_depth(h) == 0 or self._options["precision"] != _lib.PREC_COMP:
            return None
        budget = budget or self.calibration_budget
        if budget not in ("ladder", "measured"):
            raise ValueError("budget must be 'ladder' or 'measured'")
        dev, depth = self._device, int(lib.keep_vit_depth(h))
        population = float(CALIBRATION_POPULATION if population is None else population)
        probe_name = "caller's tiles"
        if tiles is None:
            probe_name = probe or self.calibration_probe
            tiles, groups, group_names = default_probe(probe_name, n_tiles, dev, seed)
        tiles = tiles.to(dev)
        members = probe_members(groups, group_names, int(tiles.shape[0]), dev)
        if text_features is None:
            if lib.keep_bert_layers(h) > 0:
                from .synth import synth_prompts
                toks = synth_prompts(64, 64, seed=seed % 100003, vocab=self.config.text.vocab_size)
                text_features = self.encode_text({k: v.to(dev) for k, v in toks.items()})
            else:
                g = torch.Generator().manual_seed(seed + 1)
                text_features = torch.randn(64, self.config.projection_dim, generator=g).to(dev)
                _lib.check(h, lib.keep_op_l2norm(h, _ptr(text_features), 64, self.config.projection_dim, _stream(dev)), "l2norm")
        bank = text_features.to(dev, torch.float32).contiguous()
        saved_opts, saved_plan = dict(self._options), (list(self._plan) if self._plan is not None else None)
        strict_blocks = int(saved_opts.get("strict_blocks") or 0)
        was, self.auto_calibrate = self.auto_calibrate, False
        shares = None
        done = False

        def verify(plan: Plan):
            self.set_plan(plan)
            f = self._encode_probe(tiles)
            return probe_statistics(f, ref_f, self.similarity(f, bank), ref, members, population, confidence, tolerance)

        def iso_var(plan: Plan):              # isotropic error variance per group of the share probe under `plan`
            self.set_plan(plan)
            f = self._encode_probe(sh_tiles)
            e2 = (f - sh_ref_f).pow(2).sum(dim=1).div_(f.shape[1])
            return [float(e2[idx].mean()) for _, idx in sh_members]

        try:
            self.set_precision("strict", strict_blocks)
            ref_f = self._encode_probe(tiles)
            ref = self.similarity(ref_f, bank)                              # cosines on the engine's exact-fp32 similarity kernel
            self.set_precision("comp", strict_blocks)
            if not bool(torch.isfinite(ref).all()):
                self._raise_flags(2)
            if budget == "ladder":
                candidates = ladder_candidates(depth)
            else:
                sel, sh_members = share_probe(members)
                sh_tiles, sh_ref_f = tiles[sel], ref_f[sel]
                shares = measure_shares(iso_var, depth, sh_members)
                rms_target = tolerance / (max_sigmas_quantile(population, confidence) * PROBE_RMS_MARGIN)
                candidates = walk_candidates(greedy_walk(shares, depth, knobs or DEFAULT_KNOBS), rms_target)
            chosen, stats, tried = search(candidates, verify, tolerance)
            if chosen is None:
                self.set_precision("strict", strict_blocks)
            self.check_errors(wait=True)
            done = True
        finally:
            self.auto_calibrate = was
            if not done:                 # an exception mid-way: put back exactly what the caller had
                self._options, self._plan = saved_opts, saved_plan
                if self._handle.value:
                    try:
                        self._apply_options()
                    except Exception:
                        pass
        unit, n_margins = 0.0, 0.0
        if chosen:
            unit, n_margins = label_margin_unit(stats.governing.sigmas, population, label_population, confidence)
            self.set_option("label_margin", math.sqrt(2.0) * unit)
            self._label_margin_unit = unit
        self.calibration = calibration_report(
            chosen=chosen, stats=stats, tried=tried, shares=shares, budget=budget, population=population, confidence=confidence, tolerance=tolerance,
            strict_blocks=strict_blocks, probe_tiles=int(tiles.shape[0]), prompts=int(bank.shape[0]), probe_name=probe_name,
            group_names=[name for name, _ in members], label_unit=unit, label_population=n_margins,
            bias_correction=bool(lib.keep_get_option(h, b"bias_ready") > 0 and lib.keep_get_option(h, b"bias_correction") > 0))
        return self.calibration

    def _encode_probe(self, x: torch.Tensor) -> torch.Tensor:
        """``encode_image`` in chunks of 256 tiles (the probes of ``calibrate``)."""
        return torch.cat([self.encode_image(x[i:i + 256]) for i in range(0, x.shape[0], 256)]) if x.shape[0] > 256 else self.encode_image(x)

    def get_option(self, name: str) -> float:
        self._ready_device()
        return float(_lib.load().keep_get_option(self._handle, name.encode()))

    def reserve(self, tiles: int = 0, prompts: int = 0, seq: int = 256):
        self._ready()
        _lib.check(self._handle, _lib.load().keep_reserve(self._handle, tiles, prompts, seq), "reserve")
        return self

    def _ready(self):
        self.check_errors(wait=False)
        if not self._loaded:
            if self._host_sd is not None:
                self.to("cuda")            # reference scripts call .to(device) themselves; be lenient
            else:
                raise _lib.KeepHipError("no weights loaded: call load_state_dict / from_pretrained first")

    # ------------------------------------------------------------------ the hot path
    def _check_hw(self, H: int, W: int, layout: str):
        """The tile-size rule: 224 x 224, or with dynamic_img_size any positive multiple of 16 in both directions."""
        if self.dynamic_img_size:
            if H < 16 or W < 16 or H % 16 or W % 16:
                raise ValueError(f"dynamic_img_size: H and W must be positive multiples of 16 (the patch size), got {layout} with "
                                 f"H={H}, W={W}")
        elif H != 224 or W != 224:
            raise ValueError(f"only 224x224 tiles are supported, got {layout} (KEEPModel(..., dynamic_img_size=True) accepts any "
                             "multiple of 16, as the reference's timm dynamic_img_size does)")

    @torch.no_grad()
    def encode_image(self, image_inputs: torch.Tensor) -> torch.Tensor:
        """keep_inference.py:54-58: normalize(visual_head(visual(x)), dim=-1) -> [B, 768] fp32.
        x: [B,3,224,224]; with ``dynamic_img_size`` [B,3,H,W], H and W multiples of 16."""
        self._ready()
        x = image_inputs
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"expected [B,3,H,W], got {tuple(x.shape)}")
        self._check_hw(int(x.shape[2]), int(x.shape[3]), f"[B,3,H,W] = {tuple(x.shape)}")
        if x.dtype not in _PIX:
            x = x.to(torch.float32)
        src_dev = x.device
        if x.shape[0] == 0:
            return torch.empty((0, self.config.projection_dim), dtype=torch.float32, device=src_dev)
        xd = x.to(self._device, non_blocking=True).contiguous()
        out = torch.empty((xd.shape[0], self.config.projection_dim), dtype=torch.float32, device=self._device)
        _lib.check(self._handle, self._encode(xd, _PIX[xd.dtype], xd.shape[2], xd.shape[3], out), "encode_image")
        self._queue_flag_check(_stream(self._device))
        if src_dev == self._device:
            return out
        res = out.to(src_dev)
        self.check_errors(wait=True)
        return res

    def _encode(self, xd: torch.Tensor, pix: int, H: int, W: int, out: torch.Tensor) -> int:
        lib = _lib.load()
        if H == 224 and W == 224:          # the entry point every 224 x 224 call has always taken
            return lib.keep_encode_image(self._handle, _ptr(xd), pix, xd.shape[0], _ptr(out), _stream(self._device))
        return lib.keep_encode_image_hw(self._handle, _ptr(xd), pix, xd.shape[0], H, W, _ptr(out), _stream(self._device))

    def _encode_tapped(self, xd: torch.Tensor, pix: int, H: int, W: int, block: int, what: str) -> Tuple[torch.Tensor, torch.Tensor]:
        """keep_encode_image_attn on device tiles -> (features [B,768], attn [B, heads, T]) on the device."""
        self._check_block(block)
        B, heads, T = int(xd.shape[0]), self.config.vision.num_heads, (H // 16) * (W // 16) + 1
        out = torch.empty((B, self.config.projection_dim), dtype=torch.float32, device=self._device)
        attn = torch.empty((B, heads, T), dtype=torch.float32, device=self._device)
        rc = _lib.load().keep_encode_image_attn(self._handle, _ptr(xd), pix, B, H, W, block, _ptr(out), _ptr(attn), _stream(self._device))
        _lib.check(self._handle, rc, what)
        self._queue_flag_check(_stream(self._device))
        return out, attn

    @torch.no_grad()
    def encode_image_attention(self, image_inputs: torch.Tensor, block: int = -1) -> Tuple[torch.Tensor, torch.Tensor]:
        """:meth:`encode_image` with the CLS query's attention of one block beside it -> (features [B,768],
        attn fp32 [B, heads, T]), T = H/16 * W/16 + 1.  ``attn[b, h]`` is the softmax over the keys of ``q_{b,h,0} . k_{b,h,k} / 8`` in
        block ``block`` (``0 .. depth - 1``, negative from the end; ValueError outside): column 0 is CLS -> CLS, columns 1.. the patch
        tokens in row-major (y, x) order, each row sums to 1.  ``keep_amd.attention.cls_attention_map`` turns it into the per-tile map
        that is usually shown, ``keep_amd.wsi.attention_heatmap`` puts it on the slide raster.  Inputs and device handling as
        :meth:`encode_image`.  The features equal :meth:`encode_image`'s with option ``graphs`` = 0 bit for bit: a tapped call is never
        replayed as a graph, so small batches cost their launches."""
        self._ready()
        x = image_inputs
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"expected [B,3,H,W], got {tuple(x.shape)}")
        H, W = int(x.shape[2]), int(x.shape[3])
        self._check_hw(H, W, f"[B,3,H,W] = {tuple(x.shape)}")
        if x.dtype not in _PIX:
            x = x.to(torch.float32)
        src_dev = x.device
        if x.shape[0] == 0:
            self._check_block(block)
            return (torch.empty((0, self.config.projection_dim), dtype=torch.float32, device=src_dev),
                    torch.empty((0, self.config.vision.num_heads, (H // 16) * (W // 16) + 1), dtype=torch.float32, device=src_dev))
        xd = x.to(self._device, non_blocking=True).contiguous()
        out, attn = self._encode_tapped(xd, _PIX[xd.dtype], H, W, block, "encode_image_attention")
        if src_dev == self._device:
            return out, attn
        res = out.to(src_dev), attn.to(src_dev)
        self.check_errors(wait=True)
        return res

    def _check_rollout(self, start_block, residual, T: int):
        """The rules keep_encode_image_rollout applies, as a ValueError before any device work (and for calls without tiles)."""
        from .attention import ROLLOUT_MAX_TOKENS
        depth = int(_lib.load().keep_vit_depth(self._handle))
        if isinstance(start_block, bool) or not isinstance(start_block, int) or not -depth <= start_block < depth:
            raise ValueError(f"start_block {start_block!r} outside [-{depth}, {depth})")
        if isinstance(residual, bool) or not isinstance(residual, (int, float)) or not 0 <= residual < 1:      # (nan fails both comparisons)
            raise ValueError(f"residual {residual!r} outside [0, 1)")
        if T > ROLLOUT_MAX_TOKENS:
            raise ValueError(f"{T} tokens per tile: the attention rollout covers at most {ROLLOUT_MAX_TOKENS}")

    def _encode_rollout(self, xd: torch.Tensor, pix: int, H: int, W: int, start_block: int, residual: float, what: str) -> Tuple[torch.Tensor, torch.Tensor]:
        """keep_encode_image_rollout on device tiles -> (features [B,768], rollout [B, 1, T]) on the device; the scratch lives for this call."""
        B, T = int(xd.shape[0]), (H // 16) * (W // 16) + 1
        self._check_rollout(start_block, residual, T)
        lib = _lib.load()
        need = C.c_int64(0)
        _lib.check(self._handle, lib.keep_rollout_scratch_bytes(self._handle, B, H, W, C.byref(need)), what)
        scratch = torch.empty(max(int(need.value), 1), dtype=torch.uint8, device=self._device)      # dropped on return; the allocator reuses it in stream order
        out = torch.empty((B, self.config.projection_dim), dtype=torch.float32, device=self._device)
        roll = torch.empty((B, 1, T), dtype=torch.float32, device=self._device)
        rc = lib.keep_encode_image_rollout(self._handle, _ptr(xd), pix, B, H, W, start_block, float(residual), _ptr(out), _ptr(roll), _ptr(scratch),
                                           scratch.numel(), _stream(self._device))
        _lib.check(self._handle, rc, what)
        self._queue_flag_check(_stream(self._device))
        return out, roll

    @torch.no_grad()
    def encode_image_rollout(self, image_inputs: torch.Tensor, start_block: int = 0, residual: float = 0.5) -> Tuple[torch.Tensor, torch.Tensor]:
        """:meth:`encode_image` with the tile's attention rollout beside it (Abnar & Zuidema 2020) -> (features
        [B,768], rollout fp32 [B, 1, T]), T = H/16 * W/16 + 1.  With ``A_l`` the head mean of block l's softmax(q k^T / 8) over all T query
        rows and ``At_l = (1 - residual) A_l + residual I``, ``rollout[b, 0]`` is row 0 (the CLS query) of ``At_{depth-1} ... At_{start_block}``:
        it sums to 1, column 0 is CLS -> CLS, columns 1.. the patch tokens in row-major (y, x) order.  ``start_block``: ``0 .. depth - 1`` or
        negative from the end; ``0 <= residual < 1`` (ValueError outside; also for more than
        ``keep_amd.attention.ROLLOUT_MAX_TOKENS`` tokens per tile).  The singleton axis is the head axis of a one-head attention tensor:
        ``cls_attention_map``, ``wsi.attention_heatmap`` and ``cell_raster`` take the result as they take
        :meth:`encode_image_attention`'s.  Inputs and device handling as :meth:`encode_image`; the features equal its with option
        ``graphs`` = 0 bit for bit (the call is never replayed as a graph)."""
        self._ready()
        x = image_inputs
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"expected [B,3,H,W], got {tuple(x.shape)}")
        H, W = int(x.shape[2]), int(x.shape[3])
        self._check_hw(H, W, f"[B,3,H,W] = {tuple(x.shape)}")
        if x.dtype not in _PIX:
            x = x.to(torch.float32)
        src_dev = x.device
        T = (H // 16) * (W // 16) + 1
        if x.shape[0] == 0:
            self._check_rollout(start_block, residual, T)
            return (torch.empty((0, self.config.projection_dim), dtype=torch.float32, device=src_dev),
                    torch.empty((0, 1, T), dtype=torch.float32, device=src_dev))
        xd = x.to(self._device, non_blocking=True).contiguous()
        out, roll = self._encode_rollout(xd, _PIX[xd.dtype], H, W, start_block, residual, "encode_image_rollout")
        if src_dev == self._device:
            return out, roll
        res = out.to(src_dev), roll.to(src_dev)
        self.check_errors(wait=True)
        return res

    def _check_block(self, block) -> int:
        """The rule keep_encode_image_attn applies, as a ValueError before any device work (and for calls without tiles)."""
        depth = int(_lib.load().keep_vit_depth(self._handle))
        if isinstance(block, bool) or not isinstance(block, int) or not -depth <= block < depth:
            raise ValueError(f"block {block!r} outside [-{depth}, {depth})")
        return block % depth

    @torch.no_grad()
    def encode_image_uint8(self, tiles_u8: torch.Tensor) -> torch.Tensor:
        """Raw RGB tiles, uint8 [B,224,224,3] (HWC, after the resize + centre crop of the reference transform):
        ToTensor and Normalize (keep_inference.py:91-92) are fused into the first kernel, so the host only ships
        150 KB per tile.  Same result as ``encode_image(normalised_float_tiles)`` up to fp32 rounding."""
        self._ready()
        x = tiles_u8
        if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
            raise ValueError(f"expected uint8 [B,H,W,3], got {x.dtype} {tuple(x.shape)}")
        self._check_hw(int(x.shape[1]), int(x.shape[2]), f"uint8 [B,H,W,3] = {tuple(x.shape)}")
        src_dev = x.device
        if x.shape[0] == 0:
            return torch.empty((0, self.config.projection_dim), dtype=torch.float32, device=src_dev)
        xd = x.to(self._device, non_blocking=True).contiguous()
        out = torch.empty((xd.shape[0], self.config.projection_dim), dtype=torch.float32, device=self._device)
        _lib.check(self._handle, self._encode(xd, _lib.PIX_U8_HWC, xd.shape[1], xd.shape[2], out), "encode_image_uint8")
        self._queue_flag_check(_stream(self._device))
        if src_dev == self._device:
            return out
        res = out.to(src_dev)                  # host inputs: the copy back synchronises anyway, so the check is free and immediate
        self.check_errors(wait=True)
        return res

    @torch.no_grad()
    def resize_crop_uint8(self, images_u8: torch.Tensor, size: int = 224) -> torch.Tensor:
        """Raw RGB images, uint8 [B,H,W,3] of ONE size -> uint8 [B,size,size,3]: the reference transform's
        ``Resize(size, BICUBIC)`` + ``CenterCrop((size, size))`` (keep_inference.py:88-90) on the device, bit-identical to the
        PIL code path torchvision runs.  Feed the result to :meth:`encode_image_uint8`."""
        from .preprocess import pil_bicubic_coeffs, resize_output_size
        self._ready_device()
        x = images_u8
        if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
            raise ValueError(f"expected uint8 [B,H,W,3], got {x.dtype} {tuple(x.shape)}")
        B, H, W, _ = x.shape
        ow, oh = resize_output_size(W, H, size)
        if ow < size or oh < size:
            raise ValueError(f"resized image {ow}x{oh} is smaller than the {size}-pixel crop (torchvision would zero-pad: not supported on the device)")
        key = (W, H, size)
        if getattr(self, "_resize_cache", None) is None:
            self._resize_cache = {}
        if key not in self._resize_cache:             # float64 table construction as in libImaging; a few ms, once per image size
            xb, xk, xks = pil_bicubic_coeffs(W, ow)
            yb, yk, yks = pil_bicubic_coeffs(H, oh)
            dev = lambda a: torch.from_numpy(a).to(self._device).contiguous()
            self._resize_cache[key] = (dev(xb), dev(xk), xks, dev(yb), dev(yk), yks)
        xb, xk, xks, yb, yk, yks = self._resize_cache[key]
        left, top = int(round((ow - size) / 2.0)), int(round((oh - size) / 2.0))
        src_dev = x.device
        xd = x.to(self._device, non_blocking=True).contiguous()
        out = torch.empty((B, size, size, 3), dtype=torch.uint8, device=self._device)
        self._call("resize_crop_u8", _ptr(xd), B, H, W, _ptr(xb), _ptr(xk), xks, ow, _ptr(yb), _ptr(yk), yks, oh, left, top, size, _ptr(out))
        return out if src_dev == self._device else out.to(src_dev)

    @torch.no_grad()
    def encode_image_raw(self, images_u8: torch.Tensor) -> torch.Tensor:
        """uint8 [B,H,W,3] raw tiles of any (common) size -> [B,768]: the whole reference transform + ``encode_image`` on the
        device (resize + crop bit-identical to PIL, /255 and mean/std fused into the first encoder kernel)."""
        self._ready()
        dev_in = images_u8.device
        out = self.encode_image_uint8(self.resize_crop_uint8(images_u8.to(self._device)))
        return out if dev_in == self._device else out.to(dev_in)

    @torch.no_grad()
    def encode_text(self, text_inputs: Mapping[str, torch.Tensor]) -> torch.Tensor:
        """keep_inference.py:60-62: normalize(text(**inputs).pooler_output, dim=-1) -> [P, 768] fp32."""
        self._ready()
        ids = text_inputs["input_ids"]
        if ids.dim() != 2:
            raise ValueError(f"input_ids must be [P,T], got {tuple(ids.shape)}")
        src_dev = ids.device
        if ids.shape[0] == 0:
            return torch.empty((0, self.config.text.hidden_size), dtype=torch.float32, device=src_dev)

        def prep(name):
            t = text_inputs.get(name) if hasattr(text_inputs, "get") else (text_inputs[name] if name in text_inputs else None)
            if t is None:
                return None
            if tuple(t.shape) != tuple(ids.shape):
                raise ValueError(f"{name} shape {tuple(t.shape)} != input_ids shape {tuple(ids.shape)}")
            return t.to(self._device, torch.int64, non_blocking=True).contiguous()

        ids_d = ids.to(self._device, torch.int64, non_blocking=True).contiguous()
        typ_d, msk_d = prep("token_type_ids"), prep("attention_mask")
        P, T = ids_d.shape
        self.last_text_length = T
        if self.trim_padding and msk_d is not None and T > 16:
            # Columns that are padding in EVERY row change nothing (their softmax weight is exactly 0, positions are
            # absolute, the pooler reads token 0): run the tower at the longest valid length, rounded up to 16.
            # A row with no valid token attends uniformly over all T keys in HF, so such a batch is left alone.
            # The length is taken from the caller's mask where it lives: a host mask (the tokenizer's output) costs no device sync.
            src_mask = text_inputs.get("attention_mask") if hasattr(text_inputs, "get") else text_inputs["attention_mask"]
            valid = (src_mask if src_mask.device.type == "cpu" else msk_d) != 0
            col = torch.nonzero(valid.any(dim=0)).flatten()
            info = torch.stack([col[-1] + 1 if col.numel() else torch.zeros((), dtype=torch.int64, device=valid.device),
                                (~valid.any(dim=1)).any().to(torch.int64)]).tolist()
            L = min(T, max(16, -(-info[0] // 16) * 16))
            if info[1] == 0 and L < T:
                ids_d, msk_d = ids_d[:, :L].contiguous(), msk_d[:, :L].contiguous()
                typ_d = typ_d[:, :L].contiguous() if typ_d is not None else None
                T = self.last_text_length = L
        out = torch.empty((P, self.config.text.hidden_size), dtype=torch.float32, device=self._device)
        self._call("encode_text", _ptr(ids_d), _ptr(typ_d), _ptr(msk_d), P, T, _ptr(out))
        self._queue_flag_check(_stream(self._device))
        if src_dev == self._device:
            return out
        res = out.to(src_dev)                  # host inputs: the copy back synchronises anyway, so the check is free and immediate
        self.check_errors(wait=True)
        return res

    def _queue_flag_check(self, st):
        """After an encode call: look at the handle's sticky error bits (out-of-range token ids, non-finite features) -- immediately
        (``check_token_ids=True``), not at all (False), or lazily: an asynchronous copy of the bits + an event, examined by the next
        engine call / ``check_errors()`` (no host synchronisation per call)."""
        lib = _lib.load()
        if self.check_token_ids == "lazy":
            if len(self._pending_token_checks) >= 64:                  # bound the queue: wait for the oldest copies
                self.check_errors(wait=True)
            flag = self._flag_pool.pop() if self._flag_pool else torch.zeros(1, dtype=torch.int32).pin_memory()
            _lib.check(self._handle, lib.keep_token_error_async(self._handle, _ptr(flag), st), "token_error_async")
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self._device))
            self._pending_token_checks.append((flag, ev))
        elif self.check_token_ids:
            self._raise_flags(self._error_bits(st))

    def _error_bits(self, st) -> int:
        """keep_token_error: the sticky error bits (>= 0, cleared by the call) or a negative error code -- a HIP failure must not be read as bits."""
        rc = int(_lib.load().keep_token_error(self._handle, st))
        if rc < 0:
            _lib.check(self._handle, rc, "token_error")
        return rc

    @staticmethod
    def _raise_flags(bits: int, earlier: bool = False):
        when = " of an earlier call" if earlier else ""
        if bits & 1:
            raise IndexError(f"index out of range in self (input_ids / token_type_ids{when} were outside the embedding tables)")
        if bits & 4:
            raise _lib.KeepHipError(f"tissue_mask / mask_regions{when}: a component-labelling loop ran into its iteration cap (the mask is not valid)")
        if bits & 2:
            raise FloatingPointError(f"non-finite output features{when}: an activation exceeded the fp16 range (65504) of the engine's qkv / "
                                     "MLP-hidden stores; these weights need the fp32 reference path")

    def check_errors(self, wait: bool = True):
        """Raise the error of an earlier encode call (lazy checking): IndexError for out-of-range token ids, FloatingPointError for
        non-finite features.  Called by every engine entry point with ``wait=False`` (only looks at copies that have already landed).
        The device-side bits are sticky and every call's copy is queued, so an error is reported by the first check after it --
        never dropped."""
        pend = self._pending_token_checks
        if not pend:
            return
        if wait:
            pend[-1][1].synchronize()
        bits = 0
        while pend and pend[0][1].query():
            flag, _ = pend.pop(0)
            bits |= int(flag.item())
            self._flag_pool.append(flag)
        if bits:
            # acknowledge (clears the sticky bits); copies still in flight were taken before the clear and would repeat the report
            bits |= self._error_bits(_stream(self._device))
            for flag, ev in pend:
                ev.synchronize()
                self._flag_pool.append(flag)
            pend.clear()
            self._raise_flags(bits, earlier=True)

    def forward(self, image_inputs, text_inputs):
        """keep_inference.py:65-73."""
        return {"vision_features": self.encode_image(image_inputs),
                "text_features": self.encode_text(text_inputs)}

    __call__ = forward

    # ------------------------------------------------------------------ similarity
    @torch.no_grad()
    def similarity(self, image_features: torch.Tensor, text_features: torch.Tensor, scale: float = 1.0,
                   mode: str = "raw"):
        """Tile x prompt similarity on the GPU.

        mode 'raw'     -> scale * I @ T^T                       [N,P] fp32   (keep_inference.py:104)
             'argmax'  -> (sim [N,P], labels [N] int32)
             'softmax' -> softmax(scale * I @ T^T, dim=1)       [N,P] fp32   (subtyping_utils.py:72, scale=10)
             'softmax_f16' -> same in fp16
             'top2score'   -> python float, rank_cls_score of I @ T^T (WSI_evaluation/utils.py:107-117)
        """
        self._ready_device()
        img = image_features.to(self._device, torch.float32).contiguous()
        txt = text_features.to(self._device, torch.float32).contiguous()
        if img.dim() != 2 or txt.dim() != 2 or img.shape[1] != txt.shape[1]:
            raise ValueError(f"feature shapes {tuple(img.shape)} x {tuple(txt.shape)}")
        N, D = img.shape
        P = txt.shape[0]
        code = {"raw": _lib.SIM_RAW, "argmax": _lib.SIM_ARGMAX, "softmax": _lib.SIM_SOFTMAX,
                "softmax_f16": _lib.SIM_SOFTMAX_F16, "top2score": _lib.SIM_TOP2SCORE}[mode]
        amax = None
        if mode == "top2score":
            out = torch.empty((1,), dtype=torch.float32, device=self._device)
        elif mode == "softmax_f16":
            out = torch.empty((N, P), dtype=torch.float16, device=self._device)
        else:
            out = torch.empty((N, P), dtype=torch.float32, device=self._device)
        if mode == "argmax":
            amax = torch.empty((N,), dtype=torch.int32, device=self._device)
        self._call("similarity", _ptr(img), _ptr(txt), N, P, D, float(scale), code, _ptr(out), _ptr(amax))
        if mode == "argmax":
            return out, amax
        if mode == "top2score":
            return float(out.item())
        return out

    @torch.no_grad()
    def classify(self, image_inputs: torch.Tensor, text_features: torch.Tensor, scale: float = 1.0, margin: Optional[float] = None,
                 return_features: bool = False):
        """Tiles -> (similarity [B,P] fp32, labels [B] int32[, features [B,768]]): ``encode_image`` + ``img @ txt.T`` + row argmax
        (keep_inference.py:101-104) with labels that are the fp32 reference's.  Every tile is encoded in the model's precision; the
        tiles whose two best prompts are closer than ``margin`` in cosine are encoded a second time with split products (``strict``) and
        take their row from that.  Default margin: what ``calibrate()`` measured -- the worst error one tile's cosine DIFFERENCE can carry at the
        calibration's confidence = (per-unit figure ``calibration["label_margin_per_unit_prompt_distance"]``) x the largest distance |t_i - t_j|
        between two prompts of ``text_features`` (at most 2; sqrt 2 for banks without negative cosines, which is what the engine's own
        ``label_margin`` option assumes for C-ABI callers); an uncalibrated handle starts at 2.5e-4 = twice the 1e-4 tolerance + 25 %.
        ``self.last_rechecked`` holds how many tiles that was.  ``text_features``: ``encode_text`` output ([P,768], unit norm)."""
        self._ready()
        x = image_inputs
        u8 = x.dtype == torch.uint8
        if u8:
            if x.dim() != 4 or tuple(x.shape[1:]) != (224, 224, 3):
                raise ValueError(f"uint8 tiles must be [B,224,224,3] (HWC), got {tuple(x.shape)}")
        else:
            if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != 224 or x.shape[3] != 224:
                raise ValueError(f"expected [B,3,224,224], got {tuple(x.shape)}")
            if x.dtype not in _PIX:
                x = x.to(torch.float32)
        src_dev = x.device
        txt = text_features.to(self._device, torch.float32).contiguous()
        D = self.config.projection_dim
        if txt.dim() != 2 or txt.shape[1] != D:
            raise ValueError(f"text_features must be [P,{D}], got {tuple(txt.shape)}")
        B, P = x.shape[0], txt.shape[0]
        if margin is None and self._label_margin_unit:
            margin = self._label_margin_unit * self._bank_diameter(txt)
        self.last_margin = float(margin) if margin is not None else (self.get_option("label_margin") if self._handle.value else None)
        sim = torch.empty((B, P), dtype=torch.float32, device=self._device)
        lab = torch.empty((B,), dtype=torch.int32, device=self._device)
        feats = torch.empty((B, D), dtype=torch.float32, device=self._device) if return_features else None
        n = C.c_int64(0)
        if B:
            xd = x.to(self._device, non_blocking=True).contiguous()
            self._call("classify", _ptr(xd), _lib.PIX_U8_HWC if u8 else _PIX[xd.dtype], B, _ptr(txt), P, float(scale),
                       -1.0 if margin is None else float(margin), _ptr(feats), _ptr(sim), _ptr(lab), C.byref(n))
            self._queue_flag_check(_stream(self._device))
        self.last_rechecked = int(n.value)
        out = (sim, lab) + ((feats,) if return_features else ())
        if src_dev == self._device:
            return out
        out = tuple(t.to(src_dev) for t in out)
        self.check_errors(wait=True)
        return out

    def _bank_diameter(self, txt: torch.Tensor) -> float:
        """max |t_i - t_j| over the rows of a prompt bank (unit rows: sqrt(2 - 2 min cos)), on the engine's own similarity kernel; cached for the
        last bank.  Banks too large for a P x P matrix (or a single prompt) take the bound 2."""
        P = int(txt.shape[0])
        if P < 2 or P > 8192:
            return 2.0
        key = (txt.data_ptr(), P, txt._version)
        if getattr(self, "_bank_diam_key", None) != key:
            cos_min = float(self.similarity(txt, txt).min())
            self._bank_diam_key, self._bank_diam = key, math.sqrt(max(2.0 - 2.0 * cos_min, 0.0))
        return max(self._bank_diam, 1e-3)

    def _ready_device(self):
        self.check_errors(wait=False)
        if not self._handle.value:
            self._create(torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0))

    def clock_probe(self, out: torch.Tensor, spin_us: int = 300, stream: Optional["torch.cuda.Stream"] = None) -> None:
        """Enqueue a shader-clock sample on ``stream`` (default: current) into ``out`` (device int64[2], allocated -- and its allocation
        synchronised -- BEFORE the work the probe runs beside was queued: a fresh tensor handed to a side stream can be a recycled block
        that kernels still pending on the allocating stream write to).  out = {shader cycles, 100 MHz ticks}; MHz = 100 * cycles / ticks."""
        self._ready_device()
        if out.dtype != torch.int64 or out.numel() < 2 or out.device != self._device or not out.is_contiguous():
            raise ValueError("clock_probe needs a contiguous int64[2] on the engine's device")
        st = C.c_void_p(stream.cuda_stream) if stream is not None else _stream(self._device)
        _lib.check(self._handle, _lib.load().keep_clock_probe(self._handle, int(spin_us), _ptr(out), st), "clock_probe")

    def mfma_ceiling(self, operands: Optional[torch.Tensor] = None, iters: int = 100_000, reps: int = 3) -> float:
        """TFLOP/s the matrix pipes alone sustain on this GPU with ``operands`` (fp16 values; default seeded N(0, 1)) and no memory traffic
        (``keep_mfma_probe``): the ceiling the socket's power cap leaves for high-entropy fp16 MFMA work -- context for roofline fractions that
        are quoted against the nominal 2.4 GHz peak."""
        self._ready_device()
        dev = self._device
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        n = cus * 512 * 48
        if operands is None:
            g = torch.Generator(device=dev).manual_seed(7)
            operands = torch.randn(n, device=dev, generator=g, dtype=torch.float32).to(torch.float16)
        src = operands.to(dev, torch.float16).contiguous().flatten()
        if src.numel() < n:
            src = src.repeat(-(-n // src.numel()))[:n].contiguous()
        sink = torch.empty(cus * 512, dtype=torch.float32, device=dev)
        fl = C.c_double(0)
        best = 0.0
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(torch.cuda.current_stream(dev))
            self._call("mfma_probe", _ptr(src), _ptr(sink), int(iters), C.byref(fl))
            b.record(torch.cuda.current_stream(dev))
            b.synchronize()
            best = max(best, fl.value / (a.elapsed_time(b) * 1e-3) / 1e12)
        return best

    # ------------------------------------------------------------------ profiling passthrough
    def profile_enable(self, tag: Optional[str] = None):
        self._ready_device()
        arg = None if tag is None else tag.encode()
        _lib.check(self._handle, _lib.load().keep_profile_enable(self._handle, arg), "profile_enable")

    def profile_disable(self):
        self.profile_enable("")

    def profile_reset(self):
        _lib.check(self._handle, _lib.load().keep_profile_reset(self._handle), "profile_reset")

    def profile_read(self, tag: str):
        ms, n, fl = C.c_double(0), C.c_int64(0), C.c_double(0)
        _lib.check(self._handle, _lib.load().keep_profile_read(self._handle, tag.encode(), C.byref(ms), C.byref(n), C.byref(fl)), tag)
        return ms.value, n.value, fl.value


_bare_engines: Dict[int, "KEEPModel"] = {}


def engine_for(device=None, model=None) -> "KEEPModel":
    """The engine the model-free slide-level functions run on: ``model`` if given (a KEEPModel or the reference's ``KEEP_model``
    dict), else the most recently created live engine on ``device`` (default: the current GPU), else a weight-less handle on
    that device (similarity / screening / refine kernels need no weights)."""
    if model is not None:
        m = model["model"] if isinstance(model, Mapping) else model
        if not isinstance(m, KEEPModel):
            raise TypeError("expected a keep_amd.KEEPModel (or the reference's KEEP_model dict holding one)")
        m._ready_device()
        return m
    if not torch.cuda.is_available():
        raise _lib.KeepHipError("no GPU visible: keep_amd has no CPU execution path")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        dev = torch.device("cuda", torch.cuda.current_device())      # features on the host: computed on the current GPU, returned to the host
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    for r in reversed(KEEPModel._live):
        m = r()
        if m is not None and m._handle.value and m._device is not None and m._device.index == idx:
            return m
    m = KEEPModel()
    m._create(torch.device("cuda", idx))
    _bare_engines[idx] = m                    # keeps the weight-less handle alive (the registry only holds weak references)
    return m


PROFILE_TAGS = ("vit.im2col", "vit.patch", "vit.ln", "vit.qkv", "vit.attn", "vit.proj", "vit.fc1", "vit.fc2",
                "vit.head", "text.embed", "text.ln", "text.qkv", "text.attn", "text.out", "text.ffn1", "text.ffn2",
                "text.pool", "sim",
                # launches with extra passes (split / compensated products of the blocks the precision setting names) and the CLS-rows-only
                # operators of the last block are timed apart, so that the plain tags hold ONE kernel instantiation each
                "vit.qkv.x", "vit.attn.x", "vit.proj.x", "vit.fc1.x", "vit.fc2.x", "vit.tail")
