"""GPU versions of the reference's slide-level zero-shot logic.

Every public function has the NAME, POSITIONAL ARGUMENTS, DEFAULTS and RETURN VALUE of its counterpart in
``WSI_evaluation/utils.py``, ``subtyping_utils.py``, ``detection_utils.py`` and ``segment_utils.py`` (cited per function), so
the call sites of the three ``zeroshot_*_WSI.py`` scripts run unchanged (``keep_amd/wsi_evaluation/`` re-exports them under the
reference's module names).  The per-classifier / per-tile Python loops of the reference (one GEMM + ``.item()`` sync per prompt
set, one ``.cpu()`` per tile) become a handful of kernel launches through the C ABI (``keep_similarity``, ``keep_prompt_scores``,
``keep_refine``).

The reference's functions are plain torch code and take no model; here the kernels belong to an engine handle, which is found
from the device (``keep_amd.model.engine_for``: the live ``KEEPModel`` on that GPU, or a weight-less handle).  An optional
keyword ``model=`` pins it (a ``KEEPModel`` or the reference's ``KEEP_model`` dict).
"""
from __future__ import annotations

import weakref
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .model import KEEPModel, _ptr, _stream, engine_for


# ------------------------------------------------------------------------------------------------
# classifier construction (utils.py:64-104) with a prompt-string cache
# ------------------------------------------------------------------------------------------------
class TextEmbeddingCache:
    """The RCC prompt bank asks for 7128 ``encode_text`` calls but holds only 264 distinct strings
    (SURVEY.md §3.2): embed each distinct string once, in batches.  A cache that belongs to an engine (``_cache_for``) refers to it
    weakly, so that it never keeps the model -- and its GPU weights -- alive."""

    def __init__(self, KEEP_model: Mapping, device, batch: int = 64, max_length: int = 256, weak: bool = False):
        model = KEEP_model["model"]
        self._model = weakref.ref(model) if weak else (lambda: model)
        self.tokenizer = KEEP_model["tokenizer"]
        self.device, self.batch, self.max_length = device, batch, max_length
        self._cache: Dict[str, torch.Tensor] = {}

    @property
    def model(self):
        m = self._model()
        if m is None:
            raise ReferenceError("the model this prompt cache was built for no longer exists")
        return m

    def embed(self, texts: Sequence[str]) -> torch.Tensor:
        todo = [t for t in dict.fromkeys(texts) if t not in self._cache]
        for i in range(0, len(todo), self.batch):
            chunk = todo[i:i + self.batch]
            # same tokenizer call as utils.py:73
            enc = self.tokenizer(chunk, max_length=self.max_length, padding="max_length", truncation=True, return_tensors="pt")
            enc = enc.to(self.device) if hasattr(enc, "to") else {k: v.to(self.device) for k, v in enc.items()}
            emb = self.model.encode_text(enc)
            for t, e in zip(chunk, emb):
                self._cache[t] = e
        return torch.stack([self._cache[t] for t in texts])


# one cache per (model, tokenizer, weights, precision setting): the reference scripts call get_zeroshot_classifier once per prompt set with
# the same KEEP_model dict (zeroshot_subtyping_WSI.py:59-62), so repeated strings are embedded once without any change to the call site.
# The cache lives ON the model object (and refers back to it weakly): it goes away with the model, and nothing global pins a model.
PROMPT_CACHE = True          # False: embed every string on every call, exactly as the reference does
TEXT_OPTIONS = ("precision", "strict_blocks")      # the engine options encode_text depends on


def _cache_for(KEEP_model, device) -> TextEmbeddingCache:
    m, tok = KEEP_model["model"], KEEP_model["tokenizer"]
    if not PROMPT_CACHE or not isinstance(m, KEEPModel):
        return TextEmbeddingCache(KEEP_model, device)
    # embeddings depend on the weights and on the precision setting of the TEXT tower (precision, strict_blocks): set_precision after the first
    # call must not return embeddings computed under the old setting.  Image-only options (the per-block plan, lanes, kernel selection) do not
    # touch the text tower and leave the cache alone.
    key = (id(tok), getattr(m, "_weights_epoch", 0), str(device), tuple((k, float(m._options.get(k, 0))) for k in TEXT_OPTIONS))
    slot = getattr(m, "_prompt_cache", None)
    if slot is None or slot[0] != key:
        slot = (key, TextEmbeddingCache(KEEP_model, device, weak=True))
        m._prompt_cache = slot
    return slot[1]


def _unit_rows(m: KEEPModel, x: torch.Tensor) -> torch.Tensor:
    """Rows of a 2-D tensor divided by max(||row||, 1e-12) on the engine (``F.normalize(x, dim=-1)`` semantics; keep_op_l2norm) --
    torch holds the storage, the arithmetic is the engine's fp32 row kernel; the result comes back in the dtype and on the device of ``x``
    (the reference's ``F.normalize`` keeps both).  There is deliberately no torch fallback: with a text encoder that is not a ``KEEPModel``
    the normalisation still runs on the engine of the device (a weight-less handle: these kernels need no weights), and without a GPU the
    call raises like every other entry point of this package."""
    dev, dt = x.device, x.dtype
    r = x.detach().to(m._device, torch.float32).contiguous().clone()
    if r.numel():
        _lib.check(m._handle, _lib.load().keep_op_l2norm(m._handle, _ptr(r), r.shape[0], r.shape[1], _stream(m._device)), "l2norm")
    if dt.is_floating_point and dt != torch.float32:
        r = r.to(dt)
    return r if dev == m._device else r.to(dev)


def zero_shot_classifier(KEEP_model, classnames, templates, device, cache: Optional[TextEmbeddingCache] = None):
    """utils.py:64-84.  Returns [feat_dim, num_classes]."""
    cache = cache or _cache_for(KEEP_model, device)
    eng = _engine(KEEP_model["model"] if isinstance(KEEP_model["model"], KEEPModel) else None, device=device)
    weights = []
    with torch.no_grad():
        for classname in classnames:
            if isinstance(templates, list):
                texts = [t.replace("CLASSNAME", classname) for t in templates]
            else:
                texts = [templates.replace("CLASSNAME", classname)]
            # the reference keeps only row 0 of the batch (`encode_text(text_inputs)[0]`, utils.py:74)
            class_embeddings = cache.embed(texts)[0].unsqueeze(0)
            # F.normalize(class_embeddings, dim=-1).mean(dim=0) over ONE row, then / norm (utils.py:76-80): two passes of the row kernel
            class_embedding = _unit_rows(eng, _unit_rows(eng, class_embeddings))[0]
            weights.append(class_embedding)
    return torch.stack(weights, dim=1).to(device)


def get_zeroshot_classifier(model, label_map, prompts, device, add_normal=False, cache: Optional[TextEmbeddingCache] = None):
    """utils.py:86-104 (``model`` is the reference's ``KEEP_model`` dict: {'model', 'tokenizer', ...})."""
    classnames, templates = prompts["classnames"], prompts["templates"]
    idx_to_class = {v: k for k, v in label_map.items()}
    n_classes = len(idx_to_class)
    if add_normal:
        idx_to_class[n_classes] = "Normal"
        n_classes = len(idx_to_class)
    classnames_text = [classnames[idx_to_class[idx]] for idx in range(n_classes)]
    return zero_shot_classifier(model, classnames_text, templates, device, cache)


def build_classifier_bank(KEEP_model, label_map, prompts, device, add_normal=False,
                          cache: Optional[TextEmbeddingCache] = None) -> List[torch.Tensor]:
    """All prompt classifiers of a prompt file at once: the loop the three scripts run over ``prompts[str(i)]``
    (zeroshot_subtyping_WSI.py:59-63 -> ``get_zeroshot_classifier`` per prompt set) with every distinct string embedded
    once and the per-class normalise -> mean -> renormalise (utils.py:76-80) done for all K x C columns in three tensor
    ops instead of K x C x 4 tiny launches.  ``prompts``: the parsed prompt JSON ({"0": {"classnames", "templates"}, ...})
    or a list of such entries.  Returns K tensors [feat_dim, C] (views of one [K, feat_dim, C] tensor)."""
    cache = cache or _cache_for(KEEP_model, device)
    entries = [prompts[str(i)] for i in range(len(prompts))] if isinstance(prompts, Mapping) else list(prompts)
    idx_to_class = {v: k for k, v in label_map.items()}
    if add_normal:
        idx_to_class[len(idx_to_class)] = "Normal"
    C_ = len(idx_to_class)
    texts = []
    for e in entries:
        tpl = e["templates"][0] if isinstance(e["templates"], list) else e["templates"]     # row 0 only, as utils.py:74
        texts.extend(tpl.replace("CLASSNAME", e["classnames"][idx_to_class[c]]) for c in range(C_))
    eng = _engine(KEEP_model["model"] if isinstance(KEEP_model["model"], KEEPModel) else None, device=device)
    emb = cache.embed(texts).to(device, torch.float32)                                      # [K*C, D]
    emb = _unit_rows(eng, emb)                                 # normalize(class_embeddings, dim=-1).mean(dim=0) over ONE row
    emb = _unit_rows(eng, emb)                                 # class_embedding /= class_embedding.norm()
    bank = emb.reshape(len(entries), C_, -1).permute(0, 2, 1).contiguous()                  # [K, D, C]
    return list(bank.unbind(0))


# ------------------------------------------------------------------------------------------------
def _engine(model=None, *tensors, device=None) -> KEEPModel:
    """The engine of a call: ``model`` if pinned, else the one that lives on the device of ``device`` / the first GPU tensor."""
    if model is not None:
        return engine_for(model=model)
    if device is None:
        for t in tensors:
            if isinstance(t, torch.Tensor) and t.device.type == "cuda":
                device = t.device
                break
    return engine_for(device=device)


def _normalized(m: KEEPModel, feats: torch.Tensor) -> torch.Tensor:
    f = feats.to(m._device, torch.float32)
    if f.dim() == 3:
        f = f.squeeze(0)
    f = f.contiguous().clone()
    _lib.check(m._handle, _lib.load().keep_op_l2norm(m._handle, _ptr(f), f.shape[0], f.shape[1], _stream(m._device)), "l2norm")
    return f


def rank_cls_score(logits: torch.Tensor, model=None) -> float:
    """utils.py:107-117 on a ready [N,C] logits matrix -> Python float."""
    m = _engine(model, logits)
    x = logits.to(m._device, torch.float32).contiguous()
    eye = torch.eye(x.shape[1], device=m._device)
    # scores of ONE classifier whose logits are given: run the group kernel with K = 1 on logits @ I
    return float(prompt_scores(x, [eye], pre_normalized=True, model=m, _logits_given=True)[0])


def prompt_scores(tile_features: torch.Tensor, classifiers: Sequence[torch.Tensor], pre_normalized: bool = False, model=None,
                  _logits_given: bool = False) -> torch.Tensor:
    """rank_cls_score of every classifier in one pass (the loop at utils.py:127-130) -> fp32 [K] on the engine's device."""
    m = _engine(model, tile_features, *classifiers[:1])
    K, (D, Cc) = len(classifiers), classifiers[0].shape
    bank = torch.stack([c.to(m._device, torch.float32).t() for c in classifiers]).reshape(K * Cc, D).contiguous()
    f = tile_features.to(m._device, torch.float32).contiguous() if pre_normalized else _normalized(m, tile_features)
    if _logits_given:       # f already holds logits [N, C]; bank is the identity: reuse the same kernels
        D = f.shape[1]
        if D % 16:
            pad = 16 - D % 16
            f = torch.nn.functional.pad(f, (0, pad)).contiguous()
            bank = torch.nn.functional.pad(bank, (0, pad)).contiguous()
            D += pad
    scores = torch.empty(K, dtype=torch.float32, device=m._device)
    rc = _lib.load().keep_prompt_scores(m._handle, _ptr(f), _ptr(bank), f.shape[0], K, Cc, D, _ptr(scores), _stream(m._device))
    _lib.check(m._handle, rc, "prompt_scores")
    return scores


def zero_shot_prompt_select(classifiers, tile_features, topn, device, model=None):
    """utils.py:119-146: score every prompt classifier on the slide, keep the top-n, sum and renormalise -> [feat_dim, C] on
    the device of the classifiers (``torch.zeros_like(classifiers[0])``, utils.py:141)."""
    m = _engine(model, device=device)
    scores = prompt_scores(tile_features, classifiers, model=m)
    # same tie behaviour as the reference: torch.sort(descending=True) on a CPU tensor of Python floats (utils.py:139)
    _, index = torch.sort(torch.tensor(scores.cpu().tolist()), descending=True)
    merge = torch.zeros_like(classifiers[0], dtype=torch.float32)
    for cls_index in index[0:topn]:
        merge += classifiers[int(cls_index)].to(merge.device, torch.float32)
    return _unit_rows(m, merge.t()).t().contiguous()            # F.normalize(merge, p=2, dim=0): the columns are the class vectors


def random_prompt_ensemble(classifiers: Sequence[torch.Tensor], topn: int, model=None) -> torch.Tensor:
    """The `prompt_screening = False` branch of the three scripts (zeroshot_subtyping_WSI.py:68-76): `topn` picks with
    `random.seed(c); random.randint(0, K-1)` for c = 0..topn-1 (so the picks are the same on every run), summed and
    column-normalised."""
    import random
    ensemble_cls = torch.zeros_like(classifiers[-1])
    for cter in range(topn):
        random.seed(cter)
        ensemble_cls += classifiers[random.randint(0, len(classifiers) - 1)]
    return _unit_rows(_engine(model, ensemble_cls), ensemble_cls.t()).t().contiguous()


def cood2str(cood):
    """utils.py:148-149."""
    return str(cood[0]) + "_" + str(cood[1])


def str2cood(str):                      # noqa: A002 -- the reference's parameter name (utils.py:150)
    """utils.py:150-151."""
    return [int(item) for item in str.split("_")]


def accuracy(logits, target, topk=(1,)):
    """utils.py:153-156."""
    pred = logits.topk(max(topk), 1, True, True)[1].t()
    correct = pred.eq(target.view(1, -1).expand_as(pred))
    return [float(correct[:k].reshape(-1).float().sum(0, keepdim=True).cpu().numpy()) for k in topk]


# ------------------------------------------------------------------------------------------------
def _probs(m: KEEPModel, classifier: torch.Tensor, tile_features: torch.Tensor) -> torch.Tensor:
    """softmax(10 * normalize(feat) @ classifier, dim=1) -- subtyping_utils.py:69-72."""
    f = _normalized(m, tile_features)
    return m.similarity(f, classifier.t().contiguous(), scale=10.0, mode="softmax")


def refine(probs: torch.Tensor, tile_coords, patch_size: int, overlap: bool, model=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Core of the three ``refine_seg`` variants.  Returns (coords [U,2], mean probs [U,C], index [U]) for the
    U distinct coordinates in first-seen order (the key order of the reference's dicts)."""
    m = _engine(model, probs)
    p = probs.to(m._device, torch.float32).contiguous()
    coords = torch.as_tensor(np.asarray(tile_coords)).to(torch.int64)
    lim = 2 ** 31 - 1 - abs(int(patch_size))
    if coords.numel() and (int(coords.min()) < -lim or int(coords.max()) > lim):
        raise ValueError("tile coordinates must fit int32 (the device-side coordinate hash packs (x, y) into 64 bits)")
    coords = coords.to(m._device).contiguous()
    N, Cc = p.shape
    out = torch.empty_like(p)
    first = torch.empty(N, dtype=torch.int32, device=m._device)
    rc = _lib.load().keep_refine(m._handle, _ptr(p), _ptr(coords), N, Cc, int(patch_size), int(bool(overlap)), _ptr(out), _ptr(first),
                                 _stream(m._device))
    _lib.check(m._handle, rc, "refine")
    idx = torch.nonzero(first, as_tuple=False).squeeze(1)
    return coords[idx], out[idx], idx


def _keys(coords: torch.Tensor) -> List[str]:
    return [f"{x}_{y}" for x, y in coords.cpu().tolist()]


def refine_seg_subtyping(logits_slide, coords_slide, patch_size=224, overlap=True, model=None) -> Dict[str, int]:
    """``refine_seg`` of subtyping_utils.py:38-65: {"x_y": predicted class} in first-seen order."""
    coords, mean, _ = refine(logits_slide, coords_slide, patch_size, overlap, model=model)
    return dict(zip(_keys(coords), mean.argmax(dim=1).cpu().tolist()))


def zero_shot_subtyping(classifier, tile_features, tile_coords, patch_size=256, overlap=True, model=None):
    """subtyping_utils.py:67-83 -> slide label (0-d int64 tensor, the reference's ``max_label``)."""
    m = _engine(model, tile_features, classifier)
    _, mean, _ = refine(_probs(m, classifier, tile_features), tile_coords, patch_size, overlap, model=m)
    pred = mean.argmax(dim=1)
    C_ = classifier.shape[1]
    # (preds == ix).sum() / len(preds) in float64, as the numpy expression at subtyping_utils.py:80
    frac = [float((pred == ix).sum().item()) / pred.shape[0] for ix in range(C_)]
    _, max_label = torch.tensor(frac[0:-1]).max(0)
    return max_label


def refine_seg_detection(logits_slide, coords_slide, patch_size=224, threshold=0.5, overlap=True, model=None):
    """``refine_seg`` of detection_utils.py:39-74: ({"x_y": 0/1}, {"x_y": tumour probability})."""
    coords, mean, _ = refine(logits_slide, coords_slide, patch_size, overlap, model=model)
    keys, p1 = _keys(coords), mean[:, 1]
    return dict(zip(keys, (p1 > threshold).to(torch.int64).cpu().tolist())), dict(zip(keys, p1.cpu().tolist()))


def zero_shot_detection(classifier, tile_features, tile_coords, patch_size=256, overlap=False, model=None):
    """detection_utils.py:88-100 -> tumour-tile ratio (float)."""
    m = _engine(model, tile_features, classifier)
    _, mean, _ = refine(_probs(m, classifier, tile_features), tile_coords, patch_size, overlap, model=m)
    return float((mean[:, 1] > 0.5).sum().item()) / mean.shape[0]


def refine_seg_segment(logits_slide, coords_slide, patch_size=224, overlap=True, model=None) -> Dict[str, float]:
    """``refine_seg`` of segment_utils.py:63-89: {"x_y": tumour probability} in first-seen order."""
    coords, mean, _ = refine(logits_slide, coords_slide, patch_size, overlap, model=model)
    return dict(zip(_keys(coords), mean[:, 1].cpu().tolist()))


def zero_shot_segment_probs(classifier, tile_features, tile_coords, patch_size=224, overlap=True, model=None) -> Dict[str, float]:
    """segment_utils.py:44-52 + refine_seg :63-89: the dense per-tile tumour-probability map of ``zero_shot_segment``."""
    m = _engine(model, tile_features, classifier)
    return refine_seg_segment(_probs(m, classifier, tile_features), tile_coords, patch_size, overlap, model=m)


def zero_shot_segment(classifier, tile_features, tile_coords, mask_path, patch_size=224, overlap=True, model=None):
    """segment_utils.py:44-60.  ``mask_path=None`` returns the probability map.  With an annotation -- a ``PolygonSet``, a pair
    ``(PolygonSet, order)``, a ``TissueMask``, or a path ending in ``.xml`` (ASAP) / ``.geojson`` / ``.json`` -- it goes on as the
    reference does: ``(auc, dice)`` from :func:`eval_seg_auc` and :func:`eval_seg_coarse` at the best threshold of the ROC
    (DESIGN.md section 17).  Any other path (a slide file: the mask pyramid of the reference needs openslide) is not read."""
    from .evaluation import resolve_annotation
    probs_all_refined = zero_shot_segment_probs(classifier, tile_features, tile_coords, patch_size, overlap, model=model)
    if mask_path is None:
        return probs_all_refined
    truth = resolve_annotation(mask_path)
    if truth is None:
        raise NotImplementedError("AUC / Dice against an openslide mask (segment_utils.py:91-152) is outside the hot path; "
                                  "call with mask_path=None and feed the returned map to the reference's eval_seg_auc / eval_seg_coarse")
    m = _engine(model, tile_features, classifier)
    auc, best_thd = eval_seg_auc(probs_all_refined, truth, patch_size=patch_size, model=m)
    dice = eval_seg_coarse(probs_all_refined, truth, patch_size=patch_size, thd=best_thd, model=m)
    return auc, dice


# ------------------------------------------------------------------------------------------------ evaluation
def _tile_probs(probs) -> Tuple[torch.Tensor, torch.Tensor]:
    """``{"x_y": p}`` or a ``(coords, p)`` pair, host or device -> (coords int64 [N,2], p [N]) as torch tensors where they were."""
    if isinstance(probs, Mapping):
        return (torch.tensor([str2cood(k) for k in probs], dtype=torch.int64).reshape(-1, 2),
                torch.tensor(list(probs.values()), dtype=torch.float64))
    coords, p = probs
    coords = torch.as_tensor(np.asarray(coords)) if not isinstance(coords, torch.Tensor) else coords
    p = torch.as_tensor(np.asarray(p)) if not isinstance(p, torch.Tensor) else p
    return coords.reshape(-1, 2), p.reshape(-1)


def _annotation(mask_path):
    """-> (PolygonSet | TissueMask, order), already resolved pairs pass through."""
    from .annotation import PolygonSet
    from .evaluation import resolve_annotation
    from .region import TissueMask
    if isinstance(mask_path, tuple) and len(mask_path) == 2 and isinstance(mask_path[0], (PolygonSet, TissueMask)) and \
            not isinstance(mask_path[1], (PolygonSet, TissueMask)):
        return mask_path
    truth = resolve_annotation(mask_path)
    if truth is None:
        raise NotImplementedError(f"mask_path {mask_path!r}: a PolygonSet, (PolygonSet, order), a TissueMask, or a path ending in .xml / "
                                  ".geojson / .json (a mask pyramid needs openslide, which this package does not read)")
    return truth


def eval_seg_auc(probs_all_refined, mask_path, patch_size=224, save_path='./', model=None, rule="union", max_band_bytes=1 << 28):
    """segment_utils.py:91-119 on the device -> ``(auc, best_threshold)`` as Python floats: a label per tile from the ground truth
    (``KEEPModel.annotation_tile_labels``: more than half of the tile's level-0 pixels set), the tile-level AUROC and
    ``thresholds[np.argmax(tpr - fpr)]`` (``KEEPModel.tile_roc``).  ``probs_all_refined``: the dict of
    ``zero_shot_segment(mask_path=None)`` or a ``(coords, p)`` pair, host or device (the scores are taken as float32, which the
    dict's values are).  ``mask_path``: see :func:`zero_shot_segment`.  ``save_path`` is unused, as in the reference."""
    truth, order = _annotation(mask_path)
    coords, p = _tile_probs(probs_all_refined)
    m = _engine(model, p, coords)
    labels = m.annotation_tile_labels(truth, coords, patch_size, order=order, rule=rule, max_band_bytes=max_band_bytes)
    roc = m.tile_roc(p.to(torch.float32), labels, curve=False)
    return roc.auc, roc.best_threshold


def bootstrap_seg_auc(probs_all_refined, mask_path, patch_size=224, save_path='./', model=None, rule="union", max_band_bytes=1 << 28,
                      n_boot=1000, seed=0):
    """:func:`eval_seg_auc`'s tile-level AUROC with its bootstrap replicates ->
    ``keep_amd.bootstrap.BootstrapResult``: ``estimate`` is the ``auc`` ``eval_seg_auc`` returns, ``ci()`` its percentile interval over
    ``n_boot`` resamples of the slide's tiles (``KEEPModel.bootstrap_roc``).  The first arguments are ``eval_seg_auc``'s."""
    truth, order = _annotation(mask_path)
    coords, p = _tile_probs(probs_all_refined)
    m = _engine(model, p, coords)
    labels = m.annotation_tile_labels(truth, coords, patch_size, order=order, rule=rule, max_band_bytes=max_band_bytes)
    return m.bootstrap_roc(p.to(torch.float32), labels, n_boot, seed)[1]


def _truth_mask16(m: KEEPModel, truth, order, shape, rule: str, d: int = 16) -> torch.Tensor:
    from .region import TissueMask
    if isinstance(truth, TissueMask):
        if truth.downsample != d or tuple(truth.mask.shape) != tuple(shape):
            raise ValueError(f"the truth mask has downsample {truth.downsample} and shape {tuple(truth.mask.shape)}, the evaluation runs at "
                             f"{d} and {tuple(shape)}")
        return truth.mask
    return m.annotation_mask(truth, d, shape, order=order, rule=rule).mask


def eval_seg_coarse(probs_all_refined, mask_path, patch_size=224, thd=0.5, model=None, shape=None, rule="union"):
    """segment_utils.py:122-152 on the device -> Dice (``2 both / (truth + pred)`` in Python integers; 1 when both masks are empty).
    At downsample 16, the reference's level: the prediction is :func:`segment_pred_mask` (255 where a tile with ``p > thd`` covers the
    pixel), the truth is the annotation filled at pixel centres (``KEEPModel.annotation_mask``; no parity with a pyramid file's own
    down-sampling is claimed) or a ``TissueMask`` of downsample 16.  ``shape``: the masks' ``(h, w)``; by default the smallest that
    covers every tile and every vertex, or the ``TissueMask``'s own."""
    from .evaluation import default_eval_shape
    from .region import TissueMask
    truth, order = _annotation(mask_path)
    coords, p = _tile_probs(probs_all_refined)
    m = _engine(model, p, coords)
    if shape is None:
        shape = tuple(truth.mask.shape) if isinstance(truth, TissueMask) else default_eval_shape(coords, truth, patch_size, 16)
    pred = segment_pred_mask((coords, p), thd, 16, shape, patch_size, model=m)
    return m.mask_overlap(_truth_mask16(m, truth, order, shape, rule), pred).dice


def segment_evaluate(classifier, tile_features, tile_coords, annotation, patch_size=224, overlap=True, shape=None, sweep=False, rule="union",
                     model=None):
    """:func:`zero_shot_segment` with an annotation, without the dict and with the whole results: ``(RocResult, MaskOverlap)`` of the
    tile ROC and of the level-16 masks at its best threshold, and with ``sweep=True`` a third, the ``RasterSweep`` of the
    refined probabilities' raster (what :func:`segment_heatmap` makes at downsample 16) against the same truth mask."""
    from .evaluation import default_eval_shape
    from .region import TissueMask
    truth, order = _annotation(annotation)
    m = _engine(model, tile_features, classifier)
    if isinstance(tile_coords, torch.Tensor):
        tile_coords = tile_coords.cpu()                             # refine checks the coordinate range on the host
    coords, mean, _ = refine(_probs(m, classifier, tile_features), tile_coords, patch_size, overlap, model=m)
    p = mean[:, 1].contiguous()
    roc = m.tile_roc(p, m.annotation_tile_labels(truth, coords, patch_size, order=order, rule=rule))
    if shape is None:
        shape = tuple(truth.mask.shape) if isinstance(truth, TissueMask) else default_eval_shape(coords, truth, patch_size, 16)
    mask16 = _truth_mask16(m, truth, order, shape, rule)
    ov = m.mask_overlap(mask16, segment_pred_mask((coords, p), roc.best_threshold, 16, shape, patch_size, model=m))
    if not sweep:
        return roc, ov
    return roc, ov, m.raster_sweep(m.tile_raster(coords, p, patch_size, 16, shape), mask16)


# ------------------------------------------------------------------------------------------------ lesion-level scoring
def segment_lesions(raster, radius, min_score=0.5, tissue=None, max_peaks=1 << 20, model=None):
    """The detections a segmentation raster proposes: the local maxima of its mean within ``radius`` raster pixels that reach
    ``min_score`` (``KEEPModel.raster_peaks``) -> ``keep_amd.lesion.LesionCandidates`` with level-0 coordinates.  ``raster``: the
    ``TileRaster`` of :func:`segment_heatmap`; ``tissue``: a ``TissueMask`` of its geometry, optional."""
    from .heatmap import TileRaster
    if not isinstance(raster, TileRaster):
        raise ValueError(f"raster must be a TileRaster, got {type(raster).__name__}")
    return _engine(model, raster.acc).raster_peaks(raster, radius, min_score, tissue, max_peaks)


def eval_seg_froc(slides, margin_px=None, radius=None, min_score=0.5, downsample=None, shape=None, rule="union", ignore_max_extent=None,
                  model=None, ignore_major_axis=None):
    """Lesion-level FROC over slides, the score of a CAMELYON16-style challenge -> ``keep_amd.lesion.FrocCurve`` (``.score``: the mean
    sensitivity at 1/4 ... 8 false positives per slide).  ``slides``: an iterable of ``(raster or candidates, annotation)``: a
    ``TileRaster`` (its peaks are taken with ``radius`` / ``min_score``, see :func:`segment_lesions`) or a ``LesionCandidates``; the
    annotation in the forms :func:`zero_shot_segment` takes.  A ``PolygonSet`` is filled in the raster's geometry (origin 0), or at
    ``downsample`` / ``shape`` beside candidates.  Per slide: ``KEEPModel.evaluation_mask`` (``margin_px`` in mask pixels, default
    ``keep_amd.lesion.camelyon16_margin()``: 75 um at downsample 32 of a 0.243 um slide), ``KEEPModel.lesion_hits``, then one
    ``FrocAccumulator``.  ``ignore_major_axis`` (``keep_amd.morphometry.camelyon16_itc_axis()``) sets the lesions aside whose major axis
    length is below it, the challenge's isolated-tumour-cell rule; ``ignore_max_extent`` is the bounding-box rule; not both.  Parity
    with the challenge's own script is not claimed (DESIGN.md sections 18 and 21)."""
    from .annotation import PolygonSet
    from .heatmap import TileRaster
    from .lesion import FrocAccumulator, LesionCandidates, camelyon16_margin
    margin_px = camelyon16_margin() if margin_px is None else margin_px
    froc, m = None, None
    for found, annotation in slides:
        truth, order = _annotation(annotation)
        if isinstance(found, TileRaster):
            if radius is None:
                raise ValueError("a raster needs radius=, the suppression radius of its peaks in raster pixels")
            m = _engine(model, found.acc)
            d, hw = found.downsample, found.shape
            found = m.raster_peaks(found, radius, min_score)
        elif isinstance(found, LesionCandidates):
            m = _engine(model, *(t for t in (found.xy, found.scores) if isinstance(t, torch.Tensor)))
            d, hw = downsample, shape
        else:
            raise ValueError(f"a slide is (TileRaster or LesionCandidates, annotation), got {type(found).__name__}")
        if isinstance(truth, PolygonSet):
            em = m.evaluation_mask(truth, margin_px, ignore_max_extent=ignore_max_extent, downsample=d, shape=hw, order=order, rule=rule,
                                   ignore_major_axis=ignore_major_axis)
        else:
            em = m.evaluation_mask(truth, margin_px, ignore_max_extent=ignore_max_extent, ignore_major_axis=ignore_major_axis)
        froc = FrocAccumulator(m) if froc is None else froc
        froc.add(m.lesion_hits(found, em))
    if froc is None:
        raise ValueError("no slides")
    return froc.curve()


# ------------------------------------------------------------------------------------------------ heatmap
def segment_heatmap(classifier, tile_features, tile_coords, downsample, shape, patch_size=224, overlap=True, cls=1, origin=(0, 0), model=None,
                    percentile=False, reference=None, blur_sigma=None, blur_radius=None, tissue=None):
    """The segmentation flow ending in slide geometry instead of a dict: ``_probs`` -> :func:`refine` -> ``KEEPModel.tile_raster`` on
    device tensors -> ``keep_amd.heatmap.TileRaster`` of class ``cls``'s refined probability (``.mean()`` is the probability map,
    ``KEEPModel.render_heatmap`` the picture).  No dict is built and the host is visited only where :func:`refine` already does.
    ``downsample`` / ``shape`` / ``origin``: the raster's geometry, that of the thumbnail and of ``KEEPModel.tissue_mask``.

    The display steps of CLAM's heatmaps, all off by default: ``percentile=True`` replaces the refined
    probabilities by their rank percentiles before rasterising, among the slide's own refined tiles or, with ``reference`` (a
    ``keep_amd.heatmap.ScoreReference``), against that population; ``blur_sigma`` (with ``blur_radius``, default ``ceil(3 sigma)``)
    smooths the raster with ``KEEPModel.smooth_raster``, under ``tissue`` (a ``TissueMask`` of the raster's geometry) if given."""
    from .heatmap import ScoreReference, check_raster_args, gaussian_taps
    from .region import TissueMask
    _, d, shape, _ = check_raster_args(patch_size, downsample, shape, origin)
    if reference is not None and not percentile:
        raise ValueError("reference= is what percentile=True ranks against: pass both")
    if reference is not None and not isinstance(reference, ScoreReference):
        raise ValueError(f"reference must be a ScoreReference, got {type(reference).__name__}")
    if blur_sigma is None and (blur_radius is not None or tissue is not None):
        raise ValueError("blur_radius= and tissue= belong to blur_sigma=: pass it too")
    taps = None if blur_sigma is None else gaussian_taps(blur_sigma, blur_radius)
    if tissue is not None:
        if not isinstance(tissue, TissueMask):
            raise ValueError(f"tissue must be a TissueMask, got {type(tissue).__name__}")
        if tissue.downsample != d or tuple(tissue.mask.shape) != shape:
            raise ValueError(f"tissue mask has downsample {tissue.downsample} and shape {tuple(tissue.mask.shape)}, the raster {d} and {shape}")
    m = _engine(model, tile_features, classifier)
    if isinstance(tile_coords, torch.Tensor):
        tile_coords = tile_coords.cpu()                             # refine checks the coordinate range on the host
    coords, mean, _ = refine(_probs(m, classifier, tile_features), tile_coords, patch_size, overlap, model=m)
    if not -mean.shape[1] <= int(cls) < mean.shape[1]:
        raise ValueError(f"cls {cls!r} outside the classifier's {mean.shape[1]} classes")
    values = mean[:, int(cls)].contiguous()
    if percentile:
        values = m.percentiles(values, reference)
    raster = m.tile_raster(coords, values, patch_size, downsample, shape, origin)
    return raster if taps is None else m.smooth_raster(raster, taps=taps, tissue=tissue)


def attention_heatmap(model, attn, coords, grid, patch_size, downsample, shape, heads=None, normalize="tile_max", origin=(0, 0), into=None):
    """The CLS attention of a slide's tiles in slide geometry -> ``keep_amd.heatmap.TileRaster``:
    ``keep_amd.attention.cls_attention_map(attn, heads, normalize)`` put on the raster by ``KEEPModel.cell_raster``.  ``attn`` [N, heads,
    gh gw + 1] and ``coords`` [N,2] as ``KEEPModel.encode_region_attention`` returns them, ``grid = (gh, gw)`` the token grid of a tile
    ((14, 14) at 224 x 224), ``patch_size`` a tile's footprint in the units of the coords; ``into=`` adds to an earlier raster."""
    from .attention import cls_attention_map
    m = _engine(model, attn)
    return m.cell_raster(coords, cls_attention_map(attn, heads, normalize), grid, patch_size, downsample, shape, origin, into)


def segment_regions(raster, thd=0.5, tissue=None, connectivity=8, min_area=1, model=None):
    """The lesion table of a segmentation raster: the connected regions of the pixels whose mean is above
    ``thd``, with area, box, centroid sums and mean / peak score -> ``keep_amd.components.RegionTable``.  ``raster``: the
    ``TileRaster`` of :func:`segment_heatmap`.  A pixel is set iff a tile covers it, ``sum > quantize(thd) * count`` (int64: the mean
    in 16-bit fixed point is above the threshold in the same fixed point) and ``tissue`` (a ``TissueMask`` of the raster's shape and
    downsample, optional) is set there."""
    from .heatmap import COUNT_SHIFT, MAX_TILES, SUM_MASK, TileRaster, quantize
    from .region import TissueMask
    if not isinstance(raster, TileRaster):
        raise ValueError(f"raster must be a TileRaster, got {type(raster).__name__}")
    if tissue is not None:
        if not isinstance(tissue, TissueMask):
            raise ValueError(f"tissue must be a TissueMask, got {type(tissue).__name__}")
        if tissue.downsample != raster.downsample or tuple(tissue.mask.shape) != raster.shape:
            raise ValueError(f"tissue mask has downsample {tissue.downsample} and shape {tuple(tissue.mask.shape)}, the raster "
                             f"{raster.downsample} and {raster.shape}")
    t16 = quantize(thd)
    S, c = raster.acc & SUM_MASK, (raster.acc >> COUNT_SHIFT) & MAX_TILES
    mask = (c > 0) & (S > t16 * c)
    if tissue is not None:
        mask &= tissue.mask.to(mask.device) != 0
    m = _engine(model, raster.acc)
    return m.mask_regions(mask, connectivity, min_area, raster=raster)


def segment_pred_mask(probs, thd, downsample, shape, patch_size=224, origin=(0, 0), model=None) -> torch.Tensor:
    """The ``pred_mask`` that ``eval_seg_coarse`` paints (segment_utils.py:134-140), at any integer ``downsample`` (the reference's
    level 16 is ``downsample=16``): uint8 {0,255} [h,w] on the device, 255 where any covering tile has ``p > thd``, overlapping tiles
    included.  ``probs``: the ``{"x_y": probability}`` dict of ``zero_shot_segment(mask_path=None)`` / ``refine_seg_segment``, or a
    ``(coords [N,2], p [N])`` pair (host or device).  The comparison is made in float32 (``float32(p) > float32(thd)``) on the values as
    given, before rasterising."""
    from .heatmap import check_raster_args
    check_raster_args(patch_size, downsample, shape, origin)
    if isinstance(probs, Mapping):
        coords = torch.tensor([str2cood(k) for k in probs], dtype=torch.int64).reshape(-1, 2)
        p = torch.tensor(list(probs.values()), dtype=torch.float64)
    else:
        coords, p = probs
        coords = torch.as_tensor(np.asarray(coords)) if not isinstance(coords, torch.Tensor) else coords
        p = torch.as_tensor(np.asarray(p)) if not isinstance(p, torch.Tensor) else p
    m = _engine(model, p, coords)
    above = (p.to(m._device).to(torch.float32) > torch.tensor(float(thd), dtype=torch.float32, device=m._device)).to(torch.float32)
    return m.tile_raster(coords, above, patch_size, downsample, shape, origin).pred()


# ------------------------------------------------------------------------------------------------ subtype map
def subtyping_map(classifier, tile_features, tile_coords, downsample, shape, patch_size=256, overlap=True, origin=(0, 0), vote=False,
                  classes=None, model=None):
    """The subtyping flow (subtyping_utils.py:67-83) ending in slide geometry instead of one label: ``_probs`` -> :func:`refine`, as
    :func:`zero_shot_subtyping` does, then ``KEEPModel.class_raster`` over the refined ``[U,C]`` probabilities ->
    ``keep_amd.classmap.ClassRaster`` (``KEEPModel.class_map`` makes the per-pixel call of it, ``render_class_map`` the picture).
    ``vote=True`` rasterises the tiles' argmax labels instead (one-hot rows): every pixel then counts the votes of its tiles, and on
    tiles that do not overlap the area shares of the label map are the tile shares of :func:`zero_shot_subtyping`.  ``classes``:
    optional names, one per column of the classifier.  ``downsample`` / ``shape`` / ``origin``: the raster's geometry."""
    from .classmap import check_class_names, check_classes
    from .heatmap import check_raster_args
    _, _, shape, _ = check_raster_args(patch_size, downsample, shape, origin)
    C_ = check_classes(classifier.shape[1], shape)
    classes = check_class_names(classes, C_)
    m = _engine(model, tile_features, classifier)
    if isinstance(tile_coords, torch.Tensor):
        tile_coords = tile_coords.cpu()                             # refine checks the coordinate range on the host
    coords, mean, _ = refine(_probs(m, classifier, tile_features), tile_coords, patch_size, overlap, model=m)
    if vote:
        return m.class_raster(coords, None, patch_size, downsample, shape, origin, labels=mean.argmax(dim=1), n_classes=C_, classes=classes)
    return m.class_raster(coords, mean, patch_size, downsample, shape, origin, classes=classes)


def cluster_map(tile_features, tile_coords, k_or_centroids, downsample, shape, patch_size=256, origin=(0, 0), model=None, **fit):
    """The unsupervised morphology map: the tiles' features clustered by cosine and the cluster labels rasterised
    as votes -> ``(keep_amd.classmap.ClassRaster, keep_amd.cluster.TileClusters)``.  ``k_or_centroids``: an integer k, which fits
    ``KEEPModel.cluster_tiles(tile_features, k, **fit)`` (``init`` / ``max_iter`` / ``tol_changed``), or fp32 centroids ``[K, D]`` (of an
    earlier fit), which only assigns.  Skipped tiles (a non-finite feature) are in no plane.  ``KEEPModel.class_map``,
    ``render_class_map`` and :func:`subtype_regions` take the raster from there."""
    from .cluster import TileClusters, check_centroids, check_features, check_k
    from .heatmap import check_raster_args
    check_raster_args(patch_size, downsample, shape, origin)
    f = tile_features.squeeze(0) if isinstance(tile_features, torch.Tensor) and tile_features.dim() == 3 else tile_features
    N, D = check_features(f)
    coords = tile_coords if isinstance(tile_coords, torch.Tensor) else torch.as_tensor(np.asarray(tile_coords))
    if tuple(coords.shape) != (N, 2):
        raise ValueError(f"tile_coords must be [{N}, 2] beside {N} feature rows, got shape {tuple(coords.shape)}")
    given = hasattr(k_or_centroids, "shape")
    K = check_centroids(k_or_centroids, D)[0] if given else check_k(k_or_centroids)
    if given and fit:
        raise ValueError(f"centroids are given: nothing is fitted, so {sorted(fit)} have no meaning")
    m = _engine(model, tile_features)
    if given:
        labels, best, margin, skipped = m.cluster_assign(f, k_or_centroids, normalize=True)
        counts = torch.bincount(labels[labels >= 0].to(torch.int64), minlength=K)
        kept = int(counts.sum())
        res = TileClusters(labels, best, margin, m._on_device(k_or_centroids), counts, int(skipped), counts == 0, 0, 0,
                           float(best.sum(dtype=torch.float64)) / kept if kept else 0.0, True)
    else:
        res = m.cluster_tiles(f, K, **fit)
    keep = res.labels >= 0
    raster = m.class_raster(coords.to(m._device)[keep], None, patch_size, downsample, shape, origin, labels=res.labels[keep], n_classes=K)
    return raster, res


def pca_map(tile_features, tile_coords, k_or_pca, downsample, shape, patch_size=256, origin=(0, 0), components=(0, 1, 2), scale="rank",
            model=None):
    """The PCA colour map of a slide: three principal components of the tiles' features as the three planes of a
    raster -> ``(keep_amd.classmap.ClassRaster, keep_amd.pca.FeaturePCA)``.  ``k_or_pca``: an integer k, which fits
    ``KEEPModel.pca_fit(tile_features, k)`` on the slide's own tiles, or a ``FeaturePCA`` (of an earlier fit), which only projects: two
    slides then share one colour space.  ``components``: the three components shown as red, green and blue.  ``scale``: ``"rank"`` maps
    every component to its percentile among the slide's tiles (``KEEPModel.percentiles``); a ``(lo, hi)`` pair of length-3 sequences clips
    linearly, ``(score - lo) / (hi - lo)`` into [0, 1].  Skipped tiles (a non-finite feature) are in no plane.
    ``KEEPModel.render_rgb_map`` paints the raster."""
    from .cluster import check_features
    from .heatmap import check_raster_args
    from .pca import FeaturePCA, check_k
    check_raster_args(patch_size, downsample, shape, origin)
    f = tile_features.squeeze(0) if isinstance(tile_features, torch.Tensor) and tile_features.dim() == 3 else tile_features
    N, D = check_features(f)
    coords = tile_coords if isinstance(tile_coords, torch.Tensor) else torch.as_tensor(np.asarray(tile_coords))
    if tuple(coords.shape) != (N, 2):
        raise ValueError(f"tile_coords must be [{N}, 2] beside {N} feature rows, got shape {tuple(coords.shape)}")
    given = isinstance(k_or_pca, FeaturePCA)
    K = k_or_pca.k if given else check_k(k_or_pca, D)
    comp = tuple(int(c) for c in components)
    if len(comp) != 3 or any(c < 0 or c >= K for c in comp):
        raise ValueError(f"components must be three component indices in 0..{K - 1}, got {components!r}")
    linear = None
    if not isinstance(scale, str):
        if len(scale) != 2 or len(scale[0]) != 3 or len(scale[1]) != 3:
            raise ValueError(f'scale must be "rank" or a (lo, hi) pair of length-3 sequences, got {scale!r}')
        linear = (np.asarray(scale[0], np.float32), np.asarray(scale[1], np.float32))
        if not bool((linear[1] > linear[0]).all()):
            raise ValueError(f"scale needs lo < hi for every component, got {scale!r}")
    elif scale != "rank":
        raise ValueError(f'scale must be "rank" or a (lo, hi) pair of length-3 sequences, got {scale!r}')
    m = _engine(model, tile_features)
    pca = k_or_pca if given else m.pca_fit(f, K)
    scores, kept = m.pca_transform(pca, f, K)
    nan = torch.full((), float("nan"), dtype=torch.float32, device=m._device)
    values = torch.empty((N, 3), dtype=torch.float32, device=m._device)
    for ch, c in enumerate(comp):
        s = torch.where(kept, scores[:, c], nan)                        # a skipped tile is no part of the population
        if linear is None:
            values[:, ch] = m.percentiles(s)
        else:
            lo, hi = float(linear[0][ch]), float(linear[1][ch])
            values[:, ch] = torch.where(kept, ((s - lo) / (hi - lo)).clamp(0.0, 1.0), nan)
    raster = m.class_raster(coords.to(m._device), values, patch_size, downsample, shape, origin, classes=[f"PC{c + 1}" for c in comp])
    return raster, pca


def tsne_map(tile_features, tile_coords, downsample, shape, patch_size=256, origin=(0, 0), model=None, **fit):
    """The t-SNE colour map of a slide: the geography of the tiles' 2-D embedding painted back onto the slide ->
    ``(keep_amd.classmap.ClassRaster, keep_amd.tsne.TileEmbedding)``.  ``KEEPModel.tsne_fit(tile_features, **fit)`` embeds the slide's own
    tiles; each embedding coordinate is ranked among them (``KEEPModel.percentiles``, as ``pca_map`` ranks a component) into planes 0 and
    1, and plane 2 is ``1 - (p0 + p1) / 2``: tiles that lie together in the embedding share a colour under ``KEEPModel.render_rgb_map``.
    Skipped tiles (a non-finite feature) are in no plane."""
    from .cluster import check_features
    from .heatmap import check_raster_args
    check_raster_args(patch_size, downsample, shape, origin)
    f = tile_features.squeeze(0) if isinstance(tile_features, torch.Tensor) and tile_features.dim() == 3 else tile_features
    N, _ = check_features(f)
    coords = tile_coords if isinstance(tile_coords, torch.Tensor) else torch.as_tensor(np.asarray(tile_coords))
    if tuple(coords.shape) != (N, 2):
        raise ValueError(f"tile_coords must be [{N}, 2] beside {N} feature rows, got shape {tuple(coords.shape)}")
    m = _engine(model, tile_features)
    emb = m.tsne_fit(f, **fit)
    p0, p1 = m.percentiles(emb.embedding[:, 0].contiguous()), m.percentiles(emb.embedding[:, 1].contiguous())   # a NaN stays NaN
    values = torch.stack([p0, p1, 1.0 - (p0 + p1) / 2.0], dim=1)
    raster = m.class_raster(coords.to(m._device), values, patch_size, downsample, shape, origin, classes=["tSNE1", "tSNE2", "rest"])
    return raster, emb


def tsne_scatter(embedding, labels, n_classes, size=(512, 512), point=3, model=None):
    """The scatter plot of an embedding on the device -> ``keep_amd.classmap.ClassRaster`` of ``size`` pixels with
    a ``point`` x ``point`` square per tile in its label's plane; ``KEEPModel.class_map`` and ``render_class_map(thumbnail=None)`` paint it.
    ``embedding``: a ``TileEmbedding`` or fp32 ``[N, 2]``; ``labels``: integers ``[N]`` in ``0 .. n_classes - 1`` (class, cluster or slide;
    -1 leaves a tile out).  Each column is scaled affinely from its minimum and maximum (one read-back) onto ``0 .. size - point``,
    column 0 along the width and column 1 down the height (``keep_amd.tsne.scatter_coords_numpy``); NaN rows are not drawn.  Pure
    composition: ``class_raster(coords, onehot, patch_size=point, downsample=1, shape=size)``."""
    from .classmap import check_classes
    from .heatmap import check_raster_args
    from .tsne import TileEmbedding, check_embedding
    y = embedding.embedding if isinstance(embedding, TileEmbedding) else embedding
    y = y if isinstance(y, torch.Tensor) else torch.as_tensor(np.asarray(y))
    N = check_embedding(y)
    C = check_classes(n_classes)
    point, _, (h, w), _ = check_raster_args(point, 1, size)
    if point > min(h, w):
        raise ValueError(f"a point of {point} pixels does not fit a canvas of {h}x{w}")
    lab = labels if isinstance(labels, torch.Tensor) else torch.as_tensor(np.asarray(labels))
    if tuple(lab.shape) != (N,) or lab.dtype.is_floating_point or lab.dtype == torch.bool:
        raise ValueError(f"labels must be integers [{N}], got {lab.dtype} {tuple(lab.shape)}")
    m = _engine(model, y)
    y, lab = y.to(m._device), lab.to(m._device, torch.int64)
    shown = ~torch.isnan(y).any(dim=1)
    coords = torch.zeros((N, 2), dtype=torch.int64, device=m._device)
    lo_hi = torch.stack([torch.where(shown[:, None], y, torch.full_like(y, float("inf"))).amin(dim=0),
                         torch.where(shown[:, None], y, torch.full_like(y, float("-inf"))).amax(dim=0),
                         torch.stack([lab.min(), lab.max()]).to(torch.float32)]).cpu().numpy()
    if lo_hi[2, 0] < -1 or lo_hi[2, 1] >= C:
        raise ValueError(f"labels must lie in -1 .. {C - 1}, got {int(lo_hi[2, 0])} .. {int(lo_hi[2, 1])}")
    if np.isfinite(lo_hi[:2]).all():
        for c, span in ((0, w - point), (1, h - point)):
            lo, hi = float(lo_hi[0, c]), float(lo_hi[1, c])
            scale = max(hi - lo, float(np.finfo(np.float32).tiny))
            v = torch.where(shown, y[:, c], torch.full_like(y[:, c], lo)).double()
            coords[:, c] = torch.floor((v - lo) / scale * float(span) + 0.5).to(torch.int64)
    onehot = torch.zeros((N, C), dtype=torch.float32, device=m._device)
    onehot.scatter_(1, lab.clamp(min=0).reshape(N, 1), 1.0)
    onehot[~(shown & (lab >= 0))] = float("nan")                        # class_raster leaves a row with a NaN out of every plane
    return m.class_raster(coords, onehot, point, 1, (h, w))


def probe_map(probe, tile_features, tile_coords, downsample, shape, patch_size=256, origin=(0, 0), vote=False, classes=None, model=None):
    """The supervised morphology map: a fitted linear probe's probabilities of every tile rasterised in slide
    geometry -> ``keep_amd.classmap.ClassRaster``.  ``probe``: a ``keep_amd.probe.LinearProbe`` (of ``KEEPModel.probe_fit``) or a
    ``(weight [C, D], bias [C])`` pair; ``vote=True`` rasterises the predicted labels as one-hot rows instead.  ``classes``: optional
    names, by default the probe's.  Skipped tiles (a non-finite feature) are in no plane.  ``KEEPModel.class_map``,
    ``render_class_map`` and :func:`subtype_regions` take the raster from there."""
    from .cluster import check_features
    from .heatmap import check_raster_args
    from .probe import LinearProbe
    check_raster_args(patch_size, downsample, shape, origin)
    f = tile_features.squeeze(0) if isinstance(tile_features, torch.Tensor) and tile_features.dim() == 3 else tile_features
    N, _ = check_features(f)
    coords = tile_coords if isinstance(tile_coords, torch.Tensor) else torch.as_tensor(np.asarray(tile_coords))
    if tuple(coords.shape) != (N, 2):
        raise ValueError(f"tile_coords must be [{N}, 2] beside {N} feature rows, got shape {tuple(coords.shape)}")
    if classes is None and isinstance(probe, LinearProbe):
        classes = probe.classes
    m = _engine(model, tile_features)
    labels, probs, _, _ = m.probe_predict(probe, f, normalize=True)
    keep = labels >= 0
    coords = coords.to(m._device)[keep]
    if vote:
        return m.class_raster(coords, None, patch_size, downsample, shape, origin, labels=labels[keep], n_classes=int(probs.shape[1]),
                              classes=classes)
    return m.class_raster(coords, probs[keep], patch_size, downsample, shape, origin, classes=classes)


def mil_attention_map(mil, tile_features, tile_coords, downsample, shape, patch_size=256, origin=(0, 0), model=None):
    """The learned attention of one slide as a heatmap: the slide's tiles are one bag, every tile's attention is
    divided by the bag's largest and rasterised by ``KEEPModel.tile_raster`` -> ``keep_amd.heatmap.TileRaster`` for ``render_heatmap``,
    ``smooth_raster`` and ``mask_regions``.  ``mil``: a ``keep_amd.mil.AttentionMIL`` (of ``KEEPModel.mil_fit``) or ``(V, bv, w, Wc, bc)``.
    Skipped tiles (a non-finite feature) are not rasterised."""
    from .cluster import check_features
    from .heatmap import check_raster_args
    check_raster_args(patch_size, downsample, shape, origin)
    f = tile_features.squeeze(0) if isinstance(tile_features, torch.Tensor) and tile_features.dim() == 3 else tile_features
    N, _ = check_features(f)
    coords = tile_coords if isinstance(tile_coords, torch.Tensor) else torch.as_tensor(np.asarray(tile_coords))
    if tuple(coords.shape) != (N, 2):
        raise ValueError(f"tile_coords must be [{N}, 2] beside {N} feature rows, got shape {tuple(coords.shape)}")
    m = _engine(model, tile_features)
    out = m.mil_forward(f, np.array([0, N], np.int64), mil)
    keep = out["scores"] > float("-inf")
    a = out["attention"][keep]
    if a.numel() == 0:
        raise ValueError("every tile of the slide is skipped: there is no attention to draw")
    return m.tile_raster(coords.to(m._device)[keep], a / a.max(), patch_size, downsample, shape, origin)


def knn_map(train_features, train_labels, n_classes, tile_features, tile_coords, downsample, shape, patch_size=256, origin=(0, 0), k=20,
            weights="softmax", temperature=0.07, vote=False, classes=None, model=None):
    """The example-based morphology map: every tile's ``k`` nearest labelled training tiles vote for its class
    (``KEEPModel.topk`` + ``knn_vote``) and the vote shares are rasterised in slide geometry -> ``keep_amd.classmap.ClassRaster``, as
    :func:`probe_map` builds one.  ``train_labels``: integers, -1 for a training tile to leave out of the bank; ``vote=True`` rasterises
    the predicted labels as one-hot rows instead.  Tiles without a label (a non-finite feature, or no voting neighbour) are in no
    plane.  ``KEEPModel.class_map``, ``render_class_map`` and :func:`subtype_regions` take the raster from there."""
    from .cluster import check_features
    from .heatmap import check_raster_args
    check_raster_args(patch_size, downsample, shape, origin)
    f = tile_features.squeeze(0) if isinstance(tile_features, torch.Tensor) and tile_features.dim() == 3 else tile_features
    N, _ = check_features(f)
    coords = tile_coords if isinstance(tile_coords, torch.Tensor) else torch.as_tensor(np.asarray(tile_coords))
    if tuple(coords.shape) != (N, 2):
        raise ValueError(f"tile_coords must be [{N}, 2] beside {N} feature rows, got shape {tuple(coords.shape)}")
    m = _engine(model, tile_features, train_features)
    m._ready_device()
    ty = m._probe_labels(train_labels, int(train_features.shape[0]))
    on = ty >= 0
    if not bool(on.any()):
        raise ValueError("no labelled training tile")
    nb = m.topk(f, m._on_device(train_features)[on].contiguous(), k)
    labels, probs, _, _ = m.knn_vote(nb, ty[on], n_classes, weights, temperature)
    keep = labels >= 0
    coords = coords.to(m._device)[keep]
    if vote:
        return m.class_raster(coords, None, patch_size, downsample, shape, origin, labels=labels[keep], n_classes=int(probs.shape[1]),
                              classes=classes)
    return m.class_raster(coords, probs[keep], patch_size, downsample, shape, origin, classes=classes)


def prototype_map(protos, feats, coords, downsample, shape, patch_size=256, origin=(0, 0), classes=None, model=None):
    """The few-shot morphology map: every tile's nearest class prototype (``KEEPModel.fewshot_predict`` with a
    one-episode ``keep_amd.fewshot.Prototypes``, say of ``KEEPModel.fewshot_fit``) rasterised as votes in slide geometry ->
    ``keep_amd.classmap.ClassRaster``, as :func:`knn_map` and :func:`cluster_map` build one.  Tiles without a label (a non-finite
    feature, or a tile equal to the support mean) are in no plane.  ``KEEPModel.class_map``, ``render_class_map`` and
    :func:`subtype_regions` take the raster from there."""
    from .cluster import check_features
    from .heatmap import check_raster_args
    check_raster_args(patch_size, downsample, shape, origin)
    f = feats.squeeze(0) if isinstance(feats, torch.Tensor) and feats.dim() == 3 else feats
    N, _ = check_features(f)
    xy = coords if isinstance(coords, torch.Tensor) else torch.as_tensor(np.asarray(coords))
    if tuple(xy.shape) != (N, 2):
        raise ValueError(f"coords must be [{N}, 2] beside {N} feature rows, got shape {tuple(xy.shape)}")
    m = _engine(model, feats, protos.bank)
    labels, scores, _, _ = m.fewshot_predict(protos, f)
    keep = labels >= 0
    return m.class_raster(xy.to(m._device)[keep], None, patch_size, downsample, shape, origin, labels=labels[keep], n_classes=int(scores.shape[1]),
                          classes=classes)


def prototype_slide_call(protos, feats, top=5, model=None):
    """The multiple-instance SimpleShot call of a slide -> ``(label, pooled fp32 [C])``: a slide's score for class
    c is the mean of its ``top`` largest tile scores ``s_c`` (``KEEPModel.fewshot_predict``; all kept tiles when the slide has fewer),
    the label the first maximum of the pooled scores; ``(-1, zeros)`` when no tile is kept.  The pooling is ``torch.topk`` on the ``[N,
    C]`` score matrix and a mean: plumbing on the device, not a kernel of this engine."""
    if isinstance(top, bool) or not isinstance(top, (int, np.integer)) or int(top) < 1:
        raise ValueError(f"top must be an integer >= 1, got {top!r}")
    f = feats.squeeze(0) if isinstance(feats, torch.Tensor) and feats.dim() == 3 else feats
    m = _engine(model, feats, protos.bank)
    labels, scores, _, _ = m.fewshot_predict(protos, f)
    s = scores[labels >= 0]
    if s.shape[0] == 0:
        return -1, torch.zeros(scores.shape[1], dtype=torch.float32, device=scores.device)
    pooled = torch.topk(s, min(int(top), int(s.shape[0])), dim=0).values.mean(0)
    return int(pooled.argmax()), pooled


def search_tiles(query_features, tile_features, k, tile_coords=None, exclude_self=False, model=None):
    """Tile search: the ``k`` tiles most like every query by cosine -> ``(index int64 [Q, k], score fp32 [Q, k],
    coords [Q, k, 2] or None)`` on the device, best first, of equal scores the lower tile first; -1 / 0 / (-1, -1) in an empty slot
    (fewer than ``k`` tiles, or a query with a non-finite feature).  ``query_features``: prompt embeddings or tile features ``[Q, D]``;
    ``tile_features`` ``[N, D]``: a slide's tiles; ``tile_coords`` ``[N, 2]``: gathered on the device into the third result.
    ``exclude_self=True`` (the queries are the tiles themselves): no tile finds itself."""
    qf = query_features.squeeze(0) if isinstance(query_features, torch.Tensor) and query_features.dim() == 3 else query_features
    tf = tile_features.squeeze(0) if isinstance(tile_features, torch.Tensor) and tile_features.dim() == 3 else tile_features
    m = _engine(model, tile_features, query_features)
    if tile_coords is not None:
        coords = tile_coords if isinstance(tile_coords, torch.Tensor) else torch.as_tensor(np.asarray(tile_coords))
        if tuple(coords.shape) != (int(tf.shape[0]), 2):
            raise ValueError(f"tile_coords must be [{int(tf.shape[0])}, 2] beside {int(tf.shape[0])} feature rows, got shape {tuple(coords.shape)}")
    nb = m.topk(qf, tf, k, exclude_self=exclude_self)
    if tile_coords is None:
        return nb.index, nb.score, None
    coords = coords.to(m._device)
    found = coords[nb.index.clamp(min=0)]
    return nb.index, nb.score, torch.where((nb.index >= 0)[..., None], found, torch.full_like(found, -1))


def subtype_regions(class_map, tissue=None, connectivity=8, min_area=1, model=None):
    """The region table of every class of a label map -> ``{c: keep_amd.components.RegionTable}``: the connected regions of the pixels
    labelled c (inside ``tissue``, a ``TissueMask`` of the map's geometry, optional), scored on the class's own plane of the
    ``ClassRaster`` the map came from, so a region's mean and peak are its own class's."""
    from .classmap import ClassMap
    from .region import TissueMask
    if not isinstance(class_map, ClassMap):
        raise ValueError(f"class_map must be a ClassMap, got {type(class_map).__name__}")
    if tissue is not None:
        if not isinstance(tissue, TissueMask):
            raise ValueError(f"tissue must be a TissueMask, got {type(tissue).__name__}")
        if tissue.downsample != class_map.downsample or tuple(tissue.mask.shape) != class_map.shape:
            raise ValueError(f"tissue mask has downsample {tissue.downsample} and shape {tuple(tissue.mask.shape)}, the label map "
                             f"{class_map.downsample} and {class_map.shape}")
    m = _engine(model, class_map.labels)
    out = {}
    for c in range(class_map.n_classes):
        mask = class_map.mask(c)
        if tissue is not None:
            mask = mask * (tissue.mask.to(mask.device) != 0).to(torch.uint8)
        out[c] = m.mask_regions(mask, connectivity, min_area, raster=class_map.raster.plane(c))
    return out
