"""Tile-level zero-shot evaluation protocol on the GPU.

Mirrors ``training/path_training/zero_shot.py:91-232`` (``zero_shot_eval``): 50 prompt rounds of zero-shot
classification scored by weighted F1 (median / Q1 / Q3 over the rounds) and text->image retrieval p@10 / p@50, with
the metric definitions of ``training/path_open_clip/zeroshot_metrics.py``.  The reference pulls every embedding to
numpy and loops in Python (50 GEMMs + N Python argmaxes per round; one dot product + argsort per caption); here the
embeddings stay on the device and the two loops are ``keep_group_argmax`` (one fp32 GEMM ``[N,768]x[768,50*C]`` +
per-(tile, round) argmax) and ``keep_retrieval_rank`` (fp32 GEMM + rank of the target per caption).  Only the
``[N,50]`` int32 labels / ``[P]`` int32 ranks cross to the host, where the F1 arithmetic runs in float64 as sklearn's.
"""
from __future__ import annotations

import json
from typing import Dict, Iterable, List, Mapping, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from .model import _ptr, _stream
from .wsi import _engine, _normalized

ROUNDS = 50          # zero_shot.py:57 / :125 hard-code 50 prompt rounds


def label2cap(prompts: Union[str, Mapping]) -> Dict[str, List[str]]:
    """zero_shot.py:49-62.  ``prompts``: the parsed prompt JSON or its path (``cfg.DATASET.ZEROSHOT_CLS_PROMPTS``)."""
    if isinstance(prompts, str):
        with open(prompts) as f:
            prompts = json.load(f)
    label_captions: Dict[str, List[str]] = {}
    for type_name in list(prompts["0"]["classnames"].keys()):
        label_captions[type_name] = [
            prompts[str(i)]["templates"].replace("CLASSNAME", prompts[str(i)]["classnames"][type_name]) for i in range(ROUNDS)]
    return label_captions


def weighted_f1_from_confusion(conf: np.ndarray) -> float:
    """sklearn ``f1_score(average='weighted')`` (zeroshot_metrics.py:31) from a confusion matrix ``conf[true, pred]``:
    per-class F1 (0 where undefined) weighted by the class's true count."""
    conf = conf.astype(np.float64)
    tp = np.diag(conf)
    fp = conf.sum(0) - tp
    fn = conf.sum(1) - tp
    den = 2 * tp + fp + fn
    f = np.divide(2 * tp, den, out=np.zeros_like(den), where=den > 0)
    return float(np.average(f, weights=tp + fn))


def _round_predictions(m, image_embeddings: torch.Tensor, cap_embeddings: Mapping[str, torch.Tensor], label_list: Sequence):
    """-> (true int64 [N], pred int32 [N,50] on the host, A = the number of class names, caption classes first)."""
    names = list(cap_embeddings.keys())
    C = len(names)
    img = _normalized(m, torch.as_tensor(image_embeddings))
    caps = torch.stack([torch.as_tensor(cap_embeddings[n]).to(m._device, torch.float32) for n in names])      # [C, 50, D]
    if caps.shape[1] < ROUNDS:
        raise ValueError(f"need {ROUNDS} caption embeddings per class, got {caps.shape[1]}")
    K, D = ROUNDS, caps.shape[2]
    bank = _normalized(m, caps[:, :K].permute(1, 0, 2).reshape(K * C, D))                                      # row k*C + c
    N = img.shape[0]
    labels = torch.empty((N, K), dtype=torch.int32, device=m._device)
    rc = _lib.load().keep_group_argmax(m._handle, _ptr(img), _ptr(bank), N, K, C, D, _ptr(labels), _stream(m._device))
    _lib.check(m._handle, rc, "group_argmax")
    pred = labels.cpu().numpy()
    all_names = names + sorted(set(label_list) - set(names))
    index = {n: i for i, n in enumerate(all_names)}
    true = np.array([index[t] for t in label_list], dtype=np.int64)
    if true.shape[0] != N:
        raise ValueError(f"{N} embeddings but {true.shape[0]} labels")
    return true, pred, len(all_names)


def classification_rounds(model, image_embeddings: torch.Tensor, cap_embeddings: Mapping[str, torch.Tensor],
                          label_list: Sequence) -> np.ndarray:
    """zero_shot.py:118-139 -> WF1 of each of the 50 prompt rounds (float64 [50]).

    ``cap_embeddings[type_name]`` is ``[50, D]`` (row i = the class's caption of round i); ``label_list`` holds the
    true class names (any label outside the caption classes counts as never predicted, as in sklearn)."""
    true, pred, A = _round_predictions(_engine(model), image_embeddings, cap_embeddings, label_list)
    K = pred.shape[1]
    out = np.empty(K)
    for k in range(K):
        conf = np.bincount(true * A + pred[:, k], minlength=A * A).reshape(A, A)
        out[k] = weighted_f1_from_confusion(conf)
    return out


def classification_rounds_ci(model, image_embeddings: torch.Tensor, cap_embeddings: Mapping[str, torch.Tensor], label_list: Sequence,
                             round: int = 0, n_boot: int = 1000, seed: int = 0):        # noqa: A002 -- the protocol's word for a prompt set
    """The weighted F1 of one prompt round with its bootstrap replicates -> ``keep_amd.bootstrap.BootstrapResult``:
    ``estimate`` is ``classification_rounds(...)[round]``, ``ci()`` its percentile interval over ``n_boot`` resamples of the tiles.
    Arguments as :func:`classification_rounds`; at most 16 class names in all (the confusion kernel's limit).  Two rounds with equal
    ``seed`` resample the same tiles: ``a.minus(b)`` is the interval of their difference."""
    m = _engine(model)
    true, pred, A = _round_predictions(m, image_embeddings, cap_embeddings, label_list)
    if not 0 <= int(round) < pred.shape[1]:
        raise ValueError(f"round must be in 0 .. {pred.shape[1] - 1}, got {round!r}")
    return m.bootstrap_metric(true, pred[:, int(round)].astype(np.int64), max(A, 2), "weighted_f1", n_boot, seed)


def linear_probe(model, train_x, train_y, test_x, test_y, n_classes: int, l2: float = 1e-3, class_weight=None, gtol: float = 1e-4,
                 max_iter: int = 1000, n_boot: int = 1000, seed: int = 0, roc: bool = True) -> dict:
    """The linear-probe protocol on frozen features: ``KEEPModel.probe_fit`` on the training tiles, then
    ``probe_predict`` on the test tiles, scored as sklearn scores predicted labels -> a dict with ``probe`` (the
    ``keep_amd.probe.LinearProbe``), ``labels`` / ``probs`` (the test predictions on the device), ``confusion`` (int64 ``[C, C]``,
    ``confusion[true, pred]``), ``balanced_accuracy`` and ``weighted_f1`` (float64 on the host, sklearn's definitions), ``skipped``
    (test tiles the skip rule left out; they are in no metric, as are test tiles labelled -1), and, for ``C <= 16`` (the confusion
    kernel's limit) and ``n_boot > 0``, ``balanced_accuracy_ci`` / ``weighted_f1_ci`` (``bootstrap_metric`` results, paired by
    ``seed``), else None; with ``roc=True`` also ``ovr_roc``: ``bootstrap_ovr_roc``'s ``(per_class, macro)`` on the probabilities."""
    from . import bootstrap
    m = _engine(model)
    probe = m.probe_fit(train_x, train_y, n_classes, l2=l2, class_weight=class_weight, gtol=gtol, max_iter=max_iter)
    C = probe.n_classes
    labels, probs, _, _ = m.probe_predict(probe, test_x)
    truth = m._probe_labels(test_y, int(labels.shape[0]))
    if int(truth.max()) >= C or int(truth.min()) < -1:
        raise ValueError(f"test labels must lie in -1..{C - 1}")
    keep = (labels >= 0) & (truth >= 0)
    t, p = truth[keep].to(torch.int64), labels[keep].to(torch.int64)
    if t.numel() == 0:
        raise ValueError("no labelled test tile is kept")
    conf = torch.bincount(t * C + p, minlength=C * C).reshape(C, C).cpu().numpy()
    out = dict(probe=probe, labels=labels, probs=probs, confusion=conf, balanced_accuracy=float(bootstrap.balanced_accuracy(conf)),
               weighted_f1=weighted_f1_from_confusion(conf), skipped=int((labels < 0).sum()), balanced_accuracy_ci=None,
               weighted_f1_ci=None, ovr_roc=None)
    if n_boot > 0 and C <= 16:
        out["balanced_accuracy_ci"] = m.bootstrap_metric(t, p, C, "balanced_accuracy", n_boot, seed)
        out["weighted_f1_ci"] = m.bootstrap_metric(t, p, C, "weighted_f1", n_boot, seed)
    if n_boot > 0 and roc:
        out["ovr_roc"] = m.bootstrap_ovr_roc(probs[keep], t, n_boot, seed)
    return out


def attention_mil(model, train_bags, train_labels, test_bags, test_labels, n_classes: int, hidden: int = 64, l2: float = 1e-4,
                  class_weight=None, lr: float = 0.01, n_steps: int = 300, fit_seed: int = 0, n_boot: int = 1000, seed: int = 0,
                  roc: bool = True) -> dict:
    """The slide-level supervised protocol on frozen features, attention-based multiple-instance learning:
    ``KEEPModel.mil_fit`` on the training slides, then ``mil_predict`` on the test slides -> :func:`linear_probe`'s dict with ``mil`` (the
    ``keep_amd.mil.AttentionMIL``) in place of ``probe`` and ``attention`` (fp32 ``[N_test]``: the test tiles' weights within their slide)
    beside it.  ``train_bags`` / ``test_bags``: ``(features fp32 [N, D], offsets [S + 1])`` pairs, ``*_labels``: integers ``[S]``, -1 for a
    slide to leave out.  ``skipped`` counts the test slides without a kept tile; they are in no metric."""
    from . import bootstrap
    m = _engine(model)
    mil = m.mil_fit(train_bags[0], train_bags[1], train_labels, n_classes, hidden=hidden, l2=l2, class_weight=class_weight, lr=lr, n_steps=n_steps,
                    seed=fit_seed)
    C = mil.n_classes
    labels, probs, attention, _ = m.mil_predict(mil, test_bags[0], test_bags[1])
    truth = m._probe_labels(test_labels, int(labels.shape[0]))
    if int(truth.max()) >= C or int(truth.min()) < -1:
        raise ValueError(f"test labels must lie in -1..{C - 1}")
    keep = (labels >= 0) & (truth >= 0)
    t, p = truth[keep].to(torch.int64), labels[keep].to(torch.int64)
    if t.numel() == 0:
        raise ValueError("no labelled test slide is kept")
    conf = torch.bincount(t * C + p, minlength=C * C).reshape(C, C).cpu().numpy()
    out = dict(mil=mil, labels=labels, probs=probs, attention=attention, confusion=conf, balanced_accuracy=float(bootstrap.balanced_accuracy(conf)),
               weighted_f1=weighted_f1_from_confusion(conf), skipped=int((labels < 0).sum()), balanced_accuracy_ci=None,
               weighted_f1_ci=None, ovr_roc=None)
    if n_boot > 0 and C <= 16:
        out["balanced_accuracy_ci"] = m.bootstrap_metric(t, p, C, "balanced_accuracy", n_boot, seed)
        out["weighted_f1_ci"] = m.bootstrap_metric(t, p, C, "weighted_f1", n_boot, seed)
    if n_boot > 0 and roc:
        out["ovr_roc"] = m.bootstrap_ovr_roc(probs[keep], t, n_boot, seed)
    return out


def knn_probe(model, train_x, train_y, test_x, test_y, n_classes: int, k: int = 20, weights: str = "softmax", temperature: float = 0.07,
              n_boot: int = 1000, seed: int = 0, roc: bool = True) -> dict:
    """The kNN-probe protocol on frozen features, :func:`linear_probe`'s non-parametric twin: every test
    tile's ``k`` nearest labelled training tiles by cosine (``KEEPModel.topk``) vote for its class (``KEEPModel.knn_vote``: uniform
    votes, or DINO's ``exp(s / temperature)`` weights) -> :func:`linear_probe`'s dict with ``neighbours`` (the ``Neighbours`` of the test
    tiles in the kept training rows) in place of ``probe``; ``probs`` are the vote shares, and ``skipped`` counts the test tiles without
    a label (the skip rule, or no voting neighbour).  Training rows labelled -1 are dropped from the bank before the search, so they
    take no neighbour slot."""
    from . import bootstrap
    from .neighbours import check_k, check_vote_args
    m = _engine(model)
    C, _, _ = check_vote_args(n_classes, weights, temperature)
    k = check_k(k)
    m._ready_device()
    ty = m._probe_labels(train_y, int(train_x.shape[0]))
    if int(ty.max()) >= C or int(ty.min()) < -1:
        raise ValueError(f"training labels must lie in -1..{C - 1}")
    on = ty >= 0
    if not bool(on.any()):
        raise ValueError("no labelled training tile")
    bank = m._on_device(train_x)[on].contiguous()
    nb = m.topk(test_x, bank, k)
    labels, probs, _, _ = m.knn_vote(nb, ty[on], C, weights, temperature)
    truth = m._probe_labels(test_y, int(labels.shape[0]))
    if int(truth.max()) >= C or int(truth.min()) < -1:
        raise ValueError(f"test labels must lie in -1..{C - 1}")
    keep = (labels >= 0) & (truth >= 0)
    t, p = truth[keep].to(torch.int64), labels[keep].to(torch.int64)
    if t.numel() == 0:
        raise ValueError("no labelled test tile is kept")
    conf = torch.bincount(t * C + p, minlength=C * C).reshape(C, C).cpu().numpy()
    out = dict(neighbours=nb, labels=labels, probs=probs, confusion=conf, balanced_accuracy=float(bootstrap.balanced_accuracy(conf)),
               weighted_f1=weighted_f1_from_confusion(conf), skipped=int((labels < 0).sum()), balanced_accuracy_ci=None,
               weighted_f1_ci=None, ovr_roc=None)
    if n_boot > 0 and C <= 16:
        out["balanced_accuracy_ci"] = m.bootstrap_metric(t, p, C, "balanced_accuracy", n_boot, seed)
        out["weighted_f1_ci"] = m.bootstrap_metric(t, p, C, "weighted_f1", n_boot, seed)
    if n_boot > 0 and roc:
        out["ovr_roc"] = m.bootstrap_ovr_roc(probs[keep], t, n_boot, seed)
    return out


def few_shot(model, train_x, train_y, test_x, test_y, n_classes: int, shots: Sequence[int] = (1, 2, 4, 8, 16, 32), n_episodes: int = 1000,
             seed: int = 0) -> dict:
    """The few-shot prototype protocol on frozen features: SimpleShot with centring and L2 normalisation over
    ``n_episodes`` random support sets per shot count (``KEEPModel.fewshot_episodes``) -> ``{k: dict}`` for every ``k`` of ``shots``, each
    with ``confusions`` (int64 ``[E, C, C]`` on the host), ``balanced_accuracy`` and ``weighted_f1`` (float64 ``[E]``, one value per
    episode) and, for either metric, ``<metric>_median`` / ``_q1`` / ``_q3`` / ``_mean`` over the episodes: the statistics the 50-round
    zero-shot protocol reports.  Every shot count draws from the same ``seed``; a class smaller than ``k`` gives all its rows."""
    from . import bootstrap
    m = _engine(model)
    out = {}
    for k in shots:
        conf = m.fewshot_episodes(train_x, train_y, test_x, test_y, n_classes, k, n_episodes, seed).cpu().numpy()
        res = dict(confusions=conf)
        for name, fn in (("balanced_accuracy", bootstrap.balanced_accuracy), ("weighted_f1", bootstrap.weighted_f1)):
            v = np.asarray(fn(conf), np.float64)
            q1, med, q3 = np.percentile(v, [25, 50, 75])
            res.update({name: v, name + "_median": float(med), name + "_q1": float(q1), name + "_q3": float(q3), name + "_mean": float(v.mean())})
        out[int(k)] = res
    return out


def retrieval_ranks(model, image_embeddings: torch.Tensor, text_embeddings: torch.Tensor,
                    targets: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Position of each caption's target image in its descending similarity list (int32 [P] on the device)."""
    m = _engine(model)
    img = _normalized(m, torch.as_tensor(image_embeddings))
    txt = _normalized(m, torch.as_tensor(text_embeddings))
    P, D = txt.shape
    tgt = None if targets is None else torch.as_tensor(targets).to(m._device, torch.int32).contiguous()
    if tgt is not None and (tgt.numel() != P or int(tgt.min()) < 0 or int(tgt.max()) >= img.shape[0]):
        raise ValueError("targets must be [P] image indices")
    rank = torch.empty(P, dtype=torch.int32, device=m._device)
    rc = _lib.load().keep_retrieval_rank(m._handle, _ptr(txt), _ptr(img), P, img.shape[0], D, _ptr(tgt), _ptr(rank), _stream(m._device))
    _lib.check(m._handle, rc, "retrieval_rank")
    return rank


def retrieval_metrics(model, image_embeddings: torch.Tensor, text_embeddings: torch.Tensor) -> Dict[str, float]:
    """zero_shot.py:161-176 + zeroshot_metrics.py:6-17 (caption t must retrieve image t)."""
    rank = retrieval_ranks(model, image_embeddings, text_embeddings).cpu().numpy()
    n = image_embeddings.shape[0]                # the reference divides by len(y_target) = number of images
    return {"p@10": int((rank < 10).sum()) / n, "p@50": int((rank < 50).sum()) / n}


def _batches(split) -> Iterable:
    return split.dataloader if hasattr(split, "dataloader") else split


def _tokenize(tokenizer, texts: Sequence[str], device):
    # zero_shot.py:72 (`pad_to_max_length=True` is the deprecated spelling of padding='max_length')
    enc = tokenizer(list(texts), add_special_tokens=True, max_length=256, padding="max_length", truncation=True, return_tensors="pt")
    return enc.to(device) if hasattr(enc, "to") else {k: v.to(device) for k, v in enc.items()}


def zero_shot_eval(model, tokenizer, data: Mapping, prompts: Union[str, Mapping, None] = None) -> Dict[str, float]:
    """zero_shot.py:79-232 for a :class:`keep_amd.KEEPModel`.

    ``data`` may hold ``'zeroshot_cls'`` (batches of ``(images, labels)``), ``'zeroshot_ret'`` and ``'zeroshot_po'``
    (batches of ``(images, captions)``); each value is an iterable of batches or an object with ``.dataloader`` as in
    the reference.  Returns the reference's result keys."""
    m = _engine(model)
    dev = m._device
    results: Dict[str, float] = {}
    if "zeroshot_cls" in data:
        feats, label_list = [], []
        for images, labels in _batches(data["zeroshot_cls"]):
            feats.append(m.encode_image(images.to(dev)))
            label_list.extend(labels)
        caps = {name: m.encode_text(_tokenize(tokenizer, c, dev)) for name, c in label2cap(prompts).items()}
        val_cls = classification_rounds(m, torch.cat(feats), caps, label_list)
        q1, med, q3 = np.percentile(val_cls, (25, 50, 75), method="midpoint")           # zero_shot.py:217
        results["zeroshot-cls-WF1-median"], results["zeroshot-cls-WF1-Q1"], results["zeroshot-cls-WF1-Q3"] = float(med), float(q1), float(q3)
    for key, tag in (("zeroshot_ret", "ret"), ("zeroshot_po", "po")):
        if key in data:
            fi, ft = [], []
            for images, texts in _batches(data[key]):
                out = m(images.to(dev), _tokenize(tokenizer, texts, dev))
                fi.append(out["vision_features"]); ft.append(out["text_features"])
            r = retrieval_metrics(m, torch.cat(fi), torch.cat(ft))
            results[f"zeroshot-{tag}-p@10"], results[f"zeroshot-{tag}-p@50"] = r["p@10"], r["p@50"]
    return results
