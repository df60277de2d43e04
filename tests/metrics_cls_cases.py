"""Labelled inputs and the reference for the class-aware detection-metrics tests
(utils.metrics.evaluate_packed_cls -> ym_eval_detections_cls).

The reference needs no new implementation: class-aware matching never mixes labels and a stable filter keeps the
order, so class c's result is the class-agnostic oracle (oracle/metrics.py) run on the predictions and targets of
label c alone (reference()).  The means over the present classes and the micro-averaged precision / recall follow
from the definition in numpy.

labelled_case(): metrics_cases.random_case with labels assigned -- targets get random classes, a prediction copies
the label of its best-overlapping GT box with probability 0.8 and takes a random class otherwise.  With `roles` the
last three classes are kept special: nc-3 only ever labels predictions (absent, its predictions are FPs), nc-2 only
GT boxes (present, AP 0) and nc-1 nothing.
segment_case(): per-class valid-prediction counts of exactly 1, AP_CHUNK, AP_CHUNK + 1 and more than 2 * AP_CHUNK,
the segment lengths at which the AP stage's chunk walk changes shape."""
import functools

import numpy as np
import torch

from metrics_cases import random_case

AP_CHUNK = 2048            # detections per block of the AP stage (csrc/metrics.hip AP_CH)
OTHER_THRESHOLDS = [(0.3, 0.25), (0.75, 0.1), (0.5, 0.0), (0.5, 0.9)]     # test_gpu_metrics.test_other_thresholds


def _iou(a, b):
    iw = np.clip(np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]), 0, None)
    ih = np.clip(np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]), 0, None)
    inter = iw * ih
    ua = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    ub = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    return inter / (ua[:, None] + ub[None, :] - inter + 1e-9)


def assign_labels(preds, tgts, seed, gt_classes, pred_classes, copy_p=0.8):
    """Labels for an unlabelled case: GT boxes draw from gt_classes; a prediction copies its best-overlapping GT
    box's label with probability copy_p when that label is in pred_classes, and draws from pred_classes otherwise."""
    rng = np.random.default_rng(1000 + seed)
    gt_classes, pred_classes = np.asarray(gt_classes), np.asarray(pred_classes)

    def draw(classes, n):             # the last class (a special one under `roles`) in one draw of ten, whatever nc
        k = len(classes)
        w = np.full(k, 1.0 / k) if k < 3 else np.concatenate([np.full(k - 1, 0.9 / (k - 1)), [0.1]])
        return rng.choice(classes, n, p=w)
    for p, t in zip(preds, tgts):
        nt, npd = len(t["boxes"]), len(p["boxes"])
        tl = draw(gt_classes, nt)
        pl = draw(pred_classes, npd)
        if nt and npd:
            src = tl[np.argmax(_iou(p["boxes"].numpy(), t["boxes"].numpy()), 1)]
            copy = (rng.random(npd) < copy_p) & np.isin(src, pred_classes)
            pl = np.where(copy, src, pl)
        t["labels"] = torch.from_numpy(tl.astype(np.int64))
        p["labels"] = torch.from_numpy(pl.astype(np.int64))
    return preds, tgts


@functools.lru_cache(maxsize=None)
def labelled_case(seed, nc, roles=True, used=None, **kw):
    """(preds, tgts).  `used`: how many of the classes below the special ones carry labels (default: all of them),
    spread over the range and always including class 0 and the highest ordinary class."""
    preds, tgts = random_case(seed, **kw)
    top = nc - 3 if roles else nc
    assert top >= 1
    ordinary = np.arange(top)
    if used is not None:
        ordinary = np.unique(np.round(np.linspace(0, top - 1, used)).astype(np.int64))
    gt_classes = list(ordinary) + ([nc - 2] if roles else [])
    pred_classes = list(ordinary) + ([nc - 3] if roles else [])
    return assign_labels(preds, tgts, seed, gt_classes, pred_classes)


@functools.lru_cache(maxsize=None)
def segment_case(conf=0.25):
    """nc = 6: the kept predictions (score >= conf) of class 0 number exactly 1, of class 1 AP_CHUNK, of class 2
    AP_CHUNK + 1 and of class 3 all the rest (more than 2 * AP_CHUNK); class 4 has GT only, class 5 nothing.  Most
    GT boxes are of class 3, so its long segment holds many TPs."""
    nc = 6
    preds, tgts = random_case(21, n_img=240, max_gt=25, max_pred=120, quant=64)
    rng = np.random.default_rng(77)
    scores = np.concatenate([p["scores"].numpy() for p in preds])
    kept = rng.permutation(np.flatnonzero(scores >= np.float32(conf)))
    lab = rng.integers(0, 4, len(scores))                       # the filtered-out predictions: any class
    lab[kept] = 3
    lab[kept[:1]] = 0
    lab[kept[1:1 + AP_CHUNK]] = 1
    lab[kept[1 + AP_CHUNK:2 + 2 * AP_CHUNK]] = 2
    off = 0
    for p, t in zip(preds, tgts):
        n = len(p["scores"])
        p["labels"] = torch.from_numpy(lab[off:off + n].astype(np.int64))
        off += n
        t["labels"] = torch.from_numpy(rng.choice([0, 1, 2, 3, 4], len(t["boxes"]),
                                                  p=[0.05, 0.1, 0.1, 0.7, 0.05]).astype(np.int64))
    return preds, tgts, nc


@functools.lru_cache(maxsize=None)
def many_gt_case(beyond_lds=True):
    """Images with thousands of GT boxes, nc = 3 labels.  beyond_lds: 2510 and 4014 GT boxes, more than the
    matcher stages in LDS (2048: the labels are read through L2 beside the boxes) and matched bits up to the 63rd of
    the lane masks.  Otherwise test_gpu_metrics.test_many_gt_per_image's input, whose largest image holds 2013 GT
    boxes: the staged path filled almost to its end."""
    if beyond_lds:
        return labelled_case(12, 3, roles=False, n_img=3, max_gt=4096, max_pred=300, quant=1024)
    return labelled_case(5, 3, roles=False, n_img=3, max_gt=3000, max_pred=400, quant=1024)


def counts(preds, tgts, nc, conf=0.25):
    """(valid predictions per class, GT boxes per class)."""
    pl = np.concatenate([p["labels"].numpy() for p in preds]) if preds else np.zeros(0, np.int64)
    ps = np.concatenate([p["scores"].numpy() for p in preds]) if preds else np.zeros(0, np.float32)
    gl = np.concatenate([t["labels"].numpy() for t in tgts]) if tgts else np.zeros(0, np.int64)
    return (np.bincount(pl[ps >= np.float32(conf)], minlength=nc), np.bincount(gl, minlength=nc))


def filter_label(preds, tgts, c):
    fp = [{k: v[p["labels"] == c] for k, v in p.items()} for p in preds]
    ft = [{k: v[t["labels"] == c] for k, v in t.items()} for t in tgts]
    return fp, ft


def reference(preds, tgts, nc, conf=0.25, iou=0.5):
    """The class-aware result from the class-agnostic oracle on each label's own predictions and targets."""
    from oracle import metrics as omet
    n_ap = len(omet.thresholds(iou))
    n = min(len(preds), len(tgts))
    preds, tgts = preds[:n], tgts[:n]
    ap = np.zeros((nc, n_ap))
    tp, fp = np.zeros(nc, np.int64), np.zeros(nc, np.int64)
    pl = np.concatenate([p["labels"].numpy() for p in preds]) if preds else np.zeros(0, np.int64)
    gl = np.concatenate([t["labels"].numpy() for t in tgts]) if tgts else np.zeros(0, np.int64)
    n_gt = np.bincount(gl, minlength=nc)
    for c in np.union1d(pl, gl):          # a class with neither: the oracle's zeros (test_metrics_cls_cpu.py)
        r = omet.evaluate_detections(*filter_label(preds, tgts, c), conf, iou, per_threshold=True)
        ap[c], tp[c], fp[c] = r["ap"], r["tp50"], r["fp50"]
    present = np.flatnonzero(n_gt > 0)
    tps, fps = int(tp.sum()), int(fp.sum())
    return {"precision": tps / (tps + fps) if tps + fps else 0.0,
            "recall": tps / int(n_gt.sum()) if n_gt.sum() else 0.0,
            "mAP50": float(np.mean(ap[present, 0])) if len(present) else 0.0,
            "mAP50-95": float(np.mean(np.mean(ap[present], 1))) if len(present) else 0.0,
            "ap": np.mean(ap[present], 0).tolist() if len(present) else [0.0] * n_ap,
            "tp50": tps, "fp50": fps, "ap_class": ap.tolist(), "n_gt_class": n_gt.tolist(),
            "tp50_class": tp.tolist(), "fp50_class": fp.tolist(), "present": present.tolist()}
