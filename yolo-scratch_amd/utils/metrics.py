"""Detection metrics: P / R / mAP50 / mAP50-95 on the MI355X (libyolomi ym_eval_detections).

Drop-in for /root/reference/yolo_scratch_cuda/utils/metrics.py: same functions, arguments
and return values --
  calculate_iou :19-46, calculate_iou_batch :49-81, evaluate_detections :84-274,
  calculate_ap :277-323.
evaluate_detections packs the per-image prediction / target dicts into flat device
arrays (image offsets, no per-box Python) and runs the whole evaluation -- conf filter,
per-image score sort, greedy matching at all IoU thresholds at once, the global
TP-before-FP score sort and the all-point AP -- as one chain of HIP launches
(csrc/metrics.hip); the host reads back 4 numbers.  CPU tensors are moved to the GPU;
there is no CPU fallback (the numpy restatement is oracle/metrics.py, test-only).

The reference's evaluation is class-agnostic and so are the functions named after it.
evaluate_packed_cls / evaluate_detections_per_class are the class-aware evaluation (not in the
reference): the same algorithm with the label added, per-class AP and the mean over the classes
that have GT (ym_eval_detections_cls).
"""
from __future__ import annotations

from ctypes import c_double as ctypes_double
from typing import Dict, List, Sequence

import numpy as np
import torch

from yolomi._lib import YolomiError, call, lib, stream_ptr

GT_MAX_PER_IMAGE = 4096
MAX_CLASSES = 1024
_MAX_THR = 15


def _device(*tensors) -> torch.device:
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise YolomiError("utils.metrics runs on the MI355X only: no GPU visible "
                          "(the CPU restatement lives in oracle/metrics.py and is test-only)")
    return torch.device("cuda", torch.cuda.current_device())


def _thresholds(iou_threshold: float) -> np.ndarray:
    """The reference's IoU thresholds (:131-136), fp64 exactly as np.arange makes them."""
    if iou_threshold == 0.5:
        return np.arange(0.5, 0.95 + 1e-6, 0.05)
    return np.arange(iou_threshold, min(1.0, iou_threshold + 0.45) + 1e-6, 0.05)


def evaluate_packed(pred_boxes: torch.Tensor, pred_scores: torch.Tensor, pred_counts: Sequence[int],
                    gt_boxes: torch.Tensor, gt_counts: Sequence[int], conf_threshold: float = 0.25,
                    iou_threshold: float = 0.5) -> Dict[str, object]:
    """evaluate_detections on flat device arrays: image b owns pred rows
    sum(pred_counts[:b]) .. +pred_counts[b] (xyxy fp32 + score) and GT rows likewise.

    Returns the reference's four metrics plus ``ap`` (one AP per IoU threshold),
    ``tp50`` / ``fp50`` and ``n_valid`` (predictions kept by ``conf_threshold``)."""
    dev = _device(pred_boxes, gt_boxes)
    n_img = len(pred_counts)
    if len(gt_counts) != n_img:
        raise YolomiError(f"evaluate: {n_img} prediction sets but {len(gt_counts)} target sets")
    max_gt = max(gt_counts) if n_img else 0
    if max_gt > GT_MAX_PER_IMAGE:
        raise YolomiError(f"evaluate: {max_gt} GT boxes in one image (the matcher holds {GT_MAX_PER_IMAGE})")
    thrs = _thresholds(float(iou_threshold))
    n_ap = len(thrs)
    if iou_threshold == 0.5:
        all_thr, pr_index = thrs, 0
    else:                                   # precision / recall are always counted at 0.5 (:252)
        all_thr, pr_index = np.concatenate([thrs, [0.5]]), n_ap
    n_thr = len(all_thr)
    if n_thr > _MAX_THR:
        raise YolomiError(f"evaluate: {n_thr} IoU thresholds (max {_MAX_THR})")
    pb = pred_boxes.to(dev, torch.float32).reshape(-1, 4).contiguous()
    ps = pred_scores.to(dev, torch.float32).reshape(-1).contiguous()
    gb = gt_boxes.to(dev, torch.float32).reshape(-1, 4).contiguous()
    n_pred, n_gt = pb.shape[0], gb.shape[0]
    if ps.numel() != n_pred or sum(pred_counts) != n_pred or sum(gt_counts) != n_gt:
        raise YolomiError("evaluate: counts do not match the packed arrays")
    offs = torch.tensor(np.concatenate([[0], np.cumsum(pred_counts, dtype=np.int64),
                                        [0], np.cumsum(gt_counts, dtype=np.int64)]).astype(np.int64))
    offs = offs.to(dev, non_blocking=True)
    poff, goff = offs[: n_img + 1], offs[n_img + 1:]
    ws_bytes = lib().ym_eval_workspace_size(n_img, max(n_pred, 1), n_thr)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(n_thr + 7, dtype=torch.float64, device=dev)
    thr_c = (ctypes_double * n_thr)(*[float(t) for t in all_thr])
    call("ym_eval_detections", pb.data_ptr(), ps.data_ptr(), poff.data_ptr(), gb.data_ptr(), goff.data_ptr(),
         n_img, n_pred, n_gt, max_gt, thr_c, n_thr, n_ap, pr_index, float(conf_threshold), ws.data_ptr(), ws_bytes,
         out.data_ptr(), stream_ptr(dev))
    o = out.cpu().tolist()                   # the single host sync
    r = o[n_thr:]
    if any(v != v for v in r[:4]):
        raise YolomiError("evaluate: an image exceeded the GT capacity of the matcher")
    return {"precision": r[0], "recall": r[1], "mAP50": r[2], "mAP50-95": r[3],
            "ap": o[:n_ap], "tp50": int(r[4]), "fp50": int(r[5]), "n_valid": int(r[6])}


def evaluate_detections(predictions: List[Dict], targets: List[Dict], conf_threshold: float = 0.25,
                        iou_threshold: float = 0.5) -> Dict[str, float]:
    """Reference :84-274.  predictions[i] = {boxes (N,4) xyxy, scores (N,), labels},
    targets[i] = {boxes (M,4), labels}; labels are ignored (class-agnostic, as the reference)."""
    n = min(len(predictions), len(targets))          # zip() semantics
    dev = _device(*[p["boxes"] for p in predictions[:n]], *[t["boxes"] for t in targets[:n]])
    pbs, pss, pc, gbs, gc = [], [], [], [], []
    for pred, tgt in zip(predictions[:n], targets[:n]):
        b = torch.as_tensor(pred["boxes"]).reshape(-1, 4)
        s = torch.as_tensor(pred["scores"]).reshape(-1)
        if len(b) == 0:
            s = s[:0]
        pbs.append(b.to(dev, torch.float32))
        pss.append(s.to(dev, torch.float32))
        pc.append(int(b.shape[0]))
        g = torch.as_tensor(tgt["boxes"]).reshape(-1, 4)
        gbs.append(g.to(dev, torch.float32))
        gc.append(int(g.shape[0]))
    empty4 = torch.zeros(0, 4, device=dev)
    pb = torch.cat(pbs) if pbs else empty4
    ps = torch.cat(pss) if pss else torch.zeros(0, device=dev)
    gb = torch.cat(gbs) if gbs else empty4
    r = evaluate_packed(pb, ps, pc, gb, gc, conf_threshold, iou_threshold)
    return {k: r[k] for k in ("precision", "recall", "mAP50", "mAP50-95")}


def evaluate_packed_cls(pred_boxes: torch.Tensor, pred_scores: torch.Tensor, pred_labels: torch.Tensor,
                        pred_counts: Sequence[int], gt_boxes: torch.Tensor, gt_labels: torch.Tensor,
                        gt_counts: Sequence[int], nc: int, conf_threshold: float = 0.25,
                        iou_threshold: float = 0.5) -> Dict[str, object]:
    """Class-aware evaluate_packed (ym_eval_detections_cls): the same algorithm with the label added.
    A prediction only takes an unmatched GT box of its own label (``pred_labels`` / ``gt_labels``, integers in
    [0, nc)); class c's AP is calculate_ap over the kept predictions of label c and the GT boxes of label c.
    A class is present when it has a GT box: ``mAP50`` / ``mAP50-95`` are means over the present classes,
    ``precision`` / ``recall`` are micro-averaged over all classes at IoU 0.5.

    Returns the keys of evaluate_packed (``ap`` is the mean over the present classes per IoU threshold) plus
    ``ap_class`` (nc x n_ap), ``n_gt_class``, ``tp50_class``, ``fp50_class`` and ``present`` (class indices)."""
    dev = _device(pred_boxes, gt_boxes)
    n_img = len(pred_counts)
    nc = int(nc)
    if not 1 <= nc <= MAX_CLASSES:
        raise YolomiError(f"evaluate: nc={nc} outside 1..{MAX_CLASSES}")
    if len(gt_counts) != n_img:
        raise YolomiError(f"evaluate: {n_img} prediction sets but {len(gt_counts)} target sets")
    max_gt = max(gt_counts) if n_img else 0
    if max_gt > GT_MAX_PER_IMAGE:
        raise YolomiError(f"evaluate: {max_gt} GT boxes in one image (the matcher holds {GT_MAX_PER_IMAGE})")
    thrs = _thresholds(float(iou_threshold))
    n_ap = len(thrs)
    if iou_threshold == 0.5:
        all_thr, pr_index = thrs, 0
    else:                                   # precision / recall are always counted at 0.5 (:252)
        all_thr, pr_index = np.concatenate([thrs, [0.5]]), n_ap
    n_thr = len(all_thr)
    if n_thr > _MAX_THR:
        raise YolomiError(f"evaluate: {n_thr} IoU thresholds (max {_MAX_THR})")
    pb = pred_boxes.to(dev, torch.float32).reshape(-1, 4).contiguous()
    ps = pred_scores.to(dev, torch.float32).reshape(-1).contiguous()
    pl = pred_labels.to(dev, torch.int64).reshape(-1).contiguous()
    gb = gt_boxes.to(dev, torch.float32).reshape(-1, 4).contiguous()
    gl = gt_labels.to(dev, torch.int64).reshape(-1).contiguous()
    n_pred, n_gt = pb.shape[0], gb.shape[0]
    if (ps.numel() != n_pred or pl.numel() != n_pred or gl.numel() != n_gt or sum(pred_counts) != n_pred
            or sum(gt_counts) != n_gt):
        raise YolomiError("evaluate: counts do not match the packed arrays")
    offs = torch.tensor(np.concatenate([[0], np.cumsum(pred_counts, dtype=np.int64),
                                        [0], np.cumsum(gt_counts, dtype=np.int64)]).astype(np.int64))
    offs = offs.to(dev, non_blocking=True)
    poff, goff = offs[: n_img + 1], offs[n_img + 1:]
    ws_bytes = lib().ym_eval_cls_workspace_size(n_img, max(n_pred, 1), n_thr, nc)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(nc * n_thr + 3 * nc + 7, dtype=torch.float64, device=dev)
    thr_c = (ctypes_double * n_thr)(*[float(t) for t in all_thr])
    call("ym_eval_detections_cls", pb.data_ptr(), ps.data_ptr(), pl.data_ptr(), poff.data_ptr(), gb.data_ptr(),
         gl.data_ptr(), goff.data_ptr(), n_img, n_pred, n_gt, max_gt, nc, thr_c, n_thr, n_ap, pr_index,
         float(conf_threshold), ws.data_ptr(), ws_bytes, out.data_ptr(), stream_ptr(dev))
    o = out.cpu().numpy()                    # the single host sync
    r = o[nc * n_thr + 3 * nc:].tolist()
    if any(v != v for v in r[:4]):
        raise YolomiError(f"evaluate: a label outside [0, {nc}) or an image over the GT capacity of the matcher")
    ap_class = o[: nc * n_thr].reshape(nc, n_thr)[:, :n_ap]
    n_gt_c, tp_c, fp_c = (o[nc * n_thr + k * nc: nc * n_thr + (k + 1) * nc].astype(np.int64).tolist() for k in range(3))
    present = [c for c in range(nc) if n_gt_c[c] > 0]
    ap = ap_class[present].mean(0).tolist() if present else [0.0] * n_ap
    return {"precision": r[0], "recall": r[1], "mAP50": r[2], "mAP50-95": r[3],
            "ap": ap, "tp50": int(r[4]), "fp50": int(r[5]), "n_valid": int(r[6]),
            "ap_class": ap_class.tolist(), "n_gt_class": n_gt_c, "tp50_class": tp_c, "fp50_class": fp_c,
            "present": present}


def evaluate_detections_per_class(predictions: List[Dict], targets: List[Dict], nc: int,
                                  conf_threshold: float = 0.25, iou_threshold: float = 0.5) -> Dict[str, object]:
    """evaluate_detections with the labels honoured (evaluate_packed_cls): the same list-of-dicts input, the four
    reference keys holding the class-aware values, plus ``per_class``: ``ap50`` (AP at the first threshold),
    ``ap`` (mean AP over the thresholds), ``n_gt``, ``tp`` and ``fp`` (at IoU 0.5), nc entries each."""
    n = min(len(predictions), len(targets))          # zip() semantics
    dev = _device(*[p["boxes"] for p in predictions[:n]], *[t["boxes"] for t in targets[:n]])
    pbs, pss, pls, pc, gbs, gls, gc = [], [], [], [], [], [], []
    for pred, tgt in zip(predictions[:n], targets[:n]):
        b = torch.as_tensor(pred["boxes"]).reshape(-1, 4)
        s = torch.as_tensor(pred["scores"]).reshape(-1)
        lb = torch.as_tensor(pred["labels"]).reshape(-1)
        if len(b) == 0:
            s, lb = s[:0], lb[:0]
        pbs.append(b.to(dev, torch.float32))
        pss.append(s.to(dev, torch.float32))
        pls.append(lb.to(dev, torch.int64))
        pc.append(int(b.shape[0]))
        g = torch.as_tensor(tgt["boxes"]).reshape(-1, 4)
        gbs.append(g.to(dev, torch.float32))
        gls.append(torch.as_tensor(tgt["labels"]).reshape(-1).to(dev, torch.int64))
        gc.append(int(g.shape[0]))
    empty4 = torch.zeros(0, 4, device=dev)
    emptyl = torch.zeros(0, dtype=torch.int64, device=dev)
    pb = torch.cat(pbs) if pbs else empty4
    ps = torch.cat(pss) if pss else torch.zeros(0, device=dev)
    pl = torch.cat(pls) if pls else emptyl
    gb = torch.cat(gbs) if gbs else empty4
    gl = torch.cat(gls) if gls else emptyl
    r = evaluate_packed_cls(pb, ps, pl, pc, gb, gl, gc, nc, conf_threshold, iou_threshold)
    out = {k: r[k] for k in ("precision", "recall", "mAP50", "mAP50-95")}
    apc = np.asarray(r["ap_class"], np.float64).reshape(int(nc), -1)
    out["per_class"] = {"ap50": apc[:, 0].tolist() if apc.shape[1] else [0.0] * int(nc),
                        "ap": apc.mean(1).tolist() if apc.shape[1] else [0.0] * int(nc),
                        "n_gt": r["n_gt_class"], "tp": r["tp50_class"], "fp": r["fp50_class"]}
    return out


def calculate_ap(tp: List[float], fp: List[float], n_gt: int) -> float:
    """Reference :277-323: all-point AP of TP / FP score lists (ym_eval_ap)."""
    dev = _device()
    scores = torch.tensor(list(tp) + list(fp), dtype=torch.float32).to(dev)
    flags = torch.tensor([1] * len(tp) + [0] * len(fp), dtype=torch.uint8).to(dev)
    n = scores.numel()
    ws_bytes = lib().ym_eval_workspace_size(1, max(n, 1), 1)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(8, dtype=torch.float64, device=dev)
    call("ym_eval_ap", scores.data_ptr(), flags.data_ptr(), n, int(n_gt), ws.data_ptr(), ws_bytes, out.data_ptr(),
         stream_ptr(dev))
    return float(out[0].item())


def calculate_iou_batch(boxes1: torch.Tensor, boxes2: torch.Tensor) -> torch.Tensor:
    """Reference :49-81: (N, M) IoU of xyxy boxes, fp32 (ym_iou_matrix)."""
    dev = _device(boxes1, boxes2)
    a = torch.as_tensor(boxes1).to(dev, torch.float32).reshape(-1, 4).contiguous()
    b = torch.as_tensor(boxes2).to(dev, torch.float32).reshape(-1, 4).contiguous()
    out = torch.empty(a.shape[0], b.shape[0], dtype=torch.float32, device=dev)
    call("ym_iou_matrix", a.data_ptr(), b.data_ptr(), a.shape[0], b.shape[0], out.data_ptr(), stream_ptr(dev))
    return out


def calculate_iou(box1, box2):
    """Reference :19-46: IoU of two xyxy boxes (0-d tensor), 0.0 when the union is not positive.
    Four scalars: evaluated with device tensor ops in the reference's order (bare union, no eps)."""
    dev = _device(box1, box2)
    b1 = torch.as_tensor(box1).to(dev, torch.float32).reshape(4)
    b2 = torch.as_tensor(box2).to(dev, torch.float32).reshape(4)
    inter = (torch.clamp(torch.min(b1[2], b2[2]) - torch.max(b1[0], b2[0]), min=0.0)
             * torch.clamp(torch.min(b1[3], b2[3]) - torch.max(b1[1], b2[1]), min=0.0))
    union = (b1[2] - b1[0]) * (b1[3] - b1[1]) + (b2[2] - b2[0]) * (b2[3] - b2[1]) - inter
    if union <= 0:
        return 0.0
    return inter / union
