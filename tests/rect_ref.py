"""Rectangular inference restated (helper of test_rect_cpu.py and test_gpu_rect.py; no test of its own).

  frame            the frame rule of DESIGN §23 in fp64, written out from its definition
  decode_wh        oracle.post.decode with the kept boxes divided by fp32 [W, H, W, H] instead of one img_size
  decode_cls_wh    the same over tests/nms_cls_ref.py's class-aware keep lists
Suppression runs on pixel boxes, so the kept lists do not depend on the frame: they are computed once per
(input, flavour, cap) and every frame divides the same pixel boxes.
"""
import math

import numpy as np

import nms_cls_ref as NR
from oracle import post as op

F32 = np.float32

# the worked values of the frame rule: (h0, w0), imgsz -> (H, W), (nw, nh, left, top)
WORKED = [
    ((480, 640), 640, (480, 640), (640, 480, 0, 0)),
    ((1080, 1920), 640, (384, 640), (640, 360, 0, 12)),
    ((1920, 1080), 640, (640, 384), (360, 640, 12, 0)),
    ((427, 640), 640, (448, 640), (640, 427, 0, 10)),
    ((3, 7), 64, (32, 64), (64, 27, 0, 2)),
    ((7, 5), 32, (32, 32), (23, 32, 4, 0)),
    ((90, 160), 160, (96, 160), (160, 90, 0, 3)),
    ((97, 160), 160, (128, 160), (160, 97, 0, 15)),
    ((241, 400), 160, (96, 160), (159, 96, 0, 0)),
    ((33, 17), 160, (160, 96), (82, 160, 7, 0)),
    ((1, 1), 160, (160, 160), (160, 160, 0, 0)),
]
WORKED_BATCH = [
    ([(60, 100), (100, 60)], 160, (160, 160)),
    ([(60, 100), (0, 0)], 160, (96, 160)),
]


def frame(hws, imgsz, stride=32):
    """(H, W): per image with pixels r = imgsz / max(h0, w0), n = min(imgsz, max(1, floor(side r + 0.5))); the
    frame's sides are the largest n rounded up to the stride; no image with pixels: (stride, stride)."""
    nh, nw = [], []
    for h0, w0 in hws:
        if h0 <= 0 or w0 <= 0:
            continue
        r = float(imgsz) / float(max(h0, w0))
        nh.append(min(imgsz, max(1, int(math.floor(h0 * r + 0.5)))))
        nw.append(min(imgsz, max(1, int(math.floor(w0 * r + 0.5)))))
    if not nh:
        return stride, stride
    return int(math.ceil(max(nh) / stride)) * stride, int(math.ceil(max(nw) / stride)) * stride


def normalise(xyxy, H, W):
    """Pixel xyxy -> the frame's normalised boxes: one fp32 division per coordinate, then the clamp."""
    d = np.array([W, H, W, H], F32)
    return np.clip(np.asarray(xyxy, F32).reshape(-1, 4) / d, 0.0, 1.0).astype(F32).reshape(-1, 4)


_KEPT = {}


def kept(name, pred, conf, iou_thr, cls=False, max_det=0):
    """Per image (pixel xyxy, scores, labels) of the kept candidates, in kept order; cached under `name` (the
    caller's name of `pred`), computed once."""
    key = (name, float(conf), float(iou_thr), bool(cls), int(max_det))
    if key not in _KEPT:
        outs = []
        for p in np.asarray(pred, F32):
            xyxy, mx, lab = NR.candidates(p, conf)
            keep = NR.nms_cls(xyxy, mx, lab, iou_thr, max_det) if cls else op.nms(xyxy, mx, iou_thr)
            outs.append((xyxy[keep].reshape(-1, 4), mx[keep], lab[keep].astype(np.int64)))
        _KEPT[key] = outs
    return _KEPT[key]


def decode_wh(name, pred, H, W, conf, iou_thr):
    """oracle.post.decode for an H x W frame -> per image (boxes, scores, labels)."""
    return [(normalise(b, H, W), s, l) for b, s, l in kept(name, pred, conf, iou_thr)]


def decode_cls_wh(name, pred, H, W, conf, iou_thr, max_det=0):
    """nms_cls_ref.decode_cls for an H x W frame -> per image (boxes, scores, labels)."""
    return [(normalise(b, H, W), s, l) for b, s, l in kept(name, pred, conf, iou_thr, True, max_det)]
