"""Decode + NMS postprocess on the GPU (libyolomi ym_decode_nms / ym_nms / ym_iou_row).

Host-side mirror of decode_predictions_for_metrics / nms_simple /
calculate_iou_batch_simple (reference train_yolo11_cuda.py:265-437): same
arguments, same return types.  The whole batch is one pair of launches; the
host synchronises once (the per-image counts) instead of once per kept box.
"""
from __future__ import annotations

import torch

from ._lib import call, ptr, require_device, stream_ptr


def iou_row(box1: torch.Tensor, boxes2: torch.Tensor) -> torch.Tensor:
    require_device(box1, boxes2)
    b1 = box1.reshape(4).float().contiguous()
    b2 = boxes2.float().contiguous()
    out = torch.empty(b2.shape[0], device=b2.device, dtype=torch.float32)
    call("ym_iou_row", ptr(b1), ptr(b2), b2.shape[0], ptr(out), stream_ptr(b2.device))
    return out


def nms(boxes: torch.Tensor, scores: torch.Tensor, iou_threshold: float, labels: torch.Tensor | None = None,
        max_det: int = 0) -> torch.Tensor:
    """Keep indices (int64, device) in kept order.

    `labels` (any integer values, one per box): a box is suppressed by boxes of its own label only (batched NMS,
    ym_nms_cls); `max_det` > 0: the first `max_det` kept indices.  With the defaults: ym_nms."""
    require_device(boxes, scores)
    from ._lib import lib
    n = boxes.shape[0]
    b = boxes.float().contiguous()
    s = scores.float().contiguous()
    cls = labels is not None or max_det != 0
    ws_bytes = (lib().ym_nms_cls_workspace_size if cls else lib().ym_nms_workspace_size)(1, max(n, 1))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=b.device)
    keep = torch.empty(max(n, 1), dtype=torch.int64, device=b.device)
    cnt = torch.zeros(1, dtype=torch.int32, device=b.device)
    if cls:
        lab = None
        if labels is not None:
            require_device(labels)
            if labels.shape[0] != n:
                raise ValueError(f"nms: {labels.shape[0]} labels for {n} boxes")
            lab = labels.reshape(-1).to(torch.int64).contiguous()
        call("ym_nms_cls", ptr(b), ptr(s), ptr(lab), n, float(iou_threshold), int(max_det), ptr(ws), ws_bytes,
             ptr(keep), ptr(cnt), stream_ptr(b.device))
    else:
        call("ym_nms", ptr(b), ptr(s), n, float(iou_threshold), ptr(ws), ws_bytes, ptr(keep), ptr(cnt),
             stream_ptr(b.device))
    return keep[: int(cnt.item())]


def decode_nms(pred: torch.Tensor, img_size, conf: float, iou_thr: float, class_aware: bool = False,
               max_det: int = 0, padded: bool = False):
    """Batched decode+NMS of pred read as (B, N, 4+C).  Returns per-image dicts.

    `class_aware`: a candidate is suppressed by kept candidates of its own label only; `max_det` > 0: at most that
    many boxes per image, the best-scoring kept ones (ym_decode_nms_cls).  With the defaults: the
    reference's class-agnostic NMS (ym_decode_nms_strided).

    `img_size`: a number, the side of a square frame (ym_decode_nms_strided / ym_decode_nms_cls), or `(img_h, img_w)`,
    a frame of img_h rows and img_w columns: kept boxes are x / img_w, y / img_h (the _wh entry points).

    `padded`: one dict for the batch instead of the list: boxes (B, N, 4), scores / labels (B, N), "count" the
    per-image counts on the device (int32) and "counts" the same on the host; rows past an image's count are
    unspecified (what datasets.letterbox.unletterbox takes)."""
    require_device(pred)
    from ._lib import lib
    p = pred.float()
    if p.stride(-1) < 1:
        p = p.contiguous()
    B, N, W = p.shape
    C = W - 4
    dev = p.device
    wh = None
    if isinstance(img_size, (tuple, list, torch.Size)):
        if len(img_size) != 2:
            raise ValueError(f"decode_nms: img_size is a number or (img_h, img_w), got {tuple(img_size)}")
        wh = (float(img_size[1]), float(img_size[0]))
    if max_det and not class_aware:
        raise ValueError("decode_nms: max_det needs class_aware=True (the class-agnostic path has no cap)")
    ws_bytes = (lib().ym_nms_cls_workspace_size if class_aware else lib().ym_nms_workspace_size)(B, max(N, 1))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    cnt = torch.empty(B, dtype=torch.int32, device=dev)          # every count is written by the launch
    boxes = torch.empty(B, N, 4, dtype=torch.float32, device=dev)
    scores = torch.empty(B, N, dtype=torch.float32, device=dev)
    labels = torch.empty(B, N, dtype=torch.int64, device=dev)
    index = torch.empty(B, N, dtype=torch.int64, device=dev)
    # a row's elements may be strided (the anchor-major view y.transpose(1, 2) of the eval output): read in place
    if wh is not None and class_aware:
        call("ym_decode_nms_cls_wh", ptr(p), B, N, C, p.stride(1), p.stride(0), p.stride(2), float(conf),
             float(iou_thr), wh[0], wh[1], int(max_det), ptr(ws), ws_bytes, ptr(cnt), ptr(boxes), ptr(scores),
             ptr(labels), ptr(index), stream_ptr(dev))
    elif wh is not None:
        call("ym_decode_nms_strided_wh", ptr(p), B, N, C, p.stride(1), p.stride(0), p.stride(2), float(conf),
             float(iou_thr), wh[0], wh[1], ptr(ws), ws_bytes, ptr(cnt), ptr(boxes), ptr(scores), ptr(labels),
             ptr(index), stream_ptr(dev))
    elif class_aware:
        call("ym_decode_nms_cls", ptr(p), B, N, C, p.stride(1), p.stride(0), p.stride(2), float(conf),
             float(iou_thr), float(img_size), int(max_det), ptr(ws), ws_bytes, ptr(cnt), ptr(boxes), ptr(scores),
             ptr(labels), ptr(index), stream_ptr(dev))
    else:
        call("ym_decode_nms_strided", ptr(p), B, N, C, p.stride(1), p.stride(0), p.stride(2), float(conf),
             float(iou_thr), float(img_size), ptr(ws), ws_bytes, ptr(cnt), ptr(boxes), ptr(scores), ptr(labels),
             ptr(index), stream_ptr(dev))
    counts = cnt.cpu().tolist()                      # the single host sync of the batch
    if padded:
        return {"boxes": boxes, "scores": scores, "labels": labels, "count": cnt, "counts": counts}
    return [{"boxes": boxes[b, :k], "scores": scores[b, :k], "labels": labels[b, :k]} for b, k in enumerate(counts)]


METRICS = {"iou": 0, "ios": 1}                          # YM_MATCH_IOU, YM_MATCH_IOS


def decode_nmm_tiles(pred: torch.Tensor, table_dev: torch.Tensor, tile_begin, conf: float, thr: float,
                     metric: str = "iou", merge: bool = False, class_aware: bool = False, max_det: int = 0,
                     edge: float = 0.0):
    """Decode + greedy merging of sliced inference (ym_decode_nmm_tiles): decode_nms_tiles's candidates
    and order; a kept box absorbs every later candidate (of its label when class_aware) whose match value with the
    kept box itself exceeds `thr`.  `metric`: "iou", or "ios", the intersection over the smaller box, which matches a
    box that a tile border cut with its whole twin.  `merge`: "boxes" holds the union of the kept box and what it
    absorbed instead of the kept box.

    Returns the dict of decode_nms_tiles plus "merged" (G, R) int32: how many candidates each kept box absorbed."""
    if metric not in METRICS:
        raise ValueError(f"decode_nmm_tiles: metric is 'iou' or 'ios', got {metric!r}")
    return _decode_tiles(pred, table_dev, tile_begin, conf, thr, class_aware, max_det, edge,
                         (METRICS[metric], int(bool(merge))))


def decode_nmw_tiles(pred: torch.Tensor, table_dev: torch.Tensor, tile_begin, conf: float, thr: float,
                     metric: str = "iou", class_aware: bool = False, max_det: int = 0, edge: float = 0.0):
    """Decode + greedy merging with a score-weighted mean box (ym_decode_nmw_tiles): everything of
    decode_nmm_tiles but "boxes", where a kept box that absorbed candidates holds the score-weighted mean of itself
    and what it absorbed, formed in fixed point on integer sums (order-independent, bit for bit reproducible); a kept
    box that absorbed nothing is unchanged.  The merge for several estimates of one whole box, as the views of
    test-time augmentation give them."""
    if metric not in METRICS:
        raise ValueError(f"decode_nmw_tiles: metric is 'iou' or 'ios', got {metric!r}")
    return _decode_tiles(pred, table_dev, tile_begin, conf, thr, class_aware, max_det, edge, (METRICS[metric], "mean"))


def decode_nms_tiles(pred: torch.Tensor, table_dev: torch.Tensor, tile_begin, conf: float, iou_thr: float,
                     class_aware: bool = False, max_det: int = 0, edge: float = 0.0):
    """Decode + NMS of sliced inference (ym_decode_nms_tiles): pred read as (T, N, 4+C), one slice per
    tile; `table_dev` the device table of ym_tile_entry (uint8 bytes, at least T entries); `tile_begin` the G + 1
    host values that give image g the tiles [tile_begin[g], tile_begin[g + 1]).  Every tile's candidates are mapped
    to source pixels, those a tile border cuts within `edge` pixels are dropped (0: none), and one NMS runs per
    image over the rest.

    Returns the padded dict of decode_nms(..., padded=True) with R = N * (the largest tile count) rows per image and
    "boxes" in source pixels (xyxy, unnormalised), plus "rows" (G, R) int64: the row of the image's (tile, row)
    concatenation a kept box came from, tile = row // N."""
    return _decode_tiles(pred, table_dev, tile_begin, conf, iou_thr, class_aware, max_det, edge, None)


def _decode_tiles(pred, table_dev, tile_begin, conf, thr, class_aware, max_det, edge, nmm):
    """nmm: None (ym_decode_nms_tiles), (metric, merge) (ym_decode_nmm_tiles, which also fills "merged") or
    (metric, "mean") (ym_decode_nmw_tiles)."""
    import ctypes
    from ._lib import TileEntry, lib
    require_device(pred, table_dev)
    p = pred.float()
    if p.stride(-1) < 1:
        p = p.contiguous()
    T, N, W = p.shape
    C = W - 4
    dev = p.device
    begin = [int(v) for v in tile_begin]
    G = len(begin) - 1
    if G < 0:
        raise ValueError("decode_nms_tiles: tile_begin holds G + 1 values")
    if max_det and not class_aware:
        raise ValueError("decode_nms_tiles: max_det needs class_aware=True (the class-agnostic path has no cap)")
    assert table_dev.dtype == torch.uint8 and table_dev.numel() >= T * ctypes.sizeof(TileEntry)
    most = max([b - a for a, b in zip(begin, begin[1:])] + [0])
    R = max(N * most, 0)
    cb = (ctypes.c_int64 * (G + 1))(*begin)
    mean = nmm is not None and nmm[1] == "mean"
    size_fn = lib().ym_decode_nmw_tiles_workspace_size if mean else lib().ym_decode_nms_tiles_workspace_size
    ws_bytes = size_fn(G, max(R, 1), int(class_aware))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    cnt = torch.empty(G, dtype=torch.int32, device=dev)          # every count is written by the launch
    boxes = torch.empty(G, R, 4, dtype=torch.float32, device=dev)
    scores = torch.empty(G, R, dtype=torch.float32, device=dev)
    labels = torch.empty(G, R, dtype=torch.int64, device=dev)
    index = torch.empty(G, R, dtype=torch.int64, device=dev)
    rows = torch.empty(G, R, dtype=torch.int64, device=dev)
    out = {"boxes": boxes, "scores": scores, "labels": labels, "count": cnt, "index": index, "rows": rows}
    if nmm is None:
        call("ym_decode_nms_tiles", ptr(p), T, N, C, p.stride(1), p.stride(0), p.stride(2), ptr(table_dev), cb, G,
             float(conf), float(thr), float(edge), int(class_aware), int(max_det), ptr(ws), ws_bytes, ptr(cnt),
             ptr(boxes), ptr(scores), ptr(labels), ptr(index), ptr(rows), stream_ptr(dev))
    elif mean:
        out["merged"] = torch.empty(G, R, dtype=torch.int32, device=dev)
        call("ym_decode_nmw_tiles", ptr(p), T, N, C, p.stride(1), p.stride(0), p.stride(2), ptr(table_dev), cb, G,
             float(conf), float(thr), nmm[0], float(edge), int(class_aware), int(max_det), ptr(ws), ws_bytes,
             ptr(cnt), ptr(boxes), ptr(scores), ptr(labels), ptr(index), ptr(rows), ptr(out["merged"]),
             stream_ptr(dev))
    else:
        out["merged"] = torch.empty(G, R, dtype=torch.int32, device=dev)
        call("ym_decode_nmm_tiles", ptr(p), T, N, C, p.stride(1), p.stride(0), p.stride(2), ptr(table_dev), cb, G,
             float(conf), float(thr), nmm[0], nmm[1], float(edge), int(class_aware), int(max_det), ptr(ws), ws_bytes,
             ptr(cnt), ptr(boxes), ptr(scores), ptr(labels), ptr(index), ptr(rows), ptr(out["merged"]),
             stream_ptr(dev))
    out["counts"] = cnt.cpu().tolist()               # the single host sync of the group
    return out
