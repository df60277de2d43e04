"""Letterbox preprocessing: the aspect ratio kept, the rest of the S x S frame filled.

The geometry of every image is computed once, here, on the host in fp64 (`letterbox_geometry`, Ultralytics'
LetterBox with a centred pad) and travels to the device in a table of ym_lb_entry (include/yolomi.h): the kernels
derive nothing, so host and device cannot disagree about a size or an offset.

  letterbox_batch   ym_letterbox_u8c: packed uint8 images -> (B, C, H, W) fp32, resized to (nw, nh) at (left, top)
  map_labels        normalised source boxes -> normalised boxes of the letterboxed frame (what the loss and the
                    validation metrics see: ground truth and predictions agree there)
  unletterbox       ym_unletterbox_boxes: detections of the letterboxed frame -> source-pixel boxes
  rect_frame        the minimal stride-multiple H x W frame of a batch (rectangular inference)
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from yolomi._lib import LbEntry


def letterbox_geometry(h0: int, w0: int, H: int, W: int, scaleup: bool = True):
    """(nw, nh, left, top) of an h0 x w0 image in an H x W frame, in fp64: r = min(H / h0, W / w0) (at most 1
    without `scaleup`), the resized size rounded half up and kept inside [1, frame], the pad split with the floor
    on the left / top (Ultralytics' round(d / 2 - 0.1)).  An image without pixels gets (0, 0, 0, 0): all fill."""
    h0, w0, H, W = int(h0), int(w0), int(H), int(W)
    if h0 <= 0 or w0 <= 0:
        return 0, 0, 0, 0
    r = min(H / h0, W / w0)
    if not scaleup:
        r = min(r, 1.0)
    nw = min(W, max(1, math.floor(w0 * r + 0.5)))
    nh = min(H, max(1, math.floor(h0 * r + 0.5)))
    return nw, nh, (W - nw) // 2, (H - nh) // 2


def rect_frame(hws, imgsz: int, stride: int = 32):
    """(H, W) of the smallest frame with sides that are multiples of `stride` holding every (h0, w0) of `hws`
    resized so that its longer side is `imgsz` (rectangular inference), in fp64: per image
    r = imgsz / max(h0, w0), nh = min(imgsz, max(1, floor(h0 r + 0.5))), nw likewise; H = ceil(max nh / stride)
    * stride, W likewise.  Images without pixels are ignored; none at all gives (stride, stride).  The image's place
    in the frame is then letterbox_geometry(h0, w0, H, W)."""
    imgsz, stride = int(imgsz), int(stride)
    if stride < 1 or imgsz < stride or imgsz % stride:
        raise ValueError(f"rect_frame: imgsz {imgsz} is not a positive multiple of the stride {stride}")
    mh = mw = 0
    for h0, w0 in hws:
        h0, w0 = int(h0), int(w0)
        if h0 <= 0 or w0 <= 0:
            continue
        r = imgsz / max(h0, w0)
        mh = max(mh, min(imgsz, max(1, math.floor(h0 * r + 0.5))))
        mw = max(mw, min(imgsz, max(1, math.floor(w0 * r + 0.5))))
    if mh == 0:
        return stride, stride
    return -(-mh // stride) * stride, -(-mw // stride) * stride


def _hw(meta):
    m = meta.cpu().numpy() if isinstance(meta, torch.Tensor) else np.asarray(meta)
    return m.reshape(-1, 3)[:, 1:].astype(np.int64)


def geometry_of(meta, H: int, W: int, scaleup: bool = True) -> np.ndarray:
    """meta (B, 3) {offset, h0, w0} -> (B, 4) int32 rows (nw, nh, left, top)."""
    return np.array([letterbox_geometry(h0, w0, H, W, scaleup) for h0, w0 in _hw(meta)], np.int32).reshape(-1, 4)


def table_of(meta, geom):
    """ctypes table of ym_lb_entry from meta and its (B, 4) geometry rows; sx = fp32(w0) / fp32(nw) in fp32."""
    hw = _hw(meta)
    geom = (geom.cpu().numpy() if isinstance(geom, torch.Tensor) else np.asarray(geom)).reshape(-1, 4)
    assert len(geom) == len(hw), (len(geom), len(hw))
    t = (LbEntry * max(len(hw), 1))()
    for e, (h0, w0), (nw, nh, left, top) in zip(t, hw, geom):
        e.nw, e.nh, e.left, e.top, e.w0, e.h0 = int(nw), int(nh), int(left), int(top), int(w0), int(h0)
        if nw > 0 and nh > 0:
            e.sx = float(np.float32(w0) / np.float32(nw))
            e.sy = float(np.float32(h0) / np.float32(nh))
    return t


def lb_table(meta, H: int, W: int, scaleup: bool = True):
    """meta (B, 3) {offset, h0, w0} -> the batch's ctypes table of ym_lb_entry."""
    return table_of(meta, geometry_of(meta, H, W, scaleup))


def table_bytes(table, n: int | None = None) -> torch.Tensor:
    """ctypes array of LbEntry -> host uint8 tensor of its first n entries (a copy)."""
    nb = (len(table) if n is None else n) * ctypes.sizeof(LbEntry)
    return torch.from_numpy(np.frombuffer(bytes(table), dtype=np.uint8)[:nb].copy())


def letterbox_batch(img_u8: torch.Tensor, meta: torch.Tensor, table: torch.Tensor, H: int, W: int, channels: int = 1,
                    fill: int = 114) -> torch.Tensor:
    """GPU: packed uint8 images (pixel-interleaved for channels > 1) + device table of ym_lb_entry (uint8 bytes)
    -> (B, channels, H, W) fp32 (ym_letterbox_u8c)."""
    from yolomi._lib import call, require_device, stream_ptr
    require_device(img_u8, meta, table)
    B = meta.shape[0]
    assert table.dtype == torch.uint8 and table.numel() >= B * ctypes.sizeof(LbEntry)
    out = torch.empty(B, channels, H, W, dtype=torch.float32, device=img_u8.device)
    call("ym_letterbox_u8c", img_u8.data_ptr(), meta.contiguous().data_ptr(), table.data_ptr(), B, channels, H, W,
         int(fill), out.data_ptr(), stream_ptr(img_u8.device))
    return out


def map_labels(xyxy_norm, geom, H: int, W: int) -> np.ndarray:
    """Boxes normalised to the source image -> normalised to the H x W frame, fp64: x' = (x * nw + left) / W,
    y' = (y * nh + top) / H.  `geom`: (nw, nh, left, top)."""
    b = np.asarray(xyxy_norm, np.float64).reshape(-1, 4)
    nw, nh, left, top = (float(v) for v in geom)
    return (b * np.array([nw, nh, nw, nh]) + np.array([left, top, left, top])) / np.array([W, H, W, H], np.float64)


def unmap_labels(xyxy_frame, geom, H: int, W: int) -> np.ndarray:
    """map_labels' inverse in fp64: x = (x' * W - left) / nw."""
    b = np.asarray(xyxy_frame, np.float64).reshape(-1, 4)
    nw, nh, left, top = (float(v) for v in geom)
    return (b * np.array([W, H, W, H], np.float64) - np.array([left, top, left, top])) / np.array([nw, nh, nw, nh])


def unletterbox_padded(boxes: torch.Tensor, count: torch.Tensor, table_dev: torch.Tensor, H: int, W: int,
                       out: torch.Tensor | None = None) -> torch.Tensor:
    """ym_unletterbox_boxes on the padded form: boxes (B, N, 4) fp32 normalised xyxy, count (B,) int32 on the
    device -> source-pixel xyxy (B, N, 4); rows past an image's count keep what `out` held (zeros when it is made
    here).  Nothing is read back."""
    from yolomi._lib import call, require_device, stream_ptr
    require_device(boxes, count, table_dev)
    B, N = int(boxes.shape[0]), int(boxes.shape[1])
    assert boxes.dtype == torch.float32 and boxes.is_contiguous() and count.dtype == torch.int32
    assert table_dev.dtype == torch.uint8 and table_dev.numel() >= B * ctypes.sizeof(LbEntry)
    if out is None:
        out = torch.zeros_like(boxes)
    call("ym_unletterbox_boxes", boxes.data_ptr(), count.data_ptr(), table_dev.data_ptr(), B, N, int(H), int(W),
         out.data_ptr(), stream_ptr(boxes.device))
    return out


def unletterbox(dets, table_dev: torch.Tensor, H: int, W: int):
    """Detections of the letterboxed frame -> source pixels.  `dets` is what yolomi.post.decode_nms returns: the
    padded dict of decode_nms(..., padded=True) (boxes (B, N, 4), count on the device, counts on the host), or the
    list of per-image dicts, whose boxes are padded here.  Returns the list of per-image dicts with "boxes" in
    source pixels; scores and labels are passed through.  The counts are already on the host (decode_nms' one
    sync): no further one is made."""
    if isinstance(dets, dict):
        boxes, count, counts = dets["boxes"], dets["count"], dets["counts"]
        scores, labels = dets["scores"], dets["labels"]
        mapped = unletterbox_padded(boxes, count, table_dev, H, W)
        return [{"boxes": mapped[b, :k], "scores": scores[b, :k], "labels": labels[b, :k]}
                for b, k in enumerate(counts)]
    if not dets:
        return []
    counts = [int(d["boxes"].shape[0]) for d in dets]
    dev = dets[0]["boxes"].device
    N = max(max(counts), 1)
    boxes = torch.zeros(len(dets), N, 4, dtype=torch.float32, device=dev)
    for b, d in enumerate(dets):
        boxes[b, :counts[b]] = d["boxes"]
    count = torch.tensor(counts, dtype=torch.int32).to(dev, non_blocking=True)
    mapped = unletterbox_padded(boxes, count, table_dev, H, W)
    return [{**d, "boxes": mapped[b, :k]} for b, (d, k) in enumerate(zip(dets, counts))]
