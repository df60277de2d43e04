"""Batch-dict contract of the reference loader.

collate_fn_cuda follows crater_dataset_cuda.py:289-346: stack images, emit
(batch_idx, cls, bboxes) with boxes converted from normalised cxcywh to xyxy
and clamped to [0, 1] (:313-322).  The crater CSV/image dataset itself
(CraterDatasetCUDA, :26-286) lives in datasets/crater.py.
"""
from __future__ import annotations

import torch


def collate_fn_cuda(batch, img_size=None, channels=1, letterbox=False, rect=False):
    """Batch dict of the reference collate (:289-346).  Images that are raw uint8 (1, h0, w0)
    (datasets.crater.CraterDatasetCUDA) are packed for the GPU resize instead of stacked:
    the dict then carries img_u8 / img_meta / img_size until datasets.prepare_batch moves it to
    the device and produces img (B, 1, S, S) fp32.  `channels` > 1: the images are pixel-interleaved
    (h0, w0, channels) (datasets.yolo_txt.YoloTxtDataset), the dict also carries img_ch and img is
    (B, channels, S, S).  `letterbox` (raw uint8 images only): the aspect ratio is kept; the dict also carries
    img_lb, (B, 4) int32 rows (nw, nh, left, top), and bboxes are normalised to the letterboxed S x S frame
    (datasets/letterbox.py).  Without it the dict has the keys and values it always had.  `rect` (with `letterbox`):
    the frame is this batch's own minimal stride-multiple H x W (datasets.letterbox.rect_frame) instead of S x S;
    img_lb and bboxes are in that frame and the dict also carries img_frame, int32 (H, W)."""
    if rect and not letterbox:
        raise ValueError("collate_fn_cuda: rect=True needs letterbox=True (a rectangular frame keeps the aspect ratio)")
    imgs, boxes_list, labels_list, _ = zip(*batch)
    if imgs and imgs[0].dtype == torch.uint8:
        from .crater import pack_images
        size = img_size or getattr(imgs[0], "img_size", None)
        if size is None:
            raise ValueError("collate_fn_cuda: raw uint8 images need img_size (functools.partial(collate_fn_cuda, "
                             "img_size=S))")
        if rect:
            out = pack_images(imgs, size, channels, letterbox, rect)
        else:
            out = pack_images(imgs, size, channels, letterbox) if letterbox else pack_images(imgs, size, channels)
    else:
        if letterbox:
            raise ValueError("collate_fn_cuda: letterbox=True needs raw uint8 images (the resize runs on the GPU)")
        out = {"img": torch.stack(imgs, 0)}
    fh, fw = (int(v) for v in out["img_frame"].tolist()) if rect else (None, None)
    bidx, cls, bboxes = [], [], []
    for i, (boxes, labels) in enumerate(zip(boxes_list, labels_list)):
        if len(boxes) == 0:
            continue
        bidx.append(torch.full((len(boxes),), i, dtype=torch.long))
        cls.append(labels.reshape(-1, 1).long())
        c, wh = boxes[:, :2], boxes[:, 2:4]
        xyxy = torch.cat((c - wh / 2, c + wh / 2), 1).clamp(0.0, 1.0)
        if letterbox:
            from .letterbox import map_labels
            xyxy = torch.from_numpy(map_labels(xyxy.numpy(), out["img_lb"][i].tolist(), fh or size, fw or size)).float()
        bboxes.append(xyxy)
    if not bidx:
        out.update({"batch_idx": torch.zeros((0,), dtype=torch.long), "cls": torch.zeros((0, 1), dtype=torch.long),
                    "bboxes": torch.zeros((0, 4), dtype=torch.float32)})
        return out
    out.update({"batch_idx": torch.cat(bidx), "cls": torch.cat(cls), "bboxes": torch.cat(bboxes).float()})
    return out
