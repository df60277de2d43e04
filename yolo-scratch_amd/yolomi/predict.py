"""From images to detections in the images' own pixels.

Predictor chains four device steps per batch, none of which leaves the GPU:
  pack + ym_letterbox_u8c    the raw uint8 images -> (B, ch, S, S) fp32, the aspect ratio kept
  eval forward               the model's one-launch eval graph (yolomi/graph.py); the batch is padded with empty
                             images to a fixed size, so the captured graph replays for every batch, the last included
  decode + NMS               yolomi.post.decode_nms on the anchor-major view (labels are classes)
  ym_unletterbox_boxes       kept boxes -> source-pixel xyxy through the same geometry table
The host synchronises once per batch, for the per-image counts.

`rect=True`: every image gets its own minimal multiple-of-32 frame (datasets.letterbox.rect_frame) in
place of the imgsz x imgsz square, images are grouped by frame, and the four steps run per group at (H, W); the
results come back in input order.

`slice=TILE`: sliced inference.  The sources of a group are packed and uploaded once; the network runs on
their overlapping TILE x TILE windows at full resolution (datasets.slicing), each letterboxed into the imgsz x imgsz
frame by ym_slice_letterbox_u8c, `batch` tiles per forward; ym_decode_nms_tiles maps every tile's candidates into
source pixels and runs one NMS per source image, so there is no unletterbox step.  One host sync per group.
`slice_merge` / `slice_metric` put ym_decode_nmm_tiles in that NMS's place: greedy merging, matched by the
IoU or by the intersection over the smaller box.

`tta=VIEWS`: test-time augmentation.  Every window (the whole image, or the tiles of `slice`) is rendered
once per view (scale, flip) by the same slice kernel, mirrored and reduced on the device from the one upload; the tile
decode maps every view's boxes back through the mirror, and one merge per image joins the views: the NMS, the greedy
merge, or `slice_merge="mean"`, ym_decode_nmw_tiles, the score-weighted mean box of every cluster.
"""
from __future__ import annotations

import numpy as np
import torch

from . import post as _post
from ._lib import YolomiError


class Predictor:
    """predictor(images) -> per image {"boxes" (n, 4) fp32 xyxy in source pixels, "scores" (n,), "labels" (n,)}, on
    the device.  `images`: uint8 arrays (or tensors), (h, w, ch) — (h, w) also for one plane.  `class_aware`: NMS
    within a class, at most `max_det` boxes per image (0: no cap); without it the class-agnostic NMS, which has no
    cap.  `batch`: the fixed batch size of the forward; more images run in several batches.  `rect`: rectangular
    frames, one per image shape (imgsz must be a multiple of 32); images of one frame run together in chunks of
    `batch`, so the plan and graph of (batch, H, W) replay, and the eval plans of at most `max_frames`
    most-recently-used frames are kept (yolomi.graph.FrameLRU).  Without `rect` nothing is ever dropped.
    `slice`: sliced inference on slice x slice windows that share `slice_overlap` of their side; `slice_full`: one more
    pass over the whole image, for objects larger than a tile; `slice_edge` > 0: a tile's boxes within that many
    pixels of a window side that is not an image side are left to the neighbouring tile.  Not with `rect`.
    `slice_merge`: "nms" suppresses the tiles' boxes, "nmm" merges them greedily: a kept box absorbs what
    matches it and becomes the union, and the results also carry "merged", the number each box absorbed;
    `slice_metric`: the match value `iou` is compared with, "iou" or "ios" (intersection over the smaller box, which
    joins a box cut by a tile border to its whole twin).  "mean" merges as "nmm" does but the kept box becomes the
    score-weighted mean of what it absorbed (the merge for the views of `tta`).  They need `slice` or `tta`.
    `tta`: None, True (datasets.tta.DEFAULT_VIEWS: scales 1 / 0.83 / 0.67, the middle view mirrored left-right) or a
    list of (scale, flip) views, 0 < scale <= 1, flip "", "lr", "ud" or "lrud"; with or without `slice`, not with
    `rect`."""

    def __init__(self, model, imgsz: int = 640, ch: int | None = None, conf: float = 0.25, iou: float = 0.45,
                 max_det: int = 300, class_aware: bool = True, device="cuda", batch: int = 8, fill: int = 114,
                 rect: bool = False, max_frames: int = 8, slice: int = 0, slice_overlap: float = 0.2,
                 slice_full: bool = True, slice_edge: float = 0.0, slice_merge: str = "nms",
                 slice_metric: str = "iou", tta=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise YolomiError("Predictor runs on the MI355X only (no CPU fallback)")
        self.model = model.to(self.device).eval()
        stem = int(model.model[0].conv.in_channels)
        self.ch = stem if ch is None else int(ch)
        if self.ch != stem:
            raise ValueError(f"Predictor: ch={self.ch} but the model's stem takes {stem} planes")
        self.imgsz, self.conf, self.iou = int(imgsz), float(conf), float(iou)
        self.max_det, self.class_aware, self.batch, self.fill = int(max_det), bool(class_aware), int(batch), int(fill)
        if self.batch < 1 or self.imgsz < 1:
            raise ValueError("Predictor: batch and imgsz are at least 1")
        self.rect, self._lru = bool(rect), None
        self.slice, self.slice_overlap = int(slice), float(slice_overlap)
        self.slice_full, self.slice_edge = bool(slice_full), float(slice_edge)
        if self.slice < 0:
            raise ValueError("Predictor: slice is a tile size in pixels (0: off)")
        self.views = None
        if tta is not None and tta is not False:
            from datasets.tta import DEFAULT_VIEWS, check_views
            self.views = check_views(DEFAULT_VIEWS if tta is True else tta)
            if rect:
                raise ValueError("Predictor: tta and rect exclude each other (views run in the imgsz x imgsz frame)")
        if slice_merge not in ("nms", "nmm", "mean") or slice_metric not in _post.METRICS:
            raise ValueError(f"Predictor: slice_merge is 'nms', 'nmm' or 'mean' and slice_metric 'iou' or 'ios', got "
                             f"{slice_merge!r}, {slice_metric!r}")
        if (slice_merge, slice_metric) != ("nms", "iou") and not self.slice and self.views is None:
            raise ValueError("Predictor: slice_merge and slice_metric belong to sliced inference (slice=TILE) and to "
                             "test-time augmentation (tta=VIEWS)")
        self.slice_merge, self.slice_metric = slice_merge, slice_metric
        if self.slice:
            if rect:
                raise ValueError("Predictor: slice and rect exclude each other (tiles run in the imgsz x imgsz frame)")
            from datasets.slicing import slice_step
            slice_step(self.slice, self.slice_overlap)               # raises on an overlap that leaves no step
        if self.rect:
            from datasets.letterbox import rect_frame
            from .graph import FrameLRU
            rect_frame([], self.imgsz)                               # raises unless imgsz is a multiple of the stride
            self._lru = FrameLRU.of(self.model, max_frames)

    def _raw(self, im) -> torch.Tensor:
        """One image in the layout pack_images takes: (1, h, w) for one plane, (h, w, ch) otherwise."""
        t = torch.from_numpy(np.ascontiguousarray(im)) if isinstance(im, np.ndarray) else im.cpu().contiguous()
        if t.dtype != torch.uint8:
            raise ValueError(f"Predictor: images are uint8, got {t.dtype}")
        if self.ch == 1 and t.dim() == 3 and t.shape[-1] == 1:
            t = t[..., 0]
        if self.ch == 1 and t.dim() == 2:
            return t.unsqueeze(0)
        if self.ch > 1 and t.dim() == 3 and t.shape[-1] == self.ch:
            return t
        raise ValueError(f"Predictor: expected (h, w{', ' + str(self.ch) if self.ch > 1 else ''}) uint8 images, got "
                         f"{tuple(t.shape)}")

    def letterbox(self, images, frame=None):
        """pack + ym_letterbox_u8c of up to `batch` images, padded with empty ones -> (img (batch, ch, H, W) on the
        device, the device table of ym_lb_entry).  `frame`: (H, W); None: the imgsz x imgsz square."""
        from datasets.crater import pack_images
        from datasets.letterbox import lb_table, letterbox_batch, table_bytes
        raw = [self._raw(im) for im in images]
        empty = torch.empty((1, 0, 0) if self.ch == 1 else (0, 0, self.ch), dtype=torch.uint8)
        raw += [empty] * (self.batch - len(raw))
        packed = pack_images(raw, self.imgsz, self.ch)
        H, W = frame or (self.imgsz, self.imgsz)
        tb = table_bytes(lb_table(packed["img_meta"], H, W), self.batch).pin_memory()
        mv = lambda t: t.to(self.device, non_blocking=True)          # noqa: E731
        table = mv(tb)
        return letterbox_batch(mv(packed["img_u8"]), mv(packed["img_meta"]), table, H, W, self.ch, self.fill), table

    @torch.no_grad()
    def _run(self, images, frame=None):
        from datasets.letterbox import unletterbox
        img, table = self.letterbox(images, frame)
        H, W = frame or (self.imgsz, self.imgsz)
        if self._lru is not None:
            self._lru.touch(self.batch, H, W)
        y = self.model(img)[0]                                       # (batch, 4 + nc, A)
        dets = _post.decode_nms(y.transpose(1, 2), self.imgsz if frame is None else (H, W), self.conf, self.iou,
                                class_aware=self.class_aware, max_det=self.max_det if self.class_aware else 0,
                                padded=True)
        return unletterbox(dets, table, H, W)[:len(images)]

    @torch.no_grad()
    def _run_sliced(self, images):
        """Up to `batch` sources: one upload, the tiles `batch` at a time through the slice kernel and the eval
        forward (the last chunk padded with src = -1 tiles, so the plan and graph of (batch, imgsz, imgsz) replay),
        every chunk's output copied into one (T, 4 + nc, A) buffer, then one ym_decode_nms_tiles and its sync.
        With `tta` the table holds every window once per view (datasets.tta.view_table); nothing else differs."""
        from datasets.crater import pack_images
        from datasets.slicing import slice_batch, tile_bytes, tile_table
        raw = [self._raw(im) for im in images]
        packed = pack_images(raw, self.imgsz, self.ch)
        S, nb = self.imgsz, self.batch
        hws = packed["img_meta"][:, 1:].tolist()
        if self.views is None:
            table, begin = tile_table(hws, self.slice, self.slice_overlap, S, self.slice_full)
        else:
            from datasets.tta import view_table
            table, begin = view_table(hws, self.views, S, self.slice, self.slice_overlap, self.slice_full)
        T = begin[-1]
        if T == 0:
            z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=self.device)    # noqa: E731
            nmm = (self.slice_merge, self.slice_metric) != ("nms", "iou")
            return [{"boxes": z(0, 4), "scores": z(0), "labels": z(0, dt=torch.int64),
                     **({"merged": z(0, dt=torch.int32)} if nmm else {})} for _ in images]
        Tp = -(-T // nb) * nb
        mv = lambda t: t.to(self.device, non_blocking=True)          # noqa: E731
        tdev = mv(tile_bytes(table, T, Tp).pin_memory())
        u8, meta = mv(packed["img_u8"]), mv(packed["img_meta"])
        ybuf = None
        for lo in range(0, Tp, nb):
            img = slice_batch(u8, meta, tdev, nb, S, S, self.ch, self.fill, first=lo)
            y = self.model(img)[0]                                   # (batch, 4 + nc, A)
            if ybuf is None:
                ybuf = torch.empty(Tp, *y.shape[1:], dtype=y.dtype, device=y.device)
            ybuf[lo:lo + nb].copy_(y)                                # before the next replay overwrites it
        kw = dict(class_aware=self.class_aware, max_det=self.max_det if self.class_aware else 0, edge=self.slice_edge)
        keys = ("boxes", "scores", "labels")
        if (self.slice_merge, self.slice_metric) == ("nms", "iou"):
            d = _post.decode_nms_tiles(ybuf[:T].transpose(1, 2), tdev, begin, self.conf, self.iou, **kw)
        elif self.slice_merge == "mean":
            d = _post.decode_nmw_tiles(ybuf[:T].transpose(1, 2), tdev, begin, self.conf, self.iou,
                                       metric=self.slice_metric, **kw)
            keys += ("merged",)
        else:
            d = _post.decode_nmm_tiles(ybuf[:T].transpose(1, 2), tdev, begin, self.conf, self.iou,
                                       metric=self.slice_metric, merge=self.slice_merge == "nmm", **kw)
            keys += ("merged",)
        return [{key: d[key][g, :k] for key in keys} for g, k in enumerate(d["counts"])]

    def frame_of(self, im):
        """(H, W) of one image's rectangular frame."""
        from datasets.letterbox import rect_frame
        t = self._raw(im)
        hw = (int(t.shape[-2]), int(t.shape[-1])) if self.ch == 1 else (int(t.shape[0]), int(t.shape[1]))
        return rect_frame([hw], self.imgsz)

    def __call__(self, images):
        images = list(images)
        if self.rect:
            groups = {}                                              # frame -> input positions, first seen first
            for i, im in enumerate(images):
                groups.setdefault(self.frame_of(im), []).append(i)
            out = [None] * len(images)
            for frame, pos in groups.items():
                for lo in range(0, len(pos), self.batch):
                    chunk = pos[lo:lo + self.batch]
                    for i, d in zip(chunk, self._run([images[i] for i in chunk], frame)):
                        out[i] = d
            return out
        out = []
        for lo in range(0, len(images), self.batch):
            out += (self._run_sliced if self.slice or self.views else self._run)(images[lo:lo + self.batch])
        return out
