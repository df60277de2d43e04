"""Train YOLOv11 on MI355X — drop-in for the reference entry point.

Same CLI flags, same functions and return conventions as the reference's
train_yolo11_cuda.py (/root/reference/yolo_scratch_cuda/train_yolo11_cuda.py):
train_one_epoch :31-98, validate :101-262, decode_predictions_for_metrics
:265-358, nms_simple :361-399, calculate_iou_batch_simple :402-437,
cosine_lr_schedule :440-451, main :454-661.

What differs underneath: the model forward/backward, the loss and the decode +
NMS postprocess run as hand-written HIP kernels for gfx950 (libyolomi.so);
per-step loss items are accumulated on the device and read back every
`LOG_EVERY` steps instead of four host syncs per step; `--synthetic N` trains
on N synthetic batches when no dataset is mounted; multi-GPU data parallelism
is enabled by launching with torchrun (one process per GPU, RCCL).
"""
from __future__ import annotations

import argparse
import math
import os
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).parent))

from models.yolo11_model import build_yolo11  # noqa: E402
from losses.yolo_v8_loss import v8DetectionLoss  # noqa: E402
from datasets import collate_fn_cuda, prepare_batch  # noqa: E402
from utils.metrics import evaluate_detections, evaluate_detections_per_class  # noqa: E402
from yolomi import post as _post  # noqa: E402

collate_fn = collate_fn_cuda
LOG_EVERY = 10


def _tqdm(it, **kw):
    try:
        from tqdm import tqdm
        return tqdm(it, **kw)
    except Exception:  # pragma: no cover
        return it


def train_one_epoch(model, dataloader, optimizer, criterion, device, epoch, epochs, dp=None, augment=None, ema=None):
    """One epoch (reference :31-98).  `dp` is an optional yolomi.dist.GradSync; `augment` an optional
    datasets.BatchAugment, applied in place of prepare_batch (the train and val subsets share one dataset
    object, so the switch lives in the step: validate never augments); `ema` an optional yolomi.ema.ModelEMA,
    updated after every optimizer step unless the optimizer does that itself (`fuses_ema`)."""
    model.train()
    pbar = _tqdm(dataloader, desc=f"Epoch {epoch}/{epochs}")
    sums = torch.zeros(4, device=device)
    n = 0
    for batch_idx, batch in enumerate(pbar):
        if augment is not None:
            batch = augment(batch, device, epoch, batch_idx)      # H2D + mosaic / affine / flip / gain in one launch
        else:
            batch = prepare_batch(batch, device)        # H2D (+ GPU resize of raw images)
        optimizer.zero_grad(set_to_none=True)
        preds = model(batch["img"])
        loss, loss_items = criterion(preds, batch)
        loss.backward()
        if dp is not None:
            dp.sync()
        if not getattr(optimizer, "fuses_clip", False):    # FusedAdamW clips on the device itself
            torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=10.0)
        optimizer.step()
        if ema is not None and not getattr(optimizer, "fuses_ema", False):    # FusedAdamW averages in its pass
            ema.update()
        sums[0] += loss.detach()
        sums[1:] += loss_items.detach()
        n += 1
        if hasattr(pbar, "set_postfix") and (batch_idx + 1) % LOG_EVERY == 0:
            s = (sums / n).tolist()
            pbar.set_postfix({"loss": f"{s[0]:.4f}", "box": f"{s[1]:.4f}", "cls": f"{s[2]:.4f}", "dfl": f"{s[3]:.4f}"})
    s = (sums / max(len(dataloader), 1)).tolist()
    return {"loss": s[0], "box_loss": s[1], "cls_loss": s[2], "dfl_loss": s[3]}


_PER_CLASS_KEYS = ("ap50", "ap", "n_gt", "tp", "fp")


def _head_nc(model):
    """Class count of the model's Detect head."""
    for m in reversed(list(model.modules())):
        if isinstance(getattr(m, "nc", None), int) and hasattr(m, "reg_max"):
            return m.nc
    raise ValueError("validate(per_class=True): the model has no Detect head to take nc from; pass nc")


@torch.no_grad()
def validate(model, dataloader, criterion, device, conf_threshold=0.25, iou_threshold=0.45, max_batches=None,
             dp=None, per_class=False, nc=None, nms_per_class=False, max_det=0, max_frames=None):
    """Validation + metrics (reference :101-262).  Under data parallelism (`dp`, a GradSync) each
    rank evaluates its ValShard of the val set (decode + NMS on its own GPU), the per-image
    detections are gathered to rank 0 in the global image order and evaluate_detections runs there
    (SURVEY §8(e)); the loss sums are all-reduced and the metrics broadcast, so every rank returns
    the same dict.

    `per_class`: the class-aware evaluation (utils.metrics.evaluate_detections_per_class) over `nc`
    classes (default: the Detect head's) in place of the reference's class-agnostic one: the same keys
    hold the class-aware values and "per_class" the per-class lists.  Its detections are decoded from the
    anchor-major view of the eval output, whose labels are classes.

    `nms_per_class` (needs `per_class`: only that read has classes for labels): class-aware NMS, a box is
    suppressed by kept boxes of its own class only, and at most `max_det` boxes per image (0: no cap), the
    usual YOLO evaluation recipe.  The result's keys do not change.

    A batch whose image is not square (the `--val-rect` loader) is decoded with its own (H, W); the
    metrics stay in the frame's normalised coordinates, where GT and predictions agree.  `max_frames`: keep the
    eval plans of at most that many most-recently-used (B, H, W) frames (yolomi.graph.FrameLRU); None, the
    default, never drops a plan."""
    if nms_per_class and not per_class:
        raise ValueError("validate(nms_per_class=True) needs per_class=True: the reference's literal read of the "
                         "eval output has anchor indices for labels, and suppression by those means nothing")
    if max_det and not nms_per_class:
        raise ValueError("validate(max_det=N) needs nms_per_class=True: the class-agnostic NMS has no cap")
    model.eval()
    if per_class and nc is None:
        nc = _head_nc(model)
    lru = None
    if max_frames is not None:
        from yolomi.graph import FrameLRU
        lru = FrameLRU.of(model, max_frames)
    sums = torch.zeros(4, device=device)
    all_predictions, all_targets = [], []
    batches = 0
    for batch in _tqdm(dataloader, desc="Validating"):
        batch = prepare_batch(batch, device)
        if lru is not None:
            lru.touch(batch["img"].shape[0], batch["img"].shape[-2], batch["img"].shape[-1])
        preds = model(batch["img"])
        loss, loss_items = criterion(preds, batch)
        sums[0] += loss
        sums[1:] += loss_items
        decoded = preds[0] if isinstance(preds, tuple) and len(preds) == 2 else model(batch["img"])[0]
        if per_class:
            # labels must be classes: decode the anchor-major view (B, A, 4+nc) of the eval output, read in place.
            # The reference's literal read of (B, 4+nc, A) takes anchors for classes
            decoded = decoded.transpose(1, 2)
        # a rectangular frame (a --val-rect batch) is normalised per axis; a square one makes the call it always made
        fh, fw = int(batch["img"].shape[-2]), int(batch["img"].shape[-1])
        frame = fw if fh == fw else (fh, fw)
        if nms_per_class:
            predictions = decode_predictions_for_metrics(decoded, frame, conf_threshold, iou_threshold, device,
                                                         class_aware=True, max_det=max_det)
        else:
            predictions = decode_predictions_for_metrics(decoded, frame, conf_threshold, iou_threshold, device)
        all_predictions.extend(predictions)
        bidx, bboxes, cls = batch["batch_idx"], batch["bboxes"], batch["cls"]
        for i in range(batch["img"].shape[0]):
            m = bidx == i
            all_targets.append({"boxes": bboxes[m], "labels": cls[m].reshape(-1)})
        batches += 1
        if max_batches is not None and batches >= max_batches:
            break
    nb = torch.tensor([float(batches)], device=device)
    world = dp.ctx.world if dp is not None else 1
    if world > 1:
        import torch.distributed as tdist
        from yolomi.dist import gather_detections
        tdist.all_reduce(sums)
        tdist.all_reduce(nb)
        all_predictions, all_targets = gather_detections(all_predictions, all_targets, dp.ctx, device)
    keys = ("precision", "recall", "mAP50", "mAP50-95")
    if all_predictions is not None:
        # predictions and targets stay in HBM: the metrics run on the GPU (utils/metrics.py)
        if per_class:
            metrics = evaluate_detections_per_class(all_predictions, all_targets, nc, conf_threshold=conf_threshold,
                                                    iou_threshold=0.5)
        else:
            metrics = evaluate_detections(all_predictions, all_targets, conf_threshold=conf_threshold,
                                          iou_threshold=0.5)
    if world > 1:
        vals = [float(metrics[k]) for k in keys] if all_predictions is not None else [0.0] * 4
        if per_class:                         # the per-class lists travel with the four scalars (counts: exact in fp64)
            vals += ([float(v) for k in _PER_CLASS_KEYS for v in metrics["per_class"][k]]
                     if all_predictions is not None else [0.0] * (len(_PER_CLASS_KEYS) * nc))
        mt = torch.tensor(vals, dtype=torch.float64, device=device)
        tdist.broadcast(mt, 0)
        mt = mt.tolist()
        metrics = dict(zip(keys, mt[:4]))
        if per_class:
            rows = {k: mt[4 + i * nc: 4 + (i + 1) * nc] for i, k in enumerate(_PER_CLASS_KEYS)}
            metrics["per_class"] = {k: ([int(v) for v in r] if k in ("n_gt", "tp", "fp") else r)
                                    for k, r in rows.items()}
    nbatch = float(nb) if (max_batches or world > 1) else len(dataloader)
    s = (sums / max(nbatch, 1)).tolist()
    return {"loss": s[0], "box_loss": s[1], "cls_loss": s[2], "dfl_loss": s[3], **metrics}


def decode_predictions_for_metrics(preds, img_size, conf_threshold, iou_threshold, device, class_aware=False,
                                   max_det=0):
    """Per-image boxes/scores/labels (normalised xyxy) from decoded predictions.

    Reads `preds` as (batch, rows, 4+C) exactly like the reference (:289-301),
    including when it is handed the (B, 4+nc, A) eval tensor.
    One batched GPU launch pair; one host sync for the per-image counts.
    `class_aware` / `max_det`: class-aware NMS with a detection cap (yolomi.post.decode_nms).
    """
    pred = preds[0] if isinstance(preds, tuple) and len(preds) == 2 else preds
    if class_aware or max_det:
        return _post.decode_nms(pred, img_size, conf_threshold, iou_threshold, class_aware=class_aware,
                                max_det=max_det)
    return _post.decode_nms(pred, img_size, conf_threshold, iou_threshold)


def nms_simple(boxes, scores, iou_threshold):
    """Greedy class-agnostic NMS; returns the list of kept indices (reference :361-399)."""
    if len(boxes) == 0:
        return []
    return _post.nms(boxes, scores, iou_threshold).cpu().tolist()


def calculate_iou_batch_simple(boxes1, boxes2):
    """IoU of boxes1 (1,4) against boxes2 (M,4) (reference :402-437)."""
    if boxes1.dim() == 1:
        boxes1 = boxes1.unsqueeze(0)
    rows = [_post.iou_row(b, boxes2) for b in boxes1]
    iou = torch.stack(rows) if rows else boxes2.new_zeros(0, boxes2.shape[0])
    return iou.squeeze() if iou.dim() > 1 and iou.shape[0] == 1 else iou


def cosine_lr_schedule(optimizer, epoch, epochs, lr_min=1e-6, lr_max=1e-3, warmup_epochs=3):
    """Per-epoch cosine schedule with linear warm-up (reference :440-451)."""
    if epoch < warmup_epochs:
        lr = lr_min + (lr_max - lr_min) * (epoch / warmup_epochs)
    else:
        progress = (epoch - warmup_epochs) / (epochs - warmup_epochs)
        lr = lr_min + (lr_max - lr_min) * 0.5 * (1 + math.cos(math.pi * progress))
    for g in optimizer.param_groups:
        g["lr"] = lr
    return lr


def make_checkpoint(epoch, model, optimizer, train_metrics, val_metrics, best_loss, best_mAP50, ema=None):
    """The reference's checkpoint dict (train_yolo11_cuda.py:628-636), key for key: last.pt / best.pt
    written by either implementation resume in the other (tests/test_models_cpu.py).  With `ema` (a
    yolomi.ema.ModelEMA) the averaged weights follow as "ema_state_dict" and "ema_updates"; "model_state_dict"
    stays the raw training weights, so the resume and the reference's loader see what they saw."""
    ckpt = {"epoch": epoch, "model_state_dict": model.state_dict(), "optimizer_state_dict": optimizer.state_dict(),
            "train_metrics": train_metrics, "val_metrics": val_metrics, "best_loss": best_loss,
            "best_mAP50": best_mAP50}
    if ema is not None:
        ckpt.update(ema.state_dict())
    return ckpt


def _np_safe_globals():
    """numpy scalar reconstructors a reference-written checkpoint needs: its evaluate_detections
    returns np.float64 mAP values (utils/metrics.py:264-274) that end up in val_metrics and
    best_mAP50.  These rebuild plain numbers; nothing else is allowed through the restricted loader."""
    import numpy as np
    out = [np.dtype, type(np.dtype(np.float64)), type(np.dtype(np.float32)), type(np.dtype(np.int64))]
    for mod in ("numpy._core.multiarray", "numpy.core.multiarray"):
        try:
            m = __import__(mod, fromlist=["scalar"])
            out.append(m.scalar)
            break
        except (ImportError, AttributeError):
            continue
    return out



def _load_np_safe(path, device):
    with torch.serialization.safe_globals(_np_safe_globals()):
        return torch.load(path, map_location=device, weights_only=True)


def load_checkpoint(path, model, device, ema=False):
    """Weights of a last.pt / best.pt into `model`, for inference -> the key they came from.  `ema`: the averaged
    weights ("ema_state_dict") when the checkpoint holds them, else (and without `ema`) "model_state_dict"."""
    ckpt = _load_np_safe(path, device)
    key = "ema_state_dict" if ema and "ema_state_dict" in ckpt else "model_state_dict"
    model.load_state_dict(ckpt[key])
    return key


def resume_checkpoint(path, model, optimizer, device, ema=None):
    """Resume as the reference does (:576-586) -> (start_epoch, best_loss, best_mAP50).  Loaded with
    weights_only=True plus the numpy scalar types a reference-written checkpoint holds (its metrics
    are np.float64); the optimizer keeps this process's fused/foreach implementation choice across a
    reference-written state.  `ema` (a yolomi.ema.ModelEMA) takes the checkpoint's average and update count;
    a checkpoint without them (written without --ema, or by the reference) restarts it from the loaded weights."""
    ckpt = _load_np_safe(path, device)
    model.load_state_dict(ckpt["model_state_dict"])
    if ema is not None:
        if "ema_state_dict" in ckpt:
            ema.load_state_dict(ckpt)
        else:
            ema.seed(model)
    impl = [{k: g.get(k) for k in ("fused", "foreach")} for g in optimizer.param_groups]
    optimizer.load_state_dict(ckpt["optimizer_state_dict"])
    for g, kv in zip(optimizer.param_groups, impl):
        g.update(kv)
    return ckpt["epoch"] + 1, ckpt.get("best_loss", float("inf")), ckpt.get("best_mAP50", 0.0)


def make_loaders(dataset, val_split, batch, workers, imgsz, dp_ctx=None, collate=None, channels=1, letterbox=False,
                 val_rect=False):
    """The reference's split and loaders (:491-543): seed-42 permutation, Subset train / val,
    shuffled train loader, ordered val loader, drop_last=False.  Under data parallelism the train set
    is sharded by a DistributedSampler(shuffle=True, drop_last=True): every rank gets the same number
    of samples and so the same number of batches (a rank with one batch more would enter the gradient
    all-reduce alone and hang), reshuffled every epoch (set_epoch); the val set by ValShard (no
    padding: no image counted twice).  `channels`: the dataset's image planes, handed to the collate; `letterbox`:
    both loaders keep the images' aspect ratio (datasets/letterbox.py) instead of stretching them.  `val_rect`: the
    val loader alone letterboxes into each batch's minimal stride-multiple frame (collate rect=True) and walks its
    images (its shard, under data parallelism) by aspect ratio (datasets.RectSampler), so neighbours share a frame.
    -> (train_loader, val_loader, train_sampler or None)."""
    import functools
    from torch.utils.data import DataLoader, DistributedSampler, Subset
    n = len(dataset)
    val_size = int(n * val_split)
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(42)).tolist()
    tr, va = Subset(dataset, idx[: n - val_size]), Subset(dataset, idx[n - val_size:])
    nw = min(workers, 4)
    col = collate or (functools.partial(collate_fn, img_size=imgsz, channels=channels, letterbox=True) if letterbox
                      else functools.partial(collate_fn, img_size=imgsz, channels=channels))
    kw = dict(batch_size=batch, num_workers=nw, collate_fn=col, pin_memory=torch.cuda.is_available(),
              persistent_workers=nw > 0, prefetch_factor=2 if nw > 0 else None, drop_last=False)
    if dp_ctx is not None and dp_ctx.world > 1:
        from yolomi.dist import ValShard
        sampler = DistributedSampler(tr, num_replicas=dp_ctx.world, rank=dp_ctx.rank, shuffle=True, seed=0,
                                     drop_last=True)
        vs = ValShard(len(va), dp_ctx.rank, dp_ctx.world)
        val = rect_val_loader(va, vs, batch, imgsz, channels, **kw) if val_rect else DataLoader(va, sampler=vs, **kw)
        return DataLoader(tr, sampler=sampler, **kw), val, sampler
    if val_rect:
        return (DataLoader(tr, shuffle=True, **kw),
                rect_val_loader(va, range(len(va)), batch, imgsz, channels, **kw), None)
    return DataLoader(tr, shuffle=True, **kw), DataLoader(va, shuffle=False, **kw), None


def rect_val_loader(va, inner, batch, imgsz, channels=1, **kw):
    """The --val-rect loader over the Subset `va`: the indices of `inner` (range(len(va)), or a rank's ValShard)
    walked by aspect ratio, every batch letterboxed into its own minimal stride-multiple frame.  `kw`: further
    DataLoader arguments."""
    import functools
    from torch.utils.data import DataLoader
    col = functools.partial(collate_fn, img_size=imgsz, channels=channels, letterbox=True, rect=True)
    return DataLoader(va, sampler=_rect_sampler(va, inner), **dict(kw, batch_size=batch, collate_fn=col))


def _rect_sampler(subset, inner):
    """`inner` (indices into the val Subset) ordered by the images' h0 / w0 when the dataset can tell the sizes
    without decoding (image_hw); otherwise as it is: the per-batch frame still applies."""
    from datasets import RectSampler
    ds = subset.dataset
    if not hasattr(ds, "image_hw"):
        return inner
    ratios = []
    for i in subset.indices:
        h0, w0 = ds.image_hw(i)
        ratios.append(h0 / max(w0, 1))
    return RectSampler(inner, ratios)


class _SyntheticLoader:
    def __init__(self, n, batch, imgsz, seed, ch=1, nc=5):
        from datasets.synthetic import synth_batch
        self._mk = lambda i: synth_batch(batch, imgsz, seed + i, nc=nc, ch=ch)
        self.n = n

    def __len__(self):
        return self.n

    def __iter__(self):
        for i in range(self.n):
            yield self._mk(i)


class _Parser(argparse.ArgumentParser):
    """Checks the combinations of flags argparse cannot express."""

    def parse_known_args(self, args=None, namespace=None):
        ns, rest = super().parse_known_args(args, namespace)
        if ns.val_nms_per_class and not ns.val_per_class:
            self.error("--val-nms-per-class needs --val-per-class (only the class-aware evaluation decodes class "
                       "labels)")
        if ns.val_max_det < 0 or (ns.val_max_det and not ns.val_nms_per_class):
            self.error("--val-max-det N needs N >= 0 and --val-nms-per-class")
        if ns.data_format == "crater" and ns.ch != 1:
            self.error("--data-format crater reads single-plane images: --ch must be 1 (colour data: --data-format "
                       "yolo)")
        if ns.data_format == "yolo" and ns.ch not in (1, 3, 4):
            self.error("--data-format yolo decodes to 1 (luma), 3 (RGB) or 4 (RGBA) planes")
        if ns.letterbox and ns.synthetic:
            self.error("--letterbox acts on a dataset's images: synthetic batches are generated at --imgsz")
        if ns.val_rect and ns.synthetic:
            self.error("--val-rect acts on a dataset's images: synthetic batches are generated at --imgsz")
        if ns.val_rect and ns.imgsz % 32:
            self.error("--val-rect needs --imgsz to be a multiple of the 32-pixel stride")
        if not 1 <= ns.ch <= 4 or ns.nc < 1:
            self.error("--ch is 1..4 and --nc at least 1")
        return ns, rest


def build_model(cfg, scale, ch, nc, device):
    """The model of a yaml file at one scale, on the device (main's and predict.py's builder)."""
    import yaml
    with open(cfg) as f:
        cfg_dict = yaml.safe_load(f)
    cfg_dict["scale"] = scale
    return build_yolo11(cfg=cfg_dict, ch=ch, nc=nc).to(device)


def build_parser():
    ap = _Parser(description="Train YOLOv11 for Crater Detection (MI355X)")
    ap.add_argument("--data", type=str, default="/content/data/train")
    ap.add_argument("--cfg", type=str, default=str(Path(__file__).parent / "configs" / "yolo11n_crater.yaml"))
    ap.add_argument("--scale", type=str, default="s", choices=["n", "s", "m", "l", "x"])
    ap.add_argument("--epochs", type=int, default=150)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--device", type=str, default="cuda")
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--lr", type=float, default=0.001)
    ap.add_argument("--weight-decay", type=float, default=0.0005)
    ap.add_argument("--val-split", type=float, default=0.2)
    ap.add_argument("--save-dir", type=str, default="/content/drive/MyDrive/YOLO11_crater_cuda")
    ap.add_argument("--resume", type=str, default="/content/drive/MyDrive/YOLO11_crater_cuda/last.pt")
    ap.add_argument("--max-val-batches", type=int, default=None)
    ap.add_argument("--val-conf", type=float, default=0.25)
    ap.add_argument("--synthetic", type=int, default=0, help="train on N synthetic batches (no dataset needed)")
    ap.add_argument("--data-format", type=str, default="crater", choices=["crater", "yolo"],
                    help="crater: the CSV + grayscale crater layout; yolo: images/ + labels/<stem>.txt with rows "
                         "`cls cx cy w h` normalised (datasets/yolo_txt.py)")
    ap.add_argument("--ch", type=int, default=1, help="image planes: 1 (luma), 3 (RGB) or 4 (RGBA); crater data is 1")
    ap.add_argument("--nc", type=int, default=5, help="number of classes")
    ap.add_argument("--augment", action="store_true", help="GPU training augmentation (datasets/augment.py)")
    ap.add_argument("--mosaic", type=float, default=1.0, help="probability of a 4-tile mosaic")
    ap.add_argument("--degrees", type=float, default=0.0, help="rotation range (+/- degrees)")
    ap.add_argument("--translate", type=float, default=0.1, help="translation range (+/- fraction of the image)")
    ap.add_argument("--aug-scale", type=float, default=0.5, help="scale range (+/- gain); Ultralytics' `scale`, "
                    "renamed because --scale selects the model size")
    ap.add_argument("--shear", type=float, default=0.0, help="shear range (+/- degrees)")
    ap.add_argument("--fliplr", type=float, default=0.5, help="probability of a left-right flip")
    ap.add_argument("--flipud", type=float, default=0.0, help="probability of an up-down flip")
    ap.add_argument("--gain", type=float, default=0.4, help="value gain range (+/- fraction; Ultralytics' hsv_v)")
    ap.add_argument("--hsv-h", type=float, default=0.015, help="hue shift range (+/- fraction of a turn); used with "
                    "--augment on 3-plane data only")
    ap.add_argument("--hsv-s", type=float, default=0.7, help="saturation factor range (+/- fraction around 1); used "
                    "with --augment on 3-plane data only")
    ap.add_argument("--mixup", type=float, default=0.0, help="probability that an image is blended with a second "
                    "mosaic + affine sample of its batch (MixUp, ratio ~ Beta(32, 32)); used with --augment")
    ap.add_argument("--close-mosaic", type=int, default=10, help="no mosaic and no MixUp in the last N epochs")
    ap.add_argument("--aug-seed", type=int, default=0)
    ap.add_argument("--val-per-class", action="store_true",
                    help="class-aware validation metrics: per-class AP, mAP over the classes with GT")
    ap.add_argument("--val-nms-per-class", action="store_true",
                    help="class-aware NMS in validation (needs --val-per-class): a box is suppressed by boxes of its "
                         "own class only")
    ap.add_argument("--val-max-det", type=int, default=0,
                    help="keep at most N boxes per image after the class-aware NMS (0: no cap)")
    ap.add_argument("--ema", action="store_true",
                    help="keep an exponential moving average of the weights (yolomi/ema.py): validated and "
                         "checkpointed as ema_state_dict")
    ap.add_argument("--ema-decay", type=float, default=0.9999, help="EMA decay once warmed up")
    ap.add_argument("--ema-tau", type=float, default=2000, help="EMA warm-up: decay * (1 - exp(-updates / tau))")
    ap.add_argument("--assigner", type=str, default="inbox", choices=["inbox", "topk"],
                    help="inbox: the reference's assignment (every in-box anchor a positive); topk: the standard "
                         "top-k task-aligned assignment with k = --tal-topk")
    ap.add_argument("--tal-topk", type=int, default=10, help="k of --assigner topk (1..64); unused with inbox")
    ap.add_argument("--letterbox", action="store_true",
                    help="keep the images' aspect ratio in the train and val loaders (resize + centred pad on the GPU, "
                         "datasets/letterbox.py) instead of stretching them to --imgsz; metrics stay in that frame")
    ap.add_argument("--val-rect", action="store_true",
                    help="validate on rectangular frames: each val batch is letterboxed into its own minimal "
                         "multiple-of-32 frame and the val set is walked by aspect ratio (DESIGN §23); the train "
                         "loader is unchanged")
    return ap


def main():
    args = build_parser().parse_args()

    from yolomi import dist as ydist
    dp_ctx = ydist.init_from_env()
    if not torch.cuda.is_available():
        raise SystemExit("yolomi runs on MI355X GPUs only (no CPU fallback)")
    device = torch.device("cuda", dp_ctx.local_rank if dp_ctx else 0)
    torch.cuda.set_device(device)
    rank0 = dp_ctx is None or dp_ctx.rank == 0
    save_dir = Path(args.save_dir)
    if rank0:
        save_dir.mkdir(parents=True, exist_ok=True)

    if args.synthetic:
        seed = 1000 * (dp_ctx.rank if dp_ctx else 0)
        train_loader = _SyntheticLoader(args.synthetic, args.batch, args.imgsz, seed, args.ch, args.nc)
        val_loader = _SyntheticLoader(max(1, args.synthetic // 5), args.batch, args.imgsz, seed + 10 ** 6, args.ch,
                                      args.nc)
        train_sampler = None
    else:
        if args.data_format == "yolo":
            from datasets import YoloTxtDataset
            dataset = YoloTxtDataset(args.data, img_size=args.imgsz, channels=args.ch, cache_images=False)
        else:
            from datasets import CraterDatasetCUDA
            dataset = CraterDatasetCUDA(args.data, img_size=args.imgsz, cache_images=False, augment=True)
        train_loader, val_loader, train_sampler = make_loaders(dataset, args.val_split, args.batch, args.workers,
                                                               args.imgsz, dp_ctx, channels=args.ch,
                                                               letterbox=args.letterbox, val_rect=args.val_rect)

    model = build_model(args.cfg, args.scale, args.ch, args.nc, device)
    if rank0:
        n_params = sum(p.numel() for p in model.parameters())
        print(f"Total parameters: {n_params:,} ({n_params / 1e6:.2f}M)")
        print(f"Assigner: {args.assigner}, tal_topk: {args.tal_topk}")
    criterion = v8DetectionLoss(model, tal_topk=args.tal_topk, assigner=args.assigner)
    # the reference's AdamW (:440-451) + clip_grad_norm_(10) (:58-62): on the GPU as yolomi's
    # FusedAdamW (a torch.optim.AdamW with the same state_dict; clipping fused into its step)
    if device.type == "cuda":
        from yolomi.optim import FusedAdamW
        optimizer = FusedAdamW(model.parameters(), lr=args.lr, weight_decay=args.weight_decay, max_grad_norm=10.0)
    else:
        optimizer = torch.optim.AdamW(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    dp = ydist.GradSync(model, dp_ctx) if dp_ctx else None
    ema = None
    if args.ema:
        from yolomi.ema import ModelEMA
        ema = ModelEMA(model, decay=args.ema_decay, tau=args.ema_tau)
        if hasattr(optimizer, "attach_ema"):
            optimizer.attach_ema(ema)      # averaged inside the AdamW pass: no launch of its own per tensor
    start_epoch, best_loss, best_mAP50 = 0, float("inf"), 0.0
    if args.resume and os.path.isfile(args.resume):
        start_epoch, best_loss, best_mAP50 = resume_checkpoint(args.resume, model, optimizer, device, ema)
        if rank0:
            print(f"Resumed from epoch {start_epoch}, best_loss={best_loss:.4f}, best_mAP50={best_mAP50:.4f}")
    if dp:
        dp.broadcast_state()
        if ema is not None:                # every rank starts from rank 0's average, as from rank 0's weights
            ydist.broadcast_buffers(ema.ema, parameters=True)

    augment = None
    if args.augment:
        from datasets import AugmentHyp, BatchAugment
        hyp = AugmentHyp(mosaic=args.mosaic, degrees=args.degrees, translate=args.translate, scale=args.aug_scale,
                         shear=args.shear, fliplr=args.fliplr, flipud=args.flipud, gain=args.gain,
                         hsv_h=args.hsv_h if args.ch == 3 else 0.0, hsv_s=args.hsv_s if args.ch == 3 else 0.0,
                         mixup=args.mixup)
        # train_one_epoch counts epochs from 1: the last `close_mosaic` of them draw no mosaic
        augment = BatchAugment(hyp, seed=args.aug_seed, rank=dp_ctx.rank if dp_ctx else 0,
                               no_mosaic_from=args.epochs - args.close_mosaic + 1)

    for epoch in range(start_epoch, args.epochs):
        lr = cosine_lr_schedule(optimizer, epoch, args.epochs, lr_min=args.lr * 0.01, lr_max=args.lr, warmup_epochs=3)
        criterion.epoch = epoch
        if train_sampler is not None:
            train_sampler.set_epoch(epoch)
        tm = train_one_epoch(model, train_loader, optimizer, criterion, device, epoch + 1, args.epochs, dp,
                             augment, ema)
        if dp:
            dp.sync_buffers()          # rank 0's BN running statistics for validation and the checkpoint
            if ema is not None:
                ema.sync_buffers(dp)
        # with --ema the averaged weights are the ones validated (and so the ones best.pt is selected by)
        vm = validate(ema.refresh() if ema is not None else model, val_loader, criterion, device,
                      conf_threshold=args.val_conf, iou_threshold=0.45, max_batches=args.max_val_batches, dp=dp,
                      per_class=args.val_per_class, nms_per_class=args.val_nms_per_class, max_det=args.val_max_det,
                      max_frames=8 if args.val_rect else None)
        if not rank0:
            continue
        print(f"\nEpoch {epoch + 1}/{args.epochs} | LR: {lr:.6f}")
        print(f"  Train - Loss: {tm['loss']:.4f}, Box: {tm['box_loss']:.4f}, Cls: {tm['cls_loss']:.4f}, "
              f"DFL: {tm['dfl_loss']:.4f}")
        print(f"  Val   - Loss: {vm['loss']:.4f}, Box: {vm['box_loss']:.4f}, Cls: {vm['cls_loss']:.4f}, "
              f"DFL: {vm['dfl_loss']:.4f}")
        print(f"  Metrics - P: {vm.get('precision', 0.0):.4f}, R: {vm.get('recall', 0.0):.4f}, "
              f"mAP50: {vm.get('mAP50', 0.0):.4f}, mAP50-95: {vm.get('mAP50-95', 0.0):.4f}")
        if args.val_per_class:
            pc = vm["per_class"]
            for c, n in enumerate(pc["n_gt"]):
                if n > 0:                              # the present classes: the ones the means run over
                    tp, fp = pc["tp"][c], pc["fp"][c]
                    print(f"    class {c}: n_gt {n}, P: {tp / (tp + fp) if tp + fp else 0.0:.4f}, R: {tp / n:.4f}, "
                          f"AP50: {pc['ap50'][c]:.4f}, AP50-95: {pc['ap'][c]:.4f}")
        ckpt = make_checkpoint(epoch, model, optimizer, tm, vm, best_loss, best_mAP50, ema)
        torch.save(ckpt, save_dir / "last.pt")
        if "mAP50" in vm:
            if vm["mAP50"] > best_mAP50:
                best_mAP50 = vm["mAP50"]
                ckpt["best_mAP50"] = best_mAP50
                torch.save(ckpt, save_dir / "best.pt")
        elif vm["loss"] < best_loss:
            best_loss = vm["loss"]
            ckpt["best_loss"] = best_loss
            torch.save(ckpt, save_dir / "best.pt")
    if dp_ctx:
        ydist.shutdown()


if __name__ == "__main__":
    main()
