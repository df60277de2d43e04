"""Run a trained YOLOv11 on image files (MI355X): boxes in each image's own pixels.

    python yolo-scratch_amd/predict.py --weights runs/best.pt --source photos/ --scale s --ch 3 --nc 80 --ema
    python yolo-scratch_amd/predict.py --weights runs/best.pt --source video_frames/ --ch 3 --nc 80 --rect
    python yolo-scratch_amd/predict.py --weights runs/best.pt --source orbital_frames/ --slice 640 --slice-edge 4
    python yolo-scratch_amd/predict.py --weights runs/best.pt --source orbital_frames/ --slice 640 --slice-merge nmm \
        --slice-metric ios
    python yolo-scratch_amd/predict.py --weights runs/best.pt --source photos/ --ch 3 --nc 80 --tta --slice-merge mean
    python yolo-scratch_amd/predict.py --weights runs/best.pt --source photos/ --tta-views 1,0.83:lr,0.67:ud

Per image `<save-dir>/<stem>.txt` with rows `cls cx cy w h conf` normalised to the source image (the label format of
datasets/yolo_txt.py plus the confidence), and one `<save-dir>/predictions.json` with the pixel boxes.  The images
are decoded on the host, letterboxed on the GPU, and everything up to the source-pixel boxes stays there
(yolomi/predict.py); the model is built and the checkpoint loaded as the trainer does it.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).parent))

import train_yolo11_cuda as T  # noqa: E402
from datasets.yolo_txt import IMG_EXTS  # noqa: E402
from yolomi.predict import Predictor  # noqa: E402


def build_parser():
    ap = argparse.ArgumentParser(description="YOLOv11 inference on image files (MI355X)")
    ap.add_argument("--weights", type=str, required=True, help="last.pt / best.pt written by train_yolo11_cuda.py")
    ap.add_argument("--source", type=str, required=True, help="an image file, or a directory searched recursively")
    ap.add_argument("--cfg", type=str, default=str(Path(__file__).parent / "configs" / "yolo11n_crater.yaml"))
    ap.add_argument("--scale", type=str, default="s", choices=["n", "s", "m", "l", "x"])
    ap.add_argument("--ch", type=int, default=1, choices=[1, 3, 4], help="image planes: 1 (luma), 3 (RGB) or 4 (RGBA)")
    ap.add_argument("--nc", type=int, default=5, help="number of classes")
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--batch", type=int, default=8, help="images per forward; the last batch is padded to it")
    ap.add_argument("--conf", type=float, default=0.25)
    ap.add_argument("--iou", type=float, default=0.45)
    ap.add_argument("--max-det", type=int, default=300, help="boxes kept per image (0: no cap)")
    ap.add_argument("--ema", action="store_true", help="load the averaged weights (ema_state_dict) when present")
    ap.add_argument("--rect", action="store_true",
                    help="run each image in its minimal multiple-of-32 frame instead of the --imgsz square (--imgsz "
                         "must be a multiple of 32); the files are walked by aspect ratio so batches share a frame")
    ap.add_argument("--slice", type=int, default=0, metavar="TILE",
                    help="sliced inference: run the network on overlapping TILE x TILE windows at full resolution and "
                         "merge their boxes in one NMS per image (0: off; not with --rect)")
    ap.add_argument("--slice-overlap", type=float, default=0.2, help="share of a window's side that neighbours overlap")
    ap.add_argument("--no-slice-full", dest="slice_full", action="store_false",
                    help="skip the extra pass over the whole image (it sees objects larger than a window)")
    ap.add_argument("--slice-edge", type=float, default=0.0,
                    help="drop a window's boxes within this many pixels of a window side inside the image (0: none)")
    ap.add_argument("--slice-merge", type=str, default="nms", choices=["nms", "nmm", "mean"],
                    help="how the boxes of an image's windows and views are joined: nms suppresses what overlaps a kept "
                         "box, nmm merges it into the kept box, which becomes the union, mean merges it and the kept "
                         "box becomes the score-weighted mean, the merge for --tta (--iou is the match threshold)")
    ap.add_argument("--slice-metric", type=str, default="iou", choices=["iou", "ios"],
                    help="the overlap --iou is compared with: iou, or ios, the intersection over the smaller box, "
                         "which joins a box cut by a window border to its whole twin")
    ap.add_argument("--tta", action="store_true",
                    help="test-time augmentation: run every image (or window of --slice) at scales 1 / 0.83 / 0.67, the "
                         "middle view mirrored left-right, and join the views' boxes per image (not with --rect)")
    ap.add_argument("--tta-views", type=str, default=None, metavar="SPEC",
                    help="the views of --tta (which it implies): comma-separated scale[:flip], 0 < scale <= 1, flip lr, "
                         "ud or lrud, e.g. 1,0.83:lr,0.67")
    ap.add_argument("--save-dir", type=str, default="runs/predict")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.slice < 0:
        ap.error("--slice is a window size in pixels")
    if args.slice and args.rect:
        ap.error("--slice and --rect exclude each other")
    args.views = None
    if args.tta_views is not None:
        from datasets.tta import parse_views
        try:
            args.views = parse_views(args.tta_views)
        except ValueError as e:
            ap.error(f"--tta-views: {e}")
        args.tta = True
    elif args.tta:
        from datasets.tta import DEFAULT_VIEWS
        args.views = list(DEFAULT_VIEWS)
    if args.tta and args.rect:
        ap.error("--tta and --rect exclude each other")
    if (args.slice_merge, args.slice_metric) != ("nms", "iou") and not args.slice and not args.tta:
        ap.error("--slice-merge and --slice-metric need --slice or --tta")
    return args


def find_images(source):
    p = Path(source)
    if p.is_dir():
        return sorted(f for f in p.rglob("*") if f.is_file() and f.suffix.lower() in IMG_EXTS)
    if p.is_file():
        return [p]
    raise FileNotFoundError(f"--source {source}: no such file or directory")


def read_image(path, ch):
    """uint8 (h, w) for one plane (the crater loader's luma), (h, w, ch) otherwise, as the datasets decode."""
    if ch == 1:
        from datasets.crater import _gray_u8
        return _gray_u8(str(path))
    from PIL import Image
    with Image.open(path) as f:
        return np.array(f.convert({3: "RGB", 4: "RGBA"}[ch]), dtype=np.uint8)


def header_ratio(path):
    """h0 / w0 from the file's header, without decoding the image."""
    from PIL import Image
    with Image.open(path) as f:
        w0, h0 = f.size
    return h0 / max(w0, 1)


def txt_rows(det, h0, w0):
    """`cls cx cy w h conf` rows, normalised to the h0 x w0 source image.  A label row has no negative size: a box
    whose corners come out in reverse is written by its extent; predictions.json keeps the corners as they are.
    (The trainer initialises the DFL conv weight at random like every conv's, as the reference does, and it is
    frozen: where its mean is negative, a barely trained head decodes negative distances.)"""
    rows = []
    for (x1, y1, x2, y2), s, c in zip(det["boxes"].tolist(), det["scores"].tolist(), det["labels"].tolist()):
        x1, x2, y1, y2 = min(x1, x2), max(x1, x2), min(y1, y2), max(y1, y2)
        rows.append(f"{int(c)} {(x1 + x2) / 2 / w0:.6f} {(y1 + y2) / 2 / h0:.6f} {(x2 - x1) / w0:.6f} "
                    f"{(y2 - y1) / h0:.6f} {s:.6f}")
    return rows


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("yolomi runs on MI355X GPUs only (no CPU fallback)")
    device = torch.device("cuda", 0)
    files = find_images(args.source)
    if not files:
        raise SystemExit(f"--source {args.source}: no images")
    model = T.build_model(args.cfg, args.scale, args.ch, args.nc, device)
    key = T.load_checkpoint(args.weights, model, device, ema=args.ema)
    print(f"Loaded {key} from {args.weights}")
    predictor = Predictor(model, imgsz=args.imgsz, ch=args.ch, conf=args.conf, iou=args.iou, max_det=args.max_det,
                          class_aware=True, device=device, batch=args.batch, rect=args.rect, slice=args.slice,
                          slice_overlap=args.slice_overlap, slice_full=args.slice_full, slice_edge=args.slice_edge,
                          slice_merge=args.slice_merge, slice_metric=args.slice_metric, tta=args.views)
    save_dir = Path(args.save_dir)
    save_dir.mkdir(parents=True, exist_ok=True)
    order = list(range(len(files)))
    if args.rect:
        order.sort(key=lambda i: header_ratio(files[i]))             # stable: neighbours share a frame
    results = [None] * len(files)
    for lo in range(0, len(order), args.batch):
        chunk = order[lo:lo + args.batch]
        images = [read_image(files[i], args.ch) for i in chunk]
        for i, im, det in zip(chunk, images, predictor(images)):
            f = files[i]
            det = {k: v.cpu() for k, v in det.items()}
            h0, w0 = im.shape[:2]
            (save_dir / f"{f.stem}.txt").write_text("".join(r + "\n" for r in txt_rows(det, h0, w0)))
            results[i] = {"image": str(f), "height": h0, "width": w0, "boxes": det["boxes"].tolist(),
                          "scores": det["scores"].tolist(), "labels": det["labels"].tolist()}
    (save_dir / "predictions.json").write_text(json.dumps({"weights": str(args.weights), "state": key,
                                                           "imgsz": args.imgsz, "conf": args.conf, "iou": args.iou,
                                                           "images": results}))
    print(f"{len(results)} images, {sum(len(r['scores']) for r in results)} boxes -> {save_dir}")


if __name__ == "__main__":
    main()
