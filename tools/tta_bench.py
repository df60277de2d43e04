"""Test-time augmentation (Predictor(tta=VIEWS)) against the hand composition it replaces, on the same
sources in one process: tools/slice_bench.py's method (HIP events on the launch stream, warm-up, `--windows`
alternating windows of `--reps` rounds per variant, the median window and the windows' spread).

The hand composition: per view a host flip / resize of every source (a plain view is the source itself; a mirrored one
is flipped in numpy; a reduced one is resized on the host to the view's size, flipped and pasted into the middle of an
imgsz x imgsz canvas of the fill value, which the plain path then copies), all views of all sources through the plain
Predictor (pack, pin, upload, letterbox, forward, decode + NMS per view, unletterbox), the boxes mapped back to source
pixels in torch (through the canvas's place and scale, then the mirror), one ym_nms_cls per source image.  The model
is the `--scale` network with random weights, `--ch` planes; random weights score every anchor alike, so `conf` is the
score quantile that makes `--cand-share` of the anchors candidates, the same value for both variants.

Three figures per variant at every `--sources` count of `--src-h` x `--src-w` images:
  predict   the whole call from host images to merged boxes (hand: the host flips and resizes included)
  device    the same chain from images packed and resident on the device: no host view, pack, pin or upload
  merge     the boxes alone from a resident forward output: one ym_decode_nms_tiles (and ym_decode_nmw_tiles, reported
            beside it) / decode + NMS per view, unletterbox, map back, ym_nms_cls per image
Writes one JSON object to `--out` and prints it; `--commit` is echoed into it.

usage: python tools/tta_bench.py [--views 1,0.83:lr,0.67 --scale s --ch 3 --sources 1 8 --out FILE]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "yolo-scratch_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rect_bench import windows  # noqa: E402


class Hand:
    """The composition by hand: views on the host, the plain Predictor, the way back in torch, one NMS per image."""

    def __init__(self, plain, ims, views):
        from datasets.tta import view_table
        self.p, self.ims, self.views = plain, ims, views
        self.table, self.begin = view_table([im.shape[:2] for im in ims], views, plain.imgsz)
        self.T = self.begin[-1]
        ents = list(self.table)[:self.T]
        f = lambda vals: torch.tensor(vals, dtype=torch.float32, device=plain.device)        # noqa: E731
        # reduced views are boxes in canvas pixels: (x - left) * sx clamped to the source; others are source pixels
        self.reduced = [(e.nw, e.nh) != self._lb(e) for e in ents]
        self.off = f([[e.left, e.top, e.left, e.top] for e in ents])
        self.mul = f([[e.sx, e.sy, e.sx, e.sy] for e in ents])
        self.lim = f([[e.tw, e.th, e.tw, e.th] for e in ents])
        self.mx = [bool(e.edges & 16) for e in ents]
        self.my = [bool(e.edges & 32) for e in ents]
        self.ents = ents

    def _lb(self, e):
        from datasets.letterbox import letterbox_geometry
        return tuple(letterbox_geometry(e.th, e.tw, self.p.imgsz, self.p.imgsz)[:2])

    def host_views(self):
        """One image per table entry, as the plain Predictor takes it."""
        from PIL import Image
        S, out = self.p.imgsz, []
        for e, red in zip(self.ents, self.reduced):
            im = self.ims[e.src]
            if red:
                small = np.asarray(Image.fromarray(im).resize((e.nw, e.nh), Image.BILINEAR))
                canvas = np.full((S, S, im.shape[2]), self.p.fill, np.uint8)
                canvas[e.top:e.top + e.nh, e.left:e.left + e.nw] = small
                im = canvas
                lo_x, hi_x, lo_y, hi_y = e.left, e.left + e.nw, e.top, e.top + e.nh
            else:
                lo_x, hi_x, lo_y, hi_y = 0, im.shape[1], 0, im.shape[0]
            if e.edges & 16:
                im = im.copy()
                im[lo_y:hi_y, lo_x:hi_x] = im[lo_y:hi_y, lo_x:hi_x][:, ::-1]
            if e.edges & 32:
                im = im.copy()
                im[lo_y:hi_y, lo_x:hi_x] = im[lo_y:hi_y, lo_x:hi_x][::-1]
            out.append(np.ascontiguousarray(im))
        return out

    def merge(self, dets):
        """Per-view detections -> per source image: back to source pixels, back through the mirror, one NMS."""
        from yolomi import post
        out = []
        for g in range(len(self.ims)):
            bx = []
            for t in range(self.begin[g], self.begin[g + 1]):
                b = dets[t]["boxes"]
                if self.reduced[t]:
                    b = torch.minimum(((b - self.off[t]) * self.mul[t]).clamp_min(0.0), self.lim[t])
                if self.mx[t]:
                    b = torch.stack([self.lim[t][0] - b[:, 2], b[:, 1], self.lim[t][0] - b[:, 0], b[:, 3]], 1)
                if self.my[t]:
                    b = torch.stack([b[:, 0], self.lim[t][1] - b[:, 3], b[:, 2], self.lim[t][1] - b[:, 1]], 1)
                bx.append(b)
            lo, hi = self.begin[g], self.begin[g + 1]
            boxes = torch.cat(bx)
            scores = torch.cat([d["scores"] for d in dets[lo:hi]])
            labels = torch.cat([d["labels"] for d in dets[lo:hi]])
            keep = post.nms(boxes, scores, self.p.iou, labels=labels, max_det=self.p.max_det)
            out.append({"boxes": boxes[keep], "scores": scores[keep], "labels": labels[keep]})
        return out

    def predict(self):
        return self.merge(self.p(self.host_views()))

    def resident(self):
        """(device, merge) closures over the views' images packed and uploaded once."""
        from datasets.crater import pack_images
        from datasets.letterbox import lb_table, letterbox_batch, table_bytes, unletterbox
        from yolomi import post
        p, S, nb = self.p, self.p.imgsz, self.p.batch
        empty = torch.empty((1, 0, 0) if p.ch == 1 else (0, 0, p.ch), dtype=torch.uint8)
        raw = [p._raw(v) for v in self.host_views()]
        chunks = []
        for lo in range(0, self.T, nb):
            part = raw[lo:lo + nb]
            packed = pack_images(part + [empty] * (nb - len(part)), S, p.ch)
            table = table_bytes(lb_table(packed["img_meta"], S, S), nb).to(p.device)
            chunks.append((packed["img_u8"].to(p.device), packed["img_meta"].to(p.device), table, len(part)))

        def boxes(ys):
            dets = []
            for y, (_, _, table, n) in zip(ys, chunks):
                d = post.decode_nms(y.transpose(1, 2), S, p.conf, p.iou, class_aware=True, max_det=p.max_det,
                                    padded=True)
                dets += unletterbox(d, table, S, S)[:n]
            return self.merge(dets)

        @torch.no_grad()
        def forward():
            return [p.model(letterbox_batch(u8, meta, table, S, S, p.ch, p.fill))[0].clone()
                    for u8, meta, table, _ in chunks]

        ys = forward()
        return (lambda: boxes(forward())), (lambda: boxes(ys))


def tta_resident(pred, ims):
    """(device, merge, merge with the mean) closures of the predictor's device steps over sources uploaded once."""
    from datasets.crater import pack_images
    from datasets.slicing import slice_batch, tile_bytes
    from datasets.tta import view_table
    from yolomi import post
    S, nb = pred.imgsz, pred.batch
    packed = pack_images([pred._raw(im) for im in ims], S, pred.ch)
    table, begin = view_table(packed["img_meta"][:, 1:].tolist(), pred.views, S)
    T = begin[-1]
    Tp = -(-T // nb) * nb
    tdev = tile_bytes(table, T, Tp).to(pred.device)
    u8, meta = packed["img_u8"].to(pred.device), packed["img_meta"].to(pred.device)

    @torch.no_grad()
    def forward():
        ybuf = None
        for lo in range(0, Tp, nb):
            y = pred.model(slice_batch(u8, meta, tdev, nb, S, S, pred.ch, pred.fill, first=lo))[0]
            if ybuf is None:
                ybuf = torch.empty(Tp, *y.shape[1:], dtype=y.dtype, device=y.device)
            ybuf[lo:lo + nb].copy_(y)
        return ybuf

    def boxes(ybuf):
        return post.decode_nms_tiles(ybuf[:T].transpose(1, 2), tdev, begin, pred.conf, pred.iou, class_aware=True,
                                     max_det=pred.max_det)

    def mean(ybuf):
        return post.decode_nmw_tiles(ybuf[:T].transpose(1, 2), tdev, begin, pred.conf, pred.iou, class_aware=True,
                                     max_det=pred.max_det)

    ybuf = forward()
    return (lambda: boxes(forward())), (lambda: boxes(ybuf)), (lambda: mean(ybuf)), T, ybuf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--views", default="1,0.83:lr,0.67")
    ap.add_argument("--scale", default="s")
    ap.add_argument("--ch", type=int, default=3)
    ap.add_argument("--nc", type=int, default=80)
    ap.add_argument("--batch", type=int, default=8, help="views per forward")
    ap.add_argument("--sources", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--src-h", type=int, default=1080)
    ap.add_argument("--src-w", type=int, default=1920)
    ap.add_argument("--conf", type=float, default=0.25)
    ap.add_argument("--cand-share", type=float, default=0.01,
                    help="set conf to the score quantile that makes this share of the anchors candidates (0: --conf)")
    ap.add_argument("--reps", type=int, default=8, help="rounds per window with one source; divided by the sources")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tta" / "tta_bench.json"))
    args = ap.parse_args()
    import train_yolo11_cuda as T
    from datasets.tta import parse_views
    from yolomi.predict import Predictor

    assert torch.cuda.is_available(), "tta_bench needs the MI355X"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cfg = str(ROOT / "yolo-scratch_amd" / "configs" / "yolo11n_crater.yaml")
    model = T.build_model(cfg, args.scale, args.ch, args.nc, dev).eval()
    views = parse_views(args.views)
    rng = np.random.default_rng(0)
    rows = []
    for n_src in args.sources:
        ims = [rng.integers(0, 256, (args.src_h, args.src_w, args.ch), dtype=np.uint8) for _ in range(n_src)]
        kw = dict(imgsz=args.imgsz, ch=args.ch, conf=args.conf, batch=args.batch, device=dev)
        tta = Predictor(model, tta=views, **kw)
        hand = Hand(Predictor(model, **kw), ims, views)
        t_dev, t_merge, t_mean, n_views, ybuf = tta_resident(tta, ims)
        h_dev, h_merge = hand.resident()
        conf = args.conf
        if args.cand_share > 0:
            best = ybuf[:n_views, 4:].amax(1).flatten()
            conf = float(best.kthvalue(max(1, round(best.numel() * (1.0 - args.cand_share)))).values)
            tta.conf = hand.p.conf = conf
        kept = [sum(len(d["scores"]) for d in o) / n_src for o in (hand.predict(), tta(ims))]
        reps = max(1, args.reps // n_src)
        parts = {"predict": {"hand": hand.predict, "tta": lambda: tta(ims)},
                 "device": {"hand": h_dev, "tta": t_dev},
                 "merge": {"hand": h_merge, "tta": t_merge, "tta_mean": t_mean}}
        row = {"sources": n_src, "src": [args.src_h, args.src_w], "views": n_views, "reps": reps, "conf": conf,
               "kept_per_image": kept}
        for part, variants in parts.items():
            tt = windows(variants, reps, args.windows, args.warmup, dev)
            med = {k: statistics.median(v) for k, v in tt.items()}
            row[part] = {"us_per_round": {k: round(v, 1) for k, v in med.items()},
                         "us_min_max": {k: [round(min(v), 1), round(max(v), 1)] for k, v in tt.items()},
                         "spread": {k: round((max(v) - min(v)) / med[k], 3) for k, v in tt.items()},
                         "tta_over_hand": round(med["tta"] / med["hand"], 3),
                         # the bar: the slowest TTA window is faster than the fastest hand window
                         "clears_the_bar": bool(max(tt["tta"]) < min(tt["hand"]))}
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"bench": "tta", "commit": args.commit, "device": torch.cuda.get_device_name(0), "imgsz": args.imgsz,
           "views": args.views, "scale": args.scale, "ch": args.ch, "nc": args.nc, "cand_share": args.cand_share,
           "batch": args.batch, "windows": args.windows, "warmup": args.warmup, "rows": rows,
           "tta_clears_the_bar": {part: all(r[part]["clears_the_bar"] for r in rows)
                                  for part in ("predict", "device", "merge")}}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
