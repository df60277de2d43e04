"""Sliced inference (Predictor(slice=TILE)) against the hand composition it replaces, on the same sources
in one process: HIP events on the launch stream, warm-up, then `--windows` alternating windows of `--reps` rounds per
variant; the figure is the median window's time per round (tools/rect_bench.py's method).  The hand composition: the
windows of the same plan cropped on the host and run through the plain Predictor (pack, pin, upload, letterbox,
forward, decode + NMS per tile, unletterbox), the boxes shifted by the window's origin in torch, one ym_nms_cls per
source image.  The model is the `--scale` network with random weights, `--ch` planes.  Four figures per variant, at
every `--sources` count of `--src-h` x `--src-w` images (random weights score every anchor alike, so `conf` is set
to the score quantile that makes `--cand-share` of the anchors candidates, the same value for both variants):
  predict   the whole call from host images to merged boxes
  device    the same chain from sources (hand: crops) packed and resident on the device: no pack, pin or upload
  slice     the tiles alone: ym_slice_letterbox_u8c over the resident sources / ym_letterbox_u8c over the resident crops
  merge     the boxes alone, from a resident forward output: ym_decode_nms_tiles / decode + NMS per tile, unletterbox,
            shift, ym_nms_cls per image
Writes one JSON object to `--out` and prints it; `--commit` is echoed into it.

usage: python tools/slice_bench.py [--tile 640 --scale s --ch 3 --sources 1 8 --out FILE]
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
    """The composition by hand over the plan's windows (the whole-image pass included, as one more crop)."""

    def __init__(self, plain, ims, tile, overlap, full):
        from datasets.slicing import tile_table
        self.p, self.ims = plain, ims
        self.table, self.begin = tile_table([im.shape[:2] for im in ims], tile, overlap, plain.imgsz, full)
        self.T = self.begin[-1]
        self.origin = torch.tensor([[e.x0, e.y0, e.x0, e.y0] for e in list(self.table)[:self.T]],
                                   dtype=torch.float32, device=plain.device)

    def crops(self):
        return [self.ims[e.src][e.y0:e.y0 + e.th, e.x0:e.x0 + e.tw] for e in list(self.table)[:self.T]]

    def merge(self, dets):
        """Per-tile detections in window pixels -> per source image, shifted and suppressed once more."""
        from yolomi import post
        out = []
        for g in range(len(self.ims)):
            lo, hi = self.begin[g], self.begin[g + 1]
            boxes = torch.cat([d["boxes"] + self.origin[t] for t, d in zip(range(lo, hi), dets[lo:hi])])
            scores = torch.cat([d["scores"] for d in dets[lo:hi]])
            labels = torch.cat([d["labels"] for d in dets[lo:hi]])
            keep = post.nms(boxes, scores, self.p.iou, labels=labels, max_det=self.p.max_det)
            out.append({"boxes": boxes[keep], "scores": scores[keep], "labels": labels[keep]})
        return out

    def predict(self):
        return self.merge(self.p(self.crops()))

    def resident(self):
        """(device, slice, merge) closures over crops packed and uploaded once."""
        from datasets.crater import pack_images
        from datasets.letterbox import lb_table, letterbox_batch, table_bytes, unletterbox
        from yolomi import post
        p, S, nb = self.p, self.p.imgsz, self.p.batch
        empty = torch.empty((1, 0, 0) if p.ch == 1 else (0, 0, p.ch), dtype=torch.uint8)
        chunks = []
        raw = [p._raw(np.ascontiguousarray(c)) for c in self.crops()]
        for lo in range(0, self.T, nb):
            part = raw[lo:lo + nb]
            packed = pack_images(part + [empty] * (nb - len(part)), S, p.ch)
            table = table_bytes(lb_table(packed["img_meta"], S, S), nb).to(p.device)
            chunks.append((packed["img_u8"].to(p.device), packed["img_meta"].to(p.device), table, len(part)))

        def tiles():
            return [letterbox_batch(u8, meta, table, S, S, p.ch, p.fill) for u8, meta, table, _ in chunks]

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
        return (lambda: boxes(forward())), tiles, (lambda: boxes(ys))


def sliced_resident(pred, ims):
    """(device, slice, merge) closures of Predictor._run_sliced's device steps over sources uploaded once."""
    from datasets.crater import pack_images
    from datasets.slicing import slice_batch, tile_bytes, tile_table
    from yolomi import post
    S, nb = pred.imgsz, pred.batch
    packed = pack_images([pred._raw(im) for im in ims], S, pred.ch)
    table, begin = tile_table(packed["img_meta"][:, 1:].tolist(), pred.slice, pred.slice_overlap, S, pred.slice_full)
    T = begin[-1]
    Tp = -(-T // nb) * nb
    tdev = tile_bytes(table, T, Tp).to(pred.device)
    u8, meta = packed["img_u8"].to(pred.device), packed["img_meta"].to(pred.device)

    def tiles():
        return [slice_batch(u8, meta, tdev, nb, S, S, pred.ch, pred.fill, first=lo) for lo in range(0, Tp, nb)]

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
                                     max_det=pred.max_det, edge=pred.slice_edge)

    ybuf = forward()
    return (lambda: boxes(forward())), tiles, (lambda: boxes(ybuf)), T, ybuf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--tile", type=int, default=640)
    ap.add_argument("--overlap", type=float, default=0.2)
    ap.add_argument("--no-full", dest="full", action="store_false")
    ap.add_argument("--scale", default="s")
    ap.add_argument("--ch", type=int, default=3)
    ap.add_argument("--nc", type=int, default=80)
    ap.add_argument("--batch", type=int, default=8, help="tiles per forward")
    ap.add_argument("--sources", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--src-h", type=int, default=2160)
    ap.add_argument("--src-w", type=int, default=3840)
    ap.add_argument("--conf", type=float, default=0.25)
    ap.add_argument("--cand-share", type=float, default=0.01,
                    help="set conf to the score quantile that makes this share of the anchors candidates (0: --conf)")
    ap.add_argument("--reps", type=int, default=8, help="rounds per window with one source; divided by the sources")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "slice" / "slice_bench.json"))
    args = ap.parse_args()
    import train_yolo11_cuda as T
    from yolomi.predict import Predictor

    assert torch.cuda.is_available(), "slice_bench needs the MI355X"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cfg = str(ROOT / "yolo-scratch_amd" / "configs" / "yolo11n_crater.yaml")
    model = T.build_model(cfg, args.scale, args.ch, args.nc, dev).eval()
    rng = np.random.default_rng(0)
    rows = []
    for n_src in args.sources:
        ims = [rng.integers(0, 256, (args.src_h, args.src_w, args.ch), dtype=np.uint8) for _ in range(n_src)]
        kw = dict(imgsz=args.imgsz, ch=args.ch, conf=args.conf, batch=args.batch, device=dev)
        sl = Predictor(model, slice=args.tile, slice_overlap=args.overlap, slice_full=args.full, **kw)
        hand = Hand(Predictor(model, **kw), ims, args.tile, args.overlap, args.full)
        h_dev, h_tiles, h_merge = hand.resident()
        s_dev, s_tiles, s_merge, n_tiles, ybuf = sliced_resident(sl, ims)
        conf = args.conf
        if args.cand_share > 0:                            # random weights score every anchor alike: a quantile
            best = ybuf[:n_tiles, 4:].amax(1).flatten()
            conf = float(best.kthvalue(max(1, round(best.numel() * (1.0 - args.cand_share)))).values)
            sl.conf = hand.p.conf = conf
        kept = [sum(len(d["scores"]) for d in o) / n_src for o in (hand.predict(), sl(ims))]
        reps = max(1, args.reps // n_src)
        parts = {"predict": {"hand": hand.predict, "sliced": lambda: sl(ims)},
                 "device": {"hand": h_dev, "sliced": s_dev},
                 "slice": {"hand": h_tiles, "sliced": s_tiles},
                 "merge": {"hand": h_merge, "sliced": s_merge}}
        row = {"sources": n_src, "src": [args.src_h, args.src_w], "tiles": n_tiles, "reps": reps, "conf": conf,
               "kept_per_image": kept}
        for part, variants in parts.items():
            tt = windows(variants, reps, args.windows, args.warmup, dev)
            med = {k: statistics.median(v) for k, v in tt.items()}
            spread = {k: (max(v) - min(v)) / med[k] for k, v in tt.items()}
            ratio = med["sliced"] / med["hand"]
            row[part] = {"us_per_round": {k: round(v, 1) for k, v in med.items()},
                         "us_min_max": {k: [round(min(v), 1), round(max(v), 1)] for k, v in tt.items()},
                         "spread": {k: round(v, 3) for k, v in spread.items()},
                         "sliced_over_hand": round(ratio, 3),
                         # the bar: faster by more than the windows' spread
                         "clears_the_bar": bool(max(tt["sliced"]) < min(tt["hand"]))}
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"bench": "slice", "commit": args.commit, "device": torch.cuda.get_device_name(0), "imgsz": args.imgsz,
           "tile": args.tile, "overlap": args.overlap, "full": args.full, "scale": args.scale, "ch": args.ch,
           "nc": args.nc, "cand_share": args.cand_share, "batch": args.batch, "windows": args.windows, "warmup": args.warmup,
           "rows": rows,
           "sliced_clears_the_bar": {part: all(r[part]["clears_the_bar"] for r in rows)
                                     for part in ("predict", "device", "slice", "merge")}}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
