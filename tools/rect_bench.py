"""Predictor with rectangular frames (rect=True) against the square Predictor of the same build on the same
sources, in one process: HIP events on the launch stream, warm-up, then `--windows` alternating windows
of `--reps` rounds per variant; the figure is the median window's time per round (tools/letterbox_bench.py's
method).  The model is the `--scale` network with random weights, `--ch` planes.  Two source sets, each at every
`--batches` size: 16:9 (`--src-h` x `--src-w`, frame 384 x 640 at imgsz 640: 0.6 of the square's pixels) and square
(`--square` = 1024: frame 640 x 640, both paths issue the same launches).  Three figures per variant:
  predict   the whole call: pack, pin, H2D, letterbox, forward, decode + NMS, unletterbox, the one host sync
  device    the same chain from packed sources already resident on the device (no pack, pin or H2D of images)
  forward   the eval forward alone on a resident batch of the frame's shape (the work the frame rule saves)
Writes one JSON object to `--out` and prints it; `--commit` is echoed into it.

usage: python tools/rect_bench.py [--imgsz 640 --scale s --ch 3 --batches 1 8 --out FILE]
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


def windows(variants, reps, n_windows, warmup, dev):
    """{name: [us per round of each window]}; the variants alternate inside every window."""
    st = torch.cuda.current_stream(dev)
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(n_windows):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(reps):
                fn()
            e1.record(st)
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps * 1e3)
    return times


def device_chain(pred, ims, frame):
    """Predictor._run's device steps over sources packed and moved once: letterbox, forward, decode + NMS (its one
    sync), unletterbox."""
    from datasets.crater import pack_images
    from datasets.letterbox import lb_table, letterbox_batch, table_bytes, unletterbox
    from yolomi import post
    H, W = frame or (pred.imgsz, pred.imgsz)
    packed = pack_images([pred._raw(im) for im in ims], pred.imgsz, pred.ch)
    table = table_bytes(lb_table(packed["img_meta"], H, W), len(ims)).to(pred.device)
    u8, meta = packed["img_u8"].to(pred.device), packed["img_meta"].to(pred.device)

    @torch.no_grad()
    def run():
        img = letterbox_batch(u8, meta, table, H, W, pred.ch, pred.fill)
        y = pred.model(img)[0]
        dets = post.decode_nms(y.transpose(1, 2), pred.imgsz if frame is None else (H, W), pred.conf, pred.iou,
                               class_aware=True, max_det=pred.max_det, padded=True)
        return unletterbox(dets, table, H, W)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--scale", default="s")
    ap.add_argument("--ch", type=int, default=3)
    ap.add_argument("--nc", type=int, default=80)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--src-h", type=int, default=1080)
    ap.add_argument("--src-w", type=int, default=1920)
    ap.add_argument("--square", type=int, default=1024)
    ap.add_argument("--conf", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rect" / "rect_bench.json"))
    args = ap.parse_args()
    import train_yolo11_cuda as T
    from yolomi.predict import Predictor

    assert torch.cuda.is_available(), "rect_bench needs the MI355X"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cfg = str(ROOT / "yolo-scratch_amd" / "configs" / "yolo11n_crater.yaml")
    model = T.build_model(cfg, args.scale, args.ch, args.nc, dev).eval()
    rng = np.random.default_rng(0)
    rows = []
    for B in args.batches:
        for name, (h, w) in (("16x9", (args.src_h, args.src_w)), ("square", (args.square, args.square))):
            ims = [rng.integers(0, 256, (h, w, args.ch), dtype=np.uint8) for _ in range(B)]
            kw = dict(imgsz=args.imgsz, ch=args.ch, conf=args.conf, batch=B, device=dev)
            sq, rc = Predictor(model, **kw), Predictor(model, rect=True, **kw)
            frame = rc.frame_of(ims[0])
            a, b = sq(ims), rc(ims)
            if frame == (args.imgsz, args.imgsz):          # the same launches: the same answer
                for x, y in zip(a, b):
                    assert all(torch.equal(x[k], y[k]) for k in x)
            kept = [sum(len(d["scores"]) for d in o) / B for o in (a, b)]
            t = windows({"square": lambda: sq(ims), "rect": lambda: rc(ims)}, args.reps, args.windows, args.warmup,
                        dev)
            d = windows({"square": device_chain(sq, ims, None), "rect": device_chain(rc, ims, frame)}, args.reps,
                        args.windows, args.warmup, dev)
            xs = torch.rand(B, args.ch, args.imgsz, args.imgsz, device=dev)
            xr = torch.rand(B, args.ch, *frame, device=dev)
            with torch.no_grad():
                f = windows({"square": lambda: model(xs), "rect": lambda: model(xr)}, args.reps, args.windows,
                            args.warmup, dev)
            row = {"batch": B, "sources": name, "src": [h, w], "frame": list(frame),
                   "pixel_ratio": round(frame[0] * frame[1] / args.imgsz ** 2, 3), "kept_per_image": kept}
            for part, tt in (("predict", t), ("device", d), ("forward", f)):
                med = {k: statistics.median(v) for k, v in tt.items()}
                row[part] = {"us_per_round": {k: round(v, 1) for k, v in med.items()},
                             "us_min_max": {k: [round(min(v), 1), round(max(v), 1)] for k, v in tt.items()},
                             "spread": {k: round((max(v) - min(v)) / med[k], 3) for k, v in tt.items()},
                             "rect_over_square": round(med["rect"] / med["square"], 3)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    res = {"bench": "rect", "commit": args.commit, "device": torch.cuda.get_device_name(0), "imgsz": args.imgsz,
           "scale": args.scale, "ch": args.ch, "nc": args.nc, "conf": args.conf, "reps": args.reps,
           "windows": args.windows, "warmup": args.warmup, "rows": rows,
           "rect_faster_on_16x9": {part: all(r[part]["rect_over_square"] < 1.0 for r in rows if r["sources"] == "16x9")
                                   for part in ("predict", "device", "forward")}}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
