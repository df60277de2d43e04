"""The letterbox launch (ym_letterbox_u8c) against the stretch launch (ym_resize_linear_u8c) of the same build on the
same sources, and the unletterbox launch (ym_unletterbox_boxes), in one process: HIP events on the launch stream,
warm-up, then `--windows` alternating windows of `--reps` rounds per variant; the figure is the median window's time
per round (tools/colour_bench.py's method).  Two source shapes: `--src-w` x `--src-h` (4:3: a quarter of the frame is
pad, so the letterbox samples 3/4 of the pixels) and square `--src-w` x `--src-w` (no pad: the two launches do the
same work, the letterbox with its table loads on top).  Writes one JSON object to `--out` and prints it; `--commit`
is echoed into it (the caller's `git rev-parse --short HEAD`).

usage: python tools/letterbox_bench.py [--batch 64 --size 640 --ch 3 --src-w 1024 --src-h 768 --out FILE]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "yolo-scratch_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402

HBM_TBPS = 6.3          # achievable HBM bandwidth of the MI355X (8 TB/s peak), for the write floor only


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--ch", type=int, default=3)
    ap.add_argument("--src-w", type=int, default=1024)
    ap.add_argument("--src-h", type=int, default=768)
    ap.add_argument("--boxes", type=int, default=8400, help="N of the unletterbox launch (B, N, 4)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "letterbox" / "letterbox_bench.json"))
    args = ap.parse_args()
    from datasets.crater import pack_images, resize_batch
    from datasets.letterbox import lb_table, letterbox_batch, table_bytes, unletterbox_padded

    assert torch.cuda.is_available(), "letterbox_bench needs the MI355X"
    dev = torch.device("cuda", 0)
    B, S, ch = args.batch, args.size, args.ch
    g = torch.Generator().manual_seed(0)
    variants, shapes = {}, {}
    for name, (h, w) in (("4x3", (args.src_h, args.src_w)), ("square", (args.src_w, args.src_w))):
        ims = [torch.randint(0, 256, (h, w, ch) if ch > 1 else (1, h, w), generator=g, dtype=torch.uint8)
               for _ in range(B)]
        host = pack_images(ims, S, channels=ch)
        table = lb_table(host["img_meta"], S, S)
        shapes[name] = {"src": [h, w], "nw": table[0].nw, "nh": table[0].nh, "left": table[0].left,
                        "top": table[0].top}
        tb = table_bytes(table, B).to(dev)
        u8, meta = host["img_u8"].to(dev), host["img_meta"].to(dev)
        variants[f"stretch_{name}"] = lambda u8=u8, meta=meta: resize_batch(u8, meta, S, ch)
        variants[f"letterbox_{name}"] = lambda u8=u8, meta=meta, tb=tb: letterbox_batch(u8, meta, tb, S, S, ch)
        if name == "square":                               # no pad: the two launches write the same image
            assert torch.equal(variants["stretch_square"](), variants["letterbox_square"]())
            boxes = torch.rand(B, args.boxes, 4, generator=g).to(dev)
            count = torch.full((B,), args.boxes, dtype=torch.int32, device=dev)
            out = torch.empty_like(boxes)
            variants["unletterbox"] = lambda boxes=boxes, count=count, tb=tb, out=out: unletterbox_padded(
                boxes, count, tb, S, S, out=out)

    st = torch.cuda.current_stream(dev)
    for fn in variants.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.windows):
        for name, fn in variants.items():                  # alternate the variants inside every window
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(args.reps):
                fn()
            e1.record(st)
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.reps * 1e3)
    us = {k: statistics.median(v) for k, v in times.items()}
    out_bytes = 4 * ch * B * S * S
    box_bytes = 2 * 16 * B * args.boxes
    res = {"bench": "letterbox", "commit": args.commit, "batch": B, "size": S, "ch": ch, "shapes": shapes,
           "boxes": args.boxes, "reps": args.reps, "windows": args.windows, "out_bytes": out_bytes,
           "write_floor_us": round(out_bytes / (HBM_TBPS * 1e12) * 1e6, 1),
           "us_per_round": {k: round(v, 2) for k, v in us.items()},
           "us_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()},
           "letterbox_over_stretch": {n: round(us[f"letterbox_{n}"] / us[f"stretch_{n}"], 3) for n in shapes},
           "unletterbox_bytes": box_bytes,
           "unletterbox_GBps": round(box_bytes / (us["unletterbox"] * 1e-6) / 1e9, 1)}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
