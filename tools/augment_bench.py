"""ym_augment_u8 against ym_resize_linear_u8 on the same packed batch: one launch each, HIP events on the launch
stream, warm-up, then `--windows` alternating windows of `--reps` launches per variant; the figure is the median
window's time per launch.  Variants: the resize launch, the augmentation with identity entries, with the default
hyperparameters (mosaic on, no rotation) and with degrees=10 (source rows no longer read along x).  Prints one JSON
line; `--commit` is echoed into it (the caller's `git rev-parse --short HEAD`).

usage: python tools/augment_bench.py [--batch 64 --size 640 --src 1024 --reps 20 --windows 15 --step-ms 18.4]
"""
import argparse
import functools
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "yolo-scratch_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--src", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--step-ms", type=float, default=18.4, help="the training step the launch's share is taken of")
    ap.add_argument("--commit", default="")
    args = ap.parse_args()
    from datasets.augment import AugmentHyp, BatchAugment, augment_batch, table_bytes
    from datasets.crater import pack_images, resize_batch

    assert torch.cuda.is_available(), "augment_bench needs the MI355X"
    dev = torch.device("cuda", 0)
    B, S = args.batch, args.size
    g = torch.Generator().manual_seed(0)
    imgs = [torch.randint(0, 256, (1, args.src, args.src), generator=g, dtype=torch.uint8) for _ in range(B)]
    host = pack_images(imgs, S)
    host.update({"batch_idx": torch.zeros((0,), dtype=torch.long), "cls": torch.zeros((0, 1), dtype=torch.long),
                 "bboxes": torch.zeros((0, 4))})
    u8, meta = host["img_u8"].to(dev), host["img_meta"].to(dev)

    def table(hyp):
        return table_bytes(BatchAugment(hyp, seed=1).plan(host, 1, 0)[0]).to(dev)

    off = AugmentHyp(mosaic=0, degrees=0, translate=0, scale=0, shear=0, fliplr=0, flipud=0, gain=0)
    tables = {"augment_identity": table(off), "augment_default": table(AugmentHyp()),
              "augment_degrees10": table(AugmentHyp(degrees=10.0))}
    variants = {"resize": lambda: resize_batch(u8, meta, S)}
    for name, t in tables.items():
        variants[name] = functools.partial(augment_batch, u8, meta, t, S)
    assert torch.equal(variants["augment_identity"](), variants["resize"]())

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
    out_bytes = 4 * B * S * S
    res = {"bench": "augment", "commit": args.commit, "batch": B, "size": S, "src": args.src, "reps": args.reps,
           "windows": args.windows,
           "us_per_launch": {k: round(v, 2) for k, v in us.items()},
           "us_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()},
           "ratio_to_resize": {k: round(us[k] / us["resize"], 3) for k in tables},
           "write_GBps": {k: round(out_bytes / (v * 1e-6) / 1e9, 1) for k, v in us.items()},
           "share_of_step": {k: round(us[k] * 1e-3 / args.step_ms, 5) for k in tables}, "step_ms": args.step_ms}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
