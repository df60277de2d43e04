"""The 3-plane augmentation launch (ym_augment_u8c) against three 1-plane launches (ym_augment_u8) of the same table,
in one process: HIP events on the launch stream, warm-up, then `--windows` alternating windows of `--reps` rounds per
variant; the figure is the median window's time per round.  Variants: three 1-plane launches over a 1-plane batch of
the same image sizes, the 3-plane launch without a colour table, the 3-plane launch with hue and saturation.  The
3-plane launch forms a third of the addresses and weights and writes the same bytes (4 * 3 * B * S * S), so it is
expected not to exceed the three launches' sum.  Writes one JSON object to `--out` and prints it; `--commit` is
echoed into it (the caller's `git rev-parse --short HEAD`).

usage: python tools/colour_bench.py [--batch 64 --size 640 --src 1024 --reps 20 --windows 15 --out FILE]
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
    ap.add_argument("--src", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "colour" / "colour_bench.json"))
    args = ap.parse_args()
    from datasets.augment import AugmentHyp, BatchAugment, augment_batch, table_bytes
    from datasets.crater import pack_images

    assert torch.cuda.is_available(), "colour_bench needs the MI355X"
    dev = torch.device("cuda", 0)
    B, S = args.batch, args.size
    g = torch.Generator().manual_seed(0)
    rgb = [torch.randint(0, 256, (args.src, args.src, 3), generator=g, dtype=torch.uint8) for _ in range(B)]
    host3 = pack_images(rgb, S, channels=3)
    host1 = pack_images([t[..., 0].contiguous().unsqueeze(0) for t in rgb], S)          # plane 0 of the same images
    for h in (host1, host3):
        h.update({"batch_idx": torch.zeros((0,), dtype=torch.long), "cls": torch.zeros((0, 1), dtype=torch.long),
                  "bboxes": torch.zeros((0, 4))})
    aug = BatchAugment(AugmentHyp(hsv_h=0.015, hsv_s=0.7), seed=1)                       # the default geometry
    table = table_bytes(aug.plan(host3, 1, 0)[0]).to(dev)
    colour = table_bytes(aug.colours(B, 1, 0)).to(dev)
    u8_3, meta3 = host3["img_u8"].to(dev), host3["img_meta"].to(dev)
    u8_1, meta1 = host1["img_u8"].to(dev), host1["img_meta"].to(dev)

    def three_planes_one_by_one():
        return [augment_batch(u8_1, meta1, table, S) for _ in range(3)]

    variants = {"augment1_x3": three_planes_one_by_one,
                "augment3": lambda: augment_batch(u8_3, meta3, table, S, 3),
                "augment3_hsv": lambda: augment_batch(u8_3, meta3, table, S, 3, colour)}
    # the same table over plane 0: the colour launch's first plane is the 1-plane launch's image
    assert torch.equal(variants["augment3"]()[:, :1], variants["augment1_x3"]()[0])

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
    out_bytes = 4 * 3 * B * S * S
    res = {"bench": "colour", "commit": args.commit, "batch": B, "size": S, "src": args.src, "reps": args.reps,
           "windows": args.windows, "out_bytes": out_bytes,
           "write_floor_us": round(out_bytes / (HBM_TBPS * 1e12) * 1e6, 1),
           "us_per_round": {k: round(v, 2) for k, v in us.items()},
           "us_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()},
           "ratio_to_three_launches": {k: round(us[k] / us["augment1_x3"], 3) for k in ("augment3", "augment3_hsv")},
           "write_GBps": {k: round(out_bytes / (v * 1e-6) / 1e9, 1) for k, v in us.items()}}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
