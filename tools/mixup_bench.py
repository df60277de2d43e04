"""MixUp in the augmentation launch (ym_augment_mix_u8c) against the unmixed launch (ym_augment_u8c) and against the
hand composition, in one process, by tools/colour_bench.py's method: HIP events on the launch stream, warm-up, then
`--windows` alternating windows of `--reps` rounds per variant; the figure is the median window's time per round and
the spread is the windows' minimum and maximum.  bs64, S = 640, 1024 x 1024 sources, 3 planes, the default geometry,
hue and saturation on.  Variants:
  a_unmixed        ym_augment_u8c
  b_mix_none       ym_augment_mix_u8c, no image mixed (every record -1, no partner table)
  c_mix_15pct      ym_augment_mix_u8c, 15 % of the images mixed (a compact partner table)
  d_mix_all        ym_augment_mix_u8c, every image mixed
  e_hand_all       the hand composition of d: two ym_augment_u8c launches into two buffers and a torch lerp (which
                   applies gain and hue / sat before the blend and blends in float: other values, the same work)
Bars: b within the windows' spread of a; the slowest d window faster than the fastest e window.  Writes one JSON
object to `--out` and prints it; `--commit` is echoed into it (the caller's `git rev-parse --short HEAD`).

usage: python tools/mixup_bench.py [--batch 64 --size 640 --src 1024 --reps 20 --windows 15 --out FILE]
"""
import argparse
import ctypes
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mixup" / "mixup_bench.json"))
    args = ap.parse_args()
    from datasets.augment import AugmentHyp, BatchAugment, augment_batch, augment_mix_batch, table_bytes
    from datasets.crater import pack_images
    from yolomi._lib import AugEntry, AugMix

    assert torch.cuda.is_available(), "mixup_bench needs the MI355X"
    dev = torch.device("cuda", 0)
    B, S = args.batch, args.size
    g = torch.Generator().manual_seed(0)
    rgb = [torch.randint(0, 256, (args.src, args.src, 3), generator=g, dtype=torch.uint8) for _ in range(B)]
    host = pack_images(rgb, S, channels=3)
    host.update({"batch_idx": torch.zeros((0,), dtype=torch.long), "cls": torch.zeros((0, 1), dtype=torch.long),
                 "bboxes": torch.zeros((0, 4))})
    aug = BatchAugment(AugmentHyp(hsv_h=0.015, hsv_s=0.7, mixup=1.0), seed=1)            # the default geometry
    table_c, _, _, _, _, partner_c, mix_c = aug.plan_mix(host, 1, 0)
    assert len(partner_c) == B
    table, colour = table_bytes(table_c).to(dev), table_bytes(aug.colours(B, 1, 0)).to(dev)
    partner_all, mix_all = table_bytes(partner_c).to(dev), table_bytes(mix_c).to(dev)
    none_c = (AugMix * B)()
    for m in none_c:
        m.ratio, m.partner = 65536, -1
    mix_none = table_bytes(none_c).to(dev)
    some = [i for i in range(B) if (i * 15) % 100 < 15]                                  # 15 % of the images, spread
    some_p, some_m = (AugEntry * max(len(some), 1))(), (AugMix * B)()
    for i in range(B):
        some_m[i].ratio, some_m[i].partner = mix_c[i].ratio, some.index(i) if i in some else -1
    for k, i in enumerate(some):
        some_p[k] = partner_c[i]
    partner_some, mix_some = table_bytes(some_p).to(dev), table_bytes(some_m).to(dev)
    u8, meta = host["img_u8"].to(dev), host["img_meta"].to(dev)
    weight = torch.tensor([m.ratio / 65536.0 for m in mix_c], device=dev).view(B, 1, 1, 1)

    def hand():
        a = augment_batch(u8, meta, table, S, 3, colour)
        p = augment_batch(u8, meta, partner_all, S, 3, colour)
        return torch.lerp(p, a, weight)

    variants = {"a_unmixed": lambda: augment_batch(u8, meta, table, S, 3, colour),
                "b_mix_none": lambda: augment_mix_batch(u8, meta, table, None, mix_none, S, 3, colour),
                "c_mix_15pct": lambda: augment_mix_batch(u8, meta, table, partner_some, mix_some, S, 3, colour),
                "d_mix_all": lambda: augment_mix_batch(u8, meta, table, partner_all, mix_all, S, 3, colour),
                "e_hand_all": hand}
    # no image mixed is the unmixed launch bit for bit; the unmixed images of c are too, the mixed ones are d's
    ref, none, part, full = (variants[k]() for k in ("a_unmixed", "b_mix_none", "c_mix_15pct", "d_mix_all"))
    assert torch.equal(ref, none)
    rest = [i for i in range(B) if i not in some]
    assert torch.equal(part[rest], ref[rest]) and torch.equal(part[some], full[some])
    assert not torch.equal(full, ref)
    # the partner entries carry gain 1 and the hand composition blends after the gain: near, not equal
    near = float((variants["e_hand_all"]() - full).abs().max())

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
    lo = {k: min(v) for k, v in times.items()}
    hi = {k: max(v) for k, v in times.items()}
    out_bytes = 4 * 3 * B * S * S
    res = {"bench": "mixup", "commit": args.commit, "batch": B, "size": S, "src": args.src, "reps": args.reps,
           "windows": args.windows, "mixed_in_c": len(some), "out_bytes": out_bytes,
           "table_bytes": {"a_unmixed": B * (ctypes.sizeof(AugEntry) + 8),
                           "d_mix_all": B * (2 * ctypes.sizeof(AugEntry) + 16)},
           "write_floor_us": round(out_bytes / (HBM_TBPS * 1e12) * 1e6, 1),
           "us_per_round": {k: round(v, 2) for k, v in us.items()},
           "us_min_max": {k: [round(lo[k], 2), round(hi[k], 2)] for k in times},
           "ratio_to_unmixed": {k: round(us[k] / us["a_unmixed"], 3) for k in us},
           "hand_vs_launch_max_abs_diff": round(near, 4),
           "bars": {"b_within_spread_of_a": bool(lo["a_unmixed"] <= us["b_mix_none"] <= hi["a_unmixed"]
                                                 or lo["b_mix_none"] <= us["a_unmixed"] <= hi["b_mix_none"]),
                    "slowest_d_beats_fastest_e": bool(hi["d_mix_all"] < lo["e_hand_all"]),
                    "d_at_most_twice_a": bool(us["d_mix_all"] <= 2.0 * us["a_unmixed"])}}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
