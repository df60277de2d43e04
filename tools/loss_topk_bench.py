"""The fused loss forward under its two assigners in one process: ym_loss_fwd (in-box) and ym_loss_fwd_topk at k = 10,
called through the C ABI on the same (B, A, 64+nc) head rows.  HIP events on the launch stream, warm-up, then
`--windows` alternating windows of `--reps` forwards per variant; the figure is the median window's time per forward.
Two batches at the bench shape (s@640 bs64: A = 8400, nc = 5): synth_batch's own targets, and the same count of
targets with large boxes (w, h in [0.4, 0.9] of the image: where the in-box rule's positives grow with box area).
Both forwards do the same B*A*M IoU work, so the in-box time of the same run is the yardstick for the top-k time.
Also records the positives per image each assigner makes.  Writes one JSON object to `--out` and prints it;
`--commit` is echoed into it.

usage: python tools/loss_topk_bench.py [--batch 64 --size 640 --topk 10 --reps 20 --windows 15 --out FILE]
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


def large_box_batch(batch):
    """synth_batch's targets with every box redrawn large: centre U(0.3, 0.7), w / h U(0.4, 0.9), clamped."""
    g = torch.Generator().manual_seed(1)
    n = batch["bboxes"].shape[0]
    c = 0.3 + 0.4 * torch.rand(n, 2, generator=g)
    wh = 0.4 + 0.5 * torch.rand(n, 2, generator=g)
    return {**batch, "bboxes": torch.cat((c - wh / 2, c + wh / 2), 1).clamp_(0.0, 1.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--nc", type=int, default=5)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tal_topk" / "loss_topk_bench.json"))
    args = ap.parse_args()
    import ctypes
    from losses.yolo_v8_loss import _LossCtx
    from yolomi._lib import call, stream_ptr
    from datasets.synthetic import synth_batch

    assert torch.cuda.is_available(), "loss_topk_bench needs the MI355X"
    dev = torch.device("cuda", 0)
    B, S, nc, k = args.batch, args.size, args.nc, args.topk
    level_hw = [(S // s, S // s) for s in (8, 16, 32)]
    A = sum(h * w for h, w in level_hw)
    g = torch.Generator().manual_seed(0)
    head = (torch.randn(B, A, 64 + nc, generator=g) * 2.0).to(dev)
    lh = (ctypes.c_int * 3)(*[h for h, _ in level_hw])
    lw = (ctypes.c_int * 3)(*[w for _, w in level_hw])
    strides = (ctypes.c_float * 3)(8.0, 16.0, 32.0)
    sb = synth_batch(B, S, seed=0, nc=nc)
    small = {n: sb[n] for n in ("batch_idx", "cls", "bboxes")}
    batches = {"synth": small, "large_boxes": large_box_batch(small)}
    st = torch.cuda.current_stream(dev)
    res = {"bench": "loss_topk", "commit": args.commit, "batch": B, "size": S, "anchors": A, "nc": nc, "topk": k,
           "reps": args.reps, "windows": args.windows, "batches": {}}
    for bname, cpu_batch in batches.items():
        bidx = cpu_batch["batch_idx"].to(dev)
        cls = cpu_batch["cls"].reshape(-1).to(dev)
        boxes = cpu_batch["bboxes"].to(dev)
        n_gt = int(cls.shape[0])
        M = int(torch.bincount(cpu_batch["batch_idx"], minlength=B).max())
        ctxs = {"inbox": _LossCtx(B, A, M, dev), "topk": _LossCtx(B, A, M, dev, "topk", k)}

        def forward(name):
            lc = ctxs[name]
            a = (head.data_ptr(), B, A, nc, 3, lh, lw, strides, bidx.data_ptr(), cls.data_ptr(), boxes.data_ptr(), n_gt,
                 M, float(S), float(S), lc.ws.data_ptr(), lc.ws_bytes, lc.gt_box.data_ptr(), lc.gt_lab.data_ptr(),
                 lc.gt_valid.data_ptr(), lc.out.data_ptr())
            if name == "topk":
                call("ym_loss_fwd_topk", *a, k, stream_ptr(dev))
            else:
                call("ym_loss_fwd", *a, stream_ptr(dev))

        pos = {}
        for name in ctxs:
            for _ in range(10):
                forward(name)
            pos[name] = float(ctxs[name].out[5]) / B
        torch.cuda.synchronize()
        times = {n: [] for n in ctxs}
        for _ in range(args.windows):
            for name in ctxs:                              # alternate the variants inside every window
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(args.reps):
                    forward(name)
                e1.record(st)
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / args.reps * 1e3)
        us = {n: statistics.median(v) for n, v in times.items()}
        res["batches"][bname] = {"targets": n_gt, "max_gt": M,
                                 "us_per_forward": {n: round(v, 2) for n, v in us.items()},
                                 "us_min_max": {n: [round(min(v), 2), round(max(v), 2)] for n, v in times.items()},
                                 "topk_over_inbox": round(us["topk"] / us["inbox"], 3),
                                 "positives_per_image": {n: round(v, 1) for n, v in pos.items()}}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
