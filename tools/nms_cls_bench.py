"""Decode + NMS timing, class-agnostic against class-aware with a detection cap.

On synth_eval_preds(B, 8400, nc) for B in 1, 8, 128 and nc in 1, 5, 80, at conf 0.25 / iou 0.45 and at
conf 0.001 / iou 0.7, four variants of one call:
  a  ym_decode_nms_strided of this build
  b  ym_decode_nms_strided of an earlier build's library (--parent-lib PATH), loaded beside this one in the process
  c  ym_decode_nms_cls, max_det 0
  d  ym_decode_nms_cls, max_det 300
The variants alternate inside each repetition; HIP events around each call; median (min .. 90th percentile) in
microseconds, and the mean kept count per image.  The nc = 1 rows put (c) beside (a) at equal kept counts.
The only condition is on the unchanged path: the median of (a) within the larger of 3 % and (b)'s min..p90 spread
of (b)'s median.

usage: python tools/nms_cls_bench.py [--parent-lib PATH] [--reps 30] [--out profiles/nms_cls/nms_cls_bench.json]"""
import argparse
import ctypes
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "yolo-scratch_amd")]
import torch  # noqa: E402
from datasets.synthetic import synth_eval_preds  # noqa: E402
from yolomi import _lib as yl  # noqa: E402

N = 8400
IMG = 640.0


def load_parent(path):
    L = ctypes.CDLL(str(path))
    for name in ("ym_nms_workspace_size", "ym_decode_nms_strided"):
        res, args = yl.SIGNATURES[name]
        getattr(L, name).restype = res
        getattr(L, name).argtypes = args
    return L


def stats(ts):
    ts = sorted(ts)
    q = lambda f: ts[min(len(ts) - 1, int(f * len(ts)))]
    return {"median_us": q(0.5) * 1e3, "min_us": ts[0] * 1e3, "p90_us": q(0.9) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", type=str, default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "nms_cls" / "nms_cls_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nms_cls_bench: needs the MI355X (no CPU timing)")
    L = yl.lib()
    LP = load_parent(args.parent_lib) if args.parent_lib else None
    dev = torch.device("cuda")
    st = yl.stream_ptr(dev)
    rows = []
    for B in (1, 8, 128):
        for nc in (1, 5, 80):
            pred = synth_eval_preds(B, N, nc=nc, seed=100 + B + nc).cuda()
            ws_bytes = max(L.ym_nms_cls_workspace_size(B, N), LP.ym_nms_workspace_size(B, N) if LP else 0)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            cnt = torch.empty(B, dtype=torch.int32, device=dev)
            boxes = torch.empty(B, N, 4, dtype=torch.float32, device=dev)
            scores = torch.empty(B, N, dtype=torch.float32, device=dev)
            labels = torch.empty(B, N, dtype=torch.int64, device=dev)
            index = torch.empty(B, N, dtype=torch.int64, device=dev)
            head = (pred.data_ptr(), B, N, nc, pred.stride(1), pred.stride(0), pred.stride(2))
            tail = (ws.data_ptr(), ws_bytes, cnt.data_ptr(), boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(),
                    index.data_ptr(), st)
            for conf, iou in ((0.25, 0.45), (0.001, 0.7)):
                thr = (conf, iou, IMG)
                variants = {"a": lambda: L.ym_decode_nms_strided(*head, *thr, *tail),
                            "c": lambda: L.ym_decode_nms_cls(*head, *thr, 0, *tail),
                            "d": lambda: L.ym_decode_nms_cls(*head, *thr, 300, *tail)}
                if LP:
                    variants["b"] = lambda: LP.ym_decode_nms_strided(*head, *thr, *tail)
                times = {k: [] for k in variants}
                kept = {}
                for rep in range(args.warmup + args.reps):
                    for k in sorted(variants):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        rc = variants[k]()
                        e1.record()
                        e1.synchronize()
                        if rc != 0:
                            raise SystemExit(f"variant {k} failed ({rc}): {L.ym_last_error().decode()}")
                        if rep >= args.warmup:
                            times[k].append(e0.elapsed_time(e1))
                        kept[k] = float(cnt.float().mean())
                row = {"B": B, "nc": nc, "conf": conf, "iou": iou}
                for k in sorted(variants):
                    s = stats(times[k])
                    s["kept_per_image"] = kept[k]
                    s["us_per_kept_box"] = s["median_us"] / max(kept[k] * B, 1.0)
                    row[k] = s
                if LP:
                    a, b = row["a"], row["b"]
                    allow = max(0.03 * b["median_us"], b["p90_us"] - b["min_us"])
                    row["a_vs_b"] = {"delta_us": a["median_us"] - b["median_us"], "allowed_us": allow,
                                     "met": a["median_us"] - b["median_us"] <= allow}
                rows.append(row)
                print(f"B {B:3d} nc {nc:2d} conf {conf:<5} iou {iou:<4} | " + " | ".join(
                    f"{k} {row[k]['median_us']:8.1f} ({row[k]['min_us']:.1f} .. {row[k]['p90_us']:.1f}) us, kept "
                    f"{row[k]['kept_per_image']:.1f}" for k in sorted(variants))
                    + (f" | a-b {row['a_vs_b']['delta_us']:+.1f} us (allowed {row['a_vs_b']['allowed_us']:.1f}): "
                       f"{'met' if row['a_vs_b']['met'] else 'NOT met'}" if LP else ""), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "anchors": N, "reps": args.reps, "warmup": args.warmup,
           "parent_lib": bool(LP), "rows": rows}
    if LP:
        out["a_within_b_everywhere"] = all(r["a_vs_b"]["met"] for r in rows)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
