"""Class-aware detection metrics (ym_eval_detections_cls) against the class-agnostic chain, timed on the GPU.

A COCO-val-sized synthetic set: --images images, each with U(0, --max-gt) GT boxes and U(0, --max-pred)
predictions (jittered copies of GT boxes and spurious boxes, scores with ties), labelled.  Inputs are resident
in HBM; each call is timed with HIP events on the launch stream, the variants alternate inside every repetition,
and the median over --reps repetitions after --warmup is reported:
  (a) ym_eval_detections                    the class-agnostic chain
  (b) ym_eval_detections_cls, nc = 1        same inputs, every label 0 (also checked equal to (a))
  (c) nc = 80   (d) nc = 1024               labels spread over the classes
--baseline-lib PATH times (a) through another build of libyolomi.so as well (an earlier commit's, for A/B).
Prints one JSON line; --out FILE also writes it there.

usage: python tools/eval_cls_bench.py [--images 5000 --max-gt 100 --max-pred 300 --reps 30]
"""
import argparse
import ctypes
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "yolo-scratch_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def workload(n_img, max_gt, max_pred, seed=0):
    rng = np.random.default_rng(seed)
    gc = rng.integers(0, max_gt + 1, n_img)
    pc = rng.integers(0, max_pred + 1, n_img)
    ng, npd = int(gc.sum()), int(pc.sum())
    c = rng.random((ng, 2))
    wh = 0.01 + 0.1 * rng.random((ng, 2))
    gb = np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)
    goff = np.concatenate([[0], np.cumsum(gc)])
    img = np.repeat(np.arange(n_img), pc)
    # a prediction: a jittered GT box of its image (70 %, when the image has one), else a spurious box
    src = goff[img] + (rng.random(npd) * np.maximum(gc[img], 1)).astype(np.int64)
    from_gt = (rng.random(npd) < 0.7) & (gc[img] > 0)
    src = np.where(from_gt, src, 0)
    pb = np.where(from_gt[:, None], gb[np.minimum(src, max(ng - 1, 0))] + rng.normal(0, 0.01, (npd, 4)),
                  rng.random((npd, 4)))
    pb = np.stack([np.minimum(pb[:, 0], pb[:, 2]), np.minimum(pb[:, 1], pb[:, 3]),
                   np.maximum(pb[:, 0], pb[:, 2]), np.maximum(pb[:, 1], pb[:, 3])], 1).astype(np.float32)
    ps = (np.floor(rng.random(npd) * 1000) / 1000).astype(np.float32)
    u_gt, u_pred = rng.random(ng), rng.random(npd)           # class = floor(u * nc): the same draw at every nc
    copy = from_gt & (rng.random(npd) < 0.8)                 # a copied box keeps its GT's label 4 times in 5
    u_pred = np.where(copy, u_gt[np.minimum(src, max(ng - 1, 0))], u_pred)
    return pb, ps, pc, gb, gc, u_pred, u_gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--max-gt", type=int, default=100)
    ap.add_argument("--max-pred", type=int, default=300)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--baseline-lib", type=str, default=None)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from yolomi._lib import SIGNATURES, lib, stream_ptr
    if not torch.cuda.is_available():
        raise SystemExit("eval_cls_bench measures on the MI355X: no GPU visible")
    dev = torch.device("cuda", 0)
    pb, ps, pc, gb, gc, u_pred, u_gt = workload(args.images, args.max_gt, args.max_pred)
    n_img, n_pred, n_gt = args.images, len(pb), len(gb)
    tpb, tps, tgb = (torch.from_numpy(x).to(dev) for x in (pb, ps, gb))
    poff = torch.from_numpy(np.concatenate([[0], np.cumsum(pc)]).astype(np.int64)).to(dev)
    goff = torch.from_numpy(np.concatenate([[0], np.cumsum(gc)]).astype(np.int64)).to(dev)
    thr = np.arange(0.5, 0.95 + 1e-6, 0.05)
    n_thr = len(thr)
    thr_c = (ctypes.c_double * n_thr)(*thr.tolist())
    st = stream_ptr(dev)
    L = lib()
    libs = {"a": L}
    if args.baseline_lib:
        B = ctypes.CDLL(args.baseline_lib)
        for name in ("ym_eval_workspace_size", "ym_eval_detections"):
            getattr(B, name).restype, getattr(B, name).argtypes = SIGNATURES[name]
        libs["a_baseline_lib"] = B
    runs, outs = {}, {}
    for key, lb in libs.items():
        nb = lb.ym_eval_workspace_size(n_img, n_pred, n_thr)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        out = torch.empty(n_thr + 7, dtype=torch.float64, device=dev)
        outs[key] = out
        runs[key] = (lambda lb=lb, ws=ws, nb=nb, out=out: lb.ym_eval_detections(
            tpb.data_ptr(), tps.data_ptr(), poff.data_ptr(), tgb.data_ptr(), goff.data_ptr(), n_img, n_pred, n_gt,
            int(gc.max()), thr_c, n_thr, n_thr, 0, 0.25, ws.data_ptr(), nb, out.data_ptr(), st))
    for key, nc in (("b_nc1", 1), ("c_nc80", 80), ("d_nc1024", 1024)):
        pl = torch.from_numpy(np.minimum((u_pred * nc).astype(np.int64), nc - 1)).to(dev)
        gl = torch.from_numpy(np.minimum((u_gt * nc).astype(np.int64), nc - 1)).to(dev)
        nb = L.ym_eval_cls_workspace_size(n_img, n_pred, n_thr, nc)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        out = torch.empty(nc * n_thr + 3 * nc + 7, dtype=torch.float64, device=dev)
        outs[key] = out
        runs[key] = (lambda pl=pl, gl=gl, ws=ws, nb=nb, out=out, nc=nc: L.ym_eval_detections_cls(
            tpb.data_ptr(), tps.data_ptr(), pl.data_ptr(), poff.data_ptr(), tgb.data_ptr(), gl.data_ptr(),
            goff.data_ptr(), n_img, n_pred, n_gt, int(gc.max()), nc, thr_c, n_thr, n_thr, 0, 0.25, ws.data_ptr(), nb,
            out.data_ptr(), st))
    stream = torch.cuda.current_stream(dev)
    times = {k: [] for k in runs}
    for rep in range(args.warmup + args.reps):
        for key, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rc = fn()
            e1.record(stream)
            e1.synchronize()
            if rc != 0:
                raise SystemExit(f"{key}: status {rc}: {L.ym_last_error().decode()}")
            if rep >= args.warmup:
                times[key].append(e0.elapsed_time(e1))
    res = {k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "p90_ms": float(np.percentile(v, 90))}
           for k, v in times.items()}
    a, b = outs["a"].cpu().numpy(), outs["b_nc1"].cpu().numpy()
    same = bool(np.array_equal(a[n_thr + 4:], b[n_thr + 3 + 4:]) and a[n_thr] == b[n_thr + 3]
                and a[n_thr + 1] == b[n_thr + 4] and np.allclose(a[:n_thr], b[:n_thr], rtol=1e-12, atol=1e-15))
    line = {"metric": "eval_detections_cls_ms", "images": n_img, "predictions": n_pred, "gt": n_gt,
            "reps": args.reps, "times": res, "b_over_a": res["b_nc1"]["median_ms"] / res["a"]["median_ms"],
            "nc1_equals_class_agnostic": same,
            "mAP50": {k: float(o[-5]) for k, o in ((k, outs[k].cpu().numpy()) for k in outs)}}
    print(json.dumps(line))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
