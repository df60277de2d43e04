"""Greedy box merging of sliced inference (ym_decode_nmm_tiles) against the suppression it stands beside
(ym_decode_nms_tiles), on the same forward output in one process: tools/slice_bench.py's method (HIP events on the
launch stream, warm-up, then `--windows` alternating windows of `--reps` rounds per variant, the median window's time
per round, the windows' spread reported) and its setup (the `--scale` network with random weights, `--ch` planes,
`--sources` images of `--src-h` x `--src-w` under `--tile` windows, `conf` at the score quantile that makes
`--cand-share` of the anchors candidates).  Four variants:
  nms        ym_decode_nms_tiles, the existing entry point
  iou        ym_decode_nmm_tiles, IoU, no merge: the existing entry point's work, plus the absorbed counts
  ios        ym_decode_nmm_tiles, IoS, no merge
  ios_merge  ym_decode_nmm_tiles, IoS, the kept boxes grown to their unions
Two figures per variant:
  merge      the boxes alone, from a resident forward output
  predict    the whole Predictor call from host images to boxes
Every variant is reported as a ratio to `nms` of the same build and process.  Random weights make random boxes: the
kept and absorbed counts describe this input, not a detector.  Writes one JSON object to `--out` and prints it.

usage: python tools/nmm_bench.py [--tile 640 --scale s --ch 3 --sources 1 8 --out FILE]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "yolo-scratch_amd"), str(ROOT / "tools")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rect_bench import windows  # noqa: E402

# variant -> (metric, merge) of decode_nmm_tiles; None: decode_nms_tiles
NMM = {"nms": None, "iou": ("iou", False), "ios": ("ios", False), "ios_merge": ("ios", True)}
# variant -> Predictor(slice_merge, slice_metric); "iou" has no Predictor spelling of its own (the defaults take the
# existing call), so its predict figure is not taken
PRED = {"nms": ("nms", "iou"), "ios": ("nms", "ios"), "ios_merge": ("nmm", "ios")}


def resident(pred, ims):
    """The forward output of Predictor._run_sliced over `ims`, resident -> (ybuf, table, tile_begin, T)."""
    from datasets.crater import pack_images
    from datasets.slicing import slice_batch, tile_bytes, tile_table
    S, nb = pred.imgsz, pred.batch
    packed = pack_images([pred._raw(im) for im in ims], S, pred.ch)
    table, begin = tile_table(packed["img_meta"][:, 1:].tolist(), pred.slice, pred.slice_overlap, S, pred.slice_full)
    T = begin[-1]
    Tp = -(-T // nb) * nb
    tdev = tile_bytes(table, T, Tp).to(pred.device)
    u8, meta = packed["img_u8"].to(pred.device), packed["img_meta"].to(pred.device)
    ybuf = None
    with torch.no_grad():
        for lo in range(0, Tp, nb):
            y = pred.model(slice_batch(u8, meta, tdev, nb, S, S, pred.ch, pred.fill, first=lo))[0]
            if ybuf is None:
                ybuf = torch.empty(Tp, *y.shape[1:], dtype=y.dtype, device=y.device)
            ybuf[lo:lo + nb].copy_(y)
    return ybuf, tdev, begin, T


def boxes_fn(name, pred, ybuf, tdev, begin, T):
    from yolomi import post
    kw = dict(class_aware=True, max_det=pred.max_det, edge=pred.slice_edge)
    if NMM[name] is None:
        return lambda: post.decode_nms_tiles(ybuf[:T].transpose(1, 2), tdev, begin, pred.conf, pred.iou, **kw)
    metric, merge = NMM[name]
    return lambda: post.decode_nmm_tiles(ybuf[:T].transpose(1, 2), tdev, begin, pred.conf, pred.iou, metric=metric,
                                         merge=merge, **kw)


def figures(tt, base="nms"):
    med = {k: statistics.median(v) for k, v in tt.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in tt.items()}
    return {"us_per_round": {k: round(v, 1) for k, v in med.items()},
            "us_min_max": {k: [round(min(v), 1), round(max(v), 1)] for k, v in tt.items()},
            "spread": {k: round(v, 3) for k, v in spread.items()},
            "over_" + base: {k: round(med[k] / med[base], 3) for k in tt if k != base}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--tile", type=int, default=640)
    ap.add_argument("--overlap", type=float, default=0.2)
    ap.add_argument("--scale", default="s")
    ap.add_argument("--ch", type=int, default=3)
    ap.add_argument("--nc", type=int, default=80)
    ap.add_argument("--batch", type=int, default=8, help="tiles per forward")
    ap.add_argument("--sources", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--src-h", type=int, default=2160)
    ap.add_argument("--src-w", type=int, default=3840)
    ap.add_argument("--iou", type=float, default=0.45, help="the match threshold of every variant")
    ap.add_argument("--max-det", type=int, default=300)
    ap.add_argument("--cand-share", type=float, default=0.01,
                    help="conf is the score quantile that makes this share of the anchors candidates")
    ap.add_argument("--reps", type=int, default=8, help="rounds per window with one source; divided by the sources")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-predict", dest="predict", action="store_false", help="the merge figure alone")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "nmm" / "nmm_bench.json"))
    args = ap.parse_args()
    import train_yolo11_cuda as T
    from yolomi.predict import Predictor

    assert torch.cuda.is_available(), "nmm_bench needs the MI355X"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cfg = str(ROOT / "yolo-scratch_amd" / "configs" / "yolo11n_crater.yaml")
    model = T.build_model(cfg, args.scale, args.ch, args.nc, dev).eval()
    rng = np.random.default_rng(0)
    rows = []
    for n_src in args.sources:
        ims = [rng.integers(0, 256, (args.src_h, args.src_w, args.ch), dtype=np.uint8) for _ in range(n_src)]
        kw = dict(imgsz=args.imgsz, ch=args.ch, iou=args.iou, max_det=args.max_det, batch=args.batch, device=dev,
                  slice=args.tile, slice_overlap=args.overlap)
        preds = {k: Predictor(model, slice_merge=m, slice_metric=q, **kw) for k, (m, q) in PRED.items()}
        ybuf, tdev, begin, n_tiles = resident(preds["nms"], ims)
        best = ybuf[:n_tiles, 4:].amax(1).flatten()
        conf = float(best.kthvalue(max(1, round(best.numel() * (1.0 - args.cand_share)))).values)
        for p in preds.values():
            p.conf = conf
        merge = {k: boxes_fn(k, preds["nms"], ybuf, tdev, begin, n_tiles) for k in NMM}
        outs = {k: fn() for k, fn in merge.items()}
        counts = {k: {"kept_per_image": sum(o["counts"]) / n_src,
                      **({"absorbed_per_image": sum(int(o["merged"][g, :c].sum())
                                                    for g, c in enumerate(o["counts"])) / n_src}
                         if "merged" in o else {})} for k, o in outs.items()}
        grew = sum(int((outs["ios_merge"]["boxes"][g, :c] != outs["ios"]["boxes"][g, :c]).any(1).sum())
                   for g, c in enumerate(outs["ios"]["counts"])) / n_src
        same = all(torch.equal(outs["iou"][key][g, :c], outs["nms"][key][g, :c])
                   for key in ("boxes", "scores", "labels", "index", "rows") for g, c in enumerate(outs["nms"]["counts"]))
        assert same and outs["iou"]["counts"] == outs["nms"]["counts"], "IoU without merge must equal the NMS entry"
        reps = max(1, args.reps // n_src)
        row = {"sources": n_src, "src": [args.src_h, args.src_w], "tiles": n_tiles, "reps": reps, "conf": conf,
               "candidates_per_image": float((best > conf).sum()) / n_src, "counts": counts,
               "unions_grown_per_image": grew, "iou_equals_nms": same,
               "merge": figures(windows(merge, reps, args.windows, args.warmup, dev))}
        m = row["merge"]
        # the IoU / no-merge variant does the existing entry point's work: slower by more than the two spreads?
        row["iou_within_spreads"] = bool(m["over_nms"]["iou"] - 1.0 <= m["spread"]["iou"] + m["spread"]["nms"])
        if args.predict:
            row["predict"] = figures(windows({k: (lambda p=p: p(ims)) for k, p in preds.items()}, reps, args.windows,
                                             args.warmup, dev))
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"bench": "nmm", "commit": args.commit, "device": torch.cuda.get_device_name(0), "imgsz": args.imgsz,
           "tile": args.tile, "overlap": args.overlap, "scale": args.scale, "ch": args.ch, "nc": args.nc,
           "iou": args.iou, "max_det": args.max_det, "cand_share": args.cand_share, "batch": args.batch,
           "windows": args.windows, "warmup": args.warmup, "rows": rows,
           "note": "random weights: the kept, absorbed and grown counts describe this input, not a detector"}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
