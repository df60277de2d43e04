"""The optimizer tail with and without the weight EMA, timed on the GPU over YOLOv11's real parameter set.

One model per variant (same seed, same gradients, resident in HBM), the tail of a training step in four forms:
  (a) FusedAdamW alone                                   ym_grad_norm + ym_adamw              (the tail without an EMA)
  (b) FusedAdamW with the EMA attached                   ym_grad_norm + ym_adamw_ema + ym_ema_update over the rest
  (c) FusedAdamW, then ModelEMA.update()                 (a) + ym_ema_update over every fp32 entry
  (d) FusedAdamW, then torch._foreach_mul_ / _foreach_add_ over every fp32 entry   (the unfused baseline)
Three timings of each, all between HIP events on the launch stream, the variants alternating inside every
repetition, median (min .. 90th percentile) over --reps repetitions after --warmup:
  kernels_ms       the C-ABI calls alone over the pointer tables the Python layer built, --inner calls back to
                   back per event pair: device time of the launches with their working set mostly in the
                   256 MiB Infinity Cache
  kernels_cold_ms  the same calls one per event pair, each after a 1 GiB fill: from HBM, as a training step's
                   tail finds them after its backward
  step_ms          the Python call a trainer makes (optimizer.step() [+ ema.update()]), --inner per event pair:
                   the launches plus the host work around them (table keys), which at four launches is most of it
The bytes are arithmetic from the element counts (28 B per stepped parameter, 8 more with the fused EMA, 12 per
element of a stand-alone EMA update); bytes / kernels_ms is an achieved rate, not a share of peak.
Prints one JSON line; --out FILE also writes it there.

usage: python tools/ema_bench.py [--scale s --reps 30 --inner 20 --out profiles/ema/ema_bench.json]
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "yolo-scratch_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=str, default="s", choices=["n", "s", "m", "l", "x"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_bench measures on the MI355X: no GPU visible")
    import yaml
    from models import build_yolo11
    from yolomi._lib import call, stream_ptr
    from yolomi.ema import ModelEMA
    from yolomi.optim import FusedAdamW
    dev = torch.device("cuda", 0)
    cfg = yaml.safe_load((ROOT / "yolo-scratch_amd" / "configs" / "yolo11n_crater.yaml").read_text())
    cfg["scale"] = args.scale

    def setup(with_ema, attach):
        torch.manual_seed(0)
        m = build_yolo11(cfg, ch=1, nc=5).to(dev).train()
        g = torch.Generator(device=dev).manual_seed(1)
        for p in m.parameters():
            if p.requires_grad:
                p.grad = torch.randn(p.shape, generator=g, device=dev) * 1e-2
        opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=5e-4, max_grad_norm=10.0)
        ema = ModelEMA(m) if with_ema else None
        if attach:
            opt.attach_ema(ema)
        return m, opt, ema

    ma, oa, _ = setup(False, False)
    mb, ob, eb = setup(True, True)
    mc, oc, ec = setup(True, False)
    md, od, ed = setup(True, False)
    d_pairs = [(e, s) for e, s in zip(ed.ema.state_dict().values(), md.state_dict().values()) if e.is_floating_point()]
    d_ema, d_src = [e for e, _ in d_pairs], [s.detach() for _, s in d_pairs]

    def foreach_ema():
        d = ed.decay_at(10 ** 6)
        torch._foreach_mul_(d_ema, d)
        torch._foreach_add_(d_ema, d_src, alpha=1.0 - d)

    steps = {"a": oa.step, "b": ob.step, "c": lambda: (oc.step(), ec.update()), "d": lambda: (od.step(), foreach_ema())}
    for fn in steps.values():                      # builds every pointer table
        fn()
    torch.cuda.synchronize()
    st = stream_ptr(dev)
    hyp = (1e-3, 0.9, 0.999, 1e-8, 5e-4, 10, 10.0)
    omd = 1.0 - 0.9999

    def tail(opt, ema_ptrs=None):
        _, ntab, n, total = opt._tables["norm"]
        _, tab, _, _ = opt._tables[0]
        nb = opt._partials.numel() - 1
        norm = opt._partials[nb:nb + 1]

        def run():
            call("ym_grad_norm", ntab.data_ptr(), n, total, opt._partials.data_ptr(), norm.data_ptr(), st)
            if ema_ptrs is None:
                call("ym_adamw", tab.data_ptr(), n, total, *hyp, norm.data_ptr(), st)
            else:
                call("ym_adamw_ema", tab.data_ptr(), ema_ptrs.data_ptr(), n, total, *hyp, norm.data_ptr(), omd, st)
        return run, n, total

    def ema_launch(ema, tag):
        key, tab, total, _ = ema._tables[tag]
        n = len(key) // 2                        # the key holds an (ema, src) pointer pair per entry
        return (lambda: call("ym_ema_update", tab.data_ptr(), n, total, omd, st)), n, total

    ta, n_par, total = tail(oa)
    tb, _, _ = tail(ob, ob._ema_ptrs[0][1])
    tc, _, _ = tail(oc)
    td, _, _ = tail(od)
    rest, n_rest, total_rest = ema_launch(eb, "rest")
    full, n_all, total_all = ema_launch(ec, "all")
    kernels = {"a": ta, "b": lambda: (tb(), rest()), "c": lambda: (tc(), full()), "d": lambda: (td(), foreach_ema())}

    stream = torch.cuda.current_stream(dev)
    times = {(kind, k): [] for kind in ("kernels_ms", "step_ms") for k in "abcd"}
    for rep in range(args.warmup + args.reps):
        for kind, fns in (("kernels_ms", kernels), ("step_ms", steps)):
            for k, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(args.inner):
                    fn()
                e1.record(stream)
                e1.synchronize()
                if rep >= args.warmup:
                    times[(kind, k)].append(e0.elapsed_time(e1) / args.inner)

    # the same launches after a 1 GiB fill has gone through the 256 MiB Infinity Cache: one call per event pair.
    # A training step reaches its tail like this (the backward before it streams gigabytes); the back-to-back
    # calls above find most of their ~0.2 GB working set still cached
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    for k in "abcd":
        times[("kernels_cold_ms", k)] = []
    for rep in range(args.warmup + args.reps):
        for k, fn in kernels.items():
            flush.fill_(float(rep))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if rep >= args.warmup:
                times[("kernels_cold_ms", k)].append(e0.elapsed_time(e1))

    def stat(v):
        return {"median": float(np.median(v)), "min": float(np.min(v)), "p90": float(np.percentile(v, 90))}
    res = {kind: {k: stat(times[(kind, k)]) for k in "abcd"} for kind in ("kernels_ms", "kernels_cold_ms", "step_ms")}
    # grad norm reads 4 B per parameter on top of the AdamW pass's 28
    byts = {"a": 32 * total, "b": 40 * total + 12 * total_rest, "c": 32 * total + 12 * total_all,
            "d": 32 * total + 20 * total_all}
    km = {k: res["kernels_ms"][k]["median"] for k in "abcd"}
    kc = {k: res["kernels_cold_ms"][k]["median"] for k in "abcd"}
    line = {"metric": "optimizer_tail_ms", "scale": args.scale, "parameters_stepped": total, "tensors_stepped": n_par,
            "ema_entries": n_all, "ema_elements": total_all, "rest_entries": n_rest, "rest_elements": total_rest,
            "reps": args.reps, "inner": args.inner, **res, "bytes": byts,
            "kernels_gb_per_s": {k: byts[k] / km[k] / 1e6 for k in "abcd"},
            "kernels_cold_gb_per_s": {k: byts[k] / kc[k] / 1e6 for k in "abcd"},
            "b_over_c_kernels": km["b"] / km["c"], "b_over_a_kernels": km["b"] / km["a"],
            "b_over_c_kernels_cold": kc["b"] / kc["c"], "b_over_a_kernels_cold": kc["b"] / kc["a"],
            "b_over_c_step": res["step_ms"]["b"]["median"] / res["step_ms"]["c"]["median"],
            "b_over_a_step": res["step_ms"]["b"]["median"] / res["step_ms"]["a"]["median"]}
    print(json.dumps(line))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
