"""What yolomi/graph.py plans and launches, recorded on the host (no GPU needed).

A Plan built on torch.device("cpu") lowers the module tree exactly as on the GPU: the buffers are host tensors and
the library's selection queries are host code.  With four stand-ins installed in THIS process only (a recorder for
graph.call, a constant for graph.stream_ptr, dummies for torch.cuda.current_stream and torch.cuda.stream),
plan.forward() and plan.backward() run to completion and leave the exact sequence of library calls with every
scalar argument.  Per configuration (CONFIGS) the tool records

  ops        class name, the views the op holds as (buffer index, c0, c, H, W) under their attribute names, and
             rw(plan, phase) of both phases with Act ids replaced by the buffer's index in plan.acts;
  schedule   for K = 3 streams and both phases: the stream of every op, the ops it waits on, the ops that record
             an event;
  trace      one forward and, for training plans, one backward at K = 1: [name, arg, ...] per call.  Ints, floats
             and None as they are; a ctypes reference as "ref"; an integer at or above 2^36 (a pointer) as p<k>,
             k the order of first appearance of that value in the configuration's trace.

tests/golden/plan_trace.json holds the record; tests/test_plan_trace_cpu.py recomputes it, so a change to graph.py
that moves, adds, drops or re-orders a launch, changes an argument, a buffer slice or the stream schedule fails
there.  The SPPF configuration `sppf_unfused` is a 48x48 map, which ym_sppf_supported (a host query) refuses, so
the one-launch-per-pool fallback is traced too.

    python tools/plan_trace.py --check            # compare graph.py with the golden file
    python tools/plan_trace.py --write            # regenerate it (only when a change of the plan is intended)
"""
from __future__ import annotations

import argparse
import contextlib
import ctypes
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "plan_trace.json"
for _p in (str(ROOT), str(ROOT / "yolo-scratch_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# (name, kind, arguments): whole models as (scale, image planes, training, batch, size); blocks as (module, its
# constructor arguments, input (B, C, H, W), input_requires_grad); Detect as (nc, level channels, level maps, batch)
CONFIGS = [
    ("model_n_train", "model", ("n", 1, True, 2, 64)),
    ("model_n_train_3planes", "model", ("n", 3, True, 2, 64)),
    ("model_s_eval", "model", ("s", 1, False, 1, 96)),
    ("block_stem", "block", ("Conv", (1, 16, 3, 2), (2, 1, 32, 32), False)),
    ("block_c3k2", "block", ("C3k2", (32, 64, 1, True), (2, 32, 16, 16), False)),
    ("block_c3k2_dx", "block", ("C3k2", (32, 64, 1, True), (2, 32, 16, 16), True)),
    ("block_sppf", "block", ("SPPF", (64, 64), (2, 64, 8, 8), False)),
    ("block_sppf_dx", "block", ("SPPF", (64, 64), (2, 64, 8, 8), True)),
    ("block_c2psa", "block", ("C2PSA", (128, 128), (2, 128, 8, 8), False)),
    ("block_c2psa_dx", "block", ("C2PSA", (128, 128), (2, 128, 8, 8), True)),
    ("sppf_unfused", "block", ("SPPF", (16, 16), (1, 16, 48, 48), True)),
    ("detect", "detect", (5, (32, 64, 128), ((8, 8), (4, 4), (2, 2)), 2)),
]
K_SCHEDULE = 3
_BYREF = type(ctypes.byref(ctypes.c_int()))


# ----------------------------------------------------------------------------- stand-ins
class _Stream:
    cuda_stream = 0


@contextlib.contextmanager
def recording(trace):
    """graph.call records into `trace` and launches nothing; the three stream lookups a CPU plan makes answer a
    dummy.  Everything is put back on exit."""
    import torch
    from yolomi import graph as G
    labels = {}

    def rec(name, *args):
        row = [name]
        for v in args:
            if v is None or isinstance(v, float):
                row.append(v)
            elif isinstance(v, int):
                row.append(f"p{labels.setdefault(v, len(labels))}" if v >= 1 << 36 else int(v))
            elif isinstance(v, _BYREF):
                row.append("ref")
            else:
                raise TypeError(f"{name}: argument of type {type(v).__name__}")
        trace.append(row)

    saved = (G.call, G.stream_ptr, torch.cuda.current_stream, torch.cuda.stream)
    G.call, G.stream_ptr = rec, lambda dev: 0
    torch.cuda.current_stream = lambda dev=None: _Stream()
    torch.cuda.stream = lambda s: contextlib.nullcontext()
    try:
        yield
    finally:
        G.call, G.stream_ptr, torch.cuda.current_stream, torch.cuda.stream = saved


# ----------------------------------------------------------------------------- plans
def _model_plan(scale, ch, training, B, S):
    import torch
    import yaml
    from models import build_yolo11
    from yolomi import graph as G
    cfg = yaml.safe_load((ROOT / "yolo-scratch_amd" / "configs" / "yolo11n_crater.yaml").read_text())
    cfg["scale"] = scale
    model = build_yolo11(cfg, ch=ch, nc=5).train(training)
    plan = G.lower_model(G.Plan(model, B, S, S, torch.device("cpu"), training, "model"), model, (B, S, S))
    plan.img = torch.zeros(B, ch, S, S)
    return plan


def _block_plan(cls, args, shape, requires_grad):
    import torch
    import models
    from yolomi import graph as G
    plan = G.block_plan(getattr(models, cls)(*args).train(), shape, torch.device("cpu"), requires_grad)
    if not plan.inputs:
        plan.img = torch.zeros(shape)
    return plan


def _detect_plan(nc, chans, maps, B):
    import torch
    from models import Detect
    from yolomi import graph as G
    shapes = [(B, c, h, w) for c, (h, w) in zip(chans, maps)]
    return G.detect_plan(Detect(nc, chans).train(), shapes, torch.device("cpu"))


# ----------------------------------------------------------------------------- the record
def _views(op, idx):
    from yolomi.graph import View
    out = {}
    for name, v in sorted(vars(op).items()):
        vs = [v] if isinstance(v, View) else [e for e in v if isinstance(e, View)] if isinstance(v, list) else []
        if vs:
            out[name] = [[idx[id(e.act)], e.c0, e.c, e.H, e.W] for e in vs]
    return out


def _rw(op, plan, phase, idx):
    return [[[k[0], idx[k[1]] if k[0] in ("a", "g") else k[1], *k[2:]] for k in keys] for keys in op.rw(plan, phase)]


def record(name, kind, args):
    import torch
    plan = {"model": _model_plan, "block": _block_plan, "detect": _detect_plan}[kind](*args)
    idx = {id(a): i for i, a in enumerate(plan.acts)}
    out = {"buffers": [[a.C, a.H, a.W] for a in plan.acts],
           "ops": [[type(op).__name__, _views(op, idx), _rw(op, plan, "fwd", idx), _rw(op, plan, "bwd", idx)]
                   for op in plan.ops],
           "schedule": {}, "trace": {}}
    for phase, ops in (("fwd", plan.ops), ("bwd", list(reversed(plan.ops)))):
        sched, need = plan._schedule(ops, phase, K_SCHEDULE)
        out["schedule"][phase] = {"stream": [s for s, _ in sched], "waits": [list(w) for _, w in sched],
                                  "events": sorted(need)}
    trace = []
    with recording(trace):
        plan.forward()
        n = len(trace)
        if plan.training:
            if plan.head is not None:
                plan.dhead = torch.zeros_like(plan.head)
            plan.backward()
    out["trace"]["fwd"], out["trace"]["bwd"] = trace[:n], trace[n:]
    return out


def record_all():
    import torch
    torch.manual_seed(0)
    return {name: record(name, kind, args) for name, kind, args in CONFIGS}


def first_difference(got, want):
    """None, or a sentence naming the first entry that differs: configuration, phase, call index and argument."""
    if list(got) != list(want):
        return f"configurations differ: got {list(got)}, golden {list(want)}"
    for cfg in got:
        g, w = got[cfg], want[cfg]
        if g["buffers"] != w["buffers"]:
            return f"{cfg}: activation buffers differ: got {g['buffers']}, golden {w['buffers']}"
        for i, (a, b) in enumerate(zip(g["ops"], w["ops"])):
            if a != b:
                return f"{cfg}: op {i}: got {a}, golden {b}"
        if len(g["ops"]) != len(w["ops"]):
            return f"{cfg}: {len(g['ops'])} ops, golden {len(w['ops'])}"
        for phase in ("fwd", "bwd"):
            for key in ("stream", "waits", "events"):
                a, b = g["schedule"][phase][key], w["schedule"][phase][key]
                if a != b:
                    i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
                    return f"{cfg}: {phase} schedule: {key}[{i}]: got {a[i:i + 1]}, golden {b[i:i + 1]}"
            a, b = g["trace"][phase], w["trace"][phase]
            for i, (x, y) in enumerate(zip(a, b)):
                if x != y:
                    j = next((j for j, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
                    return (f"{cfg}: {phase} call {i} ({y[0]}): argument {j}: got {x[j:j + 1]}, golden {y[j:j + 1]}"
                            if j else f"{cfg}: {phase} call {i}: got {x[0]}, golden {y[0]}")
            if len(a) != len(b):
                return f"{cfg}: {phase}: {len(a)} calls, golden {len(b)}"
    return None


def dump(rec, path):
    """One op / call per line: a changed launch shows as a changed line in the golden file's diff."""
    lines = ["{"]
    for ci, (cfg, r) in enumerate(rec.items()):
        lines.append(f' {json.dumps(cfg)}: {{')
        lines.append(f'  "buffers": {json.dumps(r["buffers"])},')
        lines.append('  "ops": [')
        lines += [f"   {json.dumps(op)}{',' if i + 1 < len(r['ops']) else ''}" for i, op in enumerate(r["ops"])]
        lines.append("  ],")
        lines.append(f'  "schedule": {json.dumps(r["schedule"])},')
        lines.append('  "trace": {')
        for phase in ("fwd", "bwd"):
            t = r["trace"][phase]
            lines.append(f'   "{phase}": [')
            lines += [f"    {json.dumps(c)}{',' if i + 1 < len(t) else ''}" for i, c in enumerate(t)]
            lines.append("   ]," if phase == "fwd" else "   ]")
        lines.append("  }")
        lines.append(" }," if ci + 1 < len(rec) else " }")
    lines.append("}")
    Path(path).write_text("\n".join(lines) + "\n")


def load(path):
    return json.loads(Path(path).read_text())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--check", action="store_true", help="compare what graph.py plans and launches with the golden file")
    g.add_argument("--write", action="store_true", help="write the golden file from graph.py")
    ap.add_argument("--golden", default=str(GOLDEN))
    a = ap.parse_args()
    rec = json.loads(json.dumps(record_all()))
    for cfg, r in rec.items():
        print(f"{cfg}: {len(r['buffers'])} buffers, {len(r['ops'])} ops, {len(r['trace']['fwd'])} forward and "
              f"{len(r['trace']['bwd'])} backward calls")
    if a.write:
        dump(rec, a.golden)
        print(f"wrote {a.golden}")
        return 0
    diff = first_difference(rec, load(a.golden))
    print(diff or "identical to the golden file")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
