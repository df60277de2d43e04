"""The execution plan is pinned: for the configurations of tools/plan_trace.py, yolomi/graph.py lowers the module
tree to the op list, the buffer slices and the read / write ranges that tests/golden/plan_trace.json records,
schedules them over three streams as recorded, and one forward and one backward issue the recorded library calls, in
order, with every scalar argument (pointers by order of first appearance).  No GPU: the plan is built on the host and
the launches are recorded, not made.  Zero mismatches: a refactor of graph.py must leave the golden file alone; a
change that means to move a launch regenerates it (python tools/plan_trace.py --write) and shows the moved lines
in its diff."""
import importlib.util
import inspect
import json
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
ENTRY_POINTS = ("ym_conv_fwd_bn", "ym_conv_fwd_eval", "ym_bn_bwd_apply_res", "ym_stem_bwd_wgrad_stored",
                "ym_conv_first_wgrad", "ym_dw3x3_bwd", "ym_attn_bwd", "ym_sppf_bwd", "ym_head_grad", "ym_upsample2_bwd",
                # the paths the configurations were chosen for: the per-op eval coefficients, SPPF's fp32 copy in eval
                # (the one ym_bn_apply of an eval plan) and the per-pool fallback
                "ym_bn_eval_coeff", "ym_bn_apply", "ym_maxpool5_f32_fwd", "ym_maxpool5_f32_bwd")


@pytest.fixture(scope="module")
def traces():
    spec = importlib.util.spec_from_file_location("plan_trace", ROOT / "tools" / "plan_trace.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, json.loads(json.dumps(mod.record_all())), mod.load(mod.GOLDEN)


def test_plan_trace_matches_golden(traces):
    mod, got, want = traces
    diff = mod.first_difference(got, want)
    if diff is not None:
        print(diff)
    assert diff is None, diff
    assert got == want


def test_schedule_is_a_function_of_the_ranges_and_the_stream_count(traces):
    """graph.schedule on its own, with no plan: fed the recorded read / write ranges it returns the recorded schedule;
    on one stream nothing waits; and every dependency (a range written before, or read before and written now) is
    either on the op's own stream or covered by a wait on a later-or-equal op of the dependency's stream."""
    _, _, want = traces
    from yolomi.graph import _overlap, schedule
    for cfg, r in want.items():
        for phase, col in (("fwd", 2), ("bwd", 3)):
            ops = r["ops"] if phase == "fwd" else r["ops"][::-1]
            rws = [([tuple(k) for k in op[col][0]], [tuple(k) for k in op[col][1]]) for op in ops]
            sched, need = schedule(rws, 3)
            rec = r["schedule"][phase]
            assert [s for s, _ in sched] == rec["stream"] and [w for _, w in sched] == rec["waits"], (cfg, phase)
            assert sorted(need) == rec["events"], (cfg, phase)
            one, none = schedule(rws, 1)
            assert one == [(0, [])] * len(rws) and not none, (cfg, phase)
            for i, (R, W) in enumerate(rws):
                s, waits = sched[i]
                for j in range(i):
                    Rj, Wj = rws[j]
                    if any(_overlap(a, b) for a in R + W for b in Wj) or any(_overlap(a, b) for a in W for b in Rj):
                        sj = sched[j][0]
                        assert sj == s or any(w >= j and sched[w][0] == sj for w in waits), (cfg, phase, i, j)
                assert all(w in need for w in waits), (cfg, phase, i)


def test_plan_trace_covers_every_op_class_and_entry_point(traces):
    """The golden file is not empty of what it is meant to pin: every op class of graph.py occurs, every listed
    entry point is called, the K = 3 schedule uses all three streams in both phases, and the eval plan takes the
    one-launch conv route with exactly one separate BatchNorm apply (SPPF's cv1)."""
    _, _, want = traces
    from yolomi import graph as G
    classes = {n for n, c in inspect.getmembers(G, inspect.isclass)
               if c.__module__ == G.__name__ and hasattr(c, "forward") and hasattr(c, "rw")}
    assert classes == {"ConvBN", "StemConvBN", "DWConvBN", "AttnCore", "SPPFPools", "Upsample2", "Copy", "HeadLevel"}
    assert classes == {op[0] for r in want.values() for op in r["ops"]}
    called = {c[0] for r in want.values() for phase in ("fwd", "bwd") for c in r["trace"][phase]}
    assert not [e for e in ENTRY_POINTS if e not in called]
    for cfg in ("model_n_train", "model_n_train_3planes"):
        for phase in ("fwd", "bwd"):
            assert set(want[cfg]["schedule"][phase]["stream"]) == {0, 1, 2}, (cfg, phase)
            assert want[cfg]["schedule"][phase]["events"], (cfg, phase)
    names = [c[0] for c in want["model_s_eval"]["trace"]["fwd"]]
    assert names.count("ym_bn_apply") == 1 and names.count("ym_conv_fwd_eval") >= 50, names
    assert not want["model_s_eval"]["trace"]["bwd"]
    assert "ym_stem_bwd_wgrad_stored" in [c[0] for c in want["model_n_train"]["trace"]["bwd"]]
    assert "ym_conv_first_wgrad" in [c[0] for c in want["model_n_train_3planes"]["trace"]["bwd"]]
    assert "ym_sppf_fwd" not in [c[0] for c in want["sppf_unfused"]["trace"]["fwd"]]
