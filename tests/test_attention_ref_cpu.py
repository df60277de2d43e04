"""tests/attention_ref.py on its own, no GPU: the fp64 reference against torch autograd of the plain formula, the
generators' closed forms, the budgets against a rounding-order emulation of the kernels (K = 0: the leading constants
alone have to carry a faithful implementation, or a GPU failure would prove nothing), and the checker against planted
faults — each one a way attn.hip goes subtly wrong that a whole-tensor 1e-2 cannot see, each rejected on a NAMED
(shape, generator) case of SHAPES by at least 4 times the budget, which shows the shapes and inputs are enough.
"""
import math

import pytest
import torch

import attention_ref as AR
from elementwise_ref import round16

CASES = [(s, g) for s in AR.SHAPES for g in AR.GENERATORS]
WORST = {}


def _case(shape, gen, scale=AR.SCALE):
    B, heads, N = shape
    qkv, dout = AR.make_inputs(gen, B, heads, N, scale=scale)
    return qkv, dout


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("shape", [(2, 2, 17), (1, 3, 63), (2, 2, 65)])
@pytest.mark.parametrize("gen", ["gauss", "peaked", "rising"])
def test_ref_equals_autograd(shape, gen):
    B, heads, N = shape
    qkv, dout = _case(shape, gen)
    x = qkv.double().requires_grad_(True)
    q, k, v = AR.split_heads(x, heads)
    s = q @ k.transpose(-1, -2) * AR.f32(AR.SCALE)
    out = AR.merge_heads(torch.softmax(s, -1) @ v)
    (gx,) = torch.autograd.grad(out, x, grad_outputs=dout.double())
    out, s = out.detach(), s.detach()
    r = AR.attn_ref(qkv, heads, AR.SCALE, dout)
    assert float((r["out"] - out).abs().max()) < 1e-12
    assert float((r["dqkv"] - gx).abs().max()) < 1e-12 * max(1.0, float(gx.abs().max()))
    assert float((r["lse"] - torch.logsumexp(s, -1)).abs().max()) < 1e-12
    for name in ("out", "dqkv"):            # the terms bound the results they add up to
        assert bool((r["terms"][name] >= r[name].abs() - 1e-12).all())


def test_ref_takes_d_from_the_stored_out():
    """Given out16, D = sum dO * out16: dq / dk move, dv does not."""
    qkv, dout = _case((2, 2, 17), "gauss")
    a = AR.attn_ref(qkv, 2, AR.SCALE, dout)
    o16 = round16(a["out"], "fp16")
    b = AR.attn_ref(qkv, 2, AR.SCALE, dout, o16)
    assert torch.equal(AR.part(a["dqkv"], 2, "dv"), AR.part(b["dqkv"], 2, "dv"))
    d = float((AR.part(a["dqkv"], 2, "dq") - AR.part(b["dqkv"], 2, "dq")).abs().max())
    assert 0 < d < 1e-2


@pytest.mark.parametrize("shape", [(2, 1, 15), (2, 2, 65)])
def test_flat_closed_forms(shape):
    """q = 0: P = 1 / N exactly, out the mean of v, lse = log N, dk = 0 (it is q^T dS), dv_j the mean of dO, and
    dq_i = scale / N * sum_j (dO_i . (v_j - mean v)) k_j."""
    B, heads, N = shape
    qkv, dout = _case(shape, "flat")
    r = AR.attn_ref(qkv, heads, AR.SCALE, dout)
    q, k, v = (t.double() for t in AR.split_heads(qkv, heads))
    assert float(q.abs().max()) == 0.0
    assert float((r["P"] - 1.0 / N).abs().max()) < 1e-15
    assert float((r["out"] - AR.merge_heads(v.mean(2, keepdim=True).expand_as(v))).abs().max()) < 1e-12
    assert float((r["lse"] - math.log(N)).abs().max()) < 1e-12
    assert float(AR.part(r["dqkv"], heads, "dk").abs().max()) == 0.0
    dO = dout.double().reshape(B, N, heads, AR.HD).permute(0, 2, 1, 3)
    want_dv = AR.merge_heads(dO.mean(2, keepdim=True).expand_as(dO)).reshape(B, N, heads, AR.HD)
    assert float((AR.part(r["dqkv"], heads, "dv") - want_dv).abs().max()) < 1e-12
    want_dq = AR.f32(AR.SCALE) / N * (dO @ (v - v.mean(2, keepdim=True)).transpose(-1, -2)) @ k
    assert float((AR.part(r["dqkv"], heads, "dq") - want_dq.permute(0, 2, 1, 3)).abs().max()) < 1e-12


def test_generators_do_what_they_say():
    for shape in AR.SHAPES:
        B, heads, N = shape
        r = {g: AR.attn_ref(_case(shape, g)[0], heads, AR.SCALE) for g in AR.GENERATORS}
        s = {g: torch.log(r[g]["P"]) + r[g]["lse"][..., None] for g in r}
        assert bool((s["last_key"].argmax(-1) == N - 1).all()), shape
        if N > AR.TILE:     # the maximum of every 64-key tile exceeds the last one's / is below the first one's
            tmax = lambda x: torch.stack([x[..., k0:k0 + AR.TILE].max(-1).values for k0 in range(0, N, AR.TILE)], -1)
            assert bool((tmax(s["rising"]).diff(dim=-1) > 0).all()), shape
            assert bool((tmax(s["falling"]).diff(dim=-1) < 0).all()), shape
        if N >= 15:
            assert float(r["peaked"]["P"].max(-1).values.median()) > 0.65 and r["peaked"]["E"] > 40
            assert float(r["gauss"]["P"].max(-1).values.median()) < 0.5
    # seeded: the same call gives the same bits
    assert torch.equal(AR.make_inputs("gauss", 2, 2, 17)[0], AR.make_inputs("gauss", 2, 2, 17)[0])


# ------------------------------------------------------------------------------------------------ the budget
@pytest.mark.parametrize("shape,gen", CASES)
def test_budget_met_by_emulation_without_fp32_term(shape, gen):
    """The unmutated emulation, forward and backward chained on its own out / lse, passes with K = 0."""
    B, heads, N = shape
    qkv, dout = _case(shape, gen)
    e = AR.emulate(qkv, heads, AR.SCALE, dout)
    ref = AR.attn_ref(qkv, heads, AR.SCALE, dout, e["out"])
    what = f"emulate {shape} {gen}"
    u_out, u_lse = AR.check_forward(e["out"], e["lse"], ref, N, what, K=0)
    used = AR.check_backward(e["dqkv"], ref, heads, N, what=what, K=0)
    for k, val in {"out": u_out, "lse": u_lse, **used}.items():
        WORST[k] = max(WORST.get(k, 0.0), val)


@pytest.mark.parametrize("acc", [(1, 1, 1), (1, 0, 1), (0, 1, 0)])
def test_budget_met_by_emulation_with_prior(acc):
    shape, (B, heads, N) = (2, 2, 17), (2, 2, 17)
    qkv, dout = _case(shape, "gauss")
    prior = AR.make_prior(B, heads, N)
    e = AR.emulate(qkv, heads, AR.SCALE, dout, prior=prior, acc=acc)
    ref = AR.attn_ref(qkv, heads, AR.SCALE, dout, e["out"])
    AR.check_backward(e["dqkv"], ref, heads, N, prior=prior, acc=acc, what=f"emulate acc={acc}", K=0)


def test_print_worst_slack():
    """Runs after the budget cases: the largest slack the emulation used, in units of the leading constants (lse in
    units of 2^-24 * its terms, budget K_LSE)."""
    print("\nlargest slack used by the emulation at K = 0: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
    assert all(v <= 1.0 for k, v in WORST.items() if k != "lse")
    assert WORST.get("lse", 0.0) <= AR.K_LSE


# ------------------------------------------------------------------------------------------------ the mutants
# mutation -> ((B, heads, N), generator, the output it must break, extra emulate() arguments)
MUTANT_CASES = {
    "pad_zero_key": ((2, 2, 17), "gauss", "out", {}),
    "drop_last_key": ((2, 2, 17), "last_key", "out", {}),
    "no_alpha": ((3, 2, 129), "rising", "out", {}),
    "lse_no_max": ((2, 2, 65), "gauss", "lse", {}),
    "dk_unscaled": ((2, 2, 17), "gauss", "dk", {}),
    "dq_scaled_twice": ((2, 2, 17), "gauss", "dq", {}),
    "swap_qk": ((2, 2, 17), "gauss", "out", {}),
    "head_xor": ((2, 2, 65), "gauss", "out", {}),
    "d_other_head": ((2, 2, 65), "gauss", "dq", {}),
    "acc_cross": ((2, 2, 17), "gauss", "dk", {"acc": (1, 0, 1)}),
    "acc_ignores_flag": ((2, 2, 65), "gauss", "dq", {"acc": (0, 1, 0)}),
    "last_row_unwritten": ((2, 2, 65), "gauss", "dv", {}),
    "gap_ignored": ((2, 2, 17), "gauss", "out", {"gap": 2}),
}


def _ratios(e, ref, heads, N, prior, acc):
    """|err| / budget of every output of an emulate() result, under the full budgets the GPU tests use."""
    K = AR.k_fwd(N, ref["E"])
    r = {"out": AR.excess(e["out"], ref["out"], ref["terms"]["out"], "fp16", AR.LEAD["out"], K,
                          N * 2.0 ** -25 * ref["vmax"])[0],
         "lse": AR.lse_excess(e["lse"], ref) / AR.K_LSE}
    Kb = AR.k_bwd(N, ref["E"], float(ref["lse_terms"].max())) + 1
    want, terms = ref["dqkv"], ref["terms"]["dqkv"]
    for i, w in enumerate(("dq", "dk", "dv")):
        wv, tv = AR.part(want, heads, w), AR.part(terms, heads, w)
        if acc[i]:
            wv, tv = wv + AR.part(prior.double(), heads, w), tv + AR.part(prior.double().abs(), heads, w)
        r[w] = AR.excess(AR.part(e["dqkv"], heads, w), wv, tv, "bf16", AR.LEAD[w], Kb)[0]
    return r


def test_every_mutation_has_a_case():
    assert set(MUTANT_CASES) == set(AR.MUTATIONS)
    assert all(shape in AR.SHAPES and gen in AR.GENERATORS for shape, gen, _, _ in MUTANT_CASES.values())


@pytest.mark.parametrize("mutation", AR.MUTATIONS)
def test_mutant_rejected(mutation):
    """The standalone backward's setting: out / lse of the reference (rounded), as the GPU test feeds them."""
    shape, gen, broken, kw = MUTANT_CASES[mutation]
    B, heads, N = shape
    qkv, dout = _case(shape, gen)
    acc = kw.get("acc", (0, 0, 0))
    prior = AR.make_prior(B, heads, N)
    fill = AR.make_inputs("gauss", B, heads, kw["gap"], seed=99)[0] if "gap" in kw else None
    args = dict(prior=prior, acc=acc, gap=kw.get("gap", 0), gap_fill=fill)
    ref = AR.attn_ref(qkv, heads, AR.SCALE, dout, None)
    o16, l32 = round16(ref["out"], "fp16"), ref["lse"].float()
    ref = AR.attn_ref(qkv, heads, AR.SCALE, dout, o16)
    runs = {}
    for mut in (None, mutation):
        fwd = AR.emulate(qkv, heads, AR.SCALE, mutate=mut, **args)
        bwd = AR.emulate(qkv, heads, AR.SCALE, dout, o16, l32, mutate=mut, **args)
        runs[mut] = _ratios({"out": fwd["out"], "lse": fwd["lse"], "dqkv": bwd["dqkv"]}, ref, heads, N, prior, acc)
    print(f"\n{mutation} on {shape} {gen}: |err| / budget " + ", ".join(f"{k} {v:.3g}" for k, v in runs[mutation].items()))
    assert all(v <= 1.0 for v in runs[None].values()), runs[None]        # the case itself is clean
    assert runs[mutation][broken] >= 4.0, runs[mutation]


def test_peaked_does_not_see_a_leaked_zero_key():
    """Why both generators exist: with near one-hot rows exp(0 - m) is nothing, the leak hides."""
    shape, (B, heads, N) = (2, 2, 17), (2, 2, 17)
    qkv, _ = _case(shape, "peaked")
    ref = AR.attn_ref(qkv, heads, AR.SCALE)
    e = AR.emulate(qkv, heads, AR.SCALE, mutate="pad_zero_key")
    ratio = AR.excess(e["out"], ref["out"], ref["terms"]["out"], "fp16", AR.LEAD["out"], AR.k_fwd(N, ref["E"]),
                      N * 2.0 ** -25 * ref["vmax"])[0]
    assert ratio < 4.0
