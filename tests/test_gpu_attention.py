"""The attention core on its own, at the C ABI (ym_attn_fwd, ym_attn_workspace_size, ym_attn_bwd), against the fp64
reference and the rounding budgets of tests/attention_ref.py: out / lse of the forward, dq / dk / dv of the backward fed
the reference's out and lse (a failure is the backward's own), the two chained at the tail shapes.

Every buffer is a Guarded view (test_gpu_elementwise.py).  Outputs hold NaN where a kernel must write and the
sentinel elsewhere: afterwards no NaN is left inside (the checker fails on one) and everything outside the addressed
channels and rows is bit-identical.  Inputs hold the NaN pattern outside their view — guard rows, the rows between
two images, the columns beyond the head channels — so a read past row N or into a neighbouring channel poisons the
result; they are compared whole with a snapshot afterwards.

The shapes are the ones at which the tile arithmetic changes (attention_ref.SHAPES), not the networks' shapes —
tests/test_gpu_layers.py covers those.  The largest slack each output used is collected per output and mode; with
YM_ATTENTION_SLACK_OUT=<path> the table is written there (profiles/attention/slack.txt is such a run).
"""
import os

import pytest
import torch

import attention_ref as AR
import elementwise_ref as ER
from test_gpu_elementwise import Guarded, _NAN, _abi, _dev

pytestmark = pytest.mark.gpu

SLACK = {}
CASES = [(s, g) for s in AR.SHAPES for g in AR.GENERATORS]
ERR_ARG = -1


def _record(name, used):
    SLACK[name] = max(SLACK.get(name, 0.0), used)


@pytest.fixture(scope="module", autouse=True)
def _slack_table():
    yield
    lines = [f"{k:<44s} {v:8.3f}" for k, v in sorted(SLACK.items())]
    head = ("# largest slack used over tests/test_gpu_attention.py, per output and mode.  out / dq / dk / dv: (|got - ref| - 0.5\n"
            "# ulp16 - floor) / (lead * terms_abs), lead = 2^-11 / 3 * 2^-8 / 3 * 2^-8 / 2^-8; the budget in these units is\n"
            "# 1 + K * 2^-24 / lead.  lse: |got - ref| / (2^-24 * (1 + |m| + |log l| + Labs)); the budget is K_LSE = %d\n"
            "# (tests/attention_ref.py)\n" % AR.K_LSE)
    print("\n" + head + "\n".join(lines))
    path = os.environ.get("YM_ATTENTION_SLACK_OUT")
    if path and lines:
        with open(path, "w") as f:
            f.write(head + "\n".join(lines) + "\n")


def _input(data, kind, ld, off, n, gap):
    """An input view (B * N rows of `data`) inside NaN: guard rows, gap rows and the columns outside the view."""
    rows, c = data.shape[0] * data.shape[1], data.shape[2]
    g = Guarded(rows, ld, kind, c=c, off=off, data=data.reshape(rows, c), n=n, gap=gap)
    mask = torch.ones_like(g.raw, dtype=torch.bool)
    mask[g.ridx, g.cols] = False
    g.raw[mask] = _NAN[kind]
    return g.snapshot()


def _flat32(numel, data=None):
    """A guarded fp32 vector (lse, the workspace)."""
    return Guarded(1, numel + 8, "f32", c=numel, off=0, data=None if data is None else data.reshape(1, numel))


# view layouts: (qkv ld extra, qkv channel offset, qkv gap rows, out ld extra, out channel offset, out gap rows)
DENSE = (0, 0, 0, 0, 0, 0)
PADDED = (24, 8, 1, 12, 4, 2)          # the out view at a 4-element offset, o_ld a multiple of 4 only


def _forward(qkv, heads, scale, layout, key_dim=AR.KD, head_dim=AR.HD):
    """-> (qkv view, out view, lse vector) after one ym_attn_fwd."""
    call, lib, st = _abi()
    B, N, C = qkv.shape
    qx, qo, qg, ox, oo, og = layout
    x = _input(qkv, "fp16", C + qx, qo, B, qg)
    out = Guarded(B * N, heads * AR.HD + ox, "fp16", c=heads * AR.HD, off=oo, n=B, gap=og)
    lse = _flat32(B * heads * N)
    call("ym_attn_fwd", x.ptr, x.bs, x.ld, B, heads, N, key_dim, head_dim, scale, out.ptr, out.bs, out.ld, lse.ptr, st)
    torch.cuda.synchronize()
    return x, out, lse


def _check_forward(qkv, heads, scale, layout, what, mode):
    B, N, _ = qkv.shape
    x, out, lse = _forward(qkv, heads, scale, layout)
    ref = AR.attn_ref(qkv, heads, scale)
    u_out, u_lse = AR.check_forward(out.inner().reshape(B, N, -1), lse.inner().reshape(B, heads, N), ref, N, what)
    _record(f"out {mode}", u_out)
    _record(f"lse {mode}", u_lse)
    out.check_untouched(what + " out")
    lse.check_untouched(what + " lse")
    x.check_untouched(what + " qkv")
    return out, lse


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("shape,gen", CASES)
def test_forward(shape, gen):
    """out within half an fp16 ulp + (2^-11 + K 2^-24) * softmax @ |v| + N 2^-25 max|v| of fp64, lse within K_LSE units,
    from dense views and from padded ones (q_ld = heads * 128 + 24 at channel offset 8 with a row between the images;
    the out view at channel offset 4 of o_ld = heads * 64 + 12 with two rows between the images)."""
    B, heads, N = shape
    qkv = AR.make_inputs(gen, B, heads, N)[0].to(_dev())
    for name, layout in (("dense", DENSE), ("padded", PADDED)):
        _check_forward(qkv, heads, AR.SCALE, layout, f"ym_attn_fwd {shape} {gen} {name}", "forward")


@pytest.mark.parametrize("scale", [AR.SCALE, 0.25, 1.0])
def test_forward_scale(scale):
    shape = (2, 2, 65)
    for gen in ("gauss", "rising"):
        qkv = AR.make_inputs(gen, *shape, scale=scale)[0].to(_dev())
        _check_forward(qkv, 2, scale, PADDED, f"ym_attn_fwd {shape} {gen} scale={scale}", "forward")


# ------------------------------------------------------------------------------------------------ backward
def _backward(qkv, dout, out16, lse32, heads, scale, acc=(0, 0, 0), prior=None, padded=True):
    """One ym_attn_bwd on guarded views; dout on strides different from out's.  -> (dqkv (B, N, C) bf16, the guarded
    buffers to check)."""
    call, lib, st = _abi()
    B, N, C = qkv.shape
    p = 1 if padded else 0
    x = _input(qkv, "fp16", C + 24 * p, 8 * p, B, p)
    o = _input(out16, "fp16", heads * AR.HD + 16 * p, 8 * p, B, 2 * p)
    d = _input(dout, "bf16", heads * AR.HD + 8, 0, B, 1)
    lse = _flat32(B * heads * N, lse32.contiguous()).snapshot()
    nws = lib().ym_attn_workspace_size(B, heads, N)
    assert nws == B * heads * N * 4
    ws = _flat32(nws // 4)
    data = None
    if any(acc):            # the seeded prior where the flag is set, NaN where the kernel must overwrite
        data = prior.clone().to(_dev())
        keep = torch.cat([torch.full((AR.KD,), bool(acc[0])), torch.full((AR.KD,), bool(acc[1])),
                          torch.full((AR.HD,), bool(acc[2]))]).repeat(heads).to(_dev())
        data[..., ~keep] = float("nan")
        data = data.reshape(B * N, C)
    g = Guarded(B * N, C + 12 * p, "bf16", c=C, off=4 * p, data=data, n=B, gap=3 * p)
    call("ym_attn_bwd", x.ptr, x.bs, x.ld, o.ptr, o.bs, o.ld, d.ptr, d.bs, d.ld, lse.ptr, B, heads, N, scale, ws.ptr,
         g.ptr, g.bs, g.ld, acc[0], acc[1], acc[2], st)
    torch.cuda.synchronize()
    return g.inner().reshape(B, N, C), (x, o, d, lse, ws, g)


def _check_backward(qkv, dout, out16, lse32, heads, scale, what, mode, acc=(0, 0, 0), prior=None, padded=True):
    B, N, _ = qkv.shape
    got, bufs = _backward(qkv, dout, out16, lse32, heads, scale, acc, prior, padded)
    ref = AR.attn_ref(qkv, heads, scale, dout, out16)
    used = AR.check_backward(got, ref, heads, N, prior=None if prior is None else prior.to(_dev()), acc=acc, what=what)
    for k, v in used.items():
        _record(f"{k} {mode}", v)
    ws = bufs[4]
    assert not bool(torch.isnan(ws.inner()).any()), what + ": workspace rows left unwritten"
    for b, name in zip(bufs, ("qkv", "out", "dout", "lse", "workspace", "dqkv")):
        b.check_untouched(f"{what} {name}")
    return got


def _reference_out_lse(qkv, heads, scale):
    ref = AR.attn_ref(qkv, heads, scale)
    return ER.round16(ref["out"], "fp16"), ref["lse"].float()


@pytest.mark.parametrize("shape,gen", CASES)
def test_backward(shape, gen):
    """Fed the reference's out (rounded to fp16) and lse (fp32): dv within half a bf16 ulp + (2^-8 + K 2^-24) * P^T @ |dO|,
    dq / dk within half a bf16 ulp + (3 * 2^-8 + K 2^-24) * T_q / T_k of fp64, into a dqkv view of g_ld = heads * 128 + 12
    at channel offset 4 with three rows between the images; the workspace written in full and not past its size."""
    B, heads, N = shape
    qkv, dout = (t.to(_dev()) for t in AR.make_inputs(gen, B, heads, N))
    o16, l32 = _reference_out_lse(qkv, heads, AR.SCALE)
    _check_backward(qkv, dout, o16, l32, heads, AR.SCALE, f"ym_attn_bwd {shape} {gen}", "backward")


def test_backward_dense_and_scale():
    shape = (2, 2, 65)
    for scale in (0.25, 1.0):
        qkv, dout = (t.to(_dev()) for t in AR.make_inputs("gauss", *shape, scale=scale))
        o16, l32 = _reference_out_lse(qkv, 2, scale)
        _check_backward(qkv, dout, o16, l32, 2, scale, f"ym_attn_bwd {shape} dense scale={scale}", "backward",
                        padded=False)


@pytest.mark.parametrize("acc", [(0, 0, 0), (1, 1, 1), (1, 0, 1), (0, 1, 0)])
@pytest.mark.parametrize("shape", [(2, 2, 17), (2, 2, 65)])
def test_backward_accumulate_flags(shape, acc):
    """A seeded bf16 prior where a flag is set (it joins the reference before the one rounding), NaN where it is not
    (read there, it poisons the slice; cross-wired flags lose a prior and add a NaN)."""
    B, heads, N = shape
    qkv, dout = (t.to(_dev()) for t in AR.make_inputs("gauss", B, heads, N))
    o16, l32 = _reference_out_lse(qkv, heads, AR.SCALE)
    _check_backward(qkv, dout, o16, l32, heads, AR.SCALE, f"ym_attn_bwd {shape} acc={acc}", f"backward acc={acc}",
                    acc=acc, prior=AR.make_prior(B, heads, N))


@pytest.mark.parametrize("shape", AR.TAIL_SHAPES)
def test_chained(shape):
    """Forward, then the backward on the kernels' own out and lse: the same bounds (the reference takes D from the out
    the backward read; K counts the lse error)."""
    B, heads, N = shape
    for gen in ("gauss", "rising"):
        qkv, dout = (t.to(_dev()) for t in AR.make_inputs(gen, B, heads, N))
        what = f"chained {shape} {gen}"
        out, lse = _check_forward(qkv, heads, AR.SCALE, PADDED, what, "chained")
        _check_backward(qkv, dout, out.inner().reshape(B, N, -1), lse.inner().reshape(B, heads, N), heads, AR.SCALE,
                        what, "chained")


def test_bit_identical_runs():
    B, heads, N = shape = (3, 2, 129)
    qkv, dout = (t.to(_dev()) for t in AR.make_inputs("gauss", *shape))
    runs = []
    for _ in range(2):
        _, out, lse = _forward(qkv, heads, AR.SCALE, PADDED)
        o16, l32 = out.inner().reshape(B, N, -1), lse.inner().reshape(B, heads, N)
        runs.append((o16, l32, _backward(qkv, dout, o16, l32, heads, AR.SCALE)[0]))
    ER.assert_bits_equal(runs[0][0], runs[1][0], "out of two runs")
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32)), "lse of two runs"
    ER.assert_bits_equal(runs[0][2], runs[1][2], "dqkv of two runs")


# ------------------------------------------------------------------------------------------------ the edges of the ABI
def _small():
    """Buffers of a (2, 1, 4) problem, every one in snapshot mode: nothing may be written."""
    B, heads, N = 2, 1, 4
    qkv, dout = (t.to(_dev()) for t in AR.make_inputs("gauss", B, heads, N))
    x = _input(qkv, "fp16", AR.HS + 8, 0, B, 0)
    d = _input(dout, "bf16", AR.HD + 8, 0, B, 0)
    o16, l32 = _reference_out_lse(qkv, heads, AR.SCALE)
    o = _input(o16, "fp16", AR.HD + 8, 0, B, 0)
    out = Guarded(B * N, AR.HD + 8, "fp16", c=AR.HD, off=0, n=B).snapshot()
    lse = _flat32(B * heads * N, l32.contiguous()).snapshot()
    ws = _flat32(B * heads * N).snapshot()
    g = Guarded(B * N, AR.HS + 8, "bf16", c=AR.HS, off=0, n=B).snapshot()
    return (B, heads, N), x, d, o, out, lse, ws, g


def _fwd_status(x, out, lse, b, heads, n, kd=AR.KD, hd=AR.HD, q_ld=None, o_ld=None, o_bs=None, q_bs=None):
    _, lib, st = _abi()
    r = lib().ym_attn_fwd(x.ptr, x.bs if q_bs is None else q_bs, x.ld if q_ld is None else q_ld, b, heads, n, kd, hd,
                          AR.SCALE, out.ptr, out.bs if o_bs is None else o_bs, out.ld if o_ld is None else o_ld, lse.ptr,
                          st)
    torch.cuda.synchronize()
    return r, lib().ym_last_error().decode()


def _bwd_status(x, o, d, lse, ws, g, b, heads, n, **over):
    _, lib, st = _abi()
    s = {"q_bs": x.bs, "q_ld": x.ld, "o_bs": o.bs, "o_ld": o.ld, "d_bs": d.bs, "d_ld": d.ld, "g_bs": g.bs, "g_ld": g.ld}
    s.update(over)
    r = lib().ym_attn_bwd(x.ptr, s["q_bs"], s["q_ld"], o.ptr, s["o_bs"], s["o_ld"], d.ptr, s["d_bs"], s["d_ld"], lse.ptr,
                          b, heads, n, AR.SCALE, ws.ptr, g.ptr, s["g_bs"], s["g_ld"], 0, 0, 0, st)
    torch.cuda.synchronize()
    return r, lib().ym_last_error().decode()


@pytest.mark.parametrize("b,n", [(2, 0), (0, 4)])
def test_empty_calls_write_nothing(b, n):
    (B, heads, N), x, d, o, out, lse, ws, g = _small()
    assert _fwd_status(x, out, lse, b, heads, n)[0] == 0
    assert _bwd_status(x, o, d, lse, ws, g, b, heads, n)[0] == 0
    for buf in (x, d, o, out, lse, ws, g):
        buf.check_untouched(f"b={b} n={n}")


def test_workspace_size():
    _, lib, _ = _abi()
    for B, heads, N in AR.SHAPES + [(0, 2, 17), (2, 2, 0)]:
        assert lib().ym_attn_workspace_size(B, heads, N) == B * heads * N * 4


def test_refused_arguments_write_nothing():
    (B, heads, N), x, d, o, out, lse, ws, g = _small()
    for kd, hd in ((16, 64), (32, 32), (64, 64), (32, 128)):
        r, msg = _fwd_status(x, out, lse, B, heads, N, kd=kd, hd=hd)
        assert r == ERR_ARG and msg == f"ym_attn_fwd: only key_dim=32, head_dim=64 (got {kd}, {hd})", (r, msg)
    for over in ({"q_ld": x.ld + 4}, {"q_bs": x.bs + 4}, {"o_ld": out.ld + 2}, {"o_bs": out.bs + 2}):
        r, msg = _fwd_status(x, out, lse, B, heads, N, **over)
        assert r == ERR_ARG and msg == "ym_attn_fwd: view alignment", (over, r, msg)
    for over in ({"q_ld": x.ld + 4}, {"q_bs": x.bs + 4}, {"o_ld": o.ld + 4}, {"o_bs": o.bs + 4}, {"d_ld": d.ld + 4},
                 {"d_bs": d.bs + 4}, {"g_ld": g.ld + 2}, {"g_bs": g.bs + 2}):
        r, msg = _bwd_status(x, o, d, lse, ws, g, B, heads, N, **over)
        assert r == ERR_ARG and msg == "ym_attn_bwd: view alignment", (over, r, msg)
    for buf in (x, d, o, out, lse, ws, g):
        buf.check_untouched("refused call")
