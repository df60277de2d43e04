"""Every forward kernel instance ym_conv_fwd can launch against the integer result, bit for bit.

The cases, operands, buffers and the fp64 reference are tests/fwd_exact_cases.py's (its docstring has the argument:
fp16 integer operands of magnitude <= 16, every fp32 partial sum below 2^24, so the accumulator must equal conv2d in
fp64 BY VALUE and every output is a deterministic function of it); tests/test_fwd_exact_cpu.py shows on the host that
each case runs the instance it is listed for and meets the conditions of its runs.  Here, on one stream with one
synchronize per case:

  A  fp16 z + statistics: z = fp16(v) as bit patterns (ties in (2048, 4096) pin round to nearest even), the fp64 sum
     of the stat_sum rows == sum(v) exactly (and != sum(fp16(v)): the statistics are the accumulator's), stat_sq within
     the bound of an fp32 sum of pixels + 1 terms;
  S  operands in {-1, 0, 1}: z = v by value and BOTH statistics sums exact; the rows start as NaN (every row must be
     written, also by workgroups without a tile) and the canary row behind them must stay;
  the other outputs of fwd_exact_cases.OTHER: bf16, fp32, an integer bias, accumulate into fp32 and into bf16 in the
     form of the store path (E1 / E2), and the fp16 clamp;
  ym_conv_fwd_bn on one case per family; the ABI's edges (n = 0, the refusals).
x lives in a NaN-filled buffer (an over-read poisons the result), y in a buffer of sentinels that must come back
bit-unchanged, the weights and the bias in allocations of their exact size.  A failure names the first mismatching
(image, y, x, channel), got and want.
"""
import ctypes

import pytest
import torch

import fwd_exact_cases as F

pytestmark = pytest.mark.gpu


def _launch(c, run, out_f32=2, accumulate=0, bias=False, fill=None, stats=False, fn="ym_conv_fwd", fold=None):
    """Launches one run of case c on the current stream (under the caller's policy); returns the device tensors (kept
    alive by the caller until the synchronize) and the host copies of everything the kernel must leave alone."""
    from yolomi._lib import call, lib
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    r = dict(x_h=F.x_buffer(c, run), w_h=F.weight_buffer(c, run), y_h=F.y_buffer(c, out_f32, fill), out_f32=out_f32)
    r["x"], r["w"], r["y"] = r["x_h"].to(dev), r["w_h"].to(dev), r["y_h"].to(dev)
    d = F.desc(c, out_f32=out_f32, accumulate=accumulate)
    ss = sq = b = None
    if stats:
        r["rows"] = lib().ym_conv_fwd_stat_rows(ctypes.byref(d))
        r["st_h"] = F.stat_buffer(r["rows"], c.cout)
        r["ss"], r["sq"] = r["st_h"].to(dev), r["st_h"].to(dev)
        ss, sq = r["ss"].data_ptr(), r["sq"].data_ptr()
    if bias:
        r["b_h"] = F.bias(c)
        r["b"] = r["b_h"].to(dev)
        b = r["b"].data_ptr()
    assert r["x"].data_ptr() % 16 == 0 and r["y"].data_ptr() % 16 == 0
    xp, yp = r["x"].data_ptr() + 2 * c.cx, r["y"].data_ptr() + r["y_h"].element_size() * c.cy
    if fn == "ym_conv_fwd":
        call(fn, ctypes.byref(d), xp, r["w"].data_ptr(), yp, b, ss, sq, st)
    else:
        call(fn, ctypes.byref(d), xp, r["w"].data_ptr(), yp, ss, sq, ctypes.byref(fold), st)
    return r


def _check(c, r, want, what):
    out = F.outside_mask(c)
    got_buf = r["y"].cpu()
    assert torch.equal(got_buf[out], r["y_h"][out]), f"{what}: {c.name} ({c.kname}): write outside the y view"
    got = F.y_view(c, got_buf).contiguous().view(F.OUT_DTYPE[r["out_f32"]])
    msg = F.mismatch(c, got, want)
    assert msg is None, f"{what}: {msg}"
    # the inputs were only read
    assert torch.equal(F.bits(r["x"].cpu()), F.bits(r["x_h"])) and torch.equal(F.bits(r["w"].cpu()), F.bits(r["w_h"]))
    if "b" in r:
        assert torch.equal(F.bits(r["b"].cpu()), F.bits(r["b_h"]))


def _check_stats(c, r, v, exact_sq, what):
    """The fp64 sums of the statistics rows against sum(v) and sum(v^2) over the pixels; returns them."""
    rows, cout = r["rows"], c.cout
    sums = []
    for key, name in (("ss", "stat_sum"), ("sq", "stat_sq")):
        buf = r[key].cpu()
        assert bool((buf[rows * cout:] == F.STAT_CANARY).all()), f"{what}: {c.name}: {name} row {rows} (canary) written"
        body = buf[:rows * cout].view(torch.float32).view(rows, cout)
        bad = torch.isnan(body).any(1).nonzero()
        assert bad.numel() == 0, f"{what}: {c.name} ({c.kname}): {name} row {int(bad[0])} of {rows} not written"
        sums.append(body.double().sum(0))
    S, Q = sums
    want_s, want_q = v.sum((0, 1, 2)), (v * v).sum((0, 1, 2))
    ch = (S != want_s).nonzero()
    assert ch.numel() == 0, (f"{what}: {c.name} ({c.kname}): stat_sum of channel {int(ch[0])}: got "
                             f"{float(S[int(ch[0])])!r}, want {float(want_s[int(ch[0])])!r}")
    err = (Q - want_q).abs()
    lim = torch.zeros_like(want_q) if exact_sq else F.sq_bound(c) * want_q
    ch = (err > lim).nonzero()
    assert ch.numel() == 0, (f"{what}: {c.name} ({c.kname}): stat_sq of channel {int(ch[0])}: got "
                             f"{float(Q[int(ch[0])])!r}, want {float(want_q[int(ch[0])])!r}, bound "
                             f"{float(lim[int(ch[0])])!r}")
    return S, Q


def _kernel_is(c, out_f32=2, accumulate=0):
    from yolomi._lib import lib
    d = F.desc(c, out_f32=out_f32, accumulate=accumulate)
    assert lib().ym_conv_kernel(ctypes.byref(d), 0, None, 0) == c.kid      # under the policy the calls run with


@pytest.mark.parametrize("c", F.STAT_CASES, ids=F.case_id)
def test_fwd_equals_integer_reference(c):
    with F.policy(c):
        _kernel_is(c)
        a = _launch(c, "A", stats=True)
        s = _launch(c, "S", stats=True)
        torch.cuda.synchronize()
    v = F.reference(c, "A")
    _check(c, a, F.cast(v, 2), "run A (fp16 z)")
    _check_stats(c, a, v, False, "run A")
    vs = F.reference(c, "S")
    _check(c, s, F.cast(vs, 2), "run S (z = v)")
    _check_stats(c, s, vs, True, "run S")


@pytest.mark.parametrize("cm", F.OTHER, ids=F.other_id)
def test_fwd_other_outputs(cm):
    """bf16 / fp32 outputs, an integer bias, and accumulate in the form of the store path.  A bias under a policy
    that selects a kernel without a bias term (pipelined, halo-pipelined, direct) must still be added: the route
    skips those kernels."""
    c, mode = cm
    out_f32, acc, has_bias, run = F.MODES[mode]
    with F.policy(c):
        if not has_bias:
            _kernel_is(c, out_f32, acc)
        r = _launch(c, run, out_f32=out_f32, accumulate=acc, bias=has_bias, fill=F.prefill(c, out_f32) if acc else None)
        torch.cuda.synchronize()
    form = f", form {F.bf16_form(c)}" if mode == "accbf" else ""
    _check(c, r, F.expect_other(c, mode), f"{mode}{form}")


@pytest.mark.parametrize("c", F.CLAMP_CASES, ids=F.case_id)
def test_fwd_fp16_clamp(c):
    """|v| = 73 728 in both signs: +-65504 (0x7bff / 0xfbff), not infinity, from every epilogue kind."""
    with F.policy(c):
        _kernel_is(c)
        r = _launch(c, "clamp")
        torch.cuda.synchronize()
    _check(c, r, F.expect_clamp(c), f"clamp ({F.CLAMP_KIND[c.name]})")


BN_CASES = [next(c for c in F.CASES if c.family == f and c.view == "view") for f in F.FAMILIES]


def _within_one_ulp(got, want64, what):
    want = want64.float()
    ok = (got == want) | (got == torch.nextafter(want, want + 1)) | (got == torch.nextafter(want, want - 1))
    ch = (~ok).nonzero()
    assert ch.numel() == 0, f"{what}: channel {int(ch[0])}: got {float(got[int(ch[0])])!r}, want {float(want[int(ch[0])])!r}"


@pytest.mark.parametrize("c", BN_CASES, ids=F.case_id)
def test_fwd_bn_exact(c):
    """ym_conv_fwd_bn on run S: z and the row sums as ym_conv_fwd's, mean == float(S / count) bit for bit, the other
    coefficients and the running statistics within one fp32 ulp of bn_fold.h's fp64 formula on the exact S and Q."""
    from yolomi._lib import BnFold, lib
    dev = torch.device("cuda", 0)
    cout, count, mom, eps = c.cout, float(c.pixels), 0.03, 1e-3
    g = torch.Generator().manual_seed(F._seed(c) ^ 0x7B7B)
    gamma, beta = (1 + 0.1 * torch.randn(cout, generator=g)), 0.1 * torch.randn(cout, generator=g)
    rm0, rv0 = torch.randn(cout, generator=g), 1 + torch.rand(cout, generator=g)
    gd, bd, rm, rv = gamma.to(dev), beta.to(dev), rm0.to(dev), rv0.to(dev)
    nbt = torch.full((1,), 41, dtype=torch.int64, device=dev)
    out = torch.full((4, cout), float("nan"), device=dev)
    ws = torch.zeros(lib().ym_bn_workspace_size(cout), dtype=torch.uint8, device=dev)
    f = BnFold(gamma=gd.data_ptr(), beta=bd.data_ptr(), running_mean=rm.data_ptr(), running_var=rv.data_ptr(),
               num_batches_tracked=nbt.data_ptr(), scale=out[0].data_ptr(), shift=out[1].data_ptr(),
               mean=out[2].data_ptr(), rstd=out[3].data_ptr(), workspace=ws.data_ptr(), count=count, momentum=mom,
               eps=eps)
    with F.policy(c):
        _kernel_is(c)
        d = F.desc(c)
        assert lib().ym_conv_fwd_bn_fused(ctypes.byref(d)) == (1 if c.family in ("gemm", "halo", "pipe") else 0)
        r = _launch(c, "S", stats=True, fn="ym_conv_fwd_bn", fold=f)
        torch.cuda.synchronize()
    vs = F.reference(c, "S")
    _check(c, r, F.cast(vs, 2), "ym_conv_fwd_bn z")
    S, Q = _check_stats(c, r, vs, True, "ym_conv_fwd_bn")
    scale, shift, mean, rstd = (t.cpu() for t in out)
    mu = S / count
    var = (Q / count - mu * mu).clamp(min=0)
    rs = 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))
    assert torch.equal(F.bits(mean), F.bits(mu.float())), f"{c.name}: mean != float(S / count)"
    _within_one_ulp(rstd, rs, f"{c.name}: rstd")
    _within_one_ulp(scale, gamma.double() * rs, f"{c.name}: scale")
    _within_one_ulp(shift, beta.double() - mu * scale.double(), f"{c.name}: shift")          # (of the scale it stored)
    m = float(torch.tensor(mom, dtype=torch.float32))
    _within_one_ulp(rm.cpu(), (1.0 - m) * rm0.double() + m * mu, f"{c.name}: running_mean")
    _within_one_ulp(rv.cpu(), (1.0 - m) * rv0.double() + m * var * count / (count - 1), f"{c.name}: running_var")
    assert int(nbt.cpu()) == 42
    assert int(ws[:256].cpu().view(torch.int32).abs().sum()) == 0, f"{c.name}: tickets not re-armed"
    for t, t0 in ((gd, gamma), (bd, beta)):
        assert torch.equal(F.bits(t.cpu()), F.bits(t0))


# ---- the ABI's edges
def _edge_buffers(c, out_f32=2):
    dev = torch.device("cuda", 0)
    y_h = F.y_buffer(c, out_f32, F.cast(F.reference(c, "S"), out_f32))
    return F.x_buffer(c, "A").to(dev), F.weight_buffer(c, "A").to(dev), y_h, y_h.to(dev)


@pytest.mark.parametrize("stats", [0, 1])
def test_fwd_empty_batch(stats):
    """n = 0: YM_OK before any launch — y keeps every bit, and so do the statistics rows (nothing zeroes them)."""
    from yolomi._lib import call
    c = F.find(32, "view")
    x, wt, y_h, y = _edge_buffers(c)
    st_h = F.stat_buffer(8, c.cout)
    ss, sq = st_h.cuda(), st_h.cuda()
    d = F.desc(c, n=0)
    call("ym_conv_fwd", ctypes.byref(d), x.data_ptr() + 2 * c.cx, wt.data_ptr(), y.data_ptr() + 2 * c.cy, None,
         ss.data_ptr() if stats else None, sq.data_ptr() if stats else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), y_h)
    assert torch.equal(ss.cpu(), st_h) and torch.equal(sq.cpu(), st_h)


def _refused(c, d, x, wt, y, y_h, bias=None, ss=None, sq=None, cy=None):
    from yolomi._lib import lib
    esz = y_h.element_size()
    st = lib().ym_conv_fwd(ctypes.byref(d), x.data_ptr() + 2 * c.cx, wt.data_ptr(),
                           y.data_ptr() + esz * (c.cy if cy is None else cy), bias, ss, sq,
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st != 0 and lib().ym_last_error()
    assert torch.equal(y.cpu(), y_h), "a refused call wrote y"


def test_fwd_refusals_leave_y_alone():
    """Each YM_CHECK_ARG refusal of ym_conv_fwd returns an error and writes nothing."""
    c = F.find(32, "view")
    x, wt, y_h, y = _edge_buffers(c)
    dev = y.device
    d = F.desc(c)
    d.cin = 12                                                             # cin % 8
    _refused(c, d, x, wt, y, y_h)
    b = F.bias(c).to(dev)
    st = F.stat_buffer(8, c.cout).to(dev)
    _refused(c, F.desc(c), x, wt, y, y_h, bias=b.data_ptr(), ss=st.data_ptr(), sq=st.data_ptr())   # bias + statistics
    _refused(c, F.desc(c), x, wt, y, y_h, ss=st.data_ptr())                # one statistics pointer
    assert bool((st.cpu() == F.stat_buffer(8, c.cout)).all())
    _refused(c, F.desc(c, accumulate=1), x, wt, y, y_h)                    # accumulate into fp16
    for field, delta in (("x_ld", 4), ("x_bs", 4), ("y_ld", 2), ("y_bs", 2)):   # misaligned views
        d = F.desc(c)
        setattr(d, field, getattr(d, field) + delta)
        _refused(c, d, x, wt, y, y_h)
    d = F.desc(c)
    d.k = 4                                                                # kernel size
    _refused(c, d, x, wt, y, y_h)
