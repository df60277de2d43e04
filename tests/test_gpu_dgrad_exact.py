"""Every data-gradient kernel instance ym_conv_dgrad can launch against the integer result, bit for bit.

The cases, operands, buffers and the fp64 reference are tests/dgrad_exact_cases.py's (its docstring has the argument:
integer operands in [-4, 4], every fp32 partial sum below 2^24, so the accumulator must equal
torch.nn.grad.conv2d_input in fp64 BY VALUE and the bf16 output is a deterministic function of it);
tests/test_dgrad_exact_cpu.py shows on the host that each case runs the instance it is listed for and meets the
conditions of its runs.  Here each case runs three times on the device, on one stream with one synchronize:

  A  overwrite onto NaN: bf16(v), round to nearest even — the cases reach |v| in (256, 512), where odd integers tie;
  B  accumulate of small operands (|v| <= 256) onto integers: bf16(old + v), the same bits for every kernel;
  C  accumulate of run A's operands: the form FORM lists for the instance and store path — E1 = bf16(old + v) for the
     fragment epilogues, E2 = bf16(bf16(v) + old) for the 16-byte ones.
dz lives in a NaN-filled buffer (an over-read poisons the result), dx in a buffer of sentinels that must come back
bit-unchanged, the weights in an allocation of their exact size.  A failure names the first mismatching (image, y, x,
channel), its tile / class / quad, got and want.
"""
import ctypes

import pytest
import torch

import dgrad_exact_cases as D

pytestmark = pytest.mark.gpu

# The accumulate form of each instance by store path, read from the code: (family, instance) -> (form with a dx view
# that allows 16-byte stores, form with an 8-byte view).  conv_epi.h's epilogue_store / epilogue_regs_x round the
# accumulator to bf16 and add the old value to that (E2); the fragment epilogues of conv.hip, conv_halo.hip and
# conv_direct.hip add in fp32 and round once (E1).  The GEMM's 128x32 tile never takes the 16-byte epilogue (its waves
# own 16 channels: BN / WM < 32); the pipelined and direct kernels have one epilogue each, whatever the alignment.
FORM = {
    ("gemm", "128x32"): ("E1", "E1"),
    ("gemm", "128x64"): ("E2", "E1"),
    ("gemm", "128x128"): ("E2", "E1"),
    ("halo", "C8"): ("E2", "E1"),
    ("halo", "C4"): ("E2", "E1"),
    ("pipe", "256x128 C1"): ("E2", "E2"),
    ("pipe", "256x128 GEN"): ("E2", "E2"),
    ("pipe", "256x64 C1"): ("E2", "E2"),
    ("pipe", "256x64 GEN"): ("E2", "E2"),
    ("hpipe", "128"): ("E2", None),
    ("hpipe", "64 wres"): ("E2", None),
    ("direct", "v1"): ("E2", "E2"),
    ("direct", "v3"): ("E2", "E2"),
    ("direct", "v5"): ("E2", "E2"),
    ("direct", "v7"): ("E1", "E1"),
}


def _run(c, dev, st, run, fill, accumulate):
    """Launches one run of case c; returns the device tensors (kept alive by the caller until the synchronize) and the
    host copies of the buffers the kernel must leave alone."""
    from yolomi._lib import call
    dz_h, w_h, dx_h = D.dz_buffer(c, run), D.weight_buffer(c, run), D.dx_buffer(c, fill)
    dz, wt, dx = dz_h.to(dev), w_h.to(dev), dx_h.to(dev)
    d = D.desc(c, accumulate=accumulate)
    assert dx.data_ptr() % 16 == 0 and dz.data_ptr() % 16 == 0
    call("ym_conv_dgrad", ctypes.byref(d), dz.data_ptr() + 2 * c.cy, wt.data_ptr(), dx.data_ptr() + 2 * c.cx, st)
    return dict(dz=dz, wt=wt, dx=dx, dz_h=dz_h, w_h=w_h, dx_h=dx_h)


def _check(c, r, want, what):
    out = D.outside_mask(c)
    got_buf = r["dx"].cpu()
    assert torch.equal(got_buf[out], r["dx_h"][out]), f"{what}: write outside the dx view"
    got = D.dx_view(c, got_buf).contiguous().view(torch.bfloat16)
    msg = D.mismatch(c, got, want)
    assert msg is None, f"{what}: {msg}"
    # the inputs were only read
    assert torch.equal(D.bits(r["dz"].cpu()), D.bits(r["dz_h"]))
    assert torch.equal(D.bits(r["wt"].cpu()), D.bits(r["w_h"]))


def _three_runs(c):
    from yolomi._lib import lib
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    form = FORM[(c.family, c.inst)][0 if c.aligned else 1]
    with D.policy(c):
        d = D.desc(c)
        assert lib().ym_conv_kernel(ctypes.byref(d), 1, None, 0) == c.kid      # under the policy the calls run with
        a = _run(c, dev, st, "large", None, 0)
        b = _run(c, dev, st, "small", D.prefill(c), 1)
        f = _run(c, dev, st, "large", D.prefill(c), 1)
        torch.cuda.synchronize()
    _check(c, a, D.expect_overwrite(c), "run A (overwrite)")
    _check(c, b, D.expect_small(c), "run B (accumulate, |v| <= 256)")
    _check(c, f, D.expect_form(c, form), f"run C (accumulate, form {form})")


@pytest.mark.parametrize("c", D.CASES, ids=D.case_id)
def test_dgrad_equals_integer_reference(c):
    _three_runs(c)


@pytest.mark.parametrize("c", D.EDGE_CASES, ids=D.case_id)
def test_dgrad_other_kernel_sizes_and_pads(c):
    """k = 2 with stride 2 and a 3x3 without padding: (k, pad) pairs the network does not use and the ABI accepts."""
    _three_runs(c)


@pytest.mark.parametrize("c", D.CIN4_CASES, ids=D.case_id)
def test_dgrad_cin_not_a_multiple_of_8(c):
    """cin % 8 == 4 in a 16-byte aligned view: the four channels after cin belong to the neighbouring slice and must
    stay untouched, so these views take the fragment epilogue (E1) like the 8-byte ones."""
    assert not c.aligned
    _three_runs(c)


@pytest.mark.parametrize("accumulate", [0, 1])
def test_dgrad_empty_batch(accumulate):
    """n = 0: YM_OK and nothing is written — dx keeps every bit, view and surroundings."""
    from yolomi._lib import call
    c = next(c for c in D.CASES if c.kid == 32 and c.view == "view")
    dev = torch.device("cuda", 0)
    d = D.desc(c, n=0, accumulate=accumulate)
    dz, wt = D.dz_buffer(c, "large").to(dev), D.weight_buffer(c, "large").to(dev)
    dx_h = D.dx_buffer(c, D.prefill(c))
    dx = dx_h.to(dev)
    call("ym_conv_dgrad", ctypes.byref(d), dz.data_ptr() + 2 * c.cy, wt.data_ptr(), dx.data_ptr() + 2 * c.cx,
         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(dx.cpu(), dx_h)
