"""Every weight-gradient kernel instance of csrc/wgrad.hip (ym_conv_wgrad) against the integer result, bit for bit.

The cases, operands and the fp64 reference are tests/wgrad_exact_cases.py's (its docstring has the argument: integer
operands in [-4, 4], every fp32 partial sum below 2^24, so the summation order does not matter and the kernel must
equal torch.nn.grad.conv2d_weight in fp64 BY VALUE); tests/test_wgrad_exact_cpu.py shows on the host that each case
runs the instance it is listed for, that the 24 instances are all there are, and that the split scenarios and unit
parities are what they claim.  Here each case runs on the device:

  * accumulate = 0 onto a dw prefilled with NaN, with a workspace prefilled with NaN (no zero-fill by the caller), both
    inside larger allocations with canaries before dw's first and after its last element and around the workspace's
    `need` bytes; x and dz in NaN-filled channel-slice views (an over-read poisons the result);
  * accumulate = 1 onto known integers: prefill + reference, exactly;
  * the instance id is asserted again, under the setting the call runs with.
A failure names the first mismatching (co, ci, kh, kw), its channel tile, got / want and the mismatch count.
"""
import ctypes

import pytest
import torch

import wgrad_exact_cases as W

pytestmark = pytest.mark.gpu

PAD = 64                       # floats of canary on either side (keeps dw and the workspace 256-byte aligned)
CANARY = -77777.0


def _guarded(numel, fill, dev):
    """A (numel + 2 * PAD) fp32 allocation: canaries around `numel` elements filled with `fill`."""
    buf = torch.full((numel + 2 * PAD,), CANARY, dtype=torch.float32, device=dev)
    buf[PAD:PAD + numel] = fill
    return buf


def _canaries_intact(buf, numel):
    return bool((buf[:PAD] == CANARY).all()) and bool((buf[PAD + numel:] == CANARY).all())


@pytest.mark.parametrize("c", W.CASES, ids=W.case_id)
def test_wgrad_equals_integer_reference(c):
    from yolomi._lib import call, lib
    n, h, w, cin, cout, k, s, p = c.shape
    dev = torch.device("cuda", 0)
    ref = W.reference(c)
    pre = W.prefill(c)
    xbuf_h, dzbuf_h = W.buffers(c)
    d = W.desc(c)
    st = torch.cuda.current_stream().cuda_stream
    with W.wgrad_target(c):
        assert lib().ym_conv_kernel(ctypes.byref(d), 2, None, 0) == c.kid
        need = lib().ym_conv_wgrad_workspace_size(ctypes.byref(d))      # sized under the setting it is used with
        assert need % 4 == 0 and need >= 4 * c.elems
        # every device tensor stays in a name until after the synchronize (a temporary's block goes back to the
        # caching allocator as soon as its data_ptr() is taken)
        xbuf, dzbuf = xbuf_h.to(dev), dzbuf_h.to(dev)
        ws = _guarded(need // 4, float("nan"), dev)
        dw = _guarded(c.elems, float("nan"), dev)
        dwa = _guarded(c.elems, 0.0, dev)
        dwa[PAD:PAD + c.elems] = pre.reshape(-1).to(dev)
        x_ptr, dz_ptr = xbuf.data_ptr() + 2 * c.cx, dzbuf.data_ptr() + 2 * c.cy
        ws_ptr = ws.data_ptr() + 4 * PAD
        call("ym_conv_wgrad", ctypes.byref(d), dz_ptr, x_ptr, ws_ptr, need, dw.data_ptr() + 4 * PAD, 0, st)
        torch.cuda.synchronize()
        ws.fill_(float("nan"))
        ws[:PAD] = CANARY
        ws[PAD + need // 4:] = CANARY
        call("ym_conv_wgrad", ctypes.byref(d), dz_ptr, x_ptr, ws_ptr, need, dwa.data_ptr() + 4 * PAD, 1, st)
        torch.cuda.synchronize()
    assert _canaries_intact(dw, c.elems) and _canaries_intact(dwa, c.elems), "write outside dw"
    assert _canaries_intact(ws, need // 4), "write outside the workspace's need bytes"
    got = dw[PAD:PAD + c.elems].cpu().reshape(cout, cin, k, k)
    gota = dwa[PAD:PAD + c.elems].cpu().reshape(cout, cin, k, k)
    msg = W.mismatch(c, got, ref)
    assert msg is None, "accumulate = 0: " + msg
    msg = W.mismatch(c, gota, pre.double() + ref)
    assert msg is None, "accumulate = 1: " + msg
    # the inputs were only read
    assert torch.equal(xbuf.cpu().view(torch.int16), xbuf_h.view(torch.int16))
    assert torch.equal(dzbuf.cpu().view(torch.int16), dzbuf_h.view(torch.int16))


# one instance per kernel family, and a scenario with several splits under a non-default target
SMALL_WS = [next(c for c in W.INSTANCE_CASES if c.kid == kid and c.viewed) for kid in (13002, 13503, 11064, 10064)]
SMALL_WS += [c for c in W.SPLIT_CASES if c.name.endswith(("target4", "plain6"))]


@pytest.mark.parametrize("c", SMALL_WS, ids=W.case_id)
def test_wgrad_small_workspace_is_refused(c):
    """A workspace 4 bytes short of ym_conv_wgrad_workspace_size: YM_ERR_ARG and no launch (yolomi_experimental.h) —
    dw and the workspace keep their NaN prefill.  Then the same buffers at full size give the exact result."""
    from yolomi._lib import YolomiError, call, lib
    n, h, w, cin, cout, k, s, p = c.shape
    dev = torch.device("cuda", 0)
    xbuf_h, dzbuf_h = W.buffers(c)
    d = W.desc(c)
    st = torch.cuda.current_stream().cuda_stream
    with W.wgrad_target(c):
        need = lib().ym_conv_wgrad_workspace_size(ctypes.byref(d))
        xbuf, dzbuf = xbuf_h.to(dev), dzbuf_h.to(dev)
        ws = _guarded(need // 4, float("nan"), dev)
        dw = _guarded(c.elems, float("nan"), dev)
        args = (ctypes.byref(d), dzbuf.data_ptr() + 2 * c.cy, xbuf.data_ptr() + 2 * c.cx, ws.data_ptr() + 4 * PAD)
        for acc in (0, 1):
            with pytest.raises(YolomiError, match="workspace"):
                call("ym_conv_wgrad", *args, need - 4, dw.data_ptr() + 4 * PAD, acc, st)
        torch.cuda.synchronize()
        assert bool(torch.isnan(dw[PAD:PAD + c.elems]).all()) and _canaries_intact(dw, c.elems)
        assert bool(torch.isnan(ws[PAD:PAD + need // 4]).all()) and _canaries_intact(ws, need // 4)
        call("ym_conv_wgrad", *args, need, dw.data_ptr() + 4 * PAD, 0, st)
        torch.cuda.synchronize()
    msg = W.mismatch(c, dw[PAD:PAD + c.elems].cpu().reshape(cout, cin, k, k), W.reference(c))
    assert msg is None, msg
    if c.target:
        # the setting is back at the default, whose plan has more splits: the workspace sized under c.target is too
        # small for a call made now, and that call checks it against its own plan
        assert lib().ym_conv_wgrad_workspace_size(ctypes.byref(d)) > need
        dw[PAD:PAD + c.elems] = float("nan")
        with pytest.raises(YolomiError, match="workspace"):
            call("ym_conv_wgrad", *args, need, dw.data_ptr() + 4 * PAD, 0, st)
        torch.cuda.synchronize()
        assert bool(torch.isnan(dw[PAD:PAD + c.elems]).all())


EMPTY = [next(c for c in W.INSTANCE_CASES if c.kid == kid and c.viewed) for kid in (13002, 13503, 11064, 10064)]


@pytest.mark.parametrize("c", EMPTY, ids=W.case_id)
def test_wgrad_empty_batch(c):
    """n = 0 (non-null dummy operands): no pixels, the gradient is zero — accumulate = 0 zeroes dw, accumulate = 1
    leaves it; nothing outside dw is written."""
    from yolomi._lib import call, lib
    dev = torch.device("cuda", 0)
    d = W.desc(c, n=0)
    st = torch.cuda.current_stream().cuda_stream
    need = lib().ym_conv_wgrad_workspace_size(ctypes.byref(d))
    assert need == 4 * c.elems
    dummy_x = torch.full((64,), float("nan"), dtype=torch.float16, device=dev)
    dummy_dz = torch.full((64,), float("nan"), dtype=torch.bfloat16, device=dev)
    ws = _guarded(need // 4, float("nan"), dev)
    dw = _guarded(c.elems, float("nan"), dev)
    pre = W.prefill(c).reshape(-1)
    dwa = _guarded(c.elems, 0.0, dev)
    dwa[PAD:PAD + c.elems] = pre.to(dev)
    call("ym_conv_wgrad", ctypes.byref(d), dummy_dz.data_ptr(), dummy_x.data_ptr(), ws.data_ptr() + 4 * PAD, need,
         dw.data_ptr() + 4 * PAD, 0, st)
    call("ym_conv_wgrad", ctypes.byref(d), dummy_dz.data_ptr(), dummy_x.data_ptr(), ws.data_ptr() + 4 * PAD, need,
         dwa.data_ptr() + 4 * PAD, 1, st)
    torch.cuda.synchronize()
    assert bool((dw[PAD:PAD + c.elems] == 0).all()) and _canaries_intact(dw, c.elems)
    assert torch.equal(dwa[PAD:PAD + c.elems].cpu(), pre) and _canaries_intact(dwa, c.elems)
    assert _canaries_intact(ws, need // 4)
