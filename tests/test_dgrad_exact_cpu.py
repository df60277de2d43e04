"""The exact data-gradient cases (tests/dgrad_exact_cases.py) hold their own conditions, without a GPU:

  * every case's fp64 reference (both operand sets) is integral and within the 2^24 bound that makes fp32 summation
    order-free, and the fp32 CPU conv2d_input of the same operands equals it exactly;
  * run B's max|v| <= 256 on every case (v representable in bf16: one rounding under either accumulate form);
  * run A's tie condition — |v| = 1 and 3 (mod 4) in (256, 512), in both signs where the operands are signed — on at
    least one case per kernel family, where the truncated and the half-away expectations differ from the RNE one;
  * run C's two expectations E1 and E2 differ on every case that claims to discriminate them (all but the one whose
    |v| cannot exceed 128);
  * through the library's host entry points (pure host code, like tests/test_conv_routes_cpu.py): each case runs the
    kernel id, name and template instance it is listed for, whatever its view; the 15 (family, instance) pairs
    ym_conv_dgrad can launch are all covered as a plain tensor, a 16-byte view and — where the family's plan allows
    one — both 8-byte views;
  * every buffer's canaries are in place.
"""
import ctypes

import pytest
import torch

import dgrad_exact_cases as D

# the (family, template instance) pairs of ym_conv_dgrad: launch_tile's three tiles (conv.hip), the halo kernel's C8 and
# C4 (conv_halo.hip), two pipelined tiles x {DGRAD_C1, DGRAD_GEN} (conv_pipe.hip), the halo-pipelined cfg 0 and 2
# (conv_hpipe.hip) and the direct variants 1, 3, 5, 7 (conv_direct.hip).  A 16th fails test_cases_cover_every_instance
# until it has cases.
ALL_INSTANCES = {
    ("gemm", "128x32"), ("gemm", "128x64"), ("gemm", "128x128"),
    ("halo", "C8"), ("halo", "C4"),
    ("pipe", "256x128 C1"), ("pipe", "256x128 GEN"), ("pipe", "256x64 C1"), ("pipe", "256x64 GEN"),
    ("hpipe", "128"), ("hpipe", "64 wres"),
    ("direct", "v1"), ("direct", "v3"), ("direct", "v5"), ("direct", "v7"),
}
REACHABLE_IDS = {32, 64, 128, 2000, 2001, 4000, 4002, 3001, 3003, 3005, 3007}       # and 1000 + TW, 1100 + TW


@pytest.mark.parametrize("c", D.ALL_CASES, ids=D.case_id)
def test_reference_is_exact(c):
    for run in ("large", "small"):
        v = D.reference(c, run)                              # asserts integral and the bound with the prefill
        assert v.dtype == torch.float64 and tuple(v.shape) == (c.n, c.shape[1], c.shape[2], c.shape[3])
        assert torch.equal(v, v.round())
        assert D.exact_bound(c, run) + D.PREFILL_MAX < 2 ** 24
        assert torch.equal(D.reference_f32(c, run).double(), v)
        dz, wt = D.operands(c, run)
        assert dz.dtype == torch.bfloat16 and wt.dtype == torch.bfloat16
        lo, hi = (c.lo, 4) if run == "large" else (-1, 1)
        assert -4 <= lo and float(dz.float().min()) >= lo and float(dz.float().max()) <= hi
        assert float(wt.float().min()) >= lo and float(wt.float().max()) <= hi
    assert float(D.reference(c, "small").abs().max()) <= 256           # run B's condition
    old = D.prefill(c)
    assert old.dtype == torch.bfloat16 and float(old.float().abs().max()) <= D.PREFILL_MAX
    assert torch.equal(old.float(), old.float().round())
    # run B: v is representable, so the two accumulate forms coincide bit for bit
    vs = D.reference(c, "small").float()
    assert torch.equal(vs.bfloat16().float(), vs)
    assert torch.equal(D.bits(D.expect_small(c)), D.bits((vs.bfloat16().float() + old.float()).bfloat16()))


TIE_CASES = [c for c in D.ALL_CASES if c.tie]


@pytest.mark.parametrize("c", TIE_CASES, ids=D.case_id)
def test_overwrite_run_pins_round_to_nearest_even(c):
    v = D.reference(c, "large")
    a = v.abs()
    window = (a > 256) & (a < 512)
    for sign in ((1, -1) if c.signed else (1,)):
        for r, step in ((1, -1), (3, 1)):                    # RNE: 257 -> 256, 259 -> 260
            sel = window & (a % 4 == r) & (v * sign > 0)
            assert bool(sel.any()), (c.name, sign, r)
            assert torch.equal(D.expect_overwrite(c)[sel].double(), v[sel] + sign * step)
    want = D.bits(D.expect_overwrite(c))
    assert not torch.equal(D.bits(D.round_trunc(v)), want)
    assert not torch.equal(D.bits(D.round_half_away(v)), want)
    # each wrong rounding is right where the other is wrong: 259 (mod 4: 3) / 257 (mod 4: 1)
    pos = window & (v > 0)
    assert torch.equal(D.round_trunc(v)[pos & (a % 4 == 1)].double(), v[pos & (a % 4 == 1)] - 1)
    assert torch.equal(D.round_trunc(v)[pos & (a % 4 == 3)].double(), v[pos & (a % 4 == 3)] - 1)
    assert torch.equal(D.round_half_away(v)[pos & (a % 4 == 1)].double(), v[pos & (a % 4 == 1)] + 1)
    # and a one-ulp error everywhere stays inside the 1e-2-of-max|dx| bound of tests/test_gpu_conv.py
    err = (D.round_trunc(v).double() - v).abs().max() / v.abs().max()
    assert 0 < float(err) < 1e-2


def test_tie_condition_in_every_family():
    assert {c.family for c in TIE_CASES} == set(D.FAMILIES)
    assert all(any(c.signed for c in TIE_CASES if c.family == f) for f in ("gemm", "halo", "pipe", "hpipe"))


def test_rounding_helpers():
    v = torch.tensor([257.0, 259.0, -257.0, -259.0, 256.0, 3.0, 258.0, 0.0])
    assert D.round_trunc(v).float().tolist() == [256.0, 258.0, -256.0, -258.0, 256.0, 3.0, 258.0, 0.0]
    assert D.round_half_away(v).float().tolist() == [258.0, 260.0, -258.0, -260.0, 256.0, 3.0, 258.0, 0.0]
    assert v.bfloat16().float().tolist() == [256.0, 260.0, -256.0, -260.0, 256.0, 3.0, 258.0, 0.0]


@pytest.mark.parametrize("c", D.ALL_CASES, ids=D.case_id)
def test_form_run_discriminates(c):
    e1, e2 = D.expect_form(c, "E1"), D.expect_form(c, "E2")
    if c.forms_differ:
        assert not torch.equal(D.bits(e1), D.bits(e2))
        assert float(D.reference(c, "large").abs().max()) > 256
    else:
        # every |v| is representable: the forms coincide identically, whatever the operands in [-4, 4]
        n, h, w, cin, cout, k, s, p = c.shape
        assert k * k * cout * 16 <= 256 and torch.equal(D.bits(e1), D.bits(e2))
    assert bool(torch.isfinite(e1.float()).all()) and bool(torch.isfinite(e2.float()).all())


def test_only_the_short_k_case_cannot_discriminate():
    assert {c.shape for c in D.ALL_CASES if not c.forms_differ} == {(1, 6, 6, 16, 8, 1, 1, 0)}


@pytest.mark.parametrize("c", D.ALL_CASES, ids=D.case_id)
def test_case_runs_its_instance(c):
    from yolomi._lib import lib
    n, h, w, cin, cout, k, s, p = c.shape
    for acc in (0, 1):
        assert D.kernel(c, D.desc(c, accumulate=acc)) == (c.kid, c.kname)
    assert (c.family, c.inst) in ALL_INSTANCES
    fam = {0: "gemm", 1: "halo", 2: "pipe", 3: "direct", 4: "hpipe"}[c.kid // 1000]
    assert fam == c.family
    with D.policy(c):
        d = D.desc(c)
        assert lib().ym_conv_algo(ctypes.byref(d), 1) == c.kid // 1000
    if fam == "gemm":
        assert c.inst == f"128x{c.kid}" and c.kname.endswith(" 4-class") == (s == 2)
    elif fam == "halo":
        th, tw = (int(t) for t in c.kname.split()[-1].split("x"))
        assert c.kid == 1000 + 100 * (c.inst == "C4") + tw and c.kname.split()[1] == c.inst
        assert th * tw <= (256 if c.inst == "C8" else 128) and (tw == 16 or tw == w)
    elif fam == "pipe":
        assert c.inst == f"{'256x128' if c.kid == 2000 else '256x64'} {D.pipe_inst(c.shape)}"
        assert (cin >= 128) == (c.kid == 2000)
    elif fam == "hpipe":
        assert c.inst == {4000: "128", 4002: "64 wres"}[c.kid]
    else:
        assert c.inst == f"v{c.kid - 3000}"
    assert c.kid in REACHABLE_IDS or c.kid // 100 in (10, 11)


def test_cases_cover_every_instance():
    assert set(D.INSTANCES) == ALL_INSTANCES and len(ALL_INSTANCES) == 15
    assert {(c.family, c.inst) for c in D.CASES} == ALL_INSTANCES
    assert {(c.family, c.inst) for c in D.CIN4_CASES} == {("gemm", "128x32"), ("gemm", "128x64"), ("gemm", "128x128"),
                                                          ("halo", "C4"), ("halo", "C8")}
    for fam, inst in ALL_INSTANCES:
        views = {c.view for c in D.CASES if (c.family, c.inst) == (fam, inst)}
        want = {"plain", "view"} if fam == "hpipe" else {"plain", "view", "view8", "view8p"}
        assert views == want, (fam, inst)
    # the partial halo tiles and the pipelined kernel's instances the ids do not show
    assert {c.kid for c in D.CASES if c.family == "halo"} == {1116, 1110, 1120, 1107, 1016, 1020}
    assert any(c.shape[1] % int(c.kname.split()[-1].split("x")[0]) for c in D.CASES if c.family == "halo")


def test_hpipe_refuses_the_eight_byte_views():
    """hpipe_plan requires 8-channel alignment of the dx view: its shapes under an 8-byte view run another family."""
    for c in (c for c in D.CASES if c.family == "hpipe" and c.view == "plain"):
        c8 = D.Case(c.name + "-8", c.family, c.inst, c.shape, c.kid, c.kname, view="view8", sel=c.sel)
        assert D.kernel(c8)[0] // 1000 != 4


@pytest.mark.parametrize("c", D.ALL_CASES, ids=D.case_id)
def test_buffers_and_canaries(c):
    n, h, w, cin, cout, k, s, p = c.shape
    xe, cx, x_gap, ye, cy, y_gap = D.VIEWS[c.view]
    assert ye % 8 == 0 and cy % 8 == 0 and y_gap % 8 == 0                # the ABI's 16-byte rule for dz
    assert c.x_ld % 4 == 0 and c.x_bs % 4 == 0 and cx % 4 == 0           # ... and its 8-byte rule for dx
    assert c.aligned == (c.view in ("plain", "view"))
    if c.view == "view8":
        assert c.x_ld % 8 == 4 and cx == 0
    if c.view == "view8p":
        assert c.x_ld % 8 == 0 and c.x_bs % 8 == 0 and cx % 8 == 4
    if c.view == "view4":
        # pitch, image stride and pointer all 16-byte aligned; cin ends half way through a 16-byte run
        assert cin % 8 == 4 and c.x_ld % 8 == 0 and c.x_bs % 8 == 0 and cx == 0 and c.x_ld - cin == 4
    if c.view != "plain":
        assert c.x_ld > cin and c.y_ld > cout and cy > 0 and c.x_bs > h * w * c.x_ld and c.y_bs > c.oh * c.ow * c.y_ld
    for run in ("large", "small"):
        buf = D.dz_buffer(c, run)                                        # asserts NaN everywhere outside the view
        assert buf.numel() == n * c.y_bs
        assert D.weight_buffer(c, run).numel() == cin * k * k * cout
    out = D.outside_mask(c)
    assert int((~out).sum()) == n * h * w * cin
    nanbuf = D.dx_buffer(c, None)
    assert nanbuf.dtype == torch.int16 and nanbuf.numel() == n * c.x_bs
    assert torch.equal(nanbuf[out], D.sentinel(n * c.x_bs)[out])
    assert bool(torch.isnan(nanbuf.view(torch.bfloat16).float()).all())     # the view NaN, the sentinels NaN payloads
    old = D.dx_buffer(c, D.prefill(c))
    assert torch.equal(D.dx_view(c, old), D.bits(D.prefill(c))) and torch.equal(old[out], nanbuf[out])
    # a sentinel is never a value a run expects: an over-write cannot hide
    assert int(D.sentinel(4096).min()) >= 0x7F81


def test_empty_parity_classes():
    """k = 1 with stride 2: only the (even, even) pixels receive a tap — the other three classes are exactly +0 in run
    A and bit-identical to the prefill in runs B and C."""
    cs = [c for c in D.CASES if c.shape[5] == 1 and c.shape[6] == 2]
    assert {c.view for c in cs} == {"plain", "view", "view8", "view8p"}
    for c in cs:
        empty = torch.ones(c.shape[1], c.shape[2], dtype=torch.bool)
        empty[0::2, 0::2] = False
        a = D.bits(D.expect_overwrite(c))[:, empty]
        assert a.numel() > 0 and bool((a == 0).all())                   # +0: no sign bit
        old = D.bits(D.prefill(c))[:, empty]
        assert torch.equal(D.bits(D.expect_small(c))[:, empty], old)
        assert torch.equal(D.bits(D.expect_form(c, "E1"))[:, empty], old)
        assert torch.equal(D.bits(D.expect_form(c, "E2"))[:, empty], old)
        assert bool((D.reference(c, "large")[:, ~empty] != 0).any())


def test_policy_is_restored():
    from yolomi._lib import lib
    L = lib()
    setters = (L.ym_conv_set_halo, L.ym_conv_set_pipe, L.ym_conv_set_direct, L.ym_conv_set_hpipe,
               L.ym_conv_set_select_batch)

    def snapshot():
        vals = [fn(0) for fn in setters]
        for fn, v in zip(setters, vals):
            fn(v)
        return vals

    before = snapshot()
    for c in D.ALL_CASES[::7]:
        D.kernel(c)
        with pytest.raises(RuntimeError):
            with D.policy(c):
                raise RuntimeError("inside")
    assert snapshot() == before


def test_mismatch_names_the_first_element():
    c = next(c for c in D.CASES if c.kid == 64 and c.shape[6] == 2 and c.view == "view")  # (2, 9, 11, 72, 40, 3, 2, 1)
    want = D.expect_overwrite(c)
    got = want.clone()
    assert D.mismatch(c, got, want) is None
    got[1, 4, 7, 70] = got[1, 4, 7, 70] + 2
    got[1, 8, 10, 3] = float("nan")
    msg = D.mismatch(c, got, want)
    # class (0, 1): 5 x 5 pixels per image; image 1, class row 2, column 3 -> m = 25 + 13
    assert "2 of" in msg and "(image 1, y 4, x 7, channel 70)" in msg and "class (0, 1), m-tile 0 row 38" in msg
    assert "channel tile 1" in msg and f"want {float(want[1, 4, 7, 70])!r}" in msg and "gemm 128x64 4-class" in msg
    # -0 against +0 is a mismatch: the comparison is on bit patterns
    z = torch.zeros(1, 1, 1, 1, dtype=torch.bfloat16)
    assert D.bits(z).item() == 0 and bool((D.bits(-z) != D.bits(z)).all())
    q = next(c for c in D.CASES if c.inst == "v1")
    assert D.locate(q, 0, 5, 8, 3) == "quad (2, 4) of image 0, class (1, 0)"
    t = next(c for c in D.CASES if c.kid == 1116 and c.shape[2] == 48)
    assert D.locate(t, 0, 8, 47, 3).startswith("tile (row 1, column 2) of image 0, pixel (0, 15)")
