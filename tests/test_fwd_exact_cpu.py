"""The exact forward cases (tests/fwd_exact_cases.py) hold their own conditions, without a GPU:

  * every case's fp64 reference (every operand set) is integral and within the 2^24 bound that makes fp32 summation
    order-free, and the fp32 CPU conv2d of the same operands equals it exactly;
  * run A: pixels * max|v| < 2^24 (exact statistics row sums), sum(v) != sum(fp16(v)) on every case that claims it (all
    but the ones whose |v| cannot pass 2048), and the tie condition — |v| = 1 and 3 (mod 4) in (2048, 4096), in both
    signs where the operands are signed — on at least one case per kernel family, where the truncated and the
    half-away expectations differ from the RNE one;
  * run S: max|v| <= 2048 and per channel sum(v^2) < 2^24;
  * the bf16 accumulate expectations E1 and E2 differ on every case that runs one, and the bf16 overwrite cases have
    ties in (256, 512); the clamp cases pass 65504 in both signs;
  * through the library's host entry points (pure host code): each case runs the kernel id, name and template
    instance it is listed for, whatever its view and output type; the 17 (family, instance) pairs ym_conv_fwd can
    launch are all covered as a plain tensor, a 16-byte view and — where the family's plan allows one — the 8-byte
    views, and they are the ones the launch tables of the sources hold;
  * the OTHER table covers every (family, store path, output) STORE lists; every buffer's canaries are in place.
"""
import ctypes
import re
from pathlib import Path

import pytest
import torch

import fwd_exact_cases as F

CSRC = Path(__file__).resolve().parents[1] / "yolo-scratch_amd" / "csrc"

# the (family, template instance) pairs of ym_conv_fwd: launch_tile's three tiles (conv.hip), the halo kernel's C8 and
# C4 (conv_halo.hip), two pipelined tiles x {FWD_GEN, FWD_C1, FWD_C1_TAP} (conv_pipe.hip), the halo-pipelined cfg 0 and
# 2 (conv_hpipe.hip) and the direct variants 0, 2, 4, 6 (conv_direct.hip).  An 18th fails
# test_cases_cover_every_instance until it has cases.
ALL_INSTANCES = {
    ("gemm", "128x32"), ("gemm", "128x64"), ("gemm", "128x128"),
    ("halo", "C8"), ("halo", "C4"),
    ("pipe", "256x128 GEN"), ("pipe", "256x128 C1"), ("pipe", "256x128 C1 TAP"),
    ("pipe", "256x64 GEN"), ("pipe", "256x64 C1"), ("pipe", "256x64 C1 TAP"),
    ("hpipe", "128"), ("hpipe", "64 wres"),
    ("direct", "v0"), ("direct", "v2"), ("direct", "v4"), ("direct", "v6"),
}
REACHABLE_IDS = {32, 64, 128, 2000, 2001, 4000, 4002, 3000, 3002, 3004, 3006}       # and 1000 + TW, 1100 + TW


def _runs(c):
    if c in F.CLAMP_CASES:
        return ("clamp",)
    if c in F.HEAD_CASES:
        return ("A",)
    return ("A", "S", "B")


@pytest.mark.parametrize("c", F.ALL_CASES, ids=F.case_id)
def test_reference_is_exact(c):
    n, h, w, cin, cout, k, s, p = c.shape
    assert k * k * cin * 256 < 2 ** 24 and cin % 8 == 0
    for run in _runs(c):
        v = F.reference(c, run)                              # asserts integral and the bound
        assert v.dtype == torch.float64 and tuple(v.shape) == (c.n, c.oh, c.ow, cout)
        assert torch.equal(v, v.round()) and F.exact_bound(c, run) < 2 ** 24
        assert torch.equal(F.reference_f32(c, run).double(), v)
        x, wt = F.operands(c, run)
        assert x.dtype == torch.float16 and wt.dtype == torch.float16
        lo, hi = {"A": (c.lo, c.hi), "S": (-1, 1), "B": (c.blo, 4), "clamp": (-16, 16)}[run]
        assert -16 <= lo and hi <= 16
        for t in (x, wt):
            assert float(t.float().min()) >= lo and float(t.float().max()) <= hi
            assert torch.equal(t.float(), t.float().round())


@pytest.mark.parametrize("c", F.STAT_CASES, ids=F.case_id)
def test_statistics_runs_are_exact(c):
    v = F.reference(c, "A")
    assert c.pixels * float(v.abs().max()) < 2 ** 24                     # run A: every partial row sum is exact
    z = F.cast(v, 2).double()
    assert bool(torch.isfinite(z).all())
    differs = bool((v.sum((0, 1, 2)) != z.sum((0, 1, 2))).any())
    assert differs == c.rounds, c.name
    if not c.rounds:
        n, h, w, cin, cout, k, s, p = c.shape                             # |v| cannot pass 2048: all representable
        assert k * k * cin * max(abs(c.lo), c.hi) ** 2 <= 2048 and torch.equal(z, v)
    assert 0 < F.sq_bound(c) < 1e-3
    vs = F.reference(c, "S")
    assert float(vs.abs().max()) <= 2048 and float((vs * vs).sum((0, 1, 2)).max()) < 2 ** 24
    assert torch.equal(F.cast(vs, 2).double(), vs)                        # z = v by value
    assert float(vs.abs().max()) > 0


def test_only_the_short_k_case_cannot_round():
    assert {c.shape for c in F.STAT_CASES if not c.rounds} == {(2, 68, 68, 8, 512, 1, 1, 0)}


TIE_CASES = [c for c in F.STAT_CASES if c.tie]


@pytest.mark.parametrize("c", TIE_CASES, ids=F.case_id)
def test_overwrite_run_pins_round_to_nearest_even(c):
    v = F.reference(c, "A")
    a = v.abs()
    window = (a > 2048) & (a < 4096)
    want = F.cast(v, 2)
    for sign in ((1, -1) if c.signed else (1,)):
        for r, step in ((1, -1), (3, 1)):                    # RNE: 2049 -> 2048, 2051 -> 2052
            sel = window & (a % 4 == r) & (v * sign > 0)
            assert bool(sel.any()), (c.name, sign, r)
            assert torch.equal(want[sel].double(), v[sel] + sign * step)
    assert not torch.equal(F.bits(F.round_trunc(v)), F.bits(want))
    assert not torch.equal(F.bits(F.round_half_away(v)), F.bits(want))
    pos = window & (v > 0)
    assert torch.equal(F.round_trunc(v)[pos & (a % 2 == 1)].double(), v[pos & (a % 2 == 1)] - 1)
    assert torch.equal(F.round_half_away(v)[pos & (a % 2 == 1)].double(), v[pos & (a % 2 == 1)] + 1)
    # and a one-ulp error everywhere stays inside the 1e-3-of-max|y| bound of tests/test_gpu_conv.py
    err = (F.round_trunc(v).double() - v).abs().max() / v.abs().max()
    assert 0 < float(err) < 1e-3


def test_tie_condition_in_every_family():
    assert {c.family for c in TIE_CASES} == set(F.FAMILIES)
    assert all(any(c.signed for c in TIE_CASES if c.family == f) for f in F.FAMILIES)


def test_rounding_helpers():
    v = torch.tensor([2049.0, 2051.0, -2049.0, -2051.0, 2048.0, 3.0, 2050.0, 0.0], dtype=torch.float64)
    assert F.round_trunc(v).float().tolist() == [2048.0, 2050.0, -2048.0, -2050.0, 2048.0, 3.0, 2050.0, 0.0]
    assert F.round_half_away(v).float().tolist() == [2050.0, 2052.0, -2050.0, -2052.0, 2048.0, 3.0, 2050.0, 0.0]
    assert F.cast(v, 2).float().tolist() == [2048.0, 2052.0, -2048.0, -2052.0, 2048.0, 3.0, 2050.0, 0.0]


@pytest.mark.parametrize("cm", F.OTHER, ids=F.other_id)
def test_other_outputs_discriminate(cm):
    c, mode = cm
    out_f32, acc, has_bias, run = F.MODES[mode]
    want = F.expect_other(c, mode)
    assert want.dtype == F.OUT_DTYPE[out_f32] and bool(torch.isfinite(want.float()).all())
    v = F.reference(c, run)
    if has_bias:
        b = F.bias(c)
        assert b.numel() == c.cout and torch.equal(b, b.round()) and float(b.abs().max()) <= 64
        if c.cout >= 3:                                       # (a single channel may draw 0)
            assert not torch.equal(F.bits(want), F.bits(F.cast(v, out_f32)))             # the bias shows
    if mode == "bf16":
        a = v.abs()
        assert bool(((a > 256) & (a < 512) & (a % 2 == 1)).any()), c.name                 # ties
    if mode == "accbf":
        e1, e2 = F.expect_form(c, "E1"), F.expect_form(c, "E2")
        assert not torch.equal(F.bits(e1), F.bits(e2))
        assert torch.equal(F.bits(want), F.bits(e1 if F.bf16_form(c) == "E1" else e2))
    if acc:
        old = F.prefill(c, out_f32)
        assert old.dtype == F.OUT_DTYPE[out_f32] and float(old.float().abs().max()) <= F.PREFILL_MAX
        assert torch.equal(old.float(), old.float().round())


def test_other_outputs_cover_the_store_paths():
    """One OTHER entry per (family, store path, output kind) STORE lists; fp16 is runs A / S of every case."""
    def path(c, mode):
        out_f32, acc, has_bias, run = F.MODES[mode]
        if c.cout % 4 and c.family in ("gemm", "halo"):
            return "tail"
        if c.family in ("pipe", "hpipe"):
            return "16B"
        if c.family == "halo":
            return "16B" if c.aligned and not has_bias and out_f32 != 1 else "frag"
        return "frag"                                         # gemm: everything but a bias-free fp16

    kind = {"bf16": "bf16", "f32": "f32", "bias16": "bias", "biasbf": "bias", "bias32": "bias", "acc32": "acc",
            "accbf": "acc"}
    # a bias under a policy that selects a kernel without a bias term runs the GEMM: not that family's path
    have = {(c.family, path(c, m), kind[m]) for c, m in F.OTHER
            if not (kind[m] == "bias" and c.family in ("pipe", "hpipe", "direct"))}
    for fam, paths in F.STORE.items():
        for pth, (kinds, form) in paths.items():
            for kd in kinds:
                if kd != "fp16":
                    assert (fam, pth, kd) in have, (fam, pth, kd)
    assert {c.family for c, m in F.OTHER if m == "bias16"} == set(F.FAMILIES)
    # the 16-byte path of the pipelined kernels also in an 8-byte-aligned view
    for fam, v8 in (("pipe", "view8"), ("hpipe", "view8p")):
        assert any(c.family == fam and c.view == v8 and m == "accbf" for c, m in F.OTHER)
    # fp16: 16-byte, fragment and tail paths of the GEMM and the halo kernel
    assert any(c.family == "gemm" and c.aligned and c.kid in (64, 128) for c in F.CASES)
    assert any(c.family == "gemm" and not c.aligned and c.kid in (64, 128) for c in F.CASES)
    assert {c.family for c in F.TAIL_CASES} == {"gemm", "halo"} and all(c.cout % 4 for c in F.TAIL_CASES)
    assert {(c.family, c.inst) for c in F.COUT4_CASES} == {
        ("gemm", "128x32"), ("gemm", "128x64"), ("gemm", "128x128"), ("halo", "C4"), ("halo", "C8")}
    assert {c.cout for c in F.COUT4_CASES if c.family == "gemm"} == {44, 68, 132}
    assert {c.cout for c in F.HEAD_CASES} == {1, 3, 80} and all(c.cy % 4 for c in F.HEAD_CASES)


@pytest.mark.parametrize("c", F.CLAMP_CASES, ids=F.case_id)
def test_clamp_cases_overflow_in_both_signs(c):
    v = F.reference(c, "clamp")
    assert float(v.max()) > 65504 and float(v.min()) < -65504
    want = F.bits(F.expect_clamp(c)).to(torch.int32) & 0xFFFF
    assert bool((want == 0x7BFF).any()) and bool((want == 0xFBFF).any())
    assert bool(torch.isfinite(F.expect_clamp(c).float()).all())
    assert bool(torch.isinf(v.float().half().float()).any())              # without the clamp: infinity
    if "f2h" in c.note:                                                   # the scalar tail overflows too
        assert c.cout % 4 and float(v[..., c.cout - c.cout % 4:].abs().max()) > 65504


def test_clamp_cases_cover_the_epilogue_kinds():
    assert {k for c in F.CLAMP_CASES for k in c.note.split(", ")} == {"pk2h", "f2h", "epilogue_regs", "epilogue_store"}
    assert {(c.kid, c.aligned) for c in F.CLAMP_CASES} == {(32, True), (32, False), (64, True), (3000, True)}


def _desc(c, out_f32=None):
    return F.desc(c, out_f32=(1 if c.view == "wide" else 2) if out_f32 is None else out_f32)


@pytest.mark.parametrize("c", F.ALL_CASES, ids=F.case_id)
def test_case_runs_its_instance(c):
    from yolomi._lib import lib
    n, h, w, cin, cout, k, s, p = c.shape
    assert F.kernel(c, _desc(c)) == (c.kid, c.kname)
    assert (c.family, c.inst) in ALL_INSTANCES
    fam = {0: "gemm", 1: "halo", 2: "pipe", 3: "direct", 4: "hpipe"}[c.kid // 1000]
    assert fam == c.family
    with F.policy(c):
        d = _desc(c)
        assert lib().ym_conv_algo(ctypes.byref(d), 0) == c.kid // 1000
    if fam == "gemm":
        assert c.inst == f"128x{c.kid}"
    elif fam == "halo":
        th, tw = (int(t) for t in c.kname.split()[-1].split("x"))
        assert c.kid == 1000 + 100 * (c.inst == "C4") + tw and c.kname.split()[1] == c.inst
        assert th * tw <= (256 if c.inst == "C8" else 128) and (tw == 16 or tw == c.ow)
    elif fam == "pipe":
        assert c.inst == f"{'256x128' if c.kid == 2000 else '256x64'} {F.pipe_inst(c.shape)}"
        assert (cout >= 128) == (c.kid == 2000)
    elif fam == "hpipe":
        assert c.inst == {4000: "128", 4002: "64 wres"}[c.kid]
    else:
        assert c.inst == f"v{c.kid - 3000}"
    assert c.kid in REACHABLE_IDS or c.kid // 100 in (10, 11)
    rows = F.stat_rows(c, _desc(c))
    assert rows >= 8 and rows % 8 == 0


@pytest.mark.parametrize("cm", F.OTHER, ids=F.other_id)
def test_other_output_runs_its_instance(cm):
    """The bias-free modes run the listed kernel with their own output type and accumulate flag."""
    c, mode = cm
    out_f32, acc, has_bias, run = F.MODES[mode]
    if not has_bias:
        assert F.kernel(c, F.desc(c, out_f32=out_f32, accumulate=acc)) == (c.kid, c.kname)


def test_cases_cover_every_instance():
    assert set(F.INSTANCES) == ALL_INSTANCES and len(ALL_INSTANCES) == 17
    assert {(c.family, c.inst) for c in F.CASES} == ALL_INSTANCES
    for fam, inst in ALL_INSTANCES:
        views = {c.view for c in F.CASES if (c.family, c.inst) == (fam, inst)}
        want = {"plain", "view", "view8p"} if fam == "hpipe" else {"plain", "view", "view8", "view8p"}
        assert views == want, (fam, inst)
    assert {c.kid for c in F.CASES if c.family == "halo"} == {1116, 1110, 1016, 1020}
    assert any(c.oh % int(c.kname.split()[-1].split("x")[0]) for c in F.CASES if c.family == "halo")
    assert any(c.ow == 48 and c.kid == 1116 for c in F.CASES)             # three column tiles
    # tap-innermost with two channel chunks, on both tiles; the generic instance on 81-pixel maps over 3 images
    for kid in (2000, 2001):
        assert any(c.kid == kid and c.inst.endswith("TAP") and c.shape[3] == 128 for c in F.CASES)
        assert any(c.kid == kid and c.inst.endswith("GEN") and c.n == 3 and c.oh * c.ow == 81 for c in F.CASES)


def test_instances_are_the_launch_tables():
    """The 17 pairs against the launch code of the sources: a new forward instance there fails here."""
    pipe = (CSRC / "conv_pipe.hip").read_text()
    got = {("pipe", f"256x{bn} {inst[4:].replace('_', ' ')}")
           for inst, bn in re.findall(r"case (FWD_\w+):\s+conv_pipe_kernel<256, (\d+),", pipe)}
    direct = (CSRC / "conv_direct.hip").read_text()
    table = direct[direct.index("const Variant kVariants[] = {"):direct.index("#undef DIR_VARIANT")]
    rows = re.findall(r"^\s+(?:DIR_VARIANT\(|\{)(\d+), (\d+), (\d+), (\d+), (\d+), (\d+)", table, re.M)
    assert len(rows) == 8
    got |= {("direct", f"v{i}") for i, r in enumerate(rows) if r[4] == "0"}
    halo = (CSRC / "conv_halo.hip").read_text()
    tiles = set(re.findall(r"conv_halo_kernel<(\d), 2, 4, \d, \d, \d, H_FWD>", halo))
    got |= {("halo", {"4": "C8", "2": "C4"}[t]) for t in tiles}
    hp = (CSRC / "conv_hpipe.hip").read_text()
    assert len(re.findall(r"conv_hpipe_kernel<\d+, \d, \d, HF", hp)) == 3
    # cfg 1 (the 64-channel tile without resident weights) has a launch line and no plan: hpipe_plan returns before it
    assert "if (nout < 128 && !wres) return p;" in hp and "p.cfg = nout >= 128 ? 0 : (wres ? 2 : 1);" in hp
    got |= {("hpipe", "128"), ("hpipe", "64 wres")}
    conv = (CSRC / "conv.hip").read_text()
    body = conv[conv.index("static int launch_tile_k("):conv.index("static int launch_tile(")]
    got |= {("gemm", f"128x{bn}") for bn in re.findall(r"launch_gemm<128, (\d+),", body)}
    assert got == ALL_INSTANCES


def test_hpipe_refuses_the_odd_pitch_view():
    """hpipe_plan requires 8-channel pitches of the y view: its shapes under view8 run another family."""
    for c in (c for c in F.CASES if c.family == "hpipe" and c.view == "plain"):
        c8 = F.Case(c.name + "-8", c.family, c.inst, c.shape, c.kid, c.kname, view="view8", sel=c.sel)
        assert F.kernel(c8)[0] // 1000 != 4


def test_statistics_cap_case():
    """More m-tiles than rows: the 128x32 tile's grid is cut to 1024 / 16 channel tiles = 64 rows for 73 m-tiles."""
    (c,) = F.CAP_CASES
    assert F.stat_rows(c) == 64 and -(-c.pixels // 128) == 73 and c.cout // 32 == 16
    # and the small GEMM cases run two m-tiles under a grid of 8: six workgroups own no tile
    g = F.find(32, "plain")
    assert F.stat_rows(g) == 8 and -(-g.pixels // 128) == 2


@pytest.mark.parametrize("c", F.ALL_CASES, ids=F.case_id)
def test_buffers_and_canaries(c):
    n, h, w, cin, cout, k, s, p = c.shape
    ye, cy, y_gap, xe, cx, x_gap = F.VIEWS[c.view]
    assert xe % 8 == 0 and cx % 8 == 0 and x_gap % 8 == 0                # the ABI's 16-byte rule for x
    f32 = c.view == "wide"
    if not f32:
        assert c.y_ld % 4 == 0 and c.y_bs % 4 == 0 and cy % 4 == 0       # ... and its 8-byte rule for a 16-bit y
    assert c.aligned == (c.view in ("plain", "view"))
    if c.view == "view8":
        assert c.y_ld % 8 == 4 and cy == 0
    if c.view == "view8p":
        assert c.y_ld % 8 == 0 and c.y_bs % 8 == 0 and cy % 8 == 4
    if c.view == "view4":
        assert cout % 8 == 4 and c.y_ld % 8 == 0 and c.y_bs % 8 == 0 and cy == 0 and c.y_ld - cout == 4
    if c.view == "view6":
        assert cout % 4 == 2
    if c.view != "plain":
        assert c.y_ld > cout and c.x_ld > cin and cx > 0 and c.y_bs > c.oh * c.ow * c.y_ld
    run = _runs(c)[0]
    assert F.x_buffer(c, run).numel() == n * c.x_bs                      # asserts NaN everywhere outside the view
    assert F.weight_buffer(c, run).numel() == cout * k * k * cin
    out = F.outside_mask(c)
    assert int((~out).sum()) == c.pixels * cout
    of = 1 if f32 else 2
    buf = F.y_buffer(c, of)
    assert buf.numel() == n * c.y_bs and buf.numel() * buf.element_size() <= 10 * 2 ** 20
    assert torch.equal(buf[out], F.sentinel(n * c.y_bs, of)[out])
    assert bool(torch.isnan(buf.view(F.OUT_DTYPE[of]).float()).all())   # the view NaN, the sentinels NaN payloads
    st = F.stat_buffer(8, cout)
    assert bool(torch.isnan(st.view(torch.float32)).all()) and bool((st[8 * cout:] == F.STAT_CANARY).all())
    assert bool((st[:8 * cout] != F.STAT_CANARY).all())


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
    for c in F.ALL_CASES[::9]:
        F.kernel(c)
        F.stat_rows(c)
    assert snapshot() == before


def test_mismatch_names_the_first_element():
    c = F.find(64, "view")
    want = F.cast(F.reference(c, "A"), 2)
    got = want.clone()
    assert F.mismatch(c, got, want) is None
    got[1, 4, 7, 70] = got[1, 4, 7, 70] + 16
    got[1, 8, 10, 3] = float("nan")
    msg = F.mismatch(c, got, want)
    assert "2 of" in msg and "(image 1, y 4, x 7, channel 70)" in msg and "gemm 128x64" in msg
    assert f"want {float(want[1, 4, 7, 70])!r}" in msg
    z = torch.zeros(1, 1, 1, 1, dtype=torch.float16)
    assert F.bits(z).item() == 0 and bool((F.bits(-z) != F.bits(z)).all())      # -0 against +0 is a mismatch
