"""The exact weight-gradient cases (tests/wgrad_exact_cases.py) hold their own conditions, without a GPU:

  * every case's fp64 reference is integral and within the 2^24 bound that makes fp32 summation order-free, and the
    fp32 CPU conv2d_weight of the same operands equals it exactly — the reference alone meets the exactness condition;
  * through the library's host entry points (pure host code, like tests/test_conv_routes_cpu.py): each case runs the
    kernel instance it is listed for, the instances covered are exactly the 24 that ym_conv_wgrad can launch, each
    split scenario has the split count (multiple of 8 or not: wg_tile's XCD-mapped block order) and the short last split
    it is there for, and the odd / even / single-unit cases of the paired-unit loops have those unit counts.
"""
import ctypes

import pytest
import torch

import wgrad_exact_cases as W

# the weight-gradient instances of csrc/wgrad.hip (wg3_launch: 2 strides x 4 channel tilings x {db | plain, deep db}
# + 2 x 2 whole-row units; wgrad1 64 / 128; generic 64 / 128).  A 25th instance fails test_cases_cover_every_instance
# until a case exists for it.
ALL_IDS = {13002, 13003, 13102, 13103, 13202, 13203, 13302, 13303, 13012, 13022,
           13500, 13503, 13600, 13603, 13700, 13703, 13800, 13803, 13510, 13520,
           11064, 11128, 10064, 10128}


@pytest.mark.parametrize("c", W.CASES, ids=W.case_id)
def test_reference_is_exact(c):
    ref = W.reference(c)                                     # asserts integral and the bound with the prefill
    assert ref.dtype == torch.float64
    assert torch.equal(ref, ref.round())
    assert W.exact_bound(c, W.PREFILL_MAX) < 2 ** 24
    assert float(ref.abs().max()) + W.PREFILL_MAX < 2 ** 24
    assert float(W.prefill(c).abs().max()) <= W.PREFILL_MAX
    assert torch.equal(W.reference_f32(c).double(), ref)
    if c.pin:
        assert c.m < 8192
        x, _ = W.operands(c)
        r = x.bfloat16().float()
        for v, want in ((257.0, 256.0), (-257.0, -256.0), (259.0, 260.0), (-259.0, -260.0)):
            sel = x.float() == v
            assert bool(sel.any()) and bool((r[sel] == want).all())
        # the ties matter: a reference on the unrounded x differs
        n, h, w, cin, cout, k, s, p = c.shape
        _, dz = W.operands(c)
        raw = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), (cout, cin, k, k),
                                          dz.double().permute(0, 3, 1, 2), stride=s, padding=p)
        assert not torch.equal(raw, ref)


@pytest.mark.parametrize("c", W.CASES, ids=W.case_id)
def test_operands_and_views(c):
    x, dz = W.operands(c)
    assert x.dtype == torch.float16 and dz.dtype == torch.bfloat16
    small = x.float().abs() <= 4
    assert bool(small.all()) != c.pin and bool((dz.float().abs() <= 4).all())
    assert torch.equal(x.float(), x.float().round()) and torch.equal(dz.float(), dz.float().round())
    for v in (c.xe, c.ye, c.cx, c.cy, c.x_gap):
        assert v % 8 == 0
    xbuf, dzbuf = W.buffers(c)                               # asserts every element outside the views is NaN
    assert xbuf.numel() == c.n * c.x_bs and dzbuf.numel() == c.n * c.y_bs
    d = W.desc(c)
    assert (d.x_ld > d.cin and d.y_ld > d.cout) == c.viewed


def test_every_instance_plain_and_viewed():
    for kid in ALL_IDS:
        cs = [c for c in W.CASES if c.kid == kid]
        assert any(c.xe == c.ye == c.cx == c.cy == 0 for c in cs), kid
        assert any(c.viewed for c in cs), kid
    assert {c.kid // 1000 for c in W.PIN_CASES} == {13, 11, 10}       # one rounding pin per kernel family


@pytest.mark.parametrize("c", W.CASES, ids=W.case_id)
def test_case_runs_its_instance(c):
    from yolomi._lib import lib
    d = W.desc(c)
    name = ctypes.create_string_buffer(96)
    with W.wgrad_target(c):
        assert lib().ym_conv_kernel(ctypes.byref(d), 2, name, 96) == c.kid
    assert name.value.decode() == W.INSTANCES[c.kid]
    assert W.kernel_id(c) == c.kid


def test_cases_cover_every_instance():
    assert {W.kernel_id(c) for c in W.CASES} == ALL_IDS
    assert set(W.INSTANCES) == ALL_IDS and len(ALL_IDS) == 24


@pytest.mark.parametrize("c", W.SPLIT_CASES, ids=W.case_id)
def test_split_scenarios(c):
    from yolomi._lib import lib
    before = lib().ym_wgrad_set_target(0)
    lib().ym_wgrad_set_target(before)
    splits, chunk, counts = W.split_plan(c)
    assert lib().ym_wgrad_set_target(before) == before       # the setter was restored
    assert splits == c.splits and sum(counts) == W.unit_count(c) and min(counts) >= 1
    assert c.xcd in (0, 1) and (splits % 8 == 0) == bool(c.xcd)
    if c.chunk:
        assert (chunk, counts[-1]) == (c.chunk, c.tail) and c.tail < c.chunk


def test_split_scenarios_cover_both_block_orders():
    plans = {c.name: W.split_plan(c) for c in W.SPLIT_CASES}
    mapped = [n for n, (s, _, _) in plans.items() if s % 8 == 0]
    plain_wide = [n for n, (s, _, _) in plans.items() if s >= 8 and s % 8]
    assert mapped and plain_wide                              # xcd_map on, and off at >= 8 splits
    assert any(s % 8 == 0 and counts[-1] < chunk for s, chunk, counts in plans.values())     # mapped, short tail
    assert any(c.target and c.kid // 1000 == 13 for c in W.SPLIT_CASES)
    assert any(c.target and c.kid // 1000 == 11 for c in W.SPLIT_CASES)
    # the reduce kernel: 4 split lanes, 16 splits per unrolled trip; trips only, remainder only, both
    rem = {(s > 12, (s % 16) != 0) for s, _, _ in plans.values()}
    assert {(True, False), (False, True), (True, True)} <= rem
    # the setter moves the plan: the same shape under three targets
    same = sorted(s for n, (s, _, _) in plans.items() if n.startswith("13002-n2h64w48"))
    assert same == [4, 8, 16]


@pytest.mark.parametrize("c", W.UNIT_CASES, ids=W.case_id)
def test_unit_parity_cases(c):
    assert c.kid in W.PAIRED_IDS
    splits, chunk, counts = W.split_plan(c)
    if c.units == "odd":
        assert any(k % 2 == 1 and k > 1 for k in counts)     # a pair padded with a unit of zeros, after whole pairs
    elif c.units == "even":
        assert all(k % 2 == 0 for k in counts)               # whole pairs only
    else:
        assert c.units == "single" and 1 in counts


def test_unit_parities_cover_paired_kernels():
    for kid in W.PAIRED_IDS:
        kinds = {c.units for c in W.UNIT_CASES if c.kid == kid}
        assert {"odd", "even"} <= kinds, kid
    assert any(c.units == "single" and c.kid in W.DEEP_IDS for c in W.UNIT_CASES)
    for kid in (11064, 11128):
        assert any(c.units == "single" and c.kid == kid for c in W.UNIT_CASES)


def test_empty_batch_plans():
    """n = 0: the plan has no units; the workspace query still answers (one partial), for every kernel family."""
    from yolomi._lib import lib
    for kid in (13002, 13503, 11064, 10064):
        c = next(c for c in W.INSTANCE_CASES if c.kid == kid)
        d = W.desc(c, n=0)
        assert lib().ym_conv_wgrad_workspace_size(ctypes.byref(d)) == 4 * c.elems
        assert lib().ym_conv_kernel(ctypes.byref(d), 2, None, 0) == kid


def test_mismatch_names_the_first_element():
    c = next(c for c in W.INSTANCE_CASES if c.kid == 13002 and c.viewed)          # 64 -> 72: 2 co tiles of 64
    ref = W.reference(c)
    got = ref.float()
    assert W.mismatch(c, got, ref) is None
    got[70, 33, 1, 2] += 1
    got[71, 0, 0, 0] = float("nan")
    msg = W.mismatch(c, got, ref)
    assert "2 of" in msg and "(co 70, ci 33, kh 1, kw 2)" in msg and "channel tile (co 1, ci 0)" in msg
    assert f"want {float(ref[70, 33, 1, 2])!r}" in msg and "wgrad3 s1 64x64 8x8 db" in msg
    assert W.tile_of(next(c for c in W.CASES if c.kid == 13703), 40, 40) == (0, 1)  # 64-co x 32-ci tiles
    assert W.tile_of(next(c for c in W.CASES if c.kid == 13103), 40, 40) == (1, 0)  # 32-co x 64-ci tiles
    assert W.tile_of(next(c for c in W.CASES if c.kid == 11128), 130, 90) == (1, 0)


def test_one_dropped_product_shows_at_size():
    """At M = 98304 one output pixel's dz = 1 dropped for one channel moves <= 9 * cin elements by <= 4: the exact
    comparison rejects it, the 1e-3-of-max|dw| bound of test_conv_kernels_vs_torch would let it pass."""
    c = next(c for c in W.SPLIT_CASES if c.name.endswith("reduce128"))
    n, h, w, cin, cout, k, s, p = c.shape
    x, dz = W.operands(c)
    ref = W.reference(c)
    pos = (dz[:, 20:40, 20:40] == 1).nonzero()[0]
    img, oh, ow, co = int(pos[0]), int(pos[1]) + 20, int(pos[2]) + 20, int(pos[3])
    dropped = dz.clone()
    dropped[img, oh, ow, co] = 0
    got = torch.nn.grad.conv2d_weight(x.float().permute(0, 3, 1, 2), (cout, cin, k, k),
                                      dropped.float().permute(0, 3, 1, 2), stride=s, padding=p)
    msg = W.mismatch(c, got, ref)
    assert msg is not None and f"(co {co}," in msg
    diff = (got.double() - ref).abs()
    assert 0 < int((diff > 0).sum()) <= 9 * cin and float(diff.max()) <= 4
    assert float(diff.max()) < 1e-3 * float(ref.abs().max())
