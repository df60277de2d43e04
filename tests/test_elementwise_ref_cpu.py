"""tests/elementwise_ref.py on its own, no GPU: the fp64 references against torch autograd / functional ops, the
rounding checker against planted faults (each one a way a streaming kernel goes subtly wrong and the whole-tensor
L2 bounds cannot see), and the budget K = 32 against fp32 restatements of the kernels' op order — the budget has to
be met by a correct fp32 implementation on the inputs the GPU tests use, or a GPU failure would prove nothing.
"""
import pytest
import torch
import torch.nn.functional as F

import elementwise_ref as ER


# ------------------------------------------------------------------------------------------------ references
def test_bn_apply_ref_equals_functional_batch_norm():
    g = torch.Generator().manual_seed(1)
    n, c, h, w = 3, 16, 5, 7
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64)
    gamma, beta = torch.rand(c, generator=g, dtype=torch.float64) + 0.5, torch.randn(c, generator=g, dtype=torch.float64)
    res = torch.randn(n, c, h, w, generator=g, dtype=torch.float64)
    eps = 1e-3
    mean, var = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)
    scale = gamma / torch.sqrt(var + eps)
    shift = beta - mean * scale
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, c)
    bn = F.batch_norm(x, None, None, gamma, beta, training=True, eps=eps)
    for act in (0, 1):
        want = (F.silu(bn) if act else bn) + res
        got, terms = ER.bn_apply_ref(rows(x), scale, shift, act, rows(res))
        assert float((got - rows(want)).abs().max()) < 1e-12
        assert bool((terms >= got.abs() - 1e-12).all())           # the terms bound the result they add up to
    got, _ = ER.bn_apply_ref(rows(x), scale, shift, 1, None)
    assert float((got - rows(F.silu(bn))).abs().max()) < 1e-12


@pytest.mark.parametrize("act", [0, 1])
def test_bn_bwd_apply_ref_equals_autograd(act):
    """BatchNorm (batch statistics, biased variance) + SiLU: with coef built from the true sums (k1 = gamma * rstd,
    k2 = mean(g), k3 = mean(g * xh)) the reference is dL/dz."""
    g = torch.Generator().manual_seed(2 + act)
    m, c, eps = 200, 16, 1e-3
    z = torch.randn(m, c, generator=g, dtype=torch.float64).requires_grad_(True)
    gamma, beta = torch.rand(c, generator=g, dtype=torch.float64) + 0.5, torch.randn(c, generator=g, dtype=torch.float64)
    dy = torch.randn(m, c, generator=g, dtype=torch.float64)
    mean, var = z.mean(0), z.var(0, unbiased=False)
    rstd = 1 / torch.sqrt(var + eps)
    t = (z - mean) * rstd * gamma + beta
    y = F.silu(t) if act else t
    (want,) = torch.autograd.grad(y, z, grad_outputs=dy)
    with torch.no_grad():
        scale = gamma * rstd
        shift = beta - mean * scale
        gg = dy
        if act:
            sg = torch.sigmoid(t)
            gg = dy * sg * (1 + t * (1 - sg))
        xh = (z - mean) * rstd
        coef = torch.stack([gamma * rstd, gg.mean(0), (gg * xh).mean(0)])
        got, terms = ER.bn_bwd_apply_ref(dy, z.detach(), scale, shift, mean, rstd, coef, act)
    assert float((got - want).abs().max()) < 1e-12
    assert bool((terms >= got.abs() - 1e-12).all())


def test_dw3x3_ref_channel_map_psa():
    """The PSA map (gsz 64, gstride 128, goff 64): conv channel j reads the v slice of head j // 64."""
    n, h, w, c = 2, 4, 5, 128
    d = ER.make_dw_inputs(n, h, w, c, 64, 128, 64)
    src = ER.dw_src_channels(c, 64, 128, 64)
    assert src.tolist() == list(range(64, 128)) + list(range(192, 256))
    z, terms = ER.dw3x3_ref(d["x"], d["w"], c, 64, 128, 64)
    # an independent restatement: the gathered channels through a dense loop over the taps
    xs = F.pad(d["x"][..., src].double(), (0, 0, 1, 1, 1, 1))
    want = torch.zeros(n, h, w, c, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            want += xs[:, kh:kh + h, kw:kw + w, :] * d["w"][:, kh * 3 + kw].double()
    assert float((z - want).abs().max()) < 1e-12
    assert bool((terms >= z.abs() - 1e-12).all())
    # channels outside the map do not matter
    x2 = d["x"].clone()
    other = torch.ones(d["ld"], dtype=torch.bool)
    other[src] = False
    x2[..., other] = 7.0
    assert torch.equal(ER.dw3x3_ref(x2, d["w"], c, 64, 128, 64)[0], z)


def test_dw3x3_bwd_ref_equals_autograd():
    n, h, w, c, gsz, gstride, goff = ER.DW_SHAPES[1]
    d = ER.make_dw_inputs(n, h, w, c, gsz, gstride, goff)
    x = d["x"].double().requires_grad_(True)
    src = ER.dw_src_channels(c, gsz, gstride, goff)
    wv = d["w"].double().requires_grad_(True)
    z = F.conv2d(x[..., src].permute(0, 3, 1, 2), wv.reshape(c, 1, 3, 3), padding=1, groups=c).permute(0, 2, 3, 1)
    gx, gw = torch.autograd.grad(z, (x, wv), grad_outputs=d["dz"].double())
    dx, terms, dw = ER.dw3x3_bwd_ref(d["x"], d["w"], d["dz"], c, gsz, gstride, goff)
    assert float((dx - gx[..., src]).abs().max()) < 1e-12
    assert float((dw - gw).abs().max()) < 1e-10
    assert bool((terms >= dx.abs() - 1e-12).all())
    other = torch.ones(d["ld"], dtype=torch.bool)
    other[src] = False
    assert float(gx[..., other].abs().max()) == 0.0


def test_head_grad_ref_layout():
    B, A, nc, a_off, hw = 2, 11, 9, 3, 5
    dh = torch.randn(B, A, 64 + nc, generator=torch.Generator().manual_seed(4))
    box, cls, sb, scl = ER.head_grad_ref(dh, a_off, hw, nc)
    assert box.shape == (B * hw, 64) and cls.shape == (B * hw, 16)
    assert torch.equal(box[hw + 2], dh[1, a_off + 2, :64].bfloat16())
    assert torch.equal(cls[hw + 2, :nc], dh[1, a_off + 2, 64:].bfloat16())
    assert int(ER.bits(cls[:, nc:]).abs().sum()) == 0             # padded columns +0, not -0
    assert float((sb - dh[:, a_off:a_off + hw, :64].double().sum((0, 1))).abs().max()) < 1e-12
    assert scl.shape == (nc,)


def test_bn_eval_coeff_ref():
    g = torch.Generator().manual_seed(5)
    c = 24
    gamma, beta, rm, rv = (torch.randn(c, generator=g), torch.randn(c, generator=g), torch.randn(c, generator=g),
                           torch.rand(c, generator=g) + 0.1)
    sc, sh = ER.bn_eval_coeff_ref(gamma, beta, rm, rv, 1e-3)
    x = torch.randn(4, c, 3, 3, generator=g, dtype=torch.float64)
    want = F.batch_norm(x, rm.double(), rv.double(), gamma.double(), beta.double(), training=False,
                        eps=float(torch.tensor(1e-3, dtype=torch.float32)))
    got = x * sc.view(1, c, 1, 1) + sh.view(1, c, 1, 1)
    assert float((got - want).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------------ the checker
def test_ulp_spacing():
    x = torch.tensor([0.0, 2.0 ** -30, 2.0 ** -14, 1.0, 1.5, 2.0, 65504.0], dtype=torch.float64)
    assert ER.ulp(x, "fp16").tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 32.0]
    assert ER.ulp(x[3:6], "bf16").tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6]
    # against torch's own next representable value
    for kind, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        v = torch.tensor([0.3, 1.0, 3.7, 100.0, 6e-5 if kind == "fp16" else 1e-30]).to(dt)
        nxt = ER.from_bits(ER.bits(v) + 1, kind)
        assert torch.equal(ER.ulp(v.double(), kind), nxt.double() - v.double())


def _bn_case(kind):
    """A small bn_apply (fp16) / bn_bwd_apply (bf16) problem: (reference, terms, the inputs)."""
    c, m = 24, 171
    if kind == "fp16":
        d = ER.make_bn_inputs(c, m)
        ref, terms = ER.bn_apply_ref(d["z"], d["scale"], d["shift"], 1, d["res"])
    else:
        d = ER.make_bn_bwd_inputs(c, m)
        ref, terms = ER.bn_bwd_apply_ref(d["dy"], d["z"], d["scale"], d["shift"], d["mean"], d["rstd"], d["coef"], 1)
    return ref, terms, d


@pytest.mark.parametrize("kind", ["fp16", "bf16"])
def test_checker_accepts_rne_with_no_slack(kind):
    ref, terms, _ = _bn_case(kind)
    assert ER.assert_rounded(ER.round16(ref, kind), ref, terms, kind, K=0) == 0.0


@pytest.mark.parametrize("kind", ["fp16", "bf16"])
def test_checker_catches_truncation(kind):
    ref, terms, _ = _bn_case(kind)
    got = ER.truncate16(ref, kind)
    assert bool((got.double().abs() <= ER.round16(ref, kind).double().abs()).all())
    assert float((got.double() - ref.clamp(-ER.F16_MAX, ER.F16_MAX)).abs().max()) > 0
    with pytest.raises(AssertionError, match="worst at"):
        ER.assert_rounded(got, ref, terms, kind)


@pytest.mark.parametrize("fill", ["nan", "pad"])
def test_checker_catches_unwritten_last_row(fill):
    ref, terms, _ = _bn_case("fp16")
    got = ER.round16(ref, "fp16")
    b = ER.bits(got)
    b[-1] = ER.NAN_BITS["fp16"] if fill == "nan" else ER.PAD_BITS["fp16"]
    with pytest.raises(AssertionError, match=r"worst at \(170, "):
        ER.assert_rounded(ER.from_bits(b, "fp16"), ref, terms, "fp16")


def test_checker_catches_swapped_channel_group():
    ref, terms, _ = _bn_case("fp16")
    got = ER.round16(ref, "fp16")
    got[:, 8:16], got[:, 16:24] = got[:, 16:24].clone(), got[:, 8:16].clone()
    with pytest.raises(AssertionError):
        ER.assert_rounded(got, ref, terms, "fp16")


def test_checker_catches_residual_from_next_row_on_one_row():
    ref, terms, d = _bn_case("fp16")
    res = d["res"].clone()
    res[100] = d["res"][101]
    bad, _ = ER.bn_apply_ref(d["z"], d["scale"], d["shift"], 1, res)
    with pytest.raises(AssertionError, match=r"worst at \(100, "):
        ER.assert_rounded(ER.round16(bad, "fp16"), ref, terms, "fp16")


def test_checker_catches_perturbed_silu():
    """SiLU evaluated at t * (1 + 2^-10): an error of the size of a truncated intermediate."""
    ref, terms, d = _bn_case("fp16")
    t = d["z"].double() * d["scale"].double() + d["shift"].double()
    tp = t * (1 + 2.0 ** -10)
    bad = tp * torch.sigmoid(tp) + d["res"].double()
    with pytest.raises(AssertionError):
        ER.assert_rounded(ER.round16(bad, "fp16"), ref, terms, "fp16")


def test_checker_catches_inf_where_the_store_clamps():
    ref = torch.tensor([7.0e4, -7.0e4], dtype=torch.float64)
    ok = torch.tensor([65504.0, -65504.0]).half()
    assert ER.assert_rounded(ok, ref, ref.abs(), "fp16") == 0.0
    with pytest.raises(AssertionError):
        ER.assert_rounded(torch.tensor([float("inf"), -65504.0]).half(), ref, ref.abs(), "fp16")


def test_bit_exact_helpers():
    a = torch.tensor([1.0, 1.0, 0.0, -0.0]).bfloat16()
    b = torch.tensor([2.0 ** -8, 3 * 2.0 ** -8, -0.0, -0.0]).bfloat16()      # ties: to even, down then up
    assert ER.bits(ER.add16(a, b)).tolist() == [0x3F80, 0x3F82, 0x0000, 0x8000]
    with pytest.raises(AssertionError, match="first at"):
        ER.assert_bits_equal(torch.tensor([0.0]).bfloat16(), torch.tensor([-0.0]).bfloat16())


# ------------------------------------------------------------------------------------------------ the budget
# a faithful fp32 implementation of each kernel's op order passes at K = 32 on every input the GPU tests use (the
# second-pass shapes are 10^7 elements: a few seconds each here)
@pytest.mark.parametrize("c,m", ER.BN_SHAPES)
def test_budget_met_by_fp32_bn_apply(c, m):
    d = ER.make_bn_inputs(c, m)
    worst = 0.0
    for act in (0, 1):
        for res in (None, d["res"]):
            ref, terms = ER.bn_apply_ref(d["z"], d["scale"], d["shift"], act, res)
            for fma in (False, True):
                y32, y16 = ER.bn_apply_f32(d["z"], d["scale"], d["shift"], act, res, fma)
                worst = max(worst, ER.assert_rounded(y16, ref, terms, "fp16", what=f"act{act} fma{fma}"))
                ER.assert_f32_close(y32.clamp(-ER.F16_MAX, ER.F16_MAX), ref.clamp(-ER.F16_MAX, ER.F16_MAX), terms)
    assert worst <= ER.K_FP32
    # the planted rows are there: an overflow that clamps, a subnormal SiLU
    t = d["z"].double() * d["scale"].double() + d["shift"].double()
    assert float(t.max()) > 69000.0
    silu = ER.bn_apply_ref(d["z"], d["scale"], d["shift"], 1)[0].abs()
    assert bool(((silu > 2.0 ** -24) & (silu < 2.0 ** -14)).any())
    assert float(t[t.abs() < 1e3].abs().max()) <= 24.5


@pytest.mark.parametrize("c,m", ER.BN_BWD_SHAPES)
def test_budget_met_by_fp32_bn_bwd_apply(c, m):
    d = ER.make_bn_bwd_inputs(c, m)
    t = d["z"].double() * d["scale"].double() + d["shift"].double()
    assert float(t.abs().max()) <= 24.5
    for act in (0, 1):
        ref, terms = ER.bn_bwd_apply_ref(d["dy"], d["z"], d["scale"], d["shift"], d["mean"], d["rstd"], d["coef"], act)
        for fma in (False, True):
            got = ER.bn_bwd_apply_f32(d["dy"], d["z"], d["scale"], d["shift"], d["mean"], d["rstd"], d["coef"], act, fma)
            assert ER.assert_rounded(got, ref, terms, "bf16", what=f"act{act} fma{fma}") <= ER.K_FP32


@pytest.mark.parametrize("shape", ER.DW_SHAPES)
def test_budget_met_by_fp32_dw3x3(shape):
    n, h, w, c, gsz, gstride, goff = shape
    d = ER.make_dw_inputs(*shape)
    ref, terms = ER.dw3x3_ref(d["x"], d["w"], c, gsz, gstride, goff)
    for fma in (False, True):
        got = ER.dw3x3_f32(d["x"], d["w"], c, gsz, gstride, goff, fma)
        assert ER.assert_rounded(got, ref, terms, "fp16", what=f"fma{fma}") <= ER.K_FP32
    # the grid inputs: z exact in fp16, whatever the op order
    d = ER.make_dw_inputs(*shape, grid=True)
    ref, terms = ER.dw3x3_ref(d["x"], d["w"], c, gsz, gstride, goff)
    assert torch.equal(ER.round16(ref, "fp16").double(), ref) and float(ref.abs().max()) > 0.5
    assert torch.equal(ER.dw3x3_f32(d["x"], d["w"], c, gsz, gstride, goff).double(), ref)
