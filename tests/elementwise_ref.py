"""fp64 references, input generators and the rounding checker of the streaming elementwise kernels (bn.hip
bn_apply / bn_bwd_apply, conv.hip dw3x3, misc.hip head_grad and the view conversions).  Plain torch, no GPU needed:
tests/test_elementwise_ref_cpu.py keeps this file honest, tests/test_gpu_elementwise.py holds the kernels to it
(there the same functions run on the device tensors, in fp64).

Every reference takes the operands exactly as the kernel reads them (the stored fp16 / bf16 tensors, the fp32
vectors), evaluates in fp64 and returns the unrounded value together with `terms_abs`, the sum of the absolute
values of the terms the kernel adds in fp32.  The checker then asks, per element,

    |got - ref| <= 0.5 * ulp16(max(|got|, |ref|)) + K * 2^-24 * terms_abs

i.e. the one rounding to the 16-bit output type plus K half-ulps of fp32 arithmetic on the terms.  K = 32 comes
from the kernels' code, not from their output: at most 6 fp32 roundings of 1/2 ulp, v_rcp_f32 at ~1 ulp, and
__expf (v_exp_f32 of t * log2 e), whose argument scaling costs about |t| * 2^-24 relative — hence |t| <= 24 in
the generated inputs (the planted overflow rows aside, where the sigmoid has saturated to 1).
"""
import math

import torch
import torch.nn.functional as F

K_FP32 = 32
F16_MAX = 65504.0

# 16-bit formats: (mantissa bits without the hidden one, exponent of the smallest normal)
_FMT = {"fp16": (10, -14), "bf16": (7, -126)}
_DTYPE = {"fp16": torch.float16, "bf16": torch.bfloat16}

# sentinels of the GPU tests: NaN where a kernel must write, these where it must not
PAD_BITS = {"fp16": 0x7BAD, "bf16": 0xBAAD}
NAN_BITS = {"fp16": 0x7E00, "bf16": 0x7FC0}
F32_PAD_BITS = 0x7FBADBAD            # a NaN with a payload: no kernel produces it


def kind_of(t):
    return {torch.float16: "fp16", torch.bfloat16: "bf16"}[t.dtype]


def ulp(mag64, kind):
    """Spacing of the 16-bit format `kind` at magnitude mag64 (fp64 tensor); the subnormal spacing below the
    smallest normal."""
    mant, emin = _FMT[kind]
    return _spacing(mag64, mant, emin)


def ulp32(mag64):
    return _spacing(mag64, 23, -126)


def _spacing(mag64, mant, emin):
    _, e = torch.frexp(mag64.abs())                 # |x| = f * 2^e, f in [0.5, 1): floor(log2 |x|) = e - 1
    e = torch.where(mag64 == 0, torch.full_like(e, emin), e - 1).clamp_min(emin)
    return ((e - mant + 1023).to(torch.int64) << 52).view(torch.float64)       # 2^(e - mant), exactly


def bits(t):
    """The raw 16-bit patterns of an fp16 / bf16 tensor as int32 (0..65535)."""
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def from_bits(b, kind):
    b = torch.as_tensor(b, dtype=torch.int32)
    return torch.where(b >= 32768, b - 65536, b).to(torch.int16).view(_DTYPE[kind])


def _unravel(i, shape):
    idx = []
    for d in reversed(shape):
        idx.append(i % d)
        i //= d
    return tuple(reversed(idx))


def round16(ref64, kind):
    """fp64 -> fp32 -> 16 bits, round to nearest even, fp16 clamped to +-65504 as the kernels' pk2h does."""
    if kind == "fp16":
        ref64 = ref64.clamp(-F16_MAX, F16_MAX)
    return ref64.float().to(_DTYPE[kind])


def truncate16(ref64, kind):
    """fp64 -> 16 bits rounded TOWARDS ZERO (the fault the checker has to see)."""
    r = round16(ref64, kind)
    b = bits(r)
    over = r.double().abs() > ref64.abs()
    return from_bits(torch.where(over, b - 1, b), kind)   # sign-magnitude: one step towards zero


def assert_rounded(got16, ref64, terms_abs64, kind=None, K=K_FP32, what=""):
    """Hold a kernel's 16-bit output to its fp64 reference: one rounding to `kind` plus K * 2^-24 * terms_abs of fp32
    arithmetic.  fp16 references are clamped to +-65504 first (the stores clamp instead of producing inf).  Returns
    the largest fp32 slack actually used, (|got - ref| - 0.5 ulp) / (2^-24 * terms_abs), floored at 0."""
    kind = kind or kind_of(got16)
    got = got16.double()
    ref = ref64.double()
    if kind == "fp16":
        ref = ref.clamp(-F16_MAX, F16_MAX)
    terms = terms_abs64.double().expand_as(ref)
    half = 0.5 * ulp(torch.maximum(got.abs(), ref.abs()).nan_to_num(nan=0.0, posinf=F16_MAX), kind)
    unit = 2.0 ** -24 * terms
    err = (got - ref).abs()
    budget = half + K * unit
    bad = ~(err <= budget)                          # a NaN fails
    if bool(bad.any()):
        over = torch.where(bad, (err - budget).nan_to_num(nan=math.inf, posinf=math.inf), torch.full_like(err, -1.0))
        i = int(over.reshape(-1).argmax())
        idx = _unravel(i, err.shape)
        g16 = got16.reshape(-1)[i:i + 1]
        r16 = round16(ref.reshape(-1)[i:i + 1], kind)
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements off; worst at {idx}: got {float(got.reshape(-1)[i])!r} "
            f"(bits {int(bits(g16)):#06x}) ref {float(ref.reshape(-1)[i])!r} (rounds to bits {int(bits(r16)):#06x}) "
            f"|err| {float(err.reshape(-1)[i]):.6g} > budget {float(budget.reshape(-1)[i]):.6g} "
            f"(half ulp {float(half.reshape(-1)[i]):.6g} + {K} * 2^-24 * terms {float(terms.reshape(-1)[i]):.6g})")
    used = torch.where(unit > 0, (err - half) / unit, torch.zeros_like(err))
    return max(0.0, float(used.max())) if used.numel() else 0.0


def worst_slack_index(got16, ref64, terms_abs64, kind):
    """Flat index of the element that used the most fp32 slack (for the report of where a kernel spends its budget)."""
    got, ref = got16.double(), ref64.double()
    if kind == "fp16":
        ref = ref.clamp(-F16_MAX, F16_MAX)
    unit = 2.0 ** -24 * terms_abs64.double().expand_as(ref)
    half = 0.5 * ulp(torch.maximum(got.abs(), ref.abs()), kind)
    used = torch.where(unit > 0, ((got - ref).abs() - half) / unit, torch.zeros_like(ref))
    return int(used.reshape(-1).argmax())


def assert_f32_close(got32, ref64, terms_abs64, K=K_FP32, what=""):
    """The fp32 copy of a result: the same fp32 arithmetic budget, and its own rounding to fp32."""
    got, ref = got32.double(), ref64.double()
    unit = 2.0 ** -24 * terms_abs64.double().expand_as(ref)
    err = (got - ref).abs()
    budget = 0.5 * ulp32(ref) + K * unit
    bad = ~(err <= budget)
    if bool(bad.any()):
        i = int(torch.where(bad, err - budget, torch.full_like(err, -1.0)).nan_to_num(nan=math.inf).reshape(-1).argmax())
        raise AssertionError(f"{what}: {int(bad.sum())} fp32 elements off; worst flat index {i}: got "
                             f"{float(got.reshape(-1)[i])!r} ref {float(ref.reshape(-1)[i])!r} budget "
                             f"{float(budget.reshape(-1)[i]):.6g}")
    used = torch.where(unit > 0, err / unit, torch.zeros_like(err))
    return float(used.max()) if used.numel() else 0.0


def assert_bits_equal(got16, want16, what=""):
    g, w = bits(got16), bits(want16)
    bad = g != w
    if bool(bad.any()):
        i = int(bad.reshape(-1).to(torch.int32).argmax())
        idx = _unravel(i, g.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} bit patterns differ; first at {idx}: got "
                             f"{int(g.reshape(-1)[i]):#06x} want {int(w.reshape(-1)[i]):#06x}")


def sum_rule_err(got, ref64):
    """The project's rule for reordered fp32 sums (tests/test_gpu_bn.py): relative to the sum's magnitude, floored at
    1 % of the largest one (a sum can cancel to ~0).  The caller asserts < 1e-4."""
    got, ref = got.double(), ref64.double()
    return float(((got - ref).abs() / (ref.abs() + 1e-2 * ref.abs().max())).max())


def add16(a16, b16):
    """a + b of two 16-bit tensors as the kernels do it: both widened to fp32 (exact), one fp32 add, one RNE."""
    return (a16.float() + b16.float()).to(a16.dtype)


# ------------------------------------------------------------------------------------------------ BatchNorm apply
def bn_apply_ref(z16, scale, shift, act, res16=None):
    """ym_bn_apply: t = z * scale + shift; y = t * sigmoid(t) if act else t; + res.  -> (y64, terms_abs64)."""
    z, sc, sf = z16.double(), scale.double(), shift.double()
    t = z * sc + sf
    y = t * torch.sigmoid(t) if act else t
    terms = (z * sc).abs() + sf.abs()
    if res16 is not None:
        y = y + res16.double()
        terms = terms + res16.double().abs()
    return y, terms


def bn_bwd_apply_ref(dy16, z16, scale, shift, mean, rstd, coef, act):
    """ym_bn_bwd_apply: g = dy * sg * (1 + t * (1 - sg)) if act else dy; xh = (z - mean) * rstd;
    dz = k1 * (g - k2 - xh * k3) with coef = [k1; k2; k3].  -> (dz64, terms_abs64)."""
    z, dy = z16.double(), dy16.double()
    g = dy
    if act:
        t = z * scale.double() + shift.double()
        sg = torch.sigmoid(t)
        g = dy * (sg * (1 + t * (1 - sg)))
    xh = (z - mean.double()) * rstd.double()
    k1, k2, k3 = (k.double() for k in coef)
    dz = k1 * (g - k2 - xh * k3)
    terms = k1.abs() * (g.abs() + k2.abs() + (xh * k3).abs())
    return dz, terms


def bn_eval_coeff_ref(gamma, beta, rm, rv, eps):
    """ym_bn_eval_coeff: scale = gamma / sqrt(var + eps), shift = beta - mean * scale (eps as the fp32 the ABI takes)."""
    e = float(torch.tensor(eps, dtype=torch.float32))
    sc = gamma.double() / torch.sqrt(rv.double() + e)
    return sc, beta.double() - rm.double() * sc


# ------------------------------------------------------------------------------------------------ depthwise 3x3
def dw_src_channels(c, gsz, gstride, goff):
    """Source channel of conv channel j in the x view: (j // gsz) * gstride + goff + j % gsz."""
    j = torch.arange(c)
    return (j // gsz) * gstride + goff + j % gsz


def dw3x3_ref(x16, w, c, gsz, gstride, goff):
    """ym_dw3x3_fwd: depthwise 3x3 s1 p1 over the gathered source channels of the (n, h, w, ld) view x16 with the
    fp32 weights w [c][9].  -> (z64 (n, h, w, c), terms_abs64 = sum over the taps of |w * x|)."""
    src = dw_src_channels(c, gsz, gstride, goff).to(x16.device)
    xs = x16[..., src].double().permute(0, 3, 1, 2)
    w4 = w.double().reshape(c, 1, 3, 3)
    z = F.conv2d(xs, w4, padding=1, groups=c)
    terms = F.conv2d(xs.abs(), w4.abs(), padding=1, groups=c)
    return z.permute(0, 2, 3, 1).contiguous(), terms.permute(0, 2, 3, 1).contiguous()


def dw3x3_bwd_ref(x16, w, dz16, c, gsz, gstride, goff):
    """ym_dw3x3_bwd: -> (dx64 (n, h, w, c) in conv channel order — channel j belongs at source channel
    dw_src_channels[j] of the dx view — its terms_abs64, dw64 [c][9])."""
    src = dw_src_channels(c, gsz, gstride, goff).to(x16.device)
    xs = x16[..., src].double().permute(0, 3, 1, 2)
    w4 = w.double().reshape(c, 1, 3, 3)
    dz = dz16.double().permute(0, 3, 1, 2)
    # dx[h, w] = sum dz[h + 1 - kh, w + 1 - kw] * w[kh, kw]: the correlation with the flipped kernel
    dx = F.conv2d(dz, w4.flip(2, 3), padding=1, groups=c)
    terms = F.conv2d(dz.abs(), w4.abs().flip(2, 3), padding=1, groups=c)
    wv = w4.clone().requires_grad_(True)
    (dw,) = torch.autograd.grad(F.conv2d(xs, wv, padding=1, groups=c), wv, grad_outputs=dz)
    return dx.permute(0, 2, 3, 1).contiguous(), terms.permute(0, 2, 3, 1).contiguous(), dw.reshape(c, 9)


# ------------------------------------------------------------------------------------------------ Detect gradient split
def head_grad_ref(dhead, a_off, hw, nc):
    """ym_head_grad on the level [a_off, a_off + hw) of dhead (B, A, 64 + nc) fp32: -> (dz_box bf16 (B * hw, 64),
    dz_cls bf16 (B * hw, ncp) with the padded columns +0, fp64 column sums of the box and the class rows)."""
    B = dhead.shape[0]
    lvl = dhead[:, a_off:a_off + hw, :].reshape(B * hw, 64 + nc)
    ncp = (nc + 7) // 8 * 8
    box = lvl[:, :64].bfloat16()
    cls = torch.zeros(B * hw, ncp, dtype=torch.bfloat16, device=dhead.device)
    cls[:, :nc] = lvl[:, 64:].bfloat16()
    return box, cls, lvl[:, :64].double().sum(0), lvl[:, 64:].double().sum(0)


# ------------------------------------------------------------------------------------------------ generated inputs
# (C, m) of the BatchNorm apply tests.  lanes() in bn.hip maps a 256-thread block to rows = 256 // (C / 8) pixel rows;
# the grid is capped at 2048 blocks, an iteration covers the row pair (m, m + 2048 * rows): the large shapes run a
# second grid-stride pass whose partner row falls past M.
BN_SHAPES = [(8, 1), (8, 255), (8, 257), (24, 171), (136, 15 * 7 + 1), (2048, 3),
             (2048, 2 * 2048 + 2048 + 5), (136, 2 * 2048 * 15 + 15 * 1000 + 7), (8, 2 * 2048 * 256 + 256 * 100 + 3)]
BN_BWD_SHAPES = BN_SHAPES[:3] + BN_SHAPES[6:]
T_PLANTED = (0.0, 24.0, -15.0, -24.0)       # -15: SiLU(-15) = -4.6e-6, an fp16 subnormal
T_OVERFLOW = 7.0e4                           # past the fp16 range: must store 65504, not inf


def _plant(z, scale, shift, targets):
    """Rows (all 8-channel lanes of them when m >= 8, else every 6th channel of row 0) whose t = z * scale + shift
    lands on the targets, as near as the fp16 z allows."""
    m, c = z.shape
    sc = torch.where(scale == 0, torch.ones_like(scale), scale)
    for k, tgt in enumerate(targets):
        zt = ((tgt - shift) / sc).clamp(-F16_MAX, F16_MAX).half()
        if m >= 8:
            z[(k * 37 + 3) % m] = zt
        else:
            z[0, k::len(targets) + 1] = zt[k::len(targets) + 1]


def make_bn_inputs(c, m, seed=0, overflow=True):
    """ym_bn_apply operands on the CPU: z fp16 (m, c) with the planted rows, res fp16 (m, c), scale = 1 +- 0.1 randn
    with a negative, a zero and (for the overflow row) an exact 1.25 entry, shift = 0.1 randn."""
    g = torch.Generator().manual_seed(1000 * c + m % 1000 + seed)
    z = torch.randn(m, c, generator=g).half()
    res = torch.randn(m, c, generator=g).half()
    scale = 1 + 0.1 * torch.randn(c, generator=g)
    shift = 0.1 * torch.randn(c, generator=g)
    scale[0] = -scale[0]
    scale[1] = 1.25
    scale[c // 2] = 0.0
    scale[c - 1] = -0.75
    _plant(z, scale, shift, T_PLANTED[:1] + ((T_OVERFLOW,) if overflow else ()) + T_PLANTED[1:])   # overflow on channel 1
    return {"z": z, "res": res, "scale": scale, "shift": shift}


def make_bn_bwd_inputs(c, m, seed=0):
    """ym_bn_bwd_apply operands: the forward's z / scale / shift (|t| <= 24), dy bf16, mean, rstd and coef [3][c]."""
    d = make_bn_inputs(c, m, seed + 7, overflow=False)
    g = torch.Generator().manual_seed(77 * c + m % 1000 + seed)
    d["dy"] = torch.randn(m, c, generator=g).bfloat16()
    d["dres"] = torch.randn(m, c, generator=g).bfloat16()
    # last row: dres + dy are bf16 rounding ties (to even: down, then up), and the signed zeros
    d["dy"][-1, :8] = torch.tensor([2.0 ** -8, 3 * 2.0 ** -8, -2.0 ** -8, -3 * 2.0 ** -8, 0.0, -0.0, 0.0, -0.0]).bfloat16()
    d["dres"][-1, :8] = torch.tensor([1.0, 1.0, -1.0, -1.0, 0.0, -0.0, -0.0, 0.0]).bfloat16()
    d["mean"] = 0.05 * torch.randn(c, generator=g)
    d["rstd"] = 1 + 0.1 * torch.rand(c, generator=g)
    gamma = 1 + 0.1 * torch.randn(c, generator=g)
    d["coef"] = torch.stack([gamma * d["rstd"], 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)])
    return d


# (n, h, w, c, gsz, gstride, goff) of the depthwise tests
DW_SHAPES = [(1, 1, 1, 8, 8, 8, 0), (2, 5, 3, 24, 8, 16, 8), (2, 20, 20, 128, 64, 128, 64),
             (1, 7, 9, 384, 64, 128, 64)]


def make_dw_inputs(n, h, w, c, gsz, gstride, goff, seed=0, grid=False):
    """x view (n, h, w, ld) fp16 with ld = the source channels the map spans + 8, w fp32 [c][9], dz bf16 (n, h, w, c).
    x and w lean positive (0.5 + randn, 0.25 + 0.3 randn) so that the per-channel statistics are sums that do not cancel —
    the 1e-4 rule for them is relative to the sum.
    grid=True: x multiples of 1/8 in [-3, 4], w multiples of 1/4 in [-1, 1.5]: every product is a multiple of 2^-5 and
    |z| <= 54, so z is exact in fp32 AND in fp16.  ym_dw3x3_fwd sums its statistics from the fp32 values before the
    fp16 store; only on such inputs are they sums of the very numbers it stored."""
    g = torch.Generator().manual_seed(n * 1000 + h * 100 + w * 10 + c + seed)
    ld = (int(dw_src_channels(c, gsz, gstride, goff).max()) + 1 + 7) // 8 * 8 + 8
    x = 0.5 + torch.randn(n, h, w, ld, generator=g)
    wt = 0.25 + 0.3 * torch.randn(c, 9, generator=g)
    if grid:
        x, wt = ((x * 8).round() / 8).clamp(-3, 4), ((wt * 4).round() / 4).clamp(-1, 1.5)
    dz = torch.randn(n, h, w, c, generator=g).bfloat16()
    return {"x": x.half(), "w": wt.float(), "dz": dz, "ld": ld}


# ------------------------------------------------------------------------------------------------ fp32 restatements
# The kernels' op order in IEEE fp32 on the CPU (division and exp correctly rounded): what a faithful implementation
# gives.  fma=True contracts a * b + c into one rounding (evaluated in fp64 — the product of an fp16 / bf16 and an fp32
# value is exact there — then rounded to fp32), as the compiler is free to.
def _f32(x):
    return x.float()


def _mad(a, b, c, fma):
    if fma:
        return (a.double() * b.double() + c.double()).float()
    return _f32(_f32(a * b) + c)


def _sigmoid32(t):
    e = torch.exp(-t.double()).float()           # exp in fp64, rounded to fp32
    return 1.0 / (1.0 + e)                       # fp32 add, fp32 division


def bn_apply_f32(z16, scale, shift, act, res16=None, fma=False):
    """-> (y fp32 before the 16-bit store, fp16 as stored)."""
    t = _mad(z16.float(), scale, shift, fma)
    y = t * _sigmoid32(t) if act else t
    if res16 is not None:
        y = y + res16.float()
    return y, y.clamp(-F16_MAX, F16_MAX).half()


def bn_bwd_apply_f32(dy16, z16, scale, shift, mean, rstd, coef, act, fma=False):
    z, dy = z16.float(), dy16.float()
    g = dy
    if act:
        t = _mad(z, scale, shift, fma)
        sg = _sigmoid32(t)
        one_m = 1.0 - sg
        g = dy * (sg * _mad(t, one_m, torch.ones_like(t), fma))
    xh = (z - mean) * rstd
    k1, k2, k3 = coef
    inner = g - k2
    inner = _mad(-xh, k3, inner, fma)
    return (k1 * inner).bfloat16()


def dw3x3_f32(x16, w, c, gsz, gstride, goff, fma=False):
    """Tap by tap in (kh, kw) order, fp32 accumulate, skipped taps outside the map; -> fp16 (n, h, w, c)."""
    src = dw_src_channels(c, gsz, gstride, goff)
    xs = x16[..., src].float()
    n, h, wd, _ = xs.shape
    xp = F.pad(xs, (0, 0, 1, 1, 1, 1))
    s = torch.zeros(n, h, wd, c)
    for kh in range(3):
        for kw in range(3):
            s = _mad(xp[:, kh:kh + h, kw:kw + wd, :], w[:, kh * 3 + kw], s, fma)
    return s.clamp(-F16_MAX, F16_MAX).half()
