"""fp64 reference, rounding budgets, input generators and a rounding-order emulation of the attention core
(csrc/attn.hip: attn_fwd_kernel, attn_bwd_pre_kernel, attn_bwd_kv_kernel, attn_bwd_q_kernel).  Plain torch, no GPU
needed: tests/test_attention_ref_cpu.py keeps this file honest, tests/test_gpu_attention.py holds the kernels to it
(there the same functions run on the device tensors, in fp64).

The reference takes the operands exactly as the kernels read them (fp16 q / k / v, bf16 dO, the fp16 O that
attn_bwd_pre_kernel reads for D = sum_d dO * O), evaluates in fp64 and returns the unrounded values together with
`terms_abs`, the sums of the magnitudes the kernels' roundings act on.  The checker asks, per element,

    |got - ref| <= 0.5 * ulp16(max(|got|, |ref|)) + (lead + K * 2^-24) * terms_abs + floor

The leading constants (from the kernel code, not from its output; second-order products of two roundings are left to
the slack of the first-order count):

  out (fp16)  lead = 2^-11: P = exp(s - m) is rounded ONCE to fp16 (pack_h) before the PV MFMA, l is summed from the
              unrounded P.  terms T_out = softmax @ |v|.
              floor = N * 2^-25 * max|v|: a P entry below the fp16 normal range 2^-14 is off by up to half the subnormal
              spacing, 2^-25, absolutely; l >= 1 at the final maximum and every later alpha is <= 1.  The build line
              (csrc/Makefile) has no denormal-flushing flag and the MFMA keeps subnormal fp16 A / B operands (the
              kernels' default mode keeps fp16 / fp64 denormals), so the floor is NOT widened to N * 2^-14 * max|v|.
  dv (bf16)   lead = 2^-8: P = exp(s * scale - lse) rounded once to bf16 (pack_bf).  terms T_v = P^T @ |dO|.
  dq, dk      lead = 3 * 2^-8: dS to bf16, the K / Q operand fp16 -> bf16 (h8_to_bf8), V fp16 -> bf16 inside
  (bf16)      dP = dO V^T.  With A = P * (|dO| @ |v|^T + sum_d |dO * O|) — what the V rounding and the fp32 cancellation
              dP - D act on — terms T_q = scale * (|dS| + A) @ |k|, T_k = scale * (|dS| + A)^T @ |q|;
              3 (|dS| + A) covers 2 |dS| + A.
  bf16 has fp32's exponent range: no floor for the gradients.

K, the fp32 part, in units of 2^-24 = one half ulp relative (k_fwd / k_bwd below).  Rigorous worst-case counts; they
are small against the leading constants, which is what the K = 0 run of the emulation in the CPU test shows:
  * a logit: the 32-term fp16 MFMA dot product accumulated in fp32, <= 32 units of sum_d |q_d k_d|, and the multiply
    by scale, 1 unit of |s|: 33 units of Labs = scale * |q| . |k|, ABSOLUTE in the logit, hence RELATIVE in P;
  * __expf(t) = v_exp_f32(t * log2 e): the subtraction and the argument scaling cost 2 |t| units (t = s - m, or
    s * scale - lse), v_exp_f32 itself 1 ulp = 2 units.  So P carries 33 * Labs + 2 * |t| + 2 <= K_ARG * E + 2 with
    E = max Labs + max |t| of the case, K_ARG = 33.  (|t| > 24 means P < 2^-34: under the floor.)
  * forward: l adds 16 values per lane, two cross-lane adds and l * alpha + psum per tile: 18 + 2 * tiles; the PV
    MFMAs accumulate N products and one alpha multiply per tile: N + tiles; 1 / l and o * inv: 3.  alpha itself
    multiplies o and l alike and cancels.
  * backward: the lse the kernels are handed is off by up to K_LSE units of its own terms (below), relative in P;
    dP and D are 64-term fp32 sums, 64 units of A / P each; the dV / dK / dQ MFMAs accumulate N products: N + tiles;
    the final scale, the accumulate add and the rest: 8.
  lse (fp32): |got - ref| <= K_LSE * 2^-24 * (1 + |m| + |log l| + max_j Labs_ij), K_LSE = 64: the maximum logit carries
  33 units of Labs (the Labs term is added to the form 1 + |m| + |log l| because the dot product's rounding scales
  with sum |q_d k_d|, not with |m|); the sum l 18 + 2 * tiles <= 32 at N <= 400, the P entries 2 + 2 * sum_j P_ij |t_ij|
  <= 2 + 2 log N <= 14 (sum_j P_ij (m - s_ij) <= the entropy <= log N): 48 units of the constant 1; __logf =
  v_log_f32 * ln 2: 3 units of |log l|; the final add 1 unit of |m| + |log l|.

With an accumulate flag set the fp32 prior joins the reference before the single rounding, and its magnitude joins
terms_abs.
"""
import math

import torch

from elementwise_ref import F16_MAX, _unravel, bits, round16, ulp

KD, HD, HS, TILE = 32, 64, 128, 64
SCALE = 32 ** -0.5

LEAD = {"out": 2.0 ** -11, "dv": 2.0 ** -8, "dq": 3 * 2.0 ** -8, "dk": 3 * 2.0 ** -8}
K_ARG = 33
K_LSE = 64

GENERATORS = ("gauss", "peaked", "rising", "falling", "flat", "last_key")

# (B, heads, N): below one 16-lane group, a 64 tile minus / plus one, two tiles plus one, the PSA shape at 640 px;
# B > 1 with heads > 1 at the tails 17 and 65 and at N = 129
SHAPES = [(1, 1, 1), (2, 1, 15), (1, 2, 16), (2, 2, 17), (1, 3, 63), (3, 1, 64), (2, 2, 65), (3, 2, 129), (1, 2, 400)]
TAIL_SHAPES = [s for s in SHAPES if s[2] % 16]


def f32(x):
    """The fp32 value the C ABI receives for a Python float."""
    return float(torch.tensor(x, dtype=torch.float32))


def tiles(n):
    return (n + TILE - 1) // TILE


def k_fwd(n, e):
    return (n + tiles(n)) + (18 + 2 * tiles(n)) + 3 + 2 + K_ARG * e


def k_bwd(n, e, lse_terms_max):
    return (n + tiles(n)) + 64 + 8 + 2 + K_ARG * e + K_LSE * lse_terms_max


def split_heads(qkv, heads):
    """(B, N, heads * 128) -> q (B, heads, N, 32), k, v (B, heads, N, 64)."""
    B, N, _ = qkv.shape
    x = qkv.reshape(B, N, heads, HS).permute(0, 2, 1, 3)
    return x[..., :KD], x[..., KD:2 * KD], x[..., 2 * KD:]


def merge_heads(x):
    """(B, heads, N, d) -> (B, N, heads * d)."""
    B, H, N, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, N, H * d)


def pack_qkv(q, k, v):
    """Three (B, heads, N, d) tensors -> (B, N, heads * 128) in the kernels' channel order."""
    B, H, N, _ = q.shape
    return torch.cat([q, k, v], -1).permute(0, 2, 1, 3).reshape(B, N, H * HS)


def attn_ref(qkv16, heads, scale, dout_bf16=None, out16=None):
    """fp64 softmax(q k^T * scale) v per (image, head) and its gradients.  -> dict: out (B, N, heads * 64), lse, m, l
    (B, heads, N); with dout: dq, dk, dv packed as dqkv (B, N, heads * 128); terms[...] of the same shapes; E, the
    largest Labs + |s - m| of the case, lse_terms (B, heads, N).  D uses out16 when given (any dtype), else the
    unrounded out — the plain autograd result."""
    sc = f32(scale)
    q, k, v = (t.double() for t in split_heads(qkv16, heads))
    s = q @ k.transpose(-1, -2) * sc
    labs = q.abs() @ k.abs().transpose(-1, -2) * abs(sc)
    m = s.max(-1).values
    e = torch.exp(s - m[..., None])
    l = e.sum(-1)
    P = e / l[..., None]
    lse = m + torch.log(l)
    out = P @ v
    r = {"out": merge_heads(out), "lse": lse, "m": m, "l": l, "P": P,
         "E": float((labs + (s - m[..., None]).abs()).max()),
         "lse_terms": 1 + m.abs() + torch.log(l).abs() + labs.max(-1).values,
         "vmax": float(v.abs().max()),
         "terms": {"out": merge_heads(P @ v.abs())}}
    if dout_bf16 is None:
        return r
    B, N = qkv16.shape[:2]
    dO = dout_bf16.double().reshape(B, N, heads, HD).permute(0, 2, 1, 3)
    O = (r["out"] if out16 is None else out16.double()).reshape(B, N, heads, HD).permute(0, 2, 1, 3)
    D = (dO * O).sum(-1)
    dP = dO @ v.transpose(-1, -2)
    dS = P * (dP - D[..., None])
    A = P * (dO.abs() @ v.abs().transpose(-1, -2) + (dO * O).abs().sum(-1)[..., None])
    W = dS.abs() + A
    r["dqkv"] = pack_qkv(sc * dS @ k, sc * dS.transpose(-1, -2) @ q, P.transpose(-1, -2) @ dO)
    r["terms"]["dqkv"] = pack_qkv(abs(sc) * W @ k.abs(), abs(sc) * W.transpose(-1, -2) @ q.abs(),
                                  P.transpose(-1, -2) @ dO.abs())
    return r


def part(x, heads, which):
    """The q / k / v channels of a (..., heads * 128) tensor."""
    lo, hi = {"dq": (0, KD), "dk": (KD, 2 * KD), "dv": (2 * KD, HS)}[which]
    return x.reshape(*x.shape[:-1], heads, HS)[..., lo:hi]


# ------------------------------------------------------------------------------------------------ the checker
def excess(got16, ref64, terms64, kind, lead, K, floor=0.0):
    """-> (largest |err| / budget, NaN counted as inf; largest (|err| - half ulp - floor) / (lead * terms), the slack
    used in units of the leading constant; the flat index of the worst element)."""
    got, ref = got16.double(), ref64.double()
    if kind == "fp16":
        ref = ref.clamp(-F16_MAX, F16_MAX)
    terms = terms64.double().expand_as(ref)
    lead = torch.as_tensor(lead, dtype=torch.float64, device=ref.device)
    half = 0.5 * ulp(torch.maximum(got.abs(), ref.abs()).nan_to_num(nan=0.0, posinf=F16_MAX), kind)
    err = (got - ref).abs()
    budget = half + (lead + K * 2.0 ** -24) * terms + floor
    ratio = (err / budget).nan_to_num(nan=math.inf)
    unit = (lead * terms).expand_as(ref)
    used = torch.where(unit > 0, (err - half - floor) / unit, torch.zeros_like(err)).nan_to_num(nan=math.inf)
    if not ratio.numel():
        return 0.0, 0.0, 0
    i = int(ratio.reshape(-1).argmax())
    return float(ratio.reshape(-1)[i]), max(0.0, float(used.max())), i


def assert_attn_rounded(got16, ref64, terms64, kind, lead, K, floor=0.0, what=""):
    """Hold a 16-bit output to its fp64 reference under the budget of this file's docstring.  Returns the slack used,
    in units of lead * terms_abs (the budget in the same units is 1 + K * 2^-24 / lead)."""
    ratio, used, i = excess(got16, ref64, terms64, kind, lead, K, floor)
    if not ratio <= 1.0:
        idx = _unravel(i, tuple(ref64.shape))
        g, r, t = (float(x.double().reshape(-1)[i]) for x in (got16, ref64, terms64.expand_as(ref64)))
        raise AssertionError(
            f"{what}: worst at {idx}: got {g!r} (bits {int(bits(got16.reshape(-1)[i:i + 1])):#06x}) ref {r!r} (rounds to "
            f"bits {int(bits(round16(ref64.reshape(-1)[i:i + 1].double(), kind))):#06x}) |err| {abs(g - r):.6g} is "
            f"{ratio:.3g} x the budget (terms {t:.6g}, K {K:.1f}, floor {floor:.3g})")
    return used


def lse_excess(got32, ref):
    """-> largest |got - ref| / (2^-24 * lse_terms) of the fp32 LSE rows: K_LSE is the budget."""
    err = (got32.double() - ref["lse"]).abs()
    return float((err / (2.0 ** -24 * ref["lse_terms"])).nan_to_num(nan=math.inf).max())


def assert_lse(got32, ref, what=""):
    used = lse_excess(got32, ref)
    assert used <= K_LSE, f"{what}: lse off by {used:.3g} units of 2^-24 * (1 + |m| + |log l| + Labs), budget {K_LSE}"
    return used


def check_forward(out16, lse32, ref, n, what="", K=None):
    """out and lse of one forward under their budgets.  -> (slack of out in units of 2^-11 * T_out, lse units)."""
    K = k_fwd(n, ref["E"]) if K is None else K
    u = assert_attn_rounded(out16, ref["out"], ref["terms"]["out"], "fp16", LEAD["out"], K,
                            floor=n * 2.0 ** -25 * ref["vmax"], what=what + " out")
    return u, assert_lse(lse32, ref, what)


def check_backward(dqkv16, ref, heads, n, prior=None, acc=(0, 0, 0), what="", K=None):
    """dq / dk / dv of one backward.  prior (B, N, heads * 128) bf16 joins the reference on the slices whose flag is
    set.  -> {"dq": slack, "dk": slack, "dv": slack} in units of the slice's leading constant times its terms."""
    K = k_bwd(n, ref["E"], float(ref["lse_terms"].max())) if K is None else K
    want, terms = ref["dqkv"], ref["terms"]["dqkv"]
    if prior is not None and any(acc):
        flag = torch.cat([torch.full((KD,), float(acc[0])), torch.full((KD,), float(acc[1])),
                          torch.full((HD,), float(acc[2]))]).repeat(heads).double().to(want.device)
        want = want + flag * prior.double().nan_to_num(nan=0.0)
        terms = terms + flag * prior.double().nan_to_num(nan=0.0).abs()
        K = K + 1
    used = {}
    for w in ("dq", "dk", "dv"):
        used[w] = assert_attn_rounded(part(dqkv16, heads, w), part(want, heads, w), part(terms, heads, w), "bf16",
                                      LEAD[w], K, what=f"{what} {w}")
    return used


# ------------------------------------------------------------------------------------------------ generated inputs
def make_inputs(gen, B, heads, N, seed=0, scale=SCALE):
    """-> (qkv fp16 (B, N, heads * 128), dout bf16 (B, N, heads * 64)), seeded.
    gauss     q, k, v ~ N(0, 1): logits of standard deviation ~1
    peaked    q, k x 3: near one-hot rows, |logit| up to ~50
    rising    logits ~ c_i * 8 * (j + 1) / N + noise, c_i in [0.5, 1.5]: the running maximum moves in every tile
    falling   its mirror in the key index: the maximum is met in the first tile, every later alpha is 1
    flat      q = 0: P = 1 / N exactly
    last_key  the row maximum planted at key N - 1"""
    g = torch.Generator().manual_seed(7919 * GENERATORS.index(gen) + 1000 * B + 100 * heads + N + seed)
    q = torch.randn(B, heads, N, KD, generator=g)
    k = torch.randn(B, heads, N, KD, generator=g)
    v = torch.randn(B, heads, N, HD, generator=g)
    dout = torch.randn(B, N, heads * HD, generator=g).bfloat16()
    if gen == "peaked":
        q, k = 3 * q, 3 * k
    elif gen in ("rising", "falling"):
        c = 0.5 + torch.rand(B, heads, N, 1, generator=g)
        ramp = (torch.arange(N, dtype=torch.float32) + 1) / N
        if gen == "falling":
            ramp = ramp.flip(0)
        q, k = 0.1 * q, 0.1 * k
        q[..., 0:1] = c * 4
        k[..., 0] = ramp * 2 / scale
    elif gen == "flat":
        q = torch.zeros_like(q)
    elif gen == "last_key":
        q[..., 0] = 3.0
        k[..., 0] *= 0.3
        k[..., N - 1, 0] = 16.0
    return pack_qkv(q, k, v).half(), dout


def make_prior(B, heads, N, seed=0):
    g = torch.Generator().manual_seed(31 * N + heads + seed)
    return torch.randn(B, N, heads * HS, generator=g).bfloat16()


# ------------------------------------------------------------------------------------------------ the emulation
MUTATIONS = ("pad_zero_key", "drop_last_key", "no_alpha", "lse_no_max", "dk_unscaled", "dq_scaled_twice", "swap_qk",
             "head_xor", "d_other_head", "acc_cross", "acc_ignores_flag", "last_row_unwritten", "gap_ignored")


def _rows(buf, b, N, gap, mutate):
    """Image b's N rows of a (B * (N + gap), C) buffer; the gap_ignored mutant strides by N rows."""
    r0 = b * (N if mutate == "gap_ignored" else N + gap)
    return buf[r0:r0 + N]


def emulate(qkv16, heads, scale, dout_bf16=None, out16=None, lse32=None, prior=None, acc=(0, 0, 0), mutate=None,
            gap=0, gap_fill=None):
    """The kernels' order of operations in torch fp32 (exp and log correctly rounded): 64-key tiles with the running
    maximum, alpha and l in fp32, P rounded to fp16 before PV; in the backward P = exp(s * scale - lse) and dS rounded
    to bf16, q / k / v operands rounded to bf16, one rounding at the store (after the prior when the flag is set).
    The backward's accumulators are summed in one fp32 matmul, not tile by tile: nothing is rescaled between its
    tiles.  Without out16 / lse32 the backward runs on the forward's own.

    `gap` rows (filled from gap_fill (B, gap, C), as a view with a batch stride > N * ld holds other data there)
    follow every image of the qkv buffer.  `mutate` names one planted fault (MUTATIONS).
    -> dict: out fp16 (B, N, heads * 64), lse fp32 (B, heads, N), dqkv bf16 (B, N, heads * 128) or None."""
    assert mutate is None or mutate in MUTATIONS
    B, N, C = qkv16.shape
    sc = torch.tensor(scale, dtype=torch.float32)
    if gap:
        buf = torch.cat([qkv16, gap_fill.to(qkv16.dtype)], 1).reshape(B * (N + gap), C)
    else:
        buf = qkv16.reshape(B * N, C)
    out = torch.zeros(B, N, heads * HD, dtype=torch.float16)
    lse = torch.zeros(B, heads, N, dtype=torch.float32)
    for b in range(B):
        x = _rows(buf, b, N, gap, mutate)
        for h in range(heads):
            q, k, v = x[:, h * HS:h * HS + KD], x[:, h * HS + KD:h * HS + 2 * KD], x[:, h * HS + 2 * KD:(h + 1) * HS]
            if mutate == "swap_qk":
                q, k = k, q
            S = (q.float() @ k.float().T) * sc
            m = torch.full((N,), -math.inf)
            l = torch.zeros(N)
            o = torch.zeros(N, HD)
            for k0 in range(0, N, TILE):
                k1 = min(k0 + TILE, N)
                s, vt = S[:, k0:k1], v[k0:k1].float()
                if k1 == N:
                    if mutate == "drop_last_key":
                        s, vt = s[:, :-1], vt[:-1]
                    elif mutate == "pad_zero_key" and N % TILE:       # the zero-filled LDS row of key N, unmasked
                        s, vt = torch.cat([s, torch.zeros(N, 1)], 1), torch.cat([vt, torch.zeros(1, HD)], 0)
                mn = torch.maximum(m, s.max(1).values) if s.shape[1] else m
                alpha = torch.exp(m - mn)
                p = torch.exp(s - mn[:, None])
                l = l * alpha + p.sum(1)
                if mutate != "no_alpha":
                    o = o * alpha[:, None]
                o = o + p.half().float() @ vt
                m = mn
            ho = h ^ 1 if mutate == "head_xor" and (h ^ 1) < heads else h
            out[b, :, ho * HD:(ho + 1) * HD] = (o * (1.0 / l)[:, None]).half()
            lse[b, h] = torch.log(l) if mutate == "lse_no_max" else m + torch.log(l)
    r = {"out": out, "lse": lse, "dqkv": None}
    if dout_bf16 is None:
        return r
    out16 = out if out16 is None else out16
    lse32 = lse if lse32 is None else lse32
    if mutate == "acc_cross":
        acc = (acc[0], acc[2], acc[1])
    elif mutate == "acc_ignores_flag":
        acc = (1, 1, 1)
    dqkv = torch.zeros(B, N, C, dtype=torch.bfloat16)
    old = torch.zeros(B, N, C) if prior is None else prior.float().nan_to_num(nan=0.0)
    for b in range(B):
        x = _rows(buf, b, N, gap, mutate)
        for h in range(heads):
            q, k, v = x[:, h * HS:h * HS + KD], x[:, h * HS + KD:h * HS + 2 * KD], x[:, h * HS + 2 * KD:(h + 1) * HS]
            if mutate == "swap_qk":
                q, k = k, q
            dO = dout_bf16[b, :, h * HD:(h + 1) * HD].float()
            hd = h ^ 1 if mutate == "d_other_head" and (h ^ 1) < heads else h
            D = (dO * out16[b, :, hd * HD:(hd + 1) * HD].float()).sum(1)
            P = torch.exp((q.float() @ k.float().T) * sc - lse32[b, h][:, None])
            dS = (P * (dO @ v.bfloat16().float().T - D[:, None])).bfloat16().float()
            dq = (dS @ k.bfloat16().float()) * sc
            dk = (dS.T @ q.bfloat16().float()) * sc
            dv = P.bfloat16().float().T @ dO
            if mutate == "dk_unscaled":
                dk = dS.T @ q.bfloat16().float()
            elif mutate == "dq_scaled_twice":
                dq = dq * sc
            c0 = h * HS
            for val, lo, hi, flag in ((dq, 0, KD, acc[0]), (dk, KD, 2 * KD, acc[1]), (dv, 2 * KD, HS, acc[2])):
                if flag:
                    val = val + old[b, :, c0 + lo:c0 + hi]
                dqkv[b, :, c0 + lo:c0 + hi] = val.bfloat16()
    if mutate == "last_row_unwritten":
        dqkv[:, N - 1] = 0
    r["dqkv"] = dqkv
    return r
