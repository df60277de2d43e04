"""The streaming elementwise kernels on their own, at the C ABI, against fp64 references rounded once
(tests/elementwise_ref.py): ym_bn_apply, ym_bn_bwd_apply[_res], ym_dw3x3_fwd / _bwd and ym_bn_eval_coeff under the
half-ulp + K * 2^-24 * terms budget (K = 32, derived in elementwise_ref.py), the view conversions, ym_copy2d and
ym_head_grad's dz rows bit-exact.

Every output buffer is one row longer at each end and as wide as its view's `ld`, prefilled with a sentinel bit
pattern (0x7BAD fp16 / 0xBAAD bf16 / a payload NaN fp32) and with NaN where the kernel has to write: afterwards
everything outside the addressed channels and rows must be bit-identical, and no NaN may be left inside.

The shapes are the ones at which the kernels' index arithmetic changes (bn.hip lanes(): rows = 256 // (C / 8), an
idle thread when C / 8 does not divide 256; the grid cap of 2048 blocks and the BN_ROWS row pair, whose partner
row falls past M in the second grid-stride pass; ch_pieces of the depthwise kernels; head_grad's G groups x S
slots), not the networks' shapes — tests/test_gpu_layers.py covers those.

The largest fp32 slack each kernel used is collected per kernel and mode; with YM_ELEMENTWISE_SLACK_OUT=<path>
the table is written there (profiles/elementwise/slack.txt is such a run).
"""
import os

import pytest
import torch

import elementwise_ref as ER

pytestmark = pytest.mark.gpu

_INT = {"fp16": torch.int16, "bf16": torch.int16, "f32": torch.int32, "u8": torch.uint8}
_DT = {"fp16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "u8": torch.uint8}
_PAD = {"fp16": ER.PAD_BITS["fp16"], "bf16": ER.PAD_BITS["bf16"] - 65536, "f32": ER.F32_PAD_BITS, "u8": 0xAD}
_NAN = {"fp16": ER.NAN_BITS["fp16"], "bf16": ER.NAN_BITS["bf16"], "f32": 0x7FC00000, "u8": 0x5A}
_SIZE = {"fp16": 2, "bf16": 2, "f32": 4, "u8": 1}

SLACK = {}


def _dev():
    return torch.device("cuda", 0)


def _record(name, used):
    SLACK[name] = max(SLACK.get(name, 0.0), used)


@pytest.fixture(scope="module", autouse=True)
def _slack_table():
    yield
    lines = [f"{k:<44s} {v:8.3f}" for k, v in sorted(SLACK.items())]
    print("\nfp32 slack used, in units of 2^-24 * terms_abs (budget K = %d):\n" % ER.K_FP32 + "\n".join(lines))
    path = os.environ.get("YM_ELEMENTWISE_SLACK_OUT")
    if path and lines:
        with open(path, "w") as f:
            f.write("# largest (|got - ref| - 0.5 ulp16) / (2^-24 * terms_abs) over tests/test_gpu_elementwise.py, per kernel and\n"
                    "# mode; the budget is K = %d (tests/elementwise_ref.py)\n" % ER.K_FP32 + "\n".join(lines) + "\n")


class Guarded:
    """A buffer around a (rows, cols) view: sentinel everywhere, NaN (or `data`) in the view.  One guard row at each
    end, `ld` columns wide; with n images and `gap`, `gap` more sentinel rows after every image's rows // n rows, so
    that the view's batch stride `bs` exceeds hw * ld."""

    def __init__(self, rows, ld, kind, c=None, off=0, cols=None, data=None, n=1, gap=0):
        self.kind, self.rows, self.ld = kind, rows, ld
        self.cols = torch.arange(off, off + (ld if c is None else c)) if cols is None else cols
        self.cols = self.cols.to(_dev())
        self.off = int(self.cols[0]) if len(self.cols) else 0
        hw = max(rows // n, 1)
        self.bs = (hw + gap) * ld
        r = torch.arange(rows, device=_dev())
        self.ridx = (1 + r + (r // hw) * gap)[:, None]
        self.raw = torch.full((rows + n * gap + 2, ld), _PAD[kind], dtype=_INT[kind], device=_dev())
        if data is None:
            self.raw[self.ridx, self.cols] = _NAN[kind]
        else:
            self.raw[self.ridx, self.cols] = data.to(_dev()).contiguous().view(_INT[kind]).reshape(rows, -1)
        self.before = None

    @property
    def ptr(self):
        """Address of the view's first element (row 0, first addressed column)."""
        return self.raw.data_ptr() + (self.ld + self.off) * _SIZE[self.kind]

    def inner(self):
        return self.raw[self.ridx, self.cols].contiguous().view(_DT[self.kind])

    def snapshot(self):
        self.before = self.raw.clone()
        return self

    def check_untouched(self, what=""):
        """Everything outside the view still holds the sentinel; with a snapshot, the whole buffer is unchanged."""
        if self.before is not None:
            assert torch.equal(self.raw, self.before), f"{what}: buffer written"
            return
        mask = torch.ones_like(self.raw, dtype=torch.bool)
        mask[self.ridx, self.cols] = False
        bad = mask & (self.raw != _PAD[self.kind])
        if bool(bad.any()):
            at = bad.nonzero()[0].tolist()
            raise AssertionError(f"{what}: {int(bad.sum())} sentinel elements outside the view overwritten, first at "
                                 f"buffer row {at[0] - 1} column {at[1]} ({self.rows} view rows, columns "
                                 f"{self.off}..{int(self.cols[-1]) if len(self.cols) else 0})")


def _abi():
    from yolomi._lib import call, lib, stream_ptr
    return call, lib, stream_ptr(_dev())


def _to_dev(d):
    return {k: (v.to(_dev()) if torch.is_tensor(v) else v) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------ ym_bn_apply
@pytest.mark.parametrize("c,m", ER.BN_SHAPES)
def test_bn_apply(c, m):
    """act x residual view (r_ld = c + 8) x fp32 copy, into an output view of o_ld = c + 16 at channel offset 8.
    fp16 result within half an fp16 ulp + 32 * 2^-24 * (|z * scale| + |shift| + |res|) of fp64; the planted rows hold
    t = 0, +-24, -15 (SiLU an fp16 subnormal: stored, not flushed) and 7e4 (stored as 65504, not inf).  The fp32
    copy is the value before the rounding: same fp32 budget, and the fp16 bits are exactly its clamped RNE."""
    call, lib, st = _abi()
    d = _to_dev(ER.make_bn_inputs(c, m))
    res = Guarded(m, c + 8, "fp16", c=c, off=0, data=d["res"]).snapshot()
    z = d["z"].contiguous()
    for act in (0, 1):
        for use_res in (False, True):
            ref, terms = ER.bn_apply_ref(z, d["scale"], d["shift"], act, d["res"] if use_res else None)
            for use32 in (False, True):
                what = f"ym_bn_apply C={c} m={m} act={act} res={use_res} out32={use32}"
                out = Guarded(m, c + 16, "fp16", c=c, off=8)
                o32 = Guarded(m, c, "f32") if use32 else None
                call("ym_bn_apply", z.data_ptr(), m, c, m, d["scale"].data_ptr(), d["shift"].data_ptr(), act,
                     res.ptr if use_res else None, m * (c + 8), c + 8, out.ptr, m * (c + 16), c + 16,
                     o32.ptr if use32 else None, st)
                torch.cuda.synchronize()
                got = out.inner()
                _record(f"ym_bn_apply act={act}", ER.assert_rounded(got, ref, terms, "fp16", what=what))
                out.check_untouched(what)
                res.check_untouched(what + " (residual)")
                if use32:
                    v = o32.inner()
                    _record(f"ym_bn_apply act={act} (fp32 copy)", ER.assert_f32_close(v, ref, terms, what=what + " fp32"))
                    o32.check_untouched(what + " fp32")
                    ER.assert_bits_equal(got, v.clamp(-ER.F16_MAX, ER.F16_MAX).half(), what + ": fp16 != RNE(fp32 copy)")
    if m >= 8:          # the planted rows came out as planted
        y = ER.bn_apply_ref(z, d["scale"], d["shift"], 1)[0]
        assert float(y.max()) > ER.F16_MAX and bool(((y.abs() > 2.0 ** -24) & (y.abs() < 2.0 ** -14)).any())


def test_bn_apply_m0_writes_nothing():
    call, lib, st = _abi()
    c = 24
    d = _to_dev(ER.make_bn_inputs(c, 8))
    out, o32 = Guarded(4, c + 16, "fp16", c=c, off=8).snapshot(), Guarded(4, c, "f32").snapshot()
    assert lib().ym_bn_apply(d["z"].data_ptr(), 0, c, 1, d["scale"].data_ptr(), d["shift"].data_ptr(), 1, None, 0, 0,
                             out.ptr, c + 16, c + 16, o32.ptr, st) == 0
    torch.cuda.synchronize()
    out.check_untouched("m = 0")
    o32.check_untouched("m = 0 fp32")


# ------------------------------------------------------------------------------------------------ ym_bn_bwd_apply[_res]
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("c,m", ER.BN_BWD_SHAPES)
def test_bn_bwd_apply(c, m, act):
    """dy as a channel slice (d_ld = c + 64, offset 8).  dz (bf16) within half a bf16 ulp + 32 * 2^-24 *
    |k1| (|g| + |k2| + |xh * k3|) of fp64; dz written over z in place gives the same bits; the _res form gives the same
    dz bits and dres = dy / RNE(dres + dy) bit for bit in a view of r_ld = c + 24 (rounding ties and +-0 in the last
    row, make_bn_bwd_inputs).  Measured slack (profiles/elementwise/slack.txt): 1.7 units without SiLU, up to 16.7
    with it — at t = -1.26, next to the zero of SiLU's derivative, where dsilu()'s 1 + u * (1 - sg) cancels and
    terms_abs counts only the small result.  The correctly rounded fp32 restatement uses the same 16.7 on that
    input (test_elementwise_ref_cpu.py): it is the cancellation, not v_rcp_f32 or __expf.  terms_abs can get
    arbitrarily small next to t = -1.2785, so K = 32 holds for these seeded inputs, not for every input."""
    call, lib, st = _abi()
    d = _to_dev(ER.make_bn_bwd_inputs(c, m))
    what = f"ym_bn_bwd_apply C={c} m={m} act={act}"
    dy = Guarded(m, c + 64, "bf16", c=c, off=8, data=d["dy"]).snapshot()
    z = d["z"].contiguous()
    vec = [d[k].contiguous() for k in ("scale", "shift", "mean", "rstd")]
    coef = d["coef"].contiguous()

    def args(zp):
        return (dy.ptr, m * (c + 64), c + 64, zp, m, c, m, *[v.data_ptr() for v in vec], act, coef.data_ptr())
    ref, terms = ER.bn_bwd_apply_ref(d["dy"], z, *vec, coef, act)
    dz = Guarded(m, c, "bf16")
    call("ym_bn_bwd_apply", *args(z.data_ptr()), dz.ptr, st)
    torch.cuda.synchronize()
    fresh = dz.inner()
    used = ER.assert_rounded(fresh, ref, terms, "bf16", what=what)
    _record(f"ym_bn_bwd_apply act={act}", used)
    i = ER.worst_slack_index(fresh, ref, terms, "bf16")
    t = (z.double() * vec[0].double() + vec[1].double()).reshape(-1)[i]
    print(f"{what}: slack {used:.2f} at flat index {i}, t = {float(t):.4f}")
    dz.check_untouched(what)
    # in place: dz over z
    zz = Guarded(m, c, "fp16", data=z)
    call("ym_bn_bwd_apply", *args(zz.ptr), zz.ptr, st)
    torch.cuda.synchronize()
    ER.assert_bits_equal(zz.inner().view(torch.bfloat16), fresh, what + " in place")
    zz.check_untouched(what + " in place")
    # the shortcut gradient from the same dy read
    for acc in (0, 1):
        dz2 = Guarded(m, c, "bf16")
        dres = Guarded(m, c + 24, "bf16", c=c, off=16, data=d["dres"] if acc else None)
        want = ER.add16(d["dres"], d["dy"]) if acc else d["dy"]
        call("ym_bn_bwd_apply_res", *args(z.data_ptr()), dz2.ptr, dres.ptr, m * (c + 24), c + 24, acc, st)
        torch.cuda.synchronize()
        ER.assert_bits_equal(dz2.inner(), fresh, what + f" _res acc={acc}: dz")
        ER.assert_bits_equal(dres.inner(), want, what + f" _res acc={acc}: dres")
        dz2.check_untouched(what + " _res dz")
        dres.check_untouched(what + " _res dres")
    dy.check_untouched(what + " (dy)")
    assert torch.equal(z, d["z"])


# ------------------------------------------------------------------------------------------------ view ops
VIEW_SHAPES = [(1, 1, 8), (3, 7, 24), (2, 400, 136), (3, 100000, 64)]      # the last: m * c / 8 > 8192 * 256


def _tie_data(m, c, kind, seed):
    """(a, b) 16-bit tensors (m, c): randn, with the first elements of every row built so that a + b is a rounding
    tie of the format (an integer with a full mantissa + 0.5), both ways round, and the +-0 sums."""
    g = torch.Generator().manual_seed(seed)
    dt = _DT[kind]
    a, b = torch.randn(m, c, generator=g), torch.randn(m, c, generator=g)
    lo = 1024 if kind == "fp16" else 128
    k = torch.randint(lo, 2 * lo, (m, 4), generator=g).float()
    a[:, :4] = k * torch.tensor([1.0, -1.0, 1.0, -1.0])
    b[:, :4] = torch.tensor([0.5, -0.5, -0.5, 0.5])
    a[:, 4:8] = torch.tensor([0.0, -0.0, 0.0, -0.0])
    b[:, 4:8] = torch.tensor([0.0, -0.0, -0.0, 0.0])
    return a.to(dt), b.to(dt)


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("n,hw,c", VIEW_SHAPES)
def test_view_axpy(n, hw, c, half):
    """Zero fill (src NULL), copy and accumulate between views of different strides and channel offsets, bit for
    bit: the accumulate is RNE(fp32(a) + fp32(b)) of the 16-bit operands.  Both batch strides exceed hw * ld (one /
    two sentinel rows between the images), so the kernels' n = m / hw, pix = m - n * hw split is pinned."""
    call, lib, st = _abi()
    kind = "fp16" if half else "bf16"
    m = n * hw
    a, b = _tie_data(m, c, kind, 11 * c + half)
    a, b = a.to(_dev()), b.to(_dev())
    x_ld, y_ld = c + 8, c + 24
    x = Guarded(m, x_ld, kind, c=c, off=8, data=a, n=n, gap=1).snapshot()
    for mode in ("zero", "copy", "acc"):
        what = f"ym_view_axpy {mode} n={n} hw={hw} c={c} half={half}"
        y = Guarded(m, y_ld, kind, c=c, off=16, data=b if mode == "acc" else None, n=n, gap=2)
        call("ym_view_axpy", None if mode == "zero" else x.ptr, x.bs, x_ld, y.ptr, y.bs, y_ld, m, c, hw,
             1 if mode == "acc" else 0, half, st)
        torch.cuda.synchronize()
        want = {"zero": torch.zeros_like(a), "copy": a, "acc": ER.add16(a, b)}[mode]
        ER.assert_bits_equal(y.inner(), want, what)
        y.check_untouched(what)
    x.check_untouched("ym_view_axpy (source)")


@pytest.mark.parametrize("n,hw,c", VIEW_SHAPES)
def test_view_to_f32_and_back(n, hw, c):
    call, lib, st = _abi()
    m = n * hw
    a, b = _tie_data(m, c, "bf16", 13 * c)
    a, b = a.to(_dev()), b.to(_dev())
    ld = c + 8
    what = f"n={n} hw={hw} c={c}"
    x = Guarded(m, ld, "bf16", c=c, off=8, data=a, n=n, gap=1).snapshot()       # bs > hw * ld
    y = Guarded(m, c, "f32")
    call("ym_view_to_f32", x.ptr, x.bs, ld, y.ptr, m, c, hw, st)
    torch.cuda.synchronize()
    assert torch.equal(y.inner().view(torch.int32), a.float().view(torch.int32)), "ym_view_to_f32 " + what
    y.check_untouched("ym_view_to_f32 " + what)
    x.check_untouched("ym_view_to_f32 (source) " + what)
    # fp32 values that are bf16 ties (a + b is exact in fp32 for the planted columns), then the accumulate
    f = (a.float() + b.float()).contiguous()
    for acc in (0, 1):
        v = Guarded(m, ld, "bf16", c=c, off=0, data=b if acc else None, n=n, gap=2)
        call("ym_f32_to_view", f.data_ptr(), v.ptr, v.bs, ld, m, c, hw, acc, st)
        torch.cuda.synchronize()
        want = (f + b.float()).bfloat16() if acc else f.bfloat16()
        ER.assert_bits_equal(v.inner(), want, f"ym_f32_to_view acc={acc} " + what)
        v.check_untouched(f"ym_f32_to_view acc={acc} " + what)


@pytest.mark.parametrize("width,dpitch,spitch,rows", [(24, 40, 32, 7), (64, 64, 64, 5), (24, 40, 32, 0), (0, 40, 32, 7),
                                                      (13, 17, 19, 9)])
def test_copy2d(width, dpitch, spitch, rows):
    call, lib, st = _abi()
    nr = max(rows, 1)
    g = torch.Generator().manual_seed(width + rows)
    src = torch.randint(0, 256, (nr, spitch), generator=g, dtype=torch.uint8).to(_dev())
    dst = Guarded(nr, dpitch, "u8", c=width, off=0)
    if rows == 0 or width == 0:
        dst.snapshot()
    call("ym_copy2d", dst.ptr, dpitch, src.data_ptr(), spitch, width, rows, st)
    torch.cuda.synchronize()
    if rows and width:
        assert torch.equal(dst.inner(), src[:, :width])
    dst.check_untouched(f"ym_copy2d width={width} rows={rows}")


# ------------------------------------------------------------------------------------------------ ym_head_grad
# (nc, n, hw): G = 8 + ncp / 8 channel groups, S = 256 // G pixel slots; hw no multiple of S; nc = 1 at m > 512 * S
@pytest.mark.parametrize("nc,n,hw", [(1, 2, 37), (1, 3, 6400), (8, 2, 45), (9, 2, 33), (80, 2, 45), (1024, 2, 5)])
def test_head_grad(nc, n, hw):
    """dz_box / dz_cls the RNE bf16 of the fp32 rows bit for bit (ties and +-0 planted), the padded class columns
    +0, the level at a_off > 0 inside a_total > hw; the bias gradients ADDED to what the vectors held (twice over two
    calls), against fp64 column sums by the rule for reordered fp32 sums; NULL bias vectors accepted."""
    call, lib, st = _abi()
    ncp = (nc + 7) // 8 * 8
    G = 8 + ncp // 8
    S = 256 // G
    m = n * hw
    assert hw % S != 0 or S == 1
    a_off, A = 6, hw + 13
    g = torch.Generator().manual_seed(nc + hw)
    dh = torch.randn(n, A, 64 + nc, generator=g)
    # bf16 rounding ties 1 + (2 j + 1) * 2^-8 of either sign (box columns 3 and 5, the first class column), +-0
    tie = lambda: (1 + (2 * torch.randint(0, 64, (n, A), generator=g).float() + 1) * 2.0 ** -8) * \
        (2 * torch.randint(0, 2, (n, A), generator=g).float() - 1)
    dh[:, :, 3], dh[:, :, 5], dh[:, :, 64] = tie(), tie(), tie()
    dh[:, :, 7], dh[:, :, 9] = 0.0, -0.0
    dh = dh.to(_dev())
    box_w, cls_w, sb, scl = ER.head_grad_ref(dh, a_off, hw, nc)
    ws = torch.empty(lib().ym_head_grad_workspace_size() // 4, device=_dev())
    pre_b = torch.randn(64, generator=g).to(_dev())
    pre_c = torch.randn(nc, generator=g).to(_dev())
    db = Guarded(1, 64 + 8, "f32", c=64, off=0, data=pre_b.view(1, 64))
    dc = Guarded(1, nc + 8, "f32", c=nc, off=0, data=pre_c.view(1, nc))
    what = f"ym_head_grad nc={nc} n={n} hw={hw}"
    for rep in (1, 2):
        box, cls = Guarded(m, 64, "bf16"), Guarded(m, ncp, "bf16")
        call("ym_head_grad", dh.data_ptr(), A, a_off, hw, m, nc, box.ptr, cls.ptr, db.ptr, dc.ptr, ws.data_ptr(),
             ws.numel() * 4, st)
        torch.cuda.synchronize()
        ER.assert_bits_equal(box.inner(), box_w, what + " dz_box")
        ER.assert_bits_equal(cls.inner(), cls_w, what + " dz_cls")
        box.check_untouched(what + " dz_box")
        cls.check_untouched(what + " dz_cls")
        eb = ER.sum_rule_err(db.inner().view(-1), pre_b.double() + rep * sb)
        ec = ER.sum_rule_err(dc.inner().view(-1), pre_c.double() + rep * scl)
        print(f"{what} call {rep}: dbias_box err {eb:.3g} dbias_cls err {ec:.3g}")
        assert eb < 1e-4 and ec < 1e-4, (eb, ec)
        db.check_untouched(what + " dbias_box")
        dc.check_untouched(what + " dbias_cls")
    box, cls = Guarded(m, 64, "bf16"), Guarded(m, ncp, "bf16")
    call("ym_head_grad", dh.data_ptr(), A, a_off, hw, m, nc, box.ptr, cls.ptr, None, None, ws.data_ptr(),
         ws.numel() * 4, st)
    torch.cuda.synchronize()
    ER.assert_bits_equal(box.inner(), box_w, what + " dz_box (no bias)")
    ER.assert_bits_equal(cls.inner(), cls_w, what + " dz_cls (no bias)")


# ------------------------------------------------------------------------------------------------ ym_dw3x3_fwd / _bwd
@pytest.mark.parametrize("blocks", [1, 64])
@pytest.mark.parametrize("shape", ER.DW_SHAPES)
def test_dw3x3_fwd(shape, blocks):
    """z (fp16, dense) within half an fp16 ulp + 32 * 2^-24 * sum |w * x| of the fp64 depthwise conv over the mapped
    source channels, and the `blocks` statistics rows, summed, by the rule for reordered fp32 sums.

    The kernel sums the statistics from its fp32 results BEFORE the fp16 store (as the conv epilogues do), so they
    differ from the sums of the stored z by that rounding: up to 2^-11 relative on a single pixel, 4.3e-4 / 2.4e-4
    (sum / squares) by the rule on the 2x5x3 map with generic inputs — above 1e-4 with nothing wrong.  The comparison
    with the fp64 sums of the kernel's own fp16 output therefore runs on inputs whose results are exact in fp16
    (make_dw_inputs grid=True; z is then also held bit for bit), and on the generic inputs the statistics are held
    to the fp64 sums of the unrounded reference instead."""
    call, lib, st = _abi()
    n, h, w, c, gsz, gstride, goff = shape
    for grid in (False, True):
        d = _to_dev(ER.make_dw_inputs(*shape, grid=grid))
        ld, M = d["ld"], n * h * w
        what = f"ym_dw3x3_fwd {shape} blocks={blocks} grid={grid}"
        x = Guarded(M, ld, "fp16", data=d["x"].reshape(M, ld), n=n, gap=1).snapshot()      # x_bs > h * w * ld
        wt = d["w"].contiguous()
        z = Guarded(M, c, "fp16")
        ssum, ssq = Guarded(blocks, c, "f32"), Guarded(blocks, c, "f32")
        call("ym_dw3x3_fwd", x.ptr, x.bs, ld, gsz, gstride, goff, wt.data_ptr(), z.ptr, ssum.ptr, ssq.ptr, n, h,
             w, c, blocks, st)
        torch.cuda.synchronize()
        ref, terms = ER.dw3x3_ref(d["x"], wt, c, gsz, gstride, goff)
        ref, terms = ref.reshape(M, c), terms.reshape(M, c)
        got = z.inner()
        for b in (z, ssum, ssq, x):
            b.check_untouched(what)
        if grid:
            ER.assert_bits_equal(got, ER.round16(ref, "fp16"), what)
            assert torch.equal(got.double(), ref)
            base = got.double()                  # the kernel's own fp16 output
        else:
            _record("ym_dw3x3_fwd", ER.assert_rounded(got, ref, terms, "fp16", what=what))
            base = ref                           # what the kernel sums, before its rounding
        es = ER.sum_rule_err(ssum.inner().double().sum(0), base.sum(0))
        eq = ER.sum_rule_err(ssq.inner().double().sum(0), (base ** 2).sum(0))
        print(f"{what}: sum err {es:.3g} sq err {eq:.3g}")
        assert es < 1e-4 and eq < 1e-4, (es, eq)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", ER.DW_SHAPES)
def test_dw3x3_bwd(shape, accumulate):
    """dx (bf16) into the mapped channels of a view, written or accumulated, within half a bf16 ulp + 32 * 2^-24 *
    (sum |w * dz| + |dx_old|) of fp64, every other channel of the view untouched; dw ADDED to what the tensor held
    whatever `accumulate` says."""
    call, lib, st = _abi()
    n, h, w, c, gsz, gstride, goff = shape
    d = _to_dev(ER.make_dw_inputs(*shape))
    ld, M = d["ld"], n * h * w
    what = f"ym_dw3x3_bwd {shape} accumulate={accumulate}"
    src = ER.dw_src_channels(c, gsz, gstride, goff)
    x = Guarded(M, ld, "fp16", data=d["x"].reshape(M, ld), n=n, gap=1).snapshot()      # x_bs > h * w * ld
    dz = Guarded(M, c, "bf16", data=d["dz"].reshape(M, c)).snapshot()
    wt = d["w"].contiguous()
    g = torch.Generator().manual_seed(c + accumulate)
    old = torch.randn(M, c, generator=g).bfloat16().to(_dev())
    dx_ld = ld + 8
    dx = Guarded(M, dx_ld, "bf16", cols=src, data=old if accumulate else None, n=n, gap=2)
    pre = torch.randn(c, 9, generator=g).to(_dev())
    dw = Guarded(1, c * 9 + 8, "f32", c=c * 9, off=0, data=pre.view(1, -1))
    ws = torch.empty(max(lib().ym_dw3x3_bwd_workspace_size(c) // 4, 1), device=_dev())
    # the dx view starts at channel 0: the kernel adds the source channel itself
    call("ym_dw3x3_bwd", x.ptr, x.bs, ld, gsz, gstride, goff, wt.data_ptr(), dz.ptr,
         dx.raw.data_ptr() + dx_ld * 2, dx.bs, dx_ld, dw.ptr, n, h, w, c, accumulate, ws.data_ptr(),
         ws.numel() * 4, st)
    torch.cuda.synchronize()
    rdx, terms, rdw = ER.dw3x3_bwd_ref(d["x"], wt, d["dz"], c, gsz, gstride, goff)
    rdx, terms = rdx.reshape(M, c), terms.reshape(M, c)
    if accumulate:
        rdx, terms = rdx + old.double(), terms + old.double().abs()
    _record("ym_dw3x3_bwd dx", ER.assert_rounded(dx.inner(), rdx, terms, "bf16", what=what))
    for b in (dx, dw, x, dz):
        b.check_untouched(what)
    e = ER.sum_rule_err(dw.inner().view(c, 9), pre.double() + rdw)
    print(f"{what}: dw err {e:.3g}")
    assert e < 1e-4, e


# ------------------------------------------------------------------------------------------------ ym_bn_eval_coeff
def test_bn_eval_coeff():
    """scale within 4 fp32 ulps of fp64 gamma / sqrt(var + eps) (an add, a square root, a division, a multiply);
    shift within the two roundings of beta - mean * scale on the stored scale; the batch form bit-identical."""
    from yolomi._lib import BnEvalEntry
    call, lib, st = _abi()
    eps = 1e-3
    keep, single, batch = [], [], []
    Cs = (8, 24, 257, 2048)
    table = (BnEvalEntry * len(Cs))()
    for e, C in zip(table, Cs):
        g = torch.Generator().manual_seed(C)
        p = [t.to(_dev()) for t in (1 + 0.5 * torch.randn(C, generator=g), torch.randn(C, generator=g),
                                    torch.randn(C, generator=g), torch.rand(C, generator=g) * 2 + 1e-4)]
        out = [Guarded(1, C + 8, "f32", c=C, off=0) for _ in range(4)]
        call("ym_bn_eval_coeff", C, *[t.data_ptr() for t in p], eps, out[0].ptr, out[1].ptr, st)
        e.gamma, e.beta, e.running_mean, e.running_var = (t.data_ptr() for t in p)
        e.scale, e.shift, e.c, e.eps = out[2].ptr, out[3].ptr, C, eps
        keep.append((p, out))
    tab = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(_dev())
    call("ym_bn_eval_coeff_batch", tab.data_ptr(), len(Cs), st)
    torch.cuda.synchronize()
    for C, (p, out) in zip(Cs, keep):
        sc, sh, sc_b, sh_b = (o.inner().view(-1) for o in out)
        for o in out:
            o.check_untouched(f"ym_bn_eval_coeff C={C}")
        rsc, _ = ER.bn_eval_coeff_ref(*p, eps)
        u = float(((sc.double() - rsc).abs() / ER.ulp32(rsc)).max())
        rsh = p[1].double() - p[2].double() * sc.double()
        tol = 0.5 * ER.ulp32(p[2].double() * sc.double()) + 0.5 * ER.ulp32(rsh)
        v = float(((sh.double() - rsh).abs() / tol).max())
        print(f"ym_bn_eval_coeff C={C}: scale {u:.2f} fp32 ulps, shift {v:.2f} of its two roundings")
        assert u <= 4.0 and v <= 1.0, (u, v)
        assert torch.equal(sc.view(torch.int32), sc_b.view(torch.int32))
        assert torch.equal(sh.view(torch.int32), sh_b.view(torch.int32))
