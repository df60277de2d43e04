"""Cases, integer operands, buffers and the fp64 reference of the exact data-gradient tests (ym_conv_dgrad: conv.hip,
conv_halo.hip, conv_pipe.hip, conv_hpipe.hip, conv_direct.hip).  Plain torch and ctypes descriptors, no GPU needed:
tests/test_dgrad_exact_cpu.py keeps this file honest, tests/test_gpu_dgrad_exact.py holds every kernel instance to it
bit for bit.

Why the comparison is exact.  dz (bf16) and the data-gradient weight copy (bf16, [cin][kh][kw][cout]) hold integers in
[-4, 4].  Every product is an integer of magnitude <= 16, exact in fp32; every partial sum of the fp32 MFMA accumulation
is an integer bounded by k * k * cout * 16 (`exact_bound`, < 2^24 with a wide margin: 9 * 136 * 16 = 19 584 at most
here), so the summation order does not matter and the accumulator must equal v = conv2d_input(...) BY VALUE.  The
output is then a deterministic function of v, and each case has three runs:

  A  overwrite, "large" operands ([lo, 4], lo = -4 unless the case says otherwise): dx = bf16(v), compared as int16 bit
     patterns.  Above 256 every odd integer is a bf16 tie (8 significand bits: spacing 2), so values |v| = 1 and 3
     (mod 4) in (256, 512) pin round-to-nearest-even: 257 -> 256 and 259 -> 260, where truncation gets 259 wrong and
     round-half-away 257.  dx inside the view is prefilled with NaN: every pixel and channel must be written.
  B  accumulate, "small" operands ({-1, 0, 1}; max|v| <= 256 on every case — a condition, not a tolerance, and no case
     here needs its operands thinned to meet it): v is exactly representable in bf16, so both epilogue forms give
     bf16(old + v) with a single rounding; old = integers in [-1000, 1000] through .bfloat16().  The same bits for
     every kernel.
  C  accumulate, run A's operands onto run B's prefill: the form pin.  E1 = bf16(old + v) (one rounding, the fragment
     epilogues), E2 = bf16(bf16(v) + old) (two roundings, the 16-byte epilogues); the GPU test holds each instance and
     store path to the form its code has.

Views.  dz sits in a buffer of cout + ye channels at channel offset cy, dx in one of cin + xe channels at offset cx,
both with a per-image gap.  ye, cy and the dz gap are multiples of 8 (the ABI's 16-byte rule for dz); the dx view
only needs 8 bytes (x_ld % 4 == 0): "view" is 16-byte aligned, "view8" has x_ld % 8 == 4 (xe = 4), "view8p" a 16-byte
pixel pitch but a dx pointer 8 bytes past a 16-byte boundary (cx = 4), and "view4" (CIN4_CASES) is 16-byte aligned
around a cin of 8 j + 4.  Everything of the dz buffer outside the view is NaN (the GEMM masks its K tail with
kk < Kin, the other families require whole chunks: nothing may read it), everything of the dx buffer outside the view
is a sentinel pattern that must come back bit-unchanged.
"""
import ctypes
import functools
import zlib
from dataclasses import dataclass

import torch

PREFILL_MAX = 1000                               # |old| of the accumulate runs

# every (family, template instance) ym_conv_dgrad can launch: 15.  conv.hip launch_tile (3 tiles), conv_halo.hip
# halo_launch (C8, C4), conv_pipe.hip launch (2 tiles x {DGRAD_C1, DGRAD_GEN}), conv_hpipe.hip hpipe_launch (cfg 0, 2;
# cfg 1 is unreachable), conv_direct.hip kVariants (1, 3, 5, 7).
INSTANCES = (
    ("gemm", "128x32"), ("gemm", "128x64"), ("gemm", "128x128"),
    ("halo", "C8"), ("halo", "C4"),
    ("pipe", "256x128 C1"), ("pipe", "256x128 GEN"), ("pipe", "256x64 C1"), ("pipe", "256x64 GEN"),
    ("hpipe", "128"), ("hpipe", "64 wres"),
    ("direct", "v1"), ("direct", "v3"), ("direct", "v5"), ("direct", "v7"),
)
FAMILIES = ("gemm", "halo", "pipe", "hpipe", "direct")
# the policy that selects a family: every other family off (ym_conv_set_halo / _pipe / _direct / _hpipe)
FAMILY_POLICY = {
    "gemm": dict(halo=0, pipe=0, direct=0, hpipe=0),
    "halo": dict(halo=1, pipe=0, direct=0, hpipe=0),
    "pipe": dict(halo=0, pipe=2, direct=0, hpipe=0),
    "hpipe": dict(halo=0, pipe=0, direct=0, hpipe=2),
    "direct": dict(halo=0, pipe=0, direct=2, hpipe=0),
}

# the dx / dz views: (xe, cx, x_gap, ye, cy, y_gap)
VIEWS = {
    "plain": (0, 0, 0, 0, 0, 0),
    "view": (16, 8, 64, 24, 16, 32),
    "view8": (4, 0, 12, 24, 16, 32),             # x_ld % 8 == 4, x_bs % 8 == 4
    "view8p": (8, 4, 16, 24, 16, 32),            # x_ld % 8 == 0, the dx pointer 8 bytes past a 16-byte boundary
    "view4": (4, 0, 8, 24, 16, 32),              # for cin % 8 == 4: a 16-byte aligned view ending in half a 16-byte run
}


@dataclass(frozen=True)
class Case:
    name: str
    family: str
    inst: str                    # template instance within the family (INSTANCES)
    shape: tuple                 # n, h, w, cin, cout, k, stride, pad (the FORWARD descriptor)
    kid: int                     # expected ym_conv_kernel(d, 1)
    kname: str                   # expected kernel name
    view: str = "plain"          # key of VIEWS
    sel: int = 0                 # ym_conv_set_select_batch
    default_policy: bool = False  # the ABI-edge cases: no family forced
    lo: int = -4                 # run A operands in [lo, 4]
    tie: bool = False            # the CPU test asserts run A's tie condition on this case
    forms_differ: bool = True    # run C discriminates E1 from E2 on this case
    note: str = ""

    @property
    def n(self):
        return self.shape[0]

    @property
    def oh(self):
        n, h, w, cin, cout, k, s, p = self.shape
        return (h + 2 * p - k) // s + 1

    @property
    def ow(self):
        n, h, w, cin, cout, k, s, p = self.shape
        return (w + 2 * p - k) // s + 1

    @property
    def xe(self):
        return VIEWS[self.view][0]

    @property
    def cx(self):
        return VIEWS[self.view][1]

    @property
    def ye(self):
        return VIEWS[self.view][3]

    @property
    def cy(self):
        return VIEWS[self.view][4]

    @property
    def x_ld(self):
        return self.shape[3] + self.xe

    @property
    def y_ld(self):
        return self.shape[4] + self.ye

    @property
    def x_bs(self):
        return self.shape[1] * self.shape[2] * self.x_ld + VIEWS[self.view][2]

    @property
    def y_bs(self):
        return self.oh * self.ow * self.y_ld + VIEWS[self.view][5]

    @property
    def aligned(self):
        """The dx view allows 16-byte stores of whole 8-channel runs (ym_conv_dgrad's ep_lds, halo_launch's)."""
        return self.x_ld % 8 == 0 and self.x_bs % 8 == 0 and self.cx % 8 == 0 and self.shape[3] % 8 == 0

    @property
    def signed(self):
        return self.lo < 0


def pipe_inst(shape):
    """pipe_launch's rule: the single-class instance for one output class on maps of >= 256 pixels (both tiles are 256
    pixels high), else the generic one."""
    n, h, w, cin, cout, k, s, p = shape
    return "C1" if s == 1 and h * w >= 256 else "GEN"


def _name(kid, shape, view, tag=""):
    n, h, w, cin, cout, k, s, p = shape
    return f"{kid}-n{n}h{h}w{w}c{cin}o{cout}k{k}s{s}p{p}-{view}" + (f"-{tag}" if tag else "")


def _cases(family, inst, kid, kname, shape, views, **kw):
    return [Case(_name(kid, shape, v), family, inst, shape, kid, kname, view=v, **kw) for v in views]


ALL_VIEWS = ("plain", "view", "view8", "view8p")
V16 = ("plain", "view")          # hpipe_plan requires x_ld % 8 == 0 and x_bs % 8 == 0

# (family, instance, id, name, shape, keyword arguments).  lo > -4: run A's operands in [lo, 4], so that |v| runs well
# past 256 on a short K (with lo >= 0 the case is a rounding pin of positive values).
TABLE = [
    # ---- 2-stage GEMM (conv.hip): the store path is chosen at run time, every tile runs under both
    ("gemm", "128x32", 32, "gemm 128x32", (2, 9, 11, 40, 72, 3, 1, 1), dict(tie=True)),
    ("gemm", "128x32", 32, "gemm 128x32 4-class", (2, 9, 11, 24, 40, 3, 2, 1), dict(lo=0, tie=True)),
    ("gemm", "128x32", 32, "gemm 128x32 4-class", (1, 7, 5, 48, 40, 1, 2, 0), dict(lo=2, note="three empty classes")),
    # |v| <= 8 * 16 = 128 whatever the operands: every value is representable and the two forms coincide
    ("gemm", "128x32", 32, "gemm 128x32", (1, 6, 6, 16, 8, 1, 1, 0), dict(forms_differ=False, note="Kin = 8")),
    ("gemm", "128x64", 64, "gemm 128x64", (2, 9, 11, 72, 40, 3, 1, 1), dict(sel=512)),
    ("gemm", "128x64", 64, "gemm 128x64 4-class", (2, 9, 11, 72, 40, 3, 2, 1), dict(sel=2048, lo=0)),
    ("gemm", "128x64", 64, "gemm 128x64", (2, 9, 9, 72, 136, 1, 1, 0), dict(sel=512, lo=0)),
    ("gemm", "128x128", 128, "gemm 128x128", (2, 9, 11, 136, 40, 3, 1, 1), dict(sel=512)),
    ("gemm", "128x128", 128, "gemm 128x128 4-class", (2, 9, 11, 136, 16, 3, 2, 1), dict(sel=2048, lo=2)),
    ("gemm", "128x128", 128, "gemm 128x128", (1, 9, 9, 264, 72, 1, 1, 0), dict(sel=512, lo=0)),
    # ---- halo (conv_halo.hip): 16-wide and whole-row tiles, partial last tile rows
    ("halo", "C4", 1116, "halo C4 8x16", (1, 16, 16, 64, 72, 3, 1, 1), dict(tie=True)),
    ("halo", "C4", 1116, "halo C4 8x16", (1, 9, 48, 64, 16, 3, 1, 1), dict(
        lo=0, tie=True, note="three column tiles, partial row tile")),
    ("halo", "C4", 1110, "halo C4 12x10", (2, 12, 10, 72, 40, 3, 1, 1), dict()),
    ("halo", "C4", 1120, "halo C4 6x20", (1, 11, 20, 64, 64, 3, 1, 1), dict(note="partial last tile row")),
    ("halo", "C4", 1107, "halo C4 18x7", (2, 18, 7, 64, 8, 3, 1, 1), dict(lo=0, note="Kin = 8")),
    ("halo", "C8", 1016, "halo C8 16x16", (1, 28, 16, 136, 64, 3, 1, 1), dict(sel=512, note="partial last tile row")),
    ("halo", "C8", 1020, "halo C8 12x20", (1, 23, 20, 72, 64, 3, 1, 1), dict(sel=512)),
    # ---- pipelined GEMM (conv_pipe.hip): a persistent grid of 256 workgroups over a handful of tiles
    ("pipe", "256x128 C1", 2000, "pipe 256x128", (1, 16, 16, 136, 64, 3, 1, 1), dict(sel=1024, tie=True)),
    ("pipe", "256x128 GEN", 2000, "pipe 256x128", (3, 9, 9, 128, 64, 1, 1, 0), dict(
        sel=4096, lo=0, tie=True, note="81-pixel maps: tiles span images")),
    ("pipe", "256x128 GEN", 2000, "pipe 256x128", (2, 17, 15, 128, 64, 3, 2, 1), dict(sel=4096, lo=0,
                                                                                   note="four unequal classes")),
    ("pipe", "256x64 C1", 2001, "pipe 256x64", (1, 17, 16, 72, 64, 3, 1, 1), dict(sel=1024)),
    ("pipe", "256x64 C1", 2001, "pipe 256x64", (1, 16, 17, 40, 128, 1, 1, 0), dict(sel=1024, lo=0)),
    ("pipe", "256x64 GEN", 2001, "pipe 256x64", (2, 17, 15, 64, 64, 3, 2, 1), dict(sel=4096, lo=0)),
    # ---- halo-pipelined (conv_hpipe.hip)
    ("hpipe", "128", 4000, "hpipe 16x16px x 128", (1, 16, 32, 136, 64, 3, 1, 1), dict(tie=True,
                                                                                   note="partial second channel tile")),
    ("hpipe", "128", 4000, "hpipe 16x16px x 128", (2, 16, 16, 192, 128, 3, 1, 1), dict()),
    ("hpipe", "64 wres", 4002, "hpipe 16x16px x 64 wres", (1, 16, 32, 64, 64, 3, 1, 1), dict()),
    # ---- direct (conv_direct.hip)
    ("direct", "v1", 3001, "direct v1", (1, 9, 11, 32, 64, 3, 2, 1), dict(lo=0, tie=True, note="partial quads")),
    ("direct", "v1", 3001, "direct v1", (2, 8, 6, 32, 64, 3, 2, 1), dict(lo=0, note="whole quads")),
    ("direct", "v1", 3001, "direct v1", (1, 9, 11, 24, 64, 3, 2, 1), dict(lo=0, note="Nout = 24")),
    ("direct", "v3", 3003, "direct v3", (1, 7, 9, 32, 32, 3, 1, 1), dict(lo=-2)),
    ("direct", "v3", 3003, "direct v3", (1, 7, 9, 24, 32, 3, 1, 1), dict(lo=-2, note="Nout = 24")),
    ("direct", "v5", 3005, "direct v5", (1, 5, 7, 64, 64, 1, 1, 0), dict(lo=0)),
    ("direct", "v5", 3005, "direct v5", (1, 5, 7, 56, 64, 1, 1, 0), dict(lo=0, note="Nout = 56")),
    ("direct", "v7", 3007, "direct v7", (1, 5, 7, 96, 128, 1, 1, 0), dict(lo=0)),
    ("direct", "v7", 3007, "direct v7", (1, 5, 7, 88, 128, 1, 1, 0), dict(lo=0, note="Nout = 88")),
]

CASES = [c for fam, inst, kid, kname, shape, kw in TABLE
         for c in _cases(fam, inst, kid, kname, shape, V16 if fam == "hpipe" else ALL_VIEWS, **kw)]

# ---- ABI edges: kernel sizes and pads the network does not use (ym_conv_dgrad accepts any k in 1..3 with any pad), on
# the 2-stage GEMM under the default policy
EDGE_CASES = [
    Case(_name(32, (2, 8, 8, 16, 24, 2, 2, 0), "view", "edge"), "gemm", "128x32", (2, 8, 8, 16, 24, 2, 2, 0), 32,
         "gemm 128x32 4-class", view="view", default_policy=True, lo=3, note="k = 2, stride 2"),
    Case(_name(32, (1, 9, 9, 16, 24, 3, 1, 0), "view", "edge"), "gemm", "128x32", (1, 9, 9, 16, 24, 3, 1, 0), 32,
         "gemm 128x32", view="view", default_policy=True, lo=0, note="3x3 without padding"),
]
# cin % 8 == 4 in a view whose pitch and pointer are 16-byte aligned (the ABI asks x_ld % 4 == 0 of dx and nothing of
# cin): the last 16-byte run of a pixel is half cin's, half the neighbouring slice's.  Only the GEMM and the halo
# kernel take such a cin (the other planners require cin % 8 == 0); the 16-byte epilogue of the GEMM's 64- and
# 128-channel tiles and of the halo kernel stores whole runs, so these views must take the fragment epilogue.
CIN4_CASES = [
    Case(_name(32, (2, 9, 11, 44, 72, 3, 1, 1), "view4", "cin4"), "gemm", "128x32", (2, 9, 11, 44, 72, 3, 1, 1), 32,
         "gemm 128x32", view="view4"),                         # (this tile stores fragments whatever the view)
    Case(_name(64, (2, 9, 11, 68, 40, 3, 1, 1), "view4", "cin4"), "gemm", "128x64", (2, 9, 11, 68, 40, 3, 1, 1), 64,
         "gemm 128x64", view="view4", sel=512),
    Case(_name(128, (2, 9, 11, 132, 40, 3, 1, 1), "view4", "cin4"), "gemm", "128x128", (2, 9, 11, 132, 40, 3, 1, 1),
         128, "gemm 128x128", view="view4", sel=512),
    Case(_name(1116, (1, 16, 16, 68, 72, 3, 1, 1), "view4", "cin4"), "halo", "C4", (1, 16, 16, 68, 72, 3, 1, 1), 1116,
         "halo C4 8x16", view="view4"),
    Case(_name(1016, (1, 28, 16, 132, 64, 3, 1, 1), "view4", "cin4"), "halo", "C8", (1, 28, 16, 132, 64, 3, 1, 1), 1016,
         "halo C8 16x16", view="view4", sel=512),
]
ALL_CASES = CASES + EDGE_CASES + CIN4_CASES
assert len({c.name for c in ALL_CASES}) == len(ALL_CASES)


def case_id(c):
    return c.name


# ---- descriptor and selection (host side)
def desc(c, n=None, accumulate=0):
    """The forward ym_conv_desc of case c (of n images instead of c.n if given)."""
    from yolomi._lib import ConvDesc
    _, h, w, cin, cout, k, s, p = c.shape
    d = ConvDesc()
    d.n, d.h, d.w, d.cin, d.oh, d.ow, d.cout, d.k, d.stride, d.pad = c.n if n is None else n, h, w, cin, c.oh, c.ow, \
        cout, k, s, p
    d.x_bs, d.x_ld, d.y_bs, d.y_ld = c.x_bs, c.x_ld, c.y_bs, c.y_ld
    d.out_f32, d.accumulate = 2, accumulate
    return d


class policy:
    """with policy(c): the library selects under c's family policy and selection batch; every setter is restored on
    the way out."""

    def __init__(self, c):
        self.want = {} if c.default_policy else dict(FAMILY_POLICY[c.family])
        self.want["select_batch"] = c.sel

    def __enter__(self):
        from yolomi._lib import lib
        self.prev = []
        for key, v in self.want.items():
            fn = getattr(lib(), "ym_conv_set_" + key)
            self.prev.append((fn, fn(v)))
        return self

    def __exit__(self, *exc):
        for fn, v in reversed(self.prev):
            fn(v)


def kernel(c, d=None):
    """(id, name) of the data-gradient kernel of case c under its policy."""
    from yolomi._lib import lib
    d = desc(c) if d is None else d
    name = ctypes.create_string_buffer(96)
    with policy(c):
        kid = lib().ym_conv_kernel(ctypes.byref(d), 1, name, 96)
    return kid, name.value.decode()


# ---- operands and reference
def _seed(c):
    # per shape and view, so that the views of one shape are different draws
    return zlib.crc32(c.name.encode()) & 0x7FFFFFFF


@functools.lru_cache(maxsize=None)
def operands(c, run):
    """(dz, w) of run "large" (A and C) or "small" (B): dz (n, oh, ow, cout) and w (cout, cin, k, k) bf16 integers.
    Seeded per case; shared, do not modify."""
    n, h, w, cin, cout, k, s, p = c.shape
    g = torch.Generator().manual_seed(_seed(c) ^ (0 if run == "large" else 0x3C3C))
    if run == "large":
        dz = torch.randint(c.lo, 5, (n, c.oh, c.ow, cout), generator=g)
        wt = torch.randint(c.lo, 5, (cout, cin, k, k), generator=g)
    else:
        assert run == "small"
        dz = torch.randint(-1, 2, (n, c.oh, c.ow, cout), generator=g)
        wt = torch.randint(-1, 2, (cout, cin, k, k), generator=g)
    return dz.to(torch.bfloat16), wt.to(torch.bfloat16)


def _conv2d_input(c, run, dtype):
    n, h, w, cin, cout, k, s, p = c.shape
    dz, wt = operands(c, run)
    v = torch.nn.grad.conv2d_input((n, cin, h, w), wt.to(dtype), dz.to(dtype).permute(0, 3, 1, 2), stride=s, padding=p)
    return v.permute(0, 2, 3, 1).contiguous()


def exact_bound(c, run):
    """The magnitude no partial sum of the run exceeds (before the prefill); exact while < 2^24."""
    n, h, w, cin, cout, k, s, p = c.shape
    return k * k * cout * (16 if run == "large" else 1)


@functools.lru_cache(maxsize=None)
def reference(c, run):
    """v (n, h, w, cin) in fp64 by torch.nn.grad.conv2d_input on the same integers; shared, do not modify."""
    v = _conv2d_input(c, run, torch.float64)
    assert bool((v == v.round()).all()), "reference not integral"
    assert exact_bound(c, run) + PREFILL_MAX < 2 ** 24
    assert float(v.abs().max()) <= exact_bound(c, run)
    return v


def reference_f32(c, run):
    return _conv2d_input(c, run, torch.float32)


@functools.lru_cache(maxsize=None)
def prefill(c):
    """old (n, h, w, cin) bf16: integers in [-1000, 1000] through .bfloat16() (those above 256 round to bf16's grid)."""
    n, h, w, cin, cout, k, s, p = c.shape
    g = torch.Generator().manual_seed(_seed(c) ^ 0x5A5A)
    return torch.randint(-PREFILL_MAX, PREFILL_MAX + 1, (n, h, w, cin), generator=g).float().bfloat16()


def bits(t):
    """bf16 tensor -> its int16 bit patterns."""
    assert t.dtype == torch.bfloat16
    return t.contiguous().view(torch.int16)


def expect_overwrite(c):
    """Run A: bf16(v), round to nearest even."""
    return reference(c, "large").float().bfloat16()


def expect_small(c):
    """Run B: bf16(old + v), v representable: one rounding under either form."""
    return (prefill(c).float() + reference(c, "small").float()).bfloat16()


def expect_form(c, form):
    """Run C: E1 = bf16(old + v), E2 = bf16(bf16(v) + old).  old + v is an integer below 2^24: exact in fp32."""
    v, old = reference(c, "large").float(), prefill(c).float()
    if form == "E1":
        return (old + v).bfloat16()
    assert form == "E2"
    return (v.bfloat16().float() + old).bfloat16()


def round_trunc(v):
    """fp32 -> bf16 by truncation (what a pk2bf without rounding would give)."""
    return (v.float().contiguous().view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16)


def round_half_away(v):
    """fp32 -> bf16 rounding halves away from zero."""
    b = v.float().contiguous().view(torch.int32)
    return (((b & 0x7FFFFFFF) + 0x8000) >> 16 | ((b >> 16) & 0x8000)).to(torch.int16).view(torch.bfloat16)


# ---- buffers
def sentinel(numel):
    """The pattern of dx-buffer elements outside the view: position dependent, never a bf16 the kernels produce here
    (exponent bits all set with a payload: NaNs of varying payload)."""
    i = torch.arange(numel, dtype=torch.int64)
    return ((i * 37 + 11) % 127 + 0x7F81).to(torch.int16)      # 0x7F81 .. 0x7FFF


def dz_buffer(c, run):
    """The flat NaN-filled bf16 buffer the dz view lives in; the kernel is handed data_ptr() + 2 * c.cy."""
    n, h, w, cin, cout, k, s, p = c.shape
    dz, _ = operands(c, run)
    buf = torch.full((n * c.y_bs,), float("nan"), dtype=torch.bfloat16)
    assert c.cy + cout <= c.y_ld
    buf.as_strided((n, c.oh, c.ow, cout), (c.y_bs, c.ow * c.y_ld, c.y_ld, 1), c.cy).copy_(dz)
    assert int(torch.isfinite(buf.float()).sum()) == dz.numel()
    return buf


def weight_buffer(c, run):
    """The data-gradient weight copy [cin][kh][kw][cout] bf16 at its exact size."""
    _, wt = operands(c, run)
    return wt.permute(1, 2, 3, 0).contiguous().reshape(-1)


def dx_view(c, buf):
    """The (n, h, w, cin) view of the flat dx buffer `buf` (int16 or bf16) the kernel writes."""
    n, h, w, cin, cout, k, s, p = c.shape
    return buf.as_strided((n, h, w, cin), (c.x_bs, w * c.x_ld, c.x_ld, 1), c.cx)


def dx_buffer(c, fill):
    """The flat int16 dx buffer: sentinels everywhere, `fill` (a bf16 (n, h, w, cin) tensor, or None for NaN) in the
    view; the kernel is handed data_ptr() + 2 * c.cx."""
    n, h, w, cin, cout, k, s, p = c.shape
    assert c.cx + cin <= c.x_ld
    buf = sentinel(n * c.x_bs)
    view = dx_view(c, buf)
    if fill is None:
        view.fill_(0x7FC0)                                      # the canonical quiet NaN
    else:
        view.copy_(bits(fill))
    return buf


def outside_mask(c):
    """True where a flat dx-buffer element lies outside the view."""
    m = torch.ones(c.n * c.x_bs, dtype=torch.bool)
    dx_view(c, m).fill_(False)
    return m


# ---- reporting
def locate(c, img, y, x, ch):
    """The tile, class or quad a dx element belongs to under the case's kernel."""
    n, h, w, cin, cout, k, s, p = c.shape
    if c.family == "gemm" or c.family == "pipe":
        bm = 128 if c.family == "gemm" else 256
        bn = int(c.inst.split()[0].split("x")[1])
        py, px = (y % 2, x % 2) if s == 2 else (0, 0)
        ohc, owc = (h - py + s - 1) // s, (w - px + s - 1) // s
        m = (img * ohc + y // s) * owc + x // s
        cls = f"class ({py}, {px}), " if s == 2 else ""
        return f"{cls}m-tile {m // bm} row {m % bm}, channel tile {ch // bn}"
    if c.family == "halo":
        th, tw = (int(t) for t in c.kname.split()[-1].split("x"))
        bn = 128 if c.inst == "C8" else 64
        return (f"tile (row {y // th}, column {x // tw}) of image {img}, pixel ({y % th}, {x % tw}), "
                f"channel tile {ch // bn}")
    if c.family == "hpipe":
        bn = 128 if c.inst == "128" else 64
        return f"16x16 tile ({y // 16}, {x // 16}) of image {img}, channel tile {ch // bn}"
    if c.inst == "v1":
        return f"quad ({y // 2}, {x // 2}) of image {img}, class ({y % 2}, {x % 2})"
    tp = {"v3": 2, "v5": 4, "v7": 4}[c.inst]
    m = (img * h + y) * w + x
    return f"task {m // (16 * tp)} group {m % (16 * tp) // 16} pixel {m % 16}, channel subtile {ch // 16}"


def mismatch(c, got, want):
    """None if got == want bit for bit, else a message with the count of mismatches and the first one's (image, y, x,
    channel), its tile / class / quad and got / want.  Both (n, h, w, cin) bf16 on the CPU."""
    bad = bits(got) != bits(want)
    count = int(bad.sum())
    if count == 0:
        return None
    img, y, x, ch = (int(v) for v in bad.nonzero()[0])
    g, w_ = got[img, y, x, ch], want[img, y, x, ch]
    return (f"{c.name} ({c.kname}, {c.inst}): {count} of {bad.numel()} elements differ; first at (image {img}, y {y}, "
            f"x {x}, channel {ch}), {locate(c, img, y, x, ch)}: got {float(g)!r} (0x{int(bits(g)) & 0xFFFF:04x}), want "
            f"{float(w_)!r} (0x{int(bits(w_)) & 0xFFFF:04x})")
