"""Cases, integer operands, buffers and the fp64 reference of the exact forward tests (ym_conv_fwd / ym_conv_fwd_bn:
conv.hip, conv_halo.hip, conv_pipe.hip, conv_hpipe.hip, conv_direct.hip).  Plain torch and ctypes descriptors, no GPU
needed: tests/test_fwd_exact_cpu.py keeps this file honest, tests/test_gpu_fwd_exact.py holds every kernel instance to
it bit for bit.  The policy, sentinel and seeding helpers are tests/dgrad_exact_cases.py's.

Why the comparison is exact.  x (fp16, NHWC) and w (fp16, [cout][kh][kw][cin]) hold integers of magnitude <= 16.
Every product is an integer of magnitude <= 256, exact in fp32; every partial sum of the fp32 MFMA accumulation is an
integer bounded by k * k * cin * 256 (`exact_bound`, asserted < 2^24 per case: 9 * 128 * 256 = 294 912 at most here),
so the summation order does not matter and the accumulator must equal v = conv2d(x, w) in fp64 BY VALUE.  Every
output is then a deterministic function of v:

  A  overwrite with fp16 z and statistics (the network's mode), operands in the case's [lo, hi]: z = fp16(v), compared
     as int16 bit patterns.  In (2048, 4096) fp16's spacing is 2, so every odd integer is a tie: |v| = 1 and 3 (mod 4)
     pin round-to-nearest-even (2049 -> 2048, 2051 -> 2052), where truncation gets 2051 wrong and round-half-away
     2049.  The fp64 sum of the statistics rows of stat_sum equals sum(v) exactly (pixels * max|v| < 2^24: every
     partial row sum is an exact integer under any partition) and differs from sum(fp16(v)): the statistics come
     from the accumulator.  stat_sq is an fp32 sum of squares that may round, held to the bound of `sq_bound`.
  S  the same with operands in {-1, 0, 1}: max|v| <= 2048 and per channel sum(v^2) < 2^24, so z = v by value and the
     row sums of BOTH statistics arrays are exact.  The statistics are prefilled with NaN (every row must be written,
     also by workgroups that own no tile) and followed by a canary row.
  the other outputs (OTHER): bf16 with ties in (256, 512) (operands in [blo, 4], as the data-gradient tests), fp32 by
     value, an integer bias on all three, accumulate into fp32 (old + v exactly) and bf16 (form E1 = bf16(old + v)
     or E2 = bf16(bf16(v) + old) per store path), and the fp16 clamp (CLAMP_CASES: x = 16, w = +-16 by channel parity,
     |v| = k * k * cin * 256 > 65504 at the interior pixels).

Views.  x sits in a NaN-filled buffer of cin + xe channels at channel offset cx with a per-image gap (all multiples
of 8: the ABI's 16-byte rule for x), y in a buffer of cout + ye channels at offset cy whose every element outside the
view is a sentinel that must come back bit-unchanged.  "view" is 16-byte aligned, "view8" has y_ld % 8 == 4, "view8p" a
16-byte pixel pitch but a y pointer 8 bytes past a 16-byte boundary, "view4" is 16-byte aligned around a cout of
8 j + 4, "view6" holds a cout of 4 j + 2 (6, 70) 8-byte aligned, "wide" is the Detect head's fp32 row (no alignment
at all).
"""
import functools
from dataclasses import dataclass

import torch

import dgrad_exact_cases as D

FAMILIES = D.FAMILIES
PREFILL_MAX = D.PREFILL_MAX

# every (family, template instance) ym_conv_fwd can launch: 17.  conv.hip launch_tile (3 tiles), conv_halo.hip
# halo_launch (C8, C4), conv_pipe.hip launch (2 tiles x {FWD_GEN, FWD_C1, FWD_C1_TAP}), conv_hpipe.hip hpipe_launch
# (cfg 0, 2; cfg 1 is unreachable), conv_direct.hip kVariants (0, 2, 4, 6).
INSTANCES = (
    ("gemm", "128x32"), ("gemm", "128x64"), ("gemm", "128x128"),
    ("halo", "C8"), ("halo", "C4"),
    ("pipe", "256x128 GEN"), ("pipe", "256x128 C1"), ("pipe", "256x128 C1 TAP"),
    ("pipe", "256x64 GEN"), ("pipe", "256x64 C1"), ("pipe", "256x64 C1 TAP"),
    ("hpipe", "128"), ("hpipe", "64 wres"),
    ("direct", "v0"), ("direct", "v2"), ("direct", "v4"), ("direct", "v6"),
)

# the views: (ye, cy, y_gap, xe, cx, x_gap)
VIEWS = {
    "plain": (0, 0, 0, 0, 0, 0),
    "view": (16, 8, 64, 24, 16, 32),
    "view8": (4, 0, 12, 24, 16, 32),             # y_ld % 8 == 4, y_bs % 8 == 4
    "view8p": (8, 4, 16, 24, 16, 32),            # y_ld % 8 == 0, the y pointer 8 bytes past a 16-byte boundary
    "view4": (4, 0, 8, 24, 16, 32),              # cout % 8 == 4: a 16-byte aligned view ending in half a 16-byte run
    "view6": (10, 4, 8, 24, 16, 32),             # cout % 4 == 2 (6, 70) in rows of cout + 10 channels, 8-byte aligned
    "wide": (64, 5, 7, 8, 8, 8),                 # fp32 only: the Detect head's slice of a wide row, odd offsets
}
OUT_DTYPE = {0: torch.bfloat16, 1: torch.float32, 2: torch.float16}


@dataclass(frozen=True)
class Case:
    name: str
    family: str
    inst: str                    # template instance within the family (INSTANCES)
    shape: tuple                 # n, h, w, cin, cout, k, stride, pad
    kid: int                     # expected ym_conv_kernel(d, 0)
    kname: str                   # expected kernel name
    view: str = "plain"          # key of VIEWS
    sel: int = 0                 # ym_conv_set_select_batch
    default_policy: bool = False  # no family forced
    lo: int = -16                # run A operands in [lo, hi]
    hi: int = 16
    blo: int = -4                # the bf16 runs' operands in [blo, 4]
    tie: bool = False            # the CPU test asserts run A's tie condition on this case
    rounds: bool = True          # run A: some |v| is not an fp16 value, so sum(v) != sum(fp16(v))
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
    def pixels(self):
        return self.n * self.oh * self.ow

    @property
    def cout(self):
        return self.shape[4]

    @property
    def cy(self):
        return VIEWS[self.view][1]

    @property
    def cx(self):
        return VIEWS[self.view][4]

    @property
    def y_ld(self):
        return self.shape[4] + VIEWS[self.view][0]

    @property
    def x_ld(self):
        return self.shape[3] + VIEWS[self.view][3]

    @property
    def y_bs(self):
        return self.oh * self.ow * self.y_ld + VIEWS[self.view][2]

    @property
    def x_bs(self):
        return self.shape[1] * self.shape[2] * self.x_ld + VIEWS[self.view][5]

    @property
    def aligned(self):
        """The y view allows 16-byte stores of whole 8-channel runs (conv_fwd_impl's ep_lds, halo_launch's)."""
        return self.y_ld % 8 == 0 and self.y_bs % 8 == 0 and self.cy % 8 == 0 and self.shape[4] % 8 == 0

    @property
    def signed(self):
        return self.lo < 0


def pipe_inst(shape):
    """pipe_launch's rule for the forward: the single-class instance on maps of >= 256 output pixels (both tiles are
    256 pixels high), tap-innermost where tap_inner says (3x3 stride 2 reading maps >= 128 wide); else the generic."""
    n, h, w, cin, cout, k, s, p = shape
    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    if oh * ow < 256:
        return "GEN"
    return "C1 TAP" if s == 2 and k == 3 and w >= 128 else "C1"


def _name(kid, shape, view, tag=""):
    n, h, w, cin, cout, k, s, p = shape
    return f"{kid}-n{n}h{h}w{w}c{cin}o{cout}k{k}s{s}p{p}-{view}" + (f"-{tag}" if tag else "")


ALL_VIEWS = ("plain", "view", "view8", "view8p")
V16 = ("plain", "view", "view8p")    # hpipe_plan requires y_ld % 8 == 0 and y_bs % 8 == 0 (and does not see the pointer)

# (family, instance, id, name, shape, keyword arguments).  lo >= 0: a short K needs one-signed operands to pass 2048.
TABLE = [
    # ---- 2-stage GEMM (conv.hip): 198 pixels are two m-tiles under the grid of 8 (six workgroups own no tile)
    ("gemm", "128x32", 32, "gemm 128x32", (2, 9, 11, 40, 72, 3, 1, 1), dict(tie=True)),
    ("gemm", "128x32", 32, "gemm 128x32", (2, 8, 8, 16, 24, 2, 2, 0), dict(lo=4, note="k = 2, stride 2")),
    ("gemm", "128x32", 32, "gemm 128x32", (1, 9, 9, 16, 24, 3, 1, 0), dict(lo=0, note="3x3 without padding")),
    ("gemm", "128x64", 64, "gemm 128x64", (2, 9, 11, 72, 72, 3, 1, 1), dict(sel=512, tie=True)),
    ("gemm", "128x64", 64, "gemm 128x64", (2, 9, 11, 24, 72, 3, 2, 1), dict(sel=2048, lo=0, note="stride 2")),
    ("gemm", "128x128", 128, "gemm 128x128", (2, 9, 11, 40, 136, 3, 1, 1), dict(sel=512)),
    ("gemm", "128x128", 128, "gemm 128x128", (1, 9, 9, 264, 200, 1, 1, 0), dict(sel=512, note="Kin = 264: a K tail")),
    # ---- halo (conv_halo.hip): 16-wide and whole-row tiles, partial last tile rows
    ("halo", "C4", 1116, "halo C4 8x16", (1, 16, 16, 72, 64, 3, 1, 1), dict(tie=True)),
    ("halo", "C4", 1116, "halo C4 8x16", (1, 9, 48, 64, 64, 3, 1, 1), dict(
        note="three column tiles, partial last tile row")),
    ("halo", "C4", 1110, "halo C4 12x10", (2, 12, 10, 40, 72, 3, 1, 1), dict()),
    ("halo", "C8", 1016, "halo C8 16x16", (1, 28, 16, 40, 136, 3, 1, 1), dict(sel=512, note="partial last tile row")),
    ("halo", "C8", 1020, "halo C8 12x20", (1, 23, 20, 72, 72, 3, 1, 1), dict(sel=512)),
    # ---- pipelined GEMM (conv_pipe.hip): a persistent grid of 256 workgroups over one or two tiles
    ("pipe", "256x128 C1 TAP", 2000, "pipe 256x128", (1, 9, 128, 128, 128, 3, 2, 1), dict(
        sel=1024, tie=True, note="two channel chunks, 320 pixels")),
    ("pipe", "256x64 C1 TAP", 2001, "pipe 256x64", (1, 9, 128, 128, 64, 3, 2, 1), dict(sel=1024)),
    ("pipe", "256x128 GEN", 2000, "pipe 256x128", (3, 9, 9, 128, 136, 1, 1, 0), dict(
        sel=4096, note="81-pixel maps: the tile spans three images")),
    ("pipe", "256x64 GEN", 2001, "pipe 256x64", (3, 9, 9, 64, 72, 3, 1, 1), dict(sel=4096)),
    ("pipe", "256x128 C1", 2000, "pipe 256x128", (1, 16, 17, 64, 128, 3, 1, 1), dict(sel=1024, note="a partial tile")),
    ("pipe", "256x64 C1", 2001, "pipe 256x64", (2, 17, 16, 128, 72, 1, 1, 0), dict(sel=1024, note="tiles span images")),
    # ---- halo-pipelined (conv_hpipe.hip): 256 workgroups over two to four tiles
    ("hpipe", "128", 4000, "hpipe 16x16px x 128", (1, 16, 32, 64, 136, 3, 1, 1), dict(
        tie=True, note="partial second channel tile")),
    ("hpipe", "128", 4000, "hpipe 16x16px x 128", (2, 16, 16, 128, 128, 3, 1, 1), dict()),
    ("hpipe", "64 wres", 4002, "hpipe 16x16px x 64 wres", (1, 16, 32, 64, 64, 3, 1, 1), dict()),
    # ---- direct (conv_direct.hip): cout at the top of the variant's range and 8 below; 8 workgroups, fewer tasks
    ("direct", "v0", 3000, "direct v0", (1, 9, 11, 32, 64, 3, 2, 1), dict(tie=True, note="30 pixels: one task")),
    ("direct", "v0", 3000, "direct v0", (2, 8, 6, 32, 56, 3, 2, 1), dict()),
    ("direct", "v2", 3002, "direct v2", (1, 7, 9, 32, 32, 3, 1, 1), dict()),
    ("direct", "v2", 3002, "direct v2", (1, 7, 9, 32, 24, 3, 1, 1), dict()),
    ("direct", "v4", 3004, "direct v4", (1, 5, 7, 64, 64, 1, 1, 0), dict(lo=2)),
    ("direct", "v4", 3004, "direct v4", (1, 5, 7, 64, 56, 1, 1, 0), dict(lo=2)),
    ("direct", "v6", 3006, "direct v6", (1, 5, 7, 96, 128, 1, 1, 0), dict(lo=0)),
    ("direct", "v6", 3006, "direct v6", (1, 5, 7, 96, 120, 1, 1, 0), dict(lo=0)),
]


def _cases(family, inst, kid, kname, shape, views, tag="", **kw):
    return [Case(_name(kid, shape, v, tag), family, inst, shape, kid, kname, view=v, **kw) for v in views]


CASES = [c for fam, inst, kid, kname, shape, kw in TABLE
         for c in _cases(fam, inst, kid, kname, shape, V16 if fam == "hpipe" else ALL_VIEWS, **kw)]

# the statistics cap: 73 m-tiles on the 128x32 tile (chosen for ONE image's 37 tiles: select_batch 1), 16 channel
# tiles -> grid_x = 1024 / 16 = 64 rows, so nine rows sum two tiles.  Kin = 8: |v| <= 8 * 14 * 14 = 1568, every value
# an fp16 number (rounds=False) and 9248 * 1568 < 2^24.
CAP_CASES = _cases("gemm", "128x32", 32, "gemm 128x32", (2, 68, 68, 8, 512, 1, 1, 0), ("plain",), "cap", sel=1,
                   lo=-14, hi=14, rounds=False, note="more m-tiles than statistics rows")
# cout % 8 == 4 in a view whose pitch and pointer are 16-byte aligned: the last 16-byte run of a pixel is half cout's,
# half the neighbouring slice's, so these views must store fragments (only the GEMM and the halo kernel take such a
# cout); and cout % 4 != 0: the last channels go out one by one
COUT4_CASES = (
    _cases("gemm", "128x32", 32, "gemm 128x32", (2, 9, 11, 40, 44, 3, 1, 1), ("view4",), "cout4") +
    _cases("gemm", "128x64", 64, "gemm 128x64", (2, 9, 11, 40, 68, 3, 1, 1), ("view4",), "cout4", sel=512) +
    _cases("gemm", "128x128", 128, "gemm 128x128", (2, 9, 11, 40, 132, 3, 1, 1), ("view4",), "cout4", sel=512) +
    _cases("halo", "C4", 1116, "halo C4 8x16", (1, 16, 16, 72, 68, 3, 1, 1), ("view4",), "cout4") +
    _cases("halo", "C8", 1016, "halo C8 16x16", (1, 28, 16, 40, 132, 3, 1, 1), ("view4",), "cout4", sel=512))
TAIL_CASES = (
    _cases("gemm", "128x32", 32, "gemm 128x32", (2, 9, 11, 40, 6, 3, 1, 1), ("view6",), "tail") +
    _cases("halo", "C4", 1116, "halo C4 8x16", (1, 16, 16, 72, 70, 3, 1, 1), ("view6",), "tail"))
# the Detect head's call: a 1x1 conv with bias, fp32 into a slice of a wide row, under the default policy
HEAD_CASES = [c for co in (1, 3, 80) for c in _cases("gemm", "128x32", 32, "gemm 128x32", (2, 9, 11, 64, co, 1, 1, 0),
                                                     ("wide",), "head", default_policy=True)]
# the fp16 clamp, one case per epilogue kind: K = 9 * 32 = 288, |v| = 73 728 at the interior pixels
CLAMP_CASES = (
    _cases("gemm", "128x32", 32, "gemm 128x32", (1, 6, 6, 32, 24, 3, 1, 1), ("plain",), "clamp", note="pk2h") +
    _cases("gemm", "128x32", 32, "gemm 128x32", (1, 6, 6, 32, 6, 3, 1, 1), ("view6",), "clamp", note="pk2h, f2h") +
    _cases("gemm", "128x64", 64, "gemm 128x64", (1, 6, 6, 32, 64, 3, 1, 1), ("plain",), "clamp", sel=2048,
           note="epilogue_regs") +
    _cases("direct", "v0", 3000, "direct v0", (1, 9, 11, 32, 64, 3, 2, 1), ("plain",), "clamp",
           note="epilogue_store"))
CLAMP_KIND = {c.name: c.note for c in CLAMP_CASES}

STAT_CASES = CASES + CAP_CASES + COUT4_CASES + TAIL_CASES          # fp16 z + statistics: runs A and S
ALL_CASES = STAT_CASES + HEAD_CASES + CLAMP_CASES
assert len({c.name for c in ALL_CASES}) == len(ALL_CASES)


def find(kid, view, cout=None, tag="", cases=None):
    """The first case of that kernel id and view (and cout / tag)."""
    for c in (ALL_CASES if cases is None else cases):
        if c.kid == kid and c.view == view and (cout is None or c.cout == cout) and c.name.endswith(tag):
            return c
    raise KeyError((kid, view, cout, tag))


# ---- the other outputs.  A mode is (out_f32, accumulate, bias, operands):
MODES = {
    "bf16": (0, 0, False, "B"),          # overwrite, ties in (256, 512)
    "f32": (1, 0, False, "A"),           # by value
    "bias16": (2, 0, True, "A"),         # fp16(v + bias)
    "biasbf": (0, 0, True, "B"),
    "bias32": (1, 0, True, "A"),
    "acc32": (1, 1, False, "A"),         # old + v exactly
    "accbf": (0, 1, False, "B"),         # E1 or E2 (STORE)
}
# The store paths of the forward, read from the code: (family) -> {path: (modes that take it, bf16 accumulate form)}.
#   16B   conv_epi.h epilogue_regs / epilogue_store: whole 8-channel runs; the accumulate adds the old value to the
#         ROUNDED bf16 (E2).  conv.hip takes it for fp16 without bias on the 64- and 128-channel tiles when y_ld, y_bs,
#         cout are multiples of 8 and y is 16-byte aligned; conv_halo.hip the same for fp16 and bf16; the pipelined,
#         halo-pipelined and direct (v0, v2, v4) kernels always, whatever the alignment.
#   frag  the fragment epilogues of conv.hip, conv_halo.hip and direct v6: 4 channels per lane, pk2h / pk2bf, the
#         accumulate in fp32 (E1); every fp32 output, every bias and every bf16 output of the GEMM goes this way.
#   tail  the scalar stores of cout % 4 != 0 (f2h / f2bf), E1.
STORE = {
    "gemm": {"16B": (("fp16",), None), "frag": (("fp16", "bf16", "f32", "bias", "acc"), "E1"),
             "tail": (("fp16", "bf16", "f32", "bias", "acc"), "E1")},
    "halo": {"16B": (("fp16", "bf16", "acc"), "E2"), "frag": (("fp16", "bf16", "f32", "bias", "acc"), "E1"),
             "tail": (("fp16", "bf16", "bias", "acc"), "E1")},
    "pipe": {"16B": (("fp16", "bf16", "acc"), "E2")},
    "hpipe": {"16B": (("fp16", "bf16", "acc"), "E2")},
    "direct": {"16B": (("fp16",), None), "frag": (("fp16",), None)},
}


def bf16_form(c, bias=False):
    """The accumulate form of case c's bf16 output (STORE)."""
    if c.family in ("pipe", "hpipe"):
        return "E2"
    if c.family == "halo" and c.aligned and not bias:
        return "E2"
    return "E1"


def _other():
    g32, g64, g128 = find(32, "view"), find(64, "view"), find(128, "view")
    out = []
    for c in (g32, g64, g128, find(64, "view8"), find(128, "plain")):
        out += [(c, m) for m in MODES]
    out += [(find(32, "view6", tag="tail"), m) for m in ("bf16", "biasbf", "bias16", "accbf")]
    out += [(find(32, "view4", tag="cout4"), "bias16"), (find(64, "view4", tag="cout4"), "bf16")]
    h4, h4u, h8 = find(1116, "view"), find(1116, "view8"), find(1016, "plain")
    out += [(h4, m) for m in ("bf16", "accbf", "bias16", "f32", "acc32", "bias32")]
    out += [(h4u, m) for m in ("bf16", "accbf", "bias16", "biasbf")]
    out += [(h8, m) for m in ("bf16", "accbf", "bias16")]
    out += [(find(1116, "view6", tag="tail"), m) for m in ("bf16", "accbf", "bias16")]
    for kid in (2000, 2001):
        for c in (c for c in CASES if c.kid == kid and c.view in ("plain", "view8")):
            out += [(c, "bf16"), (c, "accbf")]
    for c in (c for c in CASES if c.family == "hpipe" and c.view in ("plain", "view8p")):
        out += [(c, "bf16"), (c, "accbf")]
    # a conv with bias and a 16-bit output under the policy that selects the pipelined GEMM: the route must skip it
    # (no kernel but conv.hip's and conv_halo.hip's has a bias term)
    for c in (c for c in CASES if c.family == "pipe" and c.view in ("plain", "view8")):
        out += [(c, "bias16")]
    out += [(find(2000, "view"), "biasbf"), (find(4000, "plain"), "bias16"), (find(3000, "plain"), "bias16")]
    out += [(c, m) for c in HEAD_CASES for m in ("bias32", "f32", "acc32")]
    return out


OTHER = _other()
assert len({(c.name, m) for c, m in OTHER}) == len(OTHER)


def other_id(cm):
    return f"{cm[0].name}-{cm[1]}"


def case_id(c):
    return c.name


# ---- descriptor and selection (host side)
def desc(c, n=None, out_f32=2, accumulate=0):
    from yolomi._lib import ConvDesc
    _, h, w, cin, cout, k, s, p = c.shape
    d = ConvDesc()
    d.n, d.h, d.w, d.cin, d.oh, d.ow, d.cout, d.k, d.stride, d.pad = c.n if n is None else n, h, w, cin, c.oh, c.ow, \
        cout, k, s, p
    d.x_bs, d.x_ld, d.y_bs, d.y_ld = c.x_bs, c.x_ld, c.y_bs, c.y_ld
    d.out_f32, d.accumulate = out_f32, accumulate
    return d


policy = D.policy


def kernel(c, d=None):
    """(id, name) of the bias-free forward kernel of case c under its policy."""
    import ctypes
    from yolomi._lib import lib
    d = desc(c) if d is None else d
    name = ctypes.create_string_buffer(96)
    with policy(c):
        kid = lib().ym_conv_kernel(ctypes.byref(d), 0, name, 96)
    return kid, name.value.decode()


def stat_rows(c, d=None):
    import ctypes
    from yolomi._lib import lib
    d = desc(c) if d is None else d
    with policy(c):
        return lib().ym_conv_fwd_stat_rows(ctypes.byref(d))


# ---- operands and reference
def _seed(c):
    return D._seed(c)


@functools.lru_cache(maxsize=None)
def operands(c, run):
    """(x, w) of run "A" (operands in [lo, hi]), "S" ({-1, 0, 1}), "B" ([blo, 4]) or "clamp": x (n, h, w, cin) and
    w (cout, cin, k, k) fp16 integers.  Seeded per case; shared, do not modify."""
    n, h, w, cin, cout, k, s, p = c.shape
    if run == "clamp":
        x = torch.full((n, h, w, cin), 16.0)
        wt = torch.full((cout, cin, k, k), 16.0)
        wt[1::2] = -16.0
        return x.half(), wt.half()
    lo, hi = {"A": (c.lo, c.hi), "S": (-1, 1), "B": (c.blo, 4)}[run]
    g = torch.Generator().manual_seed(_seed(c) ^ {"A": 0, "S": 0x3C3C, "B": 0x6969}[run])
    x = torch.randint(lo, hi + 1, (n, h, w, cin), generator=g)
    wt = torch.randint(lo, hi + 1, (cout, cin, k, k), generator=g)
    return x.half(), wt.half()


def _conv2d(c, run, dtype):
    n, h, w, cin, cout, k, s, p = c.shape
    x, wt = operands(c, run)
    v = torch.nn.functional.conv2d(x.to(dtype).permute(0, 3, 1, 2), wt.to(dtype), stride=s, padding=p)
    return v.permute(0, 2, 3, 1).contiguous()


def exact_bound(c, run):
    """The magnitude no partial sum of the run exceeds; exact while < 2^24."""
    n, h, w, cin, cout, k, s, p = c.shape
    m = {"A": max(abs(c.lo), abs(c.hi)), "S": 1, "B": max(abs(c.blo), 4), "clamp": 16}[run]
    return k * k * cin * m * m


@functools.lru_cache(maxsize=None)
def reference(c, run):
    """v (n, oh, ow, cout) in fp64 by torch conv2d on the same integers; shared, do not modify."""
    v = _conv2d(c, run, torch.float64)
    assert max(abs(c.lo), abs(c.hi), abs(c.blo)) <= 16
    assert bool((v == v.round()).all()), "reference not integral"
    assert exact_bound(c, run) + PREFILL_MAX + 64 < 2 ** 24
    assert float(v.abs().max()) <= exact_bound(c, run)
    return v


def reference_f32(c, run):
    return _conv2d(c, run, torch.float32)


@functools.lru_cache(maxsize=None)
def bias(c):
    """An integer bias in [-64, 64], fp32, at its exact size."""
    g = torch.Generator().manual_seed(_seed(c) ^ 0x1B1B)
    return torch.randint(-64, 65, (c.cout,), generator=g).float()


@functools.lru_cache(maxsize=None)
def prefill(c, out_f32):
    """old (n, oh, ow, cout): integers in [-1000, 1000], through .bfloat16() for a bf16 output."""
    g = torch.Generator().manual_seed(_seed(c) ^ 0x5A5A)
    old = torch.randint(-PREFILL_MAX, PREFILL_MAX + 1, (c.n, c.oh, c.ow, c.cout), generator=g).float()
    return old.bfloat16() if out_f32 == 0 else old


def sq_bound(c):
    """Relative bound of an fp32 sum of n = pixels + 1 non-negative terms in any order (each square rounds once, every
    addition once: gamma_n = n u / (1 - n u), u = 2^-24)."""
    nu = (c.pixels + 1) * 2.0 ** -24
    return nu / (1 - nu)


def bits(t):
    """A tensor's bit patterns as integers of its width."""
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def cast(v, out_f32):
    """fp64 integers below 2^24 -> the output type, round to nearest even (fp32 holds them exactly)."""
    return v.float().to(OUT_DTYPE[out_f32])


def expect_other(c, mode):
    """The expected (n, oh, ow, cout) output of an OTHER entry."""
    out_f32, acc, has_bias, run = MODES[mode]
    v = reference(c, run)
    if has_bias:
        v = v + bias(c).double()
    if not acc:
        return cast(v, out_f32)
    old = prefill(c, out_f32).double()
    if out_f32 == 1:
        return cast(old + v, 1)
    return expect_form(c, bf16_form(c))


def expect_form(c, form):
    """bf16 accumulate of run B onto the prefill: E1 = bf16(old + v), E2 = bf16(bf16(v) + old)."""
    v, old = reference(c, "B").float(), prefill(c, 0).float()
    if form == "E1":
        return (old + v).bfloat16()
    assert form == "E2"
    return (v.bfloat16().float() + old).bfloat16()


def expect_clamp(c):
    return reference(c, "clamp").clamp(-65504, 65504).float().half()


def round_trunc(v):
    """fp64 integers -> fp16 by truncation (what a pk2h without rounding would give)."""
    h = v.float().half()
    over = h.float().abs() > v.float().abs()
    return torch.where(over, (bits(h) - 1).view(torch.float16), h)


def round_half_away(v):
    """fp64 integers -> fp16 rounding halves away from zero."""
    h = v.float().half()
    lo = round_trunc(v)
    hi = (bits(lo) + 1).view(torch.float16)
    tie = (v.float() - lo.float()).abs() == (hi.float() - v.float()).abs()
    return torch.where(tie & (lo.float() != v.float()), hi, h)


# ---- buffers
def sentinel(numel, out_f32=2):
    """Elements outside the y view: position dependent NaNs of varying payload, never a value the kernels produce."""
    s = D.sentinel(numel)                                          # 0x7F81 .. 0x7FFF: NaN as fp16 and as bf16
    return s if out_f32 != 1 else (s.to(torch.int32) << 16) | 0x1234


def x_buffer(c, run):
    """The flat NaN-filled fp16 buffer the x view lives in; the kernel is handed data_ptr() + 2 * c.cx."""
    n, h, w, cin, cout, k, s, p = c.shape
    x, _ = operands(c, run)
    buf = torch.full((n * c.x_bs,), float("nan"), dtype=torch.float16)
    assert c.cx + cin <= c.x_ld and c.x_ld % 8 == 0 and c.x_bs % 8 == 0 and c.cx % 8 == 0
    buf.as_strided((n, h, w, cin), (c.x_bs, w * c.x_ld, c.x_ld, 1), c.cx).copy_(x)
    assert int(torch.isfinite(buf.float()).sum()) == x.numel()
    return buf


def weight_buffer(c, run):
    """The forward weight copy [cout][kh][kw][cin] fp16 at its exact size."""
    _, wt = operands(c, run)
    return wt.permute(0, 2, 3, 1).contiguous().reshape(-1)


def y_view(c, buf):
    """The (n, oh, ow, cout) view of the flat y buffer `buf` the kernel writes."""
    return buf.as_strided((c.n, c.oh, c.ow, c.cout), (c.y_bs, c.ow * c.y_ld, c.y_ld, 1), c.cy)


def y_buffer(c, out_f32=2, fill=None):
    """The flat integer y buffer: sentinels everywhere, `fill` (an (n, oh, ow, cout) tensor of the output type, or
    None for NaN) in the view; the kernel is handed data_ptr() + element size * c.cy."""
    assert c.cy + c.cout <= c.y_ld
    buf = sentinel(c.n * c.y_bs, out_f32)
    if fill is None:
        y_view(c, buf).fill_(0x7FC00000 if out_f32 == 1 else 0x7E00 if out_f32 == 2 else 0x7FC0)
    else:
        assert fill.dtype == OUT_DTYPE[out_f32]
        y_view(c, buf).copy_(bits(fill))
    return buf


def outside_mask(c):
    m = torch.ones(c.n * c.y_bs, dtype=torch.bool)
    y_view(c, m).fill_(False)
    return m


STAT_CANARY = 0x7FA55A5A                                            # a NaN no kernel writes


def stat_buffer(rows, cout):
    """(rows + 1) x cout floats as int32 bits: NaN rows and the canary row after the last."""
    buf = torch.full(((rows + 1) * cout,), 0x7FC00000, dtype=torch.int32)
    buf[rows * cout:] = STAT_CANARY
    return buf


# ---- reporting
def mismatch(c, got, want):
    """None if got == want bit for bit, else a message with the count of mismatches and the first one's (image, y, x,
    channel), got and want.  Both (n, oh, ow, cout) of one type on the CPU."""
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = bits(got) != bits(want)
    count = int(bad.sum())
    if count == 0:
        return None
    img, y, x, ch = (int(v) for v in bad.nonzero()[0])
    g, w_ = got[img, y, x, ch], want[img, y, x, ch]
    mask = 0xFFFF if got.element_size() == 2 else 0xFFFFFFFF
    return (f"{c.name} ({c.kname}, {c.inst}): {count} of {bad.numel()} elements differ; first at (image {img}, y {y}, "
            f"x {x}, channel {ch}): got {float(g)!r} (0x{int(bits(g)) & mask:x}), want {float(w_)!r} "
            f"(0x{int(bits(w_)) & mask:x})")
