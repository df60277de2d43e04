"""Cases, integer operands and the fp64 reference of the exact weight-gradient tests (csrc/wgrad.hip, ym_conv_wgrad).
Plain torch and ctypes descriptors, no GPU needed: tests/test_wgrad_exact_cpu.py keeps this file honest (the reference
meets the exactness condition by itself; ids, split counts and unit parities against the library's host entry points),
tests/test_gpu_wgrad_exact.py holds every kernel instance to it bit for bit.

Why the comparison is exact.  dz (bf16) and x (fp16) hold integers in [-4, 4].  Every product is an integer of
magnitude <= 16, every fp32 MFMA accumulation, split partial, reduce and accumulate-into-dw add is a sum of such
integers, and any partial sum is bounded by 16 * M (+ the prefill of an accumulate run), M = n * oh * ow output pixels.
While that bound is below 2^24 every intermediate is an integer fp32 represents exactly, so the summation order stops
mattering and the kernel must equal the integer result by value: one dropped, doubled or misplaced term shows, at any
size.  `exact_bound` is that condition — a condition of the test, not a tolerance.

Views.  x lives in a buffer of cin + xe channels at channel offset cx, dz in one of cout + ye channels at offset cy
(the network's C3k2 concat slices: x_ld > cin, y_ld > cout, a view pointer that is not the start of a buffer; offsets
and extras are multiples of 8, as the ABI requires).  Every other element of both buffers is NaN: the kernels stage
8-channel chunks below Cin / Cout only, so any over-read poisons the result.

Rounding pin.  The kernels convert x fp16 -> bf16 at staging (h8_to_bf8).  A pin case scatters +-257 and +-259 into x:
exact in fp16, not representable in bf16 (8 significand bits: spacing 2 above 256), both ties — round-to-nearest-even
sends 257 to 256 and 259 to 260, truncation gets 259 wrong (258), round-half-away gets 257 wrong (258).  The reference
rounds x with torch's .bfloat16() first; the bound is then 4 * 260 * M < 2^24 (M < 8192 there).

Unit geometry (the K units a split-K workgroup steps over; wgrad.hip's plan): wgrad3 8x8 output-pixel blocks per
image, or whole rows on 20-wide (20 x 3) and 10-wide (10 x 6) maps with 64x64 channel tiles; wgrad1 64-pixel stages of
the flat pixel axis; chunk = ceil(units / splits) units per split, the last split takes the rest.
"""
import ctypes
import functools
import zlib
from dataclasses import dataclass

import torch

# every weight-gradient kernel instance ym_conv_wgrad can launch: id -> name (ym_conv_kernel(d, 2))
INSTANCES = {
    13002: "wgrad3 s1 64x64 8x8 db", 13003: "wgrad3 s1 64x64 8x8 deep db",
    13102: "wgrad3 s1 32x64 8x8 db", 13103: "wgrad3 s1 32x64 8x8 deep db",
    13202: "wgrad3 s1 64x32 8x8 db", 13203: "wgrad3 s1 64x32 8x8 deep db",
    13302: "wgrad3 s1 32x32 8x8 db", 13303: "wgrad3 s1 32x32 8x8 deep db",
    13012: "wgrad3 s1 64x64 20x3 db", 13022: "wgrad3 s1 64x64 10x6 db",
    13500: "wgrad3 s2 64x64 8x8", 13503: "wgrad3 s2 64x64 8x8 deep db",
    13600: "wgrad3 s2 32x64 8x8", 13603: "wgrad3 s2 32x64 8x8 deep db",
    13700: "wgrad3 s2 64x32 8x8", 13703: "wgrad3 s2 64x32 8x8 deep db",
    13800: "wgrad3 s2 32x32 8x8", 13803: "wgrad3 s2 32x32 8x8 deep db",
    13510: "wgrad3 s2 64x64 20x3", 13520: "wgrad3 s2 64x64 10x6",
    11064: "wgrad1 64", 11128: "wgrad1 128",
    10064: "wgrad generic 64", 10128: "wgrad generic 128",
}
DEEP_IDS = (13003, 13103, 13203, 13303, 13503, 13603, 13703, 13803)
PAIRED_IDS = DEEP_IDS + (11064, 11128)          # kernels whose K loop takes units in pairs

PREFILL_MAX = 1000                               # |dw prefill| of the accumulate run
VIEW = dict(xe=16, ye=24, cx=8, cy=16)           # the channel-slice view of the "view" cases: NaN channels on both sides


@dataclass(frozen=True)
class Case:
    name: str
    shape: tuple                 # n, h, w, cin, cout, k, stride, pad
    kid: int                     # expected ym_conv_kernel(d, 2)
    xe: int = 0                  # channels of the x buffer beyond cin
    ye: int = 0                  # channels of the dz buffer beyond cout
    cx: int = 0                  # channel offset of x in its buffer
    cy: int = 0                  # channel offset of dz in its buffer
    x_gap: int = 0               # x_bs = h * w * x_ld + x_gap: a batch-strided (non-whole) view
    pin: bool = False            # rounding pin: +-257 / +-259 scattered into x
    target: int = 0              # ym_wgrad_set_target for this case (0: default)
    splits: int = 0              # expected split count (0: not pinned)
    chunk: int = 0               # expected units per split (0: not pinned)
    tail: int = 0                # expected units of the last split (0: not pinned)
    xcd: int = -1                # 1 / 0: the split count is / is not a multiple of 8 (wg_tile's xcd_map), as intended
    units: str = ""              # "odd" / "even" / "single": the per-split unit counts this case is there for

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
    def m(self):
        return self.n * self.oh * self.ow

    @property
    def x_ld(self):
        return self.shape[3] + self.xe

    @property
    def y_ld(self):
        return self.shape[4] + self.ye

    @property
    def x_bs(self):
        return self.shape[1] * self.shape[2] * self.x_ld + self.x_gap

    @property
    def y_bs(self):
        return self.oh * self.ow * self.y_ld

    @property
    def elems(self):
        n, h, w, cin, cout, k, s, p = self.shape
        return cout * cin * k * k

    @property
    def viewed(self):
        return bool(self.xe and self.ye and self.cx and self.cy)


def _name(kid, shape, tag):
    n, h, w, cin, cout, k, s, p = shape
    return f"{kid}-n{n}h{h}w{w}c{cin}o{cout}k{k}s{s}p{p}-{tag}"


def _both(kid, shape, **kw):
    """An instance's shape as a whole contiguous tensor and as a channel-slice view."""
    return [Case(_name(kid, shape, "plain"), shape, kid, **kw),
            Case(_name(kid, shape, "view"), shape, kid, **VIEW, **kw)]


def _one(kid, shape, tag, view=False, **kw):
    return Case(_name(kid, shape, tag), shape, kid, **(VIEW if view else {}), **kw)


# ---- one or more shapes per instance: odd maps (partial 8x8 units, partial row units, halo rows in the padding),
# stride 2 on odd and even inputs, channel counts that leave a partial tile (72, 40, 136, 24), 96 padded into 128
TABLE = [
    (13002, (2, 13, 11, 64, 72, 3, 1, 1)),
    (13003, (1, 9, 64, 40, 64, 3, 1, 1)),
    (13102, (2, 9, 7, 64, 32, 3, 1, 1)),
    (13103, (1, 9, 64, 64, 32, 3, 1, 1)),
    (13202, (2, 8, 9, 32, 64, 3, 1, 1)),
    (13203, (1, 9, 66, 32, 72, 3, 1, 1)),
    (13302, (1, 10, 10, 8, 16, 3, 1, 1)),
    (13303, (1, 9, 65, 24, 32, 3, 1, 1)),
    (13012, (3, 7, 20, 64, 72, 3, 1, 1)),
    (13022, (2, 13, 10, 72, 64, 3, 1, 1)),
    (13500, (2, 17, 17, 64, 72, 3, 2, 1)),
    (13503, (1, 17, 129, 64, 72, 3, 2, 1)),
    (13600, (2, 17, 19, 64, 32, 3, 2, 1)),
    (13603, (1, 17, 128, 72, 32, 3, 2, 1)),
    (13700, (2, 17, 19, 32, 64, 3, 2, 1)),
    (13703, (1, 17, 130, 32, 64, 3, 2, 1)),
    (13800, (2, 11, 11, 16, 32, 3, 2, 1)),
    (13803, (1, 17, 127, 16, 24, 3, 2, 1)),
    (13510, (2, 14, 39, 72, 64, 3, 2, 1)),
    (13520, (2, 25, 19, 64, 72, 3, 2, 1)),
    (11064, (3, 7, 9, 72, 40, 1, 1, 0)),
    (11128, (2, 9, 15, 96, 136, 1, 1, 0)),
    (10064, (1, 7, 5, 48, 40, 1, 2, 0)),
    (10064, (1, 7, 9, 16, 24, 3, 1, 0)),        # 3x3 without padding
    (10064, (1, 9, 9, 24, 16, 2, 1, 0)),        # k = 2
    (10128, (1, 9, 9, 128, 136, 1, 2, 0)),
]

INSTANCE_CASES = [c for kid, shape in TABLE for c in _both(kid, shape)]
# the wgrad1 64 shape through a batch-strided view (x_bs past one whole image): not "whole", so the generic kernel
INSTANCE_CASES += _both(10064, (3, 7, 9, 72, 40, 1, 1, 0), x_gap=64)

# ---- paired-unit loops (the deep wgrad3 instances and both wgrad1 tiles take units two at a time; an odd count
# multiplies one unit of zeros): a split with an odd count, splits with even counts only, a split of exactly one unit
UNIT_CASES = [
    # s1 deep: units = n * ceil(oh / 8) * ceil(ow / 8)
    _one(13003, (1, 8, 72, 64, 64, 3, 1, 1), "odd", units="odd"),
    _one(13003, (1, 9, 64, 64, 72, 3, 1, 1), "even", True, units="even"),
    _one(13003, (3, 8, 152, 64, 64, 3, 1, 1), "single", True, units="single"),
    _one(13103, (1, 8, 72, 64, 32, 3, 1, 1), "odd", True, units="odd"),
    _one(13103, (1, 12, 64, 72, 32, 3, 1, 1), "even", units="even"),
    _one(13203, (1, 8, 72, 32, 64, 3, 1, 1), "odd", units="odd"),
    _one(13203, (1, 12, 64, 32, 72, 3, 1, 1), "even", True, units="even"),
    _one(13303, (1, 8, 72, 32, 32, 3, 1, 1), "odd", True, units="odd"),
    _one(13303, (1, 12, 64, 16, 24, 3, 1, 1), "even", units="even"),
    # s2 deep
    _one(13503, (1, 15, 143, 64, 64, 3, 2, 1), "odd", True, units="odd"),
    _one(13503, (1, 17, 128, 64, 64, 3, 2, 1), "even", units="even"),
    _one(13603, (1, 15, 143, 64, 32, 3, 2, 1), "odd", units="odd"),
    _one(13603, (1, 18, 130, 72, 32, 3, 2, 1), "even", True, units="even"),
    _one(13703, (1, 15, 143, 32, 64, 3, 2, 1), "odd", True, units="odd"),
    _one(13703, (1, 18, 128, 32, 72, 3, 2, 1), "even", units="even"),
    _one(13803, (1, 15, 143, 32, 32, 3, 2, 1), "odd", units="odd"),
    _one(13803, (1, 18, 128, 16, 24, 3, 2, 1), "even", True, units="even"),
    # wgrad1: units = ceil(M / 64)
    _one(11064, (1, 7, 9, 64, 64, 1, 1, 0), "single", True, units="single"),
    _one(11064, (2, 9, 14, 72, 40, 1, 1, 0), "even", units="even"),
    _one(11064, (3, 9, 7, 40, 72, 1, 1, 0), "odd", True, units="odd"),
    _one(11128, (1, 8, 8, 128, 128, 1, 1, 0), "single", units="single"),
    _one(11128, (2, 9, 14, 96, 136, 1, 1, 0), "even", True, units="even"),
    _one(11128, (3, 9, 11, 136, 96, 1, 1, 0), "odd", units="odd"),
]

# ---- the staging conversion fp16 -> bf16, one case per kernel family
PIN_CASES = [
    _one(13002, (2, 13, 11, 64, 72, 3, 1, 1), "pin", True, pin=True),
    _one(11064, (3, 7, 9, 72, 40, 1, 1, 0), "pin", True, pin=True),
    _one(10064, (1, 7, 9, 16, 24, 3, 1, 0), "pin", True, pin=True),
]

# ---- split scenarios: the XCD-mapped block order of wg_tile (split count a multiple of 8) and the plain one, short
# last splits, several channel tiles per split, the reduce kernel's 16-wide unrolled loop and its remainder, the setter
SPLIT_CASES = [
    _one(13002, (2, 64, 48, 64, 64, 3, 1, 1), "xcd16", splits=16, xcd=1),
    _one(13002, (2, 64, 48, 64, 64, 3, 1, 1), "target4", True, target=4, splits=8, xcd=1),
    _one(13002, (2, 64, 48, 64, 64, 3, 1, 1), "target2", target=2, splits=4, xcd=0),
    _one(13002, (4, 40, 40, 64, 64, 3, 1, 1), "plain15", True, splits=15, chunk=7, tail=2, xcd=0),
    _one(13002, (2, 48, 40, 64, 64, 3, 1, 1), "xcd8tail", splits=8, chunk=8, tail=4, xcd=1),
    _one(13002, (3, 32, 32, 128, 72, 3, 1, 1), "tiles2x2", True, splits=8, xcd=1),
    _one(13003, (3, 64, 64, 64, 64, 3, 1, 1), "reduce32", splits=32, xcd=1),
    _one(13003, (24, 64, 64, 64, 64, 3, 1, 1), "reduce128", True, splits=128, xcd=1),
    _one(13503, (4, 33, 129, 64, 64, 3, 2, 1), "s2tail", splits=8, chunk=14, tail=10, xcd=1),
    _one(11064, (6, 33, 31, 64, 64, 1, 1, 0), "xcd8", True, splits=8, xcd=1),
    _one(11128, (2, 40, 41, 128, 136, 1, 1, 0), "plain6", splits=6, chunk=9, tail=7, xcd=0),
    _one(11064, (4, 64, 64, 64, 64, 1, 1, 0), "xcd32", True, splits=32, xcd=1),
    _one(11064, (4, 64, 64, 64, 64, 1, 1, 0), "target8", target=8, splits=8, xcd=1),
]

CASES = INSTANCE_CASES + UNIT_CASES + PIN_CASES + SPLIT_CASES
assert len({c.name for c in CASES}) == len(CASES)


def case_id(c):
    return c.name


# ---- descriptor and plan (host side)
def desc(c, n=None):
    """The ym_conv_desc of case c (of n images instead of c.n if given)."""
    from yolomi._lib import ConvDesc
    _, h, w, cin, cout, k, s, p = c.shape
    d = ConvDesc()
    d.n, d.h, d.w, d.cin, d.oh, d.ow, d.cout, d.k, d.stride, d.pad = c.n if n is None else n, h, w, cin, c.oh, c.ow, \
        cout, k, s, p
    d.x_bs, d.x_ld, d.y_bs, d.y_ld = c.x_bs, c.x_ld, c.y_bs, c.y_ld
    d.out_f32, d.accumulate = 1, 0
    return d


class wgrad_target:
    """with wgrad_target(c): the library plans under c.target (ym_wgrad_set_target), restored on the way out."""

    def __init__(self, c):
        self.target = c.target

    def __enter__(self):
        from yolomi._lib import lib
        self.prev = lib().ym_wgrad_set_target(self.target) if self.target else None

    def __exit__(self, *exc):
        from yolomi._lib import lib
        if self.prev is not None:
            lib().ym_wgrad_set_target(self.prev)


def kernel_id(c):
    from yolomi._lib import lib
    d = desc(c)
    with wgrad_target(c):
        return lib().ym_conv_kernel(ctypes.byref(d), 2, None, 0)


def workspace_bytes(c):
    from yolomi._lib import lib
    d = desc(c)
    with wgrad_target(c):
        return lib().ym_conv_wgrad_workspace_size(ctypes.byref(d))


def unit_count(c):
    """K units of the case, from the documented unit geometry of its instance (None for the generic kernels, which
    reduce through atomics into one partial)."""
    fam = c.kid // 1000
    if fam == 13:
        row = (c.kid // 10) % 10                      # 1: 20 x 3 whole-row units, 2: 10 x 6, 0: 8 x 8
        tw, th = {0: (8, 8), 1: (20, 3), 2: (10, 6)}[row]
        return c.n * -(-c.oh // th) * -(-c.ow // tw)
    if fam == 11:
        return -(-c.m // 64)
    return None


def split_plan(c):
    """(splits, chunk, per-split unit counts) of the case: splits from the workspace size, chunk = ceil(units / splits)."""
    assert c.kid // 1000 != 10
    ws = workspace_bytes(c)
    assert ws % (4 * c.elems) == 0, (ws, c.elems)
    splits = ws // (4 * c.elems)
    units = unit_count(c)
    chunk = -(-units // splits)
    counts = [min(chunk, units - s * chunk) for s in range(splits)]
    return splits, chunk, counts


def tile_of(c, co, ci):
    """(co tile, ci tile) of a weight element under the case's instance: a failure names the workgroup's tile."""
    n, h, w, cin, cout, k, s, p = c.shape
    if c.kid // 1000 == 13:
        tc = (c.kid - 13000) % 500 // 100                # bit 0: 32-co tile, bit 1: 32-ci tile
        return co // (32 if tc & 1 else 64), ci // (32 if tc & 2 else 64)
    t = c.kid % 1000
    return co // t, ci // t


# ---- operands and reference
def _seed(c):
    return zlib.crc32(c.name.encode()) & 0x7FFFFFFF


@functools.lru_cache(maxsize=None)
def operands(c):
    """(x, dz): x (n, h, w, cin) fp16 and dz (n, oh, ow, cout) bf16, integers in [-4, 4] (a pin case: +-257 / +-259 on
    about one x element in 16).  Seeded per case; shared, do not modify."""
    n, h, w, cin, cout, k, s, p = c.shape
    g = torch.Generator().manual_seed(_seed(c))
    x = torch.randint(-4, 5, (n, h, w, cin), generator=g).to(torch.float16)
    dz = torch.randint(-4, 5, (n, c.oh, c.ow, cout), generator=g).to(torch.bfloat16)
    if c.pin:
        ties = torch.tensor([257.0, -257.0, 259.0, -259.0], dtype=torch.float16)
        where = torch.randperm(x.numel(), generator=g)[:max(x.numel() // 16, 64)]
        x.view(-1)[where] = ties[torch.arange(where.numel()) % 4]
        assert all(bool((x == t).any()) for t in ties)
        assert bool((x.float() == ties.float()[0]).any())            # 257 survives fp16
    return x, dz


def buffers(c):
    """(xbuf, dzbuf): the flat NaN-filled buffers the views of x and dz live in; the kernel is handed
    xbuf.data_ptr() + 2 * c.cx and dzbuf.data_ptr() + 2 * c.cy with the strides of desc(c)."""
    n, h, w, cin, cout, k, s, p = c.shape
    x, dz = operands(c)
    xbuf = torch.full((n * c.x_bs,), float("nan"), dtype=torch.float16)
    xbuf.as_strided((n, h, w, cin), (c.x_bs, w * c.x_ld, c.x_ld, 1), c.cx).copy_(x)
    dzbuf = torch.full((n * c.y_bs,), float("nan"), dtype=torch.bfloat16)
    dzbuf.as_strided((n, c.oh, c.ow, cout), (c.y_bs, c.ow * c.y_ld, c.y_ld, 1), c.cy).copy_(dz)
    assert c.cx + cin <= c.x_ld and c.cy + cout <= c.y_ld
    assert int(torch.isfinite(xbuf.float()).sum()) == x.numel() and int(torch.isfinite(dzbuf.float()).sum()) == dz.numel()
    return xbuf, dzbuf


def term_max(c):
    """Largest |dz * x| of the case."""
    return 4 * 260 if c.pin else 16


def exact_bound(c, prefill=0):
    """The magnitude no partial sum of the case exceeds; the comparison is exact while it is < 2^24."""
    return term_max(c) * c.m + prefill


def _conv2d_weight(c, dtype):
    n, h, w, cin, cout, k, s, p = c.shape
    x, dz = operands(c)
    xr = x.bfloat16() if c.pin else x                   # the staging conversion (exact on the integers in [-4, 4])
    return torch.nn.grad.conv2d_weight(xr.to(dtype).permute(0, 3, 1, 2), (cout, cin, k, k),
                                       dz.to(dtype).permute(0, 3, 1, 2), stride=s, padding=p)


@functools.lru_cache(maxsize=None)
def reference(c):
    """dW (cout, cin, k, k) in fp64 by torch.nn.grad.conv2d_weight on the same integers; shared, do not modify."""
    ref = _conv2d_weight(c, torch.float64)
    assert bool((ref == ref.round()).all()), "reference not integral"
    assert exact_bound(c, PREFILL_MAX) < 2 ** 24, (c.name, exact_bound(c, PREFILL_MAX))
    assert float(ref.abs().max()) <= exact_bound(c)
    return ref


def reference_f32(c):
    return _conv2d_weight(c, torch.float32)


def prefill(c):
    """Known integers (|v| <= PREFILL_MAX) the accumulate run adds onto, (cout, cin, k, k) fp32."""
    n, h, w, cin, cout, k, s, p = c.shape
    g = torch.Generator().manual_seed(_seed(c) ^ 0x5A5A)
    return torch.randint(-PREFILL_MAX, PREFILL_MAX + 1, (cout, cin, k, k), generator=g).float()


def mismatch(c, got, want):
    """None if got == want by value everywhere, else a message with the count of mismatches and the first one's
    (co, ci, kh, kw), channel tile and got / want values.  got fp32 (cout, cin, k, k) on the CPU, want fp64."""
    got = got.double()
    bad = ~(got == want)                                # a NaN in got is a mismatch
    count = int(bad.sum())
    if count == 0:
        return None
    co, ci, kh, kw = (int(v) for v in bad.nonzero()[0])
    cot, cit = tile_of(c, co, ci)
    return (f"{c.name} ({INSTANCES[c.kid]}): {count} of {bad.numel()} elements differ; first at (co {co}, ci {ci}, "
            f"kh {kh}, kw {kw}), channel tile (co {cot}, ci {cit}): got {float(got[co, ci, kh, kw])!r}, want "
            f"{float(want[co, ci, kh, kw])!r}")
