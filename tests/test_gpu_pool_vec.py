"""The vector forms of ym_sppf_fwd / ym_sppf_bwd (work items of 8 or 4 channels, misc.hip) and the re-indexed
ym_upsample2_bwd, bit for bit against what they replace.

SPPF: the fused chain against three chained ym_maxpool5_f32_fwd / _bwd launches on the same inputs (the
comparison of test_gpu_model.test_sppf_fused_chain_bit_identical): pool values, argmax codes, fp16 slices, the
fp32 routed gradient and the bf16 slice-0 gradient, compared as bit patterns so that NaN and -0.0 count.  Maps
whose windows clip on every side (1x1, 2x3), just stop clipping (5x5, 6x5), an odd map with 4-channel items only
(9x7 x 12), one / two / three channel groups (20x20 x 8, 16, 24), the 40x40 map, and a batch large enough for the
forward's 8-channel items (32 x 64 channels: 256 blocks); inputs in quarters so that exact ties occur, and NaN,
+inf, -inf, -0.0 planted at a corner, an edge and an interior pixel; gradients with -0.0 and one inf; with and
without accumulate, dx32 and p_out.  The same through views the vector kernels must refuse (a slice pointer one
element off its granule, a row stride that is no multiple of it), which the scalar kernels serve: the result is
the same and nothing outside the slices changes.

Upsample: the comparisons of test_gpu_upsample on one-row, one-column and ragged maps with offset slices, and on
a map with more than 2^16 work items."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 8), (2, 3, 8), (5, 5, 8), (6, 5, 8), (9, 7, 12), (20, 20, 8), (20, 20, 16), (20, 20, 24), (40, 40, 4)]
SPECIALS = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf"), "-0": -0.0}
# (extra elements per concat row, offset of slice 0 in the row)
LAYOUTS = {"dense": (0, 0), "offset1": (8, 1), "stride": (2, 0)}


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def same(a, b):
    return torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def reference(H, W, C, B, special):
    """Inputs and the chained per-pool results (dense views), computed once per case and never modified."""
    from yolomi._lib import call, stream_ptr
    g = torch.Generator().manual_seed(H * 1000 + W * 10 + C + B)
    M = B * H * W
    x = torch.randint(-8, 8, (B, H, W, C), generator=g).float() / 4      # exact ties, as chained pools make
    grad = torch.randn(B, H, W, 4 * C, generator=g).bfloat16()
    if special is not None:
        for i, (h, w) in enumerate([(0, 0), (0, W // 2), (H // 2, W // 2)]):   # corner, edge, interior
            x[0, h, w, i % C] = SPECIALS[special]
            x[B - 1, h, w, :] = SPECIALS[special]
        grad[0, 0, 0, C:] = -0.0
        grad[B - 1, H // 2, W // 2, C + 1::C] = -0.0
        grad[0, H // 2, W // 2, 3 * C + 2] = float("inf")
    x = x.reshape(M, C).cuda()
    grad = grad.cuda()
    st = stream_ptr()
    bs, ld = H * W * 4 * C, 4 * C
    sl = lambda t, j: t.data_ptr() + 2 * j * C
    P = torch.zeros(4, M, C, device="cuda")
    P[0] = x
    code = torch.zeros(3, M, C, dtype=torch.uint8, device="cuda")
    ybuf = torch.zeros(B, H, W, 4 * C, dtype=torch.float16, device="cuda")
    for j in range(3):
        call("ym_maxpool5_f32_fwd", P[j].data_ptr(), P[j + 1].data_ptr(), code[j].data_ptr(), sl(ybuf, j + 1), bs, ld,
             B, H, W, C, st)
    cur = grad[..., 3 * C:].float().reshape(M, C).contiguous()
    for j in (2, 1):
        nxt = torch.empty(M, C, device="cuda")
        call("ym_maxpool5_f32_bwd", code[j].data_ptr(), cur.data_ptr(), sl(grad, j), bs, ld, nxt.data_ptr(), None, 0,
             0, 0, B, H, W, C, st)
        cur = nxt
    dx, gout = torch.empty(M, C, device="cuda"), {}
    for acc in (0, 1):
        gout[acc] = grad.clone()
        call("ym_maxpool5_f32_bwd", code[0].data_ptr(), cur.data_ptr(), None, 0, 0, dx.data_ptr(), gout[acc].data_ptr(),
             bs, ld, acc, B, H, W, C, st)
    torch.cuda.synchronize()
    return {"x": x, "grad": grad, "P": P[1:], "code": code, "y": ybuf[..., C:], "dx": dx, "gout": gout}


def check_fused(H, W, C, B, special=None, layout="dense"):
    from yolomi._lib import call, lib, stream_ptr
    assert lib().ym_sppf_supported(H, W, C)
    ref = reference(H, W, C, B, special)
    pad, off = LAYOUTS[layout]
    M, st = B * H * W, stream_ptr()
    ld = 4 * C + pad
    bs = H * W * ld
    sl = lambda t, j: t.data_ptr() + 2 * (off + j * C)
    inside = lambda t: t[..., off:off + 4 * C]
    outside = lambda t: torch.cat([t[..., :off], t[..., off + 4 * C:]], dim=-1)
    for with_p in (True, False):
        P = torch.full((3, M, C), 3.0, device="cuda")
        code = torch.full((3, M, C), 99, dtype=torch.uint8, device="cuda")
        ybuf = torch.full((B, H, W, ld), 7.0, dtype=torch.float16, device="cuda")
        call("ym_sppf_fwd", ref["x"].data_ptr(), code.data_ptr(), sl(ybuf, 1), sl(ybuf, 2), sl(ybuf, 3), bs, ld,
             P.data_ptr() if with_p else None, B, H, W, C, st)
        torch.cuda.synchronize()
        assert same(code, ref["code"])
        assert same(inside(ybuf)[..., C:], ref["y"])
        assert bool((inside(ybuf)[..., :C] == 7.0).all()) and bool((outside(ybuf) == 7.0).all())
        assert same(P, ref["P"]) if with_p else bool((P == 3.0).all())
    for acc in (0, 1):
        for with_dx in (True, False):
            gbuf = torch.full((B, H, W, ld), 5.0, dtype=torch.bfloat16, device="cuda")
            inside(gbuf).copy_(ref["grad"])
            dx32 = torch.full((M, C), 3.0, device="cuda")
            call("ym_sppf_bwd", ref["code"].data_ptr(), sl(gbuf, 1), sl(gbuf, 2), sl(gbuf, 3), bs, ld, sl(gbuf, 0), bs, ld,
                 acc, dx32.data_ptr() if with_dx else None, B, H, W, C, st)
            torch.cuda.synchronize()
            assert same(inside(gbuf), ref["gout"][acc])
            assert bool((outside(gbuf) == 5.0).all())
            assert same(dx32, ref["dx"]) if with_dx else bool((dx32 == 3.0).all())


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W,C", SHAPES)
def test_sppf_vec_bit_identical(H, W, C, B):
    check_fused(H, W, C, B)


def test_sppf_vec_eight_channel_forward_items():
    """32 images x 64 channels: 256 blocks of 8 channels, the forward's wide items (fewer blocks run 4-channel ones)."""
    check_fused(6, 5, 64, 32)
    check_fused(6, 5, 64, 32, special="nan")


@pytest.mark.parametrize("special", list(SPECIALS))
@pytest.mark.parametrize("H,W,C,B", [(6, 5, 8, 1), (9, 7, 12, 3), (20, 20, 16, 3)])
def test_sppf_vec_special_values(H, W, C, B, special):
    check_fused(H, W, C, B, special=special)


@pytest.mark.parametrize("layout", ["offset1", "stride"])
@pytest.mark.parametrize("H,W,C,B", [(2, 3, 8, 1), (9, 7, 12, 3), (20, 20, 16, 3), (6, 5, 64, 32)])
def test_sppf_unaligned_views_take_the_scalar_kernels(H, W, C, B, layout):
    check_fused(H, W, C, B, layout=layout)
    check_fused(H, W, C, B, special="-0", layout=layout)


UPSAMPLE = [  # (n, h, w, c, x channels, x offset, y channels, y offset)
    (1, 1, 7, 8, 8, 0, 8, 0),
    (2, 5, 1, 16, 16, 0, 16, 0),
    (3, 13, 11, 40, 56, 8, 72, 16),        # ragged map, offset slices on both sides
    (1, 300, 300, 8, 8, 0, 8, 0),          # 90000 work items: past 16 bits, 1.4 MB of gradient
]


@pytest.mark.parametrize("n,h,w,c,xc,xo,yc,yo", UPSAMPLE)
@pytest.mark.parametrize("accumulate", [0, 1])
def test_upsample2_reindexed_bit_exact(n, h, w, c, xc, xo, yc, yo, accumulate):
    import test_gpu_upsample as up
    up.test_upsample2_fwd_bwd_bit_exact(n, h, w, c, xc, xo, yc, yo, accumulate)
