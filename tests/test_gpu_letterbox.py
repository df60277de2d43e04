"""ym_letterbox_u8c and ym_unletterbox_boxes on the GPU, bit for bit against the numpy restatement
(tests/letterbox_ref.py) over the case list the sanitized host build is held to (tests/test_letterbox_cpu.py): three
frames (one of odd area, one not square), `out` off the 16-byte grid, 1-4 planes, three fills, a batch whose left / top
differ per image, square sources against ym_resize_linear_u8c, the argument checks, and the Python layers above them."""
import numpy as np
import pytest
import torch

import augment_ref as AR
import letterbox_ref as LR

pytestmark = pytest.mark.gpu

FRAMES = [(32, 32), (31, 31), (32, 48)]


def _dev(ims):
    buf, meta = AR.pack(ims)
    if buf.size == 0:
        buf = np.zeros(1, np.uint8)
    return torch.from_numpy(buf).cuda(), torch.from_numpy(meta).cuda()


def _table_dev(table, n):
    from datasets.letterbox import table_bytes
    return table_bytes(table, n).cuda()


def _out(B, ch, H, W, offset):
    flat = torch.full((B * ch * H * W + 1,), -1.0, dtype=torch.float32, device="cuda")
    out = flat[1:] if offset else flat[:-1]
    assert out.data_ptr() % 16 == (4 if offset else 0)
    return out.view(B, ch, H, W)


def _letterbox(table, ims, H, W, fill=114, offset=False):
    from yolomi._lib import call, stream_ptr
    ch, B = ims[0].shape[2], len(ims)
    u8, meta = _dev(ims)
    out = _out(B, ch, H, W, offset)
    tdev = _table_dev(table, B)                            # named: alive until the launch has run
    call("ym_letterbox_u8c", u8.data_ptr(), meta.data_ptr(), tdev.data_ptr(), B, ch, H, W, fill, out.data_ptr(),
         stream_ptr(u8.device))
    return out.cpu().numpy()


def _check_exact(got, want_u8, names):
    want = LR.as_float(want_u8)
    for k, name in enumerate(names):
        assert np.array_equal(got[k], want[k]), (name, int((got[k] != want[k]).sum()))
        assert np.array_equal(np.rint(got[k] * 255.0).astype(np.int64), want_u8[k]), name


@pytest.mark.parametrize("H,W", FRAMES)
@pytest.mark.parametrize("ch", [1, 2, 3, 4])
def test_letterbox_equals_restatement(H, W, ch):
    """The whole case list in one batch: left / top, the copy, the empty image and the scale-up flag differ per image."""
    ims = LR.sources(H, W, ch)
    table = LR.entries(ims, H, W, LR.SCALEUP)
    assert len({(e.left, e.top) for e in table}) >= 5
    for fill in (0, 114, 255):
        _check_exact(_letterbox(table, ims, H, W, fill), LR.render(table, ims, H, W, fill), LR.SOURCE_SIZES)


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_out_offset_by_four_bytes(ch):
    """`out` not 16-byte aligned at a size whose groups would otherwise be vector stores; nothing written outside."""
    from yolomi._lib import call, stream_ptr
    H, W = 32, 48
    ims = LR.sources(H, W, ch)
    table = LR.entries(ims, H, W, LR.SCALEUP)
    assert np.array_equal(_letterbox(table, ims, H, W, offset=True), _letterbox(table, ims, H, W))
    u8, meta = _dev(ims)
    B = len(ims)
    flat = torch.full((B * ch * H * W + 8,), -1.0, dtype=torch.float32, device="cuda")
    tdev = _table_dev(table, B)
    call("ym_letterbox_u8c", u8.data_ptr(), meta.data_ptr(), tdev.data_ptr(), B, ch, H, W, 114, flat[1:].data_ptr(),
         stream_ptr(u8.device))
    assert float(flat[0]) == -1.0 and (flat[-7:] == -1.0).all() and (flat[1:-7] >= 0.0).all()


@pytest.mark.parametrize("S", [32, 31])
@pytest.mark.parametrize("ch", [1, 3])
def test_square_sources_equal_the_stretch_kernel(S, ch):
    from yolomi._lib import call, stream_ptr
    rng = np.random.default_rng(S + ch)
    ims = [rng.integers(0, 256, (n, n, ch), dtype=np.uint8) for n in (1, 5, S, 33, 64)]
    table = LR.entries(ims, S, S)
    assert all((e.nw, e.nh, e.left, e.top) == (S, S, 0, 0) for e in table)
    u8, meta = _dev(ims)
    want = _out(len(ims), ch, S, S, False)
    call("ym_resize_linear_u8c", u8.data_ptr(), meta.data_ptr(), len(ims), ch, S, want.data_ptr(),
         stream_ptr(u8.device))
    assert np.array_equal(_letterbox(table, ims, S, S), want.cpu().numpy())


def test_mismatched_entry_and_interior_over_the_edge():
    H = W = 32
    ims = LR.sources(H, W, 3)[1:4]
    table = LR.entries(ims, H, W)
    table[0].w0 += 1                                       # not the image's size: all fill, no source byte read
    table[1].left, table[1].top = -5, 20
    table[2].left = W - 3
    _check_exact(_letterbox(table, ims, H, W, 9), LR.render(table, ims, H, W, 9), ["mismatch", "negative", "right"])


def test_unletterbox_boxes_equals_restatement():
    from yolomi._lib import call, stream_ptr
    H = W = 32
    boxes, counts, sizes = LR.box_cases()
    table = LR.entries([np.zeros((*hw, 1), np.uint8) for hw in sizes], H, W)
    assert (table[1].left, table[2].top) == (4, 8)
    B, N = boxes.shape[:2]
    sentinel = np.full_like(boxes, -7.0)
    out = torch.from_numpy(sentinel).cuda()
    inp, cnt, tdev = torch.from_numpy(boxes).cuda(), torch.from_numpy(counts).cuda(), _table_dev(table, B)
    call("ym_unletterbox_boxes", inp.data_ptr(), cnt.data_ptr(), tdev.data_ptr(), B, N, H, W, out.data_ptr(),
         stream_ptr(out.device))
    got = out.cpu().numpy()
    want = LR.unletterbox(boxes, counts, table, H, W, out=sentinel)
    assert got.tobytes() == want.tobytes(), (got, want)
    assert (got[0] == -7.0).all() and (got[2, 2:] == -7.0).all() and (got[1] != -7.0).all()
    # the pad clamps: to 0 on the left / top, to w0 / h0 on the right / bottom; a tiny x stays 0
    assert got[1, 0, 0] == 0.0 and got[1, 0, 2] == 0.0 and got[1, 1, 2] == 5.0 and got[1, 0, 3] == 7.0
    assert got[2, 0].tolist() == [0.0, 0.0, 64.0, 32.0] and got[2, 1, 1] == 0.0 and got[2, 1, 3] == 0.0
    # in place
    call("ym_unletterbox_boxes", inp.data_ptr(), cnt.data_ptr(), tdev.data_ptr(), B, N, H, W, inp.data_ptr(),
         stream_ptr(inp.device))
    assert inp.cpu().numpy().tobytes() == LR.unletterbox(boxes, counts, table, H, W, out=boxes).tobytes()


def test_argument_checks():
    from yolomi._lib import lib, stream_ptr
    H = W = 32
    ims = LR.sources(H, W, 4)
    u8, meta = _dev(ims)
    B = len(ims)
    tb = _table_dev(LR.entries(ims, H, W), B)
    out = _out(B, 4, H, W, False)
    st = stream_ptr(u8.device)
    L = lib()
    for ch in (0, 5, -1):
        assert L.ym_letterbox_u8c(u8.data_ptr(), meta.data_ptr(), tb.data_ptr(), B, ch, H, W, 114, out.data_ptr(),
                                  st) == -1
    for h, w in ((0, 32), (32, 0), (40000, 32)):
        assert L.ym_letterbox_u8c(u8.data_ptr(), meta.data_ptr(), tb.data_ptr(), B, 4, h, w, 114, out.data_ptr(),
                                  st) == -1
    assert L.ym_letterbox_u8c(u8.data_ptr(), meta.data_ptr(), None, B, 4, H, W, 114, out.data_ptr(), st) == -1
    boxes = torch.zeros(B, 4, 4, device="cuda")
    cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    assert L.ym_unletterbox_boxes(boxes.data_ptr() + 4, cnt.data_ptr(), tb.data_ptr(), B, 3, H, W, boxes.data_ptr(),
                                  st) == -1
    assert b"aligned" in L.ym_last_error()
    assert L.ym_unletterbox_boxes(boxes.data_ptr(), cnt.data_ptr(), tb.data_ptr(), -1, 4, H, W, boxes.data_ptr(),
                                  st) == -1
    torch.cuda.synchronize()
    assert (out == -1.0).all()                             # nothing was launched


# ---------------------------------------------------------------- the Python layers
HW = [(24, 64), (64, 40), (64, 64), (10, 50)]


def _host_batch(ch, S, letterbox=True):
    from datasets import collate_fn_cuda
    rng = np.random.default_rng(12)
    ims = [rng.integers(0, 256, (*hw, ch), dtype=np.uint8) for hw in HW]
    items = [(torch.from_numpy(a[..., 0].copy()).unsqueeze(0) if ch == 1 else torch.from_numpy(a),
              torch.tensor([[0.5, 0.5, 0.5, 0.25]]), torch.tensor([i % 3]), i) for i, a in enumerate(ims)]
    return collate_fn_cuda(items, img_size=S, channels=ch, letterbox=letterbox), ims


@pytest.mark.parametrize("ch", [1, 3])
def test_prepare_batch_letterboxes(ch):
    from datasets import prepare_batch
    S = 64
    batch, ims = _host_batch(ch, S)
    d = prepare_batch(batch, torch.device("cuda"))
    assert set(d) == {"img", "batch_idx", "cls", "bboxes", "max_gt"} and d["img"].shape == (4, ch, S, S)
    want = LR.render(LR.entries(ims, S, S), ims, S, S, 114)
    assert np.array_equal(d["img"].cpu().numpy(), LR.as_float(want))
    assert torch.equal(d["bboxes"].cpu(), batch["bboxes"])
    stretched = prepare_batch(_host_batch(ch, S, letterbox=False)[0], torch.device("cuda"))
    assert not torch.equal(stretched["img"], d["img"]) and torch.equal(stretched["img"][2], d["img"][2])


def test_batch_augment_on_a_letterboxed_batch():
    """The unmodified ym_augment_u8c runs the letterboxed plan: bit for bit the restatement of its table."""
    import augment_colour_ref as CR
    from datasets import AugmentHyp, BatchAugment
    S = 64
    batch, ims = _host_batch(3, S)
    hyp = AugmentHyp(degrees=5.0, hsv_h=0.015, hsv_s=0.7)
    for step in range(2):
        aug = BatchAugment(hyp, seed=3)
        d = aug(batch, torch.device("cuda"), 1, step)
        assert set(d) == {"img", "batch_idx", "cls", "bboxes", "max_gt"}
        table = aug.plan(batch, 1, step)[0]
        col = aug.colours(4, 1, step)
        want = CR.render_c(table, ims, S, [(c.hue, c.sat) for c in col])
        assert np.array_equal(d["img"].cpu().numpy(), AR.as_float(want))


def test_unletterbox_over_decode_nms_output():
    """Both forms decode_nms returns, against the restatement; scores and labels pass through."""
    from datasets.letterbox import lb_table, table_bytes, unletterbox
    from datasets.synthetic import synth_eval_preds
    from yolomi import post
    S = 64
    pred = synth_eval_preds(3, 200, img_size=S, seed=4).cuda()
    meta = torch.tensor([[0, 24, 64], [0, 64, 40], [0, 10, 50]])
    table = lb_table(meta, S, S)
    tdev = table_bytes(table, 3).cuda()
    padded = post.decode_nms(pred, S, 0.25, 0.45, padded=True)
    listed = post.decode_nms(pred, S, 0.25, 0.45)
    assert sum(padded["counts"]) > 0 and padded["counts"] == [len(d["scores"]) for d in listed]
    want = LR.unletterbox(padded["boxes"].cpu().numpy(), padded["counts"], table, S, S)
    for got in (unletterbox(padded, tdev, S, S), unletterbox(listed, tdev, S, S)):
        for b, (g, d) in enumerate(zip(got, listed)):
            k = padded["counts"][b]
            assert g["boxes"].cpu().numpy().tobytes() == want[b, :k].tobytes(), b
            assert torch.equal(g["scores"], d["scores"]) and torch.equal(g["labels"], d["labels"])
