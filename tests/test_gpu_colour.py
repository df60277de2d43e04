"""1-4 plane GPU resize and augmentation (ym_resize_linear_u8c, ym_augment_u8c): one plane bit for bit equal to the
single-plane entry points, 2-4 planes and hue / saturation bit for bit equal to the numpy restatement
(tests/augment_colour_ref.py) over the case list the sanitized host build is held to, the argument checks,
BatchAugment on a 3-plane batch and two training steps from a YoloTxtDataset."""
import copy
import dataclasses
import functools

import numpy as np
import pytest
import torch

import augment_colour_ref as CR
import augment_ref as AR

pytestmark = pytest.mark.gpu

SIZES = [32, 31]                                           # 31: S * S is odd, the scalar-store path


def _dev(ims):
    buf, meta = AR.pack(ims)
    return torch.from_numpy(buf).cuda(), torch.from_numpy(meta).cuda()


def _bytes_dev(table):
    from datasets.augment import table_bytes
    return table_bytes(table).cuda()


def _out(B, ch, S, offset):
    """(B, ch, S, S) fp32 on the device; `offset`: starting 4 bytes into its allocation (not 16-byte aligned)."""
    flat = torch.full((B * ch * S * S + 1,), -1.0, dtype=torch.float32, device="cuda")
    out = flat[1:] if offset else flat[:-1]
    assert out.data_ptr() % 16 == (4 if offset else 0)
    return out.view(B, ch, S, S)


def _augment(table, ims, S, colours=None, offset=False):
    """One ym_augment_u8c launch over pixel-interleaved `ims` -> (B, ch, S, S) fp32 on the host."""
    from yolomi._lib import call, stream_ptr
    ch, B = ims[0].shape[2], len(ims)
    assert len(table) == B
    u8, meta = _dev(ims)
    out = _out(B, ch, S, offset)
    col = None if colours is None else _bytes_dev(CR.colour_table(colours))
    call("ym_augment_u8c", u8.data_ptr(), meta.data_ptr(), _bytes_dev(table).data_ptr(),
         None if col is None else col.data_ptr(), B, ch, S, out.data_ptr(), stream_ptr(u8.device))
    return out.cpu().numpy()


def _resize(ims, S, offset=False):
    from yolomi._lib import call, stream_ptr
    ch, B = ims[0].shape[2], len(ims)
    u8, meta = _dev(ims)
    out = _out(B, ch, S, offset)
    call("ym_resize_linear_u8c", u8.data_ptr(), meta.data_ptr(), B, ch, S, out.data_ptr(), stream_ptr(u8.device))
    return out.cpu().numpy()


def _chunks(S):
    """The case list in tables of one entry per image of the batch (the last one padded with the first case)."""
    names, entries = zip(*CR.cases(S))
    B = len(CR.SOURCE_SIZES)
    for lo in range(0, len(entries), B):
        chunk = list(entries[lo:lo + B])
        n = len(chunk)
        yield names[lo:lo + n], CR.table_of(chunk + [entries[0]] * (B - n)), n, lo


def _check_exact(got, want_u8, names):
    """Bit for bit: the floats are v / 255.0f and round back to the restatement's bytes."""
    want = AR.as_float(want_u8)
    for k, name in enumerate(names):
        assert np.array_equal(got[k], want[k]), (name, int((got[k] != want[k]).sum()))
        assert np.array_equal(np.rint(got[k] * 255.0).astype(np.int64), want_u8[k]), name


@pytest.mark.parametrize("S", SIZES)
def test_one_plane_equals_single_plane_entry_points(S):
    from datasets.augment import augment_batch
    from datasets.crater import resize_batch
    ims = CR.sources(S, 1)
    u8, meta = _dev(ims)
    assert np.array_equal(_resize(ims, S), resize_batch(u8, meta, S).cpu().numpy())
    for names, table, n, _ in _chunks(S):
        got = _augment(table, ims, S)
        want = augment_batch(u8, meta, _bytes_dev(table), S).cpu().numpy()
        for k in range(n):
            assert np.array_equal(got[k], want[k]), (names[k], int((got[k] != want[k]).sum()))


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("ch", [2, 3, 4])
def test_planes_equal_restatement(S, ch):
    ims = CR.sources(S, ch)
    for names, table, n, _ in _chunks(S):
        _check_exact(_augment(table, ims, S)[:n], CR.render_c(table, ims, S)[:n], names)
    # the resize is the stretch entry of every image without a gain
    from datasets.augment import plain_entry
    table = CR.table_of([plain_entry(b, *a.shape[:2], S) for b, a in enumerate(ims)])
    _check_exact(_resize(ims, S), CR.render_c(table, ims, S), [f"resize{b}" for b in range(len(ims))])


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_out_offset_by_four_bytes(ch):
    """`out` not 16-byte aligned at a size whose groups would otherwise be vector stores; nothing written outside."""
    S = 32
    ims = CR.sources(S, ch)
    names, table, n, _ = next(iter(_chunks(S)))
    colours = CR.colours_of(len(table), seed=1) if ch == 3 else None
    assert np.array_equal(_augment(table, ims, S, colours, offset=True), _augment(table, ims, S, colours))
    assert np.array_equal(_resize(ims, S, offset=True), _resize(ims, S))
    from yolomi._lib import call, stream_ptr
    u8, meta = _dev(ims)
    flat = torch.full((len(ims) * ch * S * S + 8,), -1.0, dtype=torch.float32, device="cuda")
    call("ym_augment_u8c", u8.data_ptr(), meta.data_ptr(), _bytes_dev(table).data_ptr(), None, len(ims), ch, S,
         flat[1:].data_ptr(), stream_ptr(u8.device))
    assert float(flat[0]) == -1.0 and (flat[-7:] == -1.0).all() and (flat[1:-7] >= 0.0).all()


@pytest.mark.parametrize("S", SIZES)
def test_hue_sat_in_the_launch_equals_restatement(S):
    ims = CR.sources(S, 3)
    for names, table, n, lo in _chunks(S):
        colours = CR.colours_of(len(table), seed=S + lo)
        _check_exact(_augment(table, ims, S, colours)[:n], CR.render_c(table, ims, S, colours)[:n], names)


def test_hue_sat_on_primaries_unit_chroma_and_random_pixels():
    """S x S sources through stretch entries (a copy): every output pixel is hue / sat of one chosen source pixel."""
    from datasets.augment import plain_entry
    S = 32
    rng = np.random.default_rng(23)
    prim = np.array([[255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255], [255, 0, 255], [0, 0, 0],
                     [255, 255, 255]], np.uint8)
    base = rng.integers(0, 255, (S * S, 1), dtype=np.uint8)
    unit = base + np.eye(3, dtype=np.uint8)[rng.integers(0, 3, S * S)] * rng.integers(0, 2, (S * S, 1), dtype=np.uint8)
    unit2 = (base + 1 - np.eye(3, dtype=np.uint8)[rng.integers(0, 3, S * S)]).astype(np.uint8)
    ims = [np.resize(prim, (S * S, 3)).reshape(S, S, 3), unit.reshape(S, S, 3), unit2.reshape(S, S, 3),
           rng.integers(0, 256, (S, S, 3), dtype=np.uint8)]
    table = CR.table_of([plain_entry(b, S, S, S, gain=g) for b, g in enumerate((1.0, 1.0, 1.1, 0.8))])
    for seed in (0, 1):
        colours = CR.colours_of(10, seed)[1 + 4 * seed:5 + 4 * seed]
        got = _augment(table, ims, S, colours)
        want = CR.render_c(table, ims, S, colours)
        _check_exact(got, want, [f"image{b} {colours[b]}" for b in range(4)])
        for b in range(2):                                 # gain 1.0: the restatement of the rule alone
            direct = CR.hue_sat(ims[b].astype(np.int64), *colours[b])
            assert np.array_equal(np.moveaxis(want[b], 0, -1), direct)


def test_grey_image_in_three_planes_equals_one_plane():
    from datasets.augment import augment_batch
    S = 32
    one = CR.sources(S, 1)
    grey = [np.repeat(a, 3, axis=2) for a in one]
    u8, meta = _dev(one)
    for names, table, n, lo in _chunks(S):
        got = _augment(table, grey, S, CR.colours_of(len(table), seed=lo))
        want = augment_batch(u8, meta, _bytes_dev(table), S).cpu().numpy()
        for c in range(3):
            assert np.array_equal(got[:n, c], want[:n, 0]), (names, c)


def test_argument_checks():
    from yolomi._lib import lib, stream_ptr
    S, B = 32, 4
    L = lib()
    for ch_buf in (1, 4):
        ims = CR.sources(S, ch_buf)
        u8, meta = _dev(ims)
        names, table, n, _ = next(iter(_chunks(S)))
        tb, col = _bytes_dev(table), _bytes_dev(CR.colour_table(CR.colours_of(B)))
        out = _out(B, 4, S, False)
        st = stream_ptr(u8.device)
        for ch in (0, 5, -1):
            assert L.ym_augment_u8c(u8.data_ptr(), meta.data_ptr(), tb.data_ptr(), None, B, ch, S, out.data_ptr(),
                                    st) == -1                                  # YM_ERR_ARG
            assert L.ym_resize_linear_u8c(u8.data_ptr(), meta.data_ptr(), B, ch, S, out.data_ptr(), st) == -1
        for ch in (1, 2, 4, 0, 5):                         # a colour table needs three planes
            assert L.ym_augment_u8c(u8.data_ptr(), meta.data_ptr(), tb.data_ptr(), col.data_ptr(), B, ch, S,
                                    out.data_ptr(), st) == -1
        assert b"ch" in L.ym_last_error()
    torch.cuda.synchronize()
    assert (out == -1.0).all()                             # nothing was launched


# ---------------------------------------------------------------- BatchAugment and the trainer
BOXES = [[[0.1, 0.2, 0.4, 0.5], [0.6, 0.6, 0.9, 0.95]], [[0.25, 0.25, 0.75, 0.5]], [], [[0.0, 0.0, 1.0, 1.0]]]
HW = [(48, 64), (70, 51), (64, 64), (10, 200)]


def _host_batch(ch, S):
    from datasets.crater import pack_images
    rng = np.random.default_rng(11)
    ims = [rng.integers(0, 256, (*hw, 3), dtype=np.uint8) for hw in HW]
    if ch == 1:
        b = pack_images([torch.from_numpy(a[..., 0].copy()).unsqueeze(0) for a in ims], S)
    else:
        b = pack_images([torch.from_numpy(a) for a in ims], S, channels=3)
    b.update({"batch_idx": torch.cat([torch.full((len(x),), i, dtype=torch.long) for i, x in enumerate(BOXES)]),
              "bboxes": torch.cat([torch.tensor(x, dtype=torch.float32).reshape(-1, 4) for x in BOXES]),
              "cls": (torch.arange(sum(len(x) for x in BOXES)) % 3).reshape(-1, 1)})
    return b, ims


def test_batch_augment_three_planes():
    from datasets import AugmentHyp, BatchAugment, prepare_batch
    S = 64
    hyp = AugmentHyp(degrees=8.0, shear=2.0, flipud=0.3, hsv_h=0.015, hsv_s=0.7)
    b3, ims = _host_batch(3, S)
    b1, _ = _host_batch(1, S)
    dev = torch.device("cuda")
    for step in range(2):
        d3 = BatchAugment(hyp, seed=11)(b3, dev, 1, step)
        d1 = BatchAugment(hyp, seed=11)(b1, dev, 1, step)
        assert set(d3) == {"img", "batch_idx", "cls", "bboxes", "max_gt"}
        assert d3["img"].shape == (4, 3, S, S) and d3["img"].dtype == torch.float32 and d3["img"].is_cuda
        assert d1["img"].shape == (4, 1, S, S)
        for k in ("batch_idx", "cls", "bboxes"):            # the labels do not depend on the plane count
            assert torch.equal(d3[k], d1[k]), k
        assert d3["max_gt"] == d1["max_gt"]
        aug = BatchAugment(hyp, seed=11)
        table = aug.plan(b3, 1, step)[0]
        col = aug.colours(4, 1, step)
        want = CR.render_c(table, ims, S, [(c.hue, c.sat) for c in col])
        assert np.array_equal(d3["img"].cpu().numpy(), AR.as_float(want))
        # without hue / saturation, plane 0 of the colour batch is the 1-plane batch (whose bytes are plane 0)
        plain = dataclasses.replace(hyp, hsv_h=0.0, hsv_s=0.0)
        p3 = BatchAugment(plain, seed=11)(b3, dev, 1, step)
        assert torch.equal(p3["img"][:, :1], BatchAugment(plain, seed=11)(b1, dev, 1, step)["img"])
    v = prepare_batch(b3, dev)                              # the validation path: the stretch of every image
    assert v["img"].shape == (4, 3, S, S) and "img_ch" not in v and "img_u8" not in v
    from datasets.augment import plain_entry
    table = CR.table_of([plain_entry(i, *hw, S) for i, hw in enumerate(HW)])
    assert np.array_equal(v["img"].cpu().numpy(), AR.as_float(CR.render_c(table, ims, S)))


def _write_yolo(root, n=4):
    from PIL import Image
    rng = np.random.default_rng(31)
    (root / "images").mkdir()
    (root / "labels").mkdir()
    for i in range(n):
        h, w = int(rng.integers(40, 90)), int(rng.integers(40, 90))
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(root / "images" / f"im{i}.png")
        rows = [f"{int(rng.integers(0, 3))} {rng.uniform(0.3, 0.7):.4f} {rng.uniform(0.3, 0.7):.4f} "
                f"{rng.uniform(0.2, 0.5):.4f} {rng.uniform(0.2, 0.5):.4f}" for _ in range(int(rng.integers(1, 4)))]
        (root / "labels" / f"im{i}.txt").write_text("\n".join(rows) + "\n")


def test_two_colour_training_steps(tmp_path):
    """Scale n, ch=3, nc=3, 64 x 64, bs 2 from a YoloTxtDataset through BatchAugment with hue and saturation."""
    import train_yolo11_cuda as T
    from datasets import AugmentHyp, BatchAugment, YoloTxtDataset, collate_fn_cuda
    from losses import v8DetectionLoss
    from test_gpu_model import _seeded_model
    from yolomi.optim import FusedAdamW
    _write_yolo(tmp_path)
    ds = YoloTxtDataset(tmp_path, img_size=64, channels=3)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False,
                                         collate_fn=functools.partial(collate_fn_cuda, img_size=64, channels=3))
    assert len(loader) == 2
    m = _seeded_model("n", nc=3, ch=3).train()
    before = copy.deepcopy(m.state_dict())
    opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=5e-4, max_grad_norm=10.0)
    aug = BatchAugment(AugmentHyp(hsv_h=0.015, hsv_s=0.7), seed=4)
    out = T.train_one_epoch(m, loader, opt, v8DetectionLoss(m), torch.device("cuda"), 1, 1, None, aug)
    assert set(out) == {"loss", "box_loss", "cls_loss", "dfl_loss"}
    assert all(np.isfinite(v) for v in out.values()), out
    changed = [k for k, v in m.named_parameters() if not torch.equal(v.detach(), before[k])]
    assert "model.0.conv.weight" in changed and m.model[0].conv.weight.shape[1] == 3      # the 3-plane stem learnt
    assert len(changed) > len(list(m.parameters())) // 2, changed
    assert all(torch.isfinite(p).all() for p in m.parameters())
