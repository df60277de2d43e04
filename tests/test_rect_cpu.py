"""Rectangular inference and validation, the host side: the frame rule, RectSampler, image_hw, the
collate with rect=True and the flags.  No GPU."""
import numpy as np
import pytest
import torch

import letterbox_ref as LR
import rect_ref as RR


# ---------------------------------------------------------------- the frame rule
def test_rect_frame_worked_values():
    from datasets.letterbox import letterbox_geometry, rect_frame
    for (h0, w0), imgsz, fr, geom in RR.WORKED:
        assert rect_frame([(h0, w0)], imgsz) == fr == RR.frame([(h0, w0)], imgsz), (h0, w0, imgsz)
        assert letterbox_geometry(h0, w0, *fr) == geom == LR.geometry(h0, w0, *fr), (h0, w0, imgsz)
    for hws, imgsz, fr in RR.WORKED_BATCH:
        assert rect_frame(hws, imgsz) == fr == RR.frame(hws, imgsz), hws
    assert rect_frame([], 160) == (32, 32) and rect_frame([(0, 5), (5, 0)], 160) == (32, 32)
    assert rect_frame([(30, 40)], 64, stride=16) == (48, 64)
    out = rect_frame(np.array([[60, 100]]), 160)
    assert out == (96, 160) and all(type(v) is int for v in out)


def test_rect_frame_rejects_a_size_off_the_stride():
    from datasets.letterbox import rect_frame
    for bad in (100, 0, -32, 16):
        with pytest.raises(ValueError):
            rect_frame([(480, 640)], bad)
    with pytest.raises(ValueError):
        rect_frame([(480, 640)], 64, stride=48)


def test_rect_frame_properties_over_random_sizes():
    from datasets.letterbox import letterbox_geometry, rect_frame
    rng = np.random.default_rng(23)
    sizes = (32, 64, 160, 320, 640, 1280)
    frames = []
    for _ in range(2000):
        h0, w0 = int(rng.integers(1, 3001)), int(rng.integers(1, 3001))
        imgsz = int(sizes[rng.integers(0, len(sizes))])
        H, W = rect_frame([(h0, w0)], imgsz)
        assert (H, W) == RR.frame([(h0, w0)], imgsz), (h0, w0, imgsz)
        assert H % 32 == 0 and W % 32 == 0 and 32 <= H <= imgsz and 32 <= W <= imgsz, (h0, w0, imgsz, H, W)
        assert max(H, W) == imgsz, (h0, w0, imgsz, H, W)
        nw, nh, left, top = letterbox_geometry(h0, w0, H, W)
        assert nw == W or nh == H, (h0, w0, imgsz, H, W, nw, nh)
        assert 0 <= W - nw < 32 and 0 <= H - nh < 32, (h0, w0, imgsz, H, W, nw, nh)
        assert left == (W - nw) // 2 and top == (H - nh) // 2
        frames.append(((h0, w0), imgsz, (H, W)))
    # a batch's frame is the element-wise maximum of its images' frames
    for imgsz in sizes:
        group = [f for f in frames if f[1] == imgsz]
        for lo in range(0, len(group) - 3, 3):
            part = group[lo:lo + 3]
            want = (max(f[2][0] for f in part), max(f[2][1] for f in part))
            assert rect_frame([f[0] for f in part] + [(0, 0)], imgsz) == want


# ---------------------------------------------------------------- RectSampler
def test_rect_sampler_order():
    from datasets import RectSampler
    from yolomi.dist import ValShard
    ratios = [1.0, 0.5, 2.0, 0.5, 1.0, 0.25, 0.5, 2.0, 1.0, 0.6]
    s = RectSampler(range(10), ratios)
    assert len(s) == 10
    assert list(s) == [5, 1, 3, 6, 9, 0, 4, 8, 2, 7]                # ties keep the inner order
    assert list(s) == list(s)                                        # every pass materialises it again
    assert list(RectSampler([7, 2, 0, 4, 8], ratios)) == [0, 4, 8, 7, 2]
    seen = []
    for rank in range(3):
        shard = ValShard(10, rank, 3)
        got = list(RectSampler(shard, ratios))
        assert sorted(got) == list(shard) and len(RectSampler(shard, ratios)) == len(shard)
        assert [ratios[i] for i in got] == sorted(ratios[i] for i in shard)
        for a, b in zip(got, got[1:]):
            assert ratios[a] < ratios[b] or a < b
        seen += got
    assert sorted(seen) == list(range(10))                           # no image twice, none lost


# ---------------------------------------------------------------- image_hw
def test_image_hw_reads_the_header(tmp_path):
    from PIL import Image
    from datasets import YoloTxtDataset
    (tmp_path / "images").mkdir()
    rng = np.random.default_rng(4)
    sizes = [(5, 9), (9, 5), (7, 7)]
    for i, hw in enumerate(sizes):
        Image.fromarray(rng.integers(0, 256, (*hw, 3), dtype=np.uint8)).save(tmp_path / "images" / f"im{i}.png")
    for ch in (1, 3):
        ds = YoloTxtDataset(tmp_path, img_size=32, channels=ch)
        for i, hw in enumerate(sizes):
            assert ds.image_hw(i) == hw == ds.load_image(i).shape[:2]
            assert ds.image_hw(i) is ds.image_hw(i)                  # cached
        with pytest.raises(IndexError):
            ds.image_hw(3)


# ---------------------------------------------------------------- collate
HWS = [(60, 100), (90, 160), (0, 0), (20, 100)]


def _items(hws=HWS):
    rng = np.random.default_rng(3)
    items = []
    for i, (h, w) in enumerate(hws):
        im = torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        n = 0 if h == 0 else i + 1
        c = rng.uniform(0.3, 0.7, (n, 2))
        boxes = torch.from_numpy(np.concatenate([c, rng.uniform(0.1, 0.5, (n, 2))], 1)).float().reshape(-1, 4)
        items.append((im, boxes, torch.full((n,), i % 3, dtype=torch.long), i))
    return items


def test_collate_rect():
    from datasets import collate_fn_cuda
    from datasets.letterbox import letterbox_geometry, map_labels, rect_frame
    items = _items()
    base = collate_fn_cuda(items, img_size=160, channels=3)
    got = collate_fn_cuda(items, img_size=160, channels=3, letterbox=True, rect=True)
    assert list(got) == ["img_u8", "img_meta", "img_size", "img_ch", "img_lb", "img_frame", "batch_idx", "cls",
                         "bboxes"]
    H, W = rect_frame(HWS, 160)
    assert (H, W) == (96, 160)
    assert got["img_frame"].dtype == torch.int32 and got["img_frame"].tolist() == [H, W] and got["img_size"] == 160
    assert got["img_lb"].dtype == torch.int32
    assert got["img_lb"].tolist() == [list(letterbox_geometry(h, w, H, W)) for h, w in HWS]
    assert got["img_lb"].tolist() == [[160, 96, 0, 0], [160, 90, 0, 3], [0, 0, 0, 0], [160, 32, 0, 32]]
    for k in ("img_u8", "img_meta", "batch_idx", "cls"):
        assert torch.equal(got[k], base[k]), k
    src = base["bboxes"].numpy()
    bidx = base["batch_idx"].tolist()
    want = np.concatenate([map_labels(src[j:j + 1], got["img_lb"][b].tolist(), H, W) for j, b in enumerate(bidx)])
    assert got["bboxes"].dtype == torch.float32 and np.array_equal(got["bboxes"].numpy(), want.astype(np.float32))
    # the frame is the batch's own: the portrait alone gets the transposed one
    tall = collate_fn_cuda(_items([(100, 60)]), img_size=160, channels=3, letterbox=True, rect=True)
    assert tall["img_frame"].tolist() == [160, 96] and tall["img_lb"].tolist() == [[96, 160, 0, 0]]


def test_collate_without_rect_is_what_it_was():
    from datasets import collate_fn_cuda
    from datasets.crater import pack_images
    items = _items()
    for kw in ({}, {"letterbox": True}):
        a = collate_fn_cuda(items, img_size=160, channels=3, **kw)
        b = collate_fn_cuda(items, img_size=160, channels=3, rect=False, **kw)
        assert list(a) == list(b) and "img_frame" not in a
        assert list(a) == ["img_u8", "img_meta", "img_size", "img_ch"] + (["img_lb"] if kw else []) + [
            "batch_idx", "cls", "bboxes"]
        for k in a:
            assert torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else a[k] == b[k], k
    lb = collate_fn_cuda(items, img_size=160, channels=3, letterbox=True)
    assert lb["img_lb"].tolist()[:2] == [[160, 96, 0, 32], [160, 90, 0, 35]]          # the square frame's rows
    raw = [it[0] for it in items]
    assert list(pack_images(raw, 160, 3, True, False)) == list(pack_images(raw, 160, 3, True))


def test_rect_needs_letterbox():
    from datasets import collate_fn_cuda
    from datasets.crater import pack_images
    items = _items()
    with pytest.raises(ValueError):
        collate_fn_cuda(items, img_size=160, channels=3, rect=True)
    with pytest.raises(ValueError):
        pack_images([it[0] for it in items], 160, 3, rect=True)
    with pytest.raises(ValueError):                                  # a frame needs imgsz on the stride
        collate_fn_cuda(items, img_size=100, channels=3, letterbox=True, rect=True)


# ---------------------------------------------------------------- the restated decode, flags
def test_restated_decode_equals_the_oracle_on_a_square_frame():
    from datasets.synthetic import synth_eval_preds
    from oracle import post as op
    pred = synth_eval_preds(3, 17, seed=31).numpy()
    got = RR.decode_wh("cpu17", pred, 640, 640, 0.25, 0.45)
    for (gb, gs, gl), (wb, ws, wl) in zip(got, op.decode(pred, 640, 0.25, 0.45)):
        assert len(ws) >= 1
        np.testing.assert_array_equal(gb, wb)
        np.testing.assert_array_equal(gs, ws)
        np.testing.assert_array_equal(gl, wl)
    a = RR.decode_wh("cpu17", pred, 384, 640, 0.25, 0.45)
    b = RR.decode_wh("cpu17", pred, 640, 384, 0.25, 0.45)
    for (ab, _, _), (bb, _, _), (gb, _, _) in zip(a, b, got):
        np.testing.assert_array_equal(ab[:, [0, 2]], gb[:, [0, 2]])  # x over 640 in both
        np.testing.assert_array_equal(bb[:, [1, 3]], gb[:, [1, 3]])
        assert not np.array_equal(ab, bb)


def test_flags(capsys):
    import inspect
    import train_yolo11_cuda as T
    ap = T.build_parser()
    assert ap.parse_args([]).val_rect is False
    ns = ap.parse_args(["--val-rect", "--data-format", "yolo", "--ch", "3"])
    assert ns.val_rect is True and ns.letterbox is False             # the train loader is what the other flags say
    with pytest.raises(SystemExit):
        ap.parse_args(["--val-rect", "--synthetic", "4"])
    with pytest.raises(SystemExit):
        ap.parse_args(["--val-rect", "--imgsz", "100"])
    capsys.readouterr()
    assert inspect.signature(T.make_loaders).parameters["val_rect"].default is False
    assert inspect.signature(T.validate).parameters["max_frames"].default is None
    import predict as P
    assert P.build_parser().parse_args(["--weights", "w.pt", "--source", "d"]).rect is False
    assert P.build_parser().parse_args(["--weights", "w.pt", "--source", "d", "--rect"]).rect is True
    from yolomi.predict import Predictor
    sig = inspect.signature(Predictor.__init__).parameters
    assert sig["rect"].default is False and sig["max_frames"].default == 8
