"""Letterbox data path without a GPU: ym_letterbox_u8c's per-pixel function (include/yolomi_augment.h) built for the
host with the address and undefined-behaviour sanitizers as a stand-alone program and held byte for byte to the numpy
restatement (tests/letterbox_ref.py) over the GPU test's case list; the host geometry; the label map and its inverse;
collating with and without the flag; BatchAugment.plan on a letterboxed batch through tests/augment_ref.py; the
trainer's and the predict CLI's flags."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest
import torch

import augment_colour_ref as CR
import augment_ref as AR
import letterbox_ref as LR
from conftest import ROOT

FRAMES = [(32, 32), (31, 31), (32, 48)]                    # (H, W); 31 x 31: odd area, the scalar-store path


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("lbhost") / "letterbox_host"
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "letterbox_host.cpp"), "-o", str(exe)], check=True)
    return exe


@pytest.mark.parametrize("H,W", FRAMES)
@pytest.mark.parametrize("ch", [1, 2, 3, 4])
def test_host_build_equals_restatement(host_program, tmp_path, H, W, ch):
    ims = LR.sources(H, W, ch)
    table = LR.entries(ims, H, W, LR.SCALEUP)
    for fill in (0, 114, 255):
        got = LR.run_host(host_program, tmp_path, table, ims, H, W, fill)
        want = LR.render(table, ims, H, W, fill)
        for i, hw in enumerate(LR.SOURCE_SIZES):
            assert np.array_equal(got[i], want[i]), (hw, fill, int((got[i] != want[i]).sum()))
    # the cases are not degenerate: pad and image both show, the empty image is all fill, the copy is a copy
    k = LR.SOURCE_SIZES.index((7, 5))
    assert (want[k] == 255).all(axis=(0, 1)).any() and (want[k] != 255).any()
    assert (want[LR.SOURCE_SIZES.index((0, 0))] == 255).all()
    c = LR.SOURCE_SIZES.index(None)
    assert np.array_equal(np.moveaxis(want[c], 0, -1), ims[c])
    no_up = want[8]                                        # (16, 12) without scale-up: 12 x 16 pixels copied
    e = table[8]
    assert (e.nw, e.nh) == (12, 16) and np.array_equal(
        np.moveaxis(no_up[:, e.top:e.top + 16, e.left:e.left + 12], 0, -1), ims[8])


def test_mismatched_entry_and_offsets_outside_the_frame(host_program, tmp_path):
    """An entry whose source size is not the image's shows the fill; an interior hanging over the frame is cut."""
    H = W = 32
    ims = LR.sources(H, W, 3)[1:4]
    table = LR.entries(ims, H, W)
    table[0].w0 += 1
    table[1].left, table[1].top = -5, 20
    table[2].left = W - 3
    got = LR.run_host(host_program, tmp_path, table, ims, H, W, 9)
    assert np.array_equal(got, LR.render(table, ims, H, W, 9))
    assert (got[0] == 9).all() and (got[1] != 9).any() and (got[2][:, :, :W - 3] == 9).all()


def test_square_source_equals_the_stretch():
    """At nw = nh = S the restatement is the loader's resize (tests/augment_colour_ref.py's stretch entry)."""
    from datasets.augment import plain_entry
    S = 32
    ims = [a for a in LR.sources(S, S, 3) if a.shape[0] == a.shape[1] and a.size]
    table = LR.entries(ims, S, S)
    assert all((e.nw, e.nh, e.left, e.top) == (S, S, 0, 0) for e in list(table)[:len(ims)])
    stretch = CR.table_of([plain_entry(b, *a.shape[:2], S) for b, a in enumerate(ims)])
    assert np.array_equal(LR.render(table, ims, S, S), CR.render_c(stretch, ims, S))


# ---------------------------------------------------------------- geometry
def test_letterbox_geometry():
    from datasets.letterbox import letterbox_geometry as g
    assert g(480, 640, 640, 640) == (640, 480, 0, 80)
    assert g(7, 5, 32, 32) == (23, 32, 4, 0)
    # w0 * r = k + 0.5 rounds up (Python's round would go to even): 3 * 1.5 = 4.5 -> 5, 1 * 1.5 -> 2
    assert g(4, 3, 6, 6) == (5, 6, 0, 0)
    assert g(4, 1, 6, 6) == (2, 6, 2, 0)
    assert g(3, 4, 6, 6) == (6, 5, 0, 0)
    # without scale-up a small image keeps its size, a large one still shrinks
    assert g(12, 16, 32, 32, scaleup=False) == (16, 12, 8, 10)
    assert g(12, 16, 32, 32) == (32, 24, 0, 4)
    assert g(64, 128, 32, 32, scaleup=False) == (32, 16, 0, 8)
    # one pixel in a dimension: at least 1 wide after a large shrink, the whole frame when it grows
    assert g(1, 1000, 32, 32) == (32, 1, 0, 15)
    assert g(1000, 1, 32, 32) == (1, 32, 15, 0)
    assert g(1, 1, 32, 48) == (32, 32, 8, 0)
    assert g(0, 5, 32, 32) == (0, 0, 0, 0) and g(5, 0, 32, 32) == (0, 0, 0, 0)
    rng = np.random.default_rng(0)
    for _ in range(2000):                                  # the restatement's rule, and the frame always holds it
        h0, w0, H, W = (int(v) for v in rng.integers(1, 700, 4))
        for up in (True, False):
            nw, nh, left, top = got = g(h0, w0, H, W, up)
            assert got == LR.geometry(h0, w0, H, W, up)
            assert 1 <= nw <= W and 1 <= nh <= H and 0 <= left and left + nw <= W and 0 <= top and top + nh <= H
            assert nw == W or nh == H or (not up and (nw, nh) == (w0, h0))


def test_table_layout_and_values():
    from datasets.letterbox import lb_table, table_bytes
    from yolomi._lib import LbEntry
    assert ctypes.sizeof(LbEntry) == 32
    assert [(n, getattr(LbEntry, n).offset) for n, _ in LbEntry._fields_] == [
        ("nw", 0), ("nh", 4), ("left", 8), ("top", 12), ("w0", 16), ("h0", 20), ("sx", 24), ("sy", 28)]
    meta = torch.tensor([[0, 7, 5], [35, 480, 640], [99, 0, 0]])
    t = lb_table(meta, 32, 32)
    assert [(e.nw, e.nh, e.left, e.top, e.w0, e.h0) for e in t] == [(23, 32, 4, 0, 5, 7), (32, 24, 0, 4, 640, 480),
                                                                    (0, 0, 0, 0, 0, 0)]
    assert np.float32(t[0].sx) == np.float32(5) / np.float32(23) and np.float32(t[1].sy) == np.float32(20.0)
    assert (t[2].sx, t[2].sy) == (0.0, 0.0)
    ims = [np.zeros((7, 5, 1), np.uint8), np.zeros((480, 640, 1), np.uint8), np.zeros((0, 0, 1), np.uint8)]
    assert bytes(t) == bytes(LR.entries(ims, 32, 32))
    assert table_bytes(t, 2).numel() == 64 and table_bytes(t).numpy().tobytes() == bytes(t)


# ---------------------------------------------------------------- labels
def test_map_labels_and_round_trip():
    from datasets.letterbox import letterbox_geometry, map_labels, unmap_labels
    geom = letterbox_geometry(480, 640, 640, 640)
    got = map_labels([[0.0, 0.0, 1.0, 1.0], [0.25, 0.5, 0.75, 1.0]], geom, 640, 640)
    assert got.dtype == np.float64
    assert np.array_equal(got, [[0.0, 0.125, 1.0, 0.875], [0.25, 0.5, 0.75, 0.875]])
    rng = np.random.default_rng(1)
    for _ in range(200):
        h0, w0, S = (int(v) for v in rng.integers(1, 900, 3))
        geom = letterbox_geometry(h0, w0, S, S)
        b = np.sort(rng.uniform(0, 1, (5, 2, 2)), axis=1).reshape(5, 4)
        m = map_labels(b, geom, S, S)
        assert (m >= 0).all() and (m <= 1).all()
        nw, nh, left, top = geom                           # the frame box lies in the interior rectangle
        assert (m[:, [0, 2]] * S >= left - 1e-9).all() and (m[:, [0, 2]] * S <= left + nw + 1e-9).all()
        assert (m[:, [1, 3]] * S >= top - 1e-9).all() and (m[:, [1, 3]] * S <= top + nh + 1e-9).all()
        # fp64 each way: a few ulp of values of at most S, taken back by a division by at least 1
        assert np.abs(unmap_labels(m, geom, S, S) - b).max() <= 8 * S * np.finfo(np.float64).eps


# ---------------------------------------------------------------- collate
def _items():
    rng = np.random.default_rng(3)
    items = []
    for i, (h, w) in enumerate(((8, 6), (5, 9), (16, 16))):
        im = torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        boxes = torch.tensor([[0.5, 0.5, 0.2, 0.4]] * (i + 1), dtype=torch.float32) if i < 2 else torch.zeros((0, 4))
        items.append((im, boxes, torch.full((len(boxes),), i, dtype=torch.long), i))
    return items


def test_collate_with_and_without_letterbox():
    from datasets import collate_fn_cuda
    from datasets.letterbox import map_labels
    items = _items()
    base = collate_fn_cuda(items, img_size=16, channels=3)
    same = collate_fn_cuda(items, img_size=16, channels=3, letterbox=False)
    assert list(base) == ["img_u8", "img_meta", "img_size", "img_ch", "batch_idx", "cls", "bboxes"] == list(same)
    assert base["img_meta"].tolist() == [[0, 8, 6], [144, 5, 9], [279, 16, 16]] and base["img_size"] == 16
    assert base["batch_idx"].tolist() == [0, 1, 1] and base["cls"].reshape(-1).tolist() == [0, 1, 1]
    assert torch.allclose(base["bboxes"], torch.tensor([[0.4, 0.3, 0.6, 0.7]] * 3))
    for k in base:
        assert torch.equal(base[k], same[k]) if isinstance(base[k], torch.Tensor) else base[k] == same[k], k
    lb = collate_fn_cuda(items, img_size=16, channels=3, letterbox=True)
    assert list(lb) == ["img_u8", "img_meta", "img_size", "img_ch", "img_lb", "batch_idx", "cls", "bboxes"]
    assert lb["img_lb"].dtype == torch.int32 and lb["img_lb"].tolist() == [[12, 16, 2, 0], [16, 9, 0, 3], [16, 16, 0, 0]]
    for k in ("img_u8", "img_meta", "batch_idx", "cls"):
        assert torch.equal(lb[k], base[k]), k
    want = np.concatenate([map_labels(base["bboxes"][:1].numpy(), (12, 16, 2, 0), 16, 16),
                           map_labels(base["bboxes"][1:].numpy(), (16, 9, 0, 3), 16, 16)]).astype(np.float32)
    assert lb["bboxes"].dtype == torch.float32 and np.array_equal(lb["bboxes"].numpy(), want)
    one = [(torch.zeros(1, 4, 8, dtype=torch.uint8), torch.zeros((0, 4)), torch.zeros((0,), dtype=torch.long), 0)]
    got = collate_fn_cuda(one, img_size=16, letterbox=True)
    assert "img_ch" not in got and got["img_lb"].tolist() == [[16, 8, 0, 4]] and got["bboxes"].shape == (0, 4)
    with pytest.raises(ValueError):                        # float images are already at their size
        collate_fn_cuda([(torch.zeros(1, 16, 16), torch.zeros((0, 4)), torch.zeros((0,)), 0)], letterbox=True)


# ---------------------------------------------------------------- BatchAugment.plan on a letterboxed batch
HW = [(24, 64), (64, 40), (64, 64), (10, 50)]
OFF = dict(mosaic=0.0, degrees=0.0, translate=0.0, scale=0.0, shear=0.0, fliplr=0.0, flipud=0.0, gain=0.0)


def _lb_batch(S):
    from datasets import collate_fn_cuda
    rng = np.random.default_rng(12)
    ims = [rng.integers(0, 256, (*hw, 1), dtype=np.uint8) for hw in HW]
    items = [(torch.from_numpy(a[..., 0].copy()).unsqueeze(0), torch.tensor([[0.5, 0.5, 0.5, 0.25]]),
              torch.tensor([i % 3]), i) for i, a in enumerate(ims)]
    return collate_fn_cuda(items, img_size=S, letterbox=True), ims


def _interior(table, S):
    m = np.zeros((len(HW), S, S), bool)
    for i in range(len(HW)):
        e = table[i]
        m[i, e.top:e.top + e.nh, e.left:e.left + e.nw] = True
    return m


def test_plan_plain_entries_equal_the_letterbox_within_one_level():
    from datasets.augment import AugmentHyp, BatchAugment
    S = 64
    batch, ims = _lb_batch(S)
    table, bi, cl, bb, max_gt = BatchAugment(AugmentHyp(**OFF), seed=2).plan(batch, 1, 0)
    assert all(table[i].flags == 0 for i in range(len(HW)))           # unflagged: the flag means the S x S stretch
    got = AR.render(table, [a[..., 0] for a in ims], S).astype(np.int64)
    lbt = LR.entries(ims, S, S)
    want = LR.render(lbt, ims, S, S, 114)[:, 0].astype(np.int64)
    inside = _interior(lbt, S)
    assert inside.any() and (~inside).any()
    assert (got[~inside] == 114).all() and (want[~inside] == 114).all()
    # the 24-bit fixed-point sampler against the float coefficient rule: the weights differ by at most 1 / 2048 each
    # way, one level after the blend
    worst = int(np.abs(got - want)[inside].max())
    print(f"plain letterboxed entries: worst difference {worst} level(s), {(got != want).mean():.4f} of the pixels")
    assert worst <= 1
    assert np.array_equal(got[2], want[2])                            # the 64 x 64 image: integer positions, a copy
    # the labels are the collate's, already in the letterboxed frame
    assert torch.equal(bi, batch["batch_idx"]) and torch.equal(bb, batch["bboxes"]) and max_gt == 1
    # without the key the plan is what it always was: stretch-flagged entries
    plain = {k: v for k, v in batch.items() if k != "img_lb"}
    t2 = BatchAugment(AugmentHyp(**OFF), seed=2).plan(plain, 1, 0)[0]
    assert all(t2[i].flags == 1 for i in range(len(HW)))


@pytest.mark.parametrize("step", [0, 1, 2])
def test_plan_mosaic_seam_cuts_padded_bands(step):
    """No affine, no flip: the output is the window [S/2, 3S/2)^2 of the 2S canvas, so the seam is in view and the
    pads of the four letterboxed tiles meet along it."""
    from datasets.augment import AugmentHyp, BatchAugment, mosaic_origins
    S = 64
    batch, ims = _lb_batch(S)
    aug = BatchAugment(AugmentHyp(**{**OFF, "mosaic": 1.0}), seed=7)
    table = aug.plan(batch, 1, step)[0]
    p = aug.draw(len(HW), 1, step)
    got = AR.render(table, [a[..., 0] for a in ims], S).astype(np.int64)
    lbt = LR.entries(ims, S, S)
    frames = LR.render(lbt, ims, S, S, 114)[:, 0].astype(np.int64)
    inside = _interior(lbt, S)
    y, x = np.meshgrid(np.arange(S) + S // 2, np.arange(S) + S // 2, indexing="ij")      # canvas pixel of each output
    for i in range(len(HW)):
        xc, yc = (int(S / 2 + c * S) for c in (p["cx"][i], p["cy"][i]))
        srcs = [i, *(int(b) for b in p["partners"][i])]
        slot = (x >= xc).astype(int) + 2 * (y >= yc).astype(int)
        want = np.full((S, S), 114, np.int64)
        shown = np.zeros((S, S), bool)
        for k, ((ox, oy), b) in enumerate(zip(mosaic_origins(xc, yc, S), srcs)):
            own = slot == k
            want[own] = frames[b][y[own] - oy, x[own] - ox]
            shown[own] = inside[b][y[own] - oy, x[own] - ox]
        assert (got[i][~shown] == 114).all(), i
        assert int(np.abs(got[i] - want)[shown].max(initial=0)) <= 1, i
        assert shown.any() and (~shown).any()
        assert len({int(s) for s in np.unique(slot)}) >= 2            # the seam is in view


# ---------------------------------------------------------------- flags
def test_trainer_and_predict_flags(capsys):
    import inspect
    import train_yolo11_cuda as T
    ap = T.build_parser()
    assert ap.parse_args([]).letterbox is False
    assert ap.parse_args(["--letterbox"]).letterbox is True
    assert ap.parse_args(["--letterbox", "--data-format", "yolo", "--ch", "3"]).letterbox is True
    with pytest.raises(SystemExit):
        ap.parse_args(["--letterbox", "--synthetic", "4"])
    capsys.readouterr()
    assert inspect.signature(T.make_loaders).parameters["letterbox"].default is False
    assert inspect.signature(T.load_checkpoint).parameters["ema"].default is False
    import predict as P
    a = P.build_parser().parse_args(["--weights", "w.pt", "--source", "d"])
    assert (a.scale, a.ch, a.nc, a.imgsz, a.batch, a.conf, a.iou, a.max_det, a.ema) == ("s", 1, 5, 640, 8, 0.25, 0.45,
                                                                                       300, False)
    with pytest.raises(SystemExit):
        P.build_parser().parse_args(["--source", "d"])
    capsys.readouterr()
    rows = P.txt_rows({"boxes": torch.tensor([[10.0, 20.0, 30.0, 60.0]]), "scores": torch.tensor([0.5]),
                       "labels": torch.tensor([2])}, 80, 40)
    assert rows == ["2 0.500000 0.500000 0.500000 0.500000 0.500000"]
