"""Sliced inference without a GPU: the window plan (datasets/slicing.py) against worked values and, over random
inputs, against properties and the restatement (tests/slice_ref.py); the table's layout, edge bits, whole-image entry
and tile_begin; ym_slice_letterbox_u8c's per-pixel function (include/yolomi_augment.h: ym_tile_sample_c) built for the
host with the address and undefined-behaviour sanitizers as a stand-alone program and held byte for byte to
letterbox_ref.render applied to numpy crops; the restatement of the decode's inputs; the predict CLI's flags."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

import letterbox_ref as LR
import slice_ref as SR
from conftest import ROOT


# ---------------------------------------------------------------- the plan
def _starts(wins, k):
    return sorted({w[k] for w in wins})


def test_worked_window_table():
    from datasets.slicing import slice_step, slice_windows
    assert slice_step(640, 0.2) == (128, 512)
    assert _starts(slice_windows(1080, 1920, 640, 0.2), 0) == [0, 512, 1024, 1280]
    assert _starts(slice_windows(1080, 1920, 640, 0.2), 1) == [0, 440]
    assert len(slice_windows(1080, 1920, 640, 0.2)) == 8
    assert _starts(slice_windows(641, 641, 640, 0.2), 0) == [0, 1]
    assert slice_windows(640, 640, 640, 0.2) == [(0, 0, 640, 640)]
    assert slice_windows(100, 640, 640, 0.2) == [(0, 0, 640, 100)]
    assert slice_windows(100, 100, 640, 0.2) == [(0, 0, 100, 100)]
    # row-major, y outer; the last window of each axis shifted back inside
    assert slice_windows(1080, 1920, 640, 0.2) == [(x, y, 640, 640) for y in (0, 440) for x in (0, 512, 1024, 1280)]
    assert slice_windows(0, 50, 32, 0.2) == [] and slice_windows(50, 0, 32, 0.2) == []
    # tile * overlap = k + 0.5 rounds up: 0.25 * 30 = 7.5 -> 8
    assert slice_step(30, 0.25) == (8, 22) and slice_step(32, 0.0) == (0, 32)


def test_window_properties_over_random_plans():
    from datasets.slicing import slice_step, slice_windows
    rng = np.random.default_rng(0)
    multi = 0
    for _ in range(2000):
        h0, w0 = (int(v) for v in rng.integers(1, 400, 2))
        tile = int(rng.integers(1, 200))
        overlap = float(rng.choice([0.0, 0.1, 0.2, 0.25, 0.5, rng.uniform(0.0, 0.9)]))
        if SR.overlap_px(tile, overlap) >= tile:
            continue
        ov, step = slice_step(tile, overlap)
        assert ov == SR.overlap_px(tile, overlap) and step == tile - ov >= 1
        wins = slice_windows(h0, w0, tile, overlap)
        assert wins == SR.windows(h0, w0, tile, overlap)
        cover = np.zeros((h0, w0), bool)
        for x0, y0, tw, th in wins:
            assert 0 <= x0 and 0 <= y0 and x0 + tw <= w0 and y0 + th <= h0 and tw >= 1 and th >= 1
            assert tw == min(tile, w0) and th == min(tile, h0)
            cover[y0:y0 + th, x0:x0 + tw] = True
        assert cover.all()
        for k, L in ((0, w0), (1, h0)):
            st = _starts(wins, k)
            assert len(wins) == len(_starts(wins, 0)) * len(_starts(wins, 1))
            assert st[0] == 0 and (L <= tile or st[-1] == L - tile)
            for a, b in zip(st, st[1:]):                   # neighbours share at least ov pixels, and move forward
                assert 0 < b - a <= step and a + tile - b >= ov
            multi += len(st) > 2
    assert multi > 500


def test_argument_errors():
    from datasets.slicing import slice_windows, tile_table
    for tile, overlap in ((0, 0.2), (-4, 0.2), (32, -0.1), (32, 1.0), (32, 0.99), (1, 0.5), (32, float("nan"))):
        with pytest.raises(ValueError):
            slice_windows(100, 100, tile, overlap)
        with pytest.raises(ValueError):
            tile_table([(100, 100)], tile, overlap, 64)
    assert len(slice_windows(100, 100, 1, 0.49)) == 100 * 100          # ov = 0: a step remains


def test_tile_table_layout_and_values():
    from datasets.letterbox import letterbox_geometry
    from datasets.slicing import tile_bytes, tile_table
    from yolomi._lib import TileEntry
    assert ctypes.sizeof(TileEntry) == 48
    assert [(n, getattr(TileEntry, n).offset) for n, _ in TileEntry._fields_] == [
        ("src", 0), ("x0", 4), ("y0", 8), ("tw", 12), ("th", 16), ("nw", 20), ("nh", 24), ("left", 28), ("top", 32),
        ("edges", 36), ("sx", 40), ("sy", 44)]
    hws = [(50, 70), (0, 9), (33, 33), (20, 30)]
    S = 64
    table, begin = tile_table(hws, 32, 0.25, S)
    # 50 x 70: y 0, 18; x 0, 24, 38 -> 6 windows + the whole image; no pixels: none; 33 x 33: 4 + 1; 20 x 30: 1 + 1
    assert begin == [0, 7, 7, 12, 14] and len(table) == 14
    want, wbegin = SR.entries(hws, 32, 0.25, S)
    assert wbegin == begin and bytes(table) == bytes(SR.as_table(want))
    got = [(e.src, e.x0, e.y0, e.tw, e.th, e.edges) for e in table]
    assert got[:7] == [(0, 0, 0, 32, 32, 2 | 8), (0, 24, 0, 32, 32, 1 | 2 | 8), (0, 38, 0, 32, 32, 1 | 8),
                       (0, 0, 18, 32, 32, 2 | 4), (0, 24, 18, 32, 32, 1 | 2 | 4), (0, 38, 18, 32, 32, 1 | 4),
                       (0, 0, 0, 70, 50, 0)]
    assert got[7:12] == [(2, 0, 0, 32, 32, 2 | 8), (2, 1, 0, 32, 32, 1 | 8), (2, 0, 1, 32, 32, 2 | 4),
                         (2, 1, 1, 32, 32, 1 | 4), (2, 0, 0, 33, 33, 0)]
    assert got[12:] == [(3, 0, 0, 30, 20, 0), (3, 0, 0, 30, 20, 0)]
    for e in table:                                        # the window's own letterbox, and the way back
        assert (e.nw, e.nh, e.left, e.top) == letterbox_geometry(e.th, e.tw, S, S)
        assert np.float32(e.sx) == np.float32(e.tw) / np.float32(e.nw)
        assert np.float32(e.sy) == np.float32(e.th) / np.float32(e.nh)
    assert (table[6].nw, table[6].nh, table[6].left, table[6].top) == (64, 46, 0, 9)
    nofull, b2 = tile_table(hws, 32, 0.25, S, full=False)
    assert b2 == [0, 6, 6, 10, 11] and [e.src for e in nofull] == [0] * 6 + [2] * 4 + [3]
    assert bytes(nofull)[:6 * 48] == bytes(table)[:6 * 48]
    empty, b3 = tile_table([(0, 0)], 32, 0.25, S)
    assert b3 == [0, 0] and empty[0].src == -1
    # the packer: n entries as they are, then src = -1 entries up to pad_to
    tb = tile_bytes(table, 14, 16)
    assert tb.dtype.is_floating_point is False and tb.numel() == 16 * 48
    assert tb.numpy()[:14 * 48].tobytes() == bytes(table)
    pad = (TileEntry * 2).from_buffer_copy(tb.numpy()[14 * 48:].tobytes())
    assert all(e.src == -1 and (e.tw, e.th, e.nw, e.nh, e.edges) == (0, 0, 0, 0, 0) for e in pad)
    assert tile_bytes(table, 3).numel() == 3 * 48 and tile_bytes(table, 14, 8).numel() == 14 * 48


# ---------------------------------------------------------------- the image
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("slhost") / "slice_host"
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "slice_host.cpp"), "-o", str(exe)], check=True)
    return exe


@pytest.mark.parametrize("H,W", SR.FRAMES)
@pytest.mark.parametrize("ch", [1, 2, 3, 4])
def test_host_build_equals_crops_through_the_letterbox(host_program, tmp_path, H, W, ch):
    ims = SR.sources(ch)
    ents, names, _ = SR.render_cases(H, W)
    for fill in (0, 114, 255):
        got = SR.run_host(host_program, tmp_path, ents, ims, H, W, fill)
        want = SR.render(ents, ims, H, W, fill)
        for k, name in enumerate(names):
            assert np.array_equal(got[k], want[k]), (name, fill, int((got[k] != want[k]).sum()))
    # the cases are not degenerate: copies and resizes both occur, windows touch the last row and column, the
    # entries that must show only the fill do, and the others show the image
    copies = [e for e in ents if SR.valid(e, ims) and (e.nw, e.nh) == (e.tw, e.th)]
    resized = [e for e in ents if SR.valid(e, ims) and (e.nw, e.nh) != (e.tw, e.th)]
    assert len(copies) >= 8 and len(resized) >= 5
    assert any(e.x0 + e.tw == 70 and e.y0 + e.th == 50 for e in copies)
    assert any(e.x0 + e.tw == 70 and e.y0 + e.th == 50 and e.tw < 32 for e in resized)
    for k, name in enumerate(names):
        fill_only = name.startswith(("leaves", "negative", "no-src", "src-past", "zero"))
        assert (want[k] == 255).all() == fill_only, name
    e = ents[0]                                            # the first window: the copy of its pixels
    assert np.array_equal(np.moveaxis(want[0][:, e.top:e.top + 32, e.left:e.left + 32], 0, -1), ims[0][:32, :32])
    # an interior window that is resized stops at its own last column: it equals the letterbox of the crop alone
    k = names.index("interior-up")
    crop = np.ascontiguousarray(ims[0][5:18, 3:23])
    assert np.array_equal(want[k], LR.render(LR.entries([crop], H, W), [crop], H, W, 255)[0])


# ---------------------------------------------------------------- the decode's inputs (the reference alone)
def test_decode_case_inputs_meet_their_conditions():
    """What tests/test_gpu_slice.py needs of its inputs holds for the restatement, before any GPU runs."""
    for shape, C, hole in (("small", 5, False), ("small", 80, False), ("small", 5, True), ("large", 5, False)):
        conf = 0.5 if shape == "small" else 0.001
        p = SR.decode_pred(shape, C, hole)
        best = p[..., 4:].max(-1)
        assert len(np.unique(best)) == best.size
        e0 = SR.decode_ref(shape, C, hole, conf, 0.45, True, 0, 0.0)
        e4 = SR.decode_ref(shape, C, hole, conf, 0.45, True, 0, 4.0)
        for out in (e0, e4):
            assert all(len(o["scores"]) >= 1 for o in out)
        assert sum(SR.cross_tile_suppressions(o, 0.45, True) for o in e0) >= 1
        assert all(sum(o["cut"][k] for o in e4) >= 1 for k in range(4)), [o["cut"] for o in e4]
        assert sum(o["clamped"] for o in e0) >= 1
        assert all(sum(o["cut"]) == 0 for o in e0)


# ---------------------------------------------------------------- flags
def test_predict_flags(capsys):
    import inspect
    import predict as P
    from yolomi.predict import Predictor
    base = ["--weights", "w.pt", "--source", "d"]
    a = P.parse_args(base)
    assert (a.slice, a.slice_overlap, a.slice_full, a.slice_edge, a.rect) == (0, 0.2, True, 0.0, False)
    a = P.parse_args(base + ["--slice", "640", "--slice-overlap", "0.3", "--no-slice-full", "--slice-edge", "4"])
    assert (a.slice, a.slice_overlap, a.slice_full, a.slice_edge) == (640, 0.3, False, 4.0)
    for bad in (["--slice", "640", "--rect"], ["--slice", "-1"], ["--slice", "x"]):
        with pytest.raises(SystemExit):
            P.parse_args(base + bad)
    capsys.readouterr()
    assert P.parse_args(base + ["--rect"]).rect is True
    sig = inspect.signature(Predictor.__init__).parameters
    assert [sig[k].default for k in ("slice", "slice_overlap", "slice_full", "slice_edge")] == [0, 0.2, True, 0.0]
