"""Test-time augmentation without a GPU: the view planner (datasets/tta.py) against worked values, against
datasets.slicing.tile_table and, over random plans, against the restatement (tests/tta_ref.py); ym_tile_sample_c with
the mirror bits, built for the host with the address and undefined-behaviour sanitizers as a stand-alone program and
held byte for byte to the reversed restatement; the fixed-point weighted mean (tta_ref.nmw) on the worked example,
against nmm_ref and inside its derived bound; the conditions the GPU tests' inputs must meet so that they cannot pass
vacuously; and what needs no GPU of the library, the parser and the signatures."""
import ctypes
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import nmm_ref as MR
import slice_ref as SR
import tta_ref as TR
from conftest import ROOT

F32 = np.float32


# ---------------------------------------------------------------- the planner
def test_parse_views():
    from datasets.tta import DEFAULT_VIEWS, parse_views
    assert parse_views("1,0.83:lr,0.67") == [(1.0, ""), (0.83, "lr"), (0.67, "")] == list(DEFAULT_VIEWS)
    assert parse_views(" 1 , 0.5:ud,0.25:lrud ") == [(1.0, ""), (0.5, "ud"), (0.25, "lrud")]
    assert parse_views("1") == [(1.0, "")] and parse_views("0.5:lr") == [(0.5, "lr")]
    assert parse_views("1,0.83:lr,0.67") == TR.views("1,0.83:lr,0.67")
    for bad in ("", ",", "1,", "0", "-0.5", "1.01", "2", "nan", "x", "1:", "1:rl", "1:LR", "1:lr:ud", "0.5;lr", "1 0.5",
                None, 1.0):
        with pytest.raises(ValueError):
            parse_views(bad)


def test_worked_view_table():
    from datasets.tta import DEFAULT_VIEWS, view_table
    table, begin = view_table([(50, 70)], DEFAULT_VIEWS, 32)
    assert begin == [0, 3] and len(table) == 3
    got = [(e.src, e.x0, e.y0, e.tw, e.th, e.nw, e.nh, e.left, e.top, e.edges) for e in table]
    assert got == [(0, 0, 0, 70, 50, 32, 23, 0, 4, 0), (0, 0, 0, 70, 50, 27, 19, 2, 6, 16),
                   (0, 0, 0, 70, 50, 21, 15, 5, 8, 0)]
    for e, nw, nh in zip(table, (32, 27, 21), (23, 19, 15)):
        assert F32(e.sx) == F32(70) / F32(nw) and F32(e.sy) == F32(50) / F32(nh)
    # with windows: view-major, the edge bits of the windows beside the mirror bits
    table, begin = view_table([(50, 70), (0, 9), (20, 30)], [(1, ""), (0.5, "lrud")], 32, tile=32, overlap=0.25)
    assert begin == [0, 14, 14, 18] and len(table) == 18
    e = [(x.x0, x.y0, x.tw, x.th, x.edges) for x in table]
    plain = [(0, 0, 32, 32, 2 | 8), (24, 0, 32, 32, 1 | 2 | 8), (38, 0, 32, 32, 1 | 8), (0, 18, 32, 32, 2 | 4),
             (24, 18, 32, 32, 1 | 2 | 4), (38, 18, 32, 32, 1 | 4), (0, 0, 70, 50, 0)]
    assert e[:7] == plain and e[7:14] == [(*w[:4], w[4] | 48) for w in plain]
    assert e[14:] == [(0, 0, 30, 20, 0)] * 2 + [(0, 0, 30, 20, 48)] * 2
    assert [(x.nw, x.nh, x.left, x.top) for x in table[7:9]] == [(16, 16, 8, 8)] * 2
    assert [x.src for x in table] == [0] * 14 + [2] * 4
    empty, b = view_table([(0, 0)], DEFAULT_VIEWS, 32)
    assert b == [0, 0] and empty[0].src == -1


def test_one_plain_view_is_tile_table():
    from datasets.slicing import tile_table
    from datasets.tta import view_table
    hws = [(50, 70), (0, 9), (33, 33), (20, 30)]
    for S in (32, 64):
        a, ba = view_table(hws, [(1, "")], S)
        b, bb = tile_table(hws, 128, 0.2, S, full=False)
        assert ba == bb and bytes(a) == bytes(b)
        for full in (True, False):
            a, ba = view_table(hws, [(1.0, "")], S, tile=32, overlap=0.25, full=full)
            b, bb = tile_table(hws, 32, 0.25, S, full=full)
            assert ba == bb and bytes(a) == bytes(b)


def test_small_scale_keeps_a_pixel():
    from datasets.tta import view_table
    table, _ = view_table([(50, 70), (1, 400)], [(0.01, "lr")], 32)
    assert [(e.nw, e.nh) for e in table] == [(1, 1), (1, 1)]
    assert [(e.left, e.top) for e in table] == [(15, 15)] * 2
    assert F32(table[0].sx) == F32(70) and F32(table[1].sy) == F32(1)


def test_view_errors():
    from datasets.tta import view_table
    for views in ([], [(0, "")], [(1.5, "")], [(1, "rl")], [(1,)], [1.0], [(float("nan"), "")], [("a", "")]):
        with pytest.raises(ValueError):
            view_table([(50, 70)], views, 32)
    with pytest.raises(ValueError):
        view_table([(50, 70)], [(1, "")], 32, tile=-1)
    with pytest.raises(ValueError):
        view_table([(50, 70)], [(1, "")], 32, tile=32, overlap=1.0)


def test_view_table_over_random_plans():
    from datasets.tta import FLIPS, view_table
    assert FLIPS == TR.FLIP_BITS
    rng = np.random.default_rng(27)
    flips = list(FLIPS)
    reduced = 0
    for _ in range(2000):
        hws = [tuple(int(v) for v in rng.integers(0, 200, 2)) for _ in range(int(rng.integers(1, 4)))]
        vws = [(float(rng.choice([1.0, 0.83, 0.67, 0.5, rng.uniform(0.01, 1.0)])), flips[int(rng.integers(0, 4))])
               for _ in range(int(rng.integers(1, 4)))]
        S = int(rng.choice([32, 48, 64]))
        tile = int(rng.choice([0, 0, 32, 50]))
        full = bool(rng.integers(0, 2))
        table, begin = view_table(hws, vws, S, tile, 0.25, full)
        want, wbegin = TR.view_entries(hws, vws, S, tile, 0.25, full)
        assert begin == wbegin
        if want:
            assert bytes(table) == bytes(SR.as_table(want))
        for g in range(len(hws)):
            n = begin[g + 1] - begin[g]
            assert n % len(vws) == 0
            per = n // len(vws)
            for k in range(n):
                e = table[begin[g] + k]
                s, f = vws[k // per]                       # view-major
                first = table[begin[g] + k % per]          # the same window in view 0
                assert (e.src, e.x0, e.y0, e.tw, e.th) == (g, first.x0, first.y0, first.tw, first.th)
                assert e.edges & 15 == first.edges & 15 and e.edges >> 4 == FLIPS[f] >> 4
                assert 1 <= e.nw <= S and 1 <= e.nh <= S and e.left >= 0 and e.top >= 0
                assert e.left + e.nw <= S and e.top + e.nh <= S
                assert abs(2 * e.left + e.nw - S) <= 1 and abs(2 * e.top + e.nh - S) <= 1      # centred
                reduced += e.nw < first.nw or s == 1.0
    assert reduced > 2000


# ---------------------------------------------------------------- the image
BITS = (0, 16, 32, 48)


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("ttahost") / "tta_host"
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "tta_host.cpp"), "-o", str(exe)], check=True)
    return exe


@pytest.mark.parametrize("H,W", SR.FRAMES)
@pytest.mark.parametrize("ch", [1, 2, 3, 4])
def test_host_build_equals_the_reversed_restatement(host_program, tmp_path, H, W, ch):
    ims = SR.sources(ch)
    ents, names, _ = SR.render_cases(H, W)
    fill = 255
    SR.write_case_file(tmp_path / "cases.bin", ents, ims, H, W, fill)
    subprocess.run([str(host_program), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], check=True, timeout=120)
    got = np.fromfile(tmp_path / "out.bin", dtype=np.uint8).reshape(4, len(ents), ch, H, W)
    plain = SR.render(ents, ims, H, W, fill)
    differ = np.zeros(4, int)
    for m, bits in enumerate(BITS):
        want = TR.render([TR.with_bits(e, bits) for e in ents], ims, H, W, fill)
        for k, name in enumerate(names):
            assert np.array_equal(got[m, k], want[k]), (bits, name, int((got[m, k] != want[k]).sum()))
            fill_only = name.startswith(("leaves", "negative", "no-src", "src-past", "zero"))
            assert (got[m, k] == 255).all() == fill_only, (bits, name)
            differ[m] += not np.array_equal(want[k], plain[k])
    # bits clear: slice_ref's tiles; every other setting changes every tile that shows more than one pixel
    shows = sum(SR.valid(e, ims) and e.nw * e.nh > 1 for e in ents)
    assert differ[0] == 0 and (differ[1:] >= shows - 1).all() and shows >= 13, (differ, shows)
    copies = [e for e in ents if SR.valid(e, ims) and (e.nw, e.nh) == (e.tw, e.th)]
    resized = [e for e in ents if SR.valid(e, ims) and (e.nw, e.nh) != (e.tw, e.th)]
    assert len(copies) >= 8 and len(resized) >= 5
    assert {"interior-up", "interior-down", "corner", "no-src", "src-past"} <= set(names)
    # a copy window mirrored in x: the crop's columns reversed
    e = ents[0]
    assert np.array_equal(np.moveaxis(got[1, 0][:, e.top:e.top + 32, e.left:e.left + 32], 0, -1), ims[0][:32, 31::-1])
    assert np.array_equal(np.moveaxis(got[3, 0][:, e.top:e.top + 32, e.left:e.left + 32], 0, -1),
                          ims[0][31::-1, 31::-1])


# ---------------------------------------------------------------- the mean
A, B, C_, D, E = (0, 0, 10, 10), (2, 2, 8, 8), (8, 0, 20, 10), (9, 1, 12, 11), (9, 10, 12, 11)
EX = np.array([A, B, C_, D, E], F32)
EX_SCORES = np.array([0.9, 0.8, 0.7, 0.6, 0.5], F32)


def test_worked_mean():
    assert [TR.q_of(s) for s in EX_SCORES] == [3686, 3277, 2867, 2458, 2048]
    assert [TR.q_of(s) for s in (0.0, -1.0, 1e-5, 1.0, 7.0, 2.0 ** -13, 3 * 2.0 ** -13)] == [1, 1, 1, 4096, 4096, 1, 2]
    assert [TR.c_of(v) for v in (0.0, 1.0, -1.0, 1 / 64, 3 / 64, 2.0 ** 21, -2.0 ** 21, 0.1)] == [
        0, 32, -32, 0, 2, 2 ** 25, -2 ** 25, 3]
    lab = np.zeros(5, np.int64)
    r = TR.nmw(EX, EX_SCORES, lab, 0.5, "ios")
    assert r["keep"].tolist() == [0, 2, 4] and r["merged"].tolist() == [1, 1, 0] and r["by"].tolist() == [-1, 0, -1, 1, -1]
    # A absorbs B: (3686 a + 3277 b) / 6963; C absorbs D: (2867 c + 2458 d) / 5325; E alone keeps its box
    want0 = [F32(float(Fraction(3686 * a + 3277 * b, 6963))) for a, b in zip(A, B)]
    want1 = [F32(float(Fraction(2867 * c + 2458 * d, 5325))) for c, d in zip(C_, D)]
    assert r["boxes"].tolist() == [want0, want1, list(map(float, E))]
    assert r["boxes"][2].tobytes() == EX[4].tobytes()
    assert np.allclose(r["boxes"][0], [0.9412, 0.9412, 9.0588, 9.0588], atol=1e-4)
    # IoU at 0.5 merges nothing: every box as stored
    r = TR.nmw(EX, EX_SCORES, lab, 0.5, "iou")
    assert r["keep"].tolist() == [0, 1, 2, 3, 4] and r["boxes"].tobytes() == EX.tobytes()
    # matching is against the head's own box, never the running mean: E does not touch C's box
    r = TR.nmw(EX, EX_SCORES, np.array([0, 1, 0, 0, 0]), 0.5, "ios", class_aware=True, max_det=1)
    assert r["keep"].tolist() == [0] and r["merged"].tolist() == [0] and r["boxes"].tobytes() == EX[:1].tobytes()


def test_sums_fit_int64_at_the_accepted_limits():
    """|q c| <= 2^12 * 2^25 = 2^37, fewer than 2^26 terms: |S_j| < 2^63, and S_q < 2^38."""
    assert TR.q_of(1.0) * abs(TR.c_of(-2.0 ** 30)) * (TR.MAX_R - 1) < 2 ** 63
    assert TR.q_of(1.0) * abs(TR.c_of(2.0 ** 30)) * TR.MAX_R >= 2 ** 63        # the bound on R is the tight power of two
    assert TR.q_of(1.0) == 2 ** TR.QS and TR.c_of(2.0 ** 30) == 2 ** 25


MEAN_INPUTS = [("small", 5), ("small", 80), ("large", 5), ("global", 5)]
MODES = {"agnostic": (False, 0), "aware": (True, 0), "capped": (True, None)}


def _cap(shape, mode):
    return 0 if mode != "capped" else (2 if shape == "small" else 40)


@pytest.mark.parametrize("shape,C", MEAN_INPUTS)
def test_mean_properties_and_bound(shape, C):
    far = 0
    for mode, (class_aware, _) in MODES.items():
        if shape == "global" and mode != "agnostic":
            continue
        for metric in ("iou", "ios"):
            max_det = _cap(shape, mode)
            got = TR.mean_ref(shape, C, metric, class_aware, max_det)
            head = TR.mean_ref(shape, C, metric, class_aware, max_det, how="match")
            union = TR.mean_ref(shape, C, metric, class_aware, max_det, how="nmm")
            assert all(len(o["scores"]) >= 1 for o in got)                       # no image is empty
            for o, h, u in zip(got, head, union):
                assert len(np.unique(o["cand_scores"])) == len(o["cand_scores"])  # tie-free
                for key in ("index", "rows", "labels", "merged", "by"):
                    assert np.array_equal(o[key], h[key]), key                   # nmm_ref in everything but the boxes
                assert o["scores"].tobytes() == h["scores"].tobytes()
                alone = o["merged"] == 0
                assert o["boxes"][alone].tobytes() == h["boxes"][alone].tobytes()
                conf = TR.MEAN_CONF[shape]
                assert float(o["cand_scores"].min()) > conf and float(o["cand_scores"].max()) <= 1.0
                cmax = float(np.abs(o["cand_boxes"]).max())
                assert cmax <= TR.CMAX
                bd = TR.bound(conf, o["spread"], o["exact"], o["merged"][:, None] + 1, cmax)
                err = np.abs(o["boxes"].astype(np.float64) - o["exact"])
                assert (err[~alone] <= bd[~alone]).all(), float((err - bd).max())
                assert (err[alone] == 0).all()
                # clearly neither the head's box nor the union: the wrong merge mode cannot pass
                d =np.minimum(np.abs(o["boxes"] - h["boxes"]), np.abs(o["boxes"] - u["boxes"]))
                far += int((d > 8 * bd).any(1).sum())
            if metric == "ios" and mode != "capped":
                assert (got[0]["merged"] >= 2).any() and (got[0]["merged"] == 0).any()
                assert far >= 1
    assert far >= 1


# ---------------------------------------------------------------- the mirrored decode case
@pytest.mark.parametrize("C", [5, 80])
def test_mirrored_decode_case_meets_its_conditions(C):
    ents, begin, N = TR.decode_plan()
    assert [e.edges >> 4 for e in ents] == [0, 1, 2, 3, 0, 1] and begin == [0, 4, 6] and N == 17
    p = TR.decode_pred(C)
    best = p[..., 4:].max(-1)
    assert len(np.unique(best)) == best.size                                     # tie-free
    for class_aware in (False, True):
        e0 = TR.decode_ref(C, "nms", "iou", class_aware, 0, 0.0)
        e4 = TR.decode_ref(C, "nms", "iou", class_aware, 0, 4.0)
        for out in (e0, e4):
            assert all(len(o["scores"]) >= 1 for o in out)                       # no image is empty
        assert sum(o["clamped"] for o in e0) >= 1 and all(not o["cut_rows"] for o in e0)
        # a kept box of a mirrored tile removes a candidate of an unmirrored tile of its image, and the other way round
        for o, first in zip(e0, begin):
            mir = np.array([ents[first + int(t)].edges >> 4 != 0 for t in o["cand_tiles"]])
            kept = np.zeros(len(mir), bool)
            kept[o["index"]] = True
            seen = set()
            for c in np.nonzero(~kept)[0]:
                k = o["index"]
                m = (o["cand_scores"][k] > o["cand_scores"][c]) & (mir[k] != mir[c])
                if class_aware:
                    m &= o["cand_labels"][k] == o["cand_labels"][c]
                if m.any() and (SR.iou64(o["cand_boxes"][c], o["cand_boxes"][k[m]]) > TR.DEC_THR + 0.02).any():
                    seen.add(bool(mir[c]))
            assert seen == {False, True}, (first, seen)
    # ignoring the mirror would change the answer: the boxes differ with the bits cleared
    blind = TR.decode_tiles(p, [TR.with_bits(e, 0) for e in ents], begin, TR.DEC_CONF, TR.DEC_THR)
    seen = TR.decode_ref(C, "nms", "iou", False, 0, 0.0)
    assert all(b["boxes"].tobytes() != s["boxes"].tobytes() for b, s in zip(blind, seen))
    # edge = 4: each mirror bit drops a candidate the unmirrored map keeps, and keeps one it drops
    for bit in (TR.MIRROR_X, TR.MIRROR_Y):
        dropped = kept = 0
        for t, e in enumerate(ents):
            if not e.edges & bit:
                continue
            with_bit = set(TR.tile_candidates(p[t], e, TR.DEC_CONF, 4.0)[5].tolist())
            without = set(TR.tile_candidates(p[t], TR.with_bits(e, (e.edges & 48) & ~bit), TR.DEC_CONF, 4.0)[5].tolist())
            dropped += len(with_bit - without)
            kept += len(without - with_bit)
        assert dropped >= 1 and kept >= 1, (bit, dropped, kept)
    # the merging forms see clusters across views
    for metric in ("iou", "ios"):
        o = TR.decode_ref(C, "mean", metric, True, 0, 0.0)
        assert sum(int((x["merged"] >= 1).sum()) for x in o) >= 2


# ---------------------------------------------------------------- without a GPU
def test_library_signatures_and_flags(capsys):
    import inspect
    import predict as P
    from yolomi._lib import SIGNATURES, lib
    from yolomi.predict import Predictor
    assert "ym_decode_nmw_tiles" in SIGNATURES and "ym_decode_nmw_tiles_workspace_size" in SIGNATURES
    assert len(SIGNATURES["ym_decode_nmw_tiles"][1]) == len(SIGNATURES["ym_decode_nmm_tiles"][1]) - 1
    L = lib()
    for G, R in ((1, 1), (2, 85), (3, 10500)):
        base = L.ym_decode_nmm_tiles_workspace_size(G, R, 1)
        got = L.ym_decode_nmw_tiles_workspace_size(G, R, 1)
        assert got == L.ym_decode_nmw_tiles_workspace_size(G, R, 0)
        assert got == base + -(-(G * R * 40) // 256) * 256                      # 5 int64 sums per output slot
    base = ["--weights", "w.pt", "--source", "d"]
    a = P.parse_args(base)
    assert (a.tta, a.tta_views, a.views, a.slice_merge) == (False, None, None, "nms")
    a = P.parse_args(base + ["--tta"])
    assert a.tta is True and a.views == [(1.0, ""), (0.83, "lr"), (0.67, "")]
    a = P.parse_args(base + ["--tta-views", "1,0.83:lr", "--slice-merge", "mean"])
    assert a.tta is True and a.views == [(1.0, ""), (0.83, "lr")] and a.slice_merge == "mean"
    a = P.parse_args(base + ["--tta", "--slice", "640", "--slice-merge", "mean", "--slice-metric", "ios"])
    assert (a.slice, a.slice_merge, a.slice_metric) == (640, "mean", "ios")
    for bad in (["--slice-merge", "mean"], ["--tta", "--rect"], ["--tta-views", "1,2"], ["--tta-views", ""],
                ["--tta-views", "1:rl"], ["--tta", "--slice-merge", "wbf"], ["--slice-metric", "ios"]):
        with pytest.raises(SystemExit):
            P.parse_args(base + bad)
    capsys.readouterr()
    assert inspect.signature(Predictor.__init__).parameters["tta"].default is None
    assert ctypes.sizeof(__import__("yolomi._lib", fromlist=["TileEntry"]).TileEntry) == 48
