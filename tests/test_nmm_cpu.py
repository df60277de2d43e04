"""Greedy box merging with the IoS metric, on the CPU: the restatement (tests/nmm_ref.py) on the worked
example and against the class-aware NMS restatement, its invariants, the conditions that the GPU tests' inputs must
meet so that they cannot pass vacuously, and what needs no GPU of the library, the parser and the signatures."""
import ctypes

import numpy as np
import pytest

import nmm_ref as MR
import nms_cls_ref as NR
import slice_ref as SR

THR = MR.THR
A, B, C_, D, E = (0, 0, 10, 10), (2, 2, 8, 8), (8, 0, 20, 10), (9, 1, 12, 11), (9, 10, 12, 11)
EX = np.array([A, B, C_, D, E], np.float32)
EX_SCORES = np.array([0.9, 0.8, 0.7, 0.6, 0.5], np.float32)


# ---------------------------------------------------------------- the worked example
def test_worked_example():
    lab = np.zeros(5, np.int64)
    r = MR.nmm(EX, EX_SCORES, lab, 0.5, "iou", True)
    assert r["keep"].tolist() == [0, 1, 2, 3, 4] and r["merged"].tolist() == [0] * 5
    assert np.array_equal(r["boxes"], EX)
    r = MR.nmm(EX, EX_SCORES, lab, 0.5, "ios", True)
    assert r["keep"].tolist() == [0, 2, 4] and r["merged"].tolist() == [1, 1, 0]
    assert r["boxes"].tolist() == [[0, 0, 10, 10], [8, 0, 20, 11], [9, 10, 12, 11]]
    assert r["by"].tolist() == [-1, 0, -1, 1, -1]
    # E lies inside C's union and has no intersection with C's own box: the greedy rule
    assert float(MR.match(EX[2], EX[4:5], "ios")[0]) == 0.0
    r0 = MR.nmm(EX, EX_SCORES, lab, 0.5, "ios", False)
    assert r0["keep"].tolist() == [0, 2, 4] and r0["merged"].tolist() == [1, 1, 0]
    assert np.array_equal(r0["boxes"], EX[[0, 2, 4]])


def test_worked_example_class_aware_and_capped():
    lab = np.array([0, 1, 0, 0, 0])                        # B of another label
    r = MR.nmm(EX, EX_SCORES, lab, 0.5, "ios", True, class_aware=True)
    assert r["keep"].tolist() == [0, 1, 2, 4] and r["merged"].tolist() == [0, 0, 1, 0]
    assert r["boxes"].tolist() == [[0, 0, 10, 10], [2, 2, 8, 8], [8, 0, 20, 11], [9, 10, 12, 11]]
    r = MR.nmm(EX, EX_SCORES, np.zeros(5, np.int64), 0.5, "ios", True, class_aware=True, max_det=1)
    assert r["keep"].tolist() == [0] and r["merged"].tolist() == [1] and r["by"].tolist() == [-1, 0, -1, -1, -1]
    # the class-agnostic form ignores the labels
    r = MR.nmm(EX, EX_SCORES, lab, 0.5, "ios", True, class_aware=False)
    assert r["keep"].tolist() == [0, 2, 4]


def test_match_values_of_a_cut_box_and_its_whole_twin():
    whole, part = np.array([3, 3, 53, 53], np.float32), np.array([[24, 24, 53, 53]], np.float32)
    assert float(MR.match(whole, part, "iou")[0]) < 0.45 and float(MR.match(whole, part, "ios")[0]) > 0.99
    assert float(MR.match(whole, whole[None], "iou")[0]) == float(MR.match(whole, whole[None], "ios")[0])


# ---------------------------------------------------------------- the built inputs
INPUTS = [("small", 5), ("small", 80), ("large", 5), ("large", 80), ("global", 5)]
MODES = {"agnostic": (False, 0), "aware": (True, 0)}


@pytest.mark.parametrize("shape,C", INPUTS)
def test_iou_without_merge_is_the_nms_restatement(shape, C):
    ents, begin, N = MR.plan(shape)
    for class_aware, max_det in [(False, 0)] + ([(True, 0), (True, 3)] if shape != "global" else []):
        for edge in (0.0, 4.0):
            got = MR.ref(shape, C, False, "iou", False, class_aware, max_det, edge)
            want = SR.decode_tiles(MR.pred(shape, C), ents, begin, MR.CONF[shape], THR, class_aware, max_det, edge)
            for g, w in zip(got, want):
                assert np.array_equal(g["index"], w["index"]) and g["boxes"].tobytes() == w["boxes"].tobytes()
                assert np.array_equal(g["rows"], w["rows"]) and np.array_equal(g["labels"], w["labels"])
                assert g["scores"].tobytes() == w["scores"].tobytes()
                keep = NR.nms_cls(g["cand_boxes"], g["cand_scores"],
                                  g["cand_labels"] if class_aware else np.zeros_like(g["cand_labels"]), THR, max_det)
                assert np.array_equal(g["index"], keep)


@pytest.mark.parametrize("shape,C", INPUTS)
def test_properties(shape, C):
    for mode, (class_aware, max_det) in MODES.items():
        if shape == "global" and class_aware:
            continue
        for metric in ("iou", "ios"):
            on = MR.ref(shape, C, False, metric, True, class_aware, max_det, 0.0)
            off = MR.ref(shape, C, False, metric, False, class_aware, max_det, 0.0)
            for a, b in zip(on, off):
                # merge changes boxes only
                for key in ("scores", "labels", "index", "rows", "merged", "by"):
                    assert np.array_equal(a[key], b[key]), key
                assert np.array_equal(b["boxes"], a["cand_boxes"][a["index"]])
                # kept + sum of merged = K without a cap
                K = len(a["cand_scores"])
                assert len(a["index"]) + int(a["merged"].sum()) == K
                assert (a["by"][a["index"]] == -1).all() and ((a["by"] >= 0).sum() == a["merged"].sum())
                # every union contains its head and each absorbed box
                for k, i in enumerate(a["index"]):
                    inside = np.concatenate([a["cand_boxes"][i][None], a["cand_boxes"][a["by"] == k]])
                    u = a["boxes"][k]
                    assert (u[:2] <= inside[:, :2]).all() and (u[2:] >= inside[:, 2:]).all()
                    assert u[0] in inside[:, 0] and u[3] in inside[:, 3]
                    if class_aware:
                        assert (a["cand_labels"][a["by"] == k] == a["cand_labels"][i]).all()


@pytest.mark.parametrize("class_aware", [False, True])
@pytest.mark.parametrize("shape,C", [i for i in INPUTS if i[0] != "global"])
def test_input_conditions(shape, C, class_aware):
    """Image 0 at thr 0.5: what the GPU comparison must exercise."""
    best = MR.pred(shape, C)[..., 4:].max(-1)
    assert len(np.unique(best)) == best.size                              # tie-free
    ios = MR.ref(shape, C, False, "ios", True, class_aware, 0, 0.0)[0]
    iou = MR.ref(shape, C, False, "iou", True, class_aware, 0, 0.0)[0]
    tiles, by, idx = ios["cand_tiles"], ios["by"], ios["index"]
    absorbed = np.nonzero(by >= 0)[0]
    assert (tiles[absorbed] != tiles[idx[by[absorbed]]]).any()            # a head absorbs another tile's candidate
    assert (ios["boxes"] != ios["cand_boxes"][idx]).any()                 # a union differs from its head's box
    low = [c for c in absorbed
           if SR.iou64(ios["cand_boxes"][idx[by[c]]], ios["cand_boxes"][c][None])[0] <= THR]
    assert len(low) >= 1                                                  # absorbed at an IoU <= thr
    assert (ios["merged"] >= 2).any()
    assert len(ios["index"]) < len(iou["index"])
    K = len(ios["cand_scores"])
    assert K > 8192 if shape == "large" else K <= 8192
    print(f"{shape} C={C} aware={class_aware}: K={K}, kept IoS {len(idx)} / IoU {len(iou['index'])}, "
          f"{int((ios['boxes'] != ios['cand_boxes'][idx]).any(1).sum())} unions grew, {len(low)} absorbed at IoU <= thr")


def test_input_conditions_global():
    ios = MR.ref("global", 5, False, "ios", True, False, 0, 0.0)[0]
    assert len(ios["cand_scores"]) > 16384
    assert (ios["boxes"] != ios["cand_boxes"][ios["index"]]).any() and (ios["merged"] >= 2).any()


def test_cap_and_hole_inputs():
    """The capped references are cut by the cap; the src = -1 plan loses its tile's rows and keeps the later ones."""
    for shape, cap in (("small", 2), ("large", 40)):
        capped = MR.ref(shape, 5, False, "ios", True, True, cap, 0.0)[0]
        free = MR.ref(shape, 5, False, "ios", True, True, 0, 0.0)[0]
        assert len(capped["index"]) == cap < len(free["index"])
        assert np.array_equal(capped["boxes"], free["boxes"][:cap]) and capped["merged"].sum() >= 1
    _, _, N = MR.plan("small", True)
    hole = MR.ref("small", 5, True, "ios", True, True, 0, 0.0)[0]
    assert not (hole["rows"] // N == 1).any() and (hole["rows"] // N >= 2).any() and hole["merged"].sum() >= 1


# ---------------------------------------------------------------- the library, the parser, the signatures
def test_workspace_size_needs_no_gpu():
    from yolomi._lib import lib
    L = lib()
    for G, R in ((1, 1), (2, 85), (8, 8400 * 29), (0, 0)):
        for cls in (0, 1):
            n = L.ym_decode_nmm_tiles_workspace_size(G, R, cls)
            assert n >= L.ym_decode_nms_tiles_workspace_size(G, R, cls) > 0


def test_signature_entry():
    import yolomi._lib as yl
    res, args = yl.SIGNATURES["ym_decode_nmm_tiles"]
    nres, nargs = yl.SIGNATURES["ym_decode_nms_tiles"]
    assert res is nres and len(args) == len(nargs) + 3
    assert args[:12] == nargs[:12] and args[12:14] == [ctypes.c_int, ctypes.c_int] and args[14:-2] == nargs[12:-1]
    assert args[-2:] == [ctypes.c_void_p, ctypes.c_void_p]
    assert yl.SIGNATURES["ym_decode_nmm_tiles_workspace_size"] == yl.SIGNATURES["ym_decode_nms_tiles_workspace_size"]
    assert hasattr(yl.lib(), "ym_decode_nmm_tiles")


def test_predict_parser_takes_the_flags():
    import predict as P
    base = ["--weights", "w.pt", "--source", "x"]
    a = P.parse_args(base)
    assert (a.slice_merge, a.slice_metric) == ("nms", "iou")
    a = P.parse_args(base + ["--slice", "640", "--slice-merge", "nmm", "--slice-metric", "ios"])
    assert (a.slice, a.slice_merge, a.slice_metric) == (640, "nmm", "ios")
    for bad in (["--slice", "640", "--slice-merge", "wbf"], ["--slice", "640", "--slice-metric", "giou"],
                ["--slice-merge", "nmm"], ["--slice-metric", "ios"]):
        with pytest.raises(SystemExit):
            P.parse_args(base + bad)
