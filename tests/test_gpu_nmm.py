"""Greedy box merging over tiles on the GPU (ym_decode_nmm_tiles), bit for bit against the numpy
restatement (tests/nmm_ref.py, whose inputs tests/test_nmm_cpu.py holds to the conditions that make the comparison
mean something): two shapes (the register form and K > 8192), two class counts (the thread and wave rowmax kernels), two
layouts of `pred`, both metrics, merge off and on, the three modes, with and without the tile-border filter, a
src = -1 tile, and K > 16384 once; IoU without merge against ym_decode_nms_tiles; the argument checks;
Predictor(slice_merge=..., slice_metric=...) against the hand composition and the restatement; the command line."""
import ctypes
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import augment_ref as AR
import nmm_ref as MR
import slice_ref as SR

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
THR = MR.THR


def _tensor(pred, layout):
    p = torch.from_numpy(np.array(pred)).cuda()
    if layout == "anchor-major":                           # the eval output's (T, 4 + C, N), read through a view
        p = p.permute(0, 2, 1).contiguous().transpose(1, 2)
        assert p.stride(2) == pred.shape[1] and p.stride(1) == 1
    return p


def _decode(pred, ents, begin, conf, metric, merge, class_aware, max_det, edge, layout="contiguous", thr=THR):
    from yolomi import post
    tdev = torch.from_numpy(SR.table_bytes(ents)).cuda()
    return post.decode_nmm_tiles(_tensor(pred, layout), tdev, begin, conf, thr, metric=metric, merge=merge,
                                 class_aware=class_aware, max_det=max_det, edge=edge)


def _check(got, ref):
    want = [len(o["scores"]) for o in ref]
    assert got["counts"] == want, (got["counts"], want)
    assert got["count"].cpu().tolist() == got["counts"]
    assert got["merged"].dtype == torch.int32 and got["merged"].shape == got["scores"].shape
    for g, o in enumerate(ref):
        k = len(o["scores"])
        assert got["boxes"][g, :k].cpu().numpy().tobytes() == o["boxes"].tobytes(), g
        assert got["scores"][g, :k].cpu().numpy().tobytes() == o["scores"].tobytes(), g
        assert np.array_equal(got["labels"][g, :k].cpu().numpy(), o["labels"]), g
        assert np.array_equal(got["index"][g, :k].cpu().numpy(), o["index"]), g
        assert np.array_equal(got["rows"][g, :k].cpu().numpy(), o["rows"]), g
        assert np.array_equal(got["merged"][g, :k].cpu().numpy(), o["merged"]), g


# ---------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("edge", [0.0, 4.0])
@pytest.mark.parametrize("mode", ["agnostic", "aware", "capped"])
@pytest.mark.parametrize("merge", [False, True])
@pytest.mark.parametrize("metric", ["iou", "ios"])
@pytest.mark.parametrize("C", [5, 80])
@pytest.mark.parametrize("shape", ["small", "large"])
def test_decode_nmm_tiles_equals_restatement(shape, C, metric, merge, mode, edge):
    """(G, tiles, N) = (2, {5, 1}, 17), and (2, {5, 1}, 2100), where K = 10500 > 8192 on image 0 at edge 0 (the
    kernel's large-K form; the register form at edge 4)."""
    class_aware = mode != "agnostic"
    max_det = 0 if mode != "capped" else (2 if shape == "small" else 40)
    ents, begin, N = MR.plan(shape)
    ref = MR.ref(shape, C, False, metric, merge, class_aware, max_det, edge)
    assert all(len(o["scores"]) >= 1 for o in ref)
    if shape == "large":
        assert (len(ref[0]["cand_scores"]) > 8192) == (edge == 0)
    if max_det:
        assert len(ref[0]["scores"]) == max_det
    if metric == "ios" and edge == 0 and not max_det:      # (test_nmm_cpu.py holds these inputs to much more)
        assert ref[0]["merged"].max() >= 2
        if merge:
            assert (ref[0]["boxes"] != ref[0]["cand_boxes"][ref[0]["index"]]).any()
    for layout in ("contiguous", "anchor-major"):
        got = _decode(MR.pred(shape, C), ents, begin, MR.CONF[shape], metric, merge, class_aware, max_det, edge, layout)
        assert got["boxes"].shape == (len(begin) - 1, 5 * N, 4)
        _check(got, ref)


@pytest.mark.parametrize("edge", [0.0, 4.0])
def test_decode_nmm_tiles_skips_a_tile_without_source(edge):
    """src = -1 in the middle of image 0: its rows are no candidates, the rows after it keep their places."""
    ents, begin, N = MR.plan("small", hole=True)
    assert ents[1].src == -1
    ref = MR.ref("small", 5, True, "ios", True, True, 0, edge)
    assert not (ref[0]["rows"] // N == 1).any() and (ref[0]["rows"] // N >= 2).any() and ref[0]["merged"].sum() >= 1
    pred = np.array(MR.pred("small", 5, True))
    pred[1] = np.nan                                       # never read
    _check(_decode(pred, ents, begin, MR.CONF["small"], "ios", True, True, 0, edge), ref)


def test_decode_nmm_tiles_sorts_in_global_memory():
    """(1, 5, 3400): K = 17000 > 16384, the keys are sorted in global memory; IoS with merge, class-agnostic."""
    ents, begin, N = MR.plan("global")
    ref = MR.ref("global", 5, False, "ios", True, False, 0, 0.0)
    assert len(ref[0]["cand_scores"]) > 16384 and (ref[0]["merged"] >= 2).any()
    _check(_decode(MR.pred("global", 5), ents, begin, MR.CONF["global"], "ios", True, False, 0, 0.0), ref)


# ---------------------------------------------------------------- against ym_decode_nms_tiles
@pytest.mark.parametrize("edge", [0.0, 4.0])
@pytest.mark.parametrize("mode", ["agnostic", "aware", "capped"])
@pytest.mark.parametrize("shape,C", [("small", 5), ("small", 80), ("large", 5)])
def test_iou_without_merge_equals_decode_nms_tiles(shape, C, mode, edge):
    """slice_ref's own decode cases: every output of the existing entry point, and merged = the candidates a kept box
    removed (kept + merged = K without a cap)."""
    from yolomi import post
    conf = 0.5 if shape == "small" else 0.001
    class_aware = mode != "agnostic"
    max_det = 0 if mode != "capped" else (2 if shape == "small" else 40)
    ents, begin, N = SR.decode_plan(shape)
    pred = SR.decode_pred(shape, C)
    tdev = torch.from_numpy(SR.table_bytes(ents)).cuda()
    p = _tensor(pred, "contiguous")
    want = post.decode_nms_tiles(p, tdev, begin, conf, 0.45, class_aware=class_aware, max_det=max_det, edge=edge)
    got = post.decode_nmm_tiles(p, tdev, begin, conf, 0.45, metric="iou", merge=False, class_aware=class_aware,
                                max_det=max_det, edge=edge)
    ref = SR.decode_ref(shape, C, False, conf, 0.45, class_aware, max_det, edge)
    assert got["counts"] == want["counts"] == [len(o["scores"]) for o in ref] and min(got["counts"]) >= 1
    for g, k in enumerate(got["counts"]):
        for key in ("boxes", "scores", "labels", "index", "rows"):
            assert torch.equal(got[key][g, :k], want[key][g, :k]), (g, key)
        if not max_det:
            assert k + int(got["merged"][g, :k].sum()) == len(ref[g]["cand_scores"])


def _raw(metric=0, merge=0, thr=THR, merged=True, **kw):
    """ym_decode_nmm_tiles called through ctypes over the small plan -> (return code, buffers)."""
    from yolomi._lib import lib, stream_ptr
    L = lib()
    ents, begin, N = MR.plan("small")
    pred = torch.from_numpy(np.array(MR.pred("small", 5))).cuda()
    T, C, G, R = 6, 5, 2, 5 * N
    tdev = torch.from_numpy(SR.table_bytes(ents)).cuda()
    nb = L.ym_decode_nmm_tiles_workspace_size(G, R, 1)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    cnt = torch.full((G,), -7, dtype=torch.int32, device="cuda")
    boxes = torch.empty(G, R, 4, device="cuda")
    scores = torch.empty(G, R, device="cuda")
    i64 = [torch.empty(G, R, dtype=torch.int64, device="cuda") for _ in range(3)]
    mg = torch.full((G, R), -7, dtype=torch.int32, device="cuda")
    a = dict(begin=begin, G=G, T=T, N=N, edge=0.0, cls=1, max_det=0, nbytes=nb)
    a.update(kw)
    cb = (ctypes.c_int64 * len(a["begin"]))(*a["begin"])
    rc = L.ym_decode_nmm_tiles(pred.data_ptr(), a["T"], a["N"], C, 4 + C, a["N"] * (4 + C), 1, tdev.data_ptr(), cb,
                               a["G"], MR.CONF["small"], thr, metric, merge, a["edge"], a["cls"], a["max_det"],
                               ws.data_ptr(), a["nbytes"], cnt.data_ptr(), boxes.data_ptr(), scores.data_ptr(),
                               *(t.data_ptr() for t in i64), mg.data_ptr() if merged else None,
                               stream_ptr(pred.device))
    torch.cuda.synchronize()
    return rc, dict(count=cnt, boxes=boxes, scores=scores, labels=i64[0], index=i64[1], rows=i64[2], merged=mg)


def test_out_merged_may_be_null():
    """Without out_merged: the same boxes (IoU without merge is then the suppression kernel itself; IoS with merge
    still forms the unions), and out_merged is not touched."""
    for metric, merge in ((0, 0), (1, 0), (1, 1)):
        rc, a = _raw(metric, merge, merged=False)
        rc2, b = _raw(metric, merge, merged=True)
        assert rc == 0 and rc2 == 0 and (a["merged"] == -7).all()
        assert torch.equal(a["count"], b["count"]) and int(a["count"].min()) >= 1
        for g, k in enumerate(a["count"].tolist()):
            for key in ("boxes", "scores", "labels", "index", "rows"):
                assert torch.equal(a[key][g, :k], b[key][g, :k]), (metric, merge, g, key)
            assert (b["merged"][g, :k] >= 0).all()


def test_decode_nmm_tiles_argument_checks():
    from yolomi._lib import lib
    L = lib()
    nb = L.ym_decode_nmm_tiles_workspace_size(2, 85, 1)

    def bad(msg=None, **kw):
        rc, out = _raw(**kw)
        assert rc == -1, kw
        if msg:
            assert msg in L.ym_last_error(), (kw, L.ym_last_error())
        assert (out["count"] == -7).all(), kw                 # nothing was launched
        assert b"ym_decode_nmm_tiles" in L.ym_last_error()

    bad(b"metric", metric=2)
    bad(b"metric", metric=-1)
    bad(b"match_thr", thr=float("nan"))
    bad(G=-1, begin=[0])
    bad(b"monotone", begin=[0, 5, 4])
    bad(begin=[0, 5, 7])                                      # tile_begin[G] > T
    bad(begin=[-1, 5, 6])
    bad(b"too large", begin=[0, 2, 2], T=2, N=1 << 29)
    bad(edge=float("nan"))
    bad(max_det=-1)
    bad(cls=0, max_det=5)
    bad(b"workspace", nbytes=nb - 257)
    for kw in (dict(), dict(metric=1, merge=1), dict(thr=float("inf")), dict(thr=-1.0), dict(merge=7, metric=1),
               dict(edge=float("inf"))):
        rc, out = _raw(**kw)
        assert rc == 0 and (out["count"] >= 0).all(), kw
    assert _raw(G=0, begin=[0])[0] == 0


def test_unknown_metric_raises():
    ents, begin, _ = MR.plan("small")
    with pytest.raises(ValueError):
        _decode(MR.pred("small", 5), ents, begin, 0.5, "giou", False, False, 0, 0.0)


# ---------------------------------------------------------------- the Predictor
from test_gpu_predict import CH, CONF, MAX_DET, NC, S, _model, _write_pngs  # noqa: E402

HW = [(50, 70), (33, 33)]
TILE, OVERLAP, IOU = 32, 0.2, 0.45


def _images(seed=71, hw=HW):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (*s, CH), dtype=np.uint8) for s in hw]


def _forward(model, ims, batch):
    """The slice kernel and the model by hand, `batch` tiles at a time -> (y (T, 4 + nc, A), table, entries, begin)."""
    from datasets.slicing import slice_batch
    ents, begin = SR.entries([a.shape[:2] for a in ims], TILE, OVERLAP, S, None, True)
    T = len(ents)
    padded = ents + [SR.entry(-1, 0, 0, 0, 0, 0, 0, S) for _ in range(-T % batch)]
    buf, meta = AR.pack(ims)
    u8, meta = torch.from_numpy(buf).cuda(), torch.from_numpy(meta).cuda()
    tdev = torch.from_numpy(SR.table_bytes(padded)).cuda()
    with torch.no_grad():
        ys = [model(slice_batch(u8, meta, tdev, batch, S, S, CH, 114, first=lo))[0].clone()
              for lo in range(0, len(padded), batch)]
    return torch.cat(ys)[:T], tdev, ents, begin


@pytest.mark.parametrize("merge,metric", [("nmm", "ios"), ("nms", "ios"), ("nmm", "iou")])
def test_predictor_merging_equals_the_composition(merge, metric):
    from yolomi import post
    from yolomi.predict import Predictor
    model = _model()
    ims = _images()
    batch = 4
    pred = Predictor(model, imgsz=S, ch=CH, conf=CONF, iou=IOU, max_det=MAX_DET, class_aware=True, device="cuda",
                     batch=batch, slice=TILE, slice_overlap=OVERLAP, slice_merge=merge, slice_metric=metric)
    y, tdev, ents, begin = _forward(model, ims, batch)
    d = post.decode_nmm_tiles(y.transpose(1, 2), tdev, begin, CONF, IOU, metric=metric, merge=merge == "nmm",
                              class_aware=True, max_det=MAX_DET)
    ref = MR.decode_tiles(y.transpose(1, 2).cpu().numpy(), ents, begin, CONF, IOU, metric, merge == "nmm", True,
                          MAX_DET, 0.0)
    print([int(r["merged"].sum()) for r in ref], "candidates absorbed;",
          [int((r["boxes"] != r["cand_boxes"][r["index"]]).any(1).sum()) for r in ref], "unions grew")
    for _ in range(3):                                     # eager, captured, replayed: the same answer
        got = pred(ims)
        assert len(got) == len(ims)
        for g, (o, r) in enumerate(zip(got, ref)):
            n = len(r["scores"])
            assert n >= 1 and d["counts"][g] == n == len(o["scores"]) and sorted(o) == sorted(
                ("boxes", "scores", "labels", "merged"))
            for key in ("boxes", "scores", "labels", "merged"):
                assert torch.equal(o[key], d[key][g, :n]), (g, key)
            assert o["boxes"].cpu().numpy().tobytes() == r["boxes"].tobytes(), g
            assert o["scores"].cpu().numpy().tobytes() == r["scores"].tobytes(), g
            assert np.array_equal(o["labels"].cpu().numpy(), r["labels"]), g
            assert np.array_equal(o["merged"].cpu().numpy(), r["merged"]), g


def test_predictor_merging_keeps_input_order_and_groups():
    """Three sources at batch 2 (two groups): each result is the source's own, whatever its place and neighbours."""
    from yolomi.predict import Predictor
    model = _model()
    a, b = _images()
    c = _images(seed=72, hw=[(20, 30)])[0]
    pred = Predictor(model, imgsz=S, ch=CH, conf=CONF, iou=IOU, max_det=MAX_DET, batch=2, slice=TILE,
                     slice_overlap=OVERLAP, slice_merge="nmm", slice_metric="ios")
    one = [pred([im])[0] for im in (a, b, c)]
    for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0]):
        got = pred([(a, b, c)[i] for i in order])
        assert len(got) == 3
        for o, i in zip(got, order):
            assert len(o["scores"]) >= 1
            for key in ("boxes", "scores", "labels", "merged"):
                assert torch.equal(o[key], one[i][key]), (order, i, key)
    assert pred([]) == []


def test_default_predictor_is_unchanged():
    """Predictor(slice=32) and its explicit spelling: ym_decode_nms_tiles over the same forward output, no "merged"."""
    from yolomi import post
    from yolomi.predict import Predictor
    model = _model()
    ims = _images()
    kw = dict(imgsz=S, ch=CH, conf=CONF, iou=IOU, max_det=MAX_DET, class_aware=True, batch=4, slice=TILE,
              slice_overlap=OVERLAP)
    y, tdev, ents, begin = _forward(model, ims, 4)
    d = post.decode_nms_tiles(y.transpose(1, 2), tdev, begin, CONF, IOU, class_aware=True, max_det=MAX_DET)
    for pred in (Predictor(model, **kw), Predictor(model, slice_merge="nms", slice_metric="iou", **kw)):
        for g, o in enumerate(pred(ims)):
            n = d["counts"][g]
            assert n >= 1 and sorted(o) == ["boxes", "labels", "scores"]
            for key in ("boxes", "scores", "labels"):
                assert torch.equal(o[key], d[key][g, :n]), (g, key)


def test_predictor_value_errors():
    from yolomi.predict import Predictor
    model = _model()
    for kw in (dict(slice_merge="nmm"), dict(slice_metric="ios"), dict(slice=TILE, slice_merge="wbf"),
               dict(slice=TILE, slice_metric="giou"), dict(slice_merge="wbf"), dict(slice_metric="")):
        with pytest.raises(ValueError):
            Predictor(model, imgsz=S, ch=CH, **kw)
    p = Predictor(model, imgsz=S, ch=CH)
    assert (p.slice_merge, p.slice_metric) == ("nms", "iou")
    p = Predictor(model, imgsz=S, ch=CH, slice=TILE, slice_merge="nmm", slice_metric="ios")
    assert (p.slice_merge, p.slice_metric) == ("nmm", "ios")


def test_predict_cli_merges(tmp_path):
    from yolomi.predict import Predictor
    ims = _images(seed=74)
    _write_pngs(tmp_path / "src", ims)
    model = _model()
    torch.save({"epoch": 0, "model_state_dict": model.state_dict()}, tmp_path / "w.pt")
    out = tmp_path / "out"
    cmd = [sys.executable, str(ROOT / "yolo-scratch_amd" / "predict.py"), "--weights", str(tmp_path / "w.pt"),
           "--source", str(tmp_path / "src"), "--scale", "n", "--ch", str(CH), "--nc", str(NC), "--imgsz", str(S),
           "--batch", "2", "--conf", str(CONF), "--iou", str(IOU), "--max-det", str(MAX_DET), "--slice", str(TILE),
           "--slice-overlap", str(OVERLAP), "--slice-merge", "nmm", "--slice-metric", "ios", "--save-dir", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    doc = json.loads((out / "predictions.json").read_text())
    want = Predictor(model, imgsz=S, ch=CH, conf=CONF, iou=IOU, max_det=MAX_DET, batch=2, slice=TILE,
                     slice_overlap=OVERLAP, slice_merge="nmm", slice_metric="ios")(ims)
    for i, (e, w) in enumerate(zip(doc["images"], want)):
        assert (e["height"], e["width"]) == HW[i] and len(e["scores"]) >= 1
        assert sorted(e) == ["boxes", "height", "image", "labels", "scores", "width"]      # the format is kept
        assert np.array_equal(np.asarray(e["scores"], np.float32), w["scores"].cpu().numpy()), i
        assert np.array_equal(np.asarray(e["boxes"], np.float32).reshape(-1, 4), w["boxes"].cpu().numpy()), i
        assert e["labels"] == w["labels"].tolist()
        assert len((out / f"im{i}.txt").read_text().splitlines()) == len(e["scores"])
