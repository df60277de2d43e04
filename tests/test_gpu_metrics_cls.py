"""Class-aware GPU detection metrics (utils.metrics.evaluate_packed_cls -> ym_eval_detections_cls) against the
class-agnostic oracle run on each label's own predictions and targets (tests/metrics_cls_cases.py:reference).

The rules are those of test_gpu_metrics.py: integer work (per-class and total TP / FP / GT counts, precision,
recall) is exact; APs and their means are fp64 sums in another order than numpy's, compared to 1e-12 relative.
tests/test_metrics_cls_cpu.py checks that every case used here holds the classes and segment sizes it is named for."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import metrics_cls_cases as MC
from metrics_cases import golden_case, random_case

pytestmark = pytest.mark.gpu
AP_RTOL = 1e-12
ROOT = Path(__file__).resolve().parents[1]


def _pack(preds, tgts):
    e4, e, el = torch.zeros(0, 4), torch.zeros(0), torch.zeros(0, dtype=torch.int64)
    pb = torch.cat([p["boxes"].reshape(-1, 4) for p in preds]) if preds else e4
    ps = torch.cat([p["scores"].reshape(-1) for p in preds]) if preds else e
    pl = torch.cat([p["labels"].reshape(-1) for p in preds]) if preds else el
    gb = torch.cat([t["boxes"].reshape(-1, 4) for t in tgts]) if tgts else e4
    gl = torch.cat([t["labels"].reshape(-1) for t in tgts]) if tgts else el
    return pb, ps, pl, [len(p["boxes"]) for p in preds], gb, gl, [len(t["boxes"]) for t in tgts]


def _gpu(preds, tgts, nc, conf=0.25, iou=0.5):
    from utils import metrics as um
    pb, ps, pl, pc, gb, gl, gc = _pack(preds, tgts)
    return um.evaluate_packed_cls(pb.cuda(), ps.cuda(), pl.cuda(), pc, gb.cuda(), gl.cuda(), gc, nc, conf, iou)


def _check(ref, got):
    for k in ("tp50", "fp50", "n_gt_class", "tp50_class", "fp50_class", "present"):
        assert got[k] == ref[k], k
    assert got["n_valid"] == ref["tp50"] + ref["fp50"]
    assert got["precision"] == ref["precision"] and got["recall"] == ref["recall"]
    np.testing.assert_allclose(got["ap_class"], ref["ap_class"], rtol=AP_RTOL, atol=1e-15)
    np.testing.assert_allclose(got["ap"], ref["ap"], rtol=AP_RTOL, atol=1e-15)
    assert got["mAP50"] == pytest.approx(ref["mAP50"], rel=AP_RTOL, abs=1e-15)
    assert got["mAP50-95"] == pytest.approx(ref["mAP50-95"], rel=AP_RTOL, abs=1e-15)


def _against_oracle(preds, tgts, nc, conf=0.25, iou=0.5):
    ref = MC.reference(preds, tgts, nc, conf, iou)
    got = _gpu(preds, tgts, nc, conf, iou)
    _check(ref, got)
    return ref, got


def _one_class_invariant(preds, tgts):
    """nc = 1, every label 0: every output equals the class-agnostic evaluation of the same tensors."""
    from utils import metrics as um
    preds = [{**p, "labels": torch.zeros(len(p["boxes"]), dtype=torch.int64)} for p in preds]
    tgts = [{**t, "labels": torch.zeros(len(t["boxes"]), dtype=torch.int64)} for t in tgts]
    pb, ps, pl, pc, gb, gl, gc = _pack(preds, tgts)
    want = um.evaluate_packed(pb.cuda(), ps.cuda(), pc, gb.cuda(), gc, 0.25, 0.5)
    got = _gpu(preds, tgts, 1)
    for k in ("tp50", "fp50", "n_valid", "precision", "recall"):
        assert got[k] == want[k], k
    assert got["tp50_class"] == [want["tp50"]] and got["fp50_class"] == [want["fp50"]]
    assert got["n_gt_class"] == [sum(gc)]
    np.testing.assert_allclose(got["ap"], want["ap"], rtol=AP_RTOL, atol=1e-15)
    np.testing.assert_allclose(got["ap_class"], [want["ap"]], rtol=AP_RTOL, atol=1e-15)
    for k in ("mAP50", "mAP50-95"):
        assert got[k] == pytest.approx(want[k], rel=AP_RTOL, abs=1e-15), k
    return want


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_one_class_equals_class_agnostic(seed):
    want = _one_class_invariant(*random_case(seed))
    assert want["tp50"] > 0 and want["fp50"] > 0


def test_one_class_equals_class_agnostic_on_the_golden_run(golden):
    _one_class_invariant(*golden_case(golden("metrics.npz")))


@pytest.mark.parametrize("nc", [5, 80])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_labelled_sets_match_filtered_oracle(nc, seed):
    preds, tgts = MC.labelled_case(seed, nc)
    ref, got = _against_oracle(preds, tgts, nc)
    assert ref["tp50"] > 0 and ref["fp50"] > 0
    assert got["ap_class"][nc - 2] == [0.0] * 10 and nc - 2 in got["present"]          # GT, never predicted
    assert nc - 3 not in got["present"] and got["fp50_class"][nc - 3] > 0              # predicted, no GT
    assert got["ap_class"][nc - 3] == [0.0] * 10 and got["ap_class"][nc - 1] == [0.0] * 10


def test_wide_class_range_mostly_empty():
    """nc = 1024, about 20 classes in use: a thousand empty segments between the real ones."""
    preds, tgts = MC.labelled_case(0, 1024, used=20)
    ref, got = _against_oracle(preds, tgts, 1024)
    assert ref["tp50"] > 0 and len(got["present"]) >= 15


def test_unequal_segments_across_the_ap_chunk():
    """Classes of exactly 1, AP_CHUNK, AP_CHUNK + 1 and more than 2 * AP_CHUNK kept predictions in one call."""
    preds, tgts, nc = MC.segment_case()
    ref, got = _against_oracle(preds, tgts, nc)
    assert [a + b for a, b in zip(got["tp50_class"], got["fp50_class"])][:3] == [1, MC.AP_CHUNK, MC.AP_CHUNK + 1]
    assert got["tp50_class"][3] > 100


@pytest.mark.parametrize("beyond_lds", [False, True])
def test_many_gt_per_image(beyond_lds):
    """The many-GT input of test_gpu_metrics.py with labels (the LDS stage filled to 2013 of 2048), and images of
    2510 and 4014 GT boxes: labels read through L2, the 64-bit masks up to 4096, with the label term on."""
    preds, tgts = MC.many_gt_case(beyond_lds)
    ref, _ = _against_oracle(preds, tgts, 3)
    assert ref["tp50"] > 0


@pytest.mark.parametrize("iou,conf", MC.OTHER_THRESHOLDS)
def test_other_thresholds(iou, conf):
    preds, tgts = MC.labelled_case(11, 5, n_img=40)
    _against_oracle(preds, tgts, 5, conf, iou)


def _d(boxes, scores=None, labels=()):
    d = {"boxes": torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4),
         "labels": torch.tensor(list(labels), dtype=torch.int64)}
    if scores is not None:
        d["scores"] = torch.tensor(scores, dtype=torch.float32)
    return d


def test_edge_cases():
    from utils import metrics as um
    box = [[0.1, 0.1, 0.4, 0.4]]
    cases = [
        ([_d([], [])] * 3, [_d(box, labels=[1])] * 3),                          # no predictions anywhere
        ([_d(box, [0.9], [2])] * 2, [_d([])] * 2),                              # no GT anywhere
        ([_d(box, [0.1], [1])], [_d(box, labels=[1])]),                         # everything below conf
        ([], []),                                                               # no images
    ]
    for preds, tgts in cases:
        _against_oracle(preds, tgts, 3)
    # one perfect box with the right label ...
    ref, got = _against_oracle([_d(box, [0.9], [1])], [_d(box, labels=[1])], 3)
    assert got["tp50"] == 1 and got["fp50"] == 0 and got["mAP50"] > 0.99 and got["ap_class"][1][0] > 0.99
    # ... and the same box with the wrong label: what the class-agnostic evaluation calls a TP is none
    wrong_p, wrong_t = [_d(box, [0.9], [2])], [_d(box, labels=[1])]
    ref, got = _against_oracle(wrong_p, wrong_t, 3)
    assert got["tp50"] == 0 and got["fp50"] == 1 and got["mAP50"] == 0.0 and got["mAP50-95"] == 0.0
    assert got["fp50_class"] == [0, 0, 1] and got["n_gt_class"] == [0, 1, 0] and got["present"] == [1]
    pb, ps, _, pc, gb, _, gc = _pack(wrong_p, wrong_t)
    agnostic = um.evaluate_packed(pb.cuda(), ps.cuda(), pc, gb.cuda(), gc, 0.25, 0.5)
    assert agnostic["tp50"] == 1 and agnostic["fp50"] == 0
    r = um.evaluate_detections_per_class([], [], nc=3)
    assert {k: r[k] for k in ("precision", "recall", "mAP50", "mAP50-95")} == {
        "precision": 0.0, "recall": 0.0, "mAP50": 0.0, "mAP50-95": 0.0}
    assert r["per_class"] == {"ap50": [0.0] * 3, "ap": [0.0] * 3, "n_gt": [0] * 3, "tp": [0] * 3, "fp": [0] * 3}
    # the list-of-dicts entry point on CPU tensors, as the sibling function is called
    r = um.evaluate_detections_per_class(wrong_p, wrong_t, nc=3)
    assert r["precision"] == 0.0 and r["per_class"]["fp"] == [0, 0, 1] and r["per_class"]["n_gt"] == [0, 1, 0]


def test_deterministic():
    """Two calls on one input: every value of the out buffer (the whole returned dict holds it) has the same bits."""
    preds, tgts = MC.labelled_case(1, 80)
    a, b = _gpu(preds, tgts, 80), _gpu(preds, tgts, 80)
    assert a == b
    assert np.array_equal(np.asarray(a["ap_class"]).view(np.int64), np.asarray(b["ap_class"]).view(np.int64))


def test_bad_label_is_refused():
    """A label outside [0, nc): YolomiError, nothing indexed by it (csrc/metrics.hip checks the range first)."""
    from yolomi import YolomiError
    box = [[0.1, 0.1, 0.4, 0.4]]
    with pytest.raises(YolomiError):
        _gpu([_d(box, [0.9], [3])], [_d(box, labels=[1])], 3)
    with pytest.raises(YolomiError):
        _gpu([_d(box, [0.9], [1])], [_d(box, labels=[-1])], 3)
    with pytest.raises(YolomiError):
        _gpu([_d(box, [0.9], [0])], [_d(box, labels=[0])], 1025)
    _against_oracle([_d(box, [0.9], [1])], [_d(box, labels=[1])], 3)       # and the next call is sound


def _collect(T, m, loader, conf, anchor_major):
    """The detections validate() evaluates: decoded from the eval output as the reference reads it, or (per_class)
    from its anchor-major view, whose labels are classes."""
    from datasets import prepare_batch
    preds, tgts = [], []
    with torch.no_grad():
        for b in loader:
            b = prepare_batch(b, torch.device("cuda"))
            y, _ = m(b["img"])
            y = y.transpose(1, 2) if anchor_major else y
            preds += T.decode_predictions_for_metrics(y, b["img"].shape[-1], conf, 0.45, torch.device("cuda"))
            for i in range(b["img"].shape[0]):
                sel = b["batch_idx"] == i
                tgts.append({"boxes": b["bboxes"][sel], "labels": b["cls"][sel].reshape(-1)})
    return preds, tgts


def test_validate_per_class():
    import train_yolo11_cuda as T
    from losses import v8DetectionLoss
    from test_gpu_model import _seeded_model
    from utils import metrics as um
    m = _seeded_model("n").train()
    crit = v8DetectionLoss(m)
    loader = T._SyntheticLoader(2, 3, 256, seed=50)
    conf = 1e-7                      # the untrained head scores ~1e-6: keep candidates
    dev = torch.device("cuda")
    plain = T.validate(m, loader, crit, dev, conf_threshold=conf, iou_threshold=0.45)
    vm = T.validate(m, loader, crit, dev, conf_threshold=conf, iou_threshold=0.45, per_class=True)
    preds, tgts = _collect(T, m, loader, conf, anchor_major=True)
    assert sum(len(p["scores"]) for p in preds) > 0
    assert all(0 <= int(p["labels"].min()) and int(p["labels"].max()) < 5 for p in preds if len(p["labels"]))
    want = um.evaluate_detections_per_class(preds, tgts, 5, conf, 0.5)
    assert set(vm) == set(plain) | {"per_class"}
    for k in ("precision", "recall", "mAP50", "mAP50-95", "per_class"):
        assert vm[k] == want[k], k
    assert len(vm["per_class"]["ap"]) == 5 and sum(vm["per_class"]["n_gt"]) == sum(len(t["boxes"]) for t in tgts)
    for k in ("loss", "box_loss", "cls_loss", "dfl_loss"):
        assert vm[k] == plain[k], k
    # without the flag: the class-agnostic evaluation of the same detections, as before
    agn = um.evaluate_detections(*_collect(T, m, loader, conf, anchor_major=False), conf, 0.5)
    assert "per_class" not in plain and {k: plain[k] for k in agn} == agn
    assert T.validate(m, loader, crit, dev, conf_threshold=conf, iou_threshold=0.45, per_class=True, nc=7)[
        "per_class"]["n_gt"][5:] == [0, 0]


def test_validate_per_class_world2(tmp_path):
    """validate(per_class=True) under data parallelism at world size 2 (two processes on GPU 0 through gloo, as
    tests/test_gpu_dp_world2.py): both ranks return the same dict, per-class lists included, equal to the
    single-process one."""
    from test_gpu_dp_world2 import _free_port
    env = dict(os.environ, YM_DIST_BACKEND="gloo", YM_DIST_DEVICE="0", PYTHONUNBUFFERED="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           str(ROOT / "tests" / "dp_cls_worker.py"), str(tmp_path)]
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                            start_new_session=True)
    try:
        out, err = proc.communicate(timeout=110)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, 9)
        out, err = proc.communicate()
        pytest.fail(f"2-rank run timed out: {err[-4000:]}")
    assert proc.returncode == 0, (out[-3000:], err[-6000:])
    res = [json.loads((tmp_path / f"res_r{k}.json").read_text()) for k in range(2)]
    v0, v1, w1 = res[0]["val_dp"], res[1]["val_dp"], res[0]["val_world1"]
    assert v0 == v1
    assert len(v0["per_class"]["ap"]) == 5 and sum(v0["per_class"]["n_gt"]) > 0
    for k in ("loss", "box_loss", "cls_loss", "dfl_loss"):
        assert abs(v0[k] - w1[k]) <= 1e-6 * max(1.0, abs(w1[k])), (k, v0[k], w1[k])
    for k in ("precision", "recall", "mAP50", "mAP50-95", "per_class"):
        assert v0[k] == w1[k], (k, v0[k], w1[k])
