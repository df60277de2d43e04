"""Class-aware detection metrics without a GPU: the filtered-oracle reference of tests/metrics_cls_cases.py is the
plain oracle at nc = 1, every generated case really holds what tests/test_gpu_metrics_cls.py relies on (so no GPU
test passes vacuously), and the public surface (utils.__all__, the trainer flag, the workspace size) is there."""
import numpy as np
import pytest

import metrics_cls_cases as MC
from metrics_cases import random_case


def _zero_labels(preds, tgts):
    return ([{**p, "labels": p["labels"] * 0} for p in preds], [{**t, "labels": t["labels"] * 0} for t in tgts])


@pytest.mark.parametrize("seed", [0, 1])
def test_filtered_oracle_at_one_class_is_the_plain_oracle(seed):
    from oracle import metrics as omet
    preds, tgts = _zero_labels(*random_case(seed))
    ref = omet.evaluate_detections(preds, tgts, 0.25, 0.5, per_threshold=True)
    got = MC.reference(preds, tgts, 1)
    for k in ("precision", "recall", "mAP50", "mAP50-95", "tp50", "fp50", "ap"):
        assert got[k] == ref[k], k
    assert got["ap_class"] == [ref["ap"]] and got["present"] == [0]
    assert got["n_gt_class"] == [sum(len(t["boxes"]) for t in tgts)]
    # a class with neither predictions nor GT: the oracle's zeros, which reference() fills in without calling it
    e = omet.evaluate_detections(*MC.filter_label(preds, tgts, 3), 0.25, 0.5, per_threshold=True)
    assert e["ap"] == [0.0] * 10 and e["tp50"] == 0 and e["fp50"] == 0


def _scores_by_class(preds, nc, conf=0.25):
    out = {}
    for p in preds:
        for s, l in zip(p["scores"].numpy(), p["labels"].numpy()):
            if s >= np.float32(conf):
                out.setdefault(int(l), []).append(float(s))
    return out


@pytest.mark.parametrize("nc", [5, 80])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_labelled_cases_hold_every_kind_of_class(nc, seed):
    preds, tgts = MC.labelled_case(seed, nc)
    npred, ngt = MC.counts(preds, tgts, nc)
    assert ngt[nc - 2] > 0 and npred[nc - 2] == 0          # GT, no predictions: present, AP 0
    assert ngt[nc - 3] == 0 and npred[nc - 3] > 0          # predictions, no GT: absent, its predictions are FPs
    assert ngt[nc - 1] == 0 and npred[nc - 1] == 0         # neither
    assert ((ngt > 0) & (npred > 0)).sum() >= 2
    by = _scores_by_class(preds, nc)
    assert any(len(set(v)) < len(v) for v in by.values())                               # ties within a class
    cls = sorted(by)
    assert any(set(by[a]) & set(by[b]) for i, a in enumerate(cls) for b in cls[i + 1:])  # and across classes
    for p, t in zip(preds, tgts):
        for lab in (p["labels"], t["labels"]):
            assert not lab.dtype.is_floating_point
            assert lab.numel() == 0 or 0 <= int(lab.min()) <= int(lab.max()) < nc


def test_wide_case_leaves_most_classes_empty():
    preds, tgts = MC.labelled_case(0, 1024, used=20)
    npred, ngt = MC.counts(preds, tgts, 1024)
    assert len(preds) == 60
    assert 15 <= ((npred > 0) | (ngt > 0)).sum() <= 22
    assert npred[0] > 0 and npred[1020] > 0                # the first and the highest ordinary class
    assert ((npred == 0) & (ngt == 0)).sum() >= 1000


def test_segment_case_sizes():
    preds, tgts, nc = MC.segment_case()
    npred, ngt = MC.counts(preds, tgts, nc)
    assert npred[0] == 1 and npred[1] == MC.AP_CHUNK and npred[2] == MC.AP_CHUNK + 1
    assert npred[3] > 2 * MC.AP_CHUNK
    assert (ngt[:5] > 0).all() and npred[4] == 0 and ngt[5] == 0 and npred[5] == 0


def test_many_gt_cases_fill_and_pass_the_lds_stage():
    for beyond, lo, hi in ((True, 2048 + 1, 4096), (False, 1985, 2048)):     # 1985: the 32nd bit of a lane mask
        preds, tgts = MC.many_gt_case(beyond)
        assert lo <= max(len(t["boxes"]) for t in tgts) <= hi
        npred, ngt = MC.counts(preds, tgts, 3)
        assert (npred > 0).all() and (ngt > 0).all()
    assert sorted(len(t["boxes"]) for t in MC.many_gt_case(True)[1]) == [0, 2510, 4014]


def test_threshold_case_and_class_aware_differs_from_class_agnostic():
    from oracle import metrics as omet
    preds, tgts = MC.labelled_case(11, 5, n_img=40)
    npred, ngt = MC.counts(preds, tgts, 5, conf=0.0)
    assert (npred[:3] > 0).all() and (ngt[:2] > 0).all() and ngt[3] > 0
    assert MC.OTHER_THRESHOLDS == [(0.3, 0.25), (0.75, 0.1), (0.5, 0.0), (0.5, 0.9)]
    aware = MC.reference(preds, tgts, 5)
    agnostic = omet.evaluate_detections(preds, tgts, 0.25, 0.5, per_threshold=True)
    assert aware["mAP50"] != agnostic["mAP50"]
    assert aware["tp50"] < agnostic["tp50"]                # a right place with the wrong label is no TP any more
    assert aware["tp50"] + aware["fp50"] == agnostic["tp50"] + agnostic["fp50"]


def test_public_names():
    import utils
    assert {"evaluate_detections_per_class", "evaluate_packed_cls"} <= set(utils.__all__)
    assert {"evaluate_detections", "evaluate_packed", "calculate_ap", "calculate_iou",
            "calculate_iou_batch"} <= set(utils.__all__)
    for n in utils.__all__:
        assert callable(getattr(utils, n))


def test_trainer_flag():
    import inspect
    import train_yolo11_cuda as T
    ap = T.build_parser()
    assert ap.parse_args([]).val_per_class is False
    assert ap.parse_args(["--val-per-class"]).val_per_class is True
    sig = inspect.signature(T.validate)
    assert sig.parameters["per_class"].default is False and sig.parameters["nc"].default is None


def test_workspace_size_without_a_gpu():
    from yolomi._lib import lib
    f = lib().ym_eval_cls_workspace_size
    assert f(10, 1000, 10, 5) > 0
    prev = 0
    for n_pred in (1, 1000, 2048, 2049, 100000, 1500000):
        cur = f(5000, n_pred, 10, 80)
        assert cur >= prev
        prev = cur
    prev = 0
    for nc in (1, 5, 80, 1024):
        cur = f(5000, 100000, 10, nc)
        assert cur >= prev
        prev = cur
