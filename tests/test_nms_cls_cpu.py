"""Class-aware NMS with a detection cap, the parts that need no GPU: the reference helper (tests/nms_cls_ref.py) against
the definition, the non-vacuity of the inputs tests/test_gpu_nms_cls.py uses, and the public surface."""
import inspect

import numpy as np
import pytest

import nms_cls_ref as R
from oracle import post as op


# seed -> (image, kept class-agnostic, kept class-aware): what the inputs were chosen for
KEPT = {11: (0, 27, 68), 12: (0, 53, 135), 13: (0, 148, 429), 14: (0, 1083, 6501), 15: (1, 8, 12), 16: (0, 28, 58),
        19: (0, 581, 1873), 17: (0, 155, 486), 18: (0, 192, 588)}


def _brute(boxes, scores, labels, thr, max_det=0):
    """The definition: walk the candidates by (score descending, index ascending); keep one iff no earlier kept
    candidate of its label has !(IoU <= thr) with it; stop at max_det."""
    order = sorted(range(len(scores)), key=lambda i: (-float(scores[i]), i))
    kept = []
    for i in order:
        ok = True
        for j in kept:
            if labels[j] == labels[i] and not (op.iou_row(boxes[j], boxes[i:i + 1])[0] <= np.float32(thr)):
                ok = False
                break
        if ok:
            kept.append(i)
            if max_det > 0 and len(kept) == max_det:
                break
    return np.asarray(kept, np.int64)


@pytest.mark.parametrize("nc,conf,iou,max_det", [(5, 0.25, 0.45, 0), (3, 0.0, 0.7, 0), (5, 0.25, 0.45, 20),
                                                 (80, 0.001, 0.45, 0)])
def test_helper_is_the_definition(nc, conf, iou, max_det):
    from datasets.synthetic import synth_eval_preds
    pred = synth_eval_preds(2, 300, nc=nc, seed=31).numpy()
    for p, (bx, sc, lb, keep) in zip(pred, R.decode_cls(pred, 640, conf, iou, max_det)):
        xyxy, mx, lab = R.candidates(p, conf)
        want = _brute(xyxy, mx, lab, iou, max_det)
        assert len(want) > 10
        np.testing.assert_array_equal(keep, want)
        np.testing.assert_array_equal(sc, mx[want])
        np.testing.assert_array_equal(lb, lab[want])
        np.testing.assert_array_equal(bx, np.clip(xyxy[want] / np.float32(640), 0.0, 1.0).astype(np.float32))
        assert np.all(np.diff(sc) < 0)                   # global score-descending order across the classes


def test_one_class_is_the_agnostic_oracle():
    from datasets.synthetic import synth_eval_preds
    pred = synth_eval_preds(3, 500, nc=1, seed=32).numpy()
    for (rb, rs, rl), (bx, sc, lb, _) in zip(op.decode(pred, 640, 0.25, 0.45), R.decode_cls(pred, 640, 0.25, 0.45)):
        assert len(rs) > 0
        np.testing.assert_array_equal(bx, rb)
        np.testing.assert_array_equal(sc, rs)
        np.testing.assert_array_equal(lb, rl)


@pytest.mark.parametrize("seed", sorted(R.CASES))
def test_gpu_cases_are_not_vacuous(seed):
    """On every input of the GPU tests the class-aware result differs from the class-agnostic one, and where a case
    is capped the uncapped kept count exceeds the cap."""
    _, B, N, nc, conf, iou = R.CASES[seed]
    pred = R.case_pred(seed).numpy()
    agn = op.decode(pred, 640, conf, iou)
    aware = R.case_ref(seed)
    differ = [len(a[1]) != len(c[1]) or not np.array_equal(a[1], c[1]) for a, c in zip(agn, aware)]
    assert any(differ), "class-aware == class-agnostic on this input"
    img, n_agn, n_aware = KEPT[seed]
    assert (len(agn[img][1]), len(aware[img][1])) == (n_agn, n_aware)
    for cap in R.MAX_DET.get(seed, ()):
        assert all(len(c[1]) > cap for c in aware), [len(c[1]) for c in aware]


def test_parser_flags():
    import train_yolo11_cuda as T
    ap = T.build_parser()
    d = ap.parse_args([])
    assert d.val_nms_per_class is False and d.val_max_det == 0
    a = ap.parse_args(["--val-per-class", "--val-nms-per-class", "--val-max-det", "300"])
    assert a.val_per_class and a.val_nms_per_class and a.val_max_det == 300
    with pytest.raises(SystemExit):
        ap.parse_args(["--val-nms-per-class"])
    with pytest.raises(SystemExit):
        ap.parse_args(["--val-per-class", "--val-nms-per-class", "--val-max-det", "-1"])


def test_keyword_defaults():
    import train_yolo11_cuda as T
    from yolomi import post
    s = inspect.signature(post.decode_nms).parameters
    assert s["class_aware"].default is False and s["max_det"].default == 0
    s = inspect.signature(post.nms).parameters
    assert s["labels"].default is None and s["max_det"].default == 0
    s = inspect.signature(T.decode_predictions_for_metrics).parameters
    assert s["class_aware"].default is False and s["max_det"].default == 0
    s = inspect.signature(T.validate).parameters
    assert s["nms_per_class"].default is False and s["max_det"].default == 0


def test_workspace_size_without_a_gpu():
    from yolomi._lib import lib
    f, g = lib().ym_nms_cls_workspace_size, lib().ym_nms_workspace_size
    for B in (1, 2, 8, 9, 128):
        prev = 0
        for N in (1, 17, 127, 128, 130, 600, 8400, 9600):      # one path per B: monotone in N along it
            cur = f(B, N)
            assert cur >= g(B, N) > 0
            assert cur >= prev, (B, N)
            prev = cur
        prev = 0
        for N in (9601, 16500, 33600):
            cur = f(B, N)
            assert cur >= g(B, N) and cur >= prev
            prev = cur
    # the bitmask path holds a sorted-label array beside the sorted boxes
    assert f(1, 8400) >= g(1, 8400) + 4 * 8400
