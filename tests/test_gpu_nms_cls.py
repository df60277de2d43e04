"""Class-aware NMS with a detection cap on the GPU (ym_decode_nms_cls / ym_nms_cls) against the per-label
oracle merge of tests/nms_cls_ref.py: every comparison exact.  tests/test_nms_cls_cpu.py shows on the CPU that each
input below tells class-aware from class-agnostic suppression and that the capped cases keep more than their cap."""
import numpy as np
import pytest
import torch

import nms_cls_ref as R
from oracle import post as op

pytestmark = pytest.mark.gpu


def _strided(pred_gpu):
    """The anchor-major view of a (B, 4+nc, A) tensor: elements A apart, as validate(per_class=True) passes it."""
    v = pred_gpu.transpose(1, 2).contiguous().transpose(1, 2)
    assert v.stride(-1) == pred_gpu.shape[1]
    return v


def _same(out, ref, cap=0):
    assert len(out) == len(ref)
    for o, (rb, rs, rl, _) in zip(out, ref):
        n = min(cap, len(rs)) if cap > 0 else len(rs)
        np.testing.assert_array_equal(o["scores"].cpu().numpy(), rs[:n])
        np.testing.assert_array_equal(o["labels"].cpu().numpy(), rl[:n])
        np.testing.assert_array_equal(o["boxes"].cpu().numpy(), rb[:n])


def _bits(out):
    return [(o["boxes"].cpu().numpy().view(np.uint32), o["scores"].cpu().numpy().view(np.uint32),
             o["labels"].cpu().numpy()) for o in out]


def _same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(_bits(a), _bits(b)):
        for u, v in zip(x, y):
            np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("seed", sorted(R.CASES))
def test_decode_nms_cls_vs_oracle(seed):
    from yolomi import post
    _, B, N, nc, conf, iou = R.CASES[seed]
    pred = R.case_pred(seed).cuda()
    ref = R.case_ref(seed)
    _same(post.decode_nms(pred, 640, conf, iou, class_aware=True), ref)
    _same(post.decode_nms(_strided(pred), 640, conf, iou, class_aware=True), ref)


@pytest.mark.parametrize("seed", [13, 19])
def test_max_det(seed):
    """Scan kernel (13: the cap falls inside a chunk) and image kernel (19): the capped result is the prefix."""
    from yolomi import post
    _, B, N, nc, conf, iou = R.CASES[seed]
    pred = R.case_pred(seed).cuda()
    ref = R.case_ref(seed)
    assert 300 % 64 != 0
    above = max(len(r[1]) for r in ref) + 5
    for cap in (0, 1, 300, above):
        out = post.decode_nms(pred, 640, conf, iou, class_aware=True, max_det=cap)
        _same(out, ref, cap)
        if cap in (1, 300):
            assert all(len(o["scores"]) == cap for o in out)
    _same(post.decode_nms(_strided(pred), 640, conf, iou, class_aware=True, max_det=300), ref, 300)


def test_negative_max_det_is_refused(golden):
    from yolomi import post
    from yolomi._lib import YolomiError
    pred = R.case_pred(11).cuda()
    _, _, _, _, conf, iou = R.CASES[11]
    with pytest.raises(YolomiError):
        post.decode_nms(pred, 640, conf, iou, class_aware=True, max_det=-1)
    d = golden("nms.npz")
    b, s = torch.from_numpy(d["n100_boxes"]).cuda(), torch.from_numpy(d["n100_scores"]).cuda()
    with pytest.raises(YolomiError):
        post.nms(b, s, 0.45, max_det=-3)
    _same(post.decode_nms(pred, 640, conf, iou, class_aware=True), R.case_ref(11))      # and the next call is sound
    np.testing.assert_array_equal(post.nms(b, s, 0.45, max_det=0, labels=None).cpu().numpy(), d["n100_keep"])


@pytest.mark.parametrize("seed", [13, 16, 17])
def test_one_class_is_bit_identical_to_the_agnostic_call(seed):
    """nc = 1, no cap: every output bit of decode_nms(class_aware=False), one case per path."""
    from datasets.synthetic import synth_eval_preds
    from yolomi import post
    s, B, N, _, conf, iou = R.CASES[seed]
    pred = synth_eval_preds(B, N, nc=1, seed=s).cuda()
    agn = post.decode_nms(pred, 640, conf, iou)
    assert sum(len(o["scores"]) for o in agn) > 0
    _same_bits(post.decode_nms(pred, 640, conf, iou, class_aware=True), agn)
    _same_bits(post.decode_nms(_strided(pred), 640, conf, iou, class_aware=True), agn)


def test_one_class_golden(golden):
    from yolomi import post
    pred = torch.from_numpy(golden("decode.npz")["am_in"][..., :5].copy()).cuda()
    agn = post.decode_nms(pred, 640, 0.25, 0.45)
    assert sum(len(o["scores"]) for o in agn) > 0
    _same_bits(post.decode_nms(pred, 640, 0.25, 0.45, class_aware=True), agn)


@pytest.mark.parametrize("n", [1000, 6700])
def test_nms_with_labels(golden, n):
    from yolomi import post
    d = golden("nms.npz")
    boxes, scores = d[f"n{n}_boxes"], d[f"n{n}_scores"]
    b, s = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()
    labels = np.arange(n, dtype=np.int64) % 7
    want = R.nms_cls(boxes, scores, labels, 0.45)
    assert len(want) > len(d[f"n{n}_keep"])
    got = post.nms(b, s, 0.45, labels=torch.from_numpy(labels).cuda())
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    # labels are compared as int64 values: the same classes far apart, equal in their low 32 bits
    wide = (labels << 33) - 5
    got = post.nms(b, s, 0.45, labels=torch.from_numpy(wide).cuda(), max_det=50)
    np.testing.assert_array_equal(got.cpu().numpy(), want[:50])
    np.testing.assert_array_equal(post.nms(b, s, 0.45, labels=None).cpu().numpy(), d[f"n{n}_keep"])
    np.testing.assert_array_equal(post.nms(b, s, 0.45, max_det=10).cpu().numpy(), d[f"n{n}_keep"][:10])


def test_nms_with_labels_empty():
    from yolomi import post
    e = post.nms(torch.zeros(0, 4).cuda(), torch.zeros(0).cuda(), 0.45, labels=torch.zeros(0, dtype=torch.int64).cuda())
    assert e.shape == (0,) and e.dtype == torch.int64


def test_image_without_candidates_in_a_batch():
    from yolomi import post
    for seed in (12, 15):                                  # bitmask path, image kernel
        _, B, N, nc, conf, iou = R.CASES[seed]
        pred = R.case_pred(seed).clone()
        pred[1, :, 4:] = 0.0                               # no score > conf
        ref = R.decode_cls(pred.numpy(), 640, conf, iou)
        assert len(ref[1][1]) == 0 and len(ref[0][1]) > 0
        _same(post.decode_nms(pred.cuda(), 640, conf, iou, class_aware=True), ref)
        _same(post.decode_nms(pred.cuda(), 640, conf, iou, class_aware=True, max_det=3), ref, 3)


def test_all_candidates_of_one_label():
    """Several class columns, every candidate's maximum in column 2: the class-agnostic result with label 2."""
    from yolomi import post
    for seed in (11, 16):
        _, B, N, nc, conf, iou = R.CASES[seed]
        pred = R.case_pred(seed).clone()
        mx = pred[..., 4:].max(-1).values
        pred[..., 4:] = 0.5 * mx.unsqueeze(-1)
        pred[..., 6] = mx
        ref = R.decode_cls(pred.numpy(), 640, conf, iou)
        for (ab, as_, al), (rb, rs, rl, _) in zip(op.decode(pred.numpy(), 640, conf, iou), ref):
            np.testing.assert_array_equal(as_, rs)
            assert np.all(rl == 2)
        _same(post.decode_nms(pred.cuda(), 640, conf, iou, class_aware=True), ref)


def test_every_candidate_its_own_label():
    """As many classes as rows, row i's maximum in column i: nothing is suppressed, all kept in score order."""
    from datasets.synthetic import synth_eval_preds
    from yolomi import post
    for B, N in ((1, 130), (9, 60)):                       # bitmask path (wave rowmax: C > 64), image kernel
        base = synth_eval_preds(B, N, nc=1, seed=21)
        pred = torch.zeros(B, N, 4 + N)
        pred[..., :4] = base[..., :4]
        pred[..., 4:] = torch.diag_embed(base[..., 4])
        out = post.decode_nms(pred.cuda(), 640, 0.0, 0.45, class_aware=True)
        for b, o in enumerate(out):
            sc, order = torch.sort(base[b, :, 4], descending=True, stable=True)
            assert len(op.decode(pred[b:b + 1].numpy(), 640, 0.0, 0.45)[0][1]) < N      # agnostic NMS does suppress
            np.testing.assert_array_equal(o["scores"].cpu().numpy(), sc.numpy())
            np.testing.assert_array_equal(o["labels"].cpu().numpy(), order.numpy())


def test_two_calls_give_identical_bits():
    from yolomi import post
    for seed in (13, 19):
        _, B, N, nc, conf, iou = R.CASES[seed]
        pred = R.case_pred(seed).cuda()
        _same_bits(post.decode_nms(pred, 640, conf, iou, class_aware=True, max_det=300),
                   post.decode_nms(pred, 640, conf, iou, class_aware=True, max_det=300))


def _collect(T, m, loader, conf, **kw):
    from datasets import prepare_batch
    preds, tgts = [], []
    with torch.no_grad():
        for b in loader:
            b = prepare_batch(b, torch.device("cuda"))
            y, _ = m(b["img"])
            preds += T.decode_predictions_for_metrics(y.transpose(1, 2), b["img"].shape[-1], conf, 0.45,
                                                      torch.device("cuda"), **kw)
            for i in range(b["img"].shape[0]):
                sel = b["batch_idx"] == i
                tgts.append({"boxes": b["bboxes"][sel], "labels": b["cls"][sel].reshape(-1)})
    return preds, tgts


def test_validate_nms_per_class():
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
    vm = T.validate(m, loader, crit, dev, conf_threshold=conf, iou_threshold=0.45, per_class=True, nms_per_class=True,
                    max_det=300)
    preds, tgts = _collect(T, m, loader, conf, class_aware=True, max_det=300)
    assert 0 < max(len(p["scores"]) for p in preds) <= 300
    want = um.evaluate_detections_per_class(preds, tgts, 5, conf, 0.5)
    assert set(vm) == set(plain) | {"per_class"}
    for k in ("precision", "recall", "mAP50", "mAP50-95", "per_class"):
        assert vm[k] == want[k], k
    for k in ("loss", "box_loss", "cls_loss", "dfl_loss"):
        assert vm[k] == plain[k], k
    # without the new arguments: the class-agnostic NMS of the same read, as before
    old = T.validate(m, loader, crit, dev, conf_threshold=conf, iou_threshold=0.45, per_class=True)
    want_old = um.evaluate_detections_per_class(*_collect(T, m, loader, conf), 5, conf, 0.5)
    for k in ("precision", "recall", "mAP50", "mAP50-95", "per_class"):
        assert old[k] == want_old[k], k
    with pytest.raises(ValueError):
        T.validate(m, loader, crit, dev, conf_threshold=conf, iou_threshold=0.45, nms_per_class=True)
