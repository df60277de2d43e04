"""Rectangular inference and validation on the GPU: the decode + NMS write stage normalised by
(img_w, img_h) bit for bit against the restatement of tests/rect_ref.py, prepare_batch on a rect batch,
Predictor(rect=True) against the composition of its parts per frame group, validate over the --val-rect loader, and
the two command lines."""
import functools
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import letterbox_ref as LR
import rect_ref as RR

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
CONF, IOU = 0.25, 0.45
FRAMES = [(384, 640), (640, 384), (640, 640)]                       # (H, W): a swapped pair cannot pass
SHAPES = {"n17": (3, 17, 41), "n8400": (2, 8400, 42)}               # name -> (B, N, seed): image kernel, bitmask path
CAPS = {"n17": 3, "n8400": 10}

_PREDS = {}


def _pred(name):
    """The case's synth_eval_preds tensor on the host (built once; read-only)."""
    from datasets.synthetic import synth_eval_preds
    if name not in _PREDS:
        B, N, seed = SHAPES[name]
        _PREDS[name] = synth_eval_preds(B, N, seed=seed)
    return _PREDS[name]


def _anchor_major(pred_gpu):
    """The (B, N, 4+C) view of a (B, 4+C, N) tensor: a row's elements N apart, as the eval output is read."""
    v = pred_gpu.transpose(1, 2).contiguous().transpose(1, 2)
    assert v.stride(-1) == pred_gpu.shape[1] and v.stride(1) == 1
    return v


def _same(out, ref):
    assert len(out) == len(ref)
    for o, (rb, rs, rl) in zip(out, ref):
        assert len(rs) >= 1, "the comparison must not pass empty"
        np.testing.assert_array_equal(o["scores"].cpu().numpy(), rs)
        np.testing.assert_array_equal(o["labels"].cpu().numpy(), rl)
        np.testing.assert_array_equal(o["boxes"].cpu().numpy(), rb)


# ---------------------------------------------------------------- decode + NMS, bit for bit
@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("frame", FRAMES)
def test_decode_nms_wh_vs_restatement(name, frame):
    from yolomi import post
    H, W = frame
    host = _pred(name)
    pred = host.cuda()
    views = (pred, _anchor_major(pred))
    cap = CAPS[name]
    refs = {
        "agnostic": RR.decode_wh(name, host.numpy(), H, W, CONF, IOU),
        "cls": RR.decode_cls_wh(name, host.numpy(), H, W, CONF, IOU),
        "cap": RR.decode_cls_wh(name, host.numpy(), H, W, CONF, IOU, cap),
    }
    assert any(len(f[1]) > len(c[1]) for f, c in zip(refs["cls"], refs["cap"])), "the cap must cut something"
    for v in views:
        _same(post.decode_nms(v, (H, W), CONF, IOU), refs["agnostic"])
        _same(post.decode_nms(v, (H, W), CONF, IOU, class_aware=True), refs["cls"])
        _same(post.decode_nms(v, (H, W), CONF, IOU, class_aware=True, max_det=cap), refs["cap"])
        _same(post.decode_nms(v, [H, W], CONF, IOU), refs["agnostic"])
    if H != W:
        # the synthetic boxes span 640 pixels: the 384 side clamps some kept coordinate to 1, the 640 side does not
        short = (1, 3) if H < W else (0, 2)
        for ref in refs.values():
            allb = np.concatenate([r[0] for r in ref])
            assert (allb[:, short] == 1.0).any(), "no kept box is clamped on the short side"
            assert (allb >= 0).all() and (allb <= 1).all()
    else:
        # a square frame through the new entry points is the existing entry points' answer, byte for byte
        for v in views:
            for kw in ({}, {"class_aware": True}, {"class_aware": True, "max_det": cap}):
                new = post.decode_nms(v, (H, W), CONF, IOU, **kw)
                old = post.decode_nms(v, W, CONF, IOU, **kw)
                for a, b in zip(new, old):
                    for k in ("boxes", "scores", "labels"):
                        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), (kw, k)
        np_ref = RR.decode_wh(name, host.numpy(), H, W, CONF, IOU)
        _same(post.decode_nms(pred, 640, CONF, IOU), np_ref)


def test_decode_nms_wh_padded_form_and_argument_checks():
    from yolomi import post
    from yolomi._lib import YolomiError
    host = _pred("n17")
    pred = host.cuda()
    ref = RR.decode_cls_wh("n17", host.numpy(), 384, 640, CONF, IOU)
    d = post.decode_nms(pred, (384, 640), CONF, IOU, class_aware=True, padded=True)
    assert d["counts"] == [len(r[1]) for r in ref] == d["count"].cpu().tolist()
    for b, (rb, rs, rl) in enumerate(ref):
        np.testing.assert_array_equal(d["boxes"][b, :len(rs)].cpu().numpy(), rb)
    for bad in ((0, 640), (384, 0), (-384, 640), (384, -1.0), (float("nan"), 640)):
        for kw in ({}, {"class_aware": True}):
            with pytest.raises(YolomiError):
                post.decode_nms(pred, bad, CONF, IOU, **kw)
    with pytest.raises(ValueError):
        post.decode_nms(pred, (384, 640, 3), CONF, IOU)
    with pytest.raises(ValueError):
        post.decode_nms(pred, (384, 640), CONF, IOU, max_det=5)     # the class-agnostic path has no cap
    with pytest.raises(YolomiError):
        post.decode_nms(pred, (384, 640), CONF, IOU, class_aware=True, max_det=-1)
    _same(post.decode_nms(pred, (384, 640), CONF, IOU, class_aware=True), ref)        # and the next call is sound


# ---------------------------------------------------------------- prepare_batch on a rect batch
def test_prepare_batch_on_a_rect_batch():
    from datasets import collate_fn_cuda, prepare_batch
    rng = np.random.default_rng(12)
    hws = [(60, 100), (90, 160), (0, 0)]
    for ch in (3, 1):
        ims = [rng.integers(0, 256, (*hw, ch), dtype=np.uint8) for hw in hws]
        items = []
        for i, a in enumerate(ims):
            t = torch.from_numpy(a if ch > 1 else np.ascontiguousarray(a[..., 0])[None])
            n = 0 if a.size == 0 else 2
            boxes = torch.tensor([[0.5, 0.5, 0.2, 0.4]] * n, dtype=torch.float32).reshape(-1, 4)
            items.append((t, boxes, torch.zeros(n, dtype=torch.long), i))
        batch = collate_fn_cuda(items, img_size=160, channels=ch, letterbox=True, rect=True)
        assert batch["img_frame"].tolist() == [96, 160]
        d = prepare_batch(batch, torch.device("cuda"))
        assert set(d) == {"img", "batch_idx", "cls", "bboxes", "max_gt"} and d["img"].shape == (3, ch, 96, 160)
        want = LR.render(LR.entries(ims, 96, 160), ims, 96, 160, 114)
        assert np.array_equal(d["img"].cpu().numpy(), LR.as_float(want))
        assert (d["img"][2] == np.float32(114) / np.float32(255)).all()              # the empty image is all fill
        assert torch.equal(d["bboxes"].cpu(), batch["bboxes"])


# ---------------------------------------------------------------- Predictor(rect=True)
S, NC, CH, BATCH = 160, 3, 3, 2
P_CONF, P_IOU, MAX_DET = 1e-7, 0.45, 50        # the untrained head scores ~1e-6: every image keeps boxes
HW = [(60, 100), (100, 60), (90, 160), (160, 160), (61, 100)]
HW_FRAMES = [(96, 160), (160, 96), (96, 160), (160, 160), (128, 160)]


def _images(hws, seed=21):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (*hw, CH), dtype=np.uint8) for hw in hws]


def _model():
    from test_gpu_model import _seeded_model
    return _seeded_model("n", nc=NC, ch=CH).eval()


def _composition(model, ims, frame):
    """The chain by hand over one frame group's chunk, padded to BATCH with empty images as the predictor pads."""
    from yolomi import post
    H, W = frame
    padded = ims + [np.zeros((0, 0, CH), np.uint8)] * (BATCH - len(ims))
    table = LR.entries(padded, H, W)
    img = torch.from_numpy(LR.as_float(LR.render(table, padded, H, W, 114))).cuda()
    with torch.no_grad():
        y = model(img)[0]
    dets = post.decode_nms(y.transpose(1, 2), (H, W), P_CONF, P_IOU, class_aware=True, max_det=MAX_DET)[:len(ims)]
    out = []
    for b, d in enumerate(dets):
        k = len(d["scores"])
        boxes = LR.unletterbox(d["boxes"].cpu().numpy()[None], [k], [table[b]], H, W)[0]
        out.append({"boxes": boxes, "scores": d["scores"].cpu().numpy(), "labels": d["labels"].cpu().numpy()})
    return out


def _want(model, ims):
    """Per input position, the composition of its frame group (groups in first-seen order, chunks of BATCH)."""
    groups = {}
    for i, a in enumerate(ims):
        groups.setdefault(RR.frame([a.shape[:2]], S), []).append(i)
    want = [None] * len(ims)
    for frame, pos in groups.items():
        for lo in range(0, len(pos), BATCH):
            chunk = pos[lo:lo + BATCH]
            for i, d in zip(chunk, _composition(model, [ims[i] for i in chunk], frame)):
                want[i] = d
    return want


def _check(got, want, hws):
    assert len(got) == len(want) == len(hws)
    for i, (g, w) in enumerate(zip(got, want)):
        n = len(w["scores"])
        assert n >= 1, "the comparison must not pass empty"
        assert len(g["scores"]) == n and n <= MAX_DET, i
        assert np.array_equal(g["labels"].cpu().numpy(), w["labels"]), i
        assert g["scores"].cpu().numpy().tobytes() == w["scores"].tobytes(), i
        assert g["boxes"].cpu().numpy().tobytes() == w["boxes"].tobytes(), i
        h0, w0 = hws[i]
        b = g["boxes"].cpu().numpy()
        assert (b >= 0).all() and (b[:, [0, 2]] <= w0).all() and (b[:, [1, 3]] <= h0).all(), i
        assert set(w["labels"].tolist()) <= set(range(NC))


def _eval_frames(model):
    """(B, H, W) of the whole-model eval plans the model holds."""
    return sorted(k[1:4] for k, v in model.__dict__.get("_ym_plans", {}).items()
                  if k[0] == "model" and not k[-1] and v)


def test_predictor_rect_equals_the_composition_per_frame_group():
    from yolomi.predict import Predictor
    assert [RR.frame([hw], S) for hw in HW] == HW_FRAMES
    model = _model()
    ims = _images(HW)
    pred = Predictor(model, imgsz=S, ch=CH, conf=P_CONF, iou=P_IOU, max_det=MAX_DET, class_aware=True, device="cuda",
                     batch=BATCH, rect=True)
    assert [pred.frame_of(a) for a in ims] == HW_FRAMES
    want = _want(model, ims)
    for _ in range(3):                                     # eager, captured, replayed: the same answer
        _check(pred(ims), want, HW)
    assert _eval_frames(model) == sorted({(BATCH, *f) for f in HW_FRAMES})
    plan = model.__dict__["_ym_plans"][("model", BATCH, 96, 160, False)][0]
    assert "fwd" in plan.__dict__.get("_graphs", {}), "the eval forward was not replayed as a graph"
    # images 0 and 2 ran in one forward of the (96, 160) group, and came back at their own positions
    assert not np.array_equal(want[0]["scores"], want[2]["scores"])
    # one frame's plans at a time: the same answers, and the model holds the last frame only
    small = _model()
    one = Predictor(small, imgsz=S, ch=CH, conf=P_CONF, iou=P_IOU, max_det=MAX_DET, batch=BATCH, rect=True,
                    max_frames=1)
    for _ in range(2):
        _check(one(ims), want, HW)
        assert _eval_frames(small) == [(BATCH, 128, 160)]
    with pytest.raises(ValueError):
        Predictor(small, imgsz=100, ch=CH, rect=True)
    with pytest.raises(ValueError):
        Predictor(small, imgsz=S, ch=CH, rect=True, max_frames=0)


def test_predictor_rect_on_square_frames_is_the_square_predictor():
    from yolomi.predict import Predictor
    hws = [(160, 160), (80, 80), (160, 150), (155, 160)]
    assert all(RR.frame([hw], S) == (S, S) for hw in hws)
    model = _model()
    ims = _images(hws, seed=22)
    kw = dict(imgsz=S, ch=CH, conf=P_CONF, iou=P_IOU, max_det=MAX_DET, batch=BATCH)
    got = Predictor(model, rect=True, **kw)(ims)
    want = Predictor(model, **kw)(ims)
    for g, w in zip(got, want):
        assert len(w["scores"]) >= 1
        for k in ("boxes", "scores", "labels"):
            assert g[k].cpu().numpy().tobytes() == w[k].cpu().numpy().tobytes(), k


def test_drop_eval_plans_leaves_other_plans_alone():
    from yolomi.graph import drop_eval_plans
    model = _model()
    x = torch.zeros(1, CH, 96, 160, device="cuda")
    with torch.no_grad():
        model(x), model(torch.zeros(1, CH, 64, 64, device="cuda"))
    model.train()
    model(x)                                               # a training plan of the same shape, its backward pending
    model.eval()
    assert _eval_frames(model) == [(1, 64, 64), (1, 96, 160)]
    assert drop_eval_plans(model, 1, 96, 160) == 1 and drop_eval_plans(model, 1, 96, 160) == 0
    assert drop_eval_plans(model, 2, 96, 160) == 0
    assert _eval_frames(model) == [(1, 64, 64)]
    assert len(model.__dict__["_ym_plans"][("model", 1, 96, 160, True)]) == 1
    with torch.no_grad():
        assert torch.isfinite(model(x)[0]).all()           # and the frame is planned again when it comes back


# ---------------------------------------------------------------- validation
VAL_HW = [(60, 100), (100, 60), (60, 100), (160, 160), (100, 60), (60, 100)]


def _write_dir(root, hws, seed=8):
    from PIL import Image
    (root / "images").mkdir(parents=True)
    (root / "labels").mkdir()
    rng = np.random.default_rng(seed)
    n_boxes = 0
    for i, hw in enumerate(hws):
        Image.fromarray(rng.integers(0, 256, (*hw, CH), dtype=np.uint8)).save(root / "images" / f"im{i}.png")
        rows = [f"{int(rng.integers(0, NC))} {rng.uniform(0.3, 0.7):.4f} {rng.uniform(0.3, 0.7):.4f} "
                f"{rng.uniform(0.2, 0.5):.4f} {rng.uniform(0.2, 0.5):.4f}" for _ in range(int(rng.integers(1, 4)))]
        n_boxes += len(rows)
        (root / "labels" / f"im{i}.txt").write_text("\n".join(rows) + "\n")
    return n_boxes


def test_validate_over_the_val_rect_loader(tmp_path):
    import train_yolo11_cuda as T
    from datasets import YoloTxtDataset, collate_fn_cuda, prepare_batch
    from losses import v8DetectionLoss
    from torch.utils.data import DataLoader, Subset
    n_boxes = _write_dir(tmp_path / "d", VAL_HW)
    ds = YoloTxtDataset(tmp_path / "d", img_size=S, channels=CH)
    va = Subset(ds, list(range(len(ds))))
    loader = T.rect_val_loader(va, range(len(va)), 2, S, CH, num_workers=0)
    # RectSampler's order: h0 / w0 ascending, ties in file order
    order = sorted(range(6), key=lambda i: VAL_HW[i][0] / VAL_HW[i][1])
    assert list(loader.sampler) == order == [0, 2, 5, 3, 1, 4]
    shapes, targets = [], 0
    for k, b in enumerate(loader):
        src = [VAL_HW[i] for i in order[2 * k:2 * k + 2]]
        assert tuple(b["img_frame"].tolist()) == RR.frame(src, S)
        d = prepare_batch(b, torch.device("cuda"))
        assert tuple(d["img"].shape) == (2, CH, *RR.frame(src, S))
        shapes.append(tuple(d["img"].shape[-2:]))
        targets += len(d["bboxes"])
    assert shapes == [(96, 160), (160, 160), (160, 96)] and targets == n_boxes
    model = _model()
    crit = v8DetectionLoss(model)
    dev = torch.device("cuda")
    for kw in ({}, {"per_class": True, "nms_per_class": True, "max_det": MAX_DET}):
        vm = T.validate(model, loader, crit, dev, conf_threshold=P_CONF, iou_threshold=P_IOU, max_frames=2, **kw)
        for key in ("loss", "box_loss", "cls_loss", "dfl_loss", "precision", "recall", "mAP50", "mAP50-95"):
            assert math.isfinite(vm[key]), (key, vm[key])
        if kw:
            assert sum(vm["per_class"]["n_gt"]) == n_boxes
        # at most two frames' eval plans were kept
        assert len({f[1:] for f in _eval_frames(model)}) <= 2
    # a directory of square images: the rect loader's result is the --letterbox loader's, exactly
    sq = [(160, 160), (80, 80), (120, 120), (160, 160)]
    _write_dir(tmp_path / "sq", sq, seed=9)
    dsq = YoloTxtDataset(tmp_path / "sq", img_size=S, channels=CH)
    vsq = Subset(dsq, list(range(len(dsq))))
    col = functools.partial(collate_fn_cuda, img_size=S, channels=CH, letterbox=True)
    lb_loader = DataLoader(vsq, batch_size=2, shuffle=False, collate_fn=col, num_workers=0)
    rect_loader = T.rect_val_loader(vsq, range(len(vsq)), 2, S, CH, num_workers=0)
    kw = dict(conf_threshold=P_CONF, iou_threshold=P_IOU, per_class=True, nms_per_class=True, max_det=MAX_DET)
    a = T.validate(model, lb_loader, crit, dev, **kw)
    b = T.validate(model, rect_loader, crit, dev, max_frames=8, **kw)
    assert set(a) == set(b)
    np.testing.assert_equal(b, a)                          # nested, exact; an AP that is NaN in both is equal


def test_trainer_val_rect_epoch_and_predict_rect(tmp_path):
    import json
    _write_dir(tmp_path / "data", VAL_HW + [(90, 160), (160, 90)], seed=41)
    script = ROOT / "yolo-scratch_amd" / "train_yolo11_cuda.py"
    cmd = [sys.executable, str(script), "--data", str(tmp_path / "data"), "--data-format", "yolo", "--ch", str(CH),
           "--nc", str(NC), "--val-rect", "--val-per-class", "--val-nms-per-class", "--epochs", "1", "--batch", "2",
           "--imgsz", str(S), "--scale", "n", "--workers", "0", "--val-split", "0.5", "--save-dir",
           str(tmp_path / "run"), "--resume", str(tmp_path / "none.pt"), "--val-conf", "0.001"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Epoch 1/1" in r.stdout and (tmp_path / "run" / "last.pt").exists()
    ck = torch.load(tmp_path / "run" / "last.pt", map_location="cpu", weights_only=True)
    assert set(ck["val_metrics"]) >= {"loss", "mAP50", "mAP50-95", "precision", "recall"}
    for part in ("train_metrics", "val_metrics"):
        for k in ("loss", "box_loss", "cls_loss", "dfl_loss"):
            assert math.isfinite(ck[part][k]), (part, k, ck[part][k])
    # predict.py --rect on the PNG directory with the weights that run wrote
    out = tmp_path / "out"
    cmd = [sys.executable, str(ROOT / "yolo-scratch_amd" / "predict.py"), "--weights", str(tmp_path / "run" / "last.pt"),
           "--source", str(tmp_path / "data" / "images"), "--scale", "n", "--ch", str(CH), "--nc", str(NC), "--imgsz",
           str(S), "--batch", "2", "--conf", str(P_CONF), "--iou", str(P_IOU), "--max-det", str(MAX_DET), "--rect",
           "--save-dir", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    doc = json.loads((out / "predictions.json").read_text())
    assert [Path(e["image"]).name for e in doc["images"]] == [f"im{i}.png" for i in range(8)]
    hws = VAL_HW + [(90, 160), (160, 90)]
    total = 0
    for i, e in enumerate(doc["images"]):
        assert (e["height"], e["width"]) == hws[i]
        rows = [ln.split() for ln in (out / f"im{i}.txt").read_text().splitlines()]
        assert len(rows) == len(e["scores"]) <= MAX_DET
        total += len(rows)
        for row, lab in zip(rows, e["labels"]):
            assert len(row) == 6 and int(row[0]) == lab and 0 <= int(row[0]) < NC
            assert all(math.isfinite(float(v)) and 0.0 <= float(v) <= 1.0 for v in row[1:]), row
    assert total >= 1
