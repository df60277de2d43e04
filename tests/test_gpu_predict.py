"""From images to source-pixel detections on the GPU: yolomi.predict.Predictor against the composition of its parts
(the restatement's letterbox, the eval forward, decode_nms, the numpy unletterbox), the predict.py command line on a
directory of PNGs with the averaged weights, and one --letterbox epoch of the trainer on a YOLO-txt directory."""
import json
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import letterbox_ref as LR

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
S, NC, CH = 64, 3, 3
HW = [(40, 64), (64, 40), (50, 50)]
CONF, IOU, MAX_DET = 1e-7, 0.45, 50           # the untrained head scores ~1e-6: every image keeps boxes


def _images(seed=21):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (*hw, CH), dtype=np.uint8) for hw in HW]


def _model():
    from test_gpu_model import _seeded_model
    return _seeded_model("n", nc=NC, ch=CH).eval()


def _composition(model, ims, batch):
    """The chain by hand over `batch` images (the last ones empty, as the predictor pads)."""
    from yolomi import post
    padded = ims + [np.zeros((0, 0, CH), np.uint8)] * (batch - len(ims))
    table = LR.entries(padded, S, S)
    img = torch.from_numpy(LR.as_float(LR.render(table, padded, S, S, 114))).cuda()
    with torch.no_grad():
        y = model(img)[0]
    dets = post.decode_nms(y.transpose(1, 2), S, CONF, IOU, class_aware=True, max_det=MAX_DET)[:len(ims)]
    out = []
    for b, d in enumerate(dets):
        k = len(d["scores"])
        boxes = LR.unletterbox(d["boxes"].cpu().numpy()[None], [k], [table[b]], S, S)[0]
        out.append({"boxes": boxes, "scores": d["scores"].cpu().numpy(), "labels": d["labels"].cpu().numpy()})
    return out


@pytest.mark.parametrize("batch", [3, 4])
def test_predictor_equals_the_composition(batch):
    from yolomi.predict import Predictor
    model = _model()
    ims = _images()
    pred = Predictor(model, imgsz=S, ch=CH, conf=CONF, iou=IOU, max_det=MAX_DET, class_aware=True, device="cuda",
                     batch=batch)
    want = _composition(model, ims, batch)
    for _ in range(3):                                     # eager, captured, replayed: the same answer
        got = pred(ims)
        assert len(got) == len(ims)
        for i, (g, w) in enumerate(zip(got, want)):
            n = len(w["scores"])
            assert n >= 1, "the comparison must not pass empty"
            assert len(g["scores"]) == n and n <= MAX_DET, i
            assert np.array_equal(g["labels"].cpu().numpy(), w["labels"]), i
            assert g["scores"].cpu().numpy().tobytes() == w["scores"].tobytes(), i
            assert g["boxes"].cpu().numpy().tobytes() == w["boxes"].tobytes(), i
            h0, w0 = HW[i]
            b = g["boxes"].cpu().numpy()
            assert (b >= 0).all() and (b[:, [0, 2]] <= w0).all() and (b[:, [1, 3]] <= h0).all()
            assert set(w["labels"].tolist()) <= set(range(NC))
    plan = next(p for k, v in model.__dict__["_ym_plans"].items() if not k[-1] for p in v)
    assert "fwd" in plan.__dict__.get("_graphs", {}), "the eval forward was not replayed as a graph"


def test_predictor_batches_and_single_plane():
    """Five images at batch 2 (three forwards, the last padded) equal the same images one at a time at batch 2."""
    from test_gpu_model import _seeded_model
    from yolomi.predict import Predictor
    model = _seeded_model("n", nc=NC, ch=1).eval()
    rng = np.random.default_rng(5)
    ims = [rng.integers(0, 256, hw, dtype=np.uint8) for hw in HW + [(64, 64), (9, 30)]]
    pred = Predictor(model, imgsz=S, conf=CONF, iou=IOU, max_det=MAX_DET, batch=2)
    assert pred.ch == 1
    got = pred(ims)
    assert len(got) == 5
    for im, g in zip(ims, got):
        one = pred([im[..., None]])[0]                     # (h, w, 1) is taken as (h, w)
        assert len(g["scores"]) >= 1
        for k in ("boxes", "scores", "labels"):
            assert torch.equal(one[k], g[k]), k
    with pytest.raises(ValueError):
        pred([np.zeros((4, 4, 3), np.uint8)])
    with pytest.raises(ValueError):
        Predictor(model, imgsz=S, ch=3)


def _write_pngs(root, ims, labels=False):
    from PIL import Image
    (root / "images").mkdir(parents=True)
    if labels:
        (root / "labels").mkdir()
    rng = np.random.default_rng(8)
    for i, a in enumerate(ims):
        Image.fromarray(a).save(root / "images" / f"im{i}.png")
        if labels:
            rows = [f"{int(rng.integers(0, NC))} {rng.uniform(0.3, 0.7):.4f} {rng.uniform(0.3, 0.7):.4f} "
                    f"{rng.uniform(0.2, 0.5):.4f} {rng.uniform(0.2, 0.5):.4f}" for _ in range(int(rng.integers(1, 4)))]
            (root / "labels" / f"im{i}.txt").write_text("\n".join(rows) + "\n")


def test_predict_cli_writes_rows_and_takes_the_averaged_weights(tmp_path):
    import train_yolo11_cuda as T
    from yolomi.predict import Predictor
    ims = _images(seed=33)
    _write_pngs(tmp_path / "src", ims)
    raw, avg = _model(), _model()
    with torch.no_grad():
        for p in avg.parameters():                         # "averaged" weights that differ from the raw ones
            p.mul_(0.97)
    torch.save({"epoch": 0, "model_state_dict": raw.state_dict(), "ema_state_dict": avg.state_dict(),
                "ema_updates": 5}, tmp_path / "w.pt")
    out = tmp_path / "out"
    cmd = [sys.executable, str(ROOT / "yolo-scratch_amd" / "predict.py"), "--weights", str(tmp_path / "w.pt"),
           "--source", str(tmp_path / "src"), "--scale", "n", "--ch", str(CH), "--nc", str(NC), "--imgsz", str(S),
           "--batch", "2", "--conf", str(CONF), "--iou", str(IOU), "--max-det", str(MAX_DET), "--ema", "--save-dir",
           str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Loaded ema_state_dict" in r.stdout
    doc = json.loads((out / "predictions.json").read_text())
    assert doc["state"] == "ema_state_dict" and [Path(e["image"]).name for e in doc["images"]] == [
        "im0.png", "im1.png", "im2.png"]
    want = Predictor(avg, imgsz=S, ch=CH, conf=CONF, iou=IOU, max_det=MAX_DET, batch=2)(ims)
    other = Predictor(raw, imgsz=S, ch=CH, conf=CONF, iou=IOU, max_det=MAX_DET, batch=2)(ims)
    for i, (e, w, o) in enumerate(zip(doc["images"], want, other)):
        assert (e["height"], e["width"]) == HW[i] and len(e["scores"]) >= 1
        assert np.array_equal(np.asarray(e["scores"], np.float32), w["scores"].cpu().numpy()), i
        assert np.array_equal(np.asarray(e["boxes"], np.float32).reshape(-1, 4), w["boxes"].cpu().numpy()), i
        assert e["labels"] == w["labels"].tolist()
        assert not np.array_equal(np.asarray(e["scores"], np.float32), o["scores"].cpu().numpy()), i
        rows = [ln.split() for ln in (out / f"im{i}.txt").read_text().splitlines()]
        assert len(rows) == len(e["scores"])
        for row, lab in zip(rows, e["labels"]):
            assert len(row) == 6 and int(row[0]) == lab and 0 <= int(row[0]) < NC
            vals = [float(v) for v in row[1:]]
            assert all(math.isfinite(v) and 0.0 <= v <= 1.0 for v in vals), row
            cx, cy, w_, h_ = vals[:4]                      # the box lies in the source image
            assert cx - w_ / 2 >= -1e-5 and cx + w_ / 2 <= 1 + 1e-5 and cy - h_ / 2 >= -1e-5 and cy + h_ / 2 <= 1 + 1e-5
    # without the flag, and with it on a checkpoint that has no average: the raw weights
    m = _model()
    assert T.load_checkpoint(tmp_path / "w.pt", m, torch.device("cuda")) == "model_state_dict"
    assert torch.equal(m.model[0].conv.weight, raw.model[0].conv.weight)
    torch.save({"epoch": 0, "model_state_dict": avg.state_dict()}, tmp_path / "plain.pt")
    assert T.load_checkpoint(tmp_path / "plain.pt", m, torch.device("cuda"), ema=True) == "model_state_dict"
    assert torch.equal(m.model[0].conv.weight, avg.model[0].conv.weight)


def test_trainer_letterbox_epoch_on_a_yolo_txt_directory(tmp_path):
    rng = np.random.default_rng(41)
    ims = [rng.integers(0, 256, (int(rng.integers(30, 90)), int(rng.integers(30, 90)), CH), dtype=np.uint8)
           for _ in range(6)]
    _write_pngs(tmp_path / "data", ims, labels=True)
    script = ROOT / "yolo-scratch_amd" / "train_yolo11_cuda.py"
    cmd = [sys.executable, str(script), "--data", str(tmp_path / "data"), "--data-format", "yolo", "--ch", str(CH),
           "--nc", str(NC), "--letterbox", "--augment", "--epochs", "1", "--batch", "2", "--imgsz", str(S), "--scale", "n",
           "--workers", "0", "--save-dir", str(tmp_path / "run"), "--resume", str(tmp_path / "none.pt"), "--val-conf",
           "0.001"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Epoch 1/1" in r.stdout and (tmp_path / "run" / "last.pt").exists()
    ck = torch.load(tmp_path / "run" / "last.pt", map_location="cpu", weights_only=True)
    assert set(ck["val_metrics"]) >= {"loss", "mAP50", "mAP50-95", "precision", "recall"}      # validation ran
    for part in ("train_metrics", "val_metrics"):
        for k in ("loss", "box_loss", "cls_loss", "dfl_loss"):
            assert math.isfinite(ck[part][k]), (part, k, ck[part][k])
