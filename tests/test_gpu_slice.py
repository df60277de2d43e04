"""Sliced inference on the GPU, bit for bit against the numpy restatement (tests/slice_ref.py):
ym_slice_letterbox_u8c over the case list the sanitized host build is held to (tests/test_slice_cpu.py), `out` off the
16-byte grid, three fills, one-tile tables against ym_letterbox_u8c; ym_decode_nms_tiles over two shapes, two class
counts, two layouts of `pred`, the three suppression modes, with and without the tile-border filter, and with a
src = -1 tile inside an image; the argument checks; Predictor(slice=...) against the hand composition of the two
entry points and against the plain Predictor; the predict.py command line."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import augment_ref as AR
import letterbox_ref as LR
import slice_ref as SR

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
IOU = 0.45


def _dev(ims):
    buf, meta = AR.pack(ims)
    return torch.from_numpy(buf).cuda(), torch.from_numpy(meta).cuda()


def _out(T, ch, H, W, offset):
    flat = torch.full((T * ch * H * W + 1,), -1.0, dtype=torch.float32, device="cuda")
    out = flat[1:] if offset else flat[:-1]
    assert out.data_ptr() % 16 == (4 if offset else 0)
    return out.view(T, ch, H, W)


def _slice(ents, ims, H, W, fill=114, offset=False):
    from yolomi._lib import call, stream_ptr
    ch, T = ims[0].shape[2], len(ents)
    u8, meta = _dev(ims)
    out = _out(T, ch, H, W, offset)
    tdev = torch.from_numpy(SR.table_bytes(ents)).cuda()   # named: alive until the launch has run
    call("ym_slice_letterbox_u8c", u8.data_ptr(), meta.data_ptr(), len(ims), tdev.data_ptr(), T, ch, H, W, fill,
         out.data_ptr(), stream_ptr(u8.device))
    return out.cpu().numpy()


def _check_exact(got, want_u8, names):
    want = LR.as_float(want_u8)
    for k, name in enumerate(names):
        assert np.array_equal(got[k], want[k]), (name, int((got[k] != want[k]).sum()))
        assert np.array_equal(np.rint(got[k] * 255.0).astype(np.int64), want_u8[k]), name


# ---------------------------------------------------------------- ym_slice_letterbox_u8c
@pytest.mark.parametrize("H,W", SR.FRAMES)
@pytest.mark.parametrize("ch", [1, 2, 3, 4])
def test_slice_equals_restatement(H, W, ch):
    """The plan of both sources and the hand-made entries in one launch: copies, resizes, windows at the images' last
    row and column, windows that leave the image, src outside the images."""
    ims = SR.sources(ch)
    ents, names, _ = SR.render_cases(H, W)
    for fill in (0, 114, 255):
        _check_exact(_slice(ents, ims, H, W, fill), SR.render(ents, ims, H, W, fill), names)


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_out_offset_by_four_bytes(ch):
    """`out` not 16-byte aligned at a size whose groups would otherwise be vector stores; nothing written outside."""
    from yolomi._lib import call, stream_ptr
    H, W = 32, 48
    ims = SR.sources(ch)
    ents, _, _ = SR.render_cases(H, W)
    assert np.array_equal(_slice(ents, ims, H, W, offset=True), _slice(ents, ims, H, W))
    u8, meta = _dev(ims)
    T = len(ents)
    flat = torch.full((T * ch * H * W + 8,), -1.0, dtype=torch.float32, device="cuda")
    tdev = torch.from_numpy(SR.table_bytes(ents)).cuda()
    call("ym_slice_letterbox_u8c", u8.data_ptr(), meta.data_ptr(), len(ims), tdev.data_ptr(), T, ch, H, W, 114,
         flat[1:].data_ptr(), stream_ptr(u8.device))
    assert float(flat[0]) == -1.0 and (flat[-7:] == -1.0).all() and (flat[1:-7] >= 0.0).all()


@pytest.mark.parametrize("H,W", [(32, 32), (31, 31), (32, 48)])
@pytest.mark.parametrize("ch", [1, 3])
def test_one_tile_table_equals_the_letterbox_kernel(H, W, ch):
    """A table whose one window is the whole image: ym_letterbox_u8c byte for byte, over its own case list."""
    from yolomi._lib import call, stream_ptr
    for im, up in zip(LR.sources(H, W, ch), LR.SCALEUP):
        h0, w0 = im.shape[:2]
        if h0 == 0 or not up:
            continue
        lbt = LR.entries([im], H, W)
        u8, meta = _dev([im])
        want = _out(1, ch, H, W, False)
        lb_dev = torch.from_numpy(np.frombuffer(bytes(lbt), np.uint8)[:32].copy()).cuda()
        call("ym_letterbox_u8c", u8.data_ptr(), meta.data_ptr(), lb_dev.data_ptr(), 1, ch, H, W, 114, want.data_ptr(),
             stream_ptr(u8.device))
        e = SR.entry(0, 0, 0, w0, h0, h0, w0, H, W)
        assert (e.nw, e.nh, e.left, e.top, e.edges) == (lbt[0].nw, lbt[0].nh, lbt[0].left, lbt[0].top, 0)
        got = _slice([e], [im], H, W)
        assert got.tobytes() == want.cpu().numpy().tobytes(), (h0, w0)


# ---------------------------------------------------------------- ym_decode_nms_tiles
def _decode(pred, ents, begin, conf, class_aware, max_det, edge, layout):
    from yolomi import post
    p = torch.from_numpy(np.array(pred)).cuda()
    if layout == "anchor-major":                           # the eval output's (T, 4 + C, N), read through a view
        p = p.permute(0, 2, 1).contiguous().transpose(1, 2)
        assert p.stride(2) == pred.shape[1] and p.stride(1) == 1
    tdev = torch.from_numpy(SR.table_bytes(ents)).cuda()
    return post.decode_nms_tiles(p, tdev, begin, conf, IOU, class_aware=class_aware, max_det=max_det, edge=edge)


def _check_decode(got, ref, N):
    assert got["counts"] == [len(o["scores"]) for o in ref], (got["counts"], [len(o["scores"]) for o in ref])
    assert got["count"].cpu().tolist() == got["counts"]
    for g, o in enumerate(ref):
        k = len(o["scores"])
        assert got["boxes"][g, :k].cpu().numpy().tobytes() == o["boxes"].tobytes(), g
        assert got["scores"][g, :k].cpu().numpy().tobytes() == o["scores"].tobytes(), g
        assert np.array_equal(got["labels"][g, :k].cpu().numpy(), o["labels"]), g
        assert np.array_equal(got["index"][g, :k].cpu().numpy(), o["index"]), g
        assert np.array_equal(got["rows"][g, :k].cpu().numpy(), o["rows"]), g


def _conditions(shape, C, hole, conf, class_aware, edge):
    """On the reference alone, uncapped: no image is empty, the scores are tie-free, and at edge 0 a kept box
    suppresses a candidate of another tile and a coordinate is clamped at a window side; at edge > 0 every one of the
    four bits drops a candidate."""
    base = SR.decode_ref(shape, C, hole, conf, IOU, class_aware, 0, edge)
    best = SR.decode_pred(shape, C, hole)[..., 4:].max(-1)
    assert len(np.unique(best)) == best.size
    assert all(len(o["scores"]) >= 1 for o in base)
    if edge == 0:
        assert sum(SR.cross_tile_suppressions(o, IOU, class_aware) for o in base) >= 1
        assert sum(o["clamped"] for o in base) >= 1
    else:
        assert all(sum(o["cut"][k] for o in base) >= 1 for k in range(4)), [o["cut"] for o in base]
    return base


@pytest.mark.parametrize("edge", [0.0, 4.0])
@pytest.mark.parametrize("mode", ["agnostic", "aware", "capped"])
@pytest.mark.parametrize("C", [5, 80])
@pytest.mark.parametrize("shape", ["small", "large"])
def test_decode_nms_tiles_equals_restatement(shape, C, mode, edge):
    """(G, tiles, N) = (2, {3, 1}, 17), and (1, 4, 2100) at a conf that lets K pass 8192 at edge 0 (the kernel's
    large-K form; the register form at edge 4)."""
    conf = 0.5 if shape == "small" else 0.001
    class_aware = mode != "agnostic"
    max_det = 0 if mode != "capped" else (2 if shape == "small" else 40)
    ents, begin, N = SR.decode_plan(shape)
    base = _conditions(shape, C, False, conf, class_aware, edge)
    if shape == "large" and edge == 0:
        assert len(base[0]["cand_scores"]) > 8192
    ref = SR.decode_ref(shape, C, False, conf, IOU, class_aware, max_det, edge)
    if max_det:
        assert any(len(o["scores"]) == max_det < len(b["scores"]) for o, b in zip(ref, base))
    pred = SR.decode_pred(shape, C)
    for layout in ("contiguous", "anchor-major"):
        got = _decode(pred, ents, begin, conf, class_aware, max_det, edge, layout)
        assert got["boxes"].shape == (len(begin) - 1, N * max(b - a for a, b in zip(begin, begin[1:])), 4)
        _check_decode(got, ref, N)


@pytest.mark.parametrize("edge", [0.0, 4.0])
def test_decode_nms_tiles_skips_a_tile_without_source(edge):
    """src = -1 in the middle of image 0: its rows are no candidates, the rows after it keep their places."""
    ents, begin, N = SR.decode_plan("small", hole=True)
    assert ents[1].src == -1 and begin == [0, 3, 4]
    _conditions("small", 5, True, 0.5, True, edge)
    ref = SR.decode_ref("small", 5, True, 0.5, IOU, True, 0, edge)
    assert not (ref[0]["rows"] // N == 1).any() and (ref[0]["rows"] // N == 2).any()
    pred = np.array(SR.decode_pred("small", 5, True))
    pred[1] = np.nan                                       # never read
    got = _decode(pred, ents, begin, 0.5, True, 0, edge, "contiguous")
    _check_decode(got, ref, N)


def test_decode_nms_tiles_argument_checks():
    from yolomi._lib import lib, stream_ptr
    import ctypes
    L = lib()
    ents, begin, N = SR.decode_plan("small")
    pred = torch.from_numpy(np.array(SR.decode_pred("small", 5))).cuda()
    T, C, G, R = 4, 5, 2, 3 * N
    tdev = torch.from_numpy(SR.table_bytes(ents)).cuda()
    nb = L.ym_decode_nms_tiles_workspace_size(G, R, 1)
    assert nb >= G * R * 32 and L.ym_decode_nms_tiles_workspace_size(G, R, 0) == nb
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    cnt = torch.full((G,), -7, dtype=torch.int32, device="cuda")
    boxes = torch.empty(G, R, 4, device="cuda")
    scores = torch.empty(G, R, device="cuda")
    i64 = [torch.empty(G, R, dtype=torch.int64, device="cuda") for _ in range(3)]
    st = stream_ptr(pred.device)

    def run(begin=begin, G=G, T=T, N=N, edge=0.0, cls=1, max_det=0, nbytes=nb):
        cb = (ctypes.c_int64 * len(begin))(*begin)
        return L.ym_decode_nms_tiles(pred.data_ptr(), T, N, C, 4 + C, N * (4 + C), 1, tdev.data_ptr(), cb, G, 0.5, IOU,
                                     edge, cls, max_det, ws.data_ptr(), nbytes, cnt.data_ptr(), boxes.data_ptr(),
                                     scores.data_ptr(), *(t.data_ptr() for t in i64), st)

    assert run(G=-1) == -1
    assert run(begin=[0, 3, 2]) == -1 and b"monotone" in L.ym_last_error()
    assert run(begin=[0, 3, 5]) == -1                      # tile_begin[G] > T
    assert run(begin=[-1, 3, 4]) == -1
    assert run(begin=[0, 2, 2], T=2, N=1 << 29) == -1 and b"too large" in L.ym_last_error()
    assert run(edge=float("nan")) == -1
    assert run(max_det=-1) == -1
    assert run(cls=0, max_det=5) == -1
    assert run(nbytes=nb - 257) == -1 and b"workspace" in L.ym_last_error()
    torch.cuda.synchronize()
    assert (cnt == -7).all()                               # nothing was launched
    assert run() == 0 and run(edge=-1.0) == 0 and run(edge=float("inf")) == 0 and run(G=0, begin=[0]) == 0
    torch.cuda.synchronize()
    assert (cnt >= 0).all()
    # out_row may be NULL
    cb = (ctypes.c_int64 * 3)(*begin)
    assert L.ym_decode_nms_tiles(pred.data_ptr(), T, N, C, 4 + C, N * (4 + C), 1, tdev.data_ptr(), cb, G, 0.5, IOU, 0.0,
                                 1, 0, ws.data_ptr(), nb, cnt.data_ptr(), boxes.data_ptr(), scores.data_ptr(),
                                 i64[0].data_ptr(), i64[1].data_ptr(), None, st) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the Predictor
from test_gpu_predict import CH, CONF, MAX_DET, NC, S, _model, _write_pngs  # noqa: E402

HW = [(50, 70), (33, 33)]
TILE, OVERLAP = 32, 0.2


def _images(seed=61, hw=HW):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (*s, CH), dtype=np.uint8) for s in hw]


def _composition(model, ims, batch, full, edge):
    """The chain by hand: the tiles `batch` at a time (the last chunk padded with src = -1 entries, as the predictor
    pads) through ym_slice_letterbox_u8c and the eval forward, then one ym_decode_nms_tiles; and the restatement of
    the decode over the same forward output."""
    from datasets.slicing import slice_batch
    from yolomi import post
    ents, begin = SR.entries([a.shape[:2] for a in ims], TILE, OVERLAP, S, None, full)
    T = len(ents)
    padded = ents + [SR.entry(-1, 0, 0, 0, 0, 0, 0, S) for _ in range(-T % batch)]
    u8, meta = _dev(ims)
    tdev = torch.from_numpy(SR.table_bytes(padded)).cuda()
    want_img = LR.as_float(SR.render(padded, ims, S, S, 114))
    ys = []
    with torch.no_grad():
        for lo in range(0, len(padded), batch):
            img = slice_batch(u8, meta, tdev, batch, S, S, CH, 114, first=lo)
            assert np.array_equal(img.cpu().numpy(), want_img[lo:lo + batch])
            ys.append(model(img)[0].clone())
    y = torch.cat(ys)[:T]
    d = post.decode_nms_tiles(y.transpose(1, 2), tdev, begin, CONF, IOU, class_aware=True, max_det=MAX_DET, edge=edge)
    ref = SR.decode_tiles(y.transpose(1, 2).cpu().numpy(), ents, begin, CONF, IOU, True, MAX_DET, edge)
    return d, ref, begin


@pytest.mark.parametrize("batch,full,edge", [(4, True, 0.0), (3, True, 4.0), (4, False, 0.0)])
def test_predictor_sliced_equals_the_composition(batch, full, edge):
    from yolomi.predict import Predictor
    model = _model()
    ims = _images()
    pred = Predictor(model, imgsz=S, ch=CH, conf=CONF, iou=IOU, max_det=MAX_DET, class_aware=True, device="cuda",
                     batch=batch, slice=TILE, slice_overlap=OVERLAP, slice_full=full, slice_edge=edge)
    d, ref, begin = _composition(model, ims, batch, full, edge)
    assert begin == ([0, 7, 12] if full else [0, 6, 10])              # 50 x 70: 2 x 3 windows; 33 x 33: 2 x 2
    for _ in range(3):                                     # eager, captured, replayed: the same answer
        got = pred(ims)
        assert len(got) == len(ims)
        for g, (o, r) in enumerate(zip(got, ref)):
            n = len(r["scores"])
            assert n >= 1, "the comparison must not pass empty"
            assert d["counts"][g] == n == len(o["scores"]) and n <= MAX_DET
            for key in ("boxes", "scores", "labels"):
                assert torch.equal(o[key], d[key][g, :n]), (g, key)
            assert o["boxes"].cpu().numpy().tobytes() == r["boxes"].tobytes(), g
            assert o["scores"].cpu().numpy().tobytes() == r["scores"].tobytes(), g
            assert np.array_equal(o["labels"].cpu().numpy(), r["labels"]), g
            h0, w0 = HW[g]
            b = o["boxes"].cpu().numpy()
            assert (b >= 0).all() and (b[:, [0, 2]] <= w0).all() and (b[:, [1, 3]] <= h0).all()
    plan = next(p for k, v in model.__dict__["_ym_plans"].items() if not k[-1] for p in v)
    assert "fwd" in plan.__dict__.get("_graphs", {}), "the eval forward was not replayed as a graph"


def test_predictor_sliced_keeps_input_order_and_groups():
    """Three sources at batch 2 (two groups): each result is the source's own, whatever its place and neighbours."""
    from yolomi.predict import Predictor
    model = _model()
    a, b = _images()
    c = _images(seed=62, hw=[(20, 30)])[0]
    pred = Predictor(model, imgsz=S, ch=CH, conf=CONF, iou=IOU, max_det=MAX_DET, batch=2, slice=TILE,
                     slice_overlap=OVERLAP)
    one = [pred([im])[0] for im in (a, b, c)]
    for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0]):
        got = pred([(a, b, c)[i] for i in order])
        assert len(got) == 3
        for o, i in zip(got, order):
            assert len(o["scores"]) >= 1
            for key in ("boxes", "scores", "labels"):
                assert torch.equal(o[key], one[i][key]), (order, i, key)
    assert not torch.equal(one[0]["boxes"], one[1]["boxes"])
    assert pred([]) == []


def test_small_source_equals_the_plain_predictor():
    """A source no larger than the tile, without the whole-image pass: its one window is the image, so the letterboxed
    frame, the forward and the candidates are the plain Predictor's.  The two differ in where a box meets the image's
    border: the plain path suppresses in frame pixels and clamps afterwards, the sliced one clamps when it maps and
    suppresses in source pixels, so the kept sets are the same by construction only when nothing is suppressed:
    iou = 1 here (no IoU exceeds it), both keep the max_det best candidates in the same order.

    The bound on a coordinate, for a frame coordinate x in [0, S]: the plain path carries x' = fl(fl(x / S) * S)
    through the map, |x' - x| <= 2 * 2^-24 * S; both then form min(max(fl(fl(z - left) * s), 0), lim) with s = sx or
    sy, where the subtraction is off by at most 2^-24 * S and the product by at most 2^-24 * S * s, in each path.
    Together |difference| <= s * (2 + 2) * 2^-24 * S + 2 * 2^-24 * S * s = 6 * 2^-24 * S * s < 2^-21 * S * s.  For x
    outside [0, S] the plain path maps 0 or S, which the clamp takes to 0 or to within 2^-23 * lim of lim, where the
    sliced path's value lies too (the map is monotone).  S = 64 and s < 1: 2^-21 * 64 * max(sx, sy) pixels."""
    from yolomi.predict import Predictor
    model = _model()
    ims = _images(seed=63, hw=[(24, 30), (32, 32), (7, 32)])
    kw = dict(imgsz=S, ch=CH, conf=CONF, iou=1.0, max_det=MAX_DET, class_aware=True, device="cuda", batch=2)
    plain = Predictor(model, **kw)(ims)
    sliced = Predictor(model, slice=TILE, slice_overlap=OVERLAP, slice_full=False, **kw)(ims)
    for im, p, s in zip(ims, plain, sliced):
        h0, w0 = im.shape[:2]
        nw, nh, _, _ = LR.geometry(h0, w0, S, S)
        bound = 2.0 ** -21 * S * max(w0 / nw, h0 / nh)
        n = len(p["scores"])
        assert n >= 1 and len(s["scores"]) == n
        assert torch.equal(p["scores"], s["scores"]) and torch.equal(p["labels"], s["labels"])
        worst = float((p["boxes"].double() - s["boxes"].double()).abs().max())
        print(f"{h0} x {w0}: {n} boxes, worst coordinate difference {worst:.3e} px (bound {bound:.3e})")
        assert worst <= bound


def test_slice_with_rect_raises():
    from yolomi.predict import Predictor
    model = _model()
    with pytest.raises(ValueError):
        Predictor(model, imgsz=S, ch=CH, rect=True, slice=TILE)
    with pytest.raises(ValueError):
        Predictor(model, imgsz=S, ch=CH, slice=TILE, slice_overlap=1.0)
    with pytest.raises(ValueError):
        Predictor(model, imgsz=S, ch=CH, slice=-1)
    assert Predictor(model, imgsz=S, ch=CH).slice == 0


def test_predict_cli_slices(tmp_path):
    from yolomi.predict import Predictor
    ims = _images(seed=64)
    _write_pngs(tmp_path / "src", ims)
    model = _model()
    torch.save({"epoch": 0, "model_state_dict": model.state_dict()}, tmp_path / "w.pt")
    out = tmp_path / "out"
    cmd = [sys.executable, str(ROOT / "yolo-scratch_amd" / "predict.py"), "--weights", str(tmp_path / "w.pt"),
           "--source", str(tmp_path / "src"), "--scale", "n", "--ch", str(CH), "--nc", str(NC), "--imgsz", str(S),
           "--batch", "2", "--conf", str(CONF), "--iou", str(IOU), "--max-det", str(MAX_DET), "--slice", str(TILE),
           "--slice-overlap", str(OVERLAP), "--slice-edge", "2", "--save-dir", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    doc = json.loads((out / "predictions.json").read_text())
    want = Predictor(model, imgsz=S, ch=CH, conf=CONF, iou=IOU, max_det=MAX_DET, batch=2, slice=TILE,
                     slice_overlap=OVERLAP, slice_edge=2.0)(ims)
    for i, (e, w) in enumerate(zip(doc["images"], want)):
        assert (e["height"], e["width"]) == HW[i] and len(e["scores"]) >= 1
        assert np.array_equal(np.asarray(e["scores"], np.float32), w["scores"].cpu().numpy()), i
        assert np.array_equal(np.asarray(e["boxes"], np.float32).reshape(-1, 4), w["boxes"].cpu().numpy()), i
        assert e["labels"] == w["labels"].tolist()
        assert len((out / f"im{i}.txt").read_text().splitlines()) == len(e["scores"])
