"""Test-time augmentation on the GPU, bit for bit against the numpy restatement (tests/tta_ref.py, whose
inputs tests/test_tta_cpu.py holds to the conditions that make the comparison mean something): ym_slice_letterbox_u8c
with the mirror bits over the case list the sanitized host build is held to; ym_decode_nms_tiles and
ym_decode_nmm_tiles over mirrored entries; ym_decode_nmw_tiles, the score-weighted mean in fixed point, over nmm_ref's
shapes (the register form, K > 8192, K > 16384); Predictor(tta=...) against the hand composition, the restatement and
the mirror symmetry; the command line."""
import ctypes
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import augment_ref as AR
import letterbox_ref as LR
import nmm_ref as MR
import slice_ref as SR
import tta_ref as TR

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
BITS = (0, 16, 32, 48)


def _dev(ims):
    buf, meta = AR.pack(ims)
    return torch.from_numpy(buf).cuda(), torch.from_numpy(meta).cuda()


def _slice(ents, ims, H, W, fill=114, offset=False):
    """ym_slice_letterbox_u8c -> (tiles as numpy, the floats before and after `out`)."""
    from yolomi._lib import call, stream_ptr
    ch, T = ims[0].shape[2], len(ents)
    u8, meta = _dev(ims)
    n = T * ch * H * W
    flat = torch.full((n + 8,), -1.0, dtype=torch.float32, device="cuda")
    first = 1 if offset else 4
    out = flat[first:first + n]
    assert out.data_ptr() % 16 == (4 if offset else 0)
    tdev = torch.from_numpy(SR.table_bytes(ents)).cuda()   # named: alive until the launch has run
    call("ym_slice_letterbox_u8c", u8.data_ptr(), meta.data_ptr(), len(ims), tdev.data_ptr(), T, ch, H, W, fill,
         out.data_ptr(), stream_ptr(u8.device))
    flat = flat.cpu().numpy()
    return flat[first:first + n].reshape(T, ch, H, W), np.concatenate([flat[:first], flat[first + n:]])


def _mirrored_cases(H, W):
    ents, names, _ = SR.render_cases(H, W)
    return ([TR.with_bits(e, b) for b in BITS for e in ents], [f"{n}/{b}" for b in BITS for n in names], len(ents))


# ---------------------------------------------------------------- ym_slice_letterbox_u8c
@pytest.mark.parametrize("H,W", SR.FRAMES)
@pytest.mark.parametrize("ch", [1, 2, 3, 4])
def test_mirrored_slice_equals_reversed_restatement(H, W, ch):
    """Every case of the list with the four settings of the mirror bits in one table: copies, resizes, windows at the
    images' last row and column, windows that leave the image and src outside the images (all fill whatever the bits);
    the entries with the bits clear, beside the mirrored ones, are slice_ref's tiles."""
    ims = SR.sources(ch)
    ents, names, n = _mirrored_cases(H, W)
    fill = 114
    got, _ = _slice(ents, ims, H, W, fill)
    want_u8 = TR.render(ents, ims, H, W, fill)
    want = LR.as_float(want_u8)
    for k, name in enumerate(names):
        assert np.array_equal(got[k], want[k]), (name, int((got[k] != want[k]).sum()))
    assert np.array_equal(want_u8[:n], SR.render(ents[:n], ims, H, W, fill))
    changed = [not np.array_equal(want_u8[k], want_u8[k % n]) for k in range(n, 4 * n)]
    assert sum(changed) >= 3 * 13                           # the bits are not ignored
    for k, name in enumerate(names):
        if name.split("/")[0].startswith(("leaves", "negative", "no-src", "src-past", "zero")):
            assert (got[k] == np.float32(fill) / np.float32(255)).all(), name


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_mirrored_slice_with_out_off_the_vector_grid(ch):
    """`out` 4 bytes off the 16-byte grid at a size whose groups would otherwise be vector stores: the same tiles, and
    nothing written outside them."""
    H, W = 32, 48
    ims = SR.sources(ch)
    ents, _, _ = _mirrored_cases(H, W)
    a, ga = _slice(ents, ims, H, W, offset=True)
    b, gb = _slice(ents, ims, H, W)
    assert np.array_equal(a, b) and (a >= 0).all()
    assert (ga == -1.0).all() and (gb == -1.0).all() and len(ga) == 8


# ---------------------------------------------------------------- ym_decode_nms_tiles / ym_decode_nmm_tiles, mirrored
def _tensor(pred, layout):
    p = torch.from_numpy(np.array(pred)).cuda()
    if layout == "anchor-major":                           # the eval output's (T, 4 + C, N), read through a view
        p = p.permute(0, 2, 1).contiguous().transpose(1, 2)
        assert p.stride(2) == pred.shape[1] and p.stride(1) == 1
    return p


def _check(got, ref, merged=True):
    want = [len(o["scores"]) for o in ref]
    assert got["counts"] == want, (got["counts"], want)
    assert got["count"].cpu().tolist() == got["counts"] and min(want) >= 1
    for g, o in enumerate(ref):
        k = len(o["scores"])
        assert got["boxes"][g, :k].cpu().numpy().tobytes() == o["boxes"].tobytes(), g
        assert got["scores"][g, :k].cpu().numpy().tobytes() == o["scores"].tobytes(), g
        assert np.array_equal(got["labels"][g, :k].cpu().numpy(), o["labels"]), g
        assert np.array_equal(got["index"][g, :k].cpu().numpy(), o["index"]), g
        assert np.array_equal(got["rows"][g, :k].cpu().numpy(), o["rows"]), g
        if merged:
            assert np.array_equal(got["merged"][g, :k].cpu().numpy(), o["merged"]), g


@pytest.mark.parametrize("edge", [0.0, 4.0])
@pytest.mark.parametrize("mode", ["agnostic", "aware", "capped"])
@pytest.mark.parametrize("C", [5, 80])
def test_mirrored_decode_equals_restatement(C, mode, edge):
    """(G, tiles, N) = (2, {4, 2}, 17): tiles mirrored in x, in y, in both, and a reduced mirrored view, beside plain
    ones; the NMS, the greedy merge with the union (IoS) and without (IoU), and the mean."""
    from yolomi import post
    class_aware = mode != "agnostic"
    max_det = 2 if mode == "capped" else 0
    ents, begin, N = TR.decode_plan()
    tdev = torch.from_numpy(SR.table_bytes(ents)).cuda()
    kw = dict(class_aware=class_aware, max_det=max_det, edge=edge)
    for layout in ("contiguous", "anchor-major"):
        p = _tensor(TR.decode_pred(C), layout)
        got = post.decode_nms_tiles(p, tdev, begin, TR.DEC_CONF, TR.DEC_THR, **kw)
        assert got["boxes"].shape == (2, 4 * N, 4)
        _check(got, TR.decode_ref(C, "nms", "iou", class_aware, max_det, edge), merged=False)
        got = post.decode_nmm_tiles(p, tdev, begin, TR.DEC_CONF, TR.DEC_THR, metric="ios", merge=True, **kw)
        _check(got, TR.decode_ref(C, "nmm", "ios", class_aware, max_det, edge))
        got = post.decode_nmm_tiles(p, tdev, begin, TR.DEC_CONF, TR.DEC_THR, metric="iou", merge=False, **kw)
        _check(got, TR.decode_ref(C, "match", "iou", class_aware, max_det, edge))
        got = post.decode_nmw_tiles(p, tdev, begin, TR.DEC_CONF, TR.DEC_THR, metric="ios", **kw)
        _check(got, TR.decode_ref(C, "mean", "ios", class_aware, max_det, edge))


# ---------------------------------------------------------------- ym_decode_nmw_tiles
def _cap(shape, mode):
    return 0 if mode != "capped" else (2 if shape == "small" else 40)


@pytest.mark.parametrize("mode", ["agnostic", "aware", "capped"])
@pytest.mark.parametrize("metric", ["iou", "ios"])
@pytest.mark.parametrize("shape,C", [("small", 5), ("small", 80), ("large", 5)])
def test_decode_nmw_tiles_equals_restatement(shape, C, metric, mode):
    """nmm_ref's plans: (2, {5, 1}, 17), and (2, {5, 1}, 2100), where K = 10500 > 8192 on image 0 (the kernel's
    large-K form, the absorbing slots in the flag words)."""
    from yolomi import post
    class_aware = mode != "agnostic"
    max_det = _cap(shape, mode)
    ents, begin, N = MR.plan(shape)
    ref = TR.mean_ref(shape, C, metric, class_aware, max_det)
    if shape == "large":
        assert len(ref[0]["cand_scores"]) > 8192
    if metric == "ios" and not max_det:
        head = TR.mean_ref(shape, C, metric, class_aware, max_det, how="match")
        assert (ref[0]["merged"] >= 2).any() and (ref[0]["merged"] == 0).any()
        assert (ref[0]["boxes"] != head[0]["boxes"]).any()
    tdev = torch.from_numpy(SR.table_bytes(ents)).cuda()
    for layout in ("contiguous", "anchor-major"):
        got = post.decode_nmw_tiles(_tensor(MR.pred(shape, C), layout), tdev, begin, TR.MEAN_CONF[shape], MR.THR,
                                    metric=metric, class_aware=class_aware, max_det=max_det)
        assert got["boxes"].shape == (len(begin) - 1, 5 * N, 4)
        _check(got, ref)


def test_decode_nmw_tiles_sorts_in_global_memory():
    """(1, 5, 3400): K = 17000 > 16384, the keys are sorted in global memory; IoS, class-agnostic."""
    from yolomi import post
    ents, begin, N = MR.plan("global")
    ref = TR.mean_ref("global", 5, "ios", False, 0)
    assert len(ref[0]["cand_scores"]) > 16384 and (ref[0]["merged"] >= 2).any()
    tdev = torch.from_numpy(SR.table_bytes(ents)).cuda()
    got = post.decode_nmw_tiles(_tensor(MR.pred("global", 5), "contiguous"), tdev, begin, TR.MEAN_CONF["global"],
                                MR.THR, metric="ios")
    _check(got, ref)


def _raw(metric=1, thr=MR.THR, merged=True, **kw):
    """ym_decode_nmw_tiles called through ctypes over nmm_ref's small plan -> (return code, buffers)."""
    from yolomi._lib import lib, stream_ptr
    L = lib()
    ents, begin, N = MR.plan("small")
    pred = torch.from_numpy(np.array(MR.pred("small", 5))).cuda()
    T, C, G, R = 6, 5, 2, 5 * N
    tdev = torch.from_numpy(SR.table_bytes(ents)).cuda()
    nb = L.ym_decode_nmw_tiles_workspace_size(G, R, 1)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    cnt = torch.full((G,), -7, dtype=torch.int32, device="cuda")
    boxes = torch.empty(G, R, 4, device="cuda")
    scores = torch.empty(G, R, device="cuda")
    i64 = [torch.empty(G, R, dtype=torch.int64, device="cuda") for _ in range(3)]
    mg = torch.full((G, R), -7, dtype=torch.int32, device="cuda")
    a = dict(begin=begin, G=G, T=T, N=N, edge=0.0, cls=1, max_det=0, nbytes=nb)
    a.update(kw)
    cb = (ctypes.c_int64 * len(a["begin"]))(*a["begin"])
    rc = L.ym_decode_nmw_tiles(pred.data_ptr(), a["T"], a["N"], C, 4 + C, a["N"] * (4 + C), 1, tdev.data_ptr(), cb,
                               a["G"], TR.MEAN_CONF["small"], thr, metric, a["edge"], a["cls"], a["max_det"],
                               ws.data_ptr(), a["nbytes"], cnt.data_ptr(), boxes.data_ptr(), scores.data_ptr(),
                               *(t.data_ptr() for t in i64), mg.data_ptr() if merged else None,
                               stream_ptr(pred.device))
    torch.cuda.synchronize()
    return rc, dict(count=cnt, boxes=boxes, scores=scores, labels=i64[0], index=i64[1], rows=i64[2], merged=mg)


def test_out_merged_may_be_null_and_calls_repeat():
    """Without out_merged the same means (the weight sums tell which heads absorbed), out_merged untouched; two calls
    back to back give the same bytes (the accumulators need no memset between them)."""
    ref = TR.mean_ref("small", 5, "ios", True, 0)
    rc, a = _raw(merged=False)
    rc2, b = _raw()
    rc3, c = _raw()
    assert rc == 0 and rc2 == 0 and rc3 == 0 and (a["merged"] == -7).all()
    assert a["count"].tolist() == [len(o["scores"]) for o in ref]
    for g, o in enumerate(ref):
        k = len(o["scores"])
        assert a["boxes"][g, :k].cpu().numpy().tobytes() == o["boxes"].tobytes(), g
        for key in ("boxes", "scores", "labels", "index", "rows"):
            assert torch.equal(a[key][g, :k], b[key][g, :k]) and torch.equal(b[key][g, :k], c[key][g, :k]), (g, key)
        assert torch.equal(b["merged"][g, :k], c["merged"][g, :k])
        assert np.array_equal(b["merged"][g, :k].cpu().numpy(), o["merged"])
    assert (ref[0]["merged"] >= 1).any()


def test_decode_nmw_tiles_argument_checks():
    from yolomi._lib import lib
    L = lib()
    nb = L.ym_decode_nmw_tiles_workspace_size(2, 85, 1)

    def bad(msg=None, **kw):
        rc, out = _raw(**kw)
        assert rc == -1, kw
        if msg:
            assert msg in L.ym_last_error(), (kw, L.ym_last_error())
        assert (out["count"] == -7).all(), kw                 # nothing was launched
        assert b"ym_decode_nmw_tiles" in L.ym_last_error()

    bad(b"metric", metric=2)
    bad(b"metric", metric=-1)
    bad(b"match_thr", thr=float("nan"))
    bad(G=-1, begin=[0])
    bad(b"monotone", begin=[0, 5, 4])
    bad(begin=[0, 5, 7])                                      # tile_begin[G] > T
    bad(begin=[-1, 5, 6])
    bad(b"too large", begin=[0, 2, 2], T=2, N=1 << 29)
    bad(b"int64 sums", begin=[0, 1, 2], T=2, N=1 << 26)      # R = 2^26: the sums could overflow
    bad(b"int64 sums", begin=[0, 2, 2], T=2, N=1 << 25)
    bad(edge=float("nan"))
    bad(max_det=-1)
    bad(cls=0, max_det=5)
    bad(b"workspace", nbytes=nb - 257)
    bad(b"workspace", nbytes=L.ym_decode_nmm_tiles_workspace_size(2, 85, 1))     # the union's size is too small
    for kw in (dict(), dict(metric=0), dict(thr=float("inf")), dict(thr=-1.0), dict(edge=float("inf"))):
        rc, out = _raw(**kw)
        assert rc == 0 and (out["count"] >= 0).all(), kw
    assert _raw(G=0, begin=[0])[0] == 0


def test_unknown_metric_raises():
    from yolomi import post
    ents, begin, _ = MR.plan("small")
    tdev = torch.from_numpy(SR.table_bytes(ents)).cuda()
    with pytest.raises(ValueError):
        post.decode_nmw_tiles(_tensor(MR.pred("small", 5), "contiguous"), tdev, begin, 0.5, 0.5, metric="giou")


# ---------------------------------------------------------------- the Predictor
from test_gpu_predict import CH, CONF, MAX_DET, NC, S, _model, _write_pngs  # noqa: E402

HW = [(50, 70), (33, 33)]
TILE, OVERLAP, IOU = 32, 0.2, 0.45


def _images(seed=81, hw=HW):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (*s, CH), dtype=np.uint8) for s in hw]


def _kw(**more):
    return dict(imgsz=S, ch=CH, conf=CONF, iou=IOU, max_det=MAX_DET, class_aware=True, device="cuda", **more)


def _forward(model, ims, batch, views, tile):
    """The slice kernel and the model by hand over tta_ref's table, `batch` tiles at a time (the rendered tiles held
    to the reversed restatement) -> (y (T, 4 + nc, A), table, entries, begin)."""
    from datasets.slicing import slice_batch
    ents, begin = TR.view_entries([a.shape[:2] for a in ims], views, S, tile, OVERLAP, True)
    T = len(ents)
    padded = ents + [SR.entry(-1, 0, 0, 0, 0, 0, 0, S) for _ in range(-T % batch)]
    u8, meta = _dev(ims)
    tdev = torch.from_numpy(SR.table_bytes(padded)).cuda()
    want_img = LR.as_float(TR.render(padded, ims, S, S, 114))
    ys = []
    with torch.no_grad():
        for lo in range(0, len(padded), batch):
            img = slice_batch(u8, meta, tdev, batch, S, S, CH, 114, first=lo)
            assert np.array_equal(img.cpu().numpy(), want_img[lo:lo + batch])
            ys.append(model(img)[0].clone())
    return torch.cat(ys)[:T], tdev, ents, begin


def test_one_plain_view_equals_the_sliced_predictor():
    """(a) tta = [(1, "")] is sliced inference over windows no smaller than the sources, without the extra pass."""
    from yolomi.predict import Predictor
    model = _model()
    ims = _images()
    a = Predictor(model, tta=[(1, "")], batch=2, **_kw())(ims)
    b = Predictor(model, slice=128, slice_full=False, batch=2, **_kw())(ims)
    for x, y in zip(a, b):
        assert len(x["scores"]) >= 1 and sorted(x) == sorted(y) == ["boxes", "labels", "scores"]
        for key in x:
            assert torch.equal(x[key], y[key]), key


@pytest.mark.parametrize("tile,batch", [(0, 4), (TILE, 3)])
def test_predictor_tta_equals_the_composition(tile, batch):
    """(b) the default views, with and without slicing: ym_decode_nms_tiles over the same forward output with
    tta_ref's table, and the numpy restatement; eager, captured and replayed."""
    from datasets.tta import DEFAULT_VIEWS
    from yolomi import post
    from yolomi.predict import Predictor
    model = _model()
    ims = _images()
    pred = Predictor(model, tta=True if tile == 0 else list(DEFAULT_VIEWS), batch=batch, slice=tile,
                     slice_overlap=OVERLAP, **_kw())
    y, tdev, ents, begin = _forward(model, ims, batch, list(DEFAULT_VIEWS), tile)
    assert begin == ([0, 3, 6] if tile == 0 else [0, 21, 36])
    d = post.decode_nms_tiles(y.transpose(1, 2), tdev, begin, CONF, IOU, class_aware=True, max_det=MAX_DET)
    ref = TR.decode_tiles(y.transpose(1, 2).cpu().numpy(), ents, begin, CONF, IOU, "nms", "iou", True, MAX_DET, 0.0)
    for _ in range(3):
        got = pred(ims)
        assert len(got) == len(ims)
        for g, (o, r) in enumerate(zip(got, ref)):
            n = len(r["scores"])
            assert n >= 1 and d["counts"][g] == n == len(o["scores"]) and sorted(o) == ["boxes", "labels", "scores"]
            for key in ("boxes", "scores", "labels"):
                assert torch.equal(o[key], d[key][g, :n]), (g, key)
            assert o["boxes"].cpu().numpy().tobytes() == r["boxes"].tobytes(), g
            assert o["scores"].cpu().numpy().tobytes() == r["scores"].tobytes(), g
            assert np.array_equal(o["labels"].cpu().numpy(), r["labels"]), g
            views_kept = {int(t) for t in r["cand_tiles"][r["index"]]}
            assert len(views_kept) >= 2, "the kept boxes come from one view only"


def test_predictor_tta_keeps_input_order_and_groups():
    """Three sources at batch 2 (two groups): each result is the source's own, whatever its place and neighbours."""
    from yolomi.predict import Predictor
    model = _model()
    a, b = _images()
    c = _images(seed=82, hw=[(20, 30)])[0]
    pred = Predictor(model, tta=True, batch=2, slice_merge="mean", **_kw())
    one = [pred([im])[0] for im in (a, b, c)]
    for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0]):
        got = pred([(a, b, c)[i] for i in order])
        assert len(got) == 3
        for o, i in zip(got, order):
            assert len(o["scores"]) >= 1
            for key in ("boxes", "scores", "labels", "merged"):
                assert torch.equal(o[key], one[i][key]), (order, i, key)
    assert pred([]) == []
    empty = pred([np.zeros((0, 0, CH), np.uint8)])[0]
    assert sorted(empty) == ["boxes", "labels", "merged", "scores"] and all(len(v) == 0 for v in empty.values())


@pytest.mark.parametrize("flip", ["lr", "ud", "lrud"])
def test_mirror_symmetry(flip):
    """(c) An S x S source is a copy in the frame, so the view `flip` of I is the plain view of I mirrored on the
    host: the same frame, forward and candidates.  iou = 1 suppresses nothing (the reasoning of
    test_small_source_equals_the_plain_predictor), both keep the max_det best in the same order, and the boxes are
    each other's images through the mirror: x1 = fp32(w0) - x2', x2 = fp32(w0) - x1', exactly."""
    from yolomi.predict import Predictor
    model = _model()
    im = _images(seed=83, hw=[(S, S)])[0]
    host = im
    if "lr" in flip:
        host = host[:, ::-1]
    if "ud" in flip:
        host = host[::-1]
    kw = _kw(batch=1)
    kw["iou"] = 1.0
    a = Predictor(model, tta=[(1, flip)], **kw)([im])[0]
    b = Predictor(model, tta=[(1, "")], **kw)([np.ascontiguousarray(host)])[0]
    n = len(a["scores"])
    assert n >= 1 and n == len(b["scores"])
    assert torch.equal(a["scores"], b["scores"]) and torch.equal(a["labels"], b["labels"])
    x = b["boxes"].clone()
    side = torch.tensor(float(S), dtype=torch.float32, device=x.device)
    if "lr" in flip:
        x[:, 0], x[:, 2] = side - b["boxes"][:, 2], side - b["boxes"][:, 0]
    if "ud" in flip:
        x[:, 1], x[:, 3] = side - b["boxes"][:, 3], side - b["boxes"][:, 1]
    assert torch.equal(a["boxes"], x)
    assert not torch.equal(a["boxes"], b["boxes"])


@pytest.mark.parametrize("metric", ["iou", "ios"])
def test_predictor_mean_equals_the_restatement(metric):
    """(d) slice_merge = "mean": ym_decode_nmw_tiles over the same forward output, and tta_ref.nmw; "merged" comes
    back.  The head is untrained, so how much its boxes overlap across views is not ours to choose: three match
    thresholds, and at least one of them must form a mean."""
    from datasets.tta import DEFAULT_VIEWS
    from yolomi import post
    from yolomi.predict import Predictor
    model = _model()
    ims = _images()
    batch = 4
    y, tdev, ents, begin = _forward(model, ims, batch, list(DEFAULT_VIEWS), 0)
    absorbed = moved = 0
    for thr in (IOU, 0.1, 0.01):
        kw = _kw(batch=batch)
        kw["iou"] = thr
        pred = Predictor(model, tta=True, slice_merge="mean", slice_metric=metric, **kw)
        d = post.decode_nmw_tiles(y.transpose(1, 2), tdev, begin, CONF, thr, metric=metric, class_aware=True,
                                  max_det=MAX_DET)
        yn = y.transpose(1, 2).cpu().numpy()
        ref = TR.decode_tiles(yn, ents, begin, CONF, thr, "mean", metric, True, MAX_DET, 0.0)
        head = TR.decode_tiles(yn, ents, begin, CONF, thr, "match", metric, True, MAX_DET, 0.0)
        print(thr, [int(r["merged"].sum()) for r in ref], "candidates absorbed")
        for _ in range(2):
            got = pred(ims)
            for g, (o, r) in enumerate(zip(got, ref)):
                n = len(r["scores"])
                assert n >= 1 and d["counts"][g] == n == len(o["scores"])
                assert sorted(o) == ["boxes", "labels", "merged", "scores"]
                for key in ("boxes", "scores", "labels", "merged"):
                    assert torch.equal(o[key], d[key][g, :n]), (g, key)
                assert o["boxes"].cpu().numpy().tobytes() == r["boxes"].tobytes(), g
                assert o["scores"].cpu().numpy().tobytes() == r["scores"].tobytes(), g
                assert np.array_equal(o["merged"].cpu().numpy(), r["merged"]), g
        absorbed += sum(int(r["merged"].sum()) for r in ref)
        moved += sum(int((r["boxes"] != h["boxes"]).any(1).sum()) for r, h in zip(ref, head))
    assert absorbed >= 1 and moved >= 1


def test_predictor_value_errors_and_defaults():
    """(e)"""
    from yolomi.predict import Predictor
    model = _model()
    for kw in (dict(tta=True, rect=True), dict(tta=[(1, "")], rect=True), dict(slice_merge="mean"),
               dict(tta=True, slice_merge="wbf"), dict(tta=True, slice_metric="giou"), dict(tta=[]),
               dict(tta=[(2.0, "")]), dict(tta=[(1.0, "rl")]), dict(tta="1,0.5")):
        with pytest.raises(ValueError):
            Predictor(model, imgsz=S, ch=CH, **kw)
    p = Predictor(model, imgsz=S, ch=CH)
    assert p.views is None and (p.slice_merge, p.slice_metric) == ("nms", "iou")
    p = Predictor(model, imgsz=S, ch=CH, tta=True, slice_merge="nmm", slice_metric="ios")
    assert p.views == [(1.0, ""), (0.83, "lr"), (0.67, "")] and (p.slice_merge, p.slice_metric) == ("nmm", "ios")
    assert Predictor(model, imgsz=S, ch=CH, slice=TILE, slice_merge="mean").slice_merge == "mean"
    # the default Predictor: tta=None and tta=False are the plain path
    ims = _images()
    a = Predictor(model, batch=2, **_kw())(ims)
    b = Predictor(model, batch=2, tta=None, **_kw())(ims)
    c = Predictor(model, batch=2, tta=False, **_kw())(ims)
    for x, y, z in zip(a, b, c):
        assert len(x["scores"]) >= 1 and sorted(x) == ["boxes", "labels", "scores"]
        for key in x:
            assert torch.equal(x[key], y[key]) and torch.equal(x[key], z[key])


def test_predict_cli_tta(tmp_path):
    """(f)"""
    from yolomi.predict import Predictor
    ims = _images(seed=84)
    _write_pngs(tmp_path / "src", ims)
    model = _model()
    torch.save({"epoch": 0, "model_state_dict": model.state_dict()}, tmp_path / "w.pt")
    out = tmp_path / "out"
    cmd = [sys.executable, str(ROOT / "yolo-scratch_amd" / "predict.py"), "--weights", str(tmp_path / "w.pt"),
           "--source", str(tmp_path / "src"), "--scale", "n", "--ch", str(CH), "--nc", str(NC), "--imgsz", str(S),
           "--batch", "2", "--conf", str(CONF), "--iou", str(IOU), "--max-det", str(MAX_DET), "--tta-views",
           "1,0.83:lr", "--slice-merge", "mean", "--save-dir", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    doc = json.loads((out / "predictions.json").read_text())
    want = Predictor(model, batch=2, tta=[(1.0, ""), (0.83, "lr")], slice_merge="mean", **_kw())(ims)
    for i, (e, w) in enumerate(zip(doc["images"], want)):
        assert (e["height"], e["width"]) == HW[i] and len(e["scores"]) >= 1
        assert sorted(e) == ["boxes", "height", "image", "labels", "scores", "width"]      # the format is kept
        assert np.array_equal(np.asarray(e["scores"], np.float32), w["scores"].cpu().numpy()), i
        assert np.array_equal(np.asarray(e["boxes"], np.float32).reshape(-1, 4), w["boxes"].cpu().numpy()), i
        assert e["labels"] == w["labels"].tolist()
