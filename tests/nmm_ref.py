"""numpy restatement of greedy box merging over tiles (ym_decode_nmm_tiles) — TEST INFRASTRUCTURE ONLY
(helper of test_nmm_cpu.py and test_gpu_nmm.py; no test of its own).

Candidates are slice_ref.tile_candidates' (the conf filter, the first maximal class, the map to source pixels in
rounded fp32 steps, the edge filter, no rows of src < 0 tiles), in the order score descending, filtered index ascending.
The match value and the greedy loop are written from the contract, one rounded fp32 operation per line; the union is
the coordinate-wise min / max over the head and what it absorbed.  Also the plan and the rows the tests share: large
source objects that every window clamps at its sides, so that a tile's part and the whole-image pass's box of one
object overlap by less than an IoU threshold.
"""
from __future__ import annotations

import functools

import numpy as np

import slice_ref as SR

F32 = np.float32
THR = 0.5


# ---------------------------------------------------------------- the restatement
def match(a, b, metric):
    """Head box a (4,) against boxes b (n, 4), fp32 -> (n,) fp32."""
    a = np.asarray(a, F32)
    b = np.asarray(b, F32).reshape(-1, 4)
    x1 = np.maximum(a[0], b[:, 0])
    y1 = np.maximum(a[1], b[:, 1])
    x2 = np.minimum(a[2], b[:, 2])
    y2 = np.minimum(a[3], b[:, 3])
    iw = x2 - x1
    ih = y2 - y1
    iw = np.where(iw < F32(0), F32(0), iw)
    ih = np.where(ih < F32(0), F32(0), ih)
    inter = iw * ih
    aw = a[2] - a[0]
    ah = a[3] - a[1]
    a1 = aw * ah
    bw = b[:, 2] - b[:, 0]
    bh = b[:, 3] - b[:, 1]
    a2 = bw * bh
    if metric == "iou":
        den = a1 + a2
        den = den - inter
    elif metric == "ios":
        den = np.minimum(a1, a2)
    else:
        raise ValueError(metric)
    den = den + F32(1e-6)
    out = inter / den
    assert out.dtype == np.float32
    return out


def nmm(boxes, scores, labels, thr, metric="iou", merge=False, class_aware=False, max_det=0):
    """-> dict: keep (candidate indices of the heads, in kept order), boxes (n_keep, 4), merged (n_keep,), by (per
    candidate: the kept slot that absorbed it, -1 for heads and for candidates never reached under a cap)."""
    boxes = np.asarray(boxes, F32).reshape(-1, 4)
    scores = np.asarray(scores, F32)
    labels = np.asarray(labels)
    K = len(scores)
    order = np.lexsort((np.arange(K), -scores.astype(np.float64)))
    alive = np.ones(K, bool)
    by = np.full(K, -1, np.int64)
    keep = []
    thr = F32(thr)
    for s in order:
        if not alive[s]:
            continue
        if max_det > 0 and len(keep) >= max_det:
            break
        alive[s] = False
        keep.append(int(s))
        m = alive & (labels == labels[s]) if class_aware else alive      # the alive ones all come later in the order
        idx = np.nonzero(m)[0]
        hit = idx[~(match(boxes[s], boxes[idx], metric) <= thr)]
        alive[hit] = False
        by[hit] = len(keep) - 1
    keep = np.asarray(keep, np.int64)
    out = boxes[keep].copy().reshape(-1, 4)
    merged = np.zeros(len(keep), np.int32)
    for k in range(len(keep)):
        a = np.nonzero(by == k)[0]
        merged[k] = len(a)
        if merge and len(a):
            out[k, 0] = min(out[k, 0], boxes[a, 0].min())
            out[k, 1] = min(out[k, 1], boxes[a, 1].min())
            out[k, 2] = max(out[k, 2], boxes[a, 2].max())
            out[k, 3] = max(out[k, 3], boxes[a, 3].max())
    return dict(keep=keep, boxes=out, merged=merged, by=by)


def decode_tiles(pred, ents, begin, conf, thr, metric="iou", merge=False, class_aware=False, max_det=0, edge=0.0):
    """pred (T, N, 4+C) -> per image {boxes, scores, labels, index, rows, merged, by, cand_*}."""
    pred = np.asarray(pred, F32)
    N = pred.shape[1]
    outs = []
    for g in range(len(begin) - 1):
        bx, sc, lb, rw, tl = [np.zeros((0, 4), F32)], [np.zeros(0, F32)], [np.zeros(0, np.int64)], [], []
        for slot, t in enumerate(range(begin[g], begin[g + 1])):
            e = ents[t]
            if e.src < 0:
                continue
            b, s, l, r, _, _ = SR.tile_candidates(pred[t], e, conf, edge)
            bx.append(b), sc.append(s), lb.append(l), rw.append(r + slot * N), tl.append(np.full(len(s), slot))
        boxes, scores, labels = np.concatenate(bx), np.concatenate(sc), np.concatenate(lb)
        rows = np.concatenate(rw) if rw else np.zeros(0, np.int64)
        tiles = np.concatenate(tl) if tl else np.zeros(0, np.int64)
        r = nmm(boxes, scores, labels, thr, metric, merge, class_aware, max_det)
        k = r["keep"]
        outs.append(dict(boxes=r["boxes"], scores=scores[k], labels=labels[k], index=k, rows=rows[k],
                         merged=r["merged"], by=r["by"], cand_boxes=boxes, cand_scores=scores, cand_labels=labels,
                         cand_tiles=tiles))
    return outs


# ---------------------------------------------------------------- the inputs
S = 48                                                     # the frame
WINDOWS = [(0, 0), (24, 0), (0, 24), (24, 24)]             # (x0, y0) of image 0's 32 x 32 windows
# source (cx, cy, w, h) of image 0: the large ones are wider than the 8-px overlap, every window clamps them
OBJECTS = [(28.0, 28.0, 50.0, 50.0), (28.0, 14.0, 6.0, 9.0), (40.0, 28.0, 12.0, 5.0), (28.0, 30.0, 40.0, 6.0),
           (12.0, 28.0, 10.0, 6.0), (30.0, 8.0, 44.0, 5.0)]
SHAPES = {"small": (2, 17), "large": (2, 2100), "global": (1, 3400)}     # images, N
CONF = {"small": 0.5, "large": 0.001, "global": 0.001}


def plan(shape: str, hole: bool = False):
    """(entries, tile_begin, N): image 0 is 56 x 56 under its four windows plus the whole-image entry (`hole`: the
    second window has src = -1); image 1 (not in "global") is 20 x 30 in one window."""
    G, N = SHAPES[shape]
    ents = [SR.entry(0, x0, y0, 32, 32, 56, 56, S) for x0, y0 in WINDOWS] + [SR.entry(0, 0, 0, 56, 56, 56, 56, S)]
    if hole:
        ents[1].src = -1
    begin = [0, 5]
    if G == 2:
        ents.append(SR.entry(1, 0, 0, 30, 20, 20, 30, S))
        begin.append(6)
    return ents, begin, N


@functools.lru_cache(maxsize=None)
def pred(shape: str, C: int, hole: bool = False):
    """(T, N, 4+C) fp32, read-only, built as slice_ref.decode_pred builds its rows: per tile of image 0 the
    projections of OBJECTS first (a little jittered), one box at each window side, then random boxes; tie-free best
    scores, the objects' rows taking the largest ones and the object's own label in every tile."""
    ents, begin, N = plan(shape, hole)
    T = len(ents)
    rng = np.random.default_rng(900 + 10 * C + sorted(SHAPES).index(shape) + 5 * hole)
    p = np.zeros((T, N, 4 + C), np.float64)
    p[..., 0:2] = rng.uniform(-2.0, S + 2.0, (T, N, 2))
    p[..., 2:4] = rng.uniform(2.0, 0.45 * S, (T, N, 2))
    is_obj = np.zeros((T, N), bool)
    lab = rng.integers(0, C, (T, N))
    for t, e in enumerate(ents):
        k = 0
        if t < begin[1]:
            for cx, cy, w, h in OBJECTS:
                p[t, k, :4] = ((cx - e.x0) / e.sx + e.left + rng.uniform(-0.2, 0.2),
                               (cy - e.y0) / e.sy + e.top + rng.uniform(-0.2, 0.2), w / e.sx, h / e.sy)
                k += 1
            is_obj[t, :len(OBJECTS)] = True
            lab[t, :len(OBJECTS)] = np.arange(len(OBJECTS)) % C
        for cx, cy in ((e.left + 2.0, S / 2), (e.left + e.nw - 2.0, S / 2), (S / 2, e.top + 2.0),
                       (S / 2, e.top + e.nh - 2.0)):
            p[t, k, :4] = (cx, cy, 3.0, 3.0)
            k += 1
    cls = rng.uniform(0.0, 0.2, (T, N, C))
    values = 0.3 + 0.65 * (np.arange(T * N) + 0.5) / (T * N)
    n_obj = int(is_obj.sum())
    best = np.zeros((T, N))
    best[is_obj] = rng.permutation(values[T * N - n_obj:])
    best[~is_obj] = rng.permutation(values[:T * N - n_obj])
    np.put_along_axis(cls, lab[..., None], best[..., None], 2)
    p[..., 4:] = cls
    out = p.astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ref(shape, C, hole, metric, merge, class_aware, max_det, edge, thr=THR):
    ents, begin, _ = plan(shape, hole)
    return decode_tiles(pred(shape, C, hole), ents, begin, CONF[shape], thr, metric, merge, class_aware, max_det, edge)
