"""numpy restatement of test-time augmentation (datasets/tta.py, the mirror bits of ym_tile_entry, ym_decode_nmw_tiles;
DESIGN §27) — TEST INFRASTRUCTURE ONLY (helper of test_tta_cpu.py and test_gpu_tta.py; no test of its own).

The plan: views() / view_entries() restate the view rule from its definition on slice_ref's windows and
letterbox_ref's geometry, independently of datasets/tta.py.
The image: a mirrored tile is slice_ref.render_tile of the entry with the columns (rows) of its nw x nh rectangle
reversed in numpy.
The boxes: slice_ref.tile_candidates' steps with the mirror put between the clamp and the edge test, one rounded fp32
operation per line; then nms_cls_ref.nms_cls, nmm_ref.nmm, or nmw() below: nmm_ref.nmm's greedy loop, the
score-weighted mean formed in Python integers.  bound() is the derived error bound of that mean.
Also the decode case with mirrored entries that the CPU test holds to its input conditions and the GPU test runs.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import letterbox_ref as LR
import nmm_ref as MR
import nms_cls_ref as NR
import slice_ref as SR

F32 = np.float32
MIRROR_X, MIRROR_Y = 16, 32
FLIP_BITS = {"": 0, "lr": 16, "ud": 32, "lrud": 48}
QS, CS, CMAX = 12, 5, 2.0 ** 20
MAX_R = 1 << 26


# ---------------------------------------------------------------- the plan
def views(spec: str):
    out = []
    for item in spec.split(","):
        parts = item.strip().split(":")
        if len(parts) > 2 or (len(parts) == 2 and parts[1] not in ("lr", "ud", "lrud")):
            raise ValueError(item)
        s = float(parts[0])
        if not 0.0 < s <= 1.0:
            raise ValueError(item)
        out.append((s, parts[1] if len(parts) == 2 else ""))
    return out


def view_entry(src, x0, y0, tw, th, h0, w0, S, scale, flip):
    e = SR.entry(src, x0, y0, tw, th, h0, w0, S)
    nw1, nh1 = LR.geometry(th, tw, S, S)[:2]
    e.nw = min(nw1, max(1, int(np.floor(np.float64(nw1) * np.float64(scale) + np.float64(0.5)))))
    e.nh = min(nh1, max(1, int(np.floor(np.float64(nh1) * np.float64(scale) + np.float64(0.5)))))
    e.left, e.top = (S - e.nw) // 2, (S - e.nh) // 2
    e.sx, e.sy = float(F32(tw) / F32(e.nw)), float(F32(th) / F32(e.nh))
    e.edges |= FLIP_BITS[flip]
    return e


def view_entries(hws, vws, S, tile=0, overlap=0.2, full=True):
    """(list of TileEntry, tile_begin): per image, per view, per window."""
    out, begin = [], [0]
    for g, (h0, w0) in enumerate(hws):
        if tile:
            wins = SR.windows(h0, w0, tile, overlap)
            if full and wins:
                wins = wins + [(0, 0, w0, h0)]
        else:
            wins = [(0, 0, w0, h0)] if h0 > 0 and w0 > 0 else []
        for s, f in vws:
            out += [view_entry(g, *win, h0, w0, S, s, f) for win in wins]
        begin.append(len(out))
    return out, begin


def with_bits(e, bits):
    """A copy of the entry with the mirror bits replaced by `bits`."""
    from yolomi._lib import TileEntry
    c = TileEntry.from_buffer_copy(bytes(e))
    c.edges = (e.edges & 15) | bits
    return c


# ---------------------------------------------------------------- the image
def render_tile(e, ims, H, W, fill):
    """uint8 (ch, H, W): slice_ref's tile, the rectangle's columns / rows reversed where the entry says so."""
    out = SR.render_tile(e, ims, H, W, fill).copy()
    if not SR.valid(e, ims):
        return out
    rect = out[:, e.top:e.top + e.nh, e.left:e.left + e.nw]
    if e.edges & MIRROR_X:
        rect = rect[:, :, ::-1]
    if e.edges & MIRROR_Y:
        rect = rect[:, ::-1, :]
    out[:, e.top:e.top + e.nh, e.left:e.left + e.nw] = rect.copy()
    return out


def render(ents, ims, H, W, fill=114):
    return np.stack([render_tile(e, ims, H, W, fill) for e in ents])


# ---------------------------------------------------------------- the boxes
def clamp_axis(v, off, sc, lim):
    u = v - F32(off)
    u = u * F32(sc)
    u = np.maximum(u, F32(0.0))
    u = np.minimum(u, F32(lim))
    return u


def tile_candidates(p, e, conf, edge):
    """One tile (N, 4+C) -> source-pixel xyxy, score, label, row of the candidates, the number of coordinates the
    window clamped (before the mirror), and the rows the edge filter dropped."""
    p = np.asarray(p, F32)
    rows = np.nonzero(p[:, 4:].max(1) > F32(conf))[0]
    xyxy, mx, lab = NR.candidates(p, conf)
    u1 = clamp_axis(xyxy[:, 0], e.left, e.sx, e.tw)
    v1 = clamp_axis(xyxy[:, 1], e.top, e.sy, e.th)
    u2 = clamp_axis(xyxy[:, 2], e.left, e.sx, e.tw)
    v2 = clamp_axis(xyxy[:, 3], e.top, e.sy, e.th)
    clamped = int((u1 == 0).sum() + (v1 == 0).sum() + (u2 == F32(e.tw)).sum() + (v2 == F32(e.th)).sum())
    if e.edges & MIRROR_X:
        a = F32(e.tw) - u2
        b = F32(e.tw) - u1
        u1, u2 = a, b
    if e.edges & MIRROR_Y:
        a = F32(e.th) - v2
        b = F32(e.th) - v1
        v1, v2 = a, b
    cut = np.zeros(len(mx), bool)
    if edge > 0:
        ed = F32(edge)
        if e.edges & 1:
            cut |= u1 < ed
        if e.edges & 2:
            cut |= u2 > F32(e.tw) - ed
        if e.edges & 4:
            cut |= v1 < ed
        if e.edges & 8:
            cut |= v2 > F32(e.th) - ed
    X1 = u1 + F32(e.x0)
    Y1 = v1 + F32(e.y0)
    X2 = u2 + F32(e.x0)
    Y2 = v2 + F32(e.y0)
    boxes = np.stack([X1, Y1, X2, Y2], 1).astype(F32).reshape(-1, 4)
    m = ~cut
    return boxes[m], mx[m], lab[m], rows[m], clamped, rows[cut]


def q_of(score) -> int:
    s = F32(min(max(F32(score), F32(0.0)), F32(1.0))) * F32(2 ** QS)
    return max(1, int(np.rint(s)))                         # half to even, as llrint


def c_of(v) -> int:
    s = F32(min(max(F32(v), F32(-CMAX)), F32(CMAX))) * F32(2 ** CS)
    return int(np.rint(s))


def nmw(boxes, scores, labels, thr, metric="iou", class_aware=False, max_det=0):
    """nmm_ref.nmm's greedy loop; a head that absorbed candidates gets the fixed-point weighted mean, sums in Python
    integers.  -> nmm's dict, plus `exact` (n_keep, 4) fp64: the fp64 weighted mean of the fp32 inputs, and `spread`
    (n_keep, 4): max - min of the cluster's coordinate."""
    boxes = np.asarray(boxes, F32).reshape(-1, 4)
    scores = np.asarray(scores, F32)
    r = MR.nmm(boxes, scores, labels, thr, metric, False, class_aware, max_det)
    out = r["boxes"].copy()
    exact = out.astype(np.float64)
    spread = np.zeros_like(exact)
    for k, h in enumerate(r["keep"]):
        a = np.nonzero(r["by"] == k)[0]
        if not len(a):
            continue
        cl = np.concatenate([[h], a])
        qs = [q_of(scores[i]) for i in cl]
        sq = sum(qs)
        w = scores[cl].astype(np.float64)
        for j in range(4):
            sj = sum(q * c_of(boxes[i, j]) for q, i in zip(qs, cl))
            assert abs(sj) < 2 ** 63 and sq < 2 ** 63
            out[k, j] = F32(np.float64(float(sj)) / (np.float64(float(sq)) * np.float64(2 ** CS)))
            x = boxes[cl, j].astype(np.float64)
            exact[k, j] = (w * x).sum() / w.sum()
            spread[k, j] = x.max() - x.min()
    return dict(r, boxes=out, exact=exact, spread=spread)


def bound(conf, spread, mean, n, cmax):
    """The derived bound on |fixed-point mean - fp64 weighted mean| for scores in (conf, 1] and |coord| <= 2^20:
    the coordinates are rounded to 2^-CS (each off by <= 2^-(CS+1), and so is any weighted mean of them); a weight is
    q / 2^QS = w (1 + h) with |h| <= eta = 2^-(QS+1) / conf, so the normalised weights move by at most a factor
    (1 + eta) / (1 - eta) and the mean, a convex combination inside an interval of length `spread`, by at most
    spread * eta / (1 - eta); the result is rounded to fp32 once (2^-24 relative; the fp64 quotient before it 2^-53);
    and the fp64 reference itself carries (n + 2) roundings of 2^-53 relative to the largest |coord| `cmax`."""
    eta = 2.0 ** -(QS + 1) / min(max(conf, 2.0 ** -(QS + 1)), 1.0)
    return (2.0 ** -(CS + 1) + spread * eta / (1.0 - eta) + (2.0 ** -24 + 2.0 ** -52) * (abs(mean) + 1.0) +
            (n + 2) * 2.0 ** -52 * cmax)


def decode_tiles(pred, ents, begin, conf, thr, how="nms", metric="iou", class_aware=False, max_det=0, edge=0.0):
    """pred (T, N, 4+C) -> per image {boxes, scores, labels, index, rows, cand_*, clamped, cut_rows [(slot, row)]} and,
    for how = "nmm" (union), "match" (greedy, the head's box) or "mean": merged, by (and exact, spread)."""
    pred = np.asarray(pred, F32)
    N = pred.shape[1]
    outs = []
    for g in range(len(begin) - 1):
        bx, sc, lb, rw, tl = [np.zeros((0, 4), F32)], [np.zeros(0, F32)], [np.zeros(0, np.int64)], [], []
        clamped, cut_rows = 0, []
        for slot, t in enumerate(range(begin[g], begin[g + 1])):
            e = ents[t]
            if e.src < 0:
                continue
            b, s, l, r, cl, cr = tile_candidates(pred[t], e, conf, edge)
            bx.append(b), sc.append(s), lb.append(l), rw.append(r + slot * N), tl.append(np.full(len(s), slot))
            clamped += cl
            cut_rows += [(slot, int(x)) for x in cr]
        boxes, scores, labels = np.concatenate(bx), np.concatenate(sc), np.concatenate(lb)
        rows = np.concatenate(rw) if rw else np.zeros(0, np.int64)
        tiles = np.concatenate(tl) if tl else np.zeros(0, np.int64)
        o = dict(cand_boxes=boxes, cand_scores=scores, cand_labels=labels, cand_tiles=tiles, cand_rows=rows,
                 clamped=clamped, cut_rows=cut_rows)
        if how == "nms":
            keep = NR.nms_cls(boxes, scores, labels if class_aware else np.zeros_like(labels), thr, max_det)
            o.update(boxes=boxes[keep], index=np.asarray(keep, np.int64))
        else:
            r = (nmw(boxes, scores, labels, thr, metric, class_aware, max_det) if how == "mean" else
                 MR.nmm(boxes, scores, labels, thr, metric, how == "nmm", class_aware, max_det))
            o.update({k: v for k, v in r.items() if k != "keep"}, index=r["keep"])
        k = o["index"]
        o.update(scores=scores[k], labels=labels[k], rows=rows[k])
        outs.append(o)
    return outs


# ---------------------------------------------------------------- the mirrored decode case
S_DEC = 48
DEC_CONF, DEC_THR = 0.5, 0.45
# source (cx, cy, w, h) of image 0 (56 x 56), in the overlaps of its windows, and of image 1 (20 x 30)
OBJECTS0 = [(28.0, 14.0, 6.0, 9.0), (40.0, 28.0, 12.0, 5.0), (28.0, 40.0, 5.0, 11.0), (27.5, 27.5, 4.0, 4.0),
            (12.0, 28.0, 10.0, 6.0), (28.0, 10.0, 5.0, 5.0)]
OBJECTS1 = [(8.0, 6.0, 7.0, 5.0), (21.0, 12.0, 9.0, 8.0), (15.0, 10.0, 20.0, 12.0)]


def decode_plan():
    """(entries, tile_begin, N): (G, tiles, N) = (2, {4, 2}, 17).  Image 0 under four 32 x 32 windows: A plain,
    M mirrored in x (left and top interior), B mirrored in y (right and top interior), O in both; image 1 whole, plain,
    and whole at scale 0.67 mirrored in x."""
    ents = [view_entry(0, 24, 0, 32, 32, 56, 56, S_DEC, 1.0, ""),
            view_entry(0, 24, 24, 32, 32, 56, 56, S_DEC, 1.0, "lr"),
            view_entry(0, 0, 24, 32, 32, 56, 56, S_DEC, 1.0, "ud"),
            view_entry(0, 0, 0, 32, 32, 56, 56, S_DEC, 0.83, "lrud"),
            view_entry(1, 0, 0, 30, 20, 20, 30, S_DEC, 1.0, ""),
            view_entry(1, 0, 0, 30, 20, 20, 30, S_DEC, 0.67, "lr")]
    return ents, [0, 4, 6], 17


def project(e, cx, cy, w, h):
    """Source-space (cx, cy, w, h) -> the tile frame's xywh, through the window, the mirror and the scale."""
    u, v = cx - e.x0, cy - e.y0
    if e.edges & MIRROR_X:
        u = e.tw - u
    if e.edges & MIRROR_Y:
        v = e.th - v
    return u / e.sx + e.left, v / e.sy + e.top, w / e.sx, h / e.sy


@functools.lru_cache(maxsize=None)
def decode_pred(C: int):
    """(T, N, 4+C) fp32, read-only: per tile the projections of the image's objects (a little jittered), one 3-pixel
    box hugging each side of the rendered rectangle, then random boxes that may hang over the frame.  Tie-free best
    scores; the objects and the side boxes take the largest ones (all above DEC_CONF), the objects their own label."""
    ents, begin, N = decode_plan()
    T = len(ents)
    rng = np.random.default_rng(2700 + C)
    S = float(S_DEC)
    p = np.zeros((T, N, 4 + C), np.float64)
    p[..., 0:2] = rng.uniform(-2.0, S + 2.0, (T, N, 2))
    p[..., 2:4] = rng.uniform(2.0, 0.45 * S, (T, N, 2))
    top = np.zeros((T, N), bool)
    lab = rng.integers(0, C, (T, N))
    for t, e in enumerate(ents):
        objs = OBJECTS0 if e.src == 0 else OBJECTS1
        k = 0
        for o in objs:
            x, y, w, h = project(e, *o)
            p[t, k, :4] = (x + rng.uniform(-0.2, 0.2), y + rng.uniform(-0.2, 0.2), w, h)
            lab[t, k] = k % C
            k += 1
        for cx, cy in ((e.left + 2.0, S / 2), (e.left + e.nw - 2.0, S / 2), (S / 2, e.top + 2.0),
                       (S / 2, e.top + e.nh - 2.0)):
            p[t, k, :4] = (cx, cy, 3.0, 3.0)
            k += 1
        top[t, :k] = True
    cls = rng.uniform(0.0, 0.2, (T, N, C))
    values = 0.3 + 0.65 * (np.arange(T * N) + 0.5) / (T * N)
    n_top = int(top.sum())
    best = np.zeros((T, N))
    best[top] = rng.permutation(values[T * N - n_top:])
    best[~top] = rng.permutation(values[:T * N - n_top])
    np.put_along_axis(cls, lab[..., None], best[..., None], 2)
    p[..., 4:] = cls
    out = p.astype(F32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def decode_ref(C, how, metric, class_aware, max_det, edge):
    ents, begin, _ = decode_plan()
    return decode_tiles(decode_pred(C), ents, begin, DEC_CONF, DEC_THR, how, metric, class_aware, max_det, edge)


# ---------------------------------------------------------------- the mean on nmm_ref's shapes
# every best score of nmm_ref.pred is >= 0.3: at 0.25 the large shapes keep every row (K > 8192, K > 16384) as at
# nmm_ref.CONF's 0.001, and the bound, which grows with 1 / conf, stays far below the clusters' spread
MEAN_CONF = {"small": 0.5, "large": 0.25, "global": 0.25}


@functools.lru_cache(maxsize=None)
def mean_ref(shape, C, metric, class_aware, max_det, edge=0.0, thr=MR.THR, how="mean"):
    ents, begin, _ = MR.plan(shape)
    return decode_tiles(MR.pred(shape, C), ents, begin, MEAN_CONF[shape], thr, how, metric, class_aware, max_det, edge)
