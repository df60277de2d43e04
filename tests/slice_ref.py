"""numpy restatement of sliced inference (datasets/slicing.py, ym_slice_letterbox_u8c, ym_decode_nms_tiles) — TEST
INFRASTRUCTURE ONLY.

The plan: windows() restates the window rule from its definition (a range plus the shifted-back last window),
independently of datasets/slicing.py; entries() builds the table with tests/letterbox_ref.py's geometry.
The image: a tile is letterbox_ref.render_entry applied to the numpy crop of its window, with the entry {nw, nh, left,
top, w0 = tw, h0 = th}; a tile that is not valid is all fill.
The boxes: nms_cls_ref.candidates per tile, the map to source pixels in numpy fp32 (one operation per line, each
rounded), the tile-border filter, then nms_cls_ref.nms_cls on the image's concatenation (one label for the
class-agnostic form).  Also the case lists shared by the host-program test (CPU) and the GPU tests, and the files the
stand-alone host program (tests/slice_host.cpp) reads.
"""
from __future__ import annotations

import ctypes
import functools
import struct
from types import SimpleNamespace

import numpy as np

import augment_ref as AR
import letterbox_ref as LR
import nms_cls_ref as NR

F32 = np.float32


# ---------------------------------------------------------------- the plan
def overlap_px(tile: int, overlap: float) -> int:
    return int(np.floor(np.float64(tile) * np.float64(overlap) + np.float64(0.5)))


def axis(L: int, tile: int, step: int):
    if L <= tile:
        return [(0, L)]
    return [(s, tile) for s in list(range(0, L - tile, step)) + [L - tile]]


def windows(h0: int, w0: int, tile: int, overlap: float):
    step = tile - overlap_px(tile, overlap)
    if h0 <= 0 or w0 <= 0:
        return []
    return [(x0, y0, tw, th) for y0, th in axis(h0, tile, step) for x0, tw in axis(w0, tile, step)]


def entry(src, x0, y0, tw, th, h0, w0, S, frame_w=None):
    """One TileEntry; the frame is S rows by (frame_w or S) columns."""
    from yolomi._lib import TileEntry
    e = TileEntry()
    e.src, e.x0, e.y0, e.tw, e.th = src, x0, y0, tw, th
    e.nw, e.nh, e.left, e.top = LR.geometry(th, tw, S, frame_w or S)
    e.edges = (x0 > 0) * 1 + (x0 + tw < w0) * 2 + (y0 > 0) * 4 + (y0 + th < h0) * 8
    if e.nw > 0 and e.nh > 0:
        e.sx, e.sy = float(F32(tw) / F32(e.nw)), float(F32(th) / F32(e.nh))
    return e


def entries(hws, tile, overlap, H, W=None, full=True):
    """(list of TileEntry, tile_begin) of the images `hws` in an H x (W or H) frame."""
    out, begin = [], [0]
    for g, (h0, w0) in enumerate(hws):
        wins = windows(h0, w0, tile, overlap)
        if full and wins:
            wins = wins + [(0, 0, w0, h0)]
        out += [entry(g, *win, h0, w0, H, W) for win in wins]
        begin.append(len(out))
    return out, begin


def as_table(ents):
    from yolomi._lib import TileEntry
    t = (TileEntry * max(len(ents), 1))()
    for k, e in enumerate(ents):
        ctypes.memmove(ctypes.byref(t, k * ctypes.sizeof(TileEntry)), ctypes.byref(e), ctypes.sizeof(TileEntry))
    return t


def table_bytes(ents) -> np.ndarray:
    return np.frombuffer(bytes(as_table(ents)), dtype=np.uint8)[:len(ents) * 48].copy()


# ---------------------------------------------------------------- the image
def valid(e, ims) -> bool:
    if not 0 <= e.src < len(ims) or min(e.tw, e.th, e.nw, e.nh) <= 0:
        return False
    h0, w0 = ims[e.src].shape[:2]
    return e.x0 >= 0 and e.y0 >= 0 and e.x0 + e.tw <= w0 and e.y0 + e.th <= h0


def render_tile(e, ims, H, W, fill):
    """uint8 (ch, H, W): the letterbox of the window's pixels taken as an image of their own."""
    ch = ims[0].shape[2]
    if not valid(e, ims):
        return np.full((ch, H, W), fill & 255, np.uint8)
    crop = np.ascontiguousarray(ims[e.src][e.y0:e.y0 + e.th, e.x0:e.x0 + e.tw])
    lb = SimpleNamespace(nw=e.nw, nh=e.nh, left=e.left, top=e.top, w0=e.tw, h0=e.th)
    return LR.render_entry(lb, crop, H, W, fill)


def render(ents, ims, H, W, fill=114) -> np.ndarray:
    """-> uint8 (len(ents), ch, H, W)."""
    return np.stack([render_tile(e, ims, H, W, fill) for e in ents])


SOURCES = [(50, 70), (33, 33)]
TILE, OVERLAP = 32, 0.25
FRAMES = [(32, 32), (32, 48)]                              # (H, W): 32 x 32 windows are copies in both


def sources(ch: int, seed: int = 0):
    rng = np.random.default_rng(7100 + ch + seed)
    return [rng.integers(0, 256, (*hw, ch), dtype=np.uint8) for hw in SOURCES]


def render_cases(H: int, W: int):
    """(entries, names): the plan of SOURCES with the whole-image pass (the resize tiles; the last windows touch the
    images' last row and column), then hand-made entries: interior windows that are resized (their taps must clamp at
    the window, not at the image), a small window in the image's last corner, windows that leave the image on each
    side, windows without pixels, and src outside the images."""
    ents, begin = entries(SOURCES, TILE, OVERLAP, H, W)
    names = [f"plan{k}" for k in range(len(ents))]
    (h0, w0), (h1, w1) = SOURCES
    extra = [("interior-up", entry(0, 3, 5, 20, 13, h0, w0, H, W)),
             ("interior-down", entry(0, 1, 2, 61, 45, h0, w0, H, W)),
             ("corner", entry(0, w0 - 17, h0 - 9, 17, 9, h0, w0, H, W)),
             ("one-pixel", entry(1, 32, 32, 1, 1, h1, w1, H, W)),
             ("leaves-right", entry(0, w0 - 31, 0, 32, 32, h0, w0, H, W)),
             ("leaves-bottom", entry(1, 0, 2, 32, 32, h1, w1, H, W)),
             ("negative-x0", entry(0, -1, 0, 32, 32, h0, w0, H, W)),
             ("negative-y0", entry(0, 0, -3, 32, 32, h0, w0, H, W)),
             ("no-src", entry(-1, 0, 0, 32, 32, h0, w0, H, W)),
             ("src-past", entry(2, 0, 0, 32, 32, h0, w0, H, W))]
    for bad in ("tw", "nh"):
        e = entry(1, 0, 0, 32, 32, h1, w1, H, W)
        setattr(e, bad, 0)
        extra.append((f"zero-{bad}", e))
    return ents + [e for _, e in extra], names + [n for n, _ in extra], begin


# ---------------------------------------------------------------- the boxes
def map_axis(v, off, sc, lim, org):
    """Frame coordinate -> (window coordinate u, source coordinate), fp32, one rounded operation per line."""
    u = v - F32(off)
    u = u * F32(sc)
    u = np.maximum(u, F32(0.0))
    u = np.minimum(u, F32(lim))
    return u, u + F32(org)


def tile_candidates(p, e, conf, edge):
    """One tile (N, 4+C) -> source-pixel xyxy, score, label, row, and per kept-or-cut candidate the bits that cut it
    (the last one for every candidate of the conf filter, before the border filter)."""
    p = np.asarray(p, np.float32)
    rows = np.nonzero(p[:, 4:].max(1) > F32(conf))[0]
    xyxy, mx, lab = NR.candidates(p, conf)
    assert len(rows) == len(mx)
    u1, X1 = map_axis(xyxy[:, 0], e.left, e.sx, e.tw, e.x0)
    v1, Y1 = map_axis(xyxy[:, 1], e.top, e.sy, e.th, e.y0)
    u2, X2 = map_axis(xyxy[:, 2], e.left, e.sx, e.tw, e.x0)
    v2, Y2 = map_axis(xyxy[:, 3], e.top, e.sy, e.th, e.y0)
    cut = np.zeros(len(mx), np.int64)
    if edge > 0:
        ed = F32(edge)
        cut |= np.where(u1 < ed, 1, 0) * bool(e.edges & 1)
        cut |= np.where(u2 > F32(e.tw) - ed, 2, 0) * bool(e.edges & 2)
        cut |= np.where(v1 < ed, 4, 0) * bool(e.edges & 4)
        cut |= np.where(v2 > F32(e.th) - ed, 8, 0) * bool(e.edges & 8)
    clamped = int(((u1 == 0) | (v1 == 0) | (u2 == F32(e.tw)) | (v2 == F32(e.th))).sum())
    m = cut == 0
    boxes = np.stack([X1, Y1, X2, Y2], 1).astype(np.float32).reshape(-1, 4)
    return boxes[m], mx[m], lab[m], rows[m], cut, clamped


def decode_tiles(pred, ents, begin, conf, iou_thr, class_aware=False, max_det=0, edge=0.0):
    """pred (T, N, 4+C) -> per image {boxes, scores, labels, index, rows, tile (of every candidate), cut (the bits
    that dropped candidates, OR-ed per bit into counts), clamped}."""
    pred = np.asarray(pred, np.float32)
    N = pred.shape[1]
    outs = []
    for g in range(len(begin) - 1):
        bx, sc, lb, rw, tl = [np.zeros((0, 4), F32)], [np.zeros(0, F32)], [np.zeros(0, np.int64)], [], []
        cuts, clamped = np.zeros(4, np.int64), 0
        for slot, t in enumerate(range(begin[g], begin[g + 1])):
            e = ents[t]
            if e.src < 0:
                continue
            b, s, l, r, cut, cl = tile_candidates(pred[t], e, conf, edge)
            bx.append(b), sc.append(s), lb.append(l), rw.append(r + slot * N), tl.append(np.full(len(s), slot))
            cuts += [int(((cut >> k) & 1).sum()) for k in range(4)]
            clamped += cl
        boxes, scores, labels = np.concatenate(bx), np.concatenate(sc), np.concatenate(lb)
        rows = np.concatenate(rw) if rw else np.zeros(0, np.int64)
        tiles = np.concatenate(tl) if tl else np.zeros(0, np.int64)
        keep = NR.nms_cls(boxes, scores, labels if class_aware else np.zeros_like(labels), iou_thr, max_det)
        outs.append(dict(boxes=boxes[keep], scores=scores[keep], labels=labels[keep], index=keep, rows=rows[keep],
                         cand_boxes=boxes, cand_scores=scores, cand_labels=labels, cand_tiles=tiles, cut=cuts,
                         clamped=clamped))
    return outs


def iou64(a, b):
    """IoU of box a with boxes b, fp64 (for conditions on test inputs only)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    iw = np.clip(np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]), 0, None)
    ih = np.clip(np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]), 0, None)
    inter = iw * ih
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) - inter + 1e-6)


def cross_tile_suppressions(out, iou_thr, class_aware, margin=0.02) -> int:
    """Candidates that were not kept and that a better-scoring kept box of ANOTHER tile overlaps by clearly more
    than the threshold (of its own label when class-aware): a box seen twice and merged."""
    kept = np.zeros(len(out["cand_scores"]), bool)
    kept[out["index"]] = True
    n = 0
    for c in np.nonzero(~kept)[0]:
        k = out["index"]
        m = (out["cand_scores"][k] > out["cand_scores"][c]) & (out["cand_tiles"][k] != out["cand_tiles"][c])
        if class_aware:
            m &= out["cand_labels"][k] == out["cand_labels"][c]
        if m.any() and (iou64(out["cand_boxes"][c], out["cand_boxes"][k[m]]) > iou_thr + margin).any():
            n += 1
    return n


# the decode cases: image 0 is 56 x 56 under 32 x 32 windows at step 24, image 1 is 20 x 30 in one window; frame 48
S_DEC = 48
_W = {"A": (24, 0), "M": (24, 24), "B": (0, 24), "O": (0, 0)}


def decode_plan(shape: str, hole: bool = False):
    """(entries, tile_begin, N).  "small": (G, tiles, N) = (2, {3, 1}, 17), the three windows of image 0 carry all
    four edge bits between them (with `hole` the middle one has src = -1 and the outer two still do); "large":
    (1, 4, 2100)."""
    if shape == "small":
        ents = [entry(0, *_W[k], 32, 32, 56, 56, S_DEC) for k in "AMB"]
        if hole:
            ents[1].src = -1
        ents.append(entry(1, 0, 0, 30, 20, 20, 30, S_DEC))
        return ents, [0, 3, 4], 17
    ents = [entry(0, *_W[k], 32, 32, 56, 56, S_DEC) for k in "OABM"]
    return ents, [0, 4], 2100


@functools.lru_cache(maxsize=None)
def decode_pred(shape: str, C: int, hole: bool = False):
    """(T, N, 4+C) fp32, read-only.  Per tile: the projections of a few source-space objects that lie in the windows'
    overlaps (seen by several tiles, a little jittered), boxes hugging each window side, and random boxes that may
    hang over the frame; every row's best class score is distinct from every other row's (tie-free)."""
    ents, begin, N = decode_plan(shape, hole)
    T = len(ents)
    rng = np.random.default_rng(500 + 10 * C + (shape == "large") + 2 * hole)
    S = float(S_DEC)
    p = np.zeros((T, N, 4 + C), np.float64)
    p[..., 0:2] = rng.uniform(-2.0, S + 2.0, (T, N, 2))
    p[..., 2:4] = rng.uniform(2.0, 0.45 * S, (T, N, 2))
    objects = [(28.0, 14.0, 6.0, 9.0), (40.0, 28.0, 12.0, 5.0), (28.0, 40.0, 5.0, 11.0), (27.5, 27.5, 4.0, 4.0),
               (12.0, 28.0, 10.0, 6.0), (28.0, 10.0, 5.0, 5.0)]                      # source (cx, cy, w, h), image 0
    for t, e in enumerate(ents):
        k = 0
        if e.tw == 32:
            for cx, cy, w, h in objects:
                p[t, k, :4] = ((cx - e.x0) / e.sx + e.left + rng.uniform(-0.2, 0.2),
                               (cy - e.y0) / e.sy + e.top + rng.uniform(-0.2, 0.2), w / e.sx, h / e.sy)
                k += 1
        for cx, cy in ((e.left + 2.0, S / 2), (e.left + e.nw - 2.0, S / 2), (S / 2, e.top + 2.0),
                       (S / 2, e.top + e.nh - 2.0)):                                  # one box at each window side
            p[t, k, :4] = (cx, cy, 3.0, 3.0)
            k += 1
    cls = rng.uniform(0.0, 0.2, (T, N, C))
    lab = rng.integers(0, C, (T, N))
    # distinct best scores; an object's rows take the largest ones and the object's own label in every tile
    is_obj = np.zeros((T, N), bool)
    for t, e in enumerate(ents):
        if e.tw == 32:
            is_obj[t, :len(objects)] = True
            lab[t, :len(objects)] = np.arange(len(objects)) % C
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
def decode_ref(shape, C, hole, conf, iou_thr, class_aware, max_det, edge):
    ents, begin, _ = decode_plan(shape, hole)
    return decode_tiles(decode_pred(shape, C, hole), ents, begin, conf, iou_thr, class_aware, max_det, edge)


# ---------------------------------------------------------------- the host program's files
def write_case_file(path, ents, ims, H: int, W: int, fill: int):
    """int64 header {n_images, n_tiles, H, W, ch, fill, n_bytes}, meta, source bytes, table bytes."""
    buf, meta = AR.pack(ims)
    with open(path, "wb") as f:
        f.write(struct.pack("=7q", len(ims), len(ents), H, W, ims[0].shape[2], fill, buf.size))
        f.write(meta.tobytes())
        f.write(buf.tobytes())
        f.write(table_bytes(ents).tobytes())


def run_host(exe, tmp_path, ents, ims, H: int, W: int, fill: int = 114, timeout=120) -> np.ndarray:
    """tests/slice_host.cpp over `ents` -> uint8 (len(ents), ch, H, W)."""
    import subprocess
    write_case_file(tmp_path / "sl_cases.bin", ents, ims, H, W, fill)
    subprocess.run([str(exe), str(tmp_path / "sl_cases.bin"), str(tmp_path / "sl_out.bin")], check=True,
                   timeout=timeout)
    return np.fromfile(tmp_path / "sl_out.bin", dtype=np.uint8).reshape(len(ents), ims[0].shape[2], H, W)
