"""Test-time augmentation: the plan of mirrored, scaled views of every window.

A view is (scale, flip): the window rendered into the S x S frame at `scale` of its letterbox size, mirrored left-right
("lr"), up-down ("ud") or both ("lrud").  Like the plan of sliced inference (datasets/slicing.py) everything is host
arithmetic; a view is one more ym_tile_entry over the same uploaded source, with the mirror bits in `edges`, so the
kernels of sliced inference render it and map its boxes back, and one merge per image joins the views.

  parse_views   "1,0.83:lr,0.67" -> [(1.0, ""), (0.83, "lr"), (0.67, "")]
  view_table    the table of a group of images, view-major per image
"""
from __future__ import annotations

import math

import numpy as np

from yolomi._lib import TileEntry

from .letterbox import letterbox_geometry
from .slicing import _entry, slice_windows

MIRROR_X, MIRROR_Y = 16, 32                       # YM_TILE_MIRROR_X, YM_TILE_MIRROR_Y
FLIPS = {"": 0, "lr": MIRROR_X, "ud": MIRROR_Y, "lrud": MIRROR_X | MIRROR_Y}
DEFAULT_VIEWS = ((1.0, ""), (0.83, "lr"), (0.67, ""))     # the scales and the flipped middle view of `augment=True`


def check_views(views):
    """[(scale, flip)] as floats and strings; ValueError unless 0 < scale <= 1, flip is a key of FLIPS and the list is
    not empty."""
    out = []
    for v in views:
        try:
            s, f = v
            s = float(s)
        except (TypeError, ValueError):
            raise ValueError(f"tta: a view is (scale, flip), got {v!r}") from None
        if not (0.0 < s <= 1.0) or f not in FLIPS:
            raise ValueError(f"tta: a view is (0 < scale <= 1, flip in {sorted(FLIPS)}), got {v!r}")
        out.append((s, f))
    if not out:
        raise ValueError("tta: no view")
    return out


def parse_views(spec: str):
    """ "1,0.83:lr,0.67" -> [(1.0, ""), (0.83, "lr"), (0.67, "")]: comma-separated `scale` or `scale:flip`."""
    if not isinstance(spec, str):
        raise ValueError(f"tta: a view list is a string like '1,0.83:lr,0.67', got {spec!r}")
    views = []
    for item in spec.split(","):
        scale, sep, flip = item.strip().partition(":")
        if sep and not flip:
            raise ValueError(f"tta: no flip after ':' in {item!r}")
        try:
            s = float(scale)
        except ValueError:
            raise ValueError(f"tta: {scale!r} is not a scale (in {spec!r})") from None
        views.append((s, flip.strip()))
    return check_views(views)


def view_table(hws, views, S: int, tile: int = 0, overlap: float = 0.2, full: bool = True):
    """(table, tile_begin) as datasets.slicing.tile_table gives them, image g's entries view-major: all windows of
    view 0, then all of view 1, ...  `tile` = 0: the one window of an image is the whole image; `tile` > 0: the
    windows are exactly what tile_table(hws, tile, overlap, S, full) lists.  An entry of view (s, flip) takes
    (nw1, nh1) = letterbox_geometry(th, tw, S, S) and renders the window at nw = min(nw1, max(1, floor(nw1 * s + 0.5)))
    by nh likewise (fp64), centred: left = (S - nw) // 2, top = (S - nh) // 2; sx = fp32(tw) / fp32(nw), sy likewise;
    the edge bits are tile_table's, plus the mirror bits of `flip`.  Every view runs in the same S x S frame (one
    plan, one graph replay); a reduced view pays for its grey border.  With views = [(1, "")] the table is byte-equal
    to tile_table's."""
    views = check_views(views)
    S, tile = int(S), int(tile)
    if tile < 0:
        raise ValueError(f"view_table: tile {tile} < 0")
    plan = []
    begin = [0]
    for g, (h0, w0) in enumerate(hws):
        h0, w0 = int(h0), int(w0)
        if tile:
            wins = slice_windows(h0, w0, tile, overlap)
            if full and wins:
                wins = wins + [(0, 0, w0, h0)]
        else:
            wins = [(0, 0, w0, h0)] if h0 > 0 and w0 > 0 else []
        plan += [(g, win, h0, w0, s, f) for s, f in views for win in wins]
        begin.append(len(plan))
    table = (TileEntry * max(len(plan), 1))()
    for e, (g, win, h0, w0, s, f) in zip(table, plan):
        _entry(e, g, *win, h0, w0, S)
        nw1, nh1 = e.nw, e.nh
        e.nw = min(nw1, max(1, math.floor(nw1 * s + 0.5)))
        e.nh = min(nh1, max(1, math.floor(nh1 * s + 0.5)))
        e.left, e.top = (S - e.nw) // 2, (S - e.nh) // 2
        e.sx = float(np.float32(e.tw) / np.float32(e.nw))
        e.sy = float(np.float32(e.th) / np.float32(e.nh))
        e.edges |= FLIPS[f]
    if not plan:
        table[0].src = -1
    return table, begin
