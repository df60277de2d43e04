"""Sliced inference: the plan of overlapping full-resolution windows ("tiles") of large images.

Everything here is host arithmetic in integers; the one rounding, of the overlap, is made once in fp64.  The plan
travels to the device as a table of ym_tile_entry (include/yolomi.h), one entry per tile: the kernels derive nothing.

  slice_windows   the windows of one image
  tile_table      the table of a group of images: per window its letterbox geometry in the S x S frame, the fp32
                  factors back to window pixels and the window sides that are not image sides
  tile_bytes      the table as bytes for the device, padded with src = -1 entries (all-fill tiles, no candidates)
  slice_batch     ym_slice_letterbox_u8c: the tiles of sources that are already on the device
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from yolomi._lib import TileEntry

from .letterbox import letterbox_geometry

EDGE_LEFT, EDGE_RIGHT, EDGE_TOP, EDGE_BOTTOM = 1, 2, 4, 8


def slice_step(tile: int, overlap: float):
    """(ov, step): ov = floor(tile * overlap + 0.5) in fp64 pixels shared by neighbouring windows, step = tile - ov."""
    tile, overlap = int(tile), float(overlap)
    if tile < 1:
        raise ValueError(f"slice_windows: tile {tile} < 1")
    if not overlap >= 0.0:
        raise ValueError(f"slice_windows: overlap {overlap} < 0")
    ov = math.floor(tile * overlap + 0.5)
    if ov >= tile:
        raise ValueError(f"slice_windows: an overlap of {ov} pixels leaves no step at tile {tile}")
    return ov, tile - ov


def _starts(L: int, tile: int, step: int):
    """[(start, length)] of the windows along an axis of L pixels."""
    if L <= tile:
        return [(0, L)]
    n = -(-(L - tile) // step) + 1
    return [(min(i * step, L - tile), tile) for i in range(n)]         # the last one shifted back inside


def slice_windows(h0: int, w0: int, tile: int, overlap: float):
    """[(x0, y0, tw, th)] of an h0 x w0 image, row-major (y outer).  Per axis of length L: one window [0, L) when
    L <= tile, otherwise ceil((L - tile) / step) + 1 windows of `tile` pixels starting at min(i * step, L - tile).
    An image without pixels has no window."""
    _, step = slice_step(tile, overlap)
    h0, w0, tile = int(h0), int(w0), int(tile)
    if h0 <= 0 or w0 <= 0:
        return []
    return [(x0, y0, tw, th) for y0, th in _starts(h0, tile, step) for x0, tw in _starts(w0, tile, step)]


def _entry(e, src, x0, y0, tw, th, h0, w0, S):
    e.src, e.x0, e.y0, e.tw, e.th = src, x0, y0, tw, th
    e.nw, e.nh, e.left, e.top = letterbox_geometry(th, tw, S, S)
    e.edges = ((EDGE_LEFT if x0 > 0 else 0) | (EDGE_RIGHT if x0 + tw < w0 else 0) | (EDGE_TOP if y0 > 0 else 0) |
               (EDGE_BOTTOM if y0 + th < h0 else 0))
    e.sx = float(np.float32(tw) / np.float32(e.nw))
    e.sy = float(np.float32(th) / np.float32(e.nh))


def tile_table(hws, tile: int, overlap: float, S: int, full: bool = True):
    """(table, tile_begin) of the images `hws` = [(h0, w0)]: a ctypes array of ym_tile_entry, image g's entries
    contiguous in [tile_begin[g], tile_begin[g + 1]), `src` = g.  `full`: after its windows every image with pixels
    gets one more entry, the whole image (no interior side), the pass that sees objects larger than a tile."""
    plan = []
    begin = [0]
    for g, (h0, w0) in enumerate(hws):
        h0, w0 = int(h0), int(w0)
        wins = slice_windows(h0, w0, tile, overlap)
        if full and wins:
            wins = wins + [(0, 0, w0, h0)]
        plan += [(g, *win, h0, w0) for win in wins]
        begin.append(len(plan))
    table = (TileEntry * max(len(plan), 1))()
    for e, item in zip(table, plan):
        _entry(e, *item, int(S))
    if not plan:
        table[0].src = -1
    return table, begin


def tile_bytes(table, n: int, pad_to: int | None = None) -> torch.Tensor:
    """The first n entries of a ctypes array of TileEntry -> host uint8 tensor (a copy), followed by zeroed entries
    with src = -1 up to `pad_to` entries."""
    size = ctypes.sizeof(TileEntry)
    total = max(n, pad_to or 0)
    pad = (TileEntry * max(total - n, 1))()
    for e in pad:
        e.src = -1
    raw = bytes(table)[:n * size] + bytes(pad)[:(total - n) * size]
    return torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy())


def slice_batch(img_u8: torch.Tensor, meta: torch.Tensor, table: torch.Tensor, n_tiles: int, H: int, W: int,
                channels: int = 1, fill: int = 114, first: int = 0) -> torch.Tensor:
    """GPU: packed uint8 sources + device table of ym_tile_entry (uint8 bytes) -> the tiles [first, first + n_tiles)
    as (n_tiles, channels, H, W) fp32 (ym_slice_letterbox_u8c)."""
    from yolomi._lib import call, require_device, stream_ptr
    require_device(img_u8, meta, table)
    size = ctypes.sizeof(TileEntry)
    assert table.dtype == torch.uint8 and first >= 0 and table.numel() >= (first + n_tiles) * size
    out = torch.empty(n_tiles, channels, H, W, dtype=torch.float32, device=img_u8.device)
    call("ym_slice_letterbox_u8c", img_u8.data_ptr(), meta.contiguous().data_ptr(), int(meta.shape[0]),
         table.data_ptr() + first * size, n_tiles, channels, H, W, int(fill), out.data_ptr(),
         stream_ptr(img_u8.device))
    return out
