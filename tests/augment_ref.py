"""numpy restatement of ym_augment_u8's per-pixel arithmetic (include/yolomi_augment.h) — TEST INFRASTRUCTURE ONLY.

render(table, ims, S) evaluates a table of ym_aug_entry (the ctypes structs of yolomi/_lib.py) over the source images
`ims` (uint8 (h0, w0) arrays, in batch order) and returns uint8 (B, S, S); as_float turns that into what the kernel
writes.  Written from the documented formats, independently of the header: int64 positions with 24 fraction bits,
rounded half up to 11-bit weights, taps clamped to the source image, OpenCV's 8-bit resize interpolation, Q16 gain.
Stretch-flagged entries go through oracle/data.py's resize_linear_u8.  Also writes / reads the plain binary case file
the stand-alone host program (tests/augment_host.cpp) consumes.
"""
from __future__ import annotations

import ctypes
import struct

import numpy as np

FB = 24
SH = FB - 11


def _map(m, x, y):
    m = [np.int64(v) for v in m]
    with np.errstate(over="ignore"):
        return m[0] * x + m[1] * y + m[2]


def _coeff(pos, n):
    q = (pos >> SH) + ((pos >> (SH - 1)) & 1)
    s = q >> 11
    f = q & 2047
    lo, hi = s < 0, s >= n - 1
    f = np.where(lo | hi, 0, f)
    s = np.where(lo, 0, np.where(hi, n - 1, s))
    return s, np.minimum(s + 1, n - 1), 2048 - f, f


def _gain(v, e):
    g = min(max(int(e.gain), 0), 1 << 23)
    return np.minimum((v.astype(np.int64) * g) >> 16, 255).astype(np.uint8)


def render_entry(e, ims, S: int) -> np.ndarray:
    from oracle.data import resize_linear_u8
    B = len(ims)
    out = np.full((S, S), int(e.fill) & 255, np.int64)
    if e.flags & 1:
        b = e.tile[0].src
        if 0 <= b < B:
            im = ims[b]
            # resize_linear_u8 copies an S x S image; the coefficient rule gives the same bytes there
            out = resize_linear_u8(im, S).astype(np.int64)
        return _gain(out, e)
    y, x = np.meshgrid(np.arange(S, dtype=np.int64), np.arange(S, dtype=np.int64), indexing="ij")
    cx, cy = _map(e.c[0:3], x, y), _map(e.c[3:6], x, y)
    slot = (cx >= e.xc).astype(np.int64) + 2 * (cy >= e.yc).astype(np.int64)
    for k in range(4):
        t = e.tile[k]
        if not 0 <= t.src < B:
            continue
        im = ims[t.src].astype(np.int64)
        h0, w0 = im.shape
        own = (slot == k) & (cx >= t.x0) & (cx < t.x1) & (cy >= t.y0) & (cy < t.y1)
        if not own.any():
            continue
        sx, sx1, a0, a1 = _coeff(_map(t.m[0:3], x, y)[own], w0)
        sy, sy1, b0, b1 = _coeff(_map(t.m[3:6], x, y)[own], h0)
        top = im[sy, sx] * a0 + im[sy, sx1] * a1
        bot = im[sy1, sx] * a0 + im[sy1, sx1] * a1
        out[own] = np.clip((((b0 * (top >> 4)) >> 16) + ((b1 * (bot >> 4)) >> 16) + 2) >> 2, 0, 255)
    return _gain(out, e)


def render(table, ims, S: int) -> np.ndarray:
    return np.stack([render_entry(table[i], ims, S) for i in range(len(table))]) if len(table) else \
        np.zeros((0, S, S), np.uint8)


def as_float(u8: np.ndarray) -> np.ndarray:
    """What the kernel writes: float(v) / 255.0f."""
    return u8.astype(np.float32) / np.float32(255.0)


def pack(ims):
    """(bytes buffer, meta (B, 3) int64 {offset, h0, w0}) as datasets.crater.pack_images lays them out."""
    meta = np.zeros((len(ims), 3), np.int64)
    off = 0
    for i, a in enumerate(ims):
        meta[i] = (off, a.shape[0], a.shape[1])
        off += a.size
    buf = np.concatenate([a.reshape(-1) for a in ims]) if ims else np.zeros(0, np.uint8)
    return buf.astype(np.uint8), meta


def write_case_file(path, table, n_entries: int, ims, S: int):
    """int64 header {B, S, n_entries, n_bytes}, meta, source bytes, table bytes (native endianness)."""
    buf, meta = pack(ims)
    with open(path, "wb") as f:
        f.write(struct.pack("=4q", len(ims), S, n_entries, buf.size))
        f.write(meta.tobytes())
        f.write(buf.tobytes())
        f.write(bytes(table)[: n_entries * ctypes.sizeof(type(table[0]))])
