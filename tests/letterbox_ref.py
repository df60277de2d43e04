"""numpy restatement of the letterbox kernels (ym_letterbox_u8c, ym_unletterbox_boxes) — TEST INFRASTRUCTURE ONLY.

The image: per plane, the coefficient rule and blend of oracle/data.py's resize (what tests/augment_ref.py renders a
stretch entry with) taken to (nh, nw) instead of (S, S), placed at (left, top) over the fill.  The geometry comes in
as table entries; geometry() restates the host rule from its definition, independently of datasets/letterbox.py.
The boxes: fp32 numpy, one operation at a time.  Also the case list shared by the host-program test (CPU) and the
GPU test, and the files the stand-alone host program (tests/letterbox_host.cpp) reads.
"""
from __future__ import annotations

import ctypes
import math
import struct

import numpy as np

import augment_ref as AR

F32 = np.float32


# ---------------------------------------------------------------- geometry
def geometry(h0: int, w0: int, H: int, W: int, scaleup: bool = True):
    if h0 <= 0 or w0 <= 0:
        return 0, 0, 0, 0
    r = min(np.float64(H) / np.float64(h0), np.float64(W) / np.float64(w0))
    if not scaleup:
        r = min(r, np.float64(1.0))
    nw = min(W, max(1, int(math.floor(np.float64(w0) * r + 0.5))))
    nh = min(H, max(1, int(math.floor(np.float64(h0) * r + 0.5))))
    return nw, nh, (W - nw) // 2, (H - nh) // 2


def entries(ims, H: int, W: int, scaleup=True):
    """ctypes table of LbEntry for `ims` ((h0, w0) or (h0, w0, ch) arrays); `scaleup` one flag or one per image."""
    from yolomi._lib import LbEntry
    flags = [scaleup] * len(ims) if isinstance(scaleup, bool) else list(scaleup)
    t = (LbEntry * max(len(ims), 1))()
    for e, a, up in zip(t, ims, flags):
        h0, w0 = a.shape[:2]
        e.nw, e.nh, e.left, e.top = geometry(h0, w0, H, W, up)
        e.w0, e.h0 = w0, h0
        if e.nw > 0 and e.nh > 0:
            e.sx, e.sy = float(F32(w0) / F32(e.nw)), float(F32(h0) / F32(e.nh))
    return t


# ---------------------------------------------------------------- the image
def resize_plane(im: np.ndarray, nh: int, nw: int) -> np.ndarray:
    """uint8 (h0, w0) -> uint8 (nh, nw): oracle.data.resize_linear_u8 with its two coefficient calls taken apart."""
    from oracle.data import _coeffs
    h0, w0 = im.shape
    if (h0, w0) == (nh, nw):
        return im.copy()
    sx, sx1, a0, a1 = _coeffs(nw, w0)
    sy, sy1, b0, b1 = _coeffs(nh, h0)
    src = im.astype(np.int64)
    h = src[:, sx] * a0 + src[:, sx1] * a1
    top = (b0[:, None] * (h[sy] >> 4)) >> 16
    bot = (b1[:, None] * (h[sy1] >> 4)) >> 16
    return np.clip((top + bot + 2) >> 2, 0, 255).astype(np.uint8)


def render_entry(e, im: np.ndarray, H: int, W: int, fill: int) -> np.ndarray:
    """One table entry over its pixel-interleaved (h0, w0, ch) source -> uint8 (ch, H, W)."""
    h0, w0, ch = im.shape
    out = np.full((ch, H, W), fill & 255, np.uint8)
    if e.nw <= 0 or e.nh <= 0 or h0 <= 0 or w0 <= 0 or (e.h0, e.w0) != (h0, w0):
        return out
    y0, y1 = max(e.top, 0), min(e.top + e.nh, H)
    x0, x1 = max(e.left, 0), min(e.left + e.nw, W)
    for c in range(ch):
        r = resize_plane(np.ascontiguousarray(im[..., c]), e.nh, e.nw)
        out[c, y0:y1, x0:x1] = r[y0 - e.top:y1 - e.top, x0 - e.left:x1 - e.left]
    return out


def render(table, ims, H: int, W: int, fill: int = 114) -> np.ndarray:
    """-> uint8 (len(ims), ch, H, W)."""
    return np.stack([render_entry(table[i], a, H, W, fill) for i, a in enumerate(ims)])


def as_float(u8):
    return AR.as_float(u8)


# ---------------------------------------------------------------- the boxes
def unletterbox(boxes, count, table, H: int, W: int, out=None) -> np.ndarray:
    """boxes (B, N, 4) fp32 normalised xyxy -> source pixels for rows below count[b]; other rows keep `out`'s."""
    boxes = np.asarray(boxes, F32)
    B, N, _ = boxes.shape
    res = np.zeros_like(boxes) if out is None else np.array(out, F32, copy=True)
    for b in range(B):
        e = table[b]
        n = min(int(count[b]), N)
        for k, (size, off, sc, lim) in enumerate(((W, e.left, e.sx, e.w0), (H, e.top, e.sy, e.h0)) * 2):
            v = boxes[b, :n, k] * F32(size)                 # each line one fp32 operation, rounded to nearest
            v = v - F32(off)
            v = v * F32(sc)
            v = np.maximum(v, F32(0.0)) + F32(0.0)          # + 0: a zero comes out positive, as the device's max
            res[b, :n, k] = np.minimum(v, F32(lim))
    return res


# ---------------------------------------------------------------- cases
SOURCE_SIZES = [(1, 1), (7, 5), (5, 7), (33, 17), (17, 33), None, (32, 64), (16, 12), (16, 12), (0, 0)]
SCALEUP = [True, True, True, True, True, True, True, True, False, True]      # (16, 12) with and without


def sources(H: int, W: int, ch: int, seed: int = 0):
    """None: exactly (H, W), the copy; (0, 0): an empty image."""
    rng = np.random.default_rng(9000 + 100 * H + 10 * W + ch + seed)
    return [rng.integers(0, 256, (*(hw or (H, W)), ch), dtype=np.uint8) for hw in SOURCE_SIZES]


def box_cases():
    """(boxes (3, 5, 4), counts, sources' (h0, w0)) for a 32 x 32 frame: boxes in the pad (clamped to 0 and to w0 /
    h0), a tiny x, ordinary ones; image 0 keeps none."""
    rng = np.random.default_rng(5)
    boxes = rng.uniform(0.0, 1.0, (3, 5, 4)).astype(F32)
    boxes[1, 0] = (1e-9, 0.0, 0.05, 1.0)                    # (7, 5) in 32 x 32: left = 4, so x = 0.05 * 32 < left
    boxes[1, 1] = (0.9, 0.5, 1.0, 0.999)                    # right pad: clamps to w0
    boxes[1, 2] = (0.5, 0.25, 0.5, 0.75)
    boxes[2, 0] = (0.0, 0.0, 1.0, 1.0)                      # (32, 64): top = 8, y clamps to 0 and h0
    boxes[2, 1] = (0.3, 0.1, 0.6, 0.2)                      # wholly in the top pad
    return boxes, np.array([0, 5, 2], np.int32), [(5, 7), (7, 5), (32, 64)]


# ---------------------------------------------------------------- the host program's files
def write_case_file(path, table, ims, H: int, W: int, fill: int):
    """int64 header {B, H, W, ch, fill, n_bytes}, meta, source bytes, table bytes (native endianness)."""
    buf, meta = AR.pack(ims)
    with open(path, "wb") as f:
        f.write(struct.pack("=6q", len(ims), H, W, ims[0].shape[2], fill, buf.size))
        f.write(meta.tobytes())
        f.write(buf.tobytes())
        f.write(bytes(table)[: len(ims) * ctypes.sizeof(type(table[0]))])


def run_host(exe, tmp_path, table, ims, H: int, W: int, fill: int = 114, timeout=120) -> np.ndarray:
    """tests/letterbox_host.cpp over `table` -> uint8 (len(ims), ch, H, W)."""
    import subprocess
    write_case_file(tmp_path / "lb_cases.bin", table, ims, H, W, fill)
    subprocess.run([str(exe), str(tmp_path / "lb_cases.bin"), str(tmp_path / "lb_out.bin")], check=True,
                   timeout=timeout)
    return np.fromfile(tmp_path / "lb_out.bin", dtype=np.uint8).reshape(len(ims), ims[0].shape[2], H, W)
