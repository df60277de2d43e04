"""numpy restatement of the 1-4 plane augmentation (ym_augment_u8c, include/yolomi_augment.h) — TEST INFRASTRUCTURE ONLY.

Built on tests/augment_ref.py, unchanged: a pixel-interleaved (h0, w0, ch) source is rendered plane by plane through
augment_ref.render_entry with the gain taken out (the planes share their taps exactly when every plane equals its
own single-plane rendering), then hue / saturation on (r, g, b) in integers, then augment_ref's gain.  hue_sat is
written from the rule in the header's comment; hue_sat_model is the real-valued hexcone it approximates.  Also the
case list shared by the host-program test (CPU) and the GPU test, and the files the stand-alone host program
(tests/augment_colour_host.cpp) reads.
"""
from __future__ import annotations

import numpy as np

import augment_ref as AR

SOURCE_SIZES = [(1, 1), (7, 5), (33, 17), None]            # None: (S, S), the copy path
FILL = 114


# ---------------------------------------------------------------- hue and saturation
def hue_sat(rgb: np.ndarray, hue: int, sat: int) -> np.ndarray:
    """(..., 3) integer colours -> (..., 3) int64; hue Q16 fraction of a turn (& 65535), sat Q16 clamped to [0, 2^17]."""
    rgb = np.asarray(rgb).astype(np.int64)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    V, m = rgb.max(-1), rgb.min(-1)
    d = V - m
    grey = d == 0
    ds = np.where(grey, 1, d)                              # grey pixels are passed through at the end
    H6 = np.where(V == r, np.where(g >= b, g - b, 5 * ds + (r - b)),
                  np.where(V == g, np.where(b >= r, 2 * ds + (b - r), ds + (g - r)),
                           np.where(r >= g, 4 * ds + (r - g), 3 * ds + (b - g))))
    H6 = (H6 + (((int(hue) & 65535) * 6 * ds + 32768) >> 16)) % (6 * ds)
    s = min(max(int(sat), 0), 1 << 17)
    d1 = np.minimum((ds * s) >> 16, V)
    k = H6 // ds
    f = H6 - k * ds
    f1 = (2 * f * d1 + ds) // (2 * ds)
    m1 = V - d1
    up, dn = m1 + f1, V - f1
    sectors = [(V, up, m1), (dn, V, m1), (m1, V, up), (m1, dn, V), (up, m1, V), (V, m1, dn)]
    out = np.empty_like(rgb)
    for c in range(3):
        out[..., c] = np.where(grey, rgb[..., c], np.choose(k, [sec[c] for sec in sectors]))
    return out


def hue_sat_model(rgb: np.ndarray, hue: float, sat: float) -> np.ndarray:
    """The real-valued hexcone in float64: hue in turns (a shift), sat a factor on the chroma, limited by V."""
    rgb = np.asarray(rgb, np.float64)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    V, m = rgb.max(-1), rgb.min(-1)
    d = V - m
    grey = d == 0
    ds = np.where(grey, 1.0, d)
    h = np.where(V == r, ((g - b) / ds) % 6.0, np.where(V == g, 2.0 + (b - r) / ds, 4.0 + (r - g) / ds))
    h = (h + 6.0 * hue) % 6.0
    d1 = np.minimum(d * sat, V)
    k = np.minimum(np.floor(h), 5.0)
    f1 = (h - k) * d1
    m1 = V - d1
    up, dn = m1 + f1, V - f1
    sectors = [(V, up, m1), (dn, V, m1), (m1, V, up), (m1, dn, V), (up, m1, V), (V, m1, dn)]
    out = np.empty_like(rgb)
    for c in range(3):
        out[..., c] = np.where(grey, rgb[..., c], np.choose(k.astype(np.int64), [sec[c] for sec in sectors]))
    return out


# ---------------------------------------------------------------- rendering
def _without_gain(e):
    u = type(e).from_buffer_copy(bytes(e))
    u.gain = 65536                                         # (v * 65536) >> 16 == v
    return u


def render_entry_c(e, ims, S: int, colour=None) -> np.ndarray:
    """`ims`: uint8 (h0, w0, ch) arrays in batch order; `colour`: (hue, sat) Q16 or None -> uint8 (ch, S, S)."""
    ch = ims[0].shape[2]
    u = _without_gain(e)
    planes = np.stack([AR.render_entry(u, [np.ascontiguousarray(a[..., c]) for a in ims], S) for c in range(ch)])
    if colour is not None:
        assert ch == 3
        planes = np.moveaxis(hue_sat(np.moveaxis(planes, 0, -1), *colour), -1, 0)
    return AR._gain(planes, e)


def render_c(table, ims, S: int, colours=None) -> np.ndarray:
    """-> uint8 (len(table), ch, S, S)."""
    return np.stack([render_entry_c(table[i], ims, S, None if colours is None else colours[i])
                     for i in range(len(table))])


# ---------------------------------------------------------------- cases
def sources(S: int, ch: int, seed: int = 0):
    rng = np.random.default_rng(7000 + 10 * S + ch + seed)
    return [rng.integers(0, 256, (*(hw or (S, S)), ch), dtype=np.uint8) for hw in SOURCE_SIZES]


def cases(S: int):
    """[(name, AugEntry)] over sources(S, ch): the table does not depend on the plane count."""
    from datasets import augment as A
    sizes = [hw or (S, S) for hw in SOURCE_SIZES]
    B = len(sizes)

    def plain(b, inv=None, **kw):
        return A.plain_entry(b, *sizes[b], S, inv, **kw)

    def inv_of(canvas, flip=(False, False), **kw):
        return np.linalg.inv(A.affine_matrix(S, canvas, **kw)) @ A.flip_matrix(S, *flip)

    def mosaic(srcs, xc, yc, flip=(False, False), **kw):
        return A.mosaic_entry(srcs, [sizes[b] for b in srcs], xc, yc, S, inv_of(2 * S, flip, **kw), gain=1.2)

    out = [(f"stretch{b}", plain(b, gain=(1.0, 1.3, 0.6, 1.0)[b])) for b in range(B)]      # 3: S x S, the copy path
    out += [("rot_fliplr", plain(2, inv_of(S, (True, False), angle=25.0, scale=0.8), gain=0.9)),
            ("rot_flipud_tiny", plain(1, inv_of(S, (False, True), angle=-40.0, scale=1.3))),
            ("one_pixel_shear", plain(0, inv_of(S, shear_x=8.0))),
            # the whole 2S canvas in view: every row, so every wave of 256 pixels, crosses the centre
            ("mosaic_split", mosaic([3, 2, 1, 0], S + 3, S - 5, scale=0.5)),
            ("mosaic_rot", mosaic([2, 3, 3, 1], S - 6, S + 4, (True, False), angle=15.0, scale=0.7, tx=0.45))]
    e = mosaic([3, 2, 1, 0], S + 1, S + 2, scale=0.5)
    e.tile[1].src = -1
    out.append(("mosaic_empty_slot", e))
    e = mosaic([3, 0, 1, 2], S - 2, S + 1, scale=0.5)
    e.tile[1].src, e.tile[3].src = B, 2 ** 31 - 1
    out.append(("mosaic_src_out_of_range", e))
    e = plain(2)
    e.tile[0].src = B
    out.append(("stretch_src_out_of_range", e))
    return out


def table_of(entries):
    from yolomi._lib import AugEntry
    t = (AugEntry * len(entries))()
    for i, e in enumerate(entries):
        t[i] = e
    return t


def colours_of(n: int, seed: int = 0):
    """n (hue, sat) Q16 pairs: the identity, the extremes and random ones (hue outside [0, 65536) and sat outside
    [0, 2^17] included: the rule masks and clamps them)."""
    fixed = [(0, 65536), (65535, 1 << 17), (21845, 0), (-3000, 40000), (70000, 200000), (32768, -5)]
    rng = np.random.default_rng(seed)
    rand = [(int(rng.integers(0, 65536)), int(rng.integers(0, (1 << 17) + 1))) for _ in range(max(n - len(fixed), 0))]
    return (fixed + rand)[:n]


def colour_table(pairs):
    from yolomi._lib import AugColour
    t = (AugColour * len(pairs))()
    for i, (h, s) in enumerate(pairs):
        t[i].hue, t[i].sat = h, s
    return t


# ---------------------------------------------------------------- the host program's files
def run_host(exe, tmp_path, table, ims, S: int, colours=None, timeout=120) -> np.ndarray:
    """tests/augment_colour_host.cpp over `table` -> uint8 (len(table), ch, S, S)."""
    import subprocess
    ch, n = ims[0].shape[2], len(table)
    AR.write_case_file(tmp_path / "cases.bin", table, n, ims, S)      # pack() counts h0 * w0 * ch bytes per image
    cmd = [str(exe), "render", str(tmp_path / "cases.bin"), str(tmp_path / "out.bin"), str(ch)]
    if colours is not None:
        (tmp_path / "colour.bin").write_bytes(bytes(colour_table(colours)))
        cmd.append(str(tmp_path / "colour.bin"))
    subprocess.run(cmd, check=True, timeout=timeout)
    return np.fromfile(tmp_path / "out.bin", dtype=np.uint8).reshape(n, ch, S, S)
