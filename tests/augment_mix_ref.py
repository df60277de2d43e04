"""numpy restatement of MixUp in the augmentation launch (ym_augment_mix_u8c, include/yolomi_augment.h) — TEST
INFRASTRUCTURE ONLY.

Built on tests/augment_ref.py and tests/augment_colour_ref.py, both unchanged: the primary and the partner entry are
each rendered plane by plane through augment_ref.render_entry with the gain taken out and no colour, the two are
blended in int64 as (a * r + p * (65536 - r)) >> 16 with r clamped to [0, 65536], then augment_colour_ref's hue / sat
and augment_ref's gain with the PRIMARY entry's gain.  An image whose `partner` index lies outside the partner table
is augment_colour_ref.render_entry_c of its primary entry.  Also the case list shared by the host-program test (CPU)
and the GPU test, and the files the stand-alone host program (tests/augment_mix_host.cpp) reads.
"""
from __future__ import annotations

import ctypes
import struct

import numpy as np

import augment_colour_ref as CR
import augment_ref as AR

ONE = 65536
RATIOS = (0, 1, 32768, 65535, 65536)                      # where the blend rule is checked over every (a, p)


# ---------------------------------------------------------------- the rule
def blend(a, p, ratio: int):
    """Integer arrays (or ints) of 8-bit values -> their blend, int64."""
    r = min(max(int(ratio), 0), ONE)
    return (np.asarray(a, np.int64) * r + np.asarray(p, np.int64) * (ONE - r)) >> 16


def raw_planes(e, ims, S: int) -> np.ndarray:
    """Entry `e` over pixel-interleaved `ims` before hue / sat and gain -> int64 (ch, S, S)."""
    u = CR._without_gain(e)
    ch = ims[0].shape[2]
    return np.stack([AR.render_entry(u, [np.ascontiguousarray(a[..., c]) for a in ims], S) for c in range(ch)]) \
        .astype(np.int64)


def render_mix_entry(e, pe, ratio: int, ims, S: int, colour=None) -> np.ndarray:
    """`pe`: the partner entry, or None for an image that is not mixed -> uint8 (ch, S, S)."""
    if pe is None:
        return CR.render_entry_c(e, ims, S, colour)
    v = blend(raw_planes(e, ims, S), raw_planes(pe, ims, S), ratio)
    if colour is not None:
        assert v.shape[0] == 3
        v = np.moveaxis(CR.hue_sat(np.moveaxis(v, 0, -1), *colour), -1, 0)
    return AR._gain(v, e)


def render_mix(table, partner, mix, ims, S: int, colours=None) -> np.ndarray:
    """`table`: one AugEntry per image; `partner`: the compact table (a sequence, may be empty); `mix`: one
    (ratio, partner index) or AugMix per image -> uint8 (len(table), ch, S, S)."""
    n = 0 if partner is None else len(partner)
    out = []
    for i in range(len(table)):
        ratio, k = (mix[i].ratio, mix[i].partner) if hasattr(mix[i], "ratio") else mix[i]
        pe = partner[k] if 0 <= k < n else None
        out.append(render_mix_entry(table[i], pe, ratio, ims, S, None if colours is None else colours[i]))
    return np.stack(out)


# ---------------------------------------------------------------- cases
NONE, AT_N, FAR, FAR_NEG = "none", "n_partner", "int32_max", "int32_min"      # `partner` of an image that is not mixed


def cases(S: int):
    """[(name, primary AugEntry, partner AugEntry or None, ratio, partner index kind)] over CR.sources(S, ch).  A
    kind other than "ok" leaves the image unmixed whatever partner entry the case carries."""
    from datasets import augment as A
    sizes = [hw or (S, S) for hw in CR.SOURCE_SIZES]
    B = len(sizes)

    def plain(b, inv=None, **kw):
        return A.plain_entry(b, *sizes[b], S, inv, **kw)

    def inv_of(canvas, flip=(False, False), **kw):
        return np.linalg.inv(A.affine_matrix(S, canvas, **kw)) @ A.flip_matrix(S, *flip)

    def mosaic(srcs, xc, yc, flip=(False, False), gain=1.0, fill=114, **kw):
        return A.mosaic_entry(srcs, [sizes[b] for b in srcs], xc, yc, S, inv_of(2 * S, flip, **kw), gain=gain,
                              fill=fill)

    rot = lambda b, **kw: plain(b, inv_of(S, (True, False), angle=25.0, scale=0.8), **kw)      # noqa: E731
    # scale 0.5 shows the whole 2S canvas: every row, so every wave of 256 pixels, crosses the mosaic's centre
    split_a = lambda **kw: mosaic([3, 2, 1, 0], S + 3, S - 5, scale=0.5, **kw)                # noqa: E731
    split_b = lambda **kw: mosaic([0, 3, 2, 1], S - 4, S + 6, scale=0.5, **kw)                # noqa: E731
    out = [("plain_x_mosaic", rot(2), split_a(), 32768, "ok"),
           ("mosaic_x_mosaic", split_a(gain=1.2), split_b(), 20000, "ok"),
           ("stretch_x_rot", plain(1, gain=1.3), rot(2), 40000, "ok"),
           ("rot_x_stretch", rot(2, gain=0.9), plain(3), 1, "ok")]
    e = mosaic([3, 2, 1, 0], S + 1, S + 2, scale=0.5)
    e.tile[1].src = -1
    out.append(("partner_empty_slot", plain(3), e, 32768, "ok"))
    e = mosaic([3, 0, 1, 2], S - 2, S + 1, scale=0.5)
    e.tile[1].src, e.tile[3].src = B, 2 ** 31 - 1
    out.append(("partner_src_out_of_range", rot(2), e, 30000, "ok"))
    e = plain(2)
    e.tile[0].src = B
    out.append(("stretch_partner_src_out_of_range", split_b(), e, 32768, "ok"))
    small = inv_of(S, scale=0.5)                           # half size: a band of fill around the image
    out += [("different_fills", plain(3, small, fill=30), plain(2, inv_of(S, scale=0.5, tx=0.7), fill=200), 32768,
             "ok"),
            ("partner_gain_ignored", rot(3, gain=0.9), plain(2, inv_of(S, angle=-10.0), gain=1.7), 32768, "ok"),
            ("ratio_0", rot(2), split_a(), 0, "ok"), ("ratio_65536", rot(2), split_a(), 65536, "ok"),
            ("ratio_65535", rot(2), split_a(), 65535, "ok"), ("ratio_negative", rot(2), split_a(), -5, "ok"),
            ("ratio_above_one", rot(2), split_a(), 70000, "ok"),
            ("partner_minus_one", rot(2, gain=1.1), split_a(), 32768, NONE),
            ("partner_equals_n", split_b(gain=0.8), rot(2), 32768, AT_N),
            ("partner_int32_max", plain(1), split_a(), 12345, FAR),
            ("partner_int32_min", rot(3), split_a(), 12345, FAR_NEG)]
    return out


def check_cases_not_degenerate(S, ch):
    """On the restatement alone: a mixed case differs from both of its unmixed renderings, the ignored gain would
    show, the end-point ratios return one image, an out-of-range partner index leaves the primary's rendering."""
    ims = CR.sources(S, ch)
    by = {c[0]: c for c in cases(S)}
    for name in ("plain_x_mosaic", "mosaic_x_mosaic", "stretch_x_rot", "partner_empty_slot", "partner_src_out_of_range",
                 "different_fills", "partner_gain_ignored", "ratio_65535"):
        _, e, pe, r, _ = by[name]
        mixed = render_mix_entry(e, pe, r, ims, S)
        lone_p = type(pe).from_buffer_copy(bytes(pe))
        lone_p.gain = e.gain
        assert not np.array_equal(mixed, CR.render_entry_c(e, ims, S)), name
        assert not np.array_equal(mixed, CR.render_entry_c(lone_p, ims, S)), name
    _, e, pe, r, _ = by["partner_gain_ignored"]
    gained = blend(raw_planes(e, ims, S), AR._gain(raw_planes(pe, ims, S), pe), r)
    assert pe.gain != 65536 and not np.array_equal(AR._gain(gained, e), render_mix_entry(e, pe, r, ims, S))
    for name, which in (("ratio_0", 1), ("ratio_negative", 1), ("ratio_65536", 0), ("ratio_above_one", 0)):
        _, e, pe, r, _ = by[name]
        want = AR._gain(raw_planes((e, pe)[which], ims, S), e)
        assert np.array_equal(render_mix_entry(e, pe, r, ims, S), want), name
    _, e, pe, _, _ = by["different_fills"]
    assert (e.fill, pe.fill) == (30, 200) and (render_mix_entry(e, pe, 32768, ims, S) == (30 + 200) // 2).any()
    _, e, pe, _, _ = by["rot_x_stretch"]                   # ratio 1: the partner but for at most one level
    d = render_mix_entry(e, pe, 1, ims, S).astype(int) - AR._gain(raw_planes(pe, ims, S), e).astype(int)
    assert np.abs(d).max() <= 1 and (d != 0).any()


def tables_of(chunk, pad_to: int | None = None):
    """Cases -> (ctypes AugEntry table, ctypes compact partner table or None, ctypes AugMix table).  `pad_to`: the
    table is padded to that many images with unmixed copies of the first case's primary entry."""
    from yolomi._lib import AugEntry, AugMix
    prim = [c[1] for c in chunk]
    part = [c[2] for c in chunk if c[4] == "ok" and c[2] is not None]
    n = len(prim) if pad_to is None else pad_to
    table, mix = (AugEntry * n)(), (AugMix * n)()
    partner = (AugEntry * len(part))() if part else None
    for k, e in enumerate(part):
        partner[k] = e
    k = 0
    for i in range(n):
        if i >= len(chunk):
            table[i], mix[i].ratio, mix[i].partner = prim[0], ONE, -1
            continue
        table[i], mix[i].ratio = prim[i], chunk[i][3]
        kind = chunk[i][4]
        if kind == "ok" and chunk[i][2] is not None:
            mix[i].partner, k = k, k + 1
        else:
            mix[i].partner = {NONE: -1, AT_N: len(part), FAR: 2 ** 31 - 1, FAR_NEG: -2 ** 31, "ok": -1}[kind]
    return table, partner, mix


def chunks(S: int, B: int | None = None):
    """The case list in tables of one entry per image of the batch -> (names, table, partner, mix, n real cases)."""
    B = B or len(CR.SOURCE_SIZES)
    cs = cases(S)
    for lo in range(0, len(cs), B):
        chunk = cs[lo:lo + B]
        yield ([c[0] for c in chunk], *tables_of(chunk, B), len(chunk))


# ---------------------------------------------------------------- the host program's files
def write_mix_file(path, partner, mix):
    """int64 header {n_partner, n_mix}, the partner entries, the mix records (native endianness)."""
    n = 0 if partner is None else len(partner)
    with open(path, "wb") as f:
        f.write(struct.pack("=2q", n, len(mix)))
        if n:
            f.write(bytes(partner))
        f.write(bytes(mix))


def run_host(exe, tmp_path, table, partner, mix, ims, S: int, colours=None, timeout=120) -> np.ndarray:
    """tests/augment_mix_host.cpp over the tables -> uint8 (len(table), ch, S, S)."""
    import subprocess
    ch, n = ims[0].shape[2], len(table)
    assert len(mix) == n and ctypes.sizeof(mix) == 8 * n
    AR.write_case_file(tmp_path / "cases.bin", table, n, ims, S)
    write_mix_file(tmp_path / "mix.bin", partner, mix)
    cmd = [str(exe), "render", str(tmp_path / "cases.bin"), str(tmp_path / "mix.bin"), str(tmp_path / "out.bin"),
           str(ch)]
    if colours is not None:
        (tmp_path / "colour.bin").write_bytes(bytes(CR.colour_table(colours)))
        cmd.append(str(tmp_path / "colour.bin"))
    subprocess.run(cmd, check=True, timeout=timeout)
    return np.fromfile(tmp_path / "out.bin", dtype=np.uint8).reshape(n, ch, S, S)
