"""Training augmentation on the GPU: mosaic, random affine, flips and a value gain in one launch.

The reference trainer builds its dataset with augment=True (train_yolo11_cuda.py:491) and never reads the flag
(crater_dataset_cuda.py:50).  Here the flag's meaning is supplied in the Ultralytics v8 style: `BatchAugment` draws
every image's parameters on the host, composes flip, affine, mosaic placement and the loader's S-stretch into one
2x3 map per tile, rounds the maps once to fixed point (include/yolomi.h: ym_aug_entry) and one ym_augment_u8 launch
samples the packed uint8 batch that `collate_fn_cuda` produced straight into the fp32 (B, 1, S, S) batch.  No S x S
intermediate exists; a mosaic's three extra tiles are other images of the same batch, already in HBM.  The boxes
(a few dozen rows) are transformed on the host, which therefore still knows max_gt.

Geometry (Ultralytics Mosaic + RandomPerspective without the perspective term), in pixel-index coordinates:
  canvas     without mosaic the S x S stretch of the image; with mosaic 2S x 2S, centre (xc, yc) integer uniform in
             [S/2, 3S/2)^2, four S x S stretched tiles touching the centre with one corner, cropped by the canvas
  affine     A = T * Shear * R(angle, scale) * C: C moves the canvas centre to the origin, T moves it to
             uniform(0.5 - translate, 0.5 + translate) * S; the output is the S x S window at the origin
  flips      on the output (pixel index S - 1 - x; boxes 1 - x on the normalised coordinate)
An image whose geometry is the identity is flagged YM_AUG_STRETCH and equals the validation path's resize bit for bit.

Batches of 2-4 planes (pixel-interleaved images, `img_ch` in the batch dict: datasets/yolo_txt.py) go through
ym_augment_u8c with the same table: the geometry is formed once per pixel, every plane is blended at the same taps and
takes the gain.  On 3-plane batches `hsv_h` / `hsv_s` add a per-image hue shift and saturation factor (a second table
of ym_aug_colour, appended to the first for the transfer); their uniforms are drawn after every other one.

MixUp (`mixup`, off by default): with that probability an image is blended with a second, independent mosaic + affine
sample around another image of the same batch, r ~ Beta(32, 32) the weight of the first.  Both samples are taken in
the one launch (ym_augment_mix_u8c) and blended per plane in integers before hue / saturation and the gain, which act
on the blend as in Ultralytics; the flips are the primary's for both, and the partner's kept boxes follow the
primary's.  Its draws come after the hue / saturation ones; mosaic closing (`no_mosaic_from`) closes it too.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math

import numpy as np
import torch

from yolomi._lib import AugColour, AugEntry, AugMix, AugTile

FB = 24                        # YM_AUG_FB
STRETCH = 1                    # YM_AUG_STRETCH
_I64_MAX = (1 << 63) - 1


@dataclasses.dataclass
class AugmentHyp:
    """Hyperparameters, named as in Ultralytics' v8 trainer (`gain` is their hsv_v and applies to every plane).
    `hsv_h` (+/- fraction of a turn, a hue shift) and `hsv_s` (+/- fraction around 1, a saturation factor) act on
    3-plane batches only and default to off: the 1-plane recipe is unchanged."""
    mosaic: float = 1.0
    degrees: float = 0.0
    translate: float = 0.1
    scale: float = 0.5
    shear: float = 0.0
    fliplr: float = 0.5
    flipud: float = 0.0
    gain: float = 0.4
    fill: int = 114
    hsv_h: float = 0.0
    hsv_s: float = 0.0
    mixup: float = 0.0             # probability that an image is blended with a second sample (off by default)

    def is_off(self) -> bool:
        return not any((self.mosaic, self.degrees, self.translate, self.scale, self.shear, self.fliplr, self.flipud,
                        self.gain, self.hsv_h, self.hsv_s, self.mixup))


def _fix(v) -> int:
    """fp64 -> fixed point with FB fraction bits, rounded once."""
    return int(np.rint(np.float64(v) * np.float64(1 << FB)))


def translation(tx, ty):
    return np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]])


def stretch_map(h0: int, w0: int, S: int):
    """Stretched-tile pixel index -> source pixel position: u = (j + 0.5) * w0 / S - 0.5 (the loader's resize)."""
    return np.array([[w0 / S, 0.0, 0.5 * w0 / S - 0.5], [0.0, h0 / S, 0.5 * h0 / S - 0.5], [0.0, 0.0, 1.0]])


def make_tile(src: int, m, rect) -> AugTile:
    """`m`: 2x3 (or 3x3) fp64 output pixel -> source position; `rect`: (x0, y0, x1, y1) canvas, half open."""
    t = AugTile()
    m = np.asarray(m, np.float64)
    for i in range(6):
        t.m[i] = _fix(m[i // 3, i % 3])
    t.x0, t.y0, t.x1, t.y1 = (_fix(v) for v in rect)
    t.src = int(src)
    return t


def make_entry(tiles, c, centre=None, gain=1.0, fill=114, stretch=False) -> AugEntry:
    """`tiles`: up to four AugTile or None by slot (slot = (cx >= xc) + 2 * (cy >= yc)); `c`: fp64 output pixel ->
    canvas; `centre`: (xc, yc) canvas pixel index of the first pixel of the right / lower tiles, or None."""
    e = AugEntry()
    for k in range(4):
        t = tiles[k] if k < len(tiles) else None
        if t is None:
            e.tile[k].src = -1
        else:
            e.tile[k] = t
    c = np.asarray(c, np.float64)
    for i in range(6):
        e.c[i] = _fix(c[i // 3, i % 3])
    if centre is None:
        e.xc = e.yc = _I64_MAX
    else:
        e.xc, e.yc = _fix(centre[0] - 0.5), _fix(centre[1] - 0.5)
    e.gain = int(np.rint(np.float64(gain) * 65536.0))
    e.fill = int(fill)
    e.flags = STRETCH if stretch else 0
    return e


def letterbox_map(h0: int, w0: int, lb):
    """Letterboxed-tile pixel index -> source pixel position: the stretch to (nw, nh) after the translation by
    (-left, -top).  `lb`: (nw, nh, left, top) with nw, nh > 0."""
    nw, nh, left, top = (int(v) for v in lb)
    m = np.array([[w0 / nw, 0.0, 0.5 * w0 / nw - 0.5], [0.0, h0 / nh, 0.5 * h0 / nh - 0.5], [0.0, 0.0, 1.0]])
    return m @ translation(-left, -top)


def _letterbox_tile(src: int, h0: int, w0: int, lb, origin, crop, inv) -> AugTile | None:
    """Tile of a letterboxed image whose frame sits at canvas pixel `origin`: sampled through letterbox_map, owned
    where the image's interior meets `crop` (canvas, half open); None when the image has no interior."""
    nw, nh, left, top = (int(v) for v in lb)
    if nw <= 0 or nh <= 0:
        return None
    ox, oy = origin
    rect = (max(crop[0], ox + left - 0.5), max(crop[1], oy + top - 0.5), min(crop[2], ox + left + nw - 0.5),
            min(crop[3], oy + top + nh - 0.5))
    return make_tile(src, letterbox_map(h0, w0, lb) @ translation(-ox, -oy) @ inv, rect)


def plain_entry(src: int, h0: int, w0: int, S: int, inv=None, gain=1.0, fill=114, lb=None) -> AugEntry:
    """One stretched image under `inv` (3x3 fp64, output pixel -> canvas pixel; None: identity, flagged).
    `lb` (nw, nh, left, top): the image is letterboxed instead; the identity then goes unflagged through the same
    fixed-point map as every other entry (the flag means the S x S stretch)."""
    if lb is not None:
        c = np.eye(3) if inv is None else inv
        return make_entry([_letterbox_tile(src, h0, w0, lb, (0, 0), (-0.5, -0.5, S - 0.5, S - 0.5), c)], c, None,
                          gain, fill)
    if inv is None:
        return make_entry([make_tile(src, stretch_map(h0, w0, S), (-0.5, -0.5, S - 0.5, S - 0.5))], np.eye(3), None,
                          gain, fill, stretch=True)
    tile = make_tile(src, stretch_map(h0, w0, S) @ inv, (-0.5, -0.5, S - 0.5, S - 0.5))
    return make_entry([tile], inv, None, gain, fill)


def mosaic_origins(xc: int, yc: int, S: int):
    """Canvas pixel index of each slot's tile origin: the tiles touch (xc, yc) with one corner."""
    return [(xc - S, yc - S), (xc, yc - S), (xc - S, yc), (xc, yc)]


def mosaic_entry(srcs, sizes, xc: int, yc: int, S: int, inv, gain=1.0, fill=114, lbs=None) -> AugEntry:
    """Four stretched tiles (`srcs` batch indices, `sizes` their (h0, w0)) on the 2S canvas around (xc, yc).
    `lbs`: the tiles' (nw, nh, left, top); they are letterboxed instead and their pad shows the fill."""
    tiles = []
    for k, ((ox, oy), b, (h0, w0)) in enumerate(zip(mosaic_origins(xc, yc, S), srcs, sizes)):
        rect = (max(ox, 0) - 0.5, max(oy, 0) - 0.5, min(ox + S, 2 * S) - 0.5, min(oy + S, 2 * S) - 0.5)
        if lbs is not None:
            tiles.append(_letterbox_tile(b, h0, w0, lbs[k], (ox, oy), rect, inv))
            continue
        tiles.append(make_tile(b, stretch_map(h0, w0, S) @ translation(-ox, -oy) @ inv, rect))
    return make_entry(tiles, inv, (xc, yc), gain, fill)


def affine_matrix(S: int, canvas: int, angle=0.0, scale=1.0, shear_x=0.0, shear_y=0.0, tx=0.5, ty=0.5):
    """A = T * Shear * R * C (3x3 fp64, canvas pixel -> output pixel); angles in degrees, tx / ty fractions of S."""
    C = translation(-canvas / 2, -canvas / 2)
    a = math.radians(angle)
    R = np.array([[scale * math.cos(a), scale * math.sin(a), 0.0], [-scale * math.sin(a), scale * math.cos(a), 0.0],
                  [0.0, 0.0, 1.0]])
    Sh = np.array([[1.0, math.tan(math.radians(shear_x)), 0.0], [math.tan(math.radians(shear_y)), 1.0, 0.0],
                   [0.0, 0.0, 1.0]])
    return translation(tx * S, ty * S) @ Sh @ R @ C


def flip_matrix(S: int, lr: bool, ud: bool):
    """Output pixel index flips (3x3 fp64)."""
    F = np.eye(3)
    if lr:
        F[0, 0], F[0, 2] = -1.0, S - 1.0
    if ud:
        F[1, 1], F[1, 2] = -1.0, S - 1.0
    return F


def box_candidates(pre, post, wh_thr=2.0, ar_thr=100.0, area_thr=0.1, eps=1e-16):
    """Ultralytics' filter on pixel xyxy rows: `pre` before and `post` after clipping to the image."""
    w1, h1 = pre[:, 2] - pre[:, 0], pre[:, 3] - pre[:, 1]
    w2, h2 = post[:, 2] - post[:, 0], post[:, 3] - post[:, 1]
    ar = np.maximum(w2 / (h2 + eps), h2 / (w2 + eps))
    return (w2 > wh_thr) & (h2 > wh_thr) & (w2 * h2 / (w1 * h1 + eps) >= area_thr) & (ar < ar_thr)


def transform_boxes(xyxy, A, S: int, lr: bool, ud: bool):
    """Canvas pixel xyxy (n, 4) fp64 -> (normalised xyxy of the survivors, keep mask): the four corners through A,
    their axis-aligned hull, clipped to [0, S], filtered, normalised, flipped."""
    n = len(xyxy)
    if n == 0:
        return np.zeros((0, 4)), np.zeros((0,), bool)
    pts = np.ones((n * 4, 3))
    pts[:, :2] = xyxy[:, [0, 1, 2, 3, 0, 3, 2, 1]].reshape(n * 4, 2)
    pts = (pts @ A.T)[:, :2].reshape(n, 4, 2)
    pre = np.concatenate([pts.min(1), pts.max(1)], 1)
    post = np.clip(pre, 0.0, float(S))
    keep = box_candidates(pre, post)
    out = post[keep] / float(S)
    if lr:
        out[:, [0, 2]] = 1.0 - out[:, [2, 0]]
    if ud:
        out[:, [1, 3]] = 1.0 - out[:, [3, 1]]
    return out, keep


def step_seed(seed: int, rank: int, epoch: int, step: int) -> int:
    """One 63-bit generator seed from the four counters (any one changing changes it)."""
    ss = np.random.SeedSequence([int(seed) & 0xFFFFFFFF, int(rank), int(epoch), int(step)])
    return int(ss.generate_state(1, np.uint64)[0]) & _I64_MAX


def augment_batch(img_u8: torch.Tensor, meta: torch.Tensor, table: torch.Tensor, img_size: int, channels: int = 1,
                  colour: torch.Tensor | None = None) -> torch.Tensor:
    """GPU: packed uint8 images + device table of ym_aug_entry (uint8 bytes) -> (B, channels, S, S) fp32
    (ym_augment_u8; ym_augment_u8c for channels > 1, whose source is pixel-interleaved, or with `colour`, a device
    table of ym_aug_colour as uint8 bytes, channels == 3 only)."""
    from yolomi._lib import call, ptr, require_device, stream_ptr
    require_device(img_u8, meta, table, colour)
    B = meta.shape[0]
    assert table.dtype == torch.uint8 and table.numel() == B * ctypes.sizeof(AugEntry)
    assert colour is None or (colour.dtype == torch.uint8 and colour.numel() == B * ctypes.sizeof(AugColour))
    out = torch.empty(B, channels, img_size, img_size, dtype=torch.float32, device=img_u8.device)
    if channels == 1 and colour is None:
        call("ym_augment_u8", img_u8.data_ptr(), meta.contiguous().data_ptr(), table.data_ptr(), B, img_size,
             out.data_ptr(), stream_ptr(img_u8.device))
    else:
        call("ym_augment_u8c", img_u8.data_ptr(), meta.contiguous().data_ptr(), table.data_ptr(), ptr(colour), B,
             channels, img_size, out.data_ptr(), stream_ptr(img_u8.device))
    return out


def augment_mix_batch(img_u8: torch.Tensor, meta: torch.Tensor, table: torch.Tensor, partner: torch.Tensor | None,
                      mix: torch.Tensor, img_size: int, channels: int = 1,
                      colour: torch.Tensor | None = None) -> torch.Tensor:
    """augment_batch with MixUp in the launch (ym_augment_mix_u8c, for every plane count): `partner` a device table
    of ym_aug_entry for the mixed images only (None: no image is mixed), `mix` one ym_aug_mix per image, both as uint8
    bytes."""
    from yolomi._lib import call, ptr, require_device, stream_ptr
    require_device(img_u8, meta, table, partner, mix, colour)
    B = meta.shape[0]
    assert table.dtype == torch.uint8 and table.numel() == B * ctypes.sizeof(AugEntry)
    n_partner = 0 if partner is None else partner.numel() // ctypes.sizeof(AugEntry)
    assert partner is None or (partner.dtype == torch.uint8 and partner.numel() == n_partner * ctypes.sizeof(AugEntry))
    assert mix.dtype == torch.uint8 and mix.numel() == B * ctypes.sizeof(AugMix)
    assert colour is None or (colour.dtype == torch.uint8 and colour.numel() == B * ctypes.sizeof(AugColour))
    out = torch.empty(B, channels, img_size, img_size, dtype=torch.float32, device=img_u8.device)
    call("ym_augment_mix_u8c", img_u8.data_ptr(), meta.contiguous().data_ptr(), table.data_ptr(), ptr(partner),
         n_partner, mix.data_ptr(), ptr(colour), B, channels, img_size, out.data_ptr(), stream_ptr(img_u8.device))
    return out


def table_bytes(entries) -> torch.Tensor:
    """ctypes array of AugEntry (or AugColour) -> host uint8 tensor (a copy)."""
    return torch.from_numpy(np.frombuffer(bytes(entries), dtype=np.uint8).copy())


def colour_table(hue, sat):
    """Per-image hue shifts (turns) and saturation factors -> ctypes array of AugColour (Q16; the hue modulo one
    turn, the factor clamped to [0, 2])."""
    n = len(hue)
    t = (AugColour * max(n, 1))()
    for i in range(n):
        t[i].hue = int(np.rint(np.float64(hue[i]) * 65536.0)) & 65535
        t[i].sat = min(max(int(np.rint(np.float64(sat[i]) * 65536.0)), 0), 1 << 17)
    return t


class BatchAugment:
    """Draws a batch's augmentation on the host and applies it on the device (see the module doc).

    aug(batch, device, epoch, step) takes a collated host batch and returns the dict `prepare_batch` returns (img,
    batch_idx, cls, bboxes, max_gt).  The parameters come from a torch.Generator seeded from (seed, rank, epoch,
    step): a run is reproducible, ranks differ, and resuming needs no saved state.  `no_mosaic_from`: epochs (the
    number handed to the call) from this one on draw no mosaic."""

    def __init__(self, hyp: AugmentHyp | None = None, seed: int = 0, rank: int = 0, no_mosaic_from: int | None = None):
        self.hyp = hyp or AugmentHyp()
        self.seed, self.rank, self.no_mosaic_from = int(seed), int(rank), no_mosaic_from

    def draw(self, B: int, epoch: int, step: int) -> dict:
        """Per-image parameters (numpy arrays of length B)."""
        h = self.hyp
        g = torch.Generator().manual_seed(step_seed(self.seed, self.rank, epoch, step))
        u = torch.rand(B, 11, generator=g, dtype=torch.float64).numpy()
        partners = torch.randint(0, max(B, 1), (B, 3), generator=g).numpy()
        mosaic_on = self.no_mosaic_from is None or epoch < self.no_mosaic_from
        sym = lambda col, r: (2.0 * u[:, col] - 1.0) * r        # noqa: E731  uniform(-r, r)
        gain = 1.0 + (2.0 * torch.rand(B, generator=g, dtype=torch.float64).numpy() - 1.0) * h.gain
        # hue and saturation are taken from the generator last: every other key is what it was before they existed
        hs = 2.0 * torch.rand(B, 2, generator=g, dtype=torch.float64).numpy() - 1.0
        out = {"mosaic": (u[:, 0] < h.mosaic) & mosaic_on, "cx": u[:, 1], "cy": u[:, 2], "partners": partners,
               "angle": sym(3, h.degrees), "scale": 1.0 + sym(4, h.scale), "shear_x": sym(5, h.shear),
               "shear_y": sym(6, h.shear), "tx": 0.5 + sym(7, h.translate), "ty": 0.5 + sym(8, h.translate),
               "fliplr": u[:, 9] < h.fliplr, "flipud": u[:, 10] < h.flipud, "gain": gain,
               "hue": hs[:, 0] * h.hsv_h, "sat": 1.0 + hs[:, 1] * h.hsv_s}
        # MixUp comes after hue and saturation for the same reason.  Column 0 of `w` is the mix decision, 1-9 the
        # partner sample's mosaic decision, centre, angle, scale, shears and translations; then its source image and
        # its three mosaic partners.  r ~ Beta(32, 32) exactly as X / (X + Y) of two Gamma(32, 1) draws, each the sum
        # of 32 Exp(1) draws -log(1 - U) of the same generator (an integer shape needs no rejection sampler).
        w = torch.rand(B, 10, generator=g, dtype=torch.float64).numpy()
        mix_src = torch.randint(0, max(B, 1), (B,), generator=g).numpy()
        mix_partners = torch.randint(0, max(B, 1), (B, 3), generator=g).numpy()
        xy = -torch.log1p(-torch.rand(B, 2, 32, generator=g, dtype=torch.float64)).sum(-1).numpy()
        symw = lambda col, r: (2.0 * w[:, col] - 1.0) * r        # noqa: E731
        out.update({"mix": (w[:, 0] < h.mixup) & mosaic_on, "mix_ratio": xy[:, 0] / (xy[:, 0] + xy[:, 1]),
                    "mix_src": mix_src, "mix_mosaic": (w[:, 1] < h.mosaic) & mosaic_on, "mix_cx": w[:, 2],
                    "mix_cy": w[:, 3], "mix_partners": mix_partners, "mix_angle": symw(4, h.degrees),
                    "mix_scale": 1.0 + symw(5, h.scale), "mix_shear_x": symw(6, h.shear),
                    "mix_shear_y": symw(7, h.shear), "mix_tx": 0.5 + symw(8, h.translate),
                    "mix_ty": 0.5 + symw(9, h.translate)})
        return out

    def colours(self, B: int, epoch: int, step: int):
        """The batch's ctypes table of AugColour, or None when hue and saturation are both off."""
        if not (self.hyp.hsv_h or self.hyp.hsv_s):
            return None
        p = self.draw(B, epoch, step)
        return colour_table(p["hue"], p["sat"])

    def _sample(self, ctx, src: int, g: dict, lr: bool, ud: bool, gain: float):
        """One mosaic + affine sample around image `src` of the batch from the parameter set `g` (mosaic, cx, cy,
        partners, angle, scale, shear_x, shear_y, tx, ty) under the flips (lr, ud) -> (AugEntry, kept classes,
        transformed boxes).  The primary and the MixUp partner of an image both come from here."""
        S, meta, geo, lb_of, rows_of, boxes, cls = ctx
        mosaic = bool(g["mosaic"])
        A = affine_matrix(S, 2 * S if mosaic else S, g["angle"], g["scale"], g["shear_x"], g["shear_y"], g["tx"],
                          g["ty"])
        if not mosaic and not lr and not ud and np.array_equal(A, np.eye(3)):
            entry = plain_entry(src, int(meta[src, 1]), int(meta[src, 2]), S, None, gain, self.hyp.fill, lb=lb_of(src))
            rows = rows_of[src]
            return entry, cls[rows], boxes[rows]
        inv = np.linalg.inv(A) @ flip_matrix(S, lr, ud)          # output pixel -> canvas pixel
        if mosaic:
            xc, yc = (int(S / 2 + c * S) for c in (g["cx"], g["cy"]))
            srcs = [src, *(int(b) for b in g["partners"])]
            entry = mosaic_entry(srcs, [(int(meta[b, 1]), int(meta[b, 2])) for b in srcs], xc, yc, S, inv, gain,
                                 self.hyp.fill, lbs=[lb_of(b) for b in srcs] if geo is not None else None)
            parts = []
            for (ox, oy), b in zip(mosaic_origins(xc, yc, S), srcs):
                parts.append(np.clip(boxes[rows_of[b]] * S + np.array([ox, oy, ox, oy], np.float64), 0, 2 * S))
            canvas_boxes = np.concatenate(parts)
            rows = np.concatenate([rows_of[b] for b in srcs])
        else:
            entry = plain_entry(src, int(meta[src, 1]), int(meta[src, 2]), S, inv, gain, self.hyp.fill, lb=lb_of(src))
            rows = rows_of[src]
            canvas_boxes = boxes[rows] * S
        out, keep = transform_boxes(canvas_boxes, A, S, lr, ud)
        return entry, cls[rows][keep], out

    _GEOMETRY = ("mosaic", "cx", "cy", "partners", "angle", "scale", "shear_x", "shear_y", "tx", "ty")

    def plan(self, batch: dict, epoch: int, step: int):
        """Host side of one batch -> (ctypes table of AugEntry, batch_idx, cls, bboxes, max_gt).  With `mixup` the
        rows of a mixed image are its own kept rows followed by its partner sample's (plan_mix gives the tables)."""
        return self.plan_mix(batch, epoch, step)[:5]

    def plan_mix(self, batch: dict, epoch: int, step: int):
        """plan()'s five, then (ctypes table of the mixed images' partner AugEntry, ctypes table of one AugMix per
        image), or (None, None) when no image of the batch is mixed.  A mixed image's partner is a second, independent
        mosaic + affine sample around another image of the batch under the primary's flips (Ultralytics flips after
        the blend); its kept boxes and classes follow the primary's in image i's rows, unweighted.  The partner
        entry's gain is 1 and is ignored by the kernel: the primary's gain acts on the blend."""
        from .crater import max_gt_count
        meta = batch["img_meta"].numpy()
        S, B = int(batch["img_size"]), int(meta.shape[0])
        p = self.draw(B, epoch, step)
        # a letterboxed batch (collate_fn_cuda(letterbox=True)): every tile keeps its aspect ratio; the boxes are
        # already in the letterboxed frame, so nothing below changes for them
        geo = batch["img_lb"].numpy() if "img_lb" in batch else None
        lb_of = (lambda b: geo[b].tolist()) if geo is not None else (lambda b: None)
        bidx = batch["batch_idx"].numpy().reshape(-1)
        boxes = batch["bboxes"].numpy().astype(np.float64).reshape(-1, 4)
        cls = batch["cls"].numpy()
        rows_of = [np.nonzero(bidx == i)[0] for i in range(B)]
        ctx = (S, meta, geo, lb_of, rows_of, boxes, cls)
        table = (AugEntry * max(B, 1))()
        mixed = [i for i in range(B) if p["mix"][i]]
        partner = (AugEntry * len(mixed))() if mixed else None
        mix = (AugMix * B)() if mixed else None
        o_idx, o_cls, o_box = [], [], []
        for i in range(B):
            lr, ud, gain = bool(p["fliplr"][i]), bool(p["flipud"][i]), float(p["gain"][i])
            table[i], kept, out = self._sample(ctx, i, {k: p[k][i] for k in self._GEOMETRY}, lr, ud, gain)
            o_idx.append(np.full(len(out), i)), o_cls.append(kept), o_box.append(out)
            if mix is None:
                continue
            mix[i].ratio, mix[i].partner = 65536, -1
            if p["mix"][i]:
                k = mixed.index(i)
                partner[k], kept, out = self._sample(ctx, int(p["mix_src"][i]),
                                                     {g: p["mix_" + g][i] for g in self._GEOMETRY}, lr, ud, 1.0)
                mix[i].ratio, mix[i].partner = int(math.floor(float(p["mix_ratio"][i]) * 65536.0 + 0.5)), k
                o_idx.append(np.full(len(out), i)), o_cls.append(kept), o_box.append(out)
        if B == 0 or not sum(len(x) for x in o_idx):
            bi, cl, bb = (torch.zeros((0,), dtype=torch.long), torch.zeros((0, 1), dtype=batch["cls"].dtype),
                          torch.zeros((0, 4), dtype=torch.float32))
        else:
            bi = torch.from_numpy(np.concatenate(o_idx)).long()
            cl = torch.from_numpy(np.concatenate(o_cls)).to(batch["cls"].dtype).reshape(-1, 1)
            bb = torch.from_numpy(np.concatenate(o_box)).float().clamp_(0.0, 1.0)
        return table, bi, cl, bb, max_gt_count(bi), partner, mix

    def __call__(self, batch: dict, device, epoch: int, step: int) -> dict:
        from .crater import prepare_batch
        if "img_u8" not in batch or self.hyp.is_off() or batch["img_meta"].shape[0] == 0:
            return prepare_batch(batch, device)              # synthetic batches carry no raw images
        table, bi, cl, bb, max_gt, partner, mix = self.plan_mix(batch, epoch, step)
        B, ch = int(batch["img_meta"].shape[0]), int(batch.get("img_ch", 1))
        colour = self.colours(B, epoch, step) if ch == 3 else None
        # one buffer, one transfer: the primary table (B * 432 bytes), then for a batch with a mixed image the partner
        # table (432 each) and the mix records (8 each), then the colour table (8 each): every offset is 8-byte aligned
        parts = [table_bytes(t) for t in (table, partner, mix, colour) if t is not None]
        cuts = np.cumsum([0] + [t.numel() for t in parts]).tolist()
        tb = torch.cat(parts) if len(parts) > 1 else parts[0]
        if torch.device(device).type == "cuda":
            tb = tb.pin_memory()
        mv = lambda t: t.to(device, non_blocking=True)          # noqa: E731
        tb = mv(tb)
        views = [tb[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])]
        col = views[-1] if colour is not None else None
        if mix is None:
            img = augment_batch(mv(batch["img_u8"]), mv(batch["img_meta"]), views[0], int(batch["img_size"]), ch, col)
        else:
            img = augment_mix_batch(mv(batch["img_u8"]), mv(batch["img_meta"]), views[0], views[1], views[2],
                                    int(batch["img_size"]), ch, col)
        return {"max_gt": max_gt, "img": img, "batch_idx": mv(bi), "cls": mv(cl), "bboxes": mv(bb)}
