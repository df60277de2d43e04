"""The table cases the augmentation kernel is held to, shared by the host-program test (CPU) and the GPU test."""
from __future__ import annotations

import numpy as np

SOURCE_SIZES = [(1, 2), (3, 1000), (81, 127), None, (480, 640), (700, 517), (1024, 1024)]      # None: (S, S)


def sources(S: int, seed: int = 0):
    rng = np.random.default_rng(1000 + S + seed)
    return [rng.integers(0, 256, hw or (S, S), dtype=np.uint8) for hw in SOURCE_SIZES]


def cases(S: int):
    """[(name, AugEntry)] over sources(S)."""
    from datasets import augment as A
    sizes = [hw or (S, S) for hw in SOURCE_SIZES]

    def plain(b, inv=None, **kw):
        return A.plain_entry(b, *sizes[b], S, inv, **kw)

    def inv_of(canvas, flip=(False, False), **kw):
        return np.linalg.inv(A.affine_matrix(S, canvas, **kw)) @ A.flip_matrix(S, *flip)

    def mosaic(srcs, xc, yc, flip=(False, False), **kw):
        return A.mosaic_entry(srcs, [sizes[b] for b in srcs], xc, yc, S, inv_of(2 * S, flip, **kw))

    out = [(f"identity{b}", plain(b)) for b in range(7)]
    out += [("fliplr", plain(2, inv_of(S, (True, False)))), ("flipud", plain(4, inv_of(S, (False, True)))),
            ("flipboth", plain(3, inv_of(S, (True, True)))),
            ("rot37_s0.5", plain(4, inv_of(S, angle=37.0, scale=0.5))),
            ("rot37_s1.5", plain(5, inv_of(S, angle=37.0, scale=1.5))),
            ("shear", plain(6, inv_of(S, shear_x=10.0, shear_y=-7.0))),
            ("pushed_out", plain(5, inv_of(S, tx=1.3, ty=-0.2))),
            ("mosaic_lo", mosaic([4, 5, 6, 2], S // 2, S // 2, scale=0.5)),
            ("mosaic_hi", mosaic([4, 5, 6, 2], 3 * S // 2, 3 * S // 2, scale=0.5)),
            ("mosaic_mid", mosaic([4, 5, 6, 2], S, S)),
            ("mosaic_off", mosaic([3, 2, 5, 4], (4 * S) // 5, (11 * S) // 10, (True, False), angle=-12.0, scale=0.8,
                                  tx=0.45, ty=0.58)),
            ("mosaic_same", mosaic([6, 6, 6, 6], S + 3, S - 5, scale=0.6)),
            ("mosaic_thin", mosaic([0, 1, 0, 1], S - 7, S + 2, scale=0.7)),
            ("gain0.6", plain(4, gain=0.6)), ("gain1.4", plain(5, gain=1.4)),
            ("gain1.4_rot", plain(6, inv_of(S, angle=5.0, scale=1.1), gain=1.4))]
    return out


def big_case():
    """S = 640, B = 4: more pixels per image than one pass of the kernel's grid covers."""
    from datasets import augment as A
    S = 640
    sizes = [(480, 640), (700, 517), (1024, 1024), (640, 640)]
    rng = np.random.default_rng(640)
    ims = [rng.integers(0, 256, hw, dtype=np.uint8) for hw in sizes]
    inv = np.linalg.inv(A.affine_matrix(S, 2 * S, scale=0.8, tx=0.55, ty=0.42)) @ A.flip_matrix(S, True, False)
    rot = np.linalg.inv(A.affine_matrix(S, S, angle=10.0, scale=1.2, shear_x=2.0))
    entries = [A.plain_entry(0, *sizes[0], S), A.mosaic_entry([1, 2, 3, 0], [sizes[b] for b in (1, 2, 3, 0)], 500, 790,
                                                              S, inv, gain=1.2),
               A.plain_entry(2, *sizes[2], S, rot, gain=0.8),
               A.plain_entry(3, *sizes[3], S, A.flip_matrix(S, False, True))]
    return ims, table_of(entries)


def table_of(entries):
    from yolomi._lib import AugEntry
    t = (AugEntry * len(entries))()
    for i, e in enumerate(entries):
        t[i] = e
    return t
