"""MixUp without a GPU: the per-pixel functions (include/yolomi_augment.h: ym_aug_mix_sample_c) built for the host
with the address and undefined-behaviour sanitizers as a stand-alone program and held byte for byte to the numpy
restatement (tests/augment_mix_ref.py) over the GPU test's case list and over adversarial tables; the blend rule over
every (a, p) pair; BatchAugment's draws and plan with `mixup`; the trainer's flag and the struct layout."""
import ctypes
import dataclasses
import shutil
import subprocess

import numpy as np
import pytest
import torch

import augment_colour_ref as CR
import augment_mix_ref as MR
import augment_ref as AR
from conftest import ROOT


# ---------------------------------------------------------------- the shared header, built for the host
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("mixhost") / "augment_mix_host"
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "augment_mix_host.cpp"), "-o", str(exe)], check=True)
    return exe


def _all_cases(S):
    cs = MR.cases(S)
    return cs, MR.tables_of(cs)


@pytest.mark.parametrize("S", [32, 31])
@pytest.mark.parametrize("ch", [1, 2, 3, 4])
def test_host_build_equals_restatement(host_program, tmp_path, S, ch):
    ims = CR.sources(S, ch)
    cs, (table, partner, mix) = _all_cases(S)
    got = MR.run_host(host_program, tmp_path, table, partner, mix, ims, S)
    want = MR.render_mix(table, partner, mix, ims, S)
    for i, c in enumerate(cs):
        assert np.array_equal(got[i], want[i]), (c[0], int((got[i] != want[i]).sum()))
    MR.check_cases_not_degenerate(S, ch)
    # an image without a valid partner is the unmixed function of its primary entry
    for i, c in enumerate(cs):
        if c[4] != "ok":
            assert np.array_equal(want[i], CR.render_entry_c(c[1], ims, S)), c[0]
    assert sum(c[4] != "ok" for c in cs) == 4 and len(partner) == len(cs) - 4
    assert mix[[c[0] for c in cs].index("partner_equals_n")].partner == len(partner)


@pytest.mark.parametrize("S", [32, 31])
def test_host_build_equals_restatement_with_colour(host_program, tmp_path, S):
    ims = CR.sources(S, 3)
    cs, (table, partner, mix) = _all_cases(S)
    colours = CR.colours_of(len(cs), seed=S)
    got = MR.run_host(host_program, tmp_path, table, partner, mix, ims, S, colours)
    want = MR.render_mix(table, partner, mix, ims, S, colours)
    for i, c in enumerate(cs):
        assert np.array_equal(got[i], want[i]), (c[0], colours[i], int((got[i] != want[i]).sum()))
    assert not np.array_equal(want[1:], MR.render_mix(table, partner, mix, ims, S)[1:])
    # hue / sat act on the blend, not on the two images: blending two coloured renderings is something else
    i = [c[0] for c in cs].index("mosaic_x_mosaic")
    e, pe, r = cs[i][1], cs[i][2], cs[i][3]
    hs = lambda x: np.moveaxis(CR.hue_sat(np.moveaxis(x, 0, -1), *colours[i]), -1, 0)      # noqa: E731
    before = AR._gain(MR.blend(hs(MR.raw_planes(e, ims, S)), hs(MR.raw_planes(pe, ims, S)), r), e)
    assert colours[i] != (0, 65536) and not np.array_equal(before, want[i])


def _random_entries(rng, n, B):
    """Entries whose every field is random.  Half of them anywhere: int64 fields of a random magnitude up to the full
    range, sources around [0, B) or anywhere in int32, any flags, fill and gain.  The other half at magnitudes where
    the maps walk over the sources (a few source pixels per output pixel), so that taps of every kind are formed."""
    from yolomi._lib import AugEntry

    def i64(bits=None):
        if bits is not None:
            return int(rng.integers(-2 ** bits, 2 ** bits, dtype=np.int64))
        return int(rng.integers(-2 ** 63, 2 ** 63, dtype=np.int64)) >> int(rng.integers(0, 64))

    def i32():
        return int(rng.integers(-2 ** 31, 2 ** 31)) >> int(rng.integers(0, 32))

    t = (AugEntry * n)()
    for j, e in enumerate(t):
        wild = j % 2 == 0
        step, off = (None, None) if wild else (27, 32)     # +/- 8 source pixels a pixel, +/- 256 pixels offset
        for tl in e.tile:
            for k in range(6):
                tl.m[k] = i64(off if k % 3 == 2 else step)
            if rng.integers(0, 2):
                tl.x0, tl.y0, tl.x1, tl.y1 = -2 ** 62, -2 ** 62, 2 ** 62, 2 ** 62
            else:
                tl.x0, tl.y0, tl.x1, tl.y1 = (i64(off) for _ in range(4))
            tl.src = int(rng.integers(-1, B + 1)) if rng.integers(0, 4) else i32()
            tl.reserved = i32()
        for k in range(6):
            e.c[k] = i64(off if k % 3 == 2 else step)
        e.xc, e.yc = i64(off), i64(off)
        e.gain = i32() if wild else int(rng.integers(30000, 140000))
        e.fill, e.flags, e.reserved = i32(), int(rng.integers(0, 4)) if wild else int(rng.integers(0, 8) == 0), i32()
    return t


@pytest.mark.parametrize("ch", [2, 3])
def test_host_build_adversarial_tables(host_program, tmp_path, ch):
    """Random primary and partner tables, partner indices in and far outside the table, ratios anywhere in int32,
    over a 1 x 2, a 3 x 1000 and a 7 x 5 source: clean under the sanitizers and equal to the restatement."""
    from yolomi._lib import AugMix
    S, n, n_partner = 24, 40, 9
    rng = np.random.default_rng(100 + ch)
    ims = [rng.integers(0, 256, (*hw, ch), dtype=np.uint8) for hw in ((1, 2), (3, 1000), (7, 5))]
    table, partner = _random_entries(rng, n, len(ims)), _random_entries(rng, n_partner, len(ims))
    mix = (AugMix * n)()
    for i, m in enumerate(mix):
        m.ratio = int(rng.integers(-2 ** 31, 2 ** 31)) >> int(rng.integers(0, 32))
        m.partner = [int(rng.integers(0, n_partner)), -1, n_partner, 2 ** 31 - 1, -2 ** 31,
                     int(rng.integers(-2 ** 31, 2 ** 31))][i % 6 if i % 12 < 6 else 0]
    colours = CR.colours_of(n, seed=ch) if ch == 3 else None
    got = MR.run_host(host_program, tmp_path, table, partner, mix, ims, S, colours)
    want = MR.render_mix(table, partner, mix, ims, S, colours)
    for i in range(n):
        assert np.array_equal(got[i], want[i]), (i, mix[i].ratio, mix[i].partner, int((got[i] != want[i]).sum()))
    mixed = [0 <= m.partner < n_partner for m in mix]
    assert sum(mixed) >= n // 2 and not all(mixed)
    assert len({int(x) for x in np.unique(want)}) > 32     # not all fill: the random maps reach the sources
    # no partner table at all: every index is outside it, and a null table is never read
    got0 = MR.run_host(host_program, tmp_path, table, None, mix, ims, S, colours)
    assert np.array_equal(got0, CR.render_c(table, ims, S, colours))


# ---------------------------------------------------------------- the blend rule
@pytest.mark.parametrize("r", MR.RATIOS)
def test_blend_rule_every_pair(host_program, tmp_path, r):
    subprocess.run([str(host_program), "blend", str(r), str(tmp_path / "blend.bin")], check=True, timeout=60)
    got = np.fromfile(tmp_path / "blend.bin", dtype=np.uint8).reshape(256, 256).astype(np.int64)
    a, p = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    v = MR.blend(a, p, r)
    assert np.array_equal(got, v)
    assert np.array_equal(v[a == p], a[a == p])                                # the fixed point
    if r == 65536:
        assert np.array_equal(v, a)
    if r == 0:
        assert np.array_equal(v, p)
    assert (v >= np.minimum(a, p)).all() and (v <= np.maximum(a, p)).all()
    # the real-valued blend truncated: 65536 * (real - v) is the remainder of the division, an exact integer
    rem = a * r + p * (65536 - r) - v * 65536
    assert (rem >= 0).all() and (rem < 65536).all()
    assert (a * r + p * (65536 - r)).max() <= 255 * 65536 < 2 ** 31            # the operands fit in int32


def test_blend_ratio_clamps():
    a, p = np.arange(256)[:, None], np.arange(256)[None, :]
    assert np.array_equal(MR.blend(a, p, -5), MR.blend(a, p, 0))
    assert np.array_equal(MR.blend(a, p, 70000), MR.blend(a, p, 65536))
    assert np.array_equal(MR.blend(a, p, -2 ** 31), MR.blend(a, p, 0))


# ---------------------------------------------------------------- draws
OLD_KEYS = ("mosaic", "cx", "cy", "partners", "angle", "scale", "shear_x", "shear_y", "tx", "ty", "fliplr", "flipud",
            "gain", "hue", "sat")
GEOMETRY = ("mosaic", "cx", "cy", "partners", "angle", "scale", "shear_x", "shear_y", "tx", "ty")


def test_draw_existing_keys_unchanged_by_mixup():
    from datasets.augment import AugmentHyp, BatchAugment
    hyp = AugmentHyp(degrees=5.0, shear=2.0, hsv_h=0.015, hsv_s=0.7)
    assert hyp.mixup == 0.0
    for seed, rank, epoch, step in ((0, 0, 1, 0), (5, 1, 3, 17), (9, 0, 2, 4)):
        base = BatchAugment(hyp, seed, rank).draw(6, epoch, step)
        mixd = BatchAugment(dataclasses.replace(hyp, mixup=0.7), seed, rank).draw(6, epoch, step)
        for k in OLD_KEYS:
            assert np.array_equal(base[k], mixd[k]), k
        assert not base["mix"].any()
        again = BatchAugment(dataclasses.replace(hyp, mixup=0.7), seed, rank).draw(6, epoch, step)
        assert all(np.array_equal(mixd[k], again[k]) for k in mixd)            # two calls agree
        other = BatchAugment(dataclasses.replace(hyp, mixup=0.7), seed, rank + 1).draw(6, epoch, step)
        assert not np.array_equal(mixd["mix_ratio"], other["mix_ratio"])       # ranks differ
        assert not np.array_equal(mixd["mix_tx"], other["mix_tx"])
        # a complete second geometry, independent of the first
        for g in GEOMETRY:
            assert mixd["mix_" + g].shape == mixd[g].shape and mixd["mix_" + g].dtype == mixd[g].dtype, g
        assert not np.array_equal(mixd["mix_tx"], mixd["tx"]) and not np.array_equal(mixd["mix_cx"], mixd["cx"])
        assert mixd["mix_src"].shape == (6,) and ((0 <= mixd["mix_src"]) & (mixd["mix_src"] < 6)).all()
        assert (np.abs(mixd["mix_angle"]) <= 5.0).all() and (np.abs(mixd["mix_tx"] - 0.5) <= 0.1).all()
    # the draws the trainer has made since hue and saturation exist, pinned: seed 1, rank 0, epoch 1, step 0
    from datasets.augment import step_seed
    g = torch.Generator().manual_seed(step_seed(1, 0, 1, 0))
    u = torch.rand(3, 11, generator=g, dtype=torch.float64).numpy()
    partners = torch.randint(0, 3, (3, 3), generator=g).numpy()
    gain = 1.0 + (2.0 * torch.rand(3, generator=g, dtype=torch.float64).numpy() - 1.0) * 0.4
    hs = 2.0 * torch.rand(3, 2, generator=g, dtype=torch.float64).numpy() - 1.0
    p = BatchAugment(AugmentHyp(hsv_h=0.5, hsv_s=0.5, mixup=0.3), seed=1).draw(3, 1, 0)
    assert np.array_equal(p["cx"], u[:, 1]) and np.array_equal(p["partners"], partners)
    assert np.array_equal(p["gain"], gain) and np.array_equal(p["hue"], hs[:, 0] * 0.5)


def test_draw_ratio_is_beta_32_32_and_share_is_mixup():
    """20 000 ratios against Beta(32, 32): mean 1/2 and variance 1/260 within 5 standard errors, the standard errors
    from the distribution's own moments E[X^k] = prod_{j<k} (a + j) / (2a + j)."""
    from datasets.augment import AugmentHyp, BatchAugment
    n, a, prob = 20000, 32.0, 0.15
    p = BatchAugment(AugmentHyp(mixup=prob), seed=3).draw(n, 1, 0)
    r = p["mix_ratio"]
    assert r.shape == (n,) and (r > 0).all() and (r < 1).all()
    raw = [np.prod([(a + j) / (2 * a + j) for j in range(k)]) for k in range(5)]           # E[X^0..4]
    mean = raw[1]
    var = raw[2] - mean ** 2
    mu4 = raw[4] - 4 * mean * raw[3] + 6 * mean ** 2 * raw[2] - 3 * mean ** 4
    assert abs(mean - 0.5) < 1e-15 and abs(var - 1.0 / 260.0) < 1e-15
    se_mean = np.sqrt(var / n)
    se_var = np.sqrt((mu4 - var ** 2) / n)                 # variance of the sample variance, to first order in 1 / n
    print(f"mean {r.mean():.5f} (se {se_mean:.5f}), variance {r.var(ddof=1):.6f} vs {var:.6f} (se {se_var:.6f})")
    assert abs(r.mean() - mean) <= 5 * se_mean
    assert abs(r.var(ddof=1) - var) <= 5 * se_var
    share = p["mix"].mean()
    se_share = np.sqrt(prob * (1 - prob) / n)
    print(f"mixed share {share:.4f} vs {prob} (se {se_share:.4f})")
    assert abs(share - prob) <= 5 * se_share
    assert BatchAugment(AugmentHyp(mixup=1.0), seed=3).draw(64, 1, 0)["mix"].all()


def test_is_off_counts_mixup():
    from datasets.augment import AugmentHyp
    off = dict(mosaic=0, degrees=0, translate=0, scale=0, shear=0, fliplr=0, flipud=0, gain=0)
    assert AugmentHyp(**off).is_off() and not AugmentHyp(**off, mixup=0.1).is_off()


# ---------------------------------------------------------------- plan
BOXES = [[[0.1, 0.2, 0.4, 0.5], [0.6, 0.6, 0.9, 0.95]], [[0.25, 0.25, 0.75, 0.5]], [], [[0.0, 0.0, 1.0, 1.0]],
         [[0.3, 0.1, 0.8, 0.7], [0.05, 0.5, 0.5, 0.9], [0.45, 0.45, 0.6, 0.6]]]
SIZES5 = [(48, 64), (70, 51), (64, 64), (10, 200), (33, 90)]


def _host_batch(S=64):
    from datasets.crater import pack_images
    rng = np.random.default_rng(11)
    b = pack_images([torch.from_numpy(rng.integers(0, 256, hw, dtype=np.uint8)).unsqueeze(0) for hw in SIZES5], S)
    b.update({"batch_idx": torch.cat([torch.full((len(x),), i, dtype=torch.long) for i, x in enumerate(BOXES)]),
              "bboxes": torch.cat([torch.tensor(x, dtype=torch.float32).reshape(-1, 4) for x in BOXES]),
              "cls": (torch.arange(sum(len(x) for x in BOXES)) % 5).reshape(-1, 1)})
    return b


def _rows_of_sample(batch, S, src, g, lr, ud):
    """The box path of one sample written out from the module's public pieces -> (classes, normalised xyxy)."""
    from datasets import augment as A
    bidx = batch["batch_idx"].numpy()
    boxes, cls = batch["bboxes"].numpy().astype(np.float64), batch["cls"].numpy()
    mosaic = bool(g["mosaic"])
    M = A.affine_matrix(S, 2 * S if mosaic else S, g["angle"], g["scale"], g["shear_x"], g["shear_y"], g["tx"], g["ty"])
    if mosaic:
        xc, yc = int(S / 2 + g["cx"] * S), int(S / 2 + g["cy"] * S)
        srcs = [src, *(int(b) for b in g["partners"])]
        canvas = np.concatenate([np.clip(boxes[bidx == b] * S + np.array([ox, oy, ox, oy], np.float64), 0, 2 * S)
                                 for (ox, oy), b in zip(A.mosaic_origins(xc, yc, S), srcs)])
        c = np.concatenate([cls[bidx == b] for b in srcs])
    else:
        canvas, c = boxes[bidx == src] * S, cls[bidx == src]
    out, keep = A.transform_boxes(canvas, M, S, lr, ud)
    return c[keep], out


@pytest.mark.parametrize("mosaic", [0.0, 1.0])
def test_plan_rows_are_primary_then_partner_under_the_shared_flip(mosaic):
    from datasets.augment import AugmentHyp, BatchAugment
    from datasets.crater import max_gt_count
    S, B = 64, len(SIZES5)
    batch = _host_batch(S)
    hyp = AugmentHyp(mosaic=mosaic, degrees=8.0, shear=2.0, flipud=0.5, mixup=1.0)
    flips = set()
    for step in range(4):
        aug = BatchAugment(hyp, seed=21)
        table, bi, cl, bb, max_gt, partner, mix = aug.plan_mix(batch, 1, step)
        five = aug.plan(batch, 1, step)
        assert bytes(five[0]) == bytes(table) and all(torch.equal(x, y) for x, y in zip(five[1:4], (bi, cl, bb)))
        assert five[4] == max_gt and len(five) == 5
        base = BatchAugment(dataclasses.replace(hyp, mixup=0.0), seed=21).plan(batch, 1, step)
        assert bytes(base[0]) == bytes(table)              # the primary table does not know about the partner
        p = aug.draw(B, 1, step)
        assert len(partner) == B and [m.partner for m in mix] == list(range(B))
        assert [m.ratio for m in mix] == [int(np.floor(r * 65536 + 0.5)) for r in p["mix_ratio"]]
        assert all(e.gain == 65536 for e in partner)       # there is no second gain
        for i in range(B):
            lr, ud = bool(p["fliplr"][i]), bool(p["flipud"][i])
            flips.add((lr, ud))
            c1, b1 = _rows_of_sample(batch, S, i, {k: p[k][i] for k in GEOMETRY}, lr, ud)
            c2, b2 = _rows_of_sample(batch, S, int(p["mix_src"][i]), {k: p["mix_" + k][i] for k in GEOMETRY}, lr, ud)
            rows = (bi == i).nonzero().reshape(-1)
            assert len(rows) == len(b1) + len(b2), (i, len(rows), len(b1), len(b2))
            want = torch.from_numpy(np.concatenate([b1, b2])).float().clamp_(0.0, 1.0)
            assert torch.equal(bb[rows], want), i
            assert np.array_equal(cl[rows].numpy().reshape(-1), np.concatenate([c1, c2]).reshape(-1)), i
            # the unmixed plan's rows of image i are the first part
            assert torch.equal(base[3][base[1] == i], bb[rows][:len(b1)])
        assert torch.equal(bi, torch.sort(bi, stable=True)[0])
        assert max_gt == max_gt_count(bi) and len(bi) > len(base[1])           # from the concatenation
        assert max_gt >= int(torch.bincount(bi, minlength=B).max())
    assert len(flips) > 1


def test_plan_partner_flip_is_the_primarys():
    """No geometry but the flip: a flipped image's partner entry is its source under the same flip."""
    from datasets.augment import AugmentHyp, BatchAugment, flip_matrix, plain_entry
    off = dict(mosaic=0.0, degrees=0.0, translate=0.0, scale=0.0, shear=0.0, flipud=0.0, gain=0.0)
    S = 64
    batch = _host_batch(S)
    aug = BatchAugment(AugmentHyp(**off, fliplr=0.5, mixup=1.0), seed=2)
    seen = set()
    for step in range(4):
        table, bi, cl, bb, max_gt, partner, mix = aug.plan_mix(batch, 1, step)
        p = aug.draw(len(SIZES5), 1, step)
        for i in range(len(SIZES5)):
            src = int(p["mix_src"][i])
            seen.add(bool(p["fliplr"][i]))
            inv = flip_matrix(S, True, False) if p["fliplr"][i] else None
            assert bytes(partner[i]) == bytes(plain_entry(src, *SIZES5[src], S, inv, 1.0, 114)), i
            assert bool(partner[i].flags & 1) == (not p["fliplr"][i])          # unflipped: the stretch-flagged entry
    assert seen == {True, False}


def test_plan_closing_and_mixup_zero():
    from datasets.augment import AugmentHyp, BatchAugment
    S = 64
    batch = _host_batch(S)
    aug = BatchAugment(AugmentHyp(mixup=1.0), seed=4, no_mosaic_from=5)
    assert aug.draw(8, 4, 0)["mix"].all() and not aug.draw(8, 5, 0)["mix"].any()
    assert not aug.draw(8, 5, 0)["mix_mosaic"].any()
    open_, closed = aug.plan_mix(batch, 4, 0), aug.plan_mix(batch, 5, 0)
    assert open_[5] is not None and closed[5] is None and closed[6] is None
    want = BatchAugment(AugmentHyp(), seed=4, no_mosaic_from=5).plan(batch, 5, 0)
    assert bytes(closed[0]) == bytes(want[0]) and torch.equal(closed[3], want[3])
    # mixup == 0: the five-tuple and the table bytes of an augmenter that has never heard of MixUp
    for step in range(3):
        z = BatchAugment(AugmentHyp(degrees=5.0, mixup=0.0), seed=9)
        t, bi, cl, bb, mg = z.plan(batch, 2, step)
        full = z.plan_mix(batch, 2, step)
        assert full[5] is None and full[6] is None and bytes(full[0]) == bytes(t)
        assert ctypes.sizeof(t) == len(SIZES5) * 432
    # some images mixed, some not: the partner table is compact and the records of the others say -1
    part = BatchAugment(AugmentHyp(mixup=0.5), seed=6)
    for step in range(6):
        *_, partner, mix = part.plan_mix(batch, 1, step)
        drawn = part.draw(len(SIZES5), 1, step)["mix"]
        if partner is None:
            assert not drawn.any()
            continue
        assert len(partner) == int(drawn.sum()) and len(mix) == len(SIZES5)
        assert [m.partner for m in mix] == [int(drawn[:i].sum()) if drawn[i] else -1 for i in range(len(SIZES5))]
        assert all(m.ratio == 65536 for m, d in zip(mix, drawn) if not d)


def test_plan_letterboxed_batch():
    """A letterboxed batch: the partner goes through the same letterboxed tiles as the primary."""
    from datasets import collate_fn_cuda
    from datasets.augment import AugmentHyp, BatchAugment, plain_entry
    S, hw = 64, [(24, 64), (64, 40), (64, 64), (10, 50)]
    rng = np.random.default_rng(12)
    items = [(torch.from_numpy(rng.integers(0, 256, h_w, dtype=np.uint8)).unsqueeze(0),
              torch.tensor([[0.5, 0.5, 0.5, 0.25]]), torch.tensor([i % 3]), i) for i, h_w in enumerate(hw)]
    batch = collate_fn_cuda(items, img_size=S, letterbox=True)
    off = dict(mosaic=0.0, degrees=0.0, translate=0.0, scale=0.0, shear=0.0, fliplr=0.0, flipud=0.0, gain=0.0)
    aug = BatchAugment(AugmentHyp(**off, mixup=1.0), seed=8)
    table, bi, cl, bb, max_gt, partner, mix = aug.plan_mix(batch, 1, 0)
    p = aug.draw(4, 1, 0)
    geo = batch["img_lb"].numpy()
    for i in range(4):
        src = int(p["mix_src"][i])
        assert bytes(partner[i]) == bytes(plain_entry(src, *hw[src], S, None, 1.0, 114, lb=geo[src].tolist())), i
        assert partner[i].flags == 0
        rows = (bi == i).nonzero().reshape(-1)
        assert len(rows) == 2 and torch.equal(bb[rows[1]], batch["bboxes"][batch["batch_idx"] == src][0])
    assert max_gt >= 2
    # with the mosaic on, the partner's tiles are letterboxed ones as well: pads show the fill in its rendering
    aug = BatchAugment(AugmentHyp(mixup=1.0), seed=8)
    table, *_, partner, mix = aug.plan_mix(batch, 1, 0)
    ims = [a[0].numpy() for a, *_ in items]
    plain = {k: v for k, v in batch.items() if k != "img_lb"}
    stretched = BatchAugment(AugmentHyp(mixup=1.0), seed=8).plan_mix(plain, 1, 0)[5]
    assert bytes(stretched) != bytes(partner)
    assert (AR.render(partner, ims, S) == 114).sum() > (AR.render(stretched, ims, S) == 114).sum()


# ---------------------------------------------------------------- flag and layout
def test_trainer_flag_and_layout(capsys):
    import train_yolo11_cuda as T
    from yolomi._lib import AugEntry, AugMix, SIGNATURES
    ap = T.build_parser()
    assert ap.parse_args([]).mixup == 0.0
    assert ap.parse_args(["--augment", "--mixup", "0.15"]).mixup == 0.15
    with pytest.raises(SystemExit):
        ap.parse_args(["--mixup", "often"])
    capsys.readouterr()
    helps = {a.dest: a.help for a in ap._actions}
    assert "--augment" in helps["mixup"] and "MixUp" in helps["close_mosaic"]
    assert ctypes.sizeof(AugMix) == 8 and AugMix.ratio.offset == 0 and AugMix.partner.offset == 4
    assert ctypes.sizeof(AugEntry) == 432                                      # unchanged
    assert len(SIGNATURES["ym_augment_mix_u8c"][1]) == 12
    hdr = (ROOT / "include" / "yolomi_augment.h").read_text()
    assert "static_assert(sizeof(ym_aug_mix) == 8" in hdr
    import datasets.augment as A
    assert callable(A.augment_mix_batch)
