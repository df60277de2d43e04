"""MixUp in the augmentation launch (ym_augment_mix_u8c): bit for bit equal to the numpy restatement
(tests/augment_mix_ref.py) over the case list the sanitized host build is held to, for 1-4 planes, on and off the
16-byte grid; a batch without a valid partner bit for bit equal to ym_augment_u8c and ym_augment_u8; the argument
checks; BatchAugment with `mixup` and one epoch of the trainer with --mixup."""
import ctypes
import dataclasses
import functools
import json
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment_colour_ref as CR
import augment_mix_ref as MR
import augment_ref as AR
from conftest import PKG

pytestmark = pytest.mark.gpu

SIZES = [32, 31]                                           # 31: S * S is odd, the per-element tail
GUARD = 8                                                  # floats kept at -1 on either side of `out`


def _dev(ims):
    buf, meta = AR.pack(ims)
    return torch.from_numpy(buf).cuda(), torch.from_numpy(meta).cuda()


def _bytes_dev(table):
    from datasets.augment import table_bytes
    return None if table is None else table_bytes(table).cuda()


def _mix_launch(table, partner, mix, ims, S, colours=None, offset=False):
    """One ym_augment_mix_u8c launch over pixel-interleaved `ims` -> (B, ch, S, S) fp32 on the host.  `out` sits
    between guard words, 16-byte aligned or (`offset`) 4 bytes past that; the guards are checked here."""
    from yolomi._lib import call, stream_ptr
    ch, B = ims[0].shape[2], len(ims)
    assert len(table) == B and len(mix) == B
    u8, meta = _dev(ims)
    n = B * ch * S * S
    lead = GUARD + (1 if offset else 0)
    flat = torch.full((lead + n + GUARD,), -1.0, dtype=torch.float32, device="cuda")
    out = flat[lead:lead + n]
    assert out.data_ptr() % 16 == (4 if offset else 0)
    tb, pb, mb = _bytes_dev(table), _bytes_dev(partner), _bytes_dev(mix)
    col = None if colours is None else _bytes_dev(CR.colour_table(colours))
    call("ym_augment_mix_u8c", u8.data_ptr(), meta.data_ptr(), tb.data_ptr(), None if pb is None else pb.data_ptr(),
         0 if partner is None else len(partner), mb.data_ptr(), None if col is None else col.data_ptr(), B, ch, S,
         out.data_ptr(), stream_ptr(u8.device))
    host = flat.cpu().numpy()
    assert (host[:lead] == -1.0).all() and (host[lead + n:] == -1.0).all(), "guard words overwritten"
    return host[lead:lead + n].reshape(B, ch, S, S)


def _plain_launch(table, ims, S, colours=None):
    from yolomi._lib import call, stream_ptr
    ch, B = ims[0].shape[2], len(ims)
    u8, meta = _dev(ims)
    out = torch.full((B, ch, S, S), -1.0, dtype=torch.float32, device="cuda")
    col = None if colours is None else _bytes_dev(CR.colour_table(colours))
    call("ym_augment_u8c", u8.data_ptr(), meta.data_ptr(), _bytes_dev(table).data_ptr(),
         None if col is None else col.data_ptr(), B, ch, S, out.data_ptr(), stream_ptr(u8.device))
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reference(S, ch, coloured):
    """The restatement of every chunk of the case list, computed once and shared: [(names, n, uint8 (B, ch, S, S))]."""
    ims = CR.sources(S, ch)
    out = []
    for k, (names, table, partner, mix, n) in enumerate(MR.chunks(S)):
        colours = CR.colours_of(len(table), seed=S + k) if coloured else None
        want = MR.render_mix(table, partner, mix, ims, S, colours)
        want.setflags(write=False)
        out.append((names, n, want))
    return out


def _check_exact(got, want_u8, names):
    """Bit for bit: the floats are v / 255.0f and round back to the restatement's bytes."""
    want = AR.as_float(want_u8)
    for k, name in enumerate(names):
        assert np.array_equal(got[k], want[k]), (name, int((got[k] != want[k]).sum()))
        assert np.array_equal(np.rint(got[k] * 255.0).astype(np.int64), want_u8[k]), name


def test_cases_are_not_degenerate():
    """On the restatement, before any launch is judged by it."""
    for S in SIZES:
        MR.check_cases_not_degenerate(S, 3)
    names = [c[0] for c in MR.cases(32)]
    assert len(set(names)) == len(names) and {"partner_minus_one", "partner_equals_n", "ratio_negative",
                                              "ratio_above_one", "mosaic_x_mosaic"} <= set(names)
    # the two mosaics of mosaic_x_mosaic have different centres, and both seams cross every wave of 256 pixels
    _, e, pe, _, _ = MR.cases(32)[names.index("mosaic_x_mosaic")]
    assert (e.xc, e.yc) != (pe.xc, pe.yc)
    for S in SIZES:
        _, e, pe, _, _ = MR.cases(S)[names.index("mosaic_x_mosaic")]
        y, x = np.meshgrid(np.arange(S, dtype=np.int64), np.arange(S, dtype=np.int64), indexing="ij")
        for en in (e, pe):
            right, low = AR._map(en.c[0:3], x, y) >= en.xc, AR._map(en.c[3:6], x, y) >= en.yc
            slot = (right.astype(int) + 2 * low.astype(int)).reshape(-1)
            for lo in range(0, S * S, 256):
                assert len(set(slot[lo:lo + 256].tolist())) > 1, (S, lo)


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("ch", [1, 2, 3, 4])
def test_kernel_equals_restatement(S, ch, offset):
    ims = CR.sources(S, ch)
    ref = _reference(S, ch, False)
    for (names, table, partner, mix, n), (_, _, want) in zip(MR.chunks(S), ref):
        _check_exact(_mix_launch(table, partner, mix, ims, S, offset=offset)[:n], want[:n], names)


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("S", SIZES)
def test_kernel_equals_restatement_with_colour(S, offset):
    ims = CR.sources(S, 3)
    ref = _reference(S, 3, True)
    for k, ((names, table, partner, mix, n), (_, _, want)) in enumerate(zip(MR.chunks(S), ref)):
        colours = CR.colours_of(len(table), seed=S + k)
        _check_exact(_mix_launch(table, partner, mix, ims, S, colours, offset=offset)[:n], want[:n], names)
    assert any(not np.array_equal(a[2], b[2]) for a, b in zip(ref, _reference(S, 3, False)))


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("ch", [1, 3])
def test_batch_without_a_valid_partner_equals_the_unmixed_launch(S, ch):
    from datasets.augment import augment_batch
    from yolomi._lib import AugMix
    ims = CR.sources(S, ch)
    B = len(ims)
    _, entries = zip(*CR.cases(S))
    junk = CR.table_of(list(entries[-2:]))                 # a partner table that must not be looked at
    for lo in range(0, len(entries) - B + 1, B):
        table = CR.table_of(list(entries[lo:lo + B]))
        for colours in ((None, CR.colours_of(B, seed=lo)) if ch == 3 else (None,)):
            want = _plain_launch(table, ims, S, colours)
            for partner, idx in ((None, [-1] * B), (junk, [-1, len(junk), 2 ** 31 - 1, -2 ** 31]),
                                 (None, [0, 1, 2, 3])):
                mix = (AugMix * B)()
                for i in range(B):
                    mix[i].ratio, mix[i].partner = 12345 * i, idx[i]
                got = _mix_launch(table, partner, mix, ims, S, colours, offset=bool((lo // B) % 2))
                assert np.array_equal(got, want), (lo, idx)
        if ch == 1:                                        # and one plane is the single-plane entry point
            u8, meta = _dev(ims)
            one = augment_batch(u8, meta, _bytes_dev(table), S).cpu().numpy()
            assert np.array_equal(want, one)


def test_argument_checks():
    from yolomi._lib import AugMix, lib, stream_ptr
    S, B = 32, 4
    L = lib()
    ims = CR.sources(S, 3)
    u8, meta = _dev(ims)
    names, table, partner, mix, n = next(iter(MR.chunks(S)))
    tb, pb, mb = _bytes_dev(table), _bytes_dev(partner), _bytes_dev(mix)
    col = _bytes_dev(CR.colour_table(CR.colours_of(B)))
    out = torch.full((B, 4, S, S), -1.0, dtype=torch.float32, device="cuda")
    st = stream_ptr(u8.device)
    args = [u8.data_ptr(), meta.data_ptr(), tb.data_ptr(), pb.data_ptr(), len(partner), mb.data_ptr(), None, B, 3, S,
            out.data_ptr(), st]

    def bad(**kw):
        a = list(args)
        for k, v in kw.items():
            a[{"src": 0, "meta": 1, "table": 2, "partner": 3, "n_partner": 4, "mix": 5, "colour": 6, "batch": 7,
               "ch": 8, "size": 9, "out": 10}[k]] = v
        return L.ym_augment_mix_u8c(*a)

    for ch in (0, 5, -1):
        assert bad(ch=ch) == -1                            # YM_ERR_ARG
    for ch in (1, 2, 4):                                   # a colour table needs three planes
        assert bad(ch=ch, colour=col.data_ptr()) == -1
        assert b"ch" in L.ym_last_error()
    for kw in (dict(src=None), dict(meta=None), dict(table=None), dict(mix=None), dict(out=None), dict(batch=-1),
               dict(size=0), dict(size=32769), dict(n_partner=-1), dict(partner=None)):
        assert bad(**kw) == -1, kw
    assert b"partner" in L.ym_last_error()
    torch.cuda.synchronize()
    assert (out == -1.0).all()                             # nothing was launched
    assert bad(batch=0) == 0 and bad(partner=None, n_partner=0) == 0
    torch.cuda.synchronize()
    flat, n = out.view(-1), B * 3 * S * S                  # three planes per image, back to back
    assert (flat[:n] >= 0.0).all() and (flat[n:] == -1.0).all()
    assert ctypes.sizeof(AugMix) == 8


# ---------------------------------------------------------------- BatchAugment and the trainer
BOXES = [[[0.1, 0.2, 0.4, 0.5], [0.6, 0.6, 0.9, 0.95]], [[0.25, 0.25, 0.75, 0.5]], [], [[0.0, 0.0, 1.0, 1.0]]]
HW = [(48, 64), (70, 51), (64, 64), (10, 200)]


def _host_batch(ch, S):
    from datasets.crater import pack_images
    rng = np.random.default_rng(11)
    ims = [rng.integers(0, 256, (*hw, 3), dtype=np.uint8) for hw in HW]
    if ch == 1:
        b = pack_images([torch.from_numpy(a[..., 0].copy()).unsqueeze(0) for a in ims], S)
        ims = [a[..., :1] for a in ims]
    else:
        b = pack_images([torch.from_numpy(a) for a in ims], S, channels=3)
    b.update({"batch_idx": torch.cat([torch.full((len(x),), i, dtype=torch.long) for i, x in enumerate(BOXES)]),
              "bboxes": torch.cat([torch.tensor(x, dtype=torch.float32).reshape(-1, 4) for x in BOXES]),
              "cls": (torch.arange(sum(len(x) for x in BOXES)) % 3).reshape(-1, 1)})
    return b, ims


@pytest.mark.parametrize("ch", [1, 3])
def test_batch_augment_with_mixup(ch):
    from datasets import AugmentHyp, BatchAugment
    S = 64
    hyp = AugmentHyp(degrees=8.0, shear=2.0, flipud=0.3, hsv_h=0.015, hsv_s=0.7, mixup=1.0)
    batch, ims = _host_batch(ch, S)
    dev = torch.device("cuda")
    for step in range(2):
        aug = BatchAugment(hyp, seed=11)
        d = aug(batch, dev, 1, step)
        assert set(d) == {"img", "batch_idx", "cls", "bboxes", "max_gt"}
        assert d["img"].shape == (4, ch, S, S) and d["img"].dtype == torch.float32 and d["img"].is_cuda
        table, bi, cl, bb, max_gt, partner, mix = aug.plan_mix(batch, 1, step)
        assert len(partner) == 4 and all(0 < m.ratio < 65536 for m in mix)
        col = aug.colours(4, 1, step) if ch == 3 else None
        pairs = None if col is None else [(c.hue, c.sat) for c in col]
        want = MR.render_mix(table, partner, mix, ims, S, pairs)
        assert np.array_equal(d["img"].cpu().numpy(), AR.as_float(want))
        assert not np.array_equal(want, CR.render_c(table, ims, S, pairs))
        five = aug.plan(batch, 1, step)                    # the targets are plan()'s
        assert torch.equal(d["batch_idx"].cpu(), five[1]) and torch.equal(d["cls"].cpu(), five[2])
        assert torch.equal(d["bboxes"].cpu(), five[3]) and d["max_gt"] == five[4]
        # mixup = 0: the call this augmenter has always made, bit for bit
        zero = BatchAugment(dataclasses.replace(hyp, mixup=0.0), seed=11)
        z = zero(batch, dev, 1, step)
        t0 = zero.plan(batch, 1, step)[0]
        assert bytes(t0) == bytes(table)
        assert np.array_equal(z["img"].cpu().numpy(), AR.as_float(CR.render_c(t0, ims, S, pairs)))
        assert len(z["batch_idx"]) < len(d["batch_idx"])
    # mosaic closing closes MixUp: the closed epoch's batch is the unmixed augmenter's
    closed = BatchAugment(hyp, seed=11, no_mosaic_from=2)(batch, dev, 2, 0)
    plain = BatchAugment(dataclasses.replace(hyp, mixup=0.0), seed=11, no_mosaic_from=2)(batch, dev, 2, 0)
    assert torch.equal(closed["img"], plain["img"]) and torch.equal(closed["bboxes"], plain["bboxes"])


def _write_yolo(root, n=4):
    from PIL import Image
    rng = np.random.default_rng(31)
    (root / "images").mkdir()
    (root / "labels").mkdir()
    for i in range(n):
        h, w = int(rng.integers(40, 90)), int(rng.integers(40, 90))
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(root / "images" / f"im{i}.png")
        rows = [f"{int(rng.integers(0, 3))} {rng.uniform(0.3, 0.7):.4f} {rng.uniform(0.3, 0.7):.4f} "
                f"{rng.uniform(0.2, 0.5):.4f} {rng.uniform(0.2, 0.5):.4f}" for _ in range(int(rng.integers(1, 4)))]
        (root / "labels" / f"im{i}.txt").write_text("\n".join(rows) + "\n")


def test_trainer_epoch_with_mixup(tmp_path):
    """One epoch of the trainer as a user starts it: --augment --mixup 0.5 on 3-plane YOLO-txt data.  The mosaic (and
    with it MixUp) stays open in that epoch: --close-mosaic 0."""
    import re
    data = tmp_path / "data"
    data.mkdir()
    _write_yolo(data, n=8)
    cmd = [sys.executable, str(PKG / "train_yolo11_cuda.py"), "--data", str(data), "--data-format", "yolo", "--ch", "3",
           "--nc", "3", "--augment", "--mixup", "0.5", "--close-mosaic", "0", "--imgsz", "64", "--batch", "4",
           "--scale", "n", "--epochs", "1", "--workers", "0", "--val-split", "0.25", "--val-conf", "0.001",
           "--save-dir", str(tmp_path / "run"), "--resume", str(tmp_path / "none.pt")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"Train - Loss: (\S+), Box: (\S+), Cls: (\S+), DFL: (\S+)", r.stdout)
    assert "Epoch 1/1" in r.stdout and m, r.stdout[-2000:]
    losses = [float(x.rstrip(",")) for x in m.groups()]
    print(json.dumps(losses))
    assert all(np.isfinite(v) for v in losses) and losses[0] > 0, losses
    # the epoch did mix: its first batch (four of the six training images, --aug-seed 0) draws partners
    from datasets import AugmentHyp, BatchAugment
    assert BatchAugment(AugmentHyp(mixup=0.5), seed=0, no_mosaic_from=2).draw(4, 1, 0)["mix"].any()
