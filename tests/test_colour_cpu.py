"""Colour data path without a GPU: the 1-4 plane per-pixel functions (include/yolomi_augment.h) built for the host
with the address and undefined-behaviour sanitizers as a stand-alone program and held byte for byte to the numpy
restatement (tests/augment_colour_ref.py) over the GPU test's case list; the integer hue / saturation rule over all
2^24 colours and against the real-valued hexcone; packing and collating interleaved images; YoloTxtDataset; the
draws that existed before hue and saturation; the trainer's flags."""
import ctypes
import functools
import shutil
import subprocess

import numpy as np
import pytest
import torch

import augment_colour_ref as CR
import augment_ref as AR
from conftest import ROOT


# ---------------------------------------------------------------- the shared header, built for the host
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("colourhost") / "augment_colour_host"
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "augment_colour_host.cpp"), "-o", str(exe)], check=True)
    return exe


@pytest.mark.parametrize("S", [32, 31])
@pytest.mark.parametrize("ch", [1, 2, 3, 4])
def test_host_build_equals_restatement(host_program, tmp_path, S, ch):
    ims = CR.sources(S, ch)
    names, entries = zip(*CR.cases(S))
    table = CR.table_of(entries)
    got = CR.run_host(host_program, tmp_path, table, ims, S)
    want = CR.render_c(table, ims, S)
    for i, name in enumerate(names):
        assert np.array_equal(got[i], want[i]), (name, int((got[i] != want[i]).sum()))
    if ch == 1:                                            # one plane is the single-plane function
        assert np.array_equal(want[:, 0], AR.render(table, [a[..., 0] for a in ims], S))
    # the cases are not degenerate: fill and image both show, the out-of-range sources show fill only
    k = names.index("mosaic_split")
    assert (want[k] != want[k][:, :1, :1]).any()
    assert (want[names.index("stretch_src_out_of_range")] == CR.FILL).all()
    assert (want[names.index("mosaic_empty_slot")] == int(CR.FILL * 1.2)).any()


@pytest.mark.parametrize("S", [32, 31])
def test_host_build_equals_restatement_with_colour(host_program, tmp_path, S):
    ims = CR.sources(S, 3)
    names, entries = zip(*CR.cases(S))
    table = CR.table_of(entries)
    colours = CR.colours_of(len(entries), seed=S)
    got = CR.run_host(host_program, tmp_path, table, ims, S, colours)
    want = CR.render_c(table, ims, S, colours)
    for i, name in enumerate(names):
        assert np.array_equal(got[i], want[i]), (name, colours[i], int((got[i] != want[i]).sum()))
    assert not np.array_equal(want[1:], CR.render_c(table, ims, S)[1:])        # the colour entries do something


def test_grey_image_in_three_planes_equals_one_plane(host_program, tmp_path):
    """r = g = b has no chroma: any hue / sat leaves it, and every plane is the 1-plane rendering."""
    S = 32
    grey = [np.repeat(a, 3, axis=2) for a in CR.sources(S, 1)]
    names, entries = zip(*CR.cases(S))
    table = CR.table_of(entries)
    got = CR.run_host(host_program, tmp_path, table, grey, S, CR.colours_of(len(entries), seed=3))
    one = AR.render(table, [a[..., 0] for a in grey], S)
    for c in range(3):
        assert np.array_equal(got[:, c], one), c


# ---------------------------------------------------------------- hue and saturation
@pytest.fixture(scope="module")
def all_colours():
    i = np.arange(1 << 24, dtype=np.int32)
    return np.stack([i >> 16, (i >> 8) & 255, i & 255], -1)


def _host_hsv(exe, tmp_path, hue, sat):
    subprocess.run([str(exe), "hsv", str(hue), str(sat), str(tmp_path / "hsv.bin")], check=True, timeout=300)
    return np.fromfile(tmp_path / "hsv.bin", dtype=np.uint8).reshape(1 << 24, 3)


def test_hue_sat_identity_all_colours(host_program, tmp_path, all_colours):
    assert np.array_equal(_host_hsv(host_program, tmp_path, 0, 65536), all_colours)
    assert np.array_equal(CR.hue_sat(all_colours, 0, 65536), all_colours)


@pytest.mark.parametrize("hue,sat", [(21845, 98304), (60000, 1 << 17), (-3000, 30000)])
def test_hue_sat_all_colours_value_kept_and_in_range(host_program, tmp_path, all_colours, hue, sat):
    got = _host_hsv(host_program, tmp_path, hue, sat)      # the program itself fails on a value outside 0..255
    want = CR.hue_sat(all_colours, hue, sat)
    assert want.min() >= 0 and want.max() <= 255
    assert np.array_equal(want.max(-1), all_colours.max(-1))                   # V preserved
    assert np.array_equal(got, want)


def test_hue_sat_primaries_and_unit_chroma():
    prim = np.array([[255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255], [255, 0, 255]])
    third = 21845                                          # a third of a turn, rounded: red -> green -> blue
    assert np.array_equal(CR.hue_sat(prim[[0, 2, 4]], third, 65536), prim[[2, 4, 0]])
    assert np.array_equal(CR.hue_sat(prim, 32768, 65536), prim[[3, 4, 5, 0, 1, 2]])          # half a turn
    assert np.array_equal(CR.hue_sat(prim, 12345, 0), np.full((6, 3), 255))    # no saturation: grey at V
    d1 = np.array([[10, 9, 9], [9, 10, 9], [9, 9, 10], [10, 10, 9], [0, 1, 0], [255, 254, 255]])
    for hue in (0, 10922, 21845, 40000, 65535):
        out = CR.hue_sat(d1, hue, 65536)
        assert np.array_equal(out.max(-1), d1.max(-1)) and (out.max(-1) - out.min(-1) <= 1).all()


def test_hue_sat_error_against_float_model():
    """At most 2.5 levels for sat in [0, 2]: 0.5 from the rounded shift scaled by d'/d <= 2, 1 from the truncation
    of d', 0.5 from f'."""
    rng = np.random.default_rng(17)
    rgb = rng.integers(0, 256, (2_000_000, 3))
    worst = 0.0
    for hue, sat in [(0.0, 1.0), (0.015, 1.7), (-0.015, 0.3), (0.25, 2.0), (0.5, 0.0), (0.8125, 1.37), (0.333, 1.999),
                     (0.0701, 0.85)]:
        q_hue, q_sat = int(np.rint(hue * 65536)), int(np.rint(sat * 65536))
        err = np.abs(CR.hue_sat(rgb, q_hue, q_sat) - CR.hue_sat_model(rgb, q_hue / 65536.0, q_sat / 65536.0)).max()
        print(f"hue {hue} sat {sat}: worst error {err:.3f} levels")
        worst = max(worst, float(err))
    assert worst <= 2.5, worst


def test_colour_entry_layout():
    from yolomi._lib import AugColour, AugEntry, AugTile
    assert ctypes.sizeof(AugColour) == 8 and AugColour.hue.offset == 0 and AugColour.sat.offset == 4
    assert ctypes.sizeof(AugTile) == 88 and ctypes.sizeof(AugEntry) == 432      # unchanged
    from datasets.augment import colour_table
    t = colour_table([0.0, -0.25, 1.5, 0.015], [1.0, 3.0, -1.0, 0.3])
    assert [(c.hue, c.sat) for c in t] == [(0, 65536), (49152, 1 << 17), (32768, 0), (983, 19661)]


# ---------------------------------------------------------------- packing and collating
def test_pack_images_channels():
    from datasets.crater import pack_images
    rng = np.random.default_rng(2)
    ims = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((4, 6), (1, 1), (5, 3))]
    p = pack_images([torch.from_numpy(a) for a in ims], 32, channels=3)
    assert p["img_ch"] == 3 and p["img_size"] == 32
    assert p["img_meta"].tolist() == [[0, 4, 6], [72, 1, 1], [75, 5, 3]]       # offsets count h * w * ch bytes
    assert p["img_u8"].numel() == 72 + 3 + 45
    for a, (o, h, w) in zip(ims, p["img_meta"].tolist()):
        assert np.array_equal(p["img_u8"].numpy()[o:o + h * w * 3].reshape(h, w, 3), a)
    buf, meta = AR.pack(ims)                               # the restatement's packing is the same bytes
    assert np.array_equal(buf, p["img_u8"].numpy()) and np.array_equal(meta, p["img_meta"].numpy())
    one = pack_images([torch.from_numpy(a[..., 0].copy()).unsqueeze(0) for a in ims], 32)
    assert "img_ch" not in one and one["img_meta"].tolist() == [[0, 4, 6], [24, 1, 1], [25, 5, 3]]
    with pytest.raises(ValueError):
        pack_images([torch.from_numpy(ims[0])], 32, channels=4)
    with pytest.raises(ValueError):
        pack_images([], 32, channels=5)


def test_collate_channels():
    from datasets import collate_fn_cuda
    rng = np.random.default_rng(3)
    items = []
    for i, (h, w) in enumerate(((8, 6), (5, 9))):
        im = torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        boxes = torch.tensor([[0.5, 0.5, 0.2, 0.4]] * (i + 1), dtype=torch.float32)
        items.append((im, boxes, torch.full((i + 1,), i, dtype=torch.long), i))
    b = collate_fn_cuda(items, img_size=16, channels=3)
    assert b["img_ch"] == 3 and b["img_meta"].tolist() == [[0, 8, 6], [144, 5, 9]]
    assert b["batch_idx"].tolist() == [0, 1, 1] and b["cls"].reshape(-1).tolist() == [0, 1, 1]
    assert torch.allclose(b["bboxes"][0], torch.tensor([0.4, 0.3, 0.6, 0.7]))
    part = functools.partial(collate_fn_cuda, img_size=16, channels=3)
    assert part(items)["img_u8"].equal(b["img_u8"])


# ---------------------------------------------------------------- YoloTxtDataset
def _write_yolo(root):
    from PIL import Image
    rng = np.random.default_rng(4)
    (root / "images" / "sub").mkdir(parents=True)
    (root / "labels" / "sub").mkdir(parents=True)
    arrs = {"a_rgb": rng.integers(0, 256, (12, 20, 3), dtype=np.uint8),
            "b_grey": rng.integers(0, 256, (9, 7), dtype=np.uint8),
            "sub/c_rgba": rng.integers(0, 256, (16, 16, 4), dtype=np.uint8),
            "d_nolabel": rng.integers(0, 256, (5, 5, 3), dtype=np.uint8)}
    for name, a in arrs.items():
        Image.fromarray(a).save(root / "images" / f"{name}.png")
    (root / "labels" / "a_rgb.txt").write_text("2 0.5 0.5 0.25 0.5\n\n0 0.1 0.2 0.05 0.1\n")
    (root / "labels" / "b_grey.txt").write_text("")
    (root / "labels" / "sub" / "c_rgba.txt").write_text("1 0.25 0.75 0.5 0.5")
    return arrs


def test_yolo_txt_dataset(tmp_path):
    from datasets import YoloTxtDataset, collate_fn_cuda
    import datasets
    assert "YoloTxtDataset" in datasets.__all__
    arrs = _write_yolo(tmp_path)
    ds = YoloTxtDataset(tmp_path, img_size=32)
    assert len(ds) == 4 and [s["img_path"].rsplit("/", 1)[-1] for s in ds.samples] == [
        "a_rgb.png", "b_grey.png", "d_nolabel.png", "c_rgba.png"]
    img, boxes, labels, idx = ds[0]
    assert img.dtype == torch.uint8 and img.shape == (12, 20, 3) and np.array_equal(img.numpy(), arrs["a_rgb"])
    assert labels.tolist() == [2, 0] and labels.dtype == torch.long and idx == 0
    assert torch.allclose(boxes, torch.tensor([[0.5, 0.5, 0.25, 0.5], [0.1, 0.2, 0.05, 0.1]]))
    img, boxes, labels, _ = ds[1]                          # an L file as three equal planes; an empty label file
    assert img.shape == (9, 7, 3) and all(np.array_equal(img.numpy()[..., c], arrs["b_grey"]) for c in range(3))
    assert boxes.shape == (0, 4) and labels.shape == (0,) and boxes.dtype == torch.float32
    img, boxes, labels, _ = ds[2]                          # no label file
    assert img.shape == (5, 5, 3) and boxes.shape == (0, 4) and labels.shape == (0,)
    img, boxes, labels, _ = ds[3]                          # RGBA read as RGB drops the alpha plane
    assert np.array_equal(img.numpy(), arrs["sub/c_rgba"][..., :3]) and labels.tolist() == [1]
    b = collate_fn_cuda([ds[i] for i in range(4)], img_size=32, channels=3)
    assert b["img_ch"] == 3 and b["img_meta"][:, 1:].tolist() == [[12, 20], [9, 7], [5, 5], [16, 16]]
    assert b["batch_idx"].tolist() == [0, 0, 3]

    four = YoloTxtDataset(tmp_path, img_size=32, channels=4)
    assert np.array_equal(four[3][0].numpy(), arrs["sub/c_rgba"])
    assert four[0][0].shape == (12, 20, 4) and (four[0][0][..., 3] == 255).all()
    one = YoloTxtDataset(tmp_path, img_size=32, channels=1, cache_images=True)
    from datasets.crater import _gray_u8
    assert one[0][0].shape == (1, 12, 20) and np.array_equal(one[0][0][0].numpy(), _gray_u8(ds.samples[0]["img_path"]))
    assert np.array_equal(one[1][0][0].numpy(), arrs["b_grey"]) and one[0][0] is not None and 0 in one._cache
    with pytest.raises(ValueError):
        YoloTxtDataset(tmp_path, channels=2)
    with pytest.raises(FileNotFoundError):
        YoloTxtDataset(tmp_path / "labels" / "nowhere")


@pytest.mark.parametrize("row", ["0 0.5 0.5 0.2", "x 0.5 0.5 0.2 0.2", "0 0.5 0.5 0.2 1.5", "-1 0.5 0.5 0.2 0.2",
                                 "0 0.5 0.5 0.2 0.2 0.9", "1.5 0.5 0.5 0.2 0.2", "0 0.5 nan 0.2 0.2"])
def test_yolo_txt_malformed_row_names_the_file(tmp_path, row):
    from datasets import YoloTxtDataset
    _write_yolo(tmp_path)
    (tmp_path / "labels" / "a_rgb.txt").write_text("1 0.5 0.5 0.1 0.1\n" + row + "\n")
    ds = YoloTxtDataset(tmp_path, img_size=32)
    with pytest.raises(ValueError, match=r"a_rgb\.txt:2"):
        ds[0]


# ---------------------------------------------------------------- draws, off switch, flags
def test_draw_keys_unchanged_by_hue_and_saturation():
    from datasets.augment import AugmentHyp, BatchAugment
    old_keys = ("mosaic", "cx", "cy", "partners", "angle", "scale", "shear_x", "shear_y", "tx", "ty", "fliplr",
                "flipud", "gain")
    for seed, rank, epoch, step in ((0, 0, 1, 0), (5, 1, 3, 17), (9, 0, 2, 4)):
        base = BatchAugment(AugmentHyp(degrees=5.0, shear=2.0), seed, rank).draw(6, epoch, step)
        hsv = BatchAugment(AugmentHyp(degrees=5.0, shear=2.0, hsv_h=0.015, hsv_s=0.7), seed, rank).draw(6, epoch, step)
        for k in old_keys:
            assert np.array_equal(base[k], hsv[k]), k
        assert (base["hue"] == 0).all() and (base["sat"] == 1).all()
        assert (np.abs(hsv["hue"]) <= 0.015).all() and (np.abs(hsv["sat"] - 1.0) <= 0.7).all()
        assert len(set(hsv["hue"])) == 6 and len(set(hsv["sat"])) == 6
    # the draws the trainer has made since the augmentation exists, pinned: seed 1, rank 0, epoch 1, step 0
    g = torch.Generator().manual_seed(__import__("datasets.augment", fromlist=["step_seed"]).step_seed(1, 0, 1, 0))
    u = torch.rand(3, 11, generator=g, dtype=torch.float64).numpy()
    partners = torch.randint(0, 3, (3, 3), generator=g).numpy()
    gain = 1.0 + (2.0 * torch.rand(3, generator=g, dtype=torch.float64).numpy() - 1.0) * 0.4
    p = BatchAugment(AugmentHyp(hsv_h=0.5, hsv_s=0.5), seed=1).draw(3, 1, 0)
    assert np.array_equal(p["cx"], u[:, 1]) and np.array_equal(p["partners"], partners)
    assert np.array_equal(p["gain"], gain)


def test_is_off_counts_hue_and_saturation():
    from datasets.augment import AugmentHyp, BatchAugment
    off = dict(mosaic=0, degrees=0, translate=0, scale=0, shear=0, fliplr=0, flipud=0, gain=0)
    assert AugmentHyp(**off).is_off() and AugmentHyp().hsv_h == 0.0 and AugmentHyp().hsv_s == 0.0
    assert not AugmentHyp(**off, hsv_h=0.01).is_off() and not AugmentHyp(**off, hsv_s=0.1).is_off()
    assert BatchAugment(AugmentHyp(**off), seed=1).colours(4, 1, 0) is None
    t = BatchAugment(AugmentHyp(**off, hsv_s=0.5), seed=1).colours(4, 1, 0)
    assert all(c.hue == 0 for c in t) and len({c.sat for c in t}) == 4


def test_trainer_flags(capsys):
    import inspect
    import train_yolo11_cuda as T
    ap = T.build_parser()
    a = ap.parse_args([])
    assert (a.data_format, a.ch, a.nc, a.hsv_h, a.hsv_s) == ("crater", 1, 5, 0.015, 0.7)
    a = ap.parse_args(["--data-format", "yolo", "--ch", "3", "--nc", "80", "--hsv-h", "0.02", "--hsv-s", "0.5"])
    assert (a.data_format, a.ch, a.nc, a.hsv_h, a.hsv_s) == ("yolo", 3, 80, 0.02, 0.5)
    assert ap.parse_args(["--data-format", "yolo"]).ch == 1
    for bad in (["--ch", "3"], ["--data-format", "crater", "--ch", "4"], ["--data-format", "yolo", "--ch", "2"],
                ["--data-format", "yolo", "--ch", "5"], ["--data-format", "coco"], ["--nc", "0"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    capsys.readouterr()
    helps = {a.dest: a.help for a in ap._actions}
    assert all("--augment on 3-plane data only" in helps[k] for k in ("hsv_h", "hsv_s"))
    assert inspect.signature(T.make_loaders).parameters["channels"].default == 1
    ld = T._SyntheticLoader(1, 2, 32, seed=0, ch=3, nc=7)
    b = next(iter(ld))
    assert b["img"].shape == (2, 3, 32, 32) and int(b["cls"].max()) < 7
