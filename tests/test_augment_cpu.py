"""Training augmentation without a GPU: the numpy restatement of the kernel arithmetic (tests/augment_ref.py) on
hand-built tables, the shared sampling header (include/yolomi_augment.h) compiled for the host and held to the
restatement bit for bit over the GPU test's case list, the host box policy, seeding and the off switch."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest
import torch

import augment_cases as AC
import augment_ref as AR
from conftest import ROOT

S0 = 32
FILL = 114


def _A():
    from datasets import augment
    return augment


def _one(m, im, S=S0, c=None, rect=None, **kw):
    """Render one single-tile entry with output -> source map `m` over `im`."""
    A = _A()
    rect = rect or (-0.5, -0.5, S - 0.5, S - 0.5)
    e = A.make_entry([A.make_tile(0, m, rect)], np.eye(3) if c is None else c, None, **kw)
    return AR.render_entry(e, [im], S)


@pytest.fixture(scope="module")
def sq():
    return np.random.default_rng(5).integers(0, 256, (S0, S0), dtype=np.uint8)


def test_entry_layout_matches_header():
    from yolomi._lib import AugEntry, AugTile
    assert ctypes.sizeof(AugTile) == 88 and ctypes.sizeof(AugEntry) == 432      # the header's static_assert


def test_ref_identity_returns_source(sq):
    assert np.array_equal(_one(np.eye(3), sq), sq)


def test_ref_flips(sq):
    A = _A()
    assert np.array_equal(_one(A.flip_matrix(S0, True, False), sq), np.fliplr(sq))
    assert np.array_equal(_one(A.flip_matrix(S0, False, True), sq), np.flipud(sq))


def test_ref_integer_translation_shifts_and_fills(sq):
    A = _A()
    inv = A.translation(-3.0, 2.0)                         # out(x, y) = src(x - 3, y + 2)
    got = _one(inv, sq, c=inv)
    want = np.full_like(sq, FILL)
    want[:S0 - 2, 3:] = sq[2:, :S0 - 3]
    assert np.array_equal(got, want)


def test_ref_rot90_about_centre(sq):
    m = np.array([[0.0, -1.0, S0 - 1.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    assert np.array_equal(_one(m, sq), np.rot90(sq))


def test_ref_constant_stays_constant():
    A = _A()
    im = np.full((81, 127), 77, np.uint8)
    inv = np.linalg.inv(A.affine_matrix(S0, S0, angle=37.0, scale=0.7, shear_x=4.0))
    got = AR.render_entry(A.plain_entry(0, 81, 127, S0, inv), [im], S0)
    assert set(np.unique(got)) == {77, FILL}


def test_ref_gain_saturates():
    im = np.full((S0, S0), 200, np.uint8)
    assert (_one(np.eye(3), im, gain=1.5) == 255).all()
    assert (_one(np.eye(3), im, gain=0.5) == 100).all()


def _mosaic4(inv, xc, yc):
    A = _A()
    rng = np.random.default_rng(9)
    ims = [rng.integers(0, 256, (S0, S0), dtype=np.uint8) for _ in range(4)]
    e = A.mosaic_entry([0, 1, 2, 3], [(S0, S0)] * 4, xc, yc, S0, inv)
    return ims, AR.render_entry(e, ims, S0)


def test_ref_mosaic_quadrants_show_their_tiles():
    A = _A()
    h = S0 // 2
    ims, got = _mosaic4(A.translation(h, h), S0, S0)       # the window is the canvas' middle S x S
    assert np.array_equal(got[:h, :h], ims[0][h:, h:]) and np.array_equal(got[:h, h:], ims[1][h:, :h])
    assert np.array_equal(got[h:, :h], ims[2][:h, h:]) and np.array_equal(got[h:, h:], ims[3][:h, :h])


def test_ref_mosaic_fill_outside_tiles():
    q = S0 // 4
    ims, got = _mosaic4(np.eye(3), S0 + q, S0 + q)         # the window is the canvas' first S x S
    assert (got[:q, :] == FILL).all() and (got[:, :q] == FILL).all()
    assert np.array_equal(got[q:, q:], ims[0][:S0 - q, :S0 - q])


# ---------------------------------------------------------------- the shared header, built for the host
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("aughost") / "augment_host"
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "augment_host.cpp"), "-o", str(exe)], check=True)
    return exe


def _run_host(exe, tmp_path, table, n, ims, S):
    AR.write_case_file(tmp_path / "cases.bin", table, n, ims, S)
    subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], check=True, timeout=120)
    return np.fromfile(tmp_path / "out.bin", dtype=np.uint8).reshape(n, S, S)


@pytest.mark.parametrize("S", [64, 96])
def test_host_build_equals_restatement(host_program, tmp_path, S):
    ims = AC.sources(S)
    names, entries = zip(*AC.cases(S))
    table = AC.table_of(entries)
    got = _run_host(host_program, tmp_path, table, len(entries), ims, S)
    want = AR.render(table, ims, S)
    for i, name in enumerate(names):
        assert np.array_equal(got[i], want[i]), (name, int((got[i] != want[i]).sum()))
    # the cases are not degenerate: the mosaics show all four tiles and fill, the rotations show fill
    for name in ("mosaic_off", "rot37_s0.5"):
        assert (want[names.index(name)] == FILL).any() and (want[names.index(name)] != FILL).sum() > S * S // 8


def test_host_build_equals_restatement_640(host_program, tmp_path):
    ims, table = AC.big_case()
    got = _run_host(host_program, tmp_path, table, len(table), ims, 640)
    assert np.array_equal(got, AR.render(table, ims, 640))


# ---------------------------------------------------------------- box policy
def _host_batch(sizes, boxes_per_image, S):
    """A collated host batch as collate_fn_cuda builds it (normalised xyxy rows)."""
    from datasets.crater import pack_images
    rng = np.random.default_rng(11)
    b = pack_images([torch.from_numpy(rng.integers(0, 256, hw, dtype=np.uint8)).unsqueeze(0) for hw in sizes], S)
    bidx = [torch.full((len(x),), i, dtype=torch.long) for i, x in enumerate(boxes_per_image)]
    bb = [torch.tensor(x, dtype=torch.float32).reshape(-1, 4) for x in boxes_per_image]
    b.update({"batch_idx": torch.cat(bidx), "bboxes": torch.cat(bb),
              "cls": (torch.arange(sum(len(x) for x in boxes_per_image)) % 5).reshape(-1, 1)})
    return b


BOXES = [[[0.1, 0.2, 0.4, 0.5], [0.6, 0.6, 0.9, 0.95]], [[0.25, 0.25, 0.75, 0.5]], [], [[0.0, 0.0, 1.0, 1.0]]]
SIZES4 = [(48, 64), (70, 51), (64, 64), (10, 200)]


def test_boxes_identity_unchanged():
    A = _A()
    b = _host_batch(SIZES4, BOXES, 64)
    aug = A.BatchAugment(A.AugmentHyp(mosaic=0, translate=0, scale=0, fliplr=0, gain=0.3), seed=1)
    table, bi, cl, bb, mg = aug.plan(b, 1, 0)
    assert torch.equal(bi, b["batch_idx"]) and torch.equal(cl, b["cls"]) and torch.equal(bb, b["bboxes"])
    assert all(table[i].flags & 1 for i in range(4)) and mg == 2
    assert len({table[i].gain for i in range(4)}) > 1


def test_boxes_flips_mirror():
    A = _A()
    xy = np.array([[6.4, 12.8, 25.6, 32.0]])
    out, keep = A.transform_boxes(xy, np.eye(3), 64, True, False)
    assert keep.all() and np.allclose(out, [[1 - 0.4, 0.2, 1 - 0.1, 0.5]], atol=1e-12)
    out, _ = A.transform_boxes(xy, np.eye(3), 64, False, True)
    assert np.allclose(out, [[0.1, 1 - 0.5, 0.4, 1 - 0.2]], atol=1e-12)
    b = _host_batch(SIZES4, BOXES, 64)
    _, bi, cl, bb, _ = A.BatchAugment(A.AugmentHyp(mosaic=0, translate=0, scale=0, fliplr=1.0, gain=0), 0).plan(b, 1, 0)
    want = b["bboxes"].clone()
    want[:, 0], want[:, 2] = 1 - b["bboxes"][:, 2], 1 - b["bboxes"][:, 0]
    assert torch.equal(bi, b["batch_idx"]) and torch.allclose(bb, want, atol=1e-6)


def test_boxes_mosaic_offsets_and_drops():
    A = _A()
    S = 64
    b = _host_batch(SIZES4, BOXES, S)
    aug = A.BatchAugment(A.AugmentHyp(mosaic=1.0, translate=0, scale=0, fliplr=0, gain=0), seed=3)
    p = aug.draw(4, 1, 0)
    table, bi, cl, bb, mg = aug.plan(b, 1, 0)
    src_boxes = [np.array(x, np.float64).reshape(-1, 4) for x in BOXES]
    src_cls = np.split(b["cls"].numpy().reshape(-1), np.cumsum([len(x) for x in BOXES])[:-1])
    for i in range(4):
        assert not table[i].flags & 1
        xc, yc = int(S / 2 + p["cx"][i] * S), int(S / 2 + p["cy"][i] * S)
        assert S // 2 <= xc < 3 * S // 2 and S // 2 <= yc < 3 * S // 2
        want, want_cls = [], []
        srcs = [i, *p["partners"][i]]
        for (ox, oy), s in zip(A.mosaic_origins(xc, yc, S), srcs):
            for row, c in zip(src_boxes[s], src_cls[s]):
                # tile placed at its offset on the 2S canvas; unit affine shows canvas [S/2, 3S/2)
                pre = np.clip(row * S + [ox, oy, ox, oy], 0, 2 * S) - S / 2
                post = np.clip(pre, 0, S)
                w, h = post[2] - post[0], post[3] - post[1]
                if w > 2 and h > 2 and w * h >= 0.1 * (pre[2] - pre[0]) * (pre[3] - pre[1]) and max(w / h, h / w) < 100:
                    want.append(post / S), want_cls.append(c)
        m = (bi == i).numpy()
        assert m.sum() == len(want)
        if want:
            assert np.allclose(bb.numpy()[m], np.array(want), atol=1e-6)
            assert np.array_equal(cl.numpy()[m].reshape(-1), np.array(want_cls))
        assert [table[i].tile[k].src for k in range(4)] == [int(s) for s in srcs]
    assert mg == (int(torch.bincount(bi).max()) if len(bi) else 0)
    assert float(bb.min()) >= 0.0 and float(bb.max()) <= 1.0


def test_boxes_outside_and_candidate_filter():
    A = _A()
    S = 64
    xy = np.array([[10.0, 10.0, 30.0, 30.0],      # stays
                   [10.0, 10.0, 11.5, 30.0],      # 1.5 px wide
                   [1.0, 1.0, 5.0, 5.0],          # pushed wholly outside by the shift
                   [0.0, 20.0, 26.0, 40.0],       # 2.5 px of 26 left: < 0.1 of its area
                   [20.0, 20.0, 60.0, 20.3]])     # 0.3 px high (also aspect > 100)
    out, keep = A.transform_boxes(xy, A.translation(-23.5, 0.0), S, False, False)
    assert keep.tolist() == [True, False, False, False, False]
    assert np.allclose(out, [[0.0, 10 / 64, 6.5 / 64, 30 / 64]])
    pre = np.array([[0.0, 0.0, 300.0, 2.5]])
    assert not A.box_candidates(pre, pre).any()            # aspect ratio 120


def test_boxes_within_unit_and_max_gt_default_hyp():
    A = _A()
    b = _host_batch(SIZES4, BOXES, 64)
    aug = A.BatchAugment(A.AugmentHyp(degrees=10.0, shear=3.0, flipud=0.5), seed=7)
    for step in range(6):
        table, bi, cl, bb, mg = aug.plan(b, 2, step)
        assert len(bi) == len(cl) == len(bb) and cl.shape[1:] == (1,) and bb.dtype == torch.float32
        if len(bb):
            assert float(bb.min()) >= 0.0 and float(bb.max()) <= 1.0
            assert (bb[:, 2] > bb[:, 0]).all() and (bb[:, 3] > bb[:, 1]).all()
        assert mg == (int(torch.bincount(bi, minlength=4).max()) if len(bi) else 0)


def test_boxes_empty_batch():
    A = _A()
    b = _host_batch(SIZES4, [[], [], [], []], 64)
    table, bi, cl, bb, mg = A.BatchAugment(seed=2).plan(b, 1, 0)
    assert bi.shape == (0,) and cl.shape == (0, 1) and bb.shape == (0, 4) and mg == 0
    from datasets.crater import pack_images
    e = pack_images([], 64)
    e.update({"batch_idx": torch.zeros((0,), dtype=torch.long), "cls": torch.zeros((0, 1), dtype=torch.long),
              "bboxes": torch.zeros((0, 4))})
    _, bi, cl, bb, mg = A.BatchAugment(seed=2).plan(e, 1, 0)
    assert bi.shape == (0,) and bb.shape == (0, 4) and mg == 0


# ---------------------------------------------------------------- seeding and the off switch
def test_seeding_reproducible_and_sensitive():
    A = _A()
    b = _host_batch(SIZES4, BOXES, 64)

    def run(seed, rank, epoch, step):
        t, bi, cl, bb, mg = A.BatchAugment(A.AugmentHyp(degrees=5.0), seed, rank).plan(b, epoch, step)
        return bytes(t), bi, bb

    base = run(5, 0, 3, 17)
    again = run(5, 0, 3, 17)
    assert base[0] == again[0] and torch.equal(base[1], again[1]) and torch.equal(base[2], again[2])
    for other in ((6, 0, 3, 17), (5, 1, 3, 17), (5, 0, 4, 17), (5, 0, 3, 18)):
        o = run(*other)
        assert o[0] != base[0], other
        assert o[2].shape != base[2].shape or not torch.equal(o[2], base[2]), other


def test_close_mosaic_epoch():
    A = _A()
    aug = A.BatchAugment(A.AugmentHyp(), seed=1, no_mosaic_from=5)
    assert aug.draw(8, 4, 0)["mosaic"].all() and not aug.draw(8, 5, 0)["mosaic"].any()


def test_off_switch_is_prepare_batch():
    A = _A()
    from datasets import prepare_batch
    from datasets.synthetic import synth_batch
    off = A.AugmentHyp(mosaic=0, degrees=0, translate=0, scale=0, shear=0, fliplr=0, flipud=0, gain=0)
    assert off.is_off() and not A.AugmentHyp().is_off()
    b = synth_batch(2, 64, seed=1)
    for hyp in (off, A.AugmentHyp()):                      # a synthetic batch carries no raw images: passed through
        got = A.BatchAugment(hyp, seed=1)(b, "cpu", 1, 0)
        want = prepare_batch(b, "cpu")
        assert set(got) == set(want)
        for k in want:
            assert torch.equal(got[k], want[k]) if isinstance(want[k], torch.Tensor) else got[k] == want[k]
    # all-zero hyperparameters on raw images draw the identity for every image
    table, bi, cl, bb, mg = A.BatchAugment(off, seed=1).plan(_host_batch(SIZES4, BOXES, 64), 1, 0)
    assert all(table[i].flags & 1 and table[i].gain == 65536 for i in range(4))


def test_exports_and_trainer_flags():
    import datasets
    import train_yolo11_cuda as T
    assert {"AugmentHyp", "BatchAugment"} <= set(datasets.__all__)
    import inspect
    sig = inspect.signature(T.train_one_epoch)
    assert sig.parameters["augment"].default is None and sig.parameters["dp"].default is None
