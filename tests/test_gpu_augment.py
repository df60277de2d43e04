"""GPU training augmentation: ym_augment_u8 bit-exact against the numpy restatement (tests/augment_ref.py) over the
case list the host build is held to (tests/augment_cases.py), identity entries bit-exact against the validation
path's resize, dataset -> collate -> BatchAugment end to end, and two augmented training steps."""
import copy
import functools

import numpy as np
import pytest
import torch

import augment_cases as AC
import augment_ref as AR
from data_cases import make_dataset

pytestmark = pytest.mark.gpu


def _launch(table, ims, S):
    """One ym_augment_u8 launch over `ims` packed as the collate packs them -> (B, S, S) fp32 on the host."""
    from datasets.augment import augment_batch, table_bytes
    from datasets.crater import pack_images
    assert len(table) == len(ims)
    p = pack_images([torch.from_numpy(a).unsqueeze(0) for a in ims], S)
    out = augment_batch(p["img_u8"].cuda(), p["img_meta"].cuda(), table_bytes(table).cuda(), S)
    assert out.shape == (len(ims), 1, S, S) and out.dtype == torch.float32
    return out[:, 0].cpu().numpy()


@pytest.mark.parametrize("S", [64, 96])
def test_kernel_equals_restatement(S):
    ims = AC.sources(S)
    names, entries = zip(*AC.cases(S))
    B = len(ims)
    pad = AC.cases(S)[0][1]                                # the table holds one entry per image of the batch
    want = AR.as_float(AR.render(AC.table_of(entries), ims, S))
    for lo in range(0, len(entries), B):
        chunk = list(entries[lo:lo + B])
        got = _launch(AC.table_of(chunk + [pad] * (B - len(chunk))), ims, S)
        for k in range(len(chunk)):
            bad = int((got[k] != want[lo + k]).sum())
            assert bad == 0, (names[lo + k], bad)


def test_kernel_equals_restatement_640_grid_stride():
    ims, table = AC.big_case()
    got = _launch(table, ims, 640)
    want = AR.as_float(AR.render(table, ims, 640))
    for k in range(len(ims)):
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("S", [64, 320, 640])
def test_identity_entries_equal_resize(S):
    from test_gpu_data import SIZES
    from datasets.augment import augment_batch, plain_entry, table_bytes
    from datasets.crater import pack_images, resize_batch
    rng = np.random.default_rng(S)
    ims = [rng.integers(0, 256, hw, dtype=np.uint8) for hw in SIZES]
    ims.append(np.zeros((S, S), np.uint8) + np.arange(S, dtype=np.uint8)[None])        # already S x S
    p = pack_images([torch.from_numpy(a).unsqueeze(0) for a in ims], S)
    u8, meta = p["img_u8"].cuda(), p["img_meta"].cuda()
    table = AC.table_of([plain_entry(i, *a.shape, S) for i, a in enumerate(ims)])
    got = augment_batch(u8, meta, table_bytes(table).cuda(), S)
    assert torch.equal(got, resize_batch(u8, meta, S))


def _fixture_loader(tmp_path, S, batch):
    from datasets import CraterDatasetCUDA, collate_fn_cuda
    make_dataset(tmp_path, seed=3)
    ds = CraterDatasetCUDA(tmp_path, img_size=S)
    return torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=False,
                                       collate_fn=functools.partial(collate_fn_cuda, img_size=S))


def test_dataset_to_augmented_batch(tmp_path):
    from datasets import AugmentHyp, BatchAugment
    S = 160
    aug = BatchAugment(AugmentHyp(degrees=8.0, shear=2.0, flipud=0.3), seed=11)
    mosaics = 0
    for step, b in enumerate(_fixture_loader(tmp_path, S, 3)):
        d = aug(b, torch.device("cuda"), 1, step)
        assert set(d) == {"img", "batch_idx", "cls", "bboxes", "max_gt"}
        B = b["img_meta"].shape[0]
        assert d["img"].shape == (B, 1, S, S) and d["img"].dtype == torch.float32 and d["img"].is_cuda
        assert d["batch_idx"].dtype == torch.long and d["cls"].dtype == torch.long and d["cls"].shape[1:] == (1,)
        assert d["bboxes"].dtype == torch.float32 and d["bboxes"].shape == (len(d["batch_idx"]), 4)
        table, bi, cl, bb, mg = aug.plan(b, 1, step)
        meta = b["img_meta"].numpy()
        buf = b["img_u8"].numpy()
        ims = [buf[o:o + h * w].reshape(h, w) for o, h, w in meta]
        want = AR.as_float(AR.render(table, ims, S)[:B])
        assert np.array_equal(d["img"][:, 0].cpu().numpy(), want)
        assert torch.equal(d["batch_idx"].cpu(), bi) and torch.equal(d["cls"].cpu(), cl)
        assert torch.equal(d["bboxes"].cpu(), bb) and d["max_gt"] == mg
        assert mg == (int(torch.bincount(bi).max()) if len(bi) else 0)
        mosaics += sum(table[i].tile[3].src >= 0 for i in range(B))
    assert mosaics > 0


def test_two_augmented_training_steps(tmp_path):
    """n@128 bs3 on the fixture dataset: finite losses, different from the un-augmented run, identical between two
    runs with one seed."""
    import train_yolo11_cuda as T
    from datasets import BatchAugment
    from losses import v8DetectionLoss
    from test_gpu_model import _seeded_model
    from yolomi.optim import FusedAdamW
    loader = _fixture_loader(tmp_path, 128, 3)             # 5 images: two steps
    base = _seeded_model("n").train()

    def run(augment):
        m = copy.deepcopy(base)
        opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=5e-4, max_grad_norm=10.0)
        return T.train_one_epoch(m, loader, opt, v8DetectionLoss(m), torch.device("cuda"), 1, 1, None, augment)

    a1, a2, plain = run(BatchAugment(seed=4)), run(BatchAugment(seed=4)), run(None)
    assert set(a1) == {"loss", "box_loss", "cls_loss", "dfl_loss"}
    assert all(np.isfinite(v) for v in a1.values()), a1
    assert a1 == a2, (a1, a2)
    assert a1["loss"] != plain["loss"], (a1, plain)
