"""bench.py --dump-outputs: the writer on CPU tensors.  Small arrays are written whole; a larger one is a fixed
seeded sample (the same positions in every run, so the dumps of two builds compare element for element); every
file is float32 and the caps keep a dump under 64 MB."""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402


def test_dump_sample_whole_and_seeded():
    t = torch.arange(1000, dtype=torch.float64).reshape(10, 100)
    whole = bench.dump_sample(t, 1000, 7)
    assert whole.dtype == np.float32 and whole.shape == (1000,)
    np.testing.assert_array_equal(whole, np.arange(1000, dtype=np.float32))
    a, b = bench.dump_sample(t, 64, 7), bench.dump_sample(t, 64, 7)
    assert a.shape == (64,) and a.dtype == np.float32
    np.testing.assert_array_equal(a, b)                     # same seed, same positions
    assert np.all(np.diff(a) >= 0) and set(a.tolist()) <= set(range(1000))
    assert not np.array_equal(a, bench.dump_sample(t, 64, 8))
    # fp16 maps come out as float32 of the same values
    h = torch.linspace(-2, 2, 33).half()
    np.testing.assert_array_equal(bench.dump_sample(h, 100, 0), h.float().numpy())


def test_dump_outputs_files(tmp_path):
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3), torch.nn.BatchNorm2d(4))
    kept = {"loss": torch.tensor(3.5), "items": torch.tensor([1.0, 2.0, 0.5]),
            "preds": [torch.randn(2, 69, 8, 8), torch.randn(2, 69, 4, 4).half()]}
    sizes = bench.dump_outputs(tmp_path / "d", kept, model)
    got = {p.stem: np.load(p) for p in (tmp_path / "d").glob("*.npy")}
    assert set(got) == {"loss", "loss_items", "pred_level0", "pred_level1", "params", "bn_running_stats"} == set(sizes)
    assert all(a.dtype == np.float32 and a.ndim == 1 and a.size == sizes[k] for k, a in got.items())
    np.testing.assert_array_equal(got["loss"], [3.5])
    np.testing.assert_array_equal(got["loss_items"], [1.0, 2.0, 0.5])
    np.testing.assert_array_equal(got["pred_level0"], kept["preds"][0].reshape(-1).numpy())
    np.testing.assert_array_equal(got["pred_level1"], kept["preds"][1].float().reshape(-1).numpy())
    sd = model.state_dict()
    want = np.concatenate([sd[k].reshape(-1).numpy() for k in ("0.weight", "0.bias", "1.weight", "1.bias")])
    np.testing.assert_array_equal(got["params"], want)
    np.testing.assert_array_equal(got["bn_running_stats"], np.concatenate([np.zeros(4), np.ones(4)]).astype(np.float32))


def test_dump_caps_stay_under_64_mb():
    # the most a dump can hold: three sampled levels, sampled parameters and statistics, the loss and its items
    elems = 3 * bench.DUMP_HEAD_ELEMS + bench.DUMP_STATE_ELEMS + bench.DUMP_STATS_ELEMS + 1 + 16
    assert 4 * elems + 7 * 128 < 64e6
