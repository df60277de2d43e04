"""Host-side checks of the weight EMA (yolomi/ema.py, train_yolo11_cuda.py --ema; no GPU): the warm-up ramp,
the trainer flags, the table entry's layout, the checkpoint keys and their round trip, and that update() has no
CPU path."""
import ctypes
import inspect
import math

import pytest
import torch


def _model():
    from test_models_cpu import _model as build
    return build("n")


def _perturbed(seed):
    """A model whose every fp32 entry differs from a fresh build's (so a copy can be told from a rebuild)."""
    m = _model()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for v in m.state_dict().values():
            if v.is_floating_point():
                v.add_(torch.randn(v.shape, generator=g) * 0.01)
            else:
                v.add_(seed)
    return m


def test_decay_ramp_closed_form():
    from yolomi.ema import ModelEMA
    ema = ModelEMA(torch.nn.Linear(2, 2), decay=0.9999, tau=2000)
    for u in (1, 2000, 10 ** 6):
        d = ema.decay_at(u)
        assert isinstance(d, float) and d == 0.9999 * (1.0 - math.exp(-u / 2000))
    assert ema.decay_at(1) < 1e-3 and ema.decay_at(10 ** 6) == 0.9999
    assert ModelEMA(torch.nn.Linear(2, 2), decay=0.5, tau=10).decay_at(10) == 0.5 * (1.0 - math.exp(-1.0))
    assert ema.updates == 0


def test_trainer_flags_and_signatures():
    import train_yolo11_cuda as T
    ap = T.build_parser()
    a = ap.parse_args([])
    assert a.ema is False and a.ema_decay == 0.9999 and a.ema_tau == 2000
    a = ap.parse_args(["--ema", "--ema-decay", "0.99", "--ema-tau", "50"])
    assert a.ema is True and a.ema_decay == 0.99 and a.ema_tau == 50
    for f in (T.train_one_epoch, T.make_checkpoint, T.resume_checkpoint):
        assert inspect.signature(f).parameters["ema"].default is None
    from yolomi.optim import FusedAdamW
    opt = FusedAdamW([torch.nn.Parameter(torch.zeros(2))])
    assert opt.fuses_ema is False and opt.ema is None


def test_ema_entry_layout():
    from yolomi._lib import EmaEntry
    assert ctypes.sizeof(EmaEntry) == 32
    assert [(n, getattr(EmaEntry, n).offset) for n, _ in EmaEntry._fields_] == [("ema", 0), ("src", 8), ("offset", 16),
                                                                                ("n", 24)]


def test_entry_points_check_arguments_before_any_launch():
    """Refused on the host: a null table, no entries, one_minus_decay outside [0, 1]; an empty table is a no-op.
    (The table pointer is never read on the host, so a dummy stands in.)"""
    from yolomi import YolomiError
    from yolomi._lib import call
    t = 64
    for args in ((None, 1, 8, 0.5, None), (t, 0, 8, 0.5, None), (t, 1, 8, 1.0001, None), (t, 1, 8, -1e-9, None)):
        with pytest.raises(YolomiError):
            call("ym_ema_update", *args)
    call("ym_ema_update", t, 1, 0, 0.5, None)
    a = (1e-3, 0.9, 0.999, 1e-8, 5e-4, 1, 0.0, None)
    for args in ((None, t, 1, 8, *a, 0.5, None), (t, None, 1, 8, *a, 0.5, None), (t, t, 0, 8, *a, 0.5, None),
                 (t, t, 1, 8, *a, 2.0, None), (t, t, 1, 8, *a[:5], 0, 0.0, None, 0.5, None),
                 (t, t, 1, 8, *a[:5], 1, 10.0, None, 0.5, None)):
        with pytest.raises(YolomiError):
            call("ym_adamw_ema", *args)
    call("ym_adamw_ema", t, t, 1, 0, *a, 0.5, None)


def test_ema_copy_is_independent():
    from yolomi.ema import ModelEMA
    m = _perturbed(1)
    m.__dict__["_ym_plans"] = {"sentinel": object()}            # what a forward caches on the module (yolomi/graph.py)
    ema = ModelEMA(m)
    assert m.__dict__["_ym_plans"].keys() == {"sentinel"}        # left in place on the source
    assert not any(k.startswith("_ym_") for mod in ema.ema.modules() for k in mod.__dict__)
    assert type(ema.ema) is type(m) and not ema.ema.training and m.training
    a, b = m.state_dict(), ema.ema.state_dict()
    assert list(a) == list(b)
    mine = {v.untyped_storage().data_ptr() for v in a.values()}
    for k, v in b.items():
        assert torch.equal(v, a[k]) and v.untyped_storage().data_ptr() not in mine, k
    assert all(not p.requires_grad for p in ema.ema.parameters())
    assert any(p.requires_grad for p in m.parameters())


def test_update_has_no_cpu_path():
    from yolomi import YolomiError
    from yolomi.ema import ModelEMA
    ema = ModelEMA(_model())
    with pytest.raises(YolomiError):
        ema.update()
    assert ema.updates == 0


def test_checkpoint_keys_with_and_without_ema():
    import train_yolo11_cuda as T
    from yolomi.ema import ModelEMA
    m = _model()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    seven = ["epoch", "model_state_dict", "optimizer_state_dict", "train_metrics", "val_metrics", "best_loss",
             "best_mAP50"]
    assert list(T.make_checkpoint(0, m, opt, {}, {}, 1.0, 0.0)) == seven
    ema = ModelEMA(m, updates=7)
    ck = T.make_checkpoint(0, m, opt, {}, {}, 1.0, 0.0, ema=ema)
    assert list(ck) == seven + ["ema_state_dict", "ema_updates"]
    assert ck["ema_updates"] == 7 and list(ck["ema_state_dict"]) == list(m.state_dict())
    # the raw training weights stay where the resume (and the reference's loader) look for them
    assert all(ck["model_state_dict"][k].data_ptr() == v.data_ptr() for k, v in m.state_dict().items())


def test_checkpoint_with_ema_round_trips(tmp_path):
    import train_yolo11_cuda as T
    from yolomi.ema import ModelEMA
    m = _perturbed(2)
    ema = ModelEMA(m, updates=123)
    with torch.no_grad():                                        # an average that is not the model
        for v in ema.ema.state_dict().values():
            if v.is_floating_point():
                v.mul_(0.5)
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.num_batches_tracked.fill_(41)                # copied into the EMA when its state is read
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    torch.save(T.make_checkpoint(3, m, opt, {"loss": 1.0}, {"loss": 2.0}, 2.0, 0.5, ema=ema), tmp_path / "last.pt")
    want = {k: v.clone() for k, v in ema.ema.state_dict().items()}
    assert int(want["model.0.bn.num_batches_tracked"]) == 41
    torch.load(tmp_path / "last.pt", map_location="cpu", weights_only=True)      # the restricted loader takes it
    m2 = _model()
    ema2 = ModelEMA(m2)
    opt2 = torch.optim.AdamW(m2.parameters(), lr=1e-3)
    assert T.resume_checkpoint(tmp_path / "last.pt", m2, opt2, torch.device("cpu"), ema=ema2) == (4, 2.0, 0.5)
    assert ema2.updates == 123
    for k, v in ema2.ema.state_dict().items():
        assert torch.equal(v, want[k]), k
    for k, v in m2.state_dict().items():
        assert torch.equal(v, m.state_dict()[k]), k
    assert not torch.equal(ema2.ema.state_dict()["model.0.conv.weight"], m2.state_dict()["model.0.conv.weight"])


def test_checkpoint_without_ema_seeds_it_from_the_model(tmp_path):
    import train_yolo11_cuda as T
    from yolomi.ema import ModelEMA
    m = _perturbed(3)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    torch.save(T.make_checkpoint(0, m, opt, {}, {}, 1.0, 0.0), tmp_path / "last.pt")
    m2 = _model()
    ema2 = ModelEMA(m2, updates=55)
    opt2 = torch.optim.AdamW(m2.parameters(), lr=1e-3)
    T.resume_checkpoint(tmp_path / "last.pt", m2, opt2, torch.device("cpu"), ema=ema2)
    assert ema2.updates == 0
    for k, v in ema2.ema.state_dict().items():
        assert torch.equal(v, m.state_dict()[k]), k
    # and without an EMA the resume is what it was
    m3 = _model()
    T.resume_checkpoint(tmp_path / "last.pt", m3, torch.optim.AdamW(m3.parameters(), lr=1e-3), torch.device("cpu"))
    assert all(torch.equal(v, m.state_dict()[k]) for k, v in m3.state_dict().items())


def test_state_dict_round_trip():
    from yolomi.ema import ModelEMA
    a, b = ModelEMA(_perturbed(4), updates=9), ModelEMA(_model())
    sd = a.state_dict()
    assert set(sd) == {"ema_state_dict", "ema_updates"}
    b.load_state_dict(sd)
    assert b.updates == 9
    assert all(torch.equal(v, a.ema.state_dict()[k]) for k, v in b.ema.state_dict().items())
