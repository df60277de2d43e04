"""The weight EMA on the GPU (csrc/optim.hip ym_ema_update / ym_adamw_ema, yolomi/ema.py, FusedAdamW.attach_ema,
train_yolo11_cuda.py --ema).

The rule is fixed, e' = fma(omd, p - e, e) in fp32 with omd = 1 - d rounded once, so it is checked against its fp64
restatement teacher-forced (each step restarts from the device's previous values) within

    |got - want| <= 2^-22 * max(|e|, |p|)      elementwise

half an ulp on p - e (|p - e| <= 2 max, times omd <= 1: 2^-23 max) plus half an ulp on the result (2^-24 max) is
0.75 * 2^-22 max.  Everything else is bit-equality: the fused pass against ym_adamw (p, exp_avg, exp_avg_sq) and
against ym_ema_update on the post-step parameters, NULL entries, the two ends of one_minus_decay, the raw weights
with and without an EMA, and the eval plan's output against a fresh model loaded from the EMA state.

Shapes: test_gpu_optim.SHAPES plus (4097,) (one past a 4096-element block) and (3, 5000) (spans blocks, starts
mid-block), and a table whose total stays below one 256-thread row.
"""
import copy
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from test_gpu_optim import SHAPES

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

BIG = list(SHAPES) + [(4097,), (3, 5000)]           # 45 908 elements: 12 blocks, boundaries anywhere inside them
SMALL = [(5,), (7, 3), (1,), (64,)]                 # 91 elements: a total below 256
SETS = [pytest.param(BIG, id="big"), pytest.param(SMALL, id="small")]
CLIPS = [(None, 1.0), (10.0, 1.0), (10.0, 0.01), (0.5, 3.0)]      # test_fused_adamw_matches_torch's
BOUND = 2.0 ** -22


def _rand(shapes, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(s, generator=g) * scale).cuda() for s in shapes]


def _omd(updates, decay=0.9999, tau=2000.0):
    return 1.0 - decay * (1.0 - math.exp(-updates / tau))


def _check_rule(prev, src, got, omd, what=""):
    """got == fp64 restatement of e + omd32 * (p - e) from `prev`, within the bound of the rule."""
    omd32 = float(np.float32(omd))
    for i, (e, p, g) in enumerate(zip(prev, src, got)):
        e, p, g = e.double(), p.double(), g.double()
        want = e + omd32 * (p - e)
        err = (g - want).abs()
        bound = BOUND * torch.maximum(e.abs(), p.abs())
        assert bool((err <= bound).all()), (what, i, float((err - bound).max()))


def _ema_table(emas, srcs):
    from yolomi._lib import EmaEntry
    arr = (EmaEntry * len(emas))()
    off = 0
    for ent, e, s in zip(arr, emas, srcs):
        ent.ema, ent.src, ent.offset, ent.n = e.data_ptr(), s.data_ptr(), off, e.numel()
        off += e.numel()
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda(), len(emas), off


def _adamw_table(ps, gs, ms, vs):
    from yolomi._lib import AdamWEntry
    arr = (AdamWEntry * len(ps))()
    off = 0
    for ent, p, g, m, v in zip(arr, ps, gs, ms, vs):
        ent.p, ent.g, ent.m, ent.v, ent.offset, ent.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), off, \
            p.numel()
        off += p.numel()
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda(), len(ps), off


def _ema_update(emas, srcs, omd):
    from yolomi._lib import call, stream_ptr
    tab, n, total = _ema_table(emas, srcs)
    call("ym_ema_update", tab.data_ptr(), n, total, omd, stream_ptr())
    torch.cuda.synchronize()


HYP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=5e-4)


def _adamw(ps, gs, ms, vs, step, ema_ptrs=None, omd=None):
    """ym_adamw, or ym_adamw_ema with the device pointer array built from `ema_ptrs` (ints, 0 = NULL)."""
    from yolomi._lib import call, stream_ptr
    tab, n, total = _adamw_table(ps, gs, ms, vs)
    h = HYP
    if ema_ptrs is None:
        call("ym_adamw", tab.data_ptr(), n, total, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], step, 0.0, None,
             stream_ptr())
    else:
        ptrs = torch.tensor(ema_ptrs, dtype=torch.int64).cuda()
        call("ym_adamw_ema", tab.data_ptr(), ptrs.data_ptr(), n, total, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"],
             step, 0.0, None, omd, stream_ptr())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ 1. ym_ema_update
@pytest.mark.parametrize("shapes", SETS)
@pytest.mark.parametrize("decay,tau", [(0.9999, 2000.0), (0.9, 2.0)])
def test_ema_update_matches_fp64_restatement(shapes, decay, tau):
    emas = _rand(shapes, 1)
    for step in range(1, 4):
        srcs = _rand(shapes, 10 + step)
        keep = [s.clone() for s in srcs]
        prev = [e.clone() for e in emas]
        omd = _omd(step, decay, tau)
        _ema_update(emas, srcs, omd)
        _check_rule(prev, srcs, emas, omd, f"step {step}")
        assert all(torch.equal(s, k) for s, k in zip(srcs, keep))          # src is only read
        assert not any(torch.equal(e, q) for e, q in zip(emas, prev))


# ------------------------------------------------------------------------- 2, 3. the fused pass, through the module
class _Bag(torch.nn.Module):
    """Parameters of the given shapes plus what an optimizer does not step: a frozen parameter (no gradient), an
    fp32 buffer that moves every step and an integer buffer."""

    def __init__(self, shapes, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes])
        self.frozen = torch.nn.Parameter(torch.randn(300, generator=g), requires_grad=False)
        self.register_buffer("stat", torch.randn(77, generator=g))
        self.register_buffer("count", torch.tensor(1))


def _set_grads(bag, shapes, step, scale):
    g = torch.Generator().manual_seed(100 + step)
    for p, s in zip(bag.ps, shapes):
        p.grad = torch.randn(s, generator=g).cuda() * scale
    with torch.no_grad():
        bag.stat.add_(0.25 * (step + 1))
        bag.frozen.mul_(1.5)
        bag.count.add_(1)


@pytest.mark.parametrize("shapes", SETS)
@pytest.mark.parametrize("clip,scale", CLIPS)
def test_fused_pass_bit_equal_to_adamw_and_to_standalone_ema(shapes, clip, scale):
    """Three runs of 4 steps on identical inputs: (a) FusedAdamW alone, (b) with the EMA attached (ym_adamw_ema +
    the launch over the rest), (c) FusedAdamW followed by ModelEMA.update() (ym_ema_update over everything).
    (b)'s p / exp_avg / exp_avg_sq equal (a)'s bit for bit, and (b)'s EMA equals (c)'s bit for bit: the fused update
    is ym_ema_update applied to the post-step parameters with the same omd."""
    from yolomi.ema import ModelEMA
    from yolomi.optim import FusedAdamW
    bags = [_Bag(shapes, 0).cuda() for _ in range(3)]
    opts = [FusedAdamW(b.parameters(), lr=1e-3, weight_decay=5e-4, max_grad_norm=clip) for b in bags]
    emas = [None, ModelEMA(bags[1], decay=0.9, tau=2.0), ModelEMA(bags[2], decay=0.9, tau=2.0)]
    opts[1].attach_ema(emas[1])
    assert opts[1].fuses_ema and not opts[2].fuses_ema
    for step in range(4):
        prev = [v.clone() for v in emas[1].ema.state_dict().values()]
        for b, o, e in zip(bags, opts, emas):
            _set_grads(b, shapes, step, scale)
            o.step()
            if e is not None and not o.fuses_ema:
                e.update()
        if step == 2:
            for o in opts:
                o.param_groups[0]["lr"] = 5e-4
        torch.cuda.synchronize()
        assert emas[1].updates == emas[2].updates == step + 1
        for pa, pb in zip(bags[0].ps, bags[1].ps):
            assert torch.equal(pa, pb)
            for k in ("exp_avg", "exp_avg_sq", "step"):
                assert torch.equal(opts[0].state[pa][k], opts[1].state[pb][k]), k
        if clip is not None:
            assert torch.equal(opts[0].last_grad_norm, opts[1].last_grad_norm)
        sb, sc = emas[1].ema.state_dict(), emas[2].ema.state_dict()
        for k in sb:
            assert torch.equal(sb[k], sc[k]), (step, k)
        # and both follow the rule (the frozen parameter and the buffer through the launch over the rest)
        fl = [k for k, v in sb.items() if v.is_floating_point()]
        src = bags[1].state_dict()
        _check_rule([p for k, p in zip(sb, prev) if k in fl], [src[k] for k in fl], [sb[k] for k in fl],
                    1.0 - emas[1].decay_at(step + 1), f"step {step}")
        assert not any(torch.equal(sb[k], src[k]) for k in fl)
    assert int(emas[1].ema.count) == 1 and int(emas[1].state_dict()["ema_state_dict"]["count"]) == 5


# ------------------------------------------------------------------------------------------ 4. NULL entries
@pytest.mark.parametrize("shapes", SETS)
def test_null_ema_pointers_write_nothing(shapes):
    """Every other entry has no EMA: the arena that would hold it (and the guard gaps between all of them) keeps
    its bits, the other entries equal ym_ema_update on the post-step parameters, and p / m / v equal ym_adamw's."""
    GAP = 64
    sizes = [int(np.prod(s)) for s in shapes]
    arena = torch.randn(sum(sizes) + GAP * (len(sizes) + 1), generator=torch.Generator().manual_seed(5)).cuda()
    views, off = [], GAP
    for n in sizes:
        views.append(arena[off:off + n])
        off += n + GAP
    before = arena.clone()
    null = [i % 2 == 1 for i in range(len(shapes))]
    omd = 0.3
    runs = []
    for fused in (False, True):
        ps, gs = _rand(shapes, 7), _rand(shapes, 8)
        ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
        for step in (1, 2):
            if fused:
                _adamw(ps, gs, ms, vs, step, [0 if z else v.data_ptr() for v, z in zip(views, null)], omd)
            else:
                _adamw(ps, gs, ms, vs, step)
        runs.append((ps, ms, vs))
    for a, b in zip(runs[0], runs[1]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the expected arena: two stand-alone updates of the live entries from the plain run's parameters
    want = before.clone()
    wviews, off = [], GAP
    for n in sizes:
        wviews.append(want[off:off + n])
        off += n + GAP
    ps, gs = _rand(shapes, 7), _rand(shapes, 8)
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    live = [i for i, z in enumerate(null) if not z]
    for step in (1, 2):
        _adamw(ps, gs, ms, vs, step)
        _ema_update([wviews[i] for i in live], [ps[i].reshape(-1) for i in live], omd)
    assert torch.equal(arena, want)
    for i, z in enumerate(null):
        assert torch.equal(views[i], before[views[i].storage_offset():][:sizes[i]]) == z, i


# ------------------------------------------------------------------------------------------ 5. the two ends
@pytest.mark.parametrize("shapes", SETS)
def test_one_minus_decay_zero_and_one(shapes):
    """0 leaves the EMA bit-unchanged (a -0.0 included), 1 makes it the parameters bit for bit, also where |e| >> |p|
    (fl(fl(p - e) + e) would not be p)."""
    emas = _rand(shapes, 1, scale=1e4)
    emas[0].view(-1)[0] = -0.0
    srcs = _rand(shapes, 2, scale=1e-4)
    keep = [e.clone() for e in emas]
    _ema_update(emas, srcs, 0.0)
    assert all(torch.equal(e.view(torch.int32), k.view(torch.int32)) for e, k in zip(emas, keep))
    _ema_update(emas, srcs, 1.0)
    assert all(torch.equal(e.view(torch.int32), s.view(torch.int32)) for e, s in zip(emas, srcs))
    # the same two ends inside the AdamW pass
    for omd in (0.0, 1.0):
        ps, gs = _rand(shapes, 3, scale=1e-4), _rand(shapes, 4)
        ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
        es = _rand(shapes, 5, scale=1e4)
        keep = [e.clone() for e in es]
        _adamw(ps, gs, ms, vs, 1, [e.data_ptr() for e in es], omd)
        want = keep if omd == 0.0 else ps
        assert all(torch.equal(e.view(torch.int32), w.view(torch.int32)) for e, w in zip(es, want)), omd


def test_argument_checks():
    from yolomi import YolomiError
    from yolomi._lib import call, stream_ptr
    e, s = _rand([(8,)], 1), _rand([(8,)], 2)
    tab, n, total = _ema_table(e, s)
    ptrs = torch.tensor([e[0].data_ptr()], dtype=torch.int64).cuda()
    st = stream_ptr()
    for args in ((None, n, total, 0.5, st), (tab.data_ptr(), 0, total, 0.5, st), (tab.data_ptr(), n, total, 1.5, st),
                 (tab.data_ptr(), n, total, -0.1, st)):
        with pytest.raises(YolomiError):
            call("ym_ema_update", *args)
    call("ym_ema_update", tab.data_ptr(), n, 0, 0.5, st)                  # total == 0: nothing to do
    a = (1e-3, 0.9, 0.999, 1e-8, 5e-4, 1, 0.0, None)
    t, q = tab.data_ptr(), ptrs.data_ptr()
    for args in ((None, q, 1, 8, *a, 0.5, st), (t, None, 1, 8, *a, 0.5, st), (t, q, 0, 8, *a, 0.5, st),
                 (t, q, 1, 8, *a, 2.0, st)):
        with pytest.raises(YolomiError):
            call("ym_adamw_ema", *args)
    call("ym_adamw_ema", t, q, 1, 0, *a, 0.5, st)


# ------------------------------------------------------------------------------------------ 6-8. through the model
def _model():
    from test_gpu_model import _seeded_model
    return _seeded_model("n").train()


def _batches(n, seed):
    from datasets.synthetic import synth_batch
    return [{k: v.cuda() for k, v in synth_batch(2, 128, seed=seed + i).items()} for i in range(n)]


def _step(m, crit, opt, b):
    opt.zero_grad(set_to_none=True)
    loss, _ = crit(m(b["img"]), b)
    loss.backward()
    opt.step()


def _floats(sd):
    return {k: v for k, v in sd.items() if v.is_floating_point()}


def test_model_training_steps_with_attached_ema():
    """YOLOv11-n (nc 5, 1 plane), batch 2 at 128 x 128, 3 steps with the EMA inside FusedAdamW.step: every EMA
    parameter (the frozen DFL projection too) and every BatchNorm statistic follows the rule teacher-forced,
    num_batches_tracked is the model's once the state is read, and the raw parameters are those of the same steps
    without an EMA, bit for bit."""
    from losses import v8DetectionLoss
    from yolomi.ema import ModelEMA
    from yolomi.optim import FusedAdamW
    m1 = _model()
    m2 = copy.deepcopy(m1)
    ema = ModelEMA(m1, decay=0.99, tau=3.0)
    o1 = FusedAdamW(m1.parameters(), lr=1e-3, weight_decay=5e-4, max_grad_norm=10.0)
    o2 = FusedAdamW(m2.parameters(), lr=1e-3, weight_decay=5e-4, max_grad_norm=10.0)
    o1.attach_ema(ema)
    c1, c2 = v8DetectionLoss(m1), v8DetectionLoss(m2)
    for i, b in enumerate(_batches(3, 70)):
        prev = {k: v.clone() for k, v in _floats(ema.ema.state_dict()).items()}
        _step(m1, c1, o1, b)
        _step(m2, c2, o2, b)
        torch.cuda.synchronize()
        assert ema.updates == i + 1
        src, got = m1.state_dict(), ema.ema.state_dict()
        assert any("running_mean" in k for k in prev) and "model.23.dfl.conv.weight" in prev
        _check_rule(list(prev.values()), [src[k] for k in prev], [got[k] for k in prev], 1.0 - ema.decay_at(i + 1),
                    f"step {i}")
        moved = [k for k in prev if not torch.equal(got[k], prev[k])]
        assert len(moved) > 0.9 * len(prev), len(moved)
    nbt = "model.0.bn.num_batches_tracked"
    n0 = int(ema.ema.state_dict()[nbt])                      # not averaged and not copied per step
    assert int(m1.state_dict()[nbt]) == n0 + 3
    sd = ema.state_dict()
    assert sd["ema_updates"] == 3
    for k, v in m1.state_dict().items():
        if not v.is_floating_point():
            assert torch.equal(sd["ema_state_dict"][k], v), k
    for (k, a), b in zip(m1.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(a, b), k
    assert not ema.ema.training and m1.training
    assert not any(k.startswith("_ym_") for mod in ema.ema.modules() for k in mod.__dict__)     # never ran a forward


def test_eval_plan_reads_the_ema_updated_in_place():
    """The averaged copy runs through the graph-replayed eval path while it is updated in place: its output after
    two more training steps is the output of a fresh model loaded from the EMA state, bit for bit, and not the
    earlier output."""
    from losses import v8DetectionLoss
    from yolomi.ema import ModelEMA
    from yolomi.optim import FusedAdamW
    m = _model()
    ema = ModelEMA(m, decay=0.99, tau=3.0)
    opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=5e-4, max_grad_norm=10.0)
    opt.attach_ema(ema)
    crit = v8DetectionLoss(m)
    bs = _batches(4, 80)
    img = bs[3]["img"]
    _step(m, crit, opt, bs[0])
    with torch.no_grad():
        for _ in range(3):                                   # eager, capture, replay
            y1 = ema.ema(img)[0].clone()
    plan = next(p for k, v in ema.ema.__dict__["_ym_plans"].items() if not k[-1] for p in v)
    assert "fwd" in plan.__dict__.get("_graphs", {}), "the eval forward of the EMA copy was not captured"
    assert "_ym_plans" in m.__dict__ and m.__dict__["_ym_plans"] is not ema.ema.__dict__["_ym_plans"]
    for b in bs[1:3]:
        _step(m, crit, opt, b)
    with torch.no_grad():
        y2 = ema.ema(img)[0].clone()
    fresh = _model()
    fresh.load_state_dict(ema.state_dict()["ema_state_dict"])
    fresh.eval()
    with torch.no_grad():
        want = fresh(img)[0]
    torch.cuda.synchronize()
    assert torch.equal(y2, want)
    assert not torch.equal(y2, y1)


def test_train_one_epoch_updates_the_ema_with_a_plain_optimizer():
    """torch.optim.AdamW has no fused EMA: train_one_epoch calls ema.update() once per step (one ym_ema_update over
    everything), and each update follows the rule."""
    import train_yolo11_cuda as T
    from losses import v8DetectionLoss
    from yolomi.ema import ModelEMA
    m = _model()
    ema = ModelEMA(m, decay=0.99, tau=3.0)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=5e-4)
    inner, seen = ema.update, []

    def checked_update():
        prev = {k: v.clone() for k, v in _floats(ema.ema.state_dict()).items()}
        inner()
        torch.cuda.synchronize()
        src, got = m.state_dict(), ema.ema.state_dict()
        _check_rule(list(prev.values()), [src[k] for k in prev], [got[k] for k in prev],
                    1.0 - ema.decay_at(ema.updates), f"update {ema.updates}")
        seen.append(ema.updates)
    ema.update = checked_update
    T.train_one_epoch(m, T._SyntheticLoader(3, 2, 128, seed=90), opt, v8DetectionLoss(m), torch.device("cuda"), 1, 1,
                      ema=ema)
    assert seen == [1, 2, 3] and ema.updates == 3
    a, b = _floats(ema.ema.state_dict()), m.state_dict()
    assert not any(torch.equal(v, b[k]) for k, v in a.items() if "conv.weight" in k and "dfl" not in k)


# ------------------------------------------------------------------------------------------ 9. the entry point
def test_main_synthetic_with_ema_checkpoint_and_resume(tmp_path):
    script = ROOT / "yolo-scratch_amd" / "train_yolo11_cuda.py"
    args = [sys.executable, str(script), "--synthetic", "2", "--scale", "n", "--imgsz", "128", "--batch", "2", "--ema",
            "--save-dir", str(tmp_path), "--val-conf", "0.001"]
    r = subprocess.run(args + ["--epochs", "1", "--resume", str(tmp_path / "none.pt")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    ck = torch.load(tmp_path / "last.pt", map_location="cpu", weights_only=True)
    assert list(ck)[-2:] == ["ema_state_dict", "ema_updates"] and ck["ema_updates"] == 2
    assert list(ck["ema_state_dict"]) == list(ck["model_state_dict"])
    w = "model.0.conv.weight"
    assert not torch.equal(ck["ema_state_dict"][w], ck["model_state_dict"][w])
    r = subprocess.run(args + ["--epochs", "2", "--resume", str(tmp_path / "last.pt")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Resumed from epoch 1" in r.stdout and "Epoch 2/2" in r.stdout
    ck2 = torch.load(tmp_path / "last.pt", map_location="cpu", weights_only=True)
    assert ck2["epoch"] == 1 and ck2["ema_updates"] == 4
    assert not torch.equal(ck2["ema_state_dict"][w], ck["ema_state_dict"][w])
