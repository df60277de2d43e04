"""The top-k task-aligned assigner on the GPU (ym_tal_assign_topk, ym_loss_fwd_topk) against its numpy
restatement (tests/tal_topk_ref.py, held to hand-worked answers by tests/test_tal_topk_cpu.py): the explicit entry
exactly, the fused loss through the CPU oracle's v8_loss with the restatement as its assigner, and the trainer."""
import numpy as np
import pytest
import torch

import tal_topk_cases as tc
import tal_topk_ref as tr

pytestmark = pytest.mark.gpu

GAP = 1e-4            # smallest relative gap a ranking may rest on: ten times the 1e-5 the scores are compared at
FUSED_SEEDS = {1: 101, 17: 117}      # (batch, head-map) seeds whose reference rankings keep GAP (asserted below)
# (nc, B, imgsz, seed): the two class counts at 256 px (A = 1344: two LDS chunks of the selection kernel), and one
# image at 640 px (A = 8400, the benchmark's anchor count: nine chunks; seed 106 is the first from 105 whose 19 boxes
# include one with fewer than k in-box anchors)
FUSED_CASES = [(1, 3, 256, FUSED_SEEDS[1]), (17, 3, 256, FUSED_SEEDS[17]), (5, 1, 640, 106)]


@pytest.fixture(scope="module")
def case():
    return tc.explicit_case()


@pytest.mark.parametrize("k", [1, 3, 10])
def test_explicit_entry_exact(case, k):
    """TaskAlignedAssigner(use_topk=True) at alpha = beta = 1, where every quantity is reproducible in fp32: fg, tgi and
    the labels equal the restatement's exactly, the scores within rtol 1e-5 / atol 1e-6 (tests/test_gpu_model.py's
    bound for the score magnitude); the hand-worked anchors carry their written-out answers.  B = 2, A = 441 (no
    multiple of 64 or 256), M = 6 with an invalid slot, duplicated prediction rows."""
    from losses.yolo_v8_loss import TaskAlignedAssigner
    ref = tr.assign(case["scores"], case["boxes"], case["anc"], case["labels"], case["gboxes"], case["mask"], k, 1.0,
                    1.0, 1e-9)
    asg = TaskAlignedAssigner(topk=k, num_classes=tc.NC, alpha=1.0, beta=1.0, use_topk=True)
    d = {n: torch.from_numpy(case[n]).cuda() for n in ("scores", "boxes", "anc", "labels", "gboxes", "mask")}
    t_lab, t_box, t_sc, fg, tgi = asg(d["scores"], d["boxes"], d["anc"], d["labels"], d["gboxes"], d["mask"])
    torch.cuda.synchronize()
    want_fg = np.stack([r["fg"] for r in ref])
    want_tgi = np.stack([r["tgi"] for r in ref])
    want_norm = np.stack([r["norm"] for r in ref])
    assert fg.dtype == torch.bool and tgi.dtype == torch.int64
    np.testing.assert_array_equal(fg.cpu().numpy(), want_fg)
    np.testing.assert_array_equal(tgi.cpu().numpy(), want_tgi)
    rows = np.arange(2)[:, None]
    want_lab = case["labels"][rows, want_tgi]
    np.testing.assert_array_equal(t_lab.cpu().numpy(), want_lab)
    np.testing.assert_array_equal(t_box.cpu().numpy(), case["gboxes"][rows, want_tgi])
    want_sc = np.zeros((2, tc.A, tc.NC), np.float32)
    np.put_along_axis(want_sc, want_lab.astype(np.int64)[..., None], (want_norm * want_fg)[..., None], 2)
    np.testing.assert_allclose(t_sc.cpu().numpy(), want_sc, rtol=1e-5, atol=1e-6)
    got_norm = t_sc.sum(-1).cpu().numpy()
    for b in range(2):
        for a in range(tc.NH):
            w = tc.HAND[k][b].get(a)
            if w is None:
                assert not fg[b, a] and tgi[b, a] == 0 and got_norm[b, a] == 0, (b, a)
            else:
                assert fg[b, a] and tgi[b, a] == w[0] and got_norm[b, a] == np.float32(w[1]), (b, a, got_norm[b, a])
    assert int(fg.sum()) <= k * int(case["mask"].sum())


def test_topk_out_of_range_is_refused(case):
    from losses.yolo_v8_loss import TaskAlignedAssigner
    from yolomi._lib import YolomiError
    d = {n: torch.from_numpy(case[n]).cuda() for n in ("scores", "boxes", "anc", "labels", "gboxes", "mask")}
    for k in (0, 65):
        asg = TaskAlignedAssigner(topk=k, num_classes=tc.NC, alpha=1.0, beta=1.0, use_topk=True)
        with pytest.raises(YolomiError, match="topk"):
            asg(d["scores"], d["boxes"], d["anc"], d["labels"], d["gboxes"], d["mask"])
        crit, fd, batch = _fused_setup(1, FUSED_SEEDS[1], tal_topk=k)
        with pytest.raises(YolomiError, match="topk"):
            crit(fd, batch)


def _stub(nc):
    import torch.nn as nn
    from models import Detect

    class Stub(nn.Module):
        def __init__(self):
            super().__init__()
            self.det = Detect(nc, (64, 128, 256))
            self.det.stride = torch.tensor([8.0, 16.0, 32.0])
    return Stub().cuda()


def fused_inputs(nc, seed, B=3, imgsz=256):
    """Random head maps and synth_batch targets, as tests/test_gpu_loss_nc.py builds them (CPU tensors)."""
    from datasets.synthetic import synth_batch
    b = synth_batch(B, imgsz, seed=seed, nc=nc)
    batch = {k: b[k] for k in ("batch_idx", "cls", "bboxes")}
    g = torch.Generator().manual_seed(seed)
    feats = [torch.randn(B, 64 + nc, imgsz // s, imgsz // s, generator=g) * 2.0 for s in (8, 16, 32)]
    return feats, batch


def _fused_setup(nc, seed, tal_topk=10, assigner="topk", stub=None, B=3, imgsz=256):
    from losses import v8DetectionLoss
    feats, batch = fused_inputs(nc, seed, B, imgsz)
    crit = v8DetectionLoss(stub if stub is not None else _stub(nc), tal_topk=tal_topk, assigner=assigner)
    return crit, [f.cuda().requires_grad_(True) for f in feats], {k: v.cuda() for k, v in batch.items()}


@pytest.mark.parametrize("nc,B,imgsz,seed", FUSED_CASES)
def test_fused_loss_vs_oracle(nc, B, imgsz, seed, monkeypatch):
    """v8DetectionLoss(assigner="topk", tal_topk=10) on random head maps (FUSED_CASES) against oracle.loss.v8_loss
    whose `assign` is the restatement: assignment exact, loss and items within 1e-4, head gradients within 1e-3
    (tests/test_gpu_loss_nc.py's bounds).  At alpha 0.5 / beta 4 the rankings go through sqrtf and powf, so the
    reference must not rest on a near-tie: every gt's k-th and (k+1)-th in-box metric and every anchor's two best
    claiming IoUs lie a relative GAP apart."""
    from oracle import loss as ol
    k = 10
    rec = []
    monkeypatch.setattr(ol, "assign", tr.oracle_assign(k, ol.ALPHA, ol.BETA, ol.EPS, record=rec))
    feats, batch = fused_inputs(nc, seed, B, imgsz)
    fr = [f.clone().requires_grad_(True) for f in feats]
    rl, ri, inter = ol.v8_loss(fr, batch, nc=nc, return_internals=True)
    rl.backward()

    gaps = [tr.min_gaps(r, k) for r in rec]
    print("relative gaps (rank, claim) per image:", gaps)
    assert min(g[0] for g in gaps) >= GAP and min(g[1] for g in gaps) >= GAP, gaps
    # the ground the inputs cover
    n_in = np.concatenate([r["inbox"].sum(1) for r in rec])
    assert (n_in > k).any() and ((n_in > 0) & (n_in < k)).any(), n_in
    claims = [np.bincount([a for cg in r["cand"] for a in cg]) for r in rec]
    assert any((c > 1).any() for c in claims)
    n_valid = int(len(batch["cls"]))

    crit, fd, dbatch = _fused_setup(nc, seed, tal_topk=k, B=B, imgsz=imgsz)
    loss, items = crit(fd, dbatch)
    tgi, fg, nm = (t.clone() for t in crit.assignment())
    loss.backward()
    num_fg = float(crit._last.out[5])
    assert 0 < num_fg == float(inter["fg"].sum()) <= k * n_valid

    np.testing.assert_array_equal(fg.cpu().numpy().astype(bool), inter["fg"].numpy())
    fgm = inter["fg"]
    np.testing.assert_array_equal(tgi.cpu()[fgm].numpy(), inter["tgi"][fgm].numpy())
    assert (tgi.cpu()[~fgm] == 0).all() and (nm.cpu()[~fgm] == 0).all()
    torch.testing.assert_close(nm.cpu(), inter["target_scores"].sum(-1), rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(items.cpu(), ri, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(loss.detach().cpu(), rl.detach(), rtol=1e-4, atol=1e-6)
    for a, r in zip(fd, fr):
        torch.testing.assert_close(a.grad.cpu(), r.grad, rtol=1e-3, atol=1e-6)

    # the in-box assigner on the same inputs makes other anchors positive
    crit_in, fd_in, _ = _fused_setup(nc, seed, assigner="inbox", stub=crit.model, B=B, imgsz=imgsz)
    crit_in(fd_in, dbatch)
    fg_in = crit_in.assignment()[1]
    assert not torch.equal(fg_in, fg) and int(fg_in.sum()) > int(fg.sum())


def test_fused_loss_without_targets():
    crit, fd, _ = _fused_setup(1, FUSED_SEEDS[1])
    empty = {"batch_idx": torch.zeros(0, dtype=torch.long, device="cuda"),
             "cls": torch.zeros(0, 1, dtype=torch.long, device="cuda"), "bboxes": torch.zeros(0, 4, device="cuda")}
    loss, items = crit(fd, empty)
    loss.backward()
    tgi, fg, nm = crit.assignment()
    assert int(fg.sum()) == 0 and int(tgi.abs().sum()) == 0 and float(nm.abs().sum()) == 0
    assert torch.isfinite(loss) and torch.isfinite(items).all() and float(loss.detach()) > 0
    assert all(torch.isfinite(f.grad).all() for f in fd)


def test_fused_loss_is_reproducible_and_leaves_the_default_alone():
    """Two runs of forward and backward are bit-identical; the default assigner on the same model after a top-k call
    equals the default assigner before it, bit for bit (tal_topk alone switches nothing on)."""
    nc, seed = 17, FUSED_SEEDS[17]
    stub = _stub(nc)

    def run(**kw):
        crit, fd, batch = _fused_setup(nc, seed, stub=stub, **kw)
        loss, items = crit(fd, batch)
        asg = [t.clone() for t in crit.assignment()]
        loss.backward()
        return [loss.detach().clone(), items.clone(), *asg, *[f.grad.clone() for f in fd]]

    before = run(assigner="inbox", tal_topk=10)
    one = run(assigner="topk", tal_topk=10)
    two = run(assigner="topk", tal_topk=10)
    from losses import v8DetectionLoss
    feats, batch = fused_inputs(nc, seed)
    crit = v8DetectionLoss(stub)                       # the default constructor, after the top-k calls
    fd = [f.cuda().requires_grad_(True) for f in feats]
    loss, items = crit(fd, {k: v.cuda() for k, v in batch.items()})
    asg = [t.clone() for t in crit.assignment()]
    loss.backward()
    after = [loss.detach().clone(), items.clone(), *asg, *[f.grad.clone() for f in fd]]
    for a, b in zip(one, two):
        assert torch.equal(a, b)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    assert not torch.equal(one[3], before[3])          # and the two assigners do differ here

    # one criterion object switched between the modes keeps a workspace per mode
    crit.assign_mode = "topk"
    fd2 = [f.cuda().requires_grad_(True) for f in feats]
    l2, _ = crit(fd2, {k: v.cuda() for k, v in batch.items()})
    assert torch.equal(l2.detach(), one[0])
    crit.assign_mode = "inbox"
    l3, _ = crit([f.cuda() for f in feats], {k: v.cuda() for k, v in batch.items()})
    assert torch.equal(l3.detach(), before[0])


def test_train_one_epoch_with_topk_assigner():
    """Three synthetic steps at 128 px through train_one_epoch with assigner="topk": finite losses, changed weights."""
    import train_yolo11_cuda as T
    from losses import v8DetectionLoss
    from yolomi.optim import FusedAdamW
    from test_gpu_model import _seeded_model
    m = _seeded_model("n").train()
    w0 = {k: v.detach().clone() for k, v in m.named_parameters()}
    opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=5e-4, max_grad_norm=10.0)
    crit = v8DetectionLoss(m, tal_topk=10, assigner="topk")
    got = T.train_one_epoch(m, T._SyntheticLoader(3, 2, 128, seed=70), opt, crit, torch.device("cuda"), 1, 1)
    assert all(np.isfinite(got[k]) for k in ("loss", "box_loss", "cls_loss", "dfl_loss")), got
    assert got["loss"] > 0
    changed = [k for k, v in m.named_parameters() if not torch.equal(v.detach(), w0[k])]
    assert len(changed) > len(w0) // 2, (len(changed), len(w0))
