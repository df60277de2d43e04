"""Exported module classes called on their own, against the reference (tests/golden/modules.npz, made by
running it — gen_golden.py gen_modules):

* Attention.forward (models/yolo11_modules.py:124-136) at heads=4 (the PSA shape, N=400) and at the
  class default heads=8: train-mode output, input gradient, parameter gradients and BN running
  statistics — the 16-bit conv path's block tolerances (1e-2 output, 2e-2 gradients);
* DFL.forward (:189-192) with its arange weights and with Kaiming weights (Q5): output within 1e-5,
  input gradient within 1e-5 (fp32 softmax + 16-tap projection);
* TaskAlignedAssigner with the class defaults alpha=1.0, beta=6.0 (losses/yolo_v8_loss.py:67):
  fg_mask / target_gt_idx / labels / boxes bit-exact, target_scores within 1e-5.
"""
import numpy as np
import pytest
import torch

from test_gpu_model import rel

pytestmark = pytest.mark.gpu

ATTN = {"attn_h4": (256, 4, (2, 256, 20, 20), 71), "attn_h8": (512, 8, (1, 512, 10, 12), 72)}


@pytest.mark.parametrize("name", sorted(ATTN))
def test_attention_standalone_vs_reference(golden, name):
    from models import Attention
    from oracle.weights import apply_seeded_weights
    d = golden("modules.npz")
    dim, heads, shape, seed = ATTN[name]
    mod = Attention(dim, num_heads=heads, attn_ratio=0.5)
    apply_seeded_weights(mod.state_dict())
    for m in mod.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eps, m.momentum = 1e-3, 0.03
    mod = mod.cuda().train()
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    dy = torch.randn(shape, generator=torch.Generator().manual_seed(seed + 100))      # y has x's shape
    xg = x.cuda().requires_grad_(True)
    y = mod(xg)
    y.backward(dy.cuda())
    assert rel(y.detach().cpu(), d[f"{name}/y"]) < 1e-2
    assert rel(xg.grad.cpu(), d[f"{name}/dx"]) < 2e-2
    named = dict(mod.named_parameters())
    for k, p in named.items():
        if f"{name}/g:{k}" in d.files:
            ref = d[f"{name}/g:{k}"]
            sib = k.replace("bn.bias", "bn.weight")
            if k.endswith("bn.bias") and np.linalg.norm(ref) < 1e-4 * np.linalg.norm(d[f"{name}/g:{sib}"]):
                # pe.bn.bias: pe's output reaches the loss only through proj's conv + TRAIN-mode BN, which
                # removes any per-channel constant, so its gradient is 0 in exact arithmetic (the reference's
                # 1.6e-4 is fp32 noise); the HIP path's is 16-bit noise: bounded against the BN's weight grad
                assert float(p.grad.norm()) < 1e-2 * np.linalg.norm(d[f"{name}/g:{sib}"]), k
                continue
            assert rel(p.grad.cpu(), ref) < 2e-2, k
        else:
            g = p.grad.detach().reshape(-1).cpu()
            step = max(1, g.numel() // 16384)
            assert rel(g[::step][:16384], d[f"{name}/gfp:{k}"]) < 2e-2, k
            assert abs(float(g.double().norm()) / float(d[f"{name}/gn:{k}"]) - 1) < 2e-2, k
    for k, v in mod.state_dict().items():
        if "running" in k:
            assert rel(v.cpu(), d[f"{name}/s:{k}"]) < 1e-2, k


def test_attention_unsupported_head_dim_raises():
    """Attention(256) with the default 8 heads has head_dim 32: the attention kernel is specialised for
    key_dim 32 / head_dim 64 (the only shape the YOLOv11 graph builds, heads = c // 64) and says so."""
    from models import Attention
    from yolomi import YolomiError
    mod = Attention(256).cuda().train()
    with pytest.raises(YolomiError, match="key_dim=32, head_dim=64"):
        mod(torch.randn(1, 256, 4, 4, device="cuda"))


def test_block_second_backward_without_zero_grad_accumulates():
    """Two forward + backward passes through one block plan without zero_grad(): each parameter's .grad is the sum
    of the two gradients taken separately (as autograd accumulates, and as the whole-model and Detect plans do).
    The sum is formed once in fp32, so the bound is this file's gradient tolerance."""
    from models import Conv
    torch.manual_seed(3)
    mod = Conv(8, 16, 3).cuda().train()
    xs = [torch.randn(2, 8, 16, 16, generator=torch.Generator().manual_seed(s)).cuda() for s in (11, 12)]
    dys = [torch.randn(2, 16, 16, 16, generator=torch.Generator().manual_seed(s)).cuda() for s in (21, 22)]
    state = {k: v.clone() for k, v in mod.state_dict().items()}
    single = []
    for x, dy in zip(xs, dys):
        mod.load_state_dict(state)                  # the same running statistics for every pass
        mod.zero_grad(set_to_none=True)
        mod(x).backward(dy)
        single.append({k: p.grad.clone() for k, p in mod.named_parameters()})
    mod.load_state_dict(state)
    mod.zero_grad(set_to_none=True)
    for x, dy in zip(xs, dys):
        mod(x).backward(dy)
    for k, p in mod.named_parameters():
        assert rel(p.grad, single[0][k] + single[1][k]) < 2e-2, k


@pytest.mark.parametrize("name", ["dfl_arange", "dfl_kaiming"])
def test_dfl_standalone_vs_reference(golden, name):
    from models import DFL
    d = golden("modules.npz")
    mod = DFL(16)
    with torch.no_grad():
        mod.conv.weight.copy_(torch.from_numpy(d[f"{name}/w"]).view(1, 16, 1, 1))
    mod = mod.cuda()
    x = torch.from_numpy(d[f"{name}/x"]).cuda().requires_grad_(True)
    y = mod(x)
    assert y.shape == (2, 4, 300)
    torch.testing.assert_close(y.detach().cpu(), torch.from_numpy(d[f"{name}/y"]), rtol=1e-5, atol=1e-5)
    y.backward(torch.from_numpy(d[f"{name}/dy"]).cuda())
    # fp32 softmax backward: the sum over bins cancels against w_j * dy (up to 15 x |dy|), so the absolute
    # bound is the output's 1e-5; relative-L2 over the whole gradient 1e-5
    torch.testing.assert_close(x.grad.cpu(), torch.from_numpy(d[f"{name}/dx"]), rtol=1e-5, atol=1e-5)
    assert rel(x.grad.cpu(), d[f"{name}/dx"]) < 1e-5
    with torch.no_grad():                     # no-grad path: same kernel, same values
        assert torch.equal(mod(x.detach()), y.detach())


def test_task_aligned_assigner_class_defaults_vs_reference(golden):
    from losses import TaskAlignedAssigner
    a, d = golden("assigner.npz"), golden("modules.npz")
    ins = [torch.from_numpy(a["as_" + k]).cuda() for k in
           ("pd_scores", "pd_bboxes", "anc_points", "gt_labels", "gt_bboxes", "mask_gt")]
    tal = TaskAlignedAssigner(num_classes=5)
    assert [tal.alpha, tal.beta, tal.eps] == d["tal_default/params"].tolist()
    tl, tb, ts, fg, tgi = tal(*ins)
    np.testing.assert_array_equal(fg.cpu().numpy(), d["tal_default/fg_mask"])
    np.testing.assert_array_equal(tgi.cpu().numpy(), d["tal_default/target_gt_idx"])
    np.testing.assert_array_equal(tl.cpu().numpy(), d["tal_default/target_labels"])
    np.testing.assert_array_equal(tb.cpu().numpy(), d["tal_default/target_bboxes"])
    torch.testing.assert_close(ts.cpu(), torch.from_numpy(d["tal_default/target_scores"]), rtol=1e-5, atol=1e-6)
