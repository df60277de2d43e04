"""Worker for tests/test_gpu_ema_dp.py: one rank of a 2-process data-parallel run on ONE GPU (torchrun,
YM_DIST_BACKEND=gloo, YM_DIST_DEVICE=0, as tests/dp_worker.py).  Not a test module (no test_ prefix): the test
launches it.

Per rank, on the YOLOv11-n plan at 128x128: two training steps on the rank's own batches with the gradients
all-reduced (GradSync) and the EMA inside FusedAdamW.step, then GradSync.sync_buffers and ModelEMA.sync_buffers.
Saved for the test: the EMA state before the buffer sync (parameters and BatchNorm statistics apart) and the
EMA state dict after it.
usage: python -m torch.distributed.run --nproc-per-node 2 ... tests/dp_ema_worker.py OUTDIR
"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "yolo-scratch_amd"), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    out = Path(sys.argv[1])
    from dp_worker import seeded
    from yolomi import dist as ydist
    from yolomi.ema import ModelEMA
    from yolomi.optim import FusedAdamW
    from losses import v8DetectionLoss
    from datasets.synthetic import synth_batch
    ctx = ydist.init_from_env()
    assert ctx is not None and ctx.world == 2, "launch with torchrun --nproc-per-node 2"
    rank = ctx.rank
    torch.cuda.set_device(0)
    m = seeded("n")
    crit = v8DetectionLoss(m)
    dp = ydist.GradSync(m, ctx)
    dp.broadcast_state()
    ema = ModelEMA(m, decay=0.99, tau=3.0)
    opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=5e-4, max_grad_norm=10.0)
    opt.attach_ema(ema)
    for step in range(2):
        b = {k: v.cuda() for k, v in synth_batch(2, 128, seed=300 + 10 * rank + step).items()}
        opt.zero_grad(set_to_none=True)
        loss, _ = crit(m(b["img"]), b)
        loss.backward()
        dp.sync()
        opt.step()
    torch.cuda.synchronize()
    params = {k: v.detach().cpu() for k, v in ema.ema.named_parameters()}
    torch.save({"params": params, "buffers": {k: v.cpu() for k, v in ema.ema.named_buffers()}},
               out / f"before_r{rank}.pt")
    dp.sync_buffers()
    ema.sync_buffers(dp)
    torch.cuda.synchronize()
    torch.save({k: (v if isinstance(v, int) else {n: t.cpu() for n, t in v.items()})
                for k, v in ema.state_dict().items()}, out / f"ema_r{rank}.pt")
    import torch.distributed as dist
    dist.barrier()
    ydist.shutdown()


if __name__ == "__main__":
    main()
