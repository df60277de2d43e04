"""Worker for tests/test_gpu_metrics_cls.py::test_validate_per_class_world2: one rank of a 2-process
data-parallel run on ONE GPU (torchrun, YM_DIST_BACKEND=gloo, YM_DIST_DEVICE=0, as tests/dp_worker.py).
Not a test module (no test_ prefix): the test launches it.

Per rank, on the YOLOv11-n plan at 256x256: train_yolo11_cuda.validate(per_class=True) under DP (each rank its
own val batches, detections and labels gathered to rank 0, the four metrics and the per-class lists broadcast),
and on rank 0 the same call with dp=None over every rank's batches.  The dicts are saved for the test to compare.
usage: python -m torch.distributed.run --nproc-per-node 2 ... tests/dp_cls_worker.py OUTDIR
"""
import json
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
    from losses import v8DetectionLoss
    import train_yolo11_cuda as T
    ctx = ydist.init_from_env()
    assert ctx is not None and ctx.world == 2, "launch with torchrun --nproc-per-node 2"
    rank = ctx.rank
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    m = seeded("n")
    crit = v8DetectionLoss(m)
    dp = ydist.GradSync(m, ctx)
    dp.broadcast_state()
    dp.sync_buffers()
    vals = [T._SyntheticLoader(2, 2, 256, seed=7000 + 1000 * r) for r in range(2)]
    conf = 1e-7                       # the untrained head scores ~1e-6: keep candidates
    res = {"val_dp": T.validate(m, vals[rank], crit, dev, conf_threshold=conf, dp=dp, per_class=True)}
    if rank == 0:
        class Both:
            def __len__(self):
                return 4

            def __iter__(self):       # the evaluation does not depend on the order of the images
                for r in range(2):
                    yield from vals[r]
        res["val_world1"] = T.validate(m, Both(), crit, dev, conf_threshold=conf, dp=None, per_class=True)
    (out / f"res_r{rank}.json").write_text(json.dumps(res))
    import torch.distributed as dist
    dist.barrier()                    # rank 1 waits for rank 0's world-1 validation before tearing down
    ydist.shutdown()


if __name__ == "__main__":
    main()
