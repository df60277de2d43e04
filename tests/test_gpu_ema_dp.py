"""The weight EMA under data parallelism at world size 2 (two fresh processes on GPU 0 through gloo, the launcher
of tests/test_gpu_dp_world2.py; worker: tests/dp_ema_worker.py).

Every rank applies the same all-reduced gradient to the same parameters, so the EMA parameters agree bit for bit
without any exchange; the BatchNorm statistics follow each rank's own batches and differ until
ModelEMA.sync_buffers broadcasts rank 0's.  After 2 steps and the sync both ranks hold bit-equal EMA state dicts.
"""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from test_gpu_dp_world2 import _free_port

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def test_ema_state_equal_on_both_ranks_after_sync(tmp_path):
    env = dict(os.environ, YM_DIST_BACKEND="gloo", YM_DIST_DEVICE="0", PYTHONUNBUFFERED="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           str(ROOT / "tests" / "dp_ema_worker.py"), str(tmp_path)]
    # own session: on a time-out the whole group (torchrun and both ranks) is killed, nothing keeps the GPU
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                            start_new_session=True)
    try:
        out, err = proc.communicate(timeout=110)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, 9)
        out, err = proc.communicate()
        pytest.fail(f"2-rank run timed out: {err[-4000:]}")
    assert proc.returncode == 0, (out[-3000:], err[-6000:])
    before = [torch.load(tmp_path / f"before_r{k}.pt", weights_only=True) for k in range(2)]
    for k, v in before[0]["params"].items():                    # no exchange needed for the parameters
        assert torch.equal(v, before[1]["params"][k]), k
    rm = [k for k in before[0]["buffers"] if k.endswith("running_mean")]
    assert rm and any(not torch.equal(before[0]["buffers"][k], before[1]["buffers"][k]) for k in rm)
    ema = [torch.load(tmp_path / f"ema_r{k}.pt", weights_only=True) for k in range(2)]
    assert ema[0]["ema_updates"] == ema[1]["ema_updates"] == 2
    a, b = ema[0]["ema_state_dict"], ema[1]["ema_state_dict"]
    assert list(a) == list(b) and len(a) > 200
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for k in rm:                                                # rank 0's statistics are the ones that count
        assert torch.equal(a[k], before[0]["buffers"][k]), k
