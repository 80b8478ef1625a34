"""Data-parallel training with the extended optimizer: two ranks on the one GPU (gloo), 3 steps with decoupled
weight decay, an EMA of the weights and a warm-up + cosine schedule.  The EMA is computed on every rank from identical bits --
no collective is added -- so params, m, v and ema are bit-identical across the ranks, and equal to one process on the
concatenated batch within the tolerance of test_data_parallel_gpu.py."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
DP_TOL = 2e-5                          # x max(1, max|p|): the tolerance of test_data_parallel_gpu.py


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_two_ranks_decay_ema_schedule_equal_one_process(tmp_path):
    import dp_optim_worker
    import dp_worker
    from wave_u_net_amd import training
    steps = 3
    out = os.path.join(str(tmp_path), "dp_optim")
    env = dict(os.environ, WUN_DIST_BACKEND="gloo", WUN_NO_TUNE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "dp_optim_worker.py"), out, str(steps)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r0, r1 = np.load(out + ".rank0.npz"), np.load(out + ".rank1.npz")
    assert int(r0["world"]) == 2
    for k in ("params", "m", "v", "ema", "lrs"):
        assert np.array_equal(r0[k].view(np.int32 if r0[k].dtype == np.float32 else np.int64),
                              r1[k].view(np.int32 if r1[k].dtype == np.float32 else np.int64)), k
    want_lrs = [training.scheduled_lr(1e-3, dp_optim_worker.SCHEDULE, s) for s in range(steps)]
    assert list(r0["lrs"]) == want_lrs and len(set(want_lrs)) > 1            # the schedule moved the lr
    assert not np.array_equal(r0["ema"], r0["params"])                       # the EMA lags the weights
    cfg = dp_optim_worker.make_cfg(12)
    tr = training.Trainer(cfg)
    mix, targets = dp_worker.global_batch(cfg, tr.t_in, tr.t_out, 12)
    mix, targets = mix.to(tr.device), targets.to(tr.device)
    for _ in range(steps):
        tr.step(mix, targets)
    torch.cuda.synchronize()
    for k, t in (("params", tr.sep.params), ("ema", tr.sep.ema)):
        ref = t.cpu().numpy()
        assert np.abs(r0[k] - ref).max() <= DP_TOL * max(1.0, np.abs(ref).max()), k
