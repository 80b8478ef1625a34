"""Worker of tests/test_gpu_optim_dp.py: one rank of a data-parallel run with decoupled weight decay, an EMA of the weights and
a learning-rate schedule (per-rank batch 6).  Launched by torch.distributed.run; every rank writes its four arenas."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dp_worker                                      # noqa: E402  (also puts the repository root on sys.path)
from wave_u_net_amd import training                  # noqa: E402

PER_RANK = 6
OPTIMIZER = {"weight_decay": 0.05, "ema_decay": 0.9, "ema_warmup": True}
SCHEDULE = {"warmup_steps": 2, "kind": "cosine", "total_steps": 8, "min_factor": 0.1}


def make_cfg(batch):
    return dict(dp_worker.make_cfg(), batch_size=batch, optimizer=OPTIMIZER, lr_schedule=SCHEDULE)


def main():
    out, steps = sys.argv[1], int(sys.argv[2])
    cfg = make_cfg(PER_RANK)
    tr = training.Trainer(cfg)
    assert tr.optimizer["ema_decay"] == 0.9 and tr.lr_schedule["total_steps"] == 8
    mix, targets = dp_worker.global_batch(cfg, tr.t_in, tr.t_out, tr.batch * tr.world)
    lo = tr.rank * tr.batch
    mix = mix[lo:lo + tr.batch].to(tr.device).contiguous()
    targets = targets[:, lo:lo + tr.batch].to(tr.device).contiguous()
    lrs = []
    for _ in range(steps):
        tr.step(mix, targets)
        lrs.append(tr.last_lr)
    torch.cuda.synchronize()
    np.savez("%s.rank%d.npz" % (out, tr.rank), params=tr.sep.params.cpu().numpy(), m=tr.sep.adam_m.cpu().numpy(),
             v=tr.sep.adam_v.cpu().numpy(), ema=tr.sep.ema.cpu().numpy(), lrs=np.array(lrs), world=tr.world)
    if tr.world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
