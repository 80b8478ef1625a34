"""Worker of tests/test_gpu_grad_accum.py: one rank of a data-parallel run with gradient accumulation (grad_accum_steps = 2,
per-rank batch 6).  Launched by torch.distributed.run; rank 0 writes its parameters after a few steps."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dp_worker                                      # noqa: E402  (also puts the repository root on sys.path)
from wave_u_net_amd import training                  # noqa: E402

PER_RANK, K = 6, 2


def main():
    out, steps = sys.argv[1], int(sys.argv[2])
    cfg = dict(dp_worker.make_cfg(), batch_size=PER_RANK, grad_accum_steps=K)
    tr = training.Trainer(cfg)
    assert tr.accum == K and tr.micro == PER_RANK // K
    mix, targets = dp_worker.global_batch(cfg, tr.t_in, tr.t_out, tr.batch * tr.world)
    lo = tr.rank * tr.batch
    mix = mix[lo:lo + tr.batch].to(tr.device).contiguous()
    targets = targets[:, lo:lo + tr.batch].to(tr.device).contiguous()
    losses = [float(tr.step(mix, targets).item()) for _ in range(steps)]
    torch.cuda.synchronize()
    if tr.rank == 0:
        np.savez(out, params=tr.sep.params.cpu().numpy(), losses=np.array(losses), world=tr.world,
                 overlap=int(tr.overlap))
    if tr.world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
