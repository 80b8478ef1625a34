"""Worker of tests/test_gpu_grad_clip.py: one rank of a data-parallel run with global-norm clipping (per-rank batch 6).
Launched by torch.distributed.run; every rank writes its parameters, Adam slots and per-step norms."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dp_worker                                      # noqa: E402  (also puts the repository root on sys.path)
from wave_u_net_amd import training                  # noqa: E402

PER_RANK = 6


def main():
    out, steps, clip = sys.argv[1], int(sys.argv[2]), float(sys.argv[3])
    cfg = dict(dp_worker.make_cfg(), batch_size=PER_RANK, clip_grad_norm=clip)
    tr = training.Trainer(cfg)
    assert tr.clip_norm == clip
    mix, targets = dp_worker.global_batch(cfg, tr.t_in, tr.t_out, tr.batch * tr.world)
    lo = tr.rank * tr.batch
    mix = mix[lo:lo + tr.batch].to(tr.device).contiguous()
    targets = targets[:, lo:lo + tr.batch].to(tr.device).contiguous()
    norms = []
    for _ in range(steps):
        tr.step(mix, targets)
        norms.append(tr.grad_norm.clone())
    torch.cuda.synchronize()
    np.savez("%s.rank%d.npz" % (out, tr.rank), params=tr.sep.params.cpu().numpy(), m=tr.sep.adam_m.cpu().numpy(),
             v=tr.sep.adam_v.cpu().numpy(), norms=torch.stack(norms).cpu().numpy(), world=tr.world)
    if tr.world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
