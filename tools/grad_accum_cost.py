#!/usr/bin/env python3
"""What gradient accumulation costs, on the benchmarked plan: configs[1], M1 with context, 147443 -> 16389
samples, the pinned tuning table imported as bench.py does.

Backward arms (B = 16; one forward pass, training = 1, + one backward call each):
  loss_ex       wun_loss_backward_ex (overwrites the gradient arena)
  loss_acc      wun_loss_backward_accumulate with select = NULL (adds to it: one extra read of the arena per call)
Trainer arms (one optimizer step each, same global batch of 16 per step):
  step_k1       Trainer(batch 16, grad_accum_steps = 1): one B = 16 micro-batch
  step_k2       Trainer(batch 16, grad_accum_steps = 2): two B = 8 micro-batches (B = 8 plan: heuristic tilings -- no pinned
                table exists for it)

  python tools/grad_accum_cost.py [--rounds 7] [--iters 10]
      HIP events on the launch stream around `iters` back-to-back iterations of one arm; the arms interleaved for `rounds`
      rounds (order rotated each round); per arm the minimum over the rounds of (time / iters).  One JSON line on stdout.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ARMS = ["loss_ex", "loss_acc", "step_k1", "step_k2"]


def setup():
    import torch
    import wave_u_net_amd as wun
    from wave_u_net_amd.training import Trainer, synthetic_source
    os.environ["WUN_NO_TUNE"] = "1"                               # (Trainer.tune: only the pinned table below)
    cfg = wun.get_config("m1_context")
    table = open(os.path.join(ROOT, "profiles", "round6_tune_table.txt")).read()
    tr1 = Trainer(cfg, batch_size=16)
    mix, targets = synthetic_source(cfg, 16, tr1.t_in, tr1.t_out, tr1.device, seed=1337)()
    tr1.sep.get_output(mix, True)
    tr1.sep.tune_import(table)
    tr2 = Trainer(cfg, batch_size=16, grad_accum_steps=2)
    sep, lib = tr1.sep, tr1.sep._lib
    tg = targets.to(torch.float32).contiguous()
    loss = torch.empty((), device=mix.device)

    def step(arm):
        if arm == "step_k1":
            tr1.step(mix, targets)
            return
        if arm == "step_k2":
            tr2.step(mix, targets)
            return
        sep.get_output(mix, True)
        ws, outs = sep._ws[sep._last_key].data_ptr(), sep._outs[sep._last_key].data_ptr()
        args = (sep._active.handle, sep.params.data_ptr(), None, ws, outs, tg.data_ptr(), sep.grads.data_ptr(), loss.data_ptr(),
                sep._stream(), None, None, 0)
        rc = lib.wun_loss_backward_ex(*args) if arm == "loss_ex" else lib.wun_loss_backward_accumulate(*args, None, 0)
        if rc:
            raise RuntimeError("%s: rc %d: %s" % (arm, rc, lib.wun_last_error().decode()))
    return torch, step


def timed(rounds, iters):
    torch, step = setup()
    for arm in ARMS:                                              # warm-up
        for _ in range(3):
            step(arm)
    torch.cuda.synchronize()
    best = {a: float("inf") for a in ARMS}
    allr = {a: [] for a in ARMS}
    for r in range(rounds):
        order = ARMS[r % len(ARMS):] + ARMS[:r % len(ARMS)]
        for arm in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                step(arm)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1) / iters
            allr[arm].append(round(ms, 4))
            best[arm] = min(best[arm], ms)
    print(json.dumps({"what": "ms per iteration (min over rounds); loss_*: forward + backward, step_*: one optimizer step",
                      "rounds": rounds, "iters": iters, "min_ms": {a: round(best[a], 4) for a in ARMS}, "rounds_ms": allr}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    timed(a.rounds, a.iters)


if __name__ == "__main__":
    main()
