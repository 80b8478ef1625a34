#!/usr/bin/env python3
"""What global-norm clipping costs, on the benchmarked arena: configs[1], M1 with context, 10 263 028 floats
(the parameter, gradient and Adam arenas are independent of the batch; the plan is the B = 16 one bench.py runs).

Arms (one call each; the gradient arena holds N(0, 1e-3) floats, so clip_norm = 0.1 x its norm clips every call):
  adam          wun_adam_step                       p, m, v read + written, g read: 28 B / float
  grad_norm     wun_grad_norm (select = NULL)       g read once: 4 B / float (+ the one-workgroup finish)
  adam_clip     wun_adam_step_clip, clipping active  grad_norm + the clipped Adam: 32 B / float
The clipped Adam kernel alone is estimated as adam_clip - grad_norm.

  python tools/clip_cost.py [--rounds 7] [--iters 50]
      HIP events on the launch stream around `iters` back-to-back calls of one arm; the arms interleaved for `rounds` rounds
      (order rotated each round); per arm the minimum over the rounds of (time / iters).  One JSON line on stdout.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ARMS = ["adam", "grad_norm", "adam_clip"]
BYTES_PER_FLOAT = {"adam": 28.0, "grad_norm": 4.0, "adam_clip": 32.0}


def setup():
    import numpy as np
    import torch
    import wave_u_net_amd as wun
    from wave_u_net_amd.separator import UnetAudioSeparator
    cfg = wun.get_config("m1_context")
    sep = UnetAudioSeparator(cfg, device="cuda:0")
    i, _ = sep.get_padding(np.array([16, cfg["num_frames"], 0]))
    sep._active = sep._plan(16, int(i[1]))
    sep._ensure_variables(sep._active)
    n = int(sep._active.info.arena_floats)
    gen = torch.Generator(device="cuda").manual_seed(5)
    sep.grads.copy_(torch.randn(n, generator=gen, device="cuda") * 1e-3)
    lib, h = sep._lib, sep._active.handle
    ws, skipped = sep._norm_buffers()
    rc = lib.wun_grad_norm(h, sep.grads.data_ptr(), 1.0, ws.data_ptr(), sep._stream(), None, 0)
    if rc:
        raise RuntimeError("wun_grad_norm: rc %d: %s" % (rc, lib.wun_last_error().decode()))
    clip = 0.1 * float(ws[len(sep._active.tensors)].item())
    p, g, m, v = (t.data_ptr() for t in (sep.params, sep.grads, sep.adam_m, sep.adam_v))

    def call(arm):
        st = sep._stream()
        if arm == "adam":
            rc = lib.wun_adam_step(h, p, g, m, v, 1, 1e-4, 0.9, 0.999, 1e-8, 1.0, st)
        elif arm == "grad_norm":
            rc = lib.wun_grad_norm(h, g, 1.0, ws.data_ptr(), st, None, 0)
        else:
            rc = lib.wun_adam_step_clip(h, p, g, m, v, 1, 1e-4, 0.9, 0.999, 1e-8, 1.0, clip, 1, ws.data_ptr(),
                                        skipped.data_ptr(), st, None, 0)
        if rc:
            raise RuntimeError("%s: rc %d: %s" % (arm, rc, lib.wun_last_error().decode()))
    return torch, call, n, clip


def timed(rounds, iters):
    torch, call, n, clip = setup()
    for arm in ARMS:                                              # warm-up
        for _ in range(5):
            call(arm)
    torch.cuda.synchronize()
    best = {a: float("inf") for a in ARMS}
    allr = {a: [] for a in ARMS}
    for r in range(rounds):
        order = ARMS[r % len(ARMS):] + ARMS[:r % len(ARMS)]
        for arm in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                call(arm)
            e1.record()
            e1.synchronize()
            us = 1e3 * e0.elapsed_time(e1) / iters
            allr[arm].append(round(us, 2))
            best[arm] = min(best[arm], us)
    gbs = {a: round(BYTES_PER_FLOAT[a] * n / (best[a] * 1e-6) / 1e9, 1) for a in ARMS}
    print(json.dumps({"what": "us per call (min over rounds); GB/s = bytes per float x arena floats / time",
                      "arena_floats": n, "clip_norm": clip, "rounds": rounds, "iters": iters,
                      "min_us": {a: round(best[a], 2) for a in ARMS}, "gb_per_s": gbs,
                      "adam_clip_minus_grad_norm_us": round(best["adam_clip"] - best["grad_norm"], 2),
                      "rounds_us": allr}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    timed(a.rounds, a.iters)


if __name__ == "__main__":
    main()
