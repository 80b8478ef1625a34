#!/usr/bin/env python3
"""What the extended optimizer costs, on the arenas of the headline plan (BASELINE.json configs[1], M1 with
context, B = 16) and of deep_l16_f48 (the arenas do not depend on the batch: that plan is built for one excerpt).

Arms (one optimizer step each; the gradient arena holds N(0, 1e-3) floats, clip_norm = 0.1 x its norm clips every call):
  a0 adam             wun_adam_step: no norm                                  28 B / float
  a  adam_clip        wun_adam_step_clip                                      32 B / float (norm 4 + Adam 28)
  b  optim_off        wun_optim_step, weight_decay 0, no EMA                  32 B / float
  c  optim_on         wun_optim_step, weight decay on every tensor + EMA      40 B / float (norm 4 + the fused pass 36)
  c2 optim_kernels    as c, decay on the conv kernels only (adam_step's default decay_variables): one run per tensor
  d  unfused          a, then params.mul_(1 - lr wd) and ema.lerp_(params, 1 - d) with torch: what c replaces
                      (32 + 8 + 12 = 52 B / float)
(c)'s fused pass alone is estimated as c - grad_norm (wun_grad_norm timed as arm n) at 36 B / float, against the measured HBM
rate of the micro-architecture guide (6.29 TB/s, float4 copy).

  python tools/optim_bench.py [--rounds 7] [--iters 30] [--out profiles/optim_bench.json]
      HIP events on the launch stream around `iters` back-to-back calls of one arm; the arms interleaved for `rounds` rounds
      (order rotated each round); per arm the median over the rounds of (time / iters), with min .. max.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ARMS = ["adam", "adam_clip", "optim_off", "optim_on", "optim_kernels", "unfused", "grad_norm"]
HBM_TBS = 6.29
LR, WD, EMA_D = 1e-4, 0.01, 0.999


def setup(name, batch):
    import numpy as np
    import torch
    import wave_u_net_amd as wun
    from wave_u_net_amd import _lib
    from wave_u_net_amd.separator import UnetAudioSeparator
    cfg = wun.get_config(name)
    sep = UnetAudioSeparator(cfg, device="cuda:0")
    i, _ = sep.get_padding(np.array([batch, cfg["num_frames"], 0]))
    sep._active = sep._plan(batch, int(i[1]))
    sep._ensure_variables(sep._active)
    n = int(sep._active.info.arena_floats)
    gen = torch.Generator(device="cuda").manual_seed(5)
    sep.grads.copy_(torch.randn(n, generator=gen, device="cuda") * 1e-3)
    ema = sep._ensure_ema()
    lib, h = sep._lib, sep._active.handle
    ws, skipped = sep._norm_buffers()
    _lib.check(lib.wun_grad_norm(h, sep.grads.data_ptr(), 1.0, ws.data_ptr(), sep._stream(), None, 0))
    clip = 0.1 * float(ws[len(sep._active.tensors)].item())
    p, g, m, v = (t.data_ptr() for t in (sep.params, sep.grads, sep.adam_m, sep.adam_v))
    kernels = sep.decay_mask(None)
    kptr = kernels.ctypes.data_as(C.POINTER(C.c_uint8))
    off = _lib.WunOptimConfig(0.9, 0.999, 1e-8, 0.0, 0.0, clip, 1)
    on = _lib.WunOptimConfig(0.9, 0.999, 1e-8, WD, EMA_D, clip, 1)
    factor, w = float(np.float32(1.0 - LR * WD)), float(np.float32(1.0 - float(np.float32(EMA_D))))

    def call(arm):
        st = sep._stream()
        if arm == "adam":
            _lib.check(lib.wun_adam_step(h, p, g, m, v, 1, LR, 0.9, 0.999, 1e-8, 1.0, st))
        elif arm in ("adam_clip", "unfused"):
            _lib.check(lib.wun_adam_step_clip(h, p, g, m, v, 1, LR, 0.9, 0.999, 1e-8, 1.0, clip, 1, ws.data_ptr(),
                                              skipped.data_ptr(), st, None, 0))
            if arm == "unfused":
                sep.params.mul_(factor)
                ema.lerp_(sep.params, w)
        elif arm == "grad_norm":
            _lib.check(lib.wun_grad_norm(h, g, 1.0, ws.data_ptr(), st, None, 0))
        elif arm == "optim_off":
            _lib.check(lib.wun_optim_step(h, p, g, m, v, None, 1, LR, 1.0, C.byref(off), ws.data_ptr(), skipped.data_ptr(), st,
                                          None, 0, None, 0))
        else:
            dec = (kptr, int(kernels.size)) if arm == "optim_kernels" else (None, 0)
            _lib.check(lib.wun_optim_step(h, p, g, m, v, ema.data_ptr(), 1, LR, 1.0, C.byref(on), ws.data_ptr(),
                                          skipped.data_ptr(), st, None, 0, *dec))
    return torch, call, n, len(sep._active.tensors)


def timed(name, batch, rounds, iters):
    torch, call, n, nt = setup(name, batch)
    for arm in ARMS:                                              # warm-up
        for _ in range(5):
            call(arm)
    torch.cuda.synchronize()
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
            allr[arm].append(1e3 * e0.elapsed_time(e1) / iters)
    med = {a: statistics.median(allr[a]) for a in ARMS}
    fused_us = med["optim_on"] - med["grad_norm"]
    tbs = 36.0 * n / (fused_us * 1e-6) / 1e12
    return {"plan": name, "arena_floats": n, "tensors": nt,
            "us": {a: {"median": round(med[a], 2), "min": round(min(allr[a]), 2), "max": round(max(allr[a]), 2)} for a in ARMS},
            "optim_off_over_adam_clip": round(med["optim_off"] / med["adam_clip"], 4),
            "optim_on_over_unfused": round(med["optim_on"] / med["unfused"], 4),
            "fused_pass_us": round(fused_us, 2), "fused_pass_tb_per_s_at_36_bytes": round(tbs, 3),
            "fraction_of_measured_hbm_rate": round(tbs / HBM_TBS, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
    a = ap.parse_args()
    res = {"what": "us per optimizer step: median over interleaved rounds (min .. max); HIP events around `iters` calls",
           "rounds": a.rounds, "iters": a.iters, "hbm_tb_per_s_measured_guide": HBM_TBS,
           "plans": [timed("m1_context", 16, a.rounds, a.iters), timed("deep_l16_f48", 1, a.rounds, a.iters)]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
