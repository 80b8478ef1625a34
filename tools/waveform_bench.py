#!/usr/bin/env python3
"""What the waveform losses cost, on two shapes: the headline plan's outputs (S = 2, B = 16, Tout = 16389,
C = 1) and a bandwidth shape (S = 2, B = 4, Tout = 589824, C = 2: the deep config's excerpt).  Estimates = targets + noise.

Arms (HIP events on the launch stream around `iters` back-to-back calls, each with d_outputs):
  spectral_mse  wun_spectral_loss at nres = 0, mse_weight 1: the yardstick (two launches)
  wave_mse      wun_waveform_loss {mse: 1}: the same two launches over the same bytes, the same bits
  wave_l1_mse   {mse: 1, l1: 1}
  wave_sisdr    {si_sdr: 1}: the row sums and row scalars before the gradient (four launches)
  wave_all      {mse: 1, l1: 1, si_sdr: 1, snr: 1}
  torch_all     wave_all's total written in eager torch with backward(): what a user of module() would otherwise run

  python tools/waveform_bench.py [--rounds 9] [--iters 10] [--out profiles/waveform_bench.json] [--arms a,b,...]
      per shape the arms interleaved in ONE process for `rounds` rounds (order rotated each round); per arm the median, the
      minimum and the maximum over the rounds of (time / iters).  For the bandwidth shape also the bytes the algorithm needs
      (outputs and targets read once per pass that reads them, d_outputs written once) over the median, against 8 TB/s.
      One JSON line on stdout, and the same in --out.  Fails without a GPU.
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ARMS = ["spectral_mse", "wave_mse", "wave_l1_mse", "wave_sisdr", "wave_all", "torch_all"]
TERMS = {"wave_mse": {"mse": 1.0}, "wave_l1_mse": {"mse": 1.0, "l1": 1.0}, "wave_sisdr": {"si_sdr": 1.0},
         "wave_all": {"mse": 1.0, "l1": 1.0, "si_sdr": 1.0, "snr": 1.0}}
SHAPES = {"headline": (2, 16, 16389, 1), "bandwidth": (2, 4, 589824, 2)}
PEAK_BYTES_PER_S = 8e12
# passes over (outputs, targets) of the library's arms: the gradient pass, and the row-sums pass when a row term is in use
READ_PASSES = {"spectral_mse": 1, "wave_mse": 1, "wave_l1_mse": 1, "wave_sisdr": 2, "wave_all": 2}


def torch_total(torch, out, tgt, eps=1e-8):
    """wave_all's total in eager torch (float32, zero_mean)."""
    S, B = out.shape[:2]
    d = out - tgt
    e, t = out.reshape(S * B, -1), tgt.reshape(S * B, -1)
    e, t = e - e.mean(1, keepdim=True), t - t.mean(1, keepdim=True)
    tt = (t * t).sum(1)
    P = (e * t).sum(1) ** 2 / (tt + eps)
    si = 10.0 * torch.log10((P + eps) / ((e * e).sum(1) - P + eps))
    snr = 10.0 * torch.log10((tt + eps) / (((e - t) ** 2).sum(1) + eps))
    return (d * d).mean() + d.abs().mean() - si.mean() - snr.mean()


def setup(shape):
    import torch
    from wave_u_net_amd import spectral, waveform
    if not torch.cuda.is_available():
        raise SystemExit("waveform_bench.py needs a GPU")
    gen = torch.Generator(device="cuda").manual_seed(1337)
    tgt = torch.randn(shape, device="cuda", generator=gen) * 0.3
    out = (tgt + 0.1 * torch.randn(shape, device="cuda", generator=gen)).contiguous()
    d_outs = torch.empty_like(out)
    spec = spectral.SpectralLoss([], mse_weight=1.0)
    sbuf = (torch.empty(spec.num_losses, dtype=torch.float32, device="cuda"), spec._scratch_for(out))
    wl = {a: waveform.WaveformLoss(t) for a, t in TERMS.items()}
    wscr = {a: l._scratch_for(out) for a, l in wl.items()}
    wbuf = {a: torch.empty(l.num_losses, dtype=torch.float32, device="cuda") for a, l in wl.items()}
    leaf = out.clone().requires_grad_(True)

    def step(arm):
        if arm == "spectral_mse":
            spec.run(out, tgt, d_outs, *sbuf)
        elif arm in wl:
            wl[arm].run(out, tgt, d_outs, wbuf[arm], wscr[arm])
        else:
            leaf.grad = None
            torch_total(torch, leaf, tgt).backward()
    return torch, step


def timed(name, shape, rounds, iters, arms):
    torch, step = setup(shape)
    for arm in arms:                                              # warm-up
        for _ in range(3):
            step(arm)
    torch.cuda.synchronize()
    allr = {a: [] for a in arms}
    for r in range(rounds):
        order = arms[r % len(arms):] + arms[:r % len(arms)]
        for arm in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                step(arm)
            e1.record()
            e1.synchronize()
            allr[arm].append(round(e0.elapsed_time(e1) / iters, 4))
    res = {"shape": list(shape), "median_ms": {a: round(statistics.median(allr[a]), 4) for a in arms},
           "min_ms": {a: min(allr[a]) for a in arms}, "max_ms": {a: max(allr[a]) for a in arms}, "rounds_ms": allr}
    if name == "bandwidth":
        n = math.prod(shape)
        res["needed_bytes"] = {a: 4 * n * (2 * READ_PASSES[a] + 1) for a in arms if a in READ_PASSES}
        res["fraction_of_8TBps"] = {a: round(b / (res["median_ms"][a] * 1e-3) / PEAK_BYTES_PER_S, 4)
                                    for a, b in res["needed_bytes"].items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "waveform_bench.json"))
    ap.add_argument("--arms", default=",".join(ARMS), help="comma-separated subset of %s" % ", ".join(ARMS))
    a = ap.parse_args()
    arms = a.arms.split(",")
    if not arms or any(x not in ARMS for x in arms):
        ap.error("--arms must name some of %s" % ", ".join(ARMS))
    res = {"what": "ms per call with d_outputs; arms interleaved in one process under HIP events", "rounds": a.rounds,
           "iters": a.iters, "shapes": {name: timed(name, shape, a.rounds, a.iters, arms) for name, shape in SHAPES.items()}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
