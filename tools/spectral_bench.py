#!/usr/bin/env python3
"""What the spectral loss costs, on the benchmarked plan: configs[1], M1 with context, 147443 -> 16389
samples, S = 2, B = 16, mono, the pinned tuning table imported as bench.py does; the reference's resolution 1024 / 768.

Kernel arms (HIP events on the launch stream around `iters` back-to-back calls, on the plan's own outputs):
  magnitude     wun_stft_magnitude of the outputs [2, 16, 16389, 1] (32 rows x 21 frames x 513 bins)
  loss_only     wun_spectral_loss, d_outputs = NULL (both signals' magnitudes, the float64 sums)
  loss_grad     wun_spectral_loss with d_outputs (plus the transposed GEMM and the overlap-add)
  terms_mag     wun_spectral_loss_terms with d_outputs, mag_l1 alone: loss_grad's work through the four-term entry
  terms_sc_log  ... sc + log_mag_l1 (the per-source sums pass and its one-block reduction before the coefficient pass)
  terms_all     ... all four terms (the forward also stores Re / Im of the targets)
  terms_mel     wun_spectral_loss_mel with d_outputs, mel_l1 + log_mel_l1 on 80 bands at 22 050 Hz and no linear-frequency term
                (the projection of both magnitudes, the mel terms pass, the adjoint inside the coefficient pass)
  terms_sc_log_mel  ... the same beside sc + log_mag_l1: terms_sc_log plus the mel stage
Trainer arms (one optimizer step each, same batch):
  step_mse      Trainer(batch 16): the time-domain MSE (wun_loss_backward)
  step_spectral Trainer(batch 16, spectral_loss = 1024 / 768, mse_weight 1): wun_spectral_loss, then wun_backward
FFT arms, interleaved with the arms above in the same process -- the GEMM arm beside an FFT arm is its yardstick:
  magnitude_fft, loss_grad_fft, terms_sc_log_fft   the arm of that name through the _fft entries (SpectralLoss(transform="fft"))
  step_spectral_fft                                step_spectral with "transform": "fft"
  magnitude_4096, loss_grad_4096, terms_sc_log_4096   the three FFT arms at 4096 / 1024, whatever --res says: no GEMM twin exists

  python tools/spectral_bench.py [--rounds 9] [--iters 10] [--out profiles/spectral_bench.json] [--arms a,b,...] [--res 1024,768]
      --res n_fft,hop: the resolution of every arm but the _4096 ones (default: the reference's)
      --arms loss_grad,terms_mag,terms_sc_log,terms_all --out profiles/spectral_terms_bench.json: the four-term entry beside the old
      --arms loss_grad,terms_sc_log,terms_mel,terms_sc_log_mel --out profiles/spectral_mel_bench.json: the mel stage beside the entry
      the arms interleaved in ONE process for `rounds` rounds (order rotated each round); per arm the median, the minimum and
      the maximum over the rounds of (time / iters).  One JSON line on stdout, and the same in --out.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ARMS = ["magnitude", "loss_only", "loss_grad", "terms_mag", "terms_sc_log", "terms_all", "step_mse", "step_spectral",
        "magnitude_fft", "loss_grad_fft", "terms_sc_log_fft", "step_spectral_fft", "magnitude_4096", "loss_grad_4096",
        "terms_sc_log_4096", "terms_mel", "terms_sc_log_mel"]
MEL = {"n_mels": 80, "sample_rate": 22050}                       # both mel terms at weight 1, log_eps 1e-3
MEL_TERMS = {"terms_mel": None, "terms_sc_log_mel": {"sc": 1.0, "log_mag_l1": 1.0}}
TERMS = {"terms_mag": {"mag_l1": 1.0}, "terms_sc_log": {"sc": 1.0, "log_mag_l1": 1.0},
         "terms_all": {"mag_l1": 1.0, "log_mag_l1": 1.0, "sc": 1.0, "complex_l1": 1.0}}
RES = [(1024, 768)]
RES_4096 = [(4096, 1024)]


def setup(arms):
    import torch
    import wave_u_net_amd as wun
    from wave_u_net_amd import spectral
    from wave_u_net_amd.training import Trainer, synthetic_source
    os.environ["WUN_NO_TUNE"] = "1"                               # (Trainer.tune: only the pinned table below)
    cfg = wun.get_config("m1_context")
    table = open(os.path.join(ROOT, "profiles", "round6_tune_table.txt")).read()
    spec = {"resolutions": [list(r) for r in RES], "mse_weight": 1.0}
    tr_mse, tr_spec = Trainer(cfg, batch_size=16), Trainer(cfg, batch_size=16, spectral_loss=spec)
    tr_fft = Trainer(cfg, batch_size=16, spectral_loss=dict(spec, transform="fft")) if "step_spectral_fft" in arms else None
    mix, targets = synthetic_source(cfg, 16, tr_mse.t_in, tr_mse.t_out, tr_mse.device, seed=1337)()
    for tr in (tr_mse, tr_spec, tr_fft):
        if tr is None:
            continue
        tr.sep.get_output(mix, True)
        tr.sep.tune_import(table)
    outs = tr_mse.sep._outs[tr_mse.sep._last_key].clone()
    tg = targets.to(torch.float32).contiguous()
    loss = spectral.SpectralLoss(RES, mse_weight=1.0)
    scratch = loss._scratch_for(outs)
    losses = torch.empty(3, dtype=torch.float32, device=outs.device)
    d_outs = torch.empty_like(outs)
    tloss = {a: spectral.SpectralLoss(RES, mse_weight=1.0, terms=t, log_eps=1.0) for a, t in TERMS.items()}   # (n_fft 1024: 5.14)
    # the FFT twins, and the 4096 / 1024 arms: (loss, its resolution list) by arm; log_eps does not change the work
    floss = {"loss_grad_fft": spectral.SpectralLoss(RES, mse_weight=1.0, transform="fft"),
             "terms_sc_log_fft": spectral.SpectralLoss(RES, mse_weight=1.0, terms=TERMS["terms_sc_log"], log_eps=1.0, transform="fft"),
             "loss_grad_4096": spectral.SpectralLoss(RES_4096, mse_weight=1.0, transform="fft"),
             "terms_sc_log_4096": spectral.SpectralLoss(RES_4096, mse_weight=1.0, terms=TERMS["terms_sc_log"], log_eps=4.0,
                                                        transform="fft")}
    floss.update({a: spectral.SpectralLoss(RES, mse_weight=1.0, terms=t, log_eps=1.0, mel=MEL) for a, t in MEL_TERMS.items()
                  if a in arms and hasattr(spectral, "MEL_TERMS")})
    tloss.update({a: l for a, l in floss.items() if a in arms})
    tbuf = {a: (torch.empty(l.num_losses, dtype=torch.float32, device=outs.device), l._scratch_for(outs)) for a, l in tloss.items()}

    def step(arm):
        if arm == "magnitude":
            spectral.stft_magnitude(outs, *RES[0])
        elif arm == "loss_only":
            loss.run(outs, tg, None, losses, scratch)
        elif arm == "loss_grad":
            loss.run(outs, tg, d_outs, losses, scratch)
        elif arm == "magnitude_fft":
            spectral.stft_magnitude(outs, *RES[0], transform="fft")
        elif arm == "magnitude_4096":
            spectral.stft_magnitude(outs, *RES_4096[0], transform="fft")
        elif arm in tloss:
            tloss[arm].run(outs, tg, d_outs, *tbuf[arm])
        elif arm == "step_mse":
            tr_mse.step(mix, targets)
        elif arm == "step_spectral_fft":
            tr_fft.step(mix, targets)
        else:
            tr_spec.step(mix, targets)
    return torch, step, tuple(outs.shape)


def timed(rounds, iters, out, arms):
    torch, step, shape = setup(arms)
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
    res = {"what": "ms per call / per optimizer step; arms interleaved in one process", "outputs_shape": shape,
           "resolutions": RES, "rounds": rounds, "iters": iters,
           "median_ms": {a: round(statistics.median(allr[a]), 4) for a in arms},
           "min_ms": {a: min(allr[a]) for a in arms}, "max_ms": {a: max(allr[a]) for a in arms}, "rounds_ms": allr}
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--arms", default=",".join(ARMS), help="comma-separated subset of %s" % ", ".join(ARMS))
    ap.add_argument("--res", default="1024,768", help="n_fft,hop of every arm but the _4096 ones")
    a = ap.parse_args()
    RES[0] = tuple(int(v) for v in a.res.split(","))
    arms = a.arms.split(",")
    if not arms or any(x not in ARMS for x in arms):
        ap.error("--arms must name some of %s" % ", ".join(ARMS))
    timed(a.rounds, a.iters, a.out, arms)


if __name__ == "__main__":
    main()
