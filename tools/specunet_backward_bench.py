#!/usr/bin/env python3
"""Milliseconds of the spectrogram U-Net's backward entries at the U7 geometry -- B = 4, T = 98 560 (F = 128 frames
of 1024 / 768), L = 6, nif = 16, two sources, dropout 0.5, fp32 -- on one training forward, the same build, the same GPU:

  loss_backward    wun_spec_loss_backward (the magnitude L1 compiled into its head; 5.18's backward pass)
  backward_mags    wun_spec_backward with d_mags alone (the one-lane-per-bin head)
  backward_audio   wun_spec_backward with d_audio alone (u = d_audio / D, then the FFT with the mask-gradient epilogue)
  backward_both    wun_spec_backward with both
  train_audio      wun_spec_train_audio (mask X of every source, then wun_istft_tf_fft)

  python tools/specunet_backward_bench.py [--rounds 5] [--iters 5] [--out profiles/specunet_backward_bench.json]
      the arms interleaved in ONE process for `rounds` rounds (order rotated each round) after a warm-up; HIP events on the
      current stream around every pass of `iters` back-to-back calls; per arm the median, minimum and maximum over the rounds of
      (time / iters).  One JSON line on stdout, and the same in --out.  Fails without a GPU.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GEOMETRY = dict(B=4, F=128, n_fft=1024, hop=768, L=6, nif=16, S=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "specunet_backward_bench.json"))
    args = ap.parse_args()
    import torch
    import wave_u_net_amd as wun
    from wave_u_net_amd.spectrogram import UnetSpectrogramSeparator
    if not torch.cuda.is_available():
        raise SystemExit("specunet_backward_bench.py needs a GPU")
    g = GEOMETRY
    T = (g["F"] - 1) * g["hop"] + g["n_fft"]
    cfg = wun.get_config("unet_spectrogram_l1")
    assert (cfg["num_layers"], cfg["num_initial_filters"], cfg["num_frames"], cfg["batch_size"]) == (g["L"], g["nif"], T, g["B"])
    sep = UnetSpectrogramSeparator(cfg, device="cuda:0")
    sep._ensure_variables()
    gen = torch.Generator(device="cuda").manual_seed(1337)
    targets = 0.2 * torch.randn((g["S"], g["B"], T), device="cuda", generator=gen)
    mix3, tg4 = targets.sum(0)[:, :, None].contiguous(), targets[..., None].contiguous()

    outs = sep.get_output(mix3, True, return_spectrogram=True)
    mags = torch.stack([outs[k] for k in sep.source_names])
    audio = torch.stack([v for v in sep.audio_output().values()])
    d_audio = (2.0 * (audio - tg4) / float(audio.numel())).contiguous()
    d_mags = (torch.randn(mags.shape, device="cuda", generator=gen) / float(mags.numel())).contiguous()

    arms = {"loss_backward": lambda: sep.loss_and_gradients(tg4),
            "backward_mags": lambda: sep.backward(d_mags=d_mags),
            "backward_audio": lambda: sep.backward(d_audio=d_audio),
            "backward_both": lambda: sep.backward(d_mags=d_mags, d_audio=d_audio),
            "train_audio": lambda: sep._train_audio(g["B"], T, audio)}

    def timed(f, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            f()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n

    for f in arms.values():                                  # warm-up
        timed(f, 2)
    times = {k: [] for k in arms}
    order = list(arms)
    for r in range(args.rounds):
        for k in order[r % len(order):] + order[:r % len(order)]:
            times[k].append(timed(arms[k], args.iters))
    res = {"what": "spectrogram U-Net backward entries on one training forward, fp32, dropout 0.5", "geometry": dict(g, T=T),
           "rounds": args.rounds, "iters": args.iters, "device": torch.cuda.get_device_name(0),
           "arms": {k: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for k, v in times.items()}}
    med = lambda k: res["arms"][k]["ms_median"]
    res["audio_head_extra_ms"] = med("backward_audio") - med("backward_mags")
    res["backward_mags_over_loss_backward"] = med("backward_mags") / med("loss_backward")
    line = json.dumps(res, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
