#!/usr/bin/env python3
"""What the soft-mask post-filter and the multichannel Wiener filter cost, on a synthetic 3-minute stereo two-source track at 22 050 Hz,
n_fft 2048, hop 512, power 2.

Kernel arms (HIP events on the launch stream around `iters` back-to-back calls, on buffers resident in HBM):
  mask_filter       wun_mask_filter: mix [n, 2], estimates [2, n, 2] -> [2, n, 2]   (n = 180 * 22050; 7 755 frames in blocks of 256)
  wiener_filter_1   wun_wiener_filter on the same buffers, 1 EM iteration: 2 passes of forward transforms, one inverse
  wiener_filter_2   the same with 2 iterations: 3 passes of forward transforms, one inverse
FFT arms (the same definitions through wun_mask_filter_fft / wun_wiener_filter_fft, same buffers, same clock):
  mask_filter_fft, wiener_filter_1_fft            at 2048 / 512 on the track above: the GEMM arms' twins
  mask_filter_fft_4096, wiener_filter_1_fft_4096  at 4096 / 1024 on the same 3 minutes at 44 100 Hz (n = 180 * 44100), which
                                                  the GEMM path refuses
Track arms (a host clock around work that ends in the download of the estimates; same separator, same samples):
  separate_track            evaluate.separate_track at the model's rate, no filter   (the comparison; there is no target)
  separate_track_filtered   the same with postfilter = the filter above

  python tools/postfilter_bench.py [--config baseline_stereo] [--rounds 7] [--iters 5] [--out profiles/postfilter_bench.json]
      the arms interleaved in ONE process for `rounds` rounds (order rotated each round); per arm the median, the minimum and
      the maximum over the rounds.  One JSON line on stdout, and the same in --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ARMS = ["mask_filter", "wiener_filter_1", "wiener_filter_2", "mask_filter_fft", "wiener_filter_1_fft", "mask_filter_fft_4096",
        "wiener_filter_1_fft_4096", "separate_track", "separate_track_filtered"]
SECONDS, N_FFT, HOP = 180, 2048, 512
HI_SR, HI_N_FFT, HI_HOP = 44100, 4096, 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="baseline_stereo")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import wave_u_net_amd as wun
    from wave_u_net_amd.evaluate import separate_track
    from wave_u_net_amd.postfilter import SoftMaskFilter, WienerFilter

    cfg = wun.get_config(args.config)
    sep = wun.UnetAudioSeparator(cfg, device="cuda:0")
    sr = int(cfg["expected_sr"])
    C = 1 if cfg["mono_downmix"] else 2
    S = len(cfg["source_names"])
    n = SECONDS * sr
    rng = np.random.default_rng(0)
    audio = rng.uniform(-0.5, 0.5, (n, C)).astype(np.float32)
    filt = SoftMaskFilter(N_FFT, HOP)
    mix = torch.from_numpy(audio).cuda()
    est = torch.from_numpy(rng.uniform(-0.5, 0.5, (S, n, C)).astype(np.float32)).cuda()
    out = torch.empty_like(est)
    scratch = torch.empty(filt.scratch_floats(S, n, C), dtype=torch.float32, device="cuda")
    wiener = {"wiener_filter_%d" % it: WienerFilter(N_FFT, HOP, iterations=it) for it in (1, 2)}
    wscratch = {a: torch.empty(w.scratch_floats(S, n, C), dtype=torch.float32, device="cuda") for a, w in wiener.items()}

    # the FFT arms: (filter, mix, estimates, out, scratch)
    n_hi = SECONDS * HI_SR
    mix_hi = torch.from_numpy(rng.uniform(-0.5, 0.5, (n_hi, C)).astype(np.float32)).cuda()
    est_hi = torch.from_numpy(rng.uniform(-0.5, 0.5, (S, n_hi, C)).astype(np.float32)).cuda()
    out_hi = torch.empty_like(est_hi)
    fft = {}
    for arm, f, bufs in (("mask_filter_fft", SoftMaskFilter(N_FFT, HOP, transform="fft"), (mix, est, out, n)),
                         ("wiener_filter_1_fft", WienerFilter(N_FFT, HOP, iterations=1, transform="fft"), (mix, est, out, n)),
                         ("mask_filter_fft_4096", SoftMaskFilter(HI_N_FFT, HI_HOP, transform="fft"), (mix_hi, est_hi, out_hi, n_hi)),
                         ("wiener_filter_1_fft_4096", WienerFilter(HI_N_FFT, HI_HOP, iterations=1, transform="fft"),
                          (mix_hi, est_hi, out_hi, n_hi))):
        fft[arm] = (f,) + bufs[:3] + (torch.empty(f.scratch_floats(S, bufs[3], C), dtype=torch.float32, device="cuda"),)

    def run(arm):
        """One measurement of the arm in ms."""
        if arm == "mask_filter" or arm in wiener or arm in fft:
            if arm in fft:
                f, mx, es, ot, sc = fft[arm]
            else:
                f, sc = (filt, scratch) if arm == "mask_filter" else (wiener[arm], wscratch[arm])
                mx, es, ot = mix, est, out
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                f.run(mx, es, ot, sc)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.iters
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        separate_track(cfg, sep, audio, sr, batch_hops=16, postfilter=filt if arm == "separate_track_filtered" else None)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for arm in ARMS:                                              # warm-up: every plan, table and kernel
        run(arm)
    times = {a: [] for a in ARMS}
    for r in range(args.rounds):
        for arm in ARMS[r % len(ARMS):] + ARMS[:r % len(ARMS)]:
            times[arm].append(run(arm))

    F = -(-(n + N_FFT - HOP) // HOP)
    K = N_FFT // 2 + 1
    flop_fwd = 2.0 * (S + 1) * C * F * N_FFT * 2 * K              # Re and Im of the estimates and the mix
    flop_inv = 2.0 * S * C * F * N_FFT * 2 * K
    res = {"tool": "postfilter_bench", "config": args.config, "seconds_of_audio": SECONDS, "expected_sr": sr, "channels": C,
           "sources": S, "n_fft": N_FFT, "hop": HOP, "power": 2, "frames": F, "rounds": args.rounds, "iters": args.iters,
           "scratch_MB": round(4 * scratch.numel() / 1e6, 1), "dense_TFLOP": {"forward": round(flop_fwd / 1e12, 3), "inverse": round(flop_inv / 1e12, 3)},
           "ms": {a: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for a, v in times.items()}}
    m = res["ms"]
    res["filter_TFLOPs_at_median"] = round((flop_fwd + flop_inv) / (m["mask_filter"]["median"] * 1e-3) / 1e12, 1)
    for a in wiener:                                              # the arithmetic expectation: (I + 1) forward passes, one inverse
        it = wiener[a].iterations
        res[a + "_over_mask_filter_at_median"] = round(m[a]["median"] / m["mask_filter"]["median"], 3)
        res[a + "_dense_flop_ratio"] = round(((it + 1) * flop_fwd + flop_inv) / (flop_fwd + flop_inv), 3)
        res[a + "_scratch_MB"] = round(4 * wscratch[a].numel() / 1e6, 1)
    res["fft"] = {"high_rate": {"expected_sr": HI_SR, "n_fft": HI_N_FFT, "hop": HI_HOP, "frames": -(-(n_hi + HI_N_FFT - HI_HOP) // HI_HOP)},
                  "mask_filter_fft_median_over_gemm_min": round(m["mask_filter_fft"]["median"] / m["mask_filter"]["min"], 4),
                  "wiener_filter_1_fft_median_over_gemm_min": round(m["wiener_filter_1_fft"]["median"] / m["wiener_filter_1"]["min"], 4),
                  "scratch_MB": {a: round(4 * v[4].numel() / 1e6, 1) for a, v in fft.items()}}
    res["separate_track_added_ms_at_median"] = round(m["separate_track_filtered"]["median"] - m["separate_track"]["median"], 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
