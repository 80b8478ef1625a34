#!/usr/bin/env python3
"""Milliseconds per forward of the spectrogram U-Net at the U7 geometry -- B = 4, T = 98 560 (F = 128 frames of
1024 / 768), L = 6, nif = 16, two sources, audio out -- for two arms on the same GPU, fp32 both:

  wun     UnetSpectrogramSeparator.get_output(mix, False): one wun_spec_forward call (the STFT, per source 12 conv launches and
          the mask product, the inverse STFT)
  torch   the same definition restated with torch.nn.functional (conv2d / conv_transpose2d through MIOpen, torch.stft for the
          analysis, the same weights): what a user would otherwise write.  Its synthesis is torch.istft-free: irfft, the
          inverse window and a fold, as tf.contrib.signal.inverse_stft does.

  python tools/specunet_bench.py [--rounds 7] [--iters 10] [--out profiles/specunet_bench.json]
      both arms interleaved in ONE process for `rounds` rounds (order rotated each round) after a warm-up of every shape; HIP
      events on the current stream around `iters` back-to-back forwards; per arm the median, minimum and maximum over the
      rounds of (time / iters).  Also the algorithmic FLOPs of the convolutions (computed from the shapes below), the rate
      they imply at the median, and the largest difference between the two arms' outputs.
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

GEOMETRY = dict(B=4, F=128, n_fft=1024, hop=768, L=6, nif=16, S=2)


def conv_flops(B, F, n_fft, L, nif, S, **_):
    """2 x multiply-adds of every conv as defined (25 taps per conv output; a transposed conv's input feeds 25 taps)."""
    H, W, c, total = F, n_fft // 2, 1, 0
    for i in range(L):
        H, W = H // 2, W // 2
        total += 2 * 25 * c * (nif << i) * B * H * W
        c = nif << i
    for i in range(L - 1):
        co = nif << (L - i - 2)
        total += 2 * 25 * c * co * B * H * W
        H, W, c = 2 * H, 2 * W, 2 * co
    total += 2 * 25 * c * 1 * B * H * W
    return S * total


def torch_forward(torch, Fn, mix, v, g, window, inv_window):
    """[B, T] -> [S, B, T]; v: name -> tensor in torch's layouts (conv [Co, Ci, 5, 5], transposed [Ci, Co, 5, 5])."""
    L, S, n_fft, hop = g["L"], g["S"], g["n_fft"], g["hop"]
    X = torch.stft(mix, n_fft, hop, n_fft, window, center=False, return_complex=True).transpose(1, 2)      # [B, F, K]
    M = X.abs()
    a0 = torch.log1p(M[:, None, :, :-1])                                        # NCHW: [B, 1, F, K - 1]
    outs = []
    for s in range(S):
        cur, enc = a0, []
        for i in range(L):
            w, b, bn = v[("down", s, i)]
            cur = Fn.conv2d(Fn.pad(cur, (1, 2, 1, 2)), w, b, stride=2)
            cur = Fn.leaky_relu((cur - bn[1][None, :, None, None]) * torch.rsqrt(bn[2] + 1e-3)[None, :, None, None] + bn[0][None, :, None, None], 0.2)
            if i < L - 1:
                enc.append(cur)
        for i in range(L):
            w, b, bn = v[("up", s, i)]
            n, m = cur.shape[2], cur.shape[3]
            cur = Fn.conv_transpose2d(cur, w, b, stride=2)[:, :, 1:1 + 2 * n, 1:1 + 2 * m]
            if i == L - 1:
                break
            cur = torch.relu((cur - bn[1][None, :, None, None]) * torch.rsqrt(bn[2] + 1e-3)[None, :, None, None] + bn[0][None, :, None, None])
            cur = torch.cat([enc[-i - 1], cur], dim=1)
        mask = Fn.pad(torch.sigmoid(cur[:, 0]), (0, 1), value=0.5)
        frames = torch.fft.irfft(mask * X, n=n_fft, dim=-1) * inv_window                                 # [B, F, n_fft]
        T = (frames.shape[1] - 1) * hop + n_fft
        y = Fn.fold(frames.transpose(1, 2), (1, T), (1, n_fft), stride=(1, hop))
        outs.append(y[:, 0, 0])
    return torch.stack(outs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "specunet_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as Fn
    import wave_u_net_amd as wun
    from wave_u_net_amd.spectrogram import UnetSpectrogramSeparator
    if not torch.cuda.is_available():
        raise SystemExit("specunet_bench.py needs a GPU")
    g = GEOMETRY
    T = (g["F"] - 1) * g["hop"] + g["n_fft"]
    cfg = wun.get_config("unet_spectrogram")
    assert (cfg["num_layers"], cfg["num_initial_filters"], cfg["num_frames"], cfg["batch_size"]) == (g["L"], g["nif"], T, g["B"])
    sep = UnetSpectrogramSeparator(cfg, device="cuda:0")
    rng = np.random.RandomState(7)
    named = {}
    for name, _, shp in sep.variable_table():                # non-trivial batch norms, so that both arms do the same work
        if name.endswith("/moving_variance"):
            named[name] = rng.uniform(0.5, 2.0, shp).astype(np.float32)
        elif not name.endswith("/kernel"):
            named[name] = (0.1 * rng.randn(*shp)).astype(np.float32)
    sep.load_variables(named)
    tv, var = {}, sep.variables()
    L = g["L"]

    def stem(kind, idx):
        return "separator/%s%s" % (kind, "" if idx == 0 else "_%d" % idx)

    for s in range(g["S"]):
        for i in range(L):
            c, b = stem("conv2d", s * L + i), stem("BatchNorm", s * (2 * L - 1) + i)
            tv[("down", s, i)] = (var[c + "/kernel"].permute(3, 2, 0, 1).contiguous(), var[c + "/bias"],
                                  [var[b + "/" + k] for k in ("beta", "moving_mean", "moving_variance")])
        for i in range(L):
            c = stem("conv2d_transpose", s * L + i)
            bn = None if i == L - 1 else [var[stem("BatchNorm", s * (2 * L - 1) + L + i) + "/" + k]
                                          for k in ("beta", "moving_mean", "moving_variance")]
            # TF [5, 5, Cout, Cin] -> torch conv_transpose2d [Cin, Cout, 5, 5]
            tv[("up", s, i)] = (var[c + "/kernel"].permute(3, 2, 0, 1).contiguous(), var[c + "/bias"], bn)
    gen = torch.Generator(device="cuda").manual_seed(1337)
    mix = 0.3 * torch.randn((g["B"], T), device="cuda", generator=gen)
    n = torch.arange(g["n_fft"], device="cuda", dtype=torch.float64)
    w64 = 0.5 - 0.5 * torch.cos(2.0 * math.pi * n / g["n_fft"])
    D = torch.stack([(w64 ** 2)[p::g["hop"]].sum() for p in range(g["hop"])])
    window, inv_window = w64.float(), (w64 / D[torch.arange(g["n_fft"], device="cuda") % g["hop"]]).float()

    arms = {
        "wun": lambda: torch.stack([o for o in sep.get_output(mix[:, :, None], False).values()])[..., 0],
        "torch": lambda: torch_forward(torch, Fn, mix, tv, g, window, inv_window),
    }
    with torch.no_grad():
        outs = {k: f().clone() for k, f in arms.items()}     # warm-up of every shape, and the agreement of the two arms
        for f in arms.values():
            f()
        torch.cuda.synchronize()
        diff = float((outs["wun"] - outs["torch"]).abs().max())
        times = {k: [] for k in arms}
        order = list(arms)
        for r in range(args.rounds):
            for k in order[r % len(order):] + order[:r % len(order)]:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    arms[k]()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / args.iters)
    flops = conv_flops(**g)
    res = {"what": "spectrogram U-Net forward, audio out, fp32", "geometry": dict(g, T=T), "rounds": args.rounds, "iters": args.iters,
           "conv_gflop_per_forward": flops / 1e9, "max_abs_diff_wun_vs_torch": diff, "max_abs_output": float(outs["torch"].abs().max()),
           "device": torch.cuda.get_device_name(0), "arms": {}}
    for k, t in times.items():
        med = statistics.median(t)
        res["arms"][k] = {"ms_median": med, "ms_min": min(t), "ms_max": max(t), "conv_tflops_at_median": flops / med / 1e9}
    res["wun_over_torch"] = res["arms"]["wun"]["ms_median"] / res["arms"]["torch"]["ms_median"]
    line = json.dumps(res, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
