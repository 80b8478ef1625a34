#!/usr/bin/env python3
"""Milliseconds per training step of the spectrogram U-Net on the magnitude objective at the U7a geometry --
B = 4, T = 98 560 (F = 128 frames of 1024 / 768), L = 6, nif = 16, two sources, dropout 0.5 -- for two arms on the same GPU, fp32:

  wun     UnetSpectrogramSeparator: get_output(mix, True, return_spectrogram=True), loss_and_gradients(targets), adam_step(lr)
          (wun_spec_train_forward, wun_spec_loss_backward, wun_spec_adam_step)
  torch   the same step restated with torch.nn.functional on the same weights: conv2d / conv_transpose2d through MIOpen,
          batch_norm(training=True) with running statistics, the wun arm's dropout masks as multipliers, the magnitude L1,
          backward() and torch.optim.Adam: what a user would otherwise write

  python tools/specunet_train_bench.py [--rounds 5] [--iters 5] [--out profiles/specunet_train_bench.json]
      both arms interleaved in ONE process for `rounds` rounds (order rotated each round) after a warm-up; HIP events on the
      current stream around every pass of `iters` back-to-back steps; per arm and pass the median, minimum and maximum over the
      rounds of (time / iters).  Before the timing: one forward + backward of both arms from the same weights with the same
      masks, and the largest difference of their gradients per kind of tensor, next to the largest gradient.
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
PASSES = ("forward", "backward", "adam")


def stem(kind, idx):
    return "separator/%s%s" % (kind, "" if idx == 0 else "_%d" % idx)


class TorchArm(object):
    """The step in torch: leaves in torch's layouts, created from the separator's variables."""

    def __init__(self, torch, sep, g, lr):
        self.torch, self.g = torch, g
        L, var = g["L"], sep.variables()
        self.p, self.names = {}, {}

        def leaf(name, t):
            t = t.detach().clone().requires_grad_(True)
            self.names[name] = t
            return t

        for s in range(g["S"]):
            for i in range(L):
                c, b = stem("conv2d", s * L + i), stem("BatchNorm", s * (2 * L - 1) + i)
                self.p[("down", s, i)] = (leaf(c + "/kernel", var[c + "/kernel"].permute(3, 2, 0, 1).contiguous()), leaf(c + "/bias", var[c + "/bias"]),
                                          leaf(b + "/beta", var[b + "/beta"]), var[b + "/moving_mean"].clone(), var[b + "/moving_variance"].clone())
            for i in range(L):
                c = stem("conv2d_transpose", s * L + i)
                bn = (None, None, None)
                if i < L - 1:
                    b = stem("BatchNorm", s * (2 * L - 1) + L + i)
                    bn = (leaf(b + "/beta", var[b + "/beta"]), var[b + "/moving_mean"].clone(), var[b + "/moving_variance"].clone())
                self.p[("up", s, i)] = (leaf(c + "/kernel", var[c + "/kernel"].permute(3, 2, 0, 1).contiguous()), leaf(c + "/bias", var[c + "/bias"])) + bn
        self.opt = torch.optim.Adam(list(self.names.values()), lr=lr)
        n = torch.arange(g["n_fft"], device="cuda", dtype=torch.float64)
        self.window = (0.5 - 0.5 * torch.cos(2.0 * math.pi * n / g["n_fft"])).float()
        self.masks = {}
        self.ones = {}                   # batch norm without gamma: a constant weight of ones per channel count

    def bn(self, x, rm, rv, beta):
        c = x.shape[1]
        if c not in self.ones:
            self.ones[c] = self.torch.ones(c, device=x.device)
        return self.torch.nn.functional.batch_norm(x, rm, rv, self.ones[c], beta, True, 0.001, 1e-3)

    def loss(self, mix, targets):
        torch, g = self.torch, self.g
        Fn = torch.nn.functional
        L, n_fft, hop = g["L"], g["n_fft"], g["hop"]
        mag = lambda x: torch.stft(x, n_fft, hop, n_fft, self.window, center=False, return_complex=True).transpose(1, 2).abs()
        M = mag(mix)
        a0 = torch.log1p(M[:, None, :, :-1])
        total = 0
        for s in range(g["S"]):
            cur, enc = a0, []
            for i in range(L):
                w, b, beta, rm, rv = self.p[("down", s, i)]
                cur = Fn.conv2d(Fn.pad(cur, (1, 2, 1, 2)), w, b, stride=2)
                cur = Fn.leaky_relu(self.bn(cur, rm, rv, beta), 0.2)
                enc.append(cur)
            for i in range(L):
                w, b, beta, rm, rv = self.p[("up", s, i)]
                if i > 0:
                    cur = torch.cat([enc[L - 1 - i], cur], dim=1)
                    if (s, i - 1) in self.masks:
                        cur = cur * self.masks[(s, i - 1)]
                n, m = cur.shape[2], cur.shape[3]
                cur = Fn.conv_transpose2d(cur, w, b, stride=2)[:, :, 1:1 + 2 * n, 1:1 + 2 * m]
                if i < L - 1:
                    cur = torch.relu(self.bn(cur, rm, rv, beta))
            mask = Fn.pad(torch.sigmoid(cur[:, 0]), (0, 1), value=0.5)
            total = total + (mag(targets[s]) - M * mask).abs().mean()
        return total / g["S"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "specunet_train_bench.json"))
    args = ap.parse_args()
    import torch
    import wave_u_net_amd as wun
    from wave_u_net_amd.spectrogram import UnetSpectrogramSeparator
    if not torch.cuda.is_available():
        raise SystemExit("specunet_train_bench.py needs a GPU")
    g = GEOMETRY
    T = (g["F"] - 1) * g["hop"] + g["n_fft"]
    cfg = wun.get_config("unet_spectrogram_l1")
    assert (cfg["num_layers"], cfg["num_initial_filters"], cfg["num_frames"], cfg["batch_size"]) == (g["L"], g["nif"], T, g["B"])
    lr = cfg["init_sup_sep_lr"]
    sep = UnetSpectrogramSeparator(cfg, device="cuda:0")
    sep._ensure_variables()
    gen = torch.Generator(device="cuda").manual_seed(1337)
    targets = 0.2 * torch.randn((g["S"], g["B"], T), device="cuda", generator=gen)
    mix = targets.sum(0)
    mix3, tg4 = mix[:, :, None].contiguous(), targets[..., None].contiguous()
    arm = TorchArm(torch, sep, g, lr)

    # one forward + backward of both arms from the same weights with the same masks
    sep.get_output(mix3, True, return_spectrogram=True)
    wun_loss = float(sep.loss_and_gradients(tg4).item())
    for s in range(g["S"]):
        for lv in range(min(3, g["L"] - 1)):
            arm.masks[(s, lv)] = sep.activation("dropout", s, lv).permute(0, 3, 1, 2).contiguous().clone()
    arm.opt.zero_grad(set_to_none=True)
    t_loss = arm.loss(mix, targets)
    t_loss.backward()
    diffs, wg = {}, sep.gradients()
    for name, leaf in arm.names.items():
        got = wg[name]
        ref = leaf.grad.permute(2, 3, 1, 0) if name.endswith("/kernel") else leaf.grad
        kind = ("transpose " if "conv2d_transpose" in name else "") + name.split("/")[-1]
        d = diffs.setdefault(kind, {"max_abs_diff": 0.0, "max_abs_grad": 0.0})
        d["max_abs_diff"] = max(d["max_abs_diff"], float((got - ref).abs().max()))
        d["max_abs_grad"] = max(d["max_abs_grad"], float(ref.abs().max()))

    ev = lambda: torch.cuda.Event(enable_timing=True)

    def wun_steps(n):
        t = dict.fromkeys(PASSES, 0.0)
        marks = []
        for _ in range(n):
            e = [ev() for _ in range(4)]
            e[0].record(); sep.get_output(mix3, True, return_spectrogram=True)
            e[1].record(); sep.loss_and_gradients(tg4)
            e[2].record(); sep.adam_step(lr)
            e[3].record()
            marks.append(e)
        marks[-1][3].synchronize()
        for e in marks:
            for i, k in enumerate(PASSES):
                t[k] += e[i].elapsed_time(e[i + 1])
        return t

    def torch_steps(n):
        t = dict.fromkeys(PASSES, 0.0)
        marks = []
        for _ in range(n):
            e = [ev() for _ in range(4)]
            arm.opt.zero_grad(set_to_none=True)
            e[0].record(); loss = arm.loss(mix, targets)
            e[1].record(); loss.backward()
            e[2].record(); arm.opt.step()
            e[3].record()
            marks.append(e)
        marks[-1][3].synchronize()
        for e in marks:
            for i, k in enumerate(PASSES):
                t[k] += e[i].elapsed_time(e[i + 1])
        return t

    arms = {"wun": wun_steps, "torch": torch_steps}
    for f in arms.values():                                  # warm-up
        f(2)
    times = {k: {p: [] for p in PASSES + ("step",)} for k in arms}
    order = list(arms)
    for r in range(args.rounds):
        for k in order[r % len(order):] + order[:r % len(order)]:
            t = arms[k](args.iters)
            for p in PASSES:
                times[k][p].append(t[p] / args.iters)
            times[k]["step"].append(sum(t.values()) / args.iters)
    res = {"what": "spectrogram U-Net training step, magnitude L1, fp32, dropout 0.5", "geometry": dict(g, T=T), "rounds": args.rounds,
           "iters": args.iters, "device": torch.cuda.get_device_name(0), "loss_wun": wun_loss, "loss_torch": float(t_loss.item()),
           "gradient_diff_wun_vs_torch": diffs, "arms": {}}
    for k in arms:
        res["arms"][k] = {p: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for p, v in times[k].items()}
    res["wun_over_torch_step"] = res["arms"]["wun"]["step"]["ms_median"] / res["arms"]["torch"]["step"]["ms_median"]
    line = json.dumps(res, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
