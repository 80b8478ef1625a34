#!/usr/bin/env python3
"""The bits of the STFT family: one `name sha256` line per output of a fixed list of small cases, run
through the library that WUN_LIB names (default libwun.so).  Two libraries that compute the same floats print the same lines:

  WUN_LIB=libwun_parent.so python tools/stft_bits.py > a.txt;  python tools/stft_bits.py > b.txt;  cmp a.txt b.txt

  transforms  wun_stft_magnitude, wun_stft_complex, wun_istft (and the _fft twins): n_fft / hop 64 / 16, 64 / 32, 2048 / 512;
              T 5, 1000, 5000 centred, and without padding where T >= n_fft; (S, B, C) (2, 1, 2) and (3, 3, 1); every case
              also from pointers 4 bytes behind an allocation's start
  loss        wun_spectral_loss at the resolutions (64, 48) and (256, 64), S 2, B 3, T 1000, C 1 and 2, with and without
              d_outputs: the losses and the gradient
  filters     wun_mask_filter and wun_wiener_filter (iterations 0, 1, 2), and the _fft twins: S 2, C 1 and 2, n 200 and 5000
              at 64 / 16 (315 frames: more than one block of 256), n 5000 at 2048 / 512, power 1 and 2; one _fft case at
              4096 / 1024
  fft loss    wun_stft_magnitude_fft on the transforms' unpadded cases and at 4096 / 1024 and 8192 / 2048; wun_spectral_loss_fft and
              wun_spectral_loss_terms_fft (all four terms) on the loss's cases and at (64, 48) + (4096, 1024), T 6149
              (DESIGN.md 5.16).  These lines come last: the lines above them are those of a library without the entries
Inputs come from fixed seeds; the whole run takes a few seconds on the GPU.
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from wave_u_net_amd import spectral  # noqa: E402
from wave_u_net_amd.postfilter import SoftMaskFilter, WienerFilter  # noqa: E402

RES = [(64, 16), (64, 32), (2048, 512)]
LENGTHS = [5, 1000, 5000]
SHAPES = [(2, 1, 2), (3, 3, 1)]                      # (S, B, C)
LOSS_RES = [(64, 48), (256, 64)]
FILTERS = [(200, 64, 16), (5000, 64, 16), (5000, 2048, 512)]     # (n, n_fft, hop)


def show(name, *tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    print(name, h.hexdigest())


def audio(seed, shape):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32)).cuda()


def offset_copy(x):
    """A copy of x whose base pointer lies one float behind an allocation's start."""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    v = buf[1:].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 8 == 4 and v.is_contiguous()
    return v


def transforms():
    for (n_fft, hop) in RES:
        for T in LENGTHS:
            for (S, B, Cn) in SHAPES:
                x = audio(n_fft + T + S, (S, B, T, Cn))
                for off in (False, True):
                    xin = offset_copy(x) if off else x
                    tag = "%d/%d T%d S%dB%dC%d%s" % (n_fft, hop, T, S, B, Cn, " +4" if off else "")
                    if T >= n_fft:
                        show("magnitude " + tag, spectral.stft_magnitude(xin, n_fft, hop))
                    for tr in spectral.TRANSFORMS:
                        for centered in (True, False):
                            if not centered and T < n_fft:
                                continue
                            name = "%s %s %s" % (tr, "centred" if centered else "unpadded", tag)
                            re, im = spectral.stft(xin, n_fft, hop, centered=centered, transform=tr)
                            show("stft " + name, re, im)
                            if off:
                                re, im = offset_copy(re), offset_copy(im)
                            show("istft " + name, spectral.istft(re, im, T, n_fft, hop, centered=centered, transform=tr))


def loss():
    S, B, T = 2, 3, 1000
    f = spectral.SpectralLoss(LOSS_RES, weights=[1.0, 0.5], mse_weight=0.5)
    for Cn in (1, 2):
        out, tgt = audio(10 + Cn, (S, B, T, Cn)), audio(20 + Cn, (S, B, T, Cn))
        for grad in (False, True):
            losses, d_out = f.loss_and_grad(out, tgt, grad=grad)
            name = "loss C%d %s" % (Cn, "grad" if grad else "only")
            show(name + " losses", losses)
            if grad:
                show(name + " d_outputs", d_out)


def filters():
    S = 2
    cases = [(tr, n, n_fft, hop, Cn, power) for tr in spectral.TRANSFORMS for (n, n_fft, hop) in FILTERS for Cn in (1, 2)
             for power in (1, 2)] + [("fft", 9000, 4096, 1024, 2, 2)]
    for (tr, n, n_fft, hop, Cn, power) in cases:
        mix, est = audio(n + n_fft + Cn, (n, Cn)), audio(n + n_fft + Cn + 100, (S, n, Cn))
        tag = "%s %d/%d n%d C%d p%d" % (tr, n_fft, hop, n, Cn, power)
        show("mask_filter " + tag, SoftMaskFilter(n_fft, hop, power, transform=tr).apply(mix, est))
        for it in (0, 1, 2):
            show("wiener_filter_%d %s" % (it, tag), WienerFilter(n_fft, hop, power, iterations=it, transform=tr).apply(mix, est))


def fft_loss():
    for (n_fft, hop, T) in [(n, h, t) for (n, h) in RES for t in LENGTHS if t >= n] + [(4096, 1024, 9000), (8192, 2048, 12293)]:
        for (S, B, Cn) in SHAPES:
            x = audio(n_fft + T + S, (S, B, T, Cn))
            for off in (False, True):
                tag = "%d/%d T%d S%dB%dC%d%s" % (n_fft, hop, T, S, B, Cn, " +4" if off else "")
                show("magnitude_fft " + tag, spectral.stft_magnitude(offset_copy(x) if off else x, n_fft, hop, transform="fft"))
    S, B = 2, 3
    terms = {"mag_l1": 0.7, "log_mag_l1": 0.4, "sc": 1.3, "complex_l1": 0.6}
    for (res, T, log_eps) in ((LOSS_RES, 1000, 1e-2), ([(64, 48), (4096, 1024)], 6149, 4.0)):
        for tname, tw in (("loss_fft", None), ("loss_terms_fft", terms)):
            f = spectral.SpectralLoss(res, weights=[1.0, 0.5], mse_weight=0.5, terms=tw, log_eps=log_eps, transform="fft")
            for Cn in (1, 2):
                out, tgt = audio(10 + Cn, (S, B, T, Cn)), audio(20 + Cn, (S, B, T, Cn))
                for grad in (False, True):
                    losses, d_out = f.loss_and_grad(out, tgt, grad=grad)
                    name = "%s %d/%d C%d %s" % (tname, res[-1][0], res[-1][1], Cn, "grad" if grad else "only")
                    show(name + " losses", losses)
                    if grad:
                        show(name + " d_outputs", d_out)


if __name__ == "__main__":
    transforms()
    loss()
    filters()
    if hasattr(spectral.SpectralLoss([]), "transform"):      # (a tree from before DESIGN.md 5.16 has no such entries)
        fft_loss()
    torch.cuda.synchronize()
