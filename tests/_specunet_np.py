"""The oracle of the spectrogram U-Net tests: the model of Models/UnetSpectrogramSeparator.py:40-108 at training=False, restated
from the reference's text in torch on the CPU, in float64 (or, as the stand-in the end-to-end tolerance is measured on, float32).

Layout is TF's: activations [B, H, W, C] (H = frames, W = bins), conv kernels [5, 5, Cin, Cout], transposed-conv kernels
[5, 5, Cout, Cin].

  conv2d_s2            tf.layers.conv2d(.., [5, 5], strides=[2, 2], padding='same') on even H, W: out = H / 2, total padding
                       (out - 1) 2 + 5 - H = 3, of which TF puts 1 before and 2 after:
                       out[y][x] = sum A[2y + ky - 1][2x + kx - 1][ci] W[ky][kx][ci][co]
  conv2d_transpose_s2  tf.layers.conv2d_transpose(.., [5, 5], strides=[2, 2], padding='same') = the gradient of the conv above with
                       respect to its input: the full transposed conv full[2 j + k] += A[j] W[k] (length 2 N + 3) without its first
                       and its last two outputs per axis
  batch_norm           tf.contrib.layers.batch_norm defaults: scale=False, epsilon=0.001, moving statistics at is_training=False
  istft_tf             tf.contrib.signal.inverse_stft with inverse_stft_window_fn(hop): irfft of every frame times
                       w / D[n mod hop], D the steady-state overlap-add of w^2, then the plain overlap-add

abs_conv / abs_transpose evaluate the same sums on absolute values: the sum |x| |w| of the standard fp32 accumulation bound
(n + c) 2^-24 sum |x| |w| the single-operator tests assert (n products, c = 4 for the epilogue's few roundings).
"""
import math

import numpy as np
import torch

BN_EPS = 1e-3


def conv2d_s2(x, w):
    """x [B, H, W, Ci] (H, W even), w [5, 5, Ci, Co] -> [B, H / 2, W / 2, Co]; differentiable."""
    B, H, W, _ = x.shape
    assert H % 2 == 0 and W % 2 == 0
    xp = torch.nn.functional.pad(x, (0, 0, 1, 2, 1, 2))
    out = 0
    for ky in range(5):
        for kx in range(5):
            out = out + xp[:, ky:ky + H:2, kx:kx + W:2, :] @ w[ky, kx]
    return out


def conv2d_transpose_s2(a, w):
    """a [B, N, M, Ci], w [5, 5, Co, Ci] -> [B, 2 N, 2 M, Co]: scatter into the full transposed conv, then the crop."""
    B, N, M, _ = a.shape
    Co = w.shape[2]
    full = torch.zeros((B, 2 * N + 3, 2 * M + 3, Co), dtype=a.dtype)
    for ky in range(5):
        for kx in range(5):
            full[:, ky:ky + 2 * N:2, kx:kx + 2 * M:2, :] += a @ w[ky, kx].transpose(0, 1)
    return full[:, 1:1 + 2 * N, 1:1 + 2 * M, :]


def batch_norm(z, mean, var, beta):
    return (z - mean) * torch.rsqrt(var + BN_EPS) + beta


def leaky_relu(z):
    return torch.where(z > 0, z, 0.2 * z)


def hann(n_fft, dtype=torch.float64):
    n = torch.arange(n_fft, dtype=torch.float64)
    return (0.5 - 0.5 * torch.cos(2.0 * math.pi * n / n_fft)).to(dtype)


def stft(x, n_fft, hop):
    """x [B, T] -> complex [B, F, K], F = 1 + (T - n_fft) // hop (pad_end=False), periodic Hann."""
    fr = x.unfold(-1, n_fft, hop) * hann(n_fft, x.dtype)
    return torch.fft.rfft(fr, dim=-1)


def steady_denominator(n_fft, hop, dtype=torch.float64):
    """D[p] = sum_i w^2[p + i hop] over 0 <= p + i hop < n_fft, p < hop."""
    w2 = hann(n_fft) ** 2
    return torch.stack([w2[p::hop].sum() for p in range(hop)]).to(dtype)


def istft_tf(z, n_fft, hop):
    """complex z [.., F, K] -> [.., (F - 1) hop + n_fft]."""
    rdtype = z.real.dtype
    F = z.shape[-2]
    D = steady_denominator(n_fft, hop, rdtype)
    n = torch.arange(n_fft)
    frames = torch.fft.irfft(z, n=n_fft, dim=-1) * (hann(n_fft, rdtype) / D[n % hop])
    y = torch.zeros(z.shape[:-2] + ((F - 1) * hop + n_fft,), dtype=rdtype)
    for f in range(F):
        y[..., f * hop:f * hop + n_fft] += frames[..., f, :]
    return y


def _suffix(stem, index):
    return stem if index == 0 else "%s_%d" % (stem, index)


def variable_shapes(L, nif, S=2):
    """[(name, shape)] in TF's graph-construction order inside scope `separator` (an index 0 has no suffix)."""
    out = []
    for s in range(S):
        for i in range(L):
            cin, cout = (1 if i == 0 else nif * 2 ** (i - 1)), nif * 2 ** i
            c, b = _suffix("conv2d", s * L + i), _suffix("BatchNorm", s * (2 * L - 1) + i)
            out += [("separator/%s/kernel" % c, (5, 5, cin, cout)), ("separator/%s/bias" % c, (cout,))]
            out += [("separator/%s/%s" % (b, leaf), (cout,)) for leaf in ("beta", "moving_mean", "moving_variance")]
        cin = nif * 2 ** (L - 1)
        for i in range(L - 1):
            cout = nif * 2 ** (L - i - 2)
            c, b = _suffix("conv2d_transpose", s * L + i), _suffix("BatchNorm", s * (2 * L - 1) + L + i)
            out += [("separator/%s/kernel" % c, (5, 5, cout, cin)), ("separator/%s/bias" % c, (cout,))]
            out += [("separator/%s/%s" % (b, leaf), (cout,)) for leaf in ("beta", "moving_mean", "moving_variance")]
            cin = 2 * cout                                   # concat([skip, up]) on the channel axis
        c = _suffix("conv2d_transpose", s * L + L - 1)
        out += [("separator/%s/kernel" % c, (5, 5, 1, cin)), ("separator/%s/bias" % c, (1,))]
    return out


def random_variables(L, nif, seed, S=2, zero_convs=False):
    """The fixtures of the end-to-end tests: glorot-scaled kernels, biases / beta / moving_mean of order 0.1, moving_variance in
    [0.5, 2].  zero_convs: every conv kernel and bias 0 (the mask is then sigmoid(0) = 0.5 exactly)."""
    rng = np.random.RandomState(seed)
    v = {}
    for name, shp in variable_shapes(L, nif, S):
        if name.endswith("/kernel"):
            lim = math.sqrt(6.0 / (25 * (shp[2] + shp[3])))
            v[name] = np.zeros(shp, np.float32) if zero_convs else rng.uniform(-lim, lim, shp).astype(np.float32)
        elif name.endswith("/moving_variance"):
            v[name] = rng.uniform(0.5, 2.0, shp).astype(np.float32)
        elif name.endswith("/bias") and zero_convs:
            v[name] = np.zeros(shp, np.float32)
        else:
            v[name] = (0.1 * rng.randn(*shp)).astype(np.float32)
    return v


def forward(mix, variables, L, nif, n_fft, hop, S=2, dtype=torch.float64, return_spectrogram=False):
    """mix [B, T] array, variables name -> array.  -> list over the sources of [B, F, K] magnitudes or [B, T] audio, numpy float64
    (computed in `dtype`), plus X and M for the structural checks: (outputs, X, M)."""
    cdtype = torch.complex128 if dtype == torch.float64 else torch.complex64
    v = {k: torch.as_tensor(np.asarray(a), dtype=dtype) for k, a in variables.items()}
    x = torch.as_tensor(np.asarray(mix), dtype=dtype)
    B, T = x.shape
    X = stft(x, n_fft, hop)                                                      # :54
    F, K = X.shape[1], X.shape[2]
    assert T == (F - 1) * hop + n_fft and F % 2 ** L == 0 and (n_fft // 2) % 2 ** L == 0
    M = X.abs()                                                                  # :55
    a0 = torch.log1p(M[:, :, :-1, None])                                         # :59-60
    outs = []
    for s in range(S):                                                           # :63
        cur, enc = a0, []
        for i in range(L):                                                       # :68-74
            c, b = "separator/" + _suffix("conv2d", s * L + i), "separator/" + _suffix("BatchNorm", s * (2 * L - 1) + i)
            cur = conv2d_s2(cur, v[c + "/kernel"]) + v[c + "/bias"]
            cur = leaky_relu(batch_norm(cur, v[b + "/moving_mean"], v[b + "/moving_variance"], v[b + "/beta"]))
            if i < L - 1:
                enc.append(cur)
        for i in range(L - 1):                                                   # :77-83 (dropout: identity)
            c = "separator/" + _suffix("conv2d_transpose", s * L + i)
            b = "separator/" + _suffix("BatchNorm", s * (2 * L - 1) + L + i)
            cur = conv2d_transpose_s2(cur, v[c + "/kernel"]) + v[c + "/bias"]
            cur = torch.relu(batch_norm(cur, v[b + "/moving_mean"], v[b + "/moving_variance"], v[b + "/beta"]))
            cur = torch.cat([enc[-i - 1], cur], dim=3)
        c = "separator/" + _suffix("conv2d_transpose", s * L + L - 1)
        mask = torch.sigmoid(conv2d_transpose_s2(cur, v[c + "/kernel"]) + v[c + "/bias"])[..., 0]   # :86
        mask = torch.cat([mask, torch.full((B, F, 1), 0.5, dtype=dtype)], dim=2)                # :87
        if return_spectrogram:
            outs.append((M * mask).double().numpy())                                             # :91
        else:
            outs.append(istft_tf((mask * M).to(cdtype) * torch.exp(1j * torch.angle(X)), n_fft, hop).double().numpy())   # :100-101
    return outs, X.to(torch.complex128).numpy(), M.double().numpy()


def abs_conv(x, w):
    """sum |x| |w| of every output of conv2d_s2, float64 numpy."""
    return conv2d_s2(torch.as_tensor(np.abs(x), dtype=torch.float64), torch.as_tensor(np.abs(w), dtype=torch.float64)).numpy()


def abs_transpose(a, w):
    return conv2d_transpose_s2(torch.as_tensor(np.abs(a), dtype=torch.float64), torch.as_tensor(np.abs(w), dtype=torch.float64)).numpy()


def epilogue(z, bias, bn, act):
    """float64 torch: + bias, batch norm (mean, var, beta) or None, act in {None, "lrelu", "relu", "sigmoid"}."""
    if bias is not None:
        z = z + bias
    if bn is not None:
        z = batch_norm(z, *bn)
    if act == "lrelu":
        z = leaky_relu(z)
    elif act == "relu":
        z = torch.relu(z)
    elif act == "sigmoid":
        z = torch.sigmoid(z)
    return z
