"""float64 oracle of the spectral loss (include/wun.h: wun_stft_*, wun_spectral_loss), for the tests only.

The transform is CPU torch.stft(center=False, window=hann_window(periodic=True)) in float64; `basis` is the direct DFT of the
definition (the two agree to ~1e-11, tests/test_spectral_host.py).  Audio is [S, B, T, C]; a row is one (s, b, c),
r = (s * B + b) * C + c.  The gradient takes the signs of M_est - M_tgt as an argument, so that a test can pin them to the
decisions the GPU made in fp32 (the L1 sign is discontinuous where two magnitudes nearly tie).
"""
import numpy as np
import torch


def rows(x):
    """[S, B, T, C] -> float64 [R, T]."""
    x = np.asarray(x, dtype=np.float64)
    S, B, T, C = x.shape
    return np.ascontiguousarray(x.transpose(0, 1, 3, 2).reshape(S * B * C, T))


def unrows(g, shape):
    S, B, T, C = shape
    return np.ascontiguousarray(g.reshape(S, B, C, T).transpose(0, 1, 3, 2))


def window(n_fft):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)


def basis(n_fft):
    """(Cb, Sb) float64 [n_fft, K]: w[n] cos and -w[n] sin of 2 pi ((n k) mod n_fft) / n_fft."""
    n = np.arange(n_fft, dtype=np.int64)[:, None]
    k = np.arange(n_fft // 2 + 1, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((n * k) % n_fft).astype(np.float64) / n_fft
    w = window(n_fft)[:, None]
    return w * np.cos(ang), -w * np.sin(ang)


def num_frames(T, n_fft, hop):
    return 1 + (T - n_fft) // hop


def stft(xr, n_fft, hop):
    """(Re, Im) float64 [R, F, K] of rows xr [R, T]."""
    win = torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
    z = torch.stft(torch.from_numpy(np.ascontiguousarray(xr)), n_fft, hop_length=hop, win_length=n_fft, window=win,
                   center=False, onesided=True, return_complex=True)                # [R, K, F]
    z = z.transpose(1, 2)
    return z.real.numpy().copy(), z.imag.numpy().copy()


def magnitude(x, n_fft, hop):
    """float64 [R, F, K]."""
    re, im = stft(rows(x), n_fft, hop)
    return np.sqrt(re * re + im * im)


def frame_view(xr, n_fft, hop):
    """[R, F, n_fft] view of the frames of rows xr."""
    F = num_frames(xr.shape[1], n_fft, hop)
    return np.lib.stride_tricks.sliding_window_view(xr, n_fft, axis=1)[:, ::hop][:, :F]


def beta(x, n_fft, hop):
    """[R, F]: n_fft * 2^-24 * sum_n |w[n] x[f hop + n]| -- the worst-case error of an fp32 dot product of the windowed frame
    with factors of modulus <= 1, in any order."""
    fr = frame_view(rows(x), n_fft, hop)
    return n_fft * 2.0 ** -24 * np.abs(fr * window(n_fft)[None, None, :]).sum(-1)


def overlap_add(dframe, T, hop):
    """[R, F, n_fft] -> [R, T]: frame f added at f * hop."""
    R, F, n_fft = dframe.shape
    g = np.zeros((R, T), dtype=dframe.dtype)
    for f in range(F):
        g[:, f * hop:f * hop + n_fft] += dframe[:, f]
    return g


def loss_and_grad(out, tgt, resolutions, weights, mse_weight, signs=None):
    """(losses, grad): losses = [total, MSE, L_0, ...] (float64, L_j unweighted), grad = d total / d out [S, B, T, C].
    signs: per resolution an [R, F, K] array used in place of sgn(M_est - M_tgt) in the gradient (None: float64's own)."""
    out = np.asarray(out, dtype=np.float64)
    tgt = np.asarray(tgt, dtype=np.float64)
    d = out - tgt
    mse = float(np.mean(d * d))
    g = mse_weight * 2.0 * d / d.size
    losses = [0.0, mse]
    total = mse_weight * mse
    xr, tr = rows(out), rows(tgt)
    T = xr.shape[1]
    for j, (n_fft, hop) in enumerate(resolutions):
        re, im = stft(xr, n_fft, hop)
        tre, tim = stft(tr, n_fft, hop)
        me, mt = np.sqrt(re * re + im * im), np.sqrt(tre * tre + tim * tim)
        lj = float(np.mean(np.abs(me - mt)))
        losses.append(lj)
        total += weights[j] * lj
        sg = np.sign(me - mt) if signs is None else np.asarray(signs[j], dtype=np.float64)
        safe = np.where(me > 0, me, 1.0)
        cre = np.where(me > 0, sg * re / safe, 0.0)
        cim = np.where(me > 0, sg * im / safe, 0.0)
        cb, sb = basis(n_fft)
        dframe = cre @ cb.T + cim @ sb.T                                            # [R, F, n_fft]
        g = g + unrows(overlap_add(dframe, T, hop) * (weights[j] / me.size), out.shape)
    losses[0] = total
    return np.array(losses), g


def grad_fp32(out, tgt, resolutions, weights, mse_weight, signs):
    """The pinned-sign gradient formula in float32 with CPU torch matmuls: a second, independent fp32 computation whose
    distance from float64 is the yardstick of the GPU's (returns float32 [S, B, T, C])."""
    out32 = np.asarray(out, dtype=np.float32)
    tgt32 = np.asarray(tgt, dtype=np.float32)
    g = (out32 - tgt32) * np.float32(np.float64(np.float32(mse_weight)) * 2.0 / out32.size)
    S, B, T, C = out32.shape
    xr = np.ascontiguousarray(out32.transpose(0, 1, 3, 2).reshape(S * B * C, T))
    for j, (n_fft, hop) in enumerate(resolutions):
        cb, sb = (torch.from_numpy(b.astype(np.float32)) for b in basis(n_fft))
        fr = torch.from_numpy(np.ascontiguousarray(frame_view(xr, n_fft, hop)))
        re, im = fr @ cb, fr @ sb
        me = torch.sqrt(re * re + im * im)
        sg = torch.from_numpy(np.asarray(signs[j], dtype=np.float32))
        live = me > 0
        safe = torch.where(live, me, torch.ones_like(me))
        cre = torch.where(live, sg * re / safe, torch.zeros_like(me))
        cim = torch.where(live, sg * im / safe, torch.zeros_like(me))
        dframe = (cre @ cb.T + cim @ sb.T).numpy()
        scale = np.float32(np.float64(np.float32(weights[j])) / me.numel())
        g = g + unrows(overlap_add(dframe, T, hop) * scale, out32.shape)
    return g.astype(np.float32)
