"""float64 oracle of the complex STFT, the inverse STFT and the soft-mask filter (include/wun.h: wun_stft_complex, wun_istft,
wun_mask_filter), for the tests only.  The header's comment is the definition:

    Centred framing : lead = n_fft - hop, F = ceil((T + lead) / hop); frame f holds x[f hop - lead + n], 0 <= n < n_fft, and
                      is zero outside [0, T).
    Complex STFT    : Re[r][f][k] = sum_n frame_f[n] Cb[n][k], Im likewise with Sb.
    Inverse STFT    : frame_f[n] = (1 / n_fft) sum_k c_k (Re[f][k] Cb[n][k] + Im[f][k] Sb[n][k]), c_0 = c_{n_fft/2} = 1, every
                      other c_k = 2;  y[t] = (sum_f frame_f[t + lead - f hop]) / (sum_f w^2[t + lead - f hop]); where the
                      denominator is below 1e-8, y[t] = 0.
    Soft-mask filter: A_s = |E_s|^p, mask_s = (A_s + eps / S) / (sum_j A_j + eps), out_s = ISTFT(mask_s X).

The transform is the direct DFT with _spectral_np.basis (tests/test_postfilter_host.py cross-checks it against torch.stft /
torch.istft where the framings coincide).  Rows are [R, T] float64 (_spectral_np.rows / unrows).

Error bounds, u = 2^-24.  A Re or Im carries at most beta[r][f] = n_fft u sum_n |w[n] frame_f[n]| (_spectral_np.beta on the padded
signal).  A frame of the inverse is a dot product of 2 K terms with factors of modulus <= 1: it carries at most
g[r][f] = 2 K u sum_k (|c_k Re| + |c_k Im|) / n_fft; an output sample the sum of g over its covering frames divided by its
window-square sum, plus 4 u |y| for the overlap-add, the denominator and the division.  An error of beta in every Re and Im
moves a frame of the inverse by at most (1 / n_fft) sum_k c_k 2 beta = 2 beta (sum_k c_k = n_fft).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _spectral_np as sp  # noqa: E402

U = 2.0 ** -24
WSUM_MIN = 1e-8
MIN_ENERGY = 1e-4          # the fixtures' floor of sum_j A_j, many orders above eps


def centered_frames(T, n_fft, hop):
    return -(-(T + n_fft - hop) // hop)


def framing(T, n_fft, hop, centered):
    """(lead, F)."""
    return (n_fft - hop, centered_frames(T, n_fft, hop)) if centered else (0, sp.num_frames(T, n_fft, hop))


def padded(xr, n_fft, hop, lead, F):
    """[R, (F - 1) hop + n_fft]: the rows with `lead` zeros before and zeros (or a cut) behind, so that frame f is
    [f hop, f hop + n_fft) of the result."""
    xr = np.asarray(xr, dtype=np.float64)
    total = (F - 1) * hop + n_fft
    out = np.zeros((xr.shape[0], total))
    n = min(xr.shape[1], total - lead)
    out[:, lead:lead + n] = xr[:, :n]
    return out


def frames_of(xr, n_fft, hop, lead, F):
    """[R, F, n_fft]."""
    return np.lib.stride_tricks.sliding_window_view(padded(xr, n_fft, hop, lead, F), n_fft, axis=1)[:, ::hop][:, :F]


def stft(xr, n_fft, hop, lead, F):
    """(Re, Im) float64 [R, F, K]."""
    cb, sb = sp.basis(n_fft)
    fr = frames_of(xr, n_fft, hop, lead, F)
    return fr @ cb, fr @ sb


def beta(xr, n_fft, hop, lead, F):
    """[R, F]: the bound of one Re or Im."""
    fr = frames_of(xr, n_fft, hop, lead, F)
    return n_fft * U * np.abs(fr * sp.window(n_fft)[None, None, :]).sum(-1)


def c_k(n_fft):
    c = np.full(n_fft // 2 + 1, 2.0)
    c[0] = c[-1] = 1.0
    return c


def _overlap_add(frames, T, hop, lead):
    """[R, F, n_fft] -> [R, T]: frame f added at f hop - lead, cut to [0, T)."""
    R, F, n_fft = frames.shape
    total = max((F - 1) * hop + n_fft, lead + T)
    y = np.zeros((R, total), dtype=frames.dtype)
    for f in range(F):
        y[:, f * hop:f * hop + n_fft] += frames[:, f]
    return y[:, lead:lead + T]


def window_sums(T, F, n_fft, hop, lead):
    """[T]: sum of w^2 over the frames covering each sample."""
    w2 = sp.window(n_fft) ** 2
    return _overlap_add(np.broadcast_to(w2, (1, F, n_fft)), T, hop, lead)[0]


def inverse_frames(re, im, n_fft):
    cb, sb = sp.basis(n_fft)
    c = c_k(n_fft) / n_fft
    return (re * c) @ cb.T + (im * c) @ sb.T


def istft(re, im, T, n_fft, hop, lead):
    """[R, T] float64."""
    F = re.shape[1]
    ws = window_sums(T, F, n_fft, hop, lead)
    y = _overlap_add(inverse_frames(re, im, n_fft), T, hop, lead)
    live = ws >= WSUM_MIN
    return np.where(live, y / np.where(live, ws, 1.0), 0.0)


def istft_bound(re, im, y, T, n_fft, hop, lead, fwd_beta=None):
    """[R, T]: the bound of an fp32 inverse of (re, im) whose float64 inverse is y; with fwd_beta [R, F] also the effect of
    an error of that size in every Re and Im.  0 where the window-square sum is below 1e-8 (those samples are exactly 0)."""
    R, F, K = re.shape
    g = 2 * K * U * ((np.abs(re) + np.abs(im)) * c_k(n_fft)).sum(-1) / n_fft        # [R, F]
    if fwd_beta is not None:
        g = g + 2.0 * fwd_beta
    ws = window_sums(T, F, n_fft, hop, lead)
    num = _overlap_add(np.broadcast_to(g[:, :, None], (R, F, n_fft)), T, hop, lead)
    live = ws >= WSUM_MIN
    return np.where(live, num / np.where(live, ws, 1.0) + 4 * U * np.abs(y), 0.0)


def istft_fp32(re, im, T, n_fft, hop, lead):
    """The inverse in float32 with numpy matmuls: the stand-in a bound is tried on before it is trusted on the device."""
    cb, sb = (b.astype(np.float32) for b in sp.basis(n_fft))
    c = (c_k(n_fft) / n_fft).astype(np.float32)
    fr = (np.asarray(re, np.float32) * c) @ cb.T + (np.asarray(im, np.float32) * c) @ sb.T
    F = fr.shape[1]
    ws = window_sums(T, F, n_fft, hop, lead)
    y = _overlap_add(fr, T, hop, lead)
    live = ws >= WSUM_MIN
    return np.where(live, y / np.where(live, ws, 1.0).astype(np.float32), np.float32(0)).astype(np.float32)


def stft_fp32(xr, n_fft, hop, lead, F):
    cb, sb = (b.astype(np.float32) for b in sp.basis(n_fft))
    fr = frames_of(xr, n_fft, hop, lead, F).astype(np.float32)
    return fr @ cb, fr @ sb


def mask_filter(mix, est, n_fft, hop, power=2, eps=1e-10):
    """mix [n, C], est [S, n, C] -> (out float64 [S, n, C], min over the bins of sum_j A_j)."""
    mix, est = np.asarray(mix, dtype=np.float64), np.asarray(est, dtype=np.float64)
    S, n, C = est.shape
    eps = float(np.float32(eps))
    lead, F = framing(n, n_fft, hop, True)
    xre, xim = stft(mix.T, n_fft, hop, lead, F)                                      # [C, F, K]
    ere, eim = stft(est.transpose(0, 2, 1).reshape(S * C, n), n_fft, hop, lead, F)
    ere, eim = ere.reshape(S, C, F, -1), eim.reshape(S, C, F, -1)
    a = ere * ere + eim * eim
    if power == 1:
        a = np.sqrt(a)
    total = a.sum(0)
    mask = (a + eps / S) / (total + eps)
    assert np.abs(mask.sum(0) - 1.0).max() < 1e-12                                   # the masks sum to 1 by construction
    out = istft((mask * xre).reshape(S * C, F, -1), (mask * xim).reshape(S * C, F, -1), n, n_fft, hop, lead)
    return out.reshape(S, C, n).transpose(0, 2, 1), float(total.min())


def filter_fixture(seed, S, n, C, n_fft, hop, power=2, eps=1e-10):
    """Gaussian noise of amplitude 0.2 - 0.3 and its float64 filter output; the mask is well conditioned: every bin of the
    summed estimates carries energy many orders above eps."""
    rng = np.random.RandomState(seed)
    mix = (0.3 * rng.randn(n, C)).astype(np.float32)
    est = ((0.2 + 0.1 * rng.rand(S, 1, 1)) * rng.randn(S, n, C)).astype(np.float32)
    out, floor = mask_filter(mix, est, n_fft, hop, power, eps)
    assert floor > MIN_ENERGY, "min sum_j A_j = %g" % floor
    return mix, est, out
