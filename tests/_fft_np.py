"""float64 oracle of the FFT path (include/wun.h: wun_stft_complex_fft, wun_istft_fft, wun_mask_filter_fft,
wun_wiener_filter_fft), for the tests only.  The definitions are _postfilter_np's and _wiener_np's -- the FFT
entries compute the same Re / Im, frames and filters as their GEMM twins -- evaluated with numpy.fft instead of the dense
basis, which would need 0.5 GB at n_fft = 8192:

    Complex STFT    : Re + i Im [r][f][k] = rfft(w frame_f)[k], frame_f from _postfilter_np.frames_of
    Inverse STFT    : frame_f[n] = w[n] irfft(Re + i Im)[n] (Im of the bins 0 and n_fft / 2 not read), then _postfilter_np's
                      overlap-add over the window-square sums with its 1e-8 rule
    Filters         : _postfilter_np.mask_filter / _wiener_np.wiener_filter with these transforms

The bounds beta and istft_bound are _postfilter_np's: they bound any float32 evaluation of an n_fft-term sum with factors of
modulus <= 1, whatever its order.  The float32 stand-ins here are scipy.fft.rfft / irfft on float32 input (pocketfft computes
in the input's precision): what an FFT in float32 costs on these very inputs.
"""
import os
import sys

import numpy as np
import scipy.fft

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _postfilter_np as ora  # noqa: E402
import _spectral_np as sp  # noqa: E402
import _wiener_np as wie  # noqa: E402
from _postfilter_np import MIN_ENERGY, U, beta, centered_frames, framing, frames_of, istft_bound, window_sums  # noqa: E402,F401


def stft(xr, n_fft, hop, lead, F):
    """(Re, Im) float64 [R, F, K]."""
    z = np.fft.rfft(frames_of(xr, n_fft, hop, lead, F) * sp.window(n_fft), axis=-1)
    return np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)


def stft_fp32(xr, n_fft, hop, lead, F):
    """The float32 stand-in: scipy's rfft of the float32 windowed frames (the window rounded once, one float32 product)."""
    fr = frames_of(xr, n_fft, hop, lead, F).astype(np.float32) * sp.window(n_fft).astype(np.float32)
    z = scipy.fft.rfft(fr, axis=-1)
    assert z.dtype == np.complex64
    return z.real.astype(np.float64), z.imag.astype(np.float64)


def inverse_frames(re, im, n_fft):
    z = np.asarray(re, np.float64) + 1j * np.asarray(im, np.float64)
    z[..., 0] = z[..., 0].real
    z[..., -1] = z[..., -1].real
    return np.fft.irfft(z, n=n_fft, axis=-1) * sp.window(n_fft)


def _finish(fr, T, hop, lead, dtype):
    ws = window_sums(T, fr.shape[1], fr.shape[2], hop, lead)
    y = ora._overlap_add(fr, T, hop, lead)
    live = ws >= ora.WSUM_MIN
    return np.where(live, y / np.where(live, ws, 1.0).astype(dtype), dtype(0))


def istft(re, im, T, n_fft, hop, lead):
    """[R, T] float64."""
    return _finish(inverse_frames(re, im, n_fft), T, hop, lead, np.float64)


def istft_fp32(re, im, T, n_fft, hop, lead):
    z = (np.asarray(re, np.float32) + 1j * np.asarray(im, np.float32)).astype(np.complex64)
    z[..., 0] = z[..., 0].real
    z[..., -1] = z[..., -1].real
    fr = scipy.fft.irfft(z, n=n_fft, axis=-1)
    assert fr.dtype == np.float32
    return _finish(fr * sp.window(n_fft).astype(np.float32), T, hop, lead, np.float32).astype(np.float32)


def _spectra(mix, est, n_fft, hop):
    mix, est = np.asarray(mix, dtype=np.float64), np.asarray(est, dtype=np.float64)
    S, n, C = est.shape
    lead, F = framing(n, n_fft, hop, True)
    xre, xim = stft(mix.T, n_fft, hop, lead, F)
    ere, eim = stft(est.transpose(0, 2, 1).reshape(S * C, n), n_fft, hop, lead, F)
    return xre + 1j * xim, (ere + 1j * eim).reshape(S, C, F, -1), lead, F


def wiener_filter(mix, est, n_fft, hop, power=2, mask_eps=1e-10, iterations=1, eps=1e-10):
    """mix [n, C], est [S, n, C] -> (out float64 [S, n, C], min over the bins of sum_j A_j).  iterations = 0: the soft mask."""
    S, n, C = np.asarray(est).shape
    mask_eps, eps = float(np.float32(mask_eps)), float(np.float32(eps))
    X, E, lead, F = _spectra(mix, est, n_fft, hop)
    y = wie.masked(X, E, power, mask_eps)
    for _ in range(iterations):
        y = wie.em_step(y, X, eps)[0]
    out = istft(y.real.reshape(S * C, F, -1), y.imag.reshape(S * C, F, -1), n, n_fft, hop, lead)
    return out.reshape(S, C, n).transpose(0, 2, 1), float((np.abs(E) ** power).sum(0).min())


def mask_filter(mix, est, n_fft, hop, power=2, eps=1e-10):
    return wiener_filter(mix, est, n_fft, hop, power, eps, 0)


def fixture(seed, S, n, C, n_fft, hop, power=2, iterations=0):
    """_postfilter_np.filter_fixture's recipe (Gaussian noise of amplitude 0.2 - 0.3) and the float64 output of the soft mask
    (iterations = 0) or the Wiener filter: (mix, est, out).  The mask must be well conditioned, as there."""
    rng = np.random.RandomState(seed)
    mix = (0.3 * rng.randn(n, C)).astype(np.float32)
    est = ((0.2 + 0.1 * rng.rand(S, 1, 1)) * rng.randn(S, n, C)).astype(np.float32)
    out, floor = wiener_filter(mix, est, n_fft, hop, power, iterations=iterations)
    assert S == 1 or floor > MIN_ENERGY, "min sum_j A_j = %g" % floor
    return mix, est, out


def loud_fixture(seed, n, n_fft, hop):
    """The conditioning case of DESIGN.md 5.13: source 0 is a 0.9-amplitude sine hard-panned to channel 0, source 1 is noise of
    amplitude 1e-3 on both channels; the estimates are the sources plus 1e-4 noise.  (mix [n, 2], est [2, n, 2], the float64
    Wiener output at I = 1.)  The sine's bins reach 0.9 n_fft / 4 next to bins of about 0.03: the widest range of spectra and
    of v = mean_c |y|^2 (12 orders) that audio in [-1, 1] with a noise floor gives at that n_fft."""
    rng = np.random.RandomState(seed)
    src = np.zeros((2, n, 2))
    src[0, :, 0] = 0.9 * np.sin(2 * np.pi * 440.0 / 44100.0 * np.arange(n))
    src[1] = 1e-3 * rng.randn(n, 2)
    mix = src.sum(0).astype(np.float32)
    est = (src + 1e-4 * rng.randn(2, n, 2)).astype(np.float32)
    out, _ = wiener_filter(mix, est, n_fft, hop, iterations=1)
    return mix, est, out


def wiener_filter_fp32(mix, est, n_fft, hop, power=2, mask_eps=1e-10, iterations=1, eps=1e-10):
    """_wiener_np.wiener_filter_fp32 with this module's float32 transforms: every stored spectrum rounded to float32, the EM
    step in float64 between them.  Its distance from wiener_filter is what float32 FFTs and storage cost on the given inputs."""
    mix, est = np.asarray(mix, dtype=np.float32), np.asarray(est, dtype=np.float32)
    S, n, C = est.shape
    mask_eps, eps = float(np.float32(mask_eps)), float(np.float32(eps))
    lead, F = framing(n, n_fft, hop, True)
    xre, xim = stft_fp32(mix.T, n_fft, hop, lead, F)
    ere, eim = stft_fp32(est.transpose(0, 2, 1).reshape(S * C, n), n_fft, hop, lead, F)
    X = xre + 1j * xim
    E = (ere + 1j * eim).reshape(S, C, F, -1)
    y = wie.masked(X, E, power, mask_eps).astype(np.complex64).astype(np.complex128)
    for _ in range(iterations):
        y = wie.em_step(y, X, eps)[0].astype(np.complex64).astype(np.complex128)
    out = istft_fp32(y.real.reshape(S * C, F, -1), y.imag.reshape(S * C, F, -1), n, n_fft, hop, lead)
    return out.reshape(S, C, n).transpose(0, 2, 1)
