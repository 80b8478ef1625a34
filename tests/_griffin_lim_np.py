"""float64 oracle of Griffin-Lim phase reconstruction (include/wun.h: wun_griffin_lim), for the tests only.
Written from the header's definitions on the FFT path's oracle (_fft_np: STFT = rfft of the windowed frames, ISTFT = windowed
irfft over the window-square sums with the 1e-8 rule):

    unit(c)        c / |c|, unit(0) = 1
    one step       c = STFT(y_prev) (or the given spectrum, Im of the bins 0 and n_fft / 2 taken as 0);
                   t = c + momentum (c - c_prev), t = c on the first step;  S = mag unit(t);  y = ISTFT(S)
    inconsistency  sum (|c| - mag)^2 and sum mag^2 over all rows, frames and bins, for a step that ran the forward transform

The one-step rule's pointwise bound (a priori, not fitted).  With L = log2 n_fft and u = 2^-24, a float32 FFT of the windowed
frame carries at most beta_f = (L + 2) u sum_n |w[n] frame_f[n]| per Re / Im.  An error of beta in Re and Im moves unit(c) by at
most delta = min(2, 4 beta / |c|); the projected bin by mag delta; the inverse frame by sum_k c_k mag delta / n_fft, plus its
own rounding (L + 4) u sum_k c_k mag / n_fft; a sample by the window-weighted sum of that over its covering frames divided by
the window-square sum, plus 4 u |y| for the overlap-add and the division.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fft_np as fo  # noqa: E402
import _postfilter_np as ora  # noqa: E402
import _spectral_np as sp  # noqa: E402

U = 2.0 ** -24


def unit(c):
    c = np.asarray(c, dtype=np.complex128)
    a = np.abs(c)
    return np.where(a == 0, 1.0 + 0j, c / np.where(a == 0, 1.0, a))


def given(re, im):
    """The complex float64 spectrum of a caller's (re, im): Im of the bins 0 and n_fft / 2 counts as 0."""
    c = np.asarray(re, np.float64) + 1j * np.asarray(im, np.float64)
    c[..., 0] = c[..., 0].real
    c[..., -1] = c[..., -1].real
    return c


def forward(y, n_fft, hop, lead, F):
    re, im = fo.stft(np.asarray(y, np.float64), n_fft, hop, lead, F)
    im[..., 0] = 0.0
    im[..., -1] = 0.0
    return re + 1j * im


def inconsistency(c, mag):
    mag = np.asarray(mag, np.float64)
    return np.array([((np.abs(c) - mag) ** 2).sum(), (mag * mag).sum()])


def project_invert(c, mag, T, n_fft, hop, lead, c_prev=None, momentum=0.0):
    """y [R, T] of one step from its spectrum c."""
    t = c if (c_prev is None or momentum == 0.0) else c + momentum * (c - c_prev)
    s = np.asarray(mag, np.float64) * unit(t)
    return fo.istft(s.real, s.imag, T, n_fft, hop, lead)


def step(y_prev, mag, n_fft, hop, lead, c_prev=None, momentum=0.0):
    """(y, c, [sum (|c| - mag)^2, sum mag^2]) of one step from audio y_prev [R, T]."""
    T, F = np.asarray(y_prev).shape[1], np.asarray(mag).shape[1]
    c = forward(y_prev, n_fft, hop, lead, F)
    return project_invert(c, mag, T, n_fft, hop, lead, c_prev, momentum), c, inconsistency(c, mag)


def iterate(mag, T, n_fft, hop, lead, iterations, c0=None, y0=None, momentum=0.0):
    """(y [R, T], inconsistency [iterations, 2], every y_i) of the whole iteration; exactly one of c0 (complex) and y0."""
    assert (c0 is None) != (y0 is None)
    inc = np.full((iterations, 2), np.nan)
    ys, c_prev, y = [], None, y0
    for i in range(iterations):
        if i == 0 and c0 is not None:
            c = np.asarray(c0, np.complex128)
        else:
            c = forward(y, n_fft, hop, lead, np.asarray(mag).shape[1])
            inc[i] = inconsistency(c, mag)
        y = project_invert(c, mag, T, n_fft, hop, lead, c_prev, momentum)
        c_prev = c
        ys.append(y)
    return y, inc, ys


def beta(y_prev, n_fft, hop, lead, F):
    """[R, F]: the forward transform's bound per Re / Im, (log2 n_fft + 2) u sum_n |w[n] frame_f[n]|."""
    fr = ora.frames_of(np.asarray(y_prev, np.float64), n_fft, hop, lead, F)
    return (np.log2(n_fft) + 2) * U * np.abs(fr * sp.window(n_fft)[None, None, :]).sum(-1)


def step_bound(c, mag, y, T, n_fft, hop, lead, fwd_beta=None, delta=None):
    """([R, T] bound of a float32 step whose float64 spectrum is c and result y, the fraction of bins with delta = 2).
    fwd_beta None: the spectrum was given exactly (no forward transform): delta = 0.  With momentum pass t for c and
    (1 + 2 momentum) beta (t = (1 + m) c_i - m c_{i-1}, each spectrum within its beta).  `delta` overrides the rule."""
    mag = np.asarray(mag, np.float64)
    R, F, K = mag.shape
    ck = ora.c_k(n_fft)
    L = np.log2(n_fft)
    if delta is not None:
        delta = np.broadcast_to(np.asarray(delta, np.float64), mag.shape)
    elif fwd_beta is None:
        delta = np.zeros_like(mag)
    else:
        a = np.abs(c)
        delta = np.minimum(2.0, 4.0 * fwd_beta[:, :, None] / np.where(a == 0, 1e-300, a))
    g = ((ck * mag * delta).sum(-1) + (L + 4) * U * (ck * mag).sum(-1)) / n_fft                  # [R, F]
    w = sp.window(n_fft)
    num = ora._overlap_add(g[:, :, None] * w[None, None, :], T, hop, lead)
    ws = ora.window_sums(T, F, n_fft, hop, lead)
    live = ws >= ora.WSUM_MIN
    bound = np.where(live, num / np.where(live, ws, 1.0) + 4 * U * np.abs(y), 0.0)
    return bound, float((delta >= 2.0).mean())


def fixture(seed, R, T, n_fft, hop, lead, F):
    """White noise of amplitude 0.3, the magnitudes of another noise perturbed by up to 20 % -- no spectrogram of a signal --, and
    a noisy copy of the first noise as the audio start: (mag float32 [R, F, K], y_init float32 [R, T])."""
    rng = np.random.RandomState(seed)
    x = 0.3 * rng.randn(R, T)
    mag = np.abs(forward(0.3 * rng.randn(R, T), n_fft, hop, lead, F)) * (1.0 + 0.2 * rng.rand(R, F, n_fft // 2 + 1))
    return mag.astype(np.float32), (x + 0.05 * rng.randn(R, T)).astype(np.float32)


def rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))
