"""The contract of wun_time_stretch (include/wun.h) restated in float64 numpy on float32 inputs: the same
analysis positions a_f, the product X_f conj(P_f), the zero rule of the angle, the float32 rounding of the phase increment and
the sequential float64 phase accumulator.  The transforms are numpy's float64 FFTs, so the difference to the library is the
float32 arithmetic of its FFT and what that does to the angles."""
import numpy as np


def stretch_frames(n_in, num, den):
    """ceil(n_in * den / num): wun_time_stretch_frames."""
    return -((-int(n_in) * int(den)) // int(num))


def centered_frames(n, n_fft, hop):
    """wun_fft_centered_frames: frames at f * hop - (n_fft - hop) that cover [0, n)."""
    return (int(n) + (n_fft - hop) + hop - 1) // hop


def window(n_fft):
    """The periodic Hann window as the library's table holds it (float32), and its float64 squares (the normaliser's)."""
    n = np.arange(n_fft, dtype=np.float64)
    w64 = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / n_fft)
    return w64.astype(np.float32).astype(np.float64), w64 * w64


def _angle_turns(re, im):
    ang = np.arctan2(im, re) / (2.0 * np.pi)
    return np.where((re == 0.0) & (im == 0.0), 0.0, ang)


def _frames_at(x, starts, n_fft):
    """[len(starts), n_fft] of x[start + n], +0 outside [0, len(x))."""
    idx = starts[:, None] + np.arange(n_fft)[None, :]
    ok = (idx >= 0) & (idx < len(x))
    return np.where(ok, x[np.clip(idx, 0, len(x) - 1)], 0.0)


def time_stretch(x, num, den, n_fft, hop, n_out=None):
    """x [n_in, C] float32 -> y [n_out, C] float64 at the tempo ratio num / den."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    n_in, C = x.shape
    if n_out is None:
        n_out = stretch_frames(n_in, num, den)
    assert 1 <= n_out <= stretch_frames(n_in, num, den)
    N, h, K, lead = n_fft, hop, n_fft // 2 + 1, n_fft - hop
    F = centered_frames(n_out, N, h)
    w, wsq = window(N)
    f = np.arange(F, dtype=np.int64)
    a = (f * h * num) // den
    k = np.arange(K, dtype=np.int64)
    adv = ((k * h) % N).astype(np.float64) / N
    y = np.zeros((n_out, C), np.float64)
    den_sum = np.zeros(n_out + N + F * h, np.float64)
    for fi in range(F):
        den_sum[fi * h:fi * h + N] += wsq
    for c in range(C):
        xc = x[:, c].astype(np.float64)
        X = np.fft.rfft(_frames_at(xc, a - lead, N) * w, axis=1)
        P = np.fft.rfft(_frames_at(xc, a - h - lead, N) * w, axis=1)
        X.imag[:, 0] = 0.0
        X.imag[:, -1] = 0.0
        P.imag[:, 0] = 0.0
        P.imag[:, -1] = 0.0
        mag = np.abs(X)
        q = X * np.conj(P)
        d = _angle_turns(q.real, q.imag) - adv[None, :]
        delta = (d - np.rint(d)).astype(np.float32).astype(np.float64)
        delta[0] = _angle_turns(X.real[0], X.imag[0]).astype(np.float32).astype(np.float64)
        phi = np.empty((F, K), np.float64)
        phi[0] = delta[0]
        for fi in range(1, F):                           # sequential, ascending f
            phi[fi] = phi[fi - 1] + (adv + delta[fi])
        Y = mag * np.cos(2.0 * np.pi * phi) + 1j * (mag * np.sin(2.0 * np.pi * phi))
        Y.imag[:, 0] = 0.0
        Y.imag[:, -1] = 0.0
        fr = np.fft.irfft(Y, n=N, axis=1) * w
        acc = np.zeros(n_out + N + F * h, np.float64)
        for fi in range(F):
            acc[fi * h:fi * h + N] += fr[fi]
        s = den_sum[lead:lead + n_out]
        y[:, c] = np.where(s < 1e-8, 0.0, acc[lead:lead + n_out] / np.where(s < 1e-8, 1.0, s))
    return y


def peak_frequency(y, n_edge):
    """Cycles per sample of the strongest bin of the Hann-windowed FFT of y[n_edge:-n_edge], by parabolic interpolation on the
    log magnitudes."""
    v = np.asarray(y, np.float64)[n_edge:len(y) - n_edge]
    n = len(v)
    wv = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)
    m = np.abs(np.fft.rfft(v * wv))
    i = int(np.argmax(m[1:-1])) + 1
    la, lb, lc = np.log(m[i - 1]), np.log(m[i]), np.log(m[i + 1])
    return (i + 0.5 * (la - lc) / (la - 2.0 * lb + lc)) / n
