"""float64 oracle of the multichannel Wiener post-filter (include/wun.h: wun_wiener_filter), for the tests
only.  The header's comment is the definition; for one track with mix [n, C] and estimates [S, n, C], in the centred framing,
X = STFT(mix), E_s = STFT(est_s), vectors over the C channels:

    y_s(0)   = mask_s X, the soft-mask filter (mask_s = (A_s + mask_eps / S) / (sum_j A_j + mask_eps), A = |E|^p)
    for it = 1 .. I:
      v_s[f,k]  = (1 / C) sum_c |y_s[f,k,c]|^2
      R_s[k]    = (sum_f y_s[f,k] y_s[f,k]^H) / (eps + sum_f v_s[f,k])          over all F frames of the track
      Cxx[f,k]  = sum_s v_s[f,k] R_s[k] + sqrt(eps) I
      y_s[f,k] <- v_s[f,k] R_s[k] Cxx[f,k]^-1 X[f,k]
    out_s = ISTFT(y_s(I)) over [0, n)

Everything here is float64 -- the transforms (tests/_postfilter_np.py), the statistics, and the algebra through general C x C
matrices and numpy.linalg (no closed forms, no float32 spectra): the float32 storage of the device and of the CPU
WienerFilter is part of their distance from this oracle.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _postfilter_np as ora  # noqa: E402


def spectra(mix, est, n_fft, hop):
    """(X complex [C, F, K], E complex [S, C, F, K], lead)."""
    mix, est = np.asarray(mix, dtype=np.float64), np.asarray(est, dtype=np.float64)
    S, n, C = est.shape
    lead, F = ora.framing(n, n_fft, hop, True)
    xre, xim = ora.stft(mix.T, n_fft, hop, lead, F)
    ere, eim = ora.stft(est.transpose(0, 2, 1).reshape(S * C, n), n_fft, hop, lead, F)
    return xre + 1j * xim, (ere + 1j * eim).reshape(S, C, F, -1), lead


def masked(X, E, power, mask_eps):
    """y(0) [S, C, F, K]."""
    S = E.shape[0]
    a = np.abs(E) ** 2 if power == 2 else np.abs(E)
    return (a + mask_eps / S) / (a.sum(0) + mask_eps) * X


def em_step(y, X, eps):
    """One iteration: (the new y, Cxx^-1 X [F, K, C])."""
    S, C, F, K = y.shape
    v = (np.abs(y) ** 2).sum(1) / C                                                  # [S, F, K]
    yv = y.transpose(0, 2, 3, 1)                                                     # [S, F, K, C]
    R = (yv[..., :, None] * yv[..., None, :].conj()).sum(1) / (eps + v.sum(1))[:, :, None, None]       # [S, K, C, C]
    Cxx = (v[..., None, None] * R[:, None]).sum(0) + np.sqrt(eps) * np.eye(C)        # [F, K, C, C]
    z = np.linalg.solve(Cxx, X.transpose(1, 2, 0)[..., None])                        # [F, K, C, 1]
    new = v[..., None] * (R[:, None] @ z[None])[..., 0]                              # [S, F, K, C]
    return new.transpose(0, 3, 1, 2), z[..., 0]


def wiener_filter(mix, est, n_fft, hop, power=2, mask_eps=1e-10, iterations=1, eps=1e-10, details=False):
    """mix [n, C], est [S, n, C] -> out float64 [S, n, C]; with details also max |Cxx^-1 X| of the last iteration (0 when
    there is none) and the min over the bins of sum_j A_j."""
    S, n, C = np.asarray(est).shape
    mask_eps, eps = float(np.float32(mask_eps)), float(np.float32(eps))
    X, E, lead = spectra(mix, est, n_fft, hop)
    y = masked(X, E, power, mask_eps)
    zmax = 0.0
    for _ in range(iterations):
        y, z = em_step(y, X, eps)
        zmax = float(np.abs(z).max())
    F = y.shape[2]
    out = ora.istft(y.real.reshape(S * C, F, -1), y.imag.reshape(S * C, F, -1), n, n_fft, hop, lead)
    out = out.reshape(S, C, n).transpose(0, 2, 1)
    return (out, zmax, float((np.abs(E) ** power).sum(0).min())) if details else out


def regulariser_bound(zmax, n, n_fft, hop, eps=1e-10):
    """How far sum_s out_s may lie from the mix because of the regulariser: the y_s sum to X - sqrt(eps) Cxx^-1 X.  With every
    |(Cxx^-1 X)_c| <= zmax, a sample of an inverse frame is at most (1 / n_fft) sum_k c_k (|Re| + |Im|) <= sqrt(2 eps) zmax
    (sum_k c_k = n_fft); an output sample adds at most ceil(n_fft / hop) frames and divides by its window-square sum."""
    lead, F = ora.framing(n, n_fft, hop, True)
    ws = ora.window_sums(n, F, n_fft, hop, lead).min()
    return -(-n_fft // hop) * np.sqrt(2.0 * float(np.float32(eps))) * zmax / ws


def wiener_filter_fp32(mix, est, n_fft, hop, power=2, mask_eps=1e-10, iterations=1, eps=1e-10):
    """The same definition on a float32 stand-in: numpy float32 matmuls for the transforms (_postfilter_np.stft_fp32 /
    istft_fp32), every stored spectrum rounded to float32, the EM step of this module in float64 between them.  Its distance
    from wiener_filter is what float32 transforms and storage cost on the given inputs, whatever their conditioning: the
    tests bound the implementations by a multiple of it."""
    mix, est = np.asarray(mix, dtype=np.float32), np.asarray(est, dtype=np.float32)
    S, n, C = est.shape
    mask_eps, eps = float(np.float32(mask_eps)), float(np.float32(eps))
    lead, F = ora.framing(n, n_fft, hop, True)
    xre, xim = ora.stft_fp32(mix.T, n_fft, hop, lead, F)
    ere, eim = ora.stft_fp32(est.transpose(0, 2, 1).reshape(S * C, n), n_fft, hop, lead, F)
    X = (xre + 1j * xim).astype(np.complex128)
    E = (ere + 1j * eim).astype(np.complex128).reshape(S, C, F, -1)
    y = masked(X, E, power, mask_eps).astype(np.complex64).astype(np.complex128)
    for _ in range(iterations):
        y = em_step(y, X, eps)[0].astype(np.complex64).astype(np.complex128)
    out = ora.istft_fp32(y.real.reshape(S * C, F, -1), y.imag.reshape(S * C, F, -1), n, n_fft, hop, lead)
    return out.reshape(S, C, n).transpose(0, 2, 1)


def fixture(seed, S, n, C, n_fft, hop, power=2, iterations=1, details=False):
    """_postfilter_np.filter_fixture's recipe (Gaussian noise of amplitude 0.2 - 0.3) and the float64 Wiener output: (mix,
    est, out), with details also max |Cxx^-1 X|.  For S > 1 the mask must be well conditioned, as there: every bin of the
    summed estimates many orders above mask_eps (with one source the mask is 1 whatever the bin holds)."""
    rng = np.random.RandomState(seed)
    mix = (0.3 * rng.randn(n, C)).astype(np.float32)
    est = ((0.2 + 0.1 * rng.rand(S, 1, 1)) * rng.randn(S, n, C)).astype(np.float32)
    out, zmax, floor = wiener_filter(mix, est, n_fft, hop, power, iterations=iterations, details=True)
    assert S == 1 or floor > ora.MIN_ENERGY, "min sum_j A_j = %g" % floor
    return (mix, est, out, zmax) if details else (mix, est, out)


PANS = np.array([[1.0, 0.2], [0.3, 1.0]])


def panned_fixture(seed, n=1500):
    """Two spectrally overlapping noise sources at fixed pans [1, 0.2] and [0.3, 1]; the estimates are the true source +
    0.5 x the other source + 0.05 noise.  (mix [n, 2], estimates [2, n, 2], true sources [2, n, 2]), float32."""
    rng = np.random.RandomState(seed)
    src = rng.randn(2, n)[:, :, None] * PANS[:, None, :]                             # [2, n, 2]
    est = src + 0.5 * src[::-1] + 0.05 * rng.randn(2, n, 2)
    src = src.astype(np.float32)
    return src.sum(0), est.astype(np.float32), src


def rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, dtype=np.float64) ** 2)))
