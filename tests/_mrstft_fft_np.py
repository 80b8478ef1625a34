"""float64 oracle of the spectral loss's FFT path (include/wun.h: wun_stft_magnitude_fft, wun_spectral_loss_fft,
wun_spectral_loss_terms_fft), for the tests only.

The definitions are tests/_mrstft_np.py's (and, with mag_l1 alone, tests/_spectral_np.py's): the FFT entries compute the same
losses and the same gradient as their GEMM twins.  _mrstft_np.loss_and_grad / grad_fp32 multiply by a dense [n_fft, K] basis,
0.5 GB at n_fft = 8192; here the two frame transforms go through numpy.fft instead:

    forward    Re + i Im [r][f][k] = rfft(w frame_f)[k] on _spectral_np.frame_view's frames
    adjoint    dframe[n] = w[n] sum_{k = 0..n_fft/2} (cre[k] cos(2 pi n k / n_fft) - cim[k] sin(2 pi n k / n_fft)), every bin ONCE
               = w[n] (n_fft / 2) irfft(Z)[n] with Z[k] = cre[k] + i cim[k] between the edges and Z = 2 cre at k = 0 and n_fft / 2
               (irfft counts the bins between the edges twice and ignores the edges' imaginary parts, whose sines are 0)

mag_terms, source_sums, term_weights and the coefficient formula are _mrstft_np's, beta is _spectral_np's, by import.  The
float32 yardstick grad_fp32_fft is the same formula on scipy.fft with float32 input (pocketfft computes in the input's
precision; tests/_fft_np.py uses the same stand-in): what an FFT in float32 costs on these very inputs.

The module also holds the cases of tests/test_gpu_spectral_fft.py, so that tests/test_spectral_fft_host.py can check on the CPU
what the GPU test assumes of them (log_eps above four times the magnitude bound; the yardstick's own signs inside the tie rule).
"""
import os
import sys

import numpy as np
import scipy.fft

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mrstft_np as mr  # noqa: E402
import _spectral_np as sp  # noqa: E402
from _mrstft_np import TERMS, mag_terms, source_sums, term_weights  # noqa: E402,F401
from _spectral_np import beta  # noqa: E402,F401

SQRT2 = np.sqrt(2.0)
T_SMALL = 64 + 2 * 48 + 5          # 64 / 16: 7 frames per row; 64 / 48: 3
# name -> (S, B, C, Tout, resolutions, weights, log_eps).  T = n_fft + 2 hop + a small odd remainder: samples behind the last
# frame exist.  log_eps: the smallest power of two (1e-3 at n_fft 64) with every magnitude bound delta <= log_eps / 4 on the
# case's randn audio (test_spectral_fft_host.py::test_log_eps_of_the_cases recomputes the choice on the CPU).
CASES = {
    "64_16": (2, 3, 2, T_SMALL, [(64, 16)], [1.0], 1e-3),                            # 84 frame rows: 3 workgroups of 32, the last part-filled
    "64_48": (2, 3, 2, T_SMALL, [(64, 48)], [1.0], 1e-3),                            # few frames per row
    "512_128": (2, 1, 2, 512 + 2 * 128 + 3, [(512, 128)], [1.0], 2.0 ** -4),         # 4 frames per workgroup, pure radix 4
    "1024_768": (2, 2, 1, 1024 + 2 * 768 + 3, [(1024, 768)], [1.0], 2.0 ** -2),      # the reference's resolution; 2 frames per workgroup
    "2048_512": (2, 1, 1, 2048 + 2 * 512 + 5, [(2048, 512)], [1.0], 1.0),            # one frame per workgroup
    "4096_1024": (2, 1, 2, 4096 + 2 * 1024 + 5, [(4096, 1024)], [1.0], 4.0),         # 2 butterflies per lane, radix 2 last
    "8192_2048": (2, 1, 1, 8192 + 2 * 2048 + 5, [(8192, 2048)], [1.0], 16.0),        # 4 butterflies per lane, 64 KB LDS
    "two_resolutions": (2, 3, 2, 4096 + 2 * 1024 + 5, [(64, 48), (4096, 1024)], [1.0, 0.5], 4.0),
    "three_sources": (3, 3, 1, T_SMALL, [(64, 48)], [1.0], 1e-3),                    # three sources in one 1024-bin block
}
_CACHE = {}


def case(name):
    """Inputs of a case (randn audio from a fixed seed) and room for what tests compute from them once."""
    if name not in _CACHE:
        S, B, C, T, res, w, le = CASES[name]
        rng = np.random.RandomState(5160 + sorted(CASES).index(name))
        out = rng.randn(S, B, T, C).astype(np.float32)
        tgt = rng.randn(S, B, T, C).astype(np.float32)
        _CACHE[name] = {"out": out, "tgt": tgt, "res": res, "w": w, "log_eps": le, "S": S, "oracle": {}, "gpu_mags": None,
                        "gemm_mags": None}
    return _CACHE[name]


def stft(xr, n_fft, hop):
    """(Re, Im) float64 [R, F, K] of rows xr [R, T]: the loss's framing, no padding."""
    z = np.fft.rfft(sp.frame_view(np.asarray(xr, np.float64), n_fft, hop) * sp.window(n_fft), axis=-1)
    return np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)


def magnitude(x, n_fft, hop):
    """float64 [R, F, K] of audio [S, B, T, C]."""
    re, im = stft(sp.rows(x), n_fft, hop)
    return np.sqrt(re * re + im * im)


def _edges_doubled(cre, cim, ctype):
    z = (cre + 1j * cim).astype(ctype)
    z[..., 0] = 2.0 * cre[..., 0]
    z[..., -1] = 2.0 * cre[..., -1]
    return z


def adjoint(cre, cim, n_fft):
    """dframe float64 [R, F, n_fft]: sum_k cre Cb[n][k] + cim Sb[n][k] over the windowed bases, every bin once."""
    z = _edges_doubled(np.asarray(cre, np.float64), np.asarray(cim, np.float64), np.complex128)
    return np.fft.irfft(z, n=n_fft, axis=-1) * (0.5 * n_fft) * sp.window(n_fft)


def loss_and_grad(out, tgt, resolutions, weights, mse_weight, terms, log_eps, sc_eps, signs=None):
    """_mrstft_np.loss_and_grad through numpy.fft: (losses [2 + 5 nres], grad [S, B, T, C]) in float64.  signs: per resolution
    an [R, F, K] array used in place of sgn(Me - Mt) in the gradient (None: float64's own)."""
    out = np.asarray(out, dtype=np.float64)
    tgt = np.asarray(tgt, dtype=np.float64)
    w = term_weights(terms)
    S = out.shape[0]
    nres = len(resolutions)
    d = out - tgt
    mse = float(np.mean(d * d))
    g = mse_weight * 2.0 * d / d.size
    losses = np.zeros(2 + 5 * nres)
    losses[1] = mse
    total = mse_weight * mse
    xr, tr = sp.rows(out), sp.rows(tgt)
    T = xr.shape[1]
    for j, (n_fft, hop) in enumerate(resolutions):
        re, im = stft(xr, n_fft, hop)
        tre, tim = stft(tr, n_fft, hop)
        me, mt = np.sqrt(re * re + im * im), np.sqrt(tre * tre + tim * tim)
        mag, lg, sc, _ = mag_terms(me, mt, S, log_eps, sc_eps)
        cx = np.sqrt((re - tre) ** 2 + (im - tim) ** 2).mean()
        vals = [v if wt > 0 else 0.0 for v, wt in zip((mag, lg, sc, cx), w)]
        losses[2 + nres + 4 * j:2 + nres + 4 * j + 4] = vals
        losses[2 + j] = sum(wt * v for wt, v in zip(w, vals))
        total += weights[j] * losses[2 + j]
        sg = np.sign(me - mt) if signs is None else np.asarray(signs[j], dtype=np.float64)
        D, N = source_sums(me, mt, S)
        cre, cim = mr._coefficients(np, re, im, tre, tim, me, mt, sg, S, w, log_eps, sc_eps, D, N)
        g = g + sp.unrows(sp.overlap_add(adjoint(cre, cim, n_fft), T, hop) * weights[j], out.shape)
    losses[0] = total
    return losses, g


def _rows32(x):
    S, B, T, C = x.shape
    return np.ascontiguousarray(x.transpose(0, 1, 3, 2).reshape(S * B * C, T))


def stft_fp32(xr32, n_fft, hop):
    """(Re, Im) float32 of float32 rows: scipy's rfft of the float32 windowed frames (the window rounded once, one product)."""
    fr = np.ascontiguousarray(sp.frame_view(xr32, n_fft, hop)) * sp.window(n_fft).astype(np.float32)
    z = scipy.fft.rfft(fr, axis=-1)
    assert z.dtype == np.complex64
    return np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)


def magnitude_fp32(x, n_fft, hop):
    """float32 [R, F, K]: the yardstick's own magnitudes."""
    re, im = stft_fp32(_rows32(np.asarray(x, dtype=np.float32)), n_fft, hop)
    return np.sqrt(re * re + im * im)


def grad_fp32_fft(out, tgt, resolutions, weights, mse_weight, terms, log_eps, sc_eps, signs):
    """_mrstft_np.grad_fp32 with float32 FFTs in place of its float32 matmuls: the pinned-sign gradient formula in float32 (D_s
    and N_s summed in float64 from the fp32 d and Mt, as the definition has them).  Its distance from float64 is the yardstick
    of the GPU's (returns float32 [S, B, T, C])."""
    out32 = np.asarray(out, dtype=np.float32)
    tgt32 = np.asarray(tgt, dtype=np.float32)
    w = term_weights(terms)
    g = (out32 - tgt32) * np.float32(np.float64(np.float32(mse_weight)) * 2.0 / out32.size)
    S, B, T, C = out32.shape
    xr, tr = _rows32(out32), _rows32(tgt32)
    for j, (n_fft, hop) in enumerate(resolutions):
        re, im = stft_fp32(xr, n_fft, hop)
        tre, tim = stft_fp32(tr, n_fft, hop)
        me, mt = np.sqrt(re * re + im * im), np.sqrt(tre * tre + tim * tim)
        sg = np.asarray(signs[j], dtype=np.float32)
        D, N = source_sums(me, mt, S)
        cre, cim = mr._coefficients(np, re, im, tre, tim, me, mt, sg, S, [np.float32(x) for x in w], np.float32(log_eps),
                                    np.float64(np.float32(sc_eps)), D, N)
        z = _edges_doubled(cre.astype(np.float32), cim.astype(np.float32), np.complex64)
        fr = scipy.fft.irfft(z, n=n_fft, axis=-1)
        assert fr.dtype == np.float32
        dframe = fr * np.float32(0.5 * n_fft) * sp.window(n_fft).astype(np.float32)
        g = g + sp.unrows(sp.overlap_add(dframe, T, hop) * np.float32(weights[j]), out32.shape)
    return g.astype(np.float32)


def magnitude_bound(x, n_fft, hop, m64):
    """delta [R, F, K]: sqrt(2) beta + 2^-22 M, the bound of a float32 magnitude whatever the order of its transform's sums."""
    return SQRT2 * beta(x, n_fft, hop)[:, :, None] + 2.0 ** -22 * m64


def tie(out, tgt, n_fft, hop):
    """(d64, tie): float64's Me - Mt and where the two magnitudes tie within their bounds -- the only bins where the sign of a
    float32 difference may differ from float64's."""
    m_e, m_t = magnitude(out, n_fft, hop), magnitude(tgt, n_fft, hop)
    d64 = m_e - m_t
    return d64, np.abs(d64) <= magnitude_bound(out, n_fft, hop, m_e) + magnitude_bound(tgt, n_fft, hop, m_t)
