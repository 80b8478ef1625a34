"""Float64 numpy / scipy restatement of the BSS Eval v4 definition of DESIGN.md 5.9 (test infrastructure; written from the
definition, not from the device code): correlations by np.correlate (short signals) or FFT, np.linalg.solve for the filters,
scipy.signal.fftconvolve for the projections.

Shapes: references, estimates [S, n, C]; A = S * C reference signals, signal a = j * C + c."""
import numpy as np
from scipy.signal import fftconvolve

EPS = 2.0 ** -52
ENERGY_NAMES = ("s", "est", "est-s", "Pown-s", "Pown", "Pall-Pown", "Pall", "est-Pall")


def windows(n, window, hop):
    """(starts, lengths): nwin = floor((n - W + H) / H) windows [kH, kH + W), the last extended to n; n < W or no window:
    one window [0, n)."""
    if not window or n < window:
        return [0], [n]
    nwin = (n - window + hop) // hop
    starts = [k * hop for k in range(nwin)]
    lengths = [window] * nwin
    lengths[-1] = n - starts[-1]
    return starts, lengths


def _xcorr(x, y, L):
    """sum_t x[t] * y[t + l] for l in [0, L), signals zero outside [0, n)."""
    n = len(x)
    out = np.zeros(L)
    if n <= 4096:
        full = np.correlate(y, x, mode="full")          # full[k] = sum_t y[t + k - (n - 1)] * x[t]
        m = min(L, n)
        out[:m] = full[n - 1:n - 1 + m]
        return out
    nfft = 1 << int(np.ceil(np.log2(n + L)))
    r = np.fft.irfft(np.conj(np.fft.rfft(x, nfft)) * np.fft.rfft(y, nfft), nfft)
    return r[:L].copy()


def _signals(x):
    """[S, n, C] -> [A, n] float64, a = j * C + c."""
    S, n, C = x.shape
    return np.ascontiguousarray(np.transpose(x.astype(np.float64), (0, 2, 1)).reshape(S * C, n))


def correlations(references, estimates, L):
    """R[a][b][l] = r_ab[l], D[a][q][l] = d_a,q[l] for l in [0, L): [A, A, L] each (r_ab[-l] = R[b][a][l])."""
    s, e = _signals(references), _signals(estimates)
    A, n = s.shape
    R = np.zeros((A, A, L))
    D = np.zeros((A, A, L))
    if n > 4096:                                          # one FFT per signal, one inverse per pair
        nfft = 1 << int(np.ceil(np.log2(n + L)))
        fs, fe = np.fft.rfft(s, nfft, axis=1), np.fft.rfft(e, nfft, axis=1)
        for a in range(A):
            ca = np.conj(fs[a])
            for b in range(A):
                R[a, b] = np.fft.irfft(ca * fs[b], nfft)[:L]
                D[a, b] = np.fft.irfft(ca * fe[b], nfft)[:L]
        return R, D
    for a in range(A):
        for b in range(A):
            R[a, b] = _xcorr(s[a], s[b], L)
            D[a, b] = _xcorr(s[a], e[b], L)
    return R, D


def _gram(R, idx):
    """G[(a,l1),(b,l2)] = r_ab[l1 - l2] over the reference signals idx."""
    L = R.shape[2]
    m = len(idx)
    G = np.zeros((m, L, m, L))
    lag = np.arange(L)[:, None] - np.arange(L)[None, :]
    for i, a in enumerate(idx):
        for k, b in enumerate(idx):
            G[i, :, k, :] = np.where(lag >= 0, R[a, b][np.abs(lag)], R[b, a][np.abs(lag)])
    return G.reshape(m * L, m * L)


def _solve(G, D):
    try:
        return np.linalg.solve(G + EPS * np.eye(G.shape[0]), D)
    except np.linalg.LinAlgError:
        return np.linalg.lstsq(G, D, rcond=None)[0]


def filters(R, D, S, C):
    """C_all [S, A, L, C], C_own [S, C, L, C]: causal filters, est_j[t][c] ~ sum_a sum_l C[a][l][c] * s_a[t - l]."""
    A, L = S * C, R.shape[2]
    G = _gram(R, list(range(A)))
    c_all = np.zeros((S, A, L, C))
    c_own = np.zeros((S, C, L, C))
    for j in range(S):
        own = list(range(j * C, (j + 1) * C))
        Dj = np.transpose(D[:, own, :], (0, 2, 1))                     # [A, L, C]
        c_all[j] = _solve(G, Dj.reshape(A * L, C)).reshape(A, L, C)
        c_own[j] = _solve(_gram(R, own), Dj[own].reshape(C * L, C)).reshape(C, L, C)
    return c_all, c_own


def window_energies(references, estimates, starts, lengths, c_all=None, c_own=None):
    """[nwin, S, 8] (ENERGY_NAMES); without filters only the first three are computed (the rest 0)."""
    S, n, C = references.shape
    out = np.zeros((len(starts), S, 8))
    for k, (t0, w) in enumerate(zip(starts, lengths)):
        L = 1 if c_all is None else c_all.shape[2]
        pad = np.zeros((S, L - 1, C))
        s = np.concatenate([references[:, t0:t0 + w].astype(np.float64), pad], axis=1)
        e = np.concatenate([estimates[:, t0:t0 + w].astype(np.float64), pad], axis=1)
        for j in range(S):
            out[k, j, 0] = np.sum(s[j] ** 2)
            out[k, j, 1] = np.sum(e[j] ** 2)
            out[k, j, 2] = np.sum((e[j] - s[j]) ** 2)
            if c_all is None:
                continue
            p_all = np.zeros((w + L - 1, C))
            p_own = np.zeros((w + L - 1, C))
            for jj in range(S):
                for cc in range(C):
                    sl = s[jj, :w, cc]
                    for c in range(C):
                        p_all[:, c] += fftconvolve(sl, c_all[j, jj * C + cc, :, c]) if w + L > 64 else np.convolve(sl, c_all[j, jj * C + cc, :, c])
                        if jj == j:
                            p_own[:, c] += fftconvolve(sl, c_own[j, cc, :, c]) if w + L > 64 else np.convolve(sl, c_own[j, cc, :, c])
            out[k, j, 3] = np.sum((p_own - s[j]) ** 2)
            out[k, j, 4] = np.sum(p_own ** 2)
            out[k, j, 5] = np.sum((p_all - p_own) ** 2)
            out[k, j, 6] = np.sum(p_all ** 2)
            out[k, j, 7] = np.sum((e[j] - p_all) ** 2)
    return out


def _db(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(b == 0, np.inf, 10.0 * np.log10(a / np.where(b == 0, 1.0, b)))


def metrics_from_energies(E, names=("SDR", "ISR", "SIR", "SAR")):
    """{metric: [S, nwin]} from [nwin, S, 8]; a window where any reference or any estimate is all zero is NaN throughout."""
    E = np.asarray(E, np.float64)
    table = {"SDR": (0, 2), "ISR": (0, 3), "SIR": (4, 5), "SAR": (6, 7)}
    silent = np.any(E[:, :, 0] == 0, axis=1) | np.any(E[:, :, 1] == 0, axis=1)      # [nwin]
    out = {}
    for m in names:
        a, b = table[m]
        v = _db(E[:, :, a], E[:, :, b]).astype(np.float64)
        v[silent, :] = np.nan
        out[m] = np.ascontiguousarray(v.T)
    return out


def bss_eval(references, estimates, sr, window=1.0, hop=1.0, filters_len=512, metrics=("SDR", "ISR", "SIR", "SAR")):
    references = np.asarray(references, np.float32)
    estimates = np.asarray(estimates, np.float32)
    S, n, C = references.shape
    if window is None:
        starts, lengths = windows(n, 0, 0)
    else:
        starts, lengths = windows(n, int(window * sr), int(hop * sr))
    if tuple(metrics) == ("SDR",):
        E = window_energies(references, estimates, starts, lengths)
    else:
        R, D = correlations(references, estimates, filters_len)
        c_all, c_own = filters(R, D, S, C)
        E = window_energies(references, estimates, starts, lengths, c_all, c_own)
    return metrics_from_energies(E, metrics)
