"""Float64 numpy oracle of the rest of the EBU R 128 meter, written from the definitions and independently of
the device code, on top of tests/_loudness_np.py:
  oversampling       the true-peak oversampling factor of a sample rate
  true_peak          max |scipy.signal.resample_poly(x, L, 1)|, overall and per channel
  short_term         the 3 s blocks at the meter's 0.1 s step: geometry, mean squares z3, loudness s
  loudness_range     both gates on the short-term values and the two ranks of the sorted survivors
  r128               the eight readings of the report"""
import numpy as np

import _loudness_np as ora


def oversampling(sr):
    L = 1
    while L < 32 and L * int(sr) < 176400:
        L *= 2
    return L


def true_peak(x, sr, L=None):
    """(overall, per channel [C]) of x [n, C]: the float64 maximum of |resample_poly(x, L, 1)| (scipy's default Kaiser design)."""
    from scipy.signal import resample_poly
    x = np.asarray(x, np.float64)
    L = oversampling(sr) if L is None else int(L)
    r = resample_poly(x, L, 1, axis=0) if L > 1 else x
    per = np.max(np.abs(r), axis=0)
    return float(per.max()), per


def short_term_geometry(n, sr):
    N3, step = (30 * int(sr) + 5) // 10, (int(sr) + 5) // 10          # round(3 sr), round(0.1 sr), halves up
    nb3 = (n - N3) // step + 1 if n >= N3 else 0
    return N3, step, nb3


def short_term(x, sr, filt=ora.sosfilt_fast):
    """(z3 [nb3], s [nb3]) of x [n, C]: the K-weighted mean squares of the 3 s blocks summed over the channels, and their
    loudness."""
    x = np.asarray(x)
    y = filt(ora.kweight_sos(sr), x)
    N3, step, nb3 = short_term_geometry(x.shape[0], sr)
    z3 = np.array([np.sum(np.mean(y[j * step:j * step + N3] ** 2, axis=0)) for j in range(nb3)], np.float64).reshape(nb3)
    with np.errstate(divide="ignore"):
        return z3, -0.691 + 10.0 * np.log10(z3)


def ranks(m):
    return ((m - 1) * 10 + 50) // 100, ((m - 1) * 95 + 50) // 100


def loudness_range(z3, s):
    """(LRA, kept mask, relative gate, indices (lo, hi) of the two selected blocks or None): absolute gate s > -70, relative gate
    20 LU under the absolute-gated mean, both strict; the survivors sorted ascending, ties by block index."""
    if np.isnan(s).any():
        return np.nan, np.zeros(s.shape, bool), np.nan, None
    absg = s > -70.0
    if not absg.any():
        return 0.0, absg, np.nan, None
    gate = -0.691 + 10.0 * np.log10(np.mean(z3[absg])) - 20.0
    keep = absg & (s > gate)
    idx = np.nonzero(keep)[0]
    if idx.size == 0:
        return 0.0, keep, gate, None
    order = idx[np.argsort(s[idx], kind="stable")]                       # stable: ties by block index
    lo, hi = ranks(idx.size)
    return float(s[order[hi]] - s[order[lo]]), keep, gate, (int(order[lo]), int(order[hi]))


def r128(x, sr):
    """The report [8] of x [n, C] as float64 numpy, and the short-term values s."""
    L, kept, nb, peak, l = ora.loudness(x, sr)
    z3, s = short_term(x, sr)
    lra, keep, _, _ = loudness_range(z3, s)
    tp = true_peak(x, sr)[0]
    top = lambda v: float(np.max(v)) if v.size else -np.inf              # noqa: E731
    return np.array([L, lra, top(l), top(s), tp, peak, kept, int(keep.sum())], np.float64), s
