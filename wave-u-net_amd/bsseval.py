"""BSS Eval v4 (SDR / ISR / SIR / SAR, image version) on the device -- the scoring the reference leaves to
museval.eval_mus_track at the end of Evaluate.predict (Evaluate.py:146-158).  DESIGN.md 5.9 holds the definition this module
implements; parity with a museval-written JSON file is NOT claimed (museval is not available where this was developed).

Hot path: the lagged correlations and the windowed projections + energies are HIP kernels of libwun.so
(include/wun.h: wun_bss_correlations, wun_bss_window_energies).  Plumbing in between: the block-Toeplitz system is
assembled from the correlation buffers and solved in float64 with torch.linalg -- on the HOST by default (`solve_device`),
see DESIGN.md 5.9 for why.  There is no CPU fallback for the kernels: tensors are scored on a GPU.
"""
import ctypes as C
import json
import os

import numpy as np
import torch

from . import _lib

METRICS = ("SDR", "ISR", "SIR", "SAR")
EPS = 2.0 ** -52
_ENERGY_PAIR = {"SDR": (0, 2), "ISR": (0, 3), "SIR": (4, 5), "SAR": (6, 7)}
LAUNCHES = {"correlations": 0, "energies": 0}      # calls of the two entries made by this module (tests, tools)


def window_table(n, window, hop):
    """(starts, lengths) in frames, as python lists (wun_bss_windows): windows [k hop, k hop + window), the last one extended
    to n; window 0 / None or n < window: one window over everything."""
    lib = _lib.load()
    window, hop = int(window or 0), int(hop or 0)
    count = _lib.count(lib.wun_bss_windows(int(n), window, hop, None, None, 0))
    starts, lengths = (C.c_int64 * count)(), (C.c_int64 * count)()
    got = _lib.count(lib.wun_bss_windows(int(n), window, hop, starts, lengths, count))
    return list(starts), list(lengths)


def scratch_doubles(S, n, Cc, L, nwin, max_len):
    return _lib.count(_lib.load().wun_bss_scratch_doubles(int(S), int(n), int(Cc), int(L), int(nwin), int(max_len)))


def _as_device(x, device):
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))
    if t.dim() != 3:
        raise ValueError("signals must be [S, n, C], got shape %s" % (tuple(t.shape),))
    return t.to(device=device, dtype=torch.float32).contiguous()


def _pick_device(references, estimates, device):
    if device is not None:
        return torch.device(device)
    for x in (references, estimates):
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    return torch.device("cuda:0")


def correlations(references, estimates, filters_len=512, scratch=None):
    """(R, D): float64 device tensors [A, A, L], R[a][b][l] = sum_t s_a[t] s_b[t + l], D[a][q][l] = sum_t s_a[t] est_q[t + l]
    for l in [0, L); negative lags are r_ab[-l] = R[b][a][l].  references, estimates: float32 device tensors [S, n, C]."""
    S, n, Cc = (int(v) for v in references.shape)
    L, A = int(filters_len), S * Cc
    dev = references.device
    if scratch is None:
        scratch = torch.empty(scratch_doubles(S, n, Cc, L, 0, 0), dtype=torch.float64, device=dev)
    R = torch.empty((A, A, L), dtype=torch.float64, device=dev)
    D = torch.empty((A, A, L), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().wun_bss_correlations(references.data_ptr(), estimates.data_ptr(), S, n, Cc, L, R.data_ptr(),
                                                    D.data_ptr(), scratch.data_ptr(), _lib.stream(dev)))
    LAUNCHES["correlations"] += 1
    return R, D


def window_energies(references, estimates, starts, lengths, c_all=None, c_own=None, filters_len=512, scratch=None):
    """float64 device tensor [nwin, S, 8] (include/wun.h: wun_bss_window_energies).  c_all [S, A, L, C] and c_own [S, C, L, C]
    float64 device tensors, or both None: the filter-free form (energies 0..2 only)."""
    S, n, Cc = (int(v) for v in references.shape)
    dev = references.device
    nwin = len(starts)
    L = int(c_all.shape[2]) if c_all is not None else int(filters_len)
    if scratch is None:
        scratch = torch.empty(scratch_doubles(S, n, Cc, L if c_all is not None else 1, nwin, max(lengths)),
                              dtype=torch.float64, device=dev)
    out = torch.empty((nwin, S, 8), dtype=torch.float64, device=dev)
    st, ln = (C.c_int64 * nwin)(*starts), (C.c_int64 * nwin)(*lengths)
    if c_all is not None:
        assert c_all.dtype == c_own.dtype == torch.float64 and c_all.is_contiguous() and c_own.is_contiguous()
        assert tuple(c_all.shape) == (S, S * Cc, L, Cc) and tuple(c_own.shape) == (S, Cc, L, Cc)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().wun_bss_window_energies(
            references.data_ptr(), estimates.data_ptr(), S, n, Cc, L,
            c_all.data_ptr() if c_all is not None else None, c_own.data_ptr() if c_own is not None else None,
            st, ln, nwin, out.data_ptr(), scratch.data_ptr(), _lib.stream(dev)))
    LAUNCHES["energies"] += 1
    return out


def _gram(Rfull, idx, L):
    """G[(a,l1),(b,l2)] = r_ab[l1 - l2] over the signals idx, from Rfull[a][b][lag + L - 1]."""
    lag = (torch.arange(L, device=Rfull.device)[:, None] - torch.arange(L, device=Rfull.device)[None, :]) + (L - 1)
    sub = Rfull[idx][:, idx]                                   # [m, m, 2L - 1]
    m = len(idx)
    return sub[:, :, lag].permute(0, 2, 1, 3).reshape(m * L, m * L)


def _solve(G, D):
    G = G.clone()
    G.diagonal().add_(EPS)
    try:
        X = torch.linalg.solve(G, D)
        if bool(torch.isfinite(X).all()):
            return X
    except RuntimeError:
        pass
    G.diagonal().sub_(EPS)
    return torch.linalg.lstsq(G, D).solution


def solve_filters(R, D, S, Cc, solve_device="cpu"):
    """C_all [S, A, L, C], C_own [S, C, L, C] (float64, on R's device) from the correlation buffers: solve(G + eps I, D_j) with
    eps = 2^-52, least squares if the solve fails.  G is common to all sources, so C_all is ONE factorisation with S * C right-hand
    sides; C_own is one [C L, C L] system per source.  solve_device: where torch.linalg runs ("cpu" default, or R's device)."""
    A, L = S * Cc, int(R.shape[2])
    home = R.device
    where = home if solve_device in (None, "device") else torch.device(solve_device)
    R, D = R.to(where), D.to(where)
    Rfull = torch.cat([R.transpose(0, 1)[:, :, 1:].flip(2), R], dim=2)      # [A, A, 2L - 1]: index lag + L - 1
    rhs = D.permute(0, 2, 1).reshape(A * L, A)                               # [(a, l), q]
    c_all = _solve(_gram(Rfull, list(range(A)), L), rhs).reshape(A, L, S, Cc).permute(2, 0, 1, 3).contiguous()
    c_own = torch.empty((S, Cc, L, Cc), dtype=torch.float64, device=where)
    for j in range(S):
        own = list(range(j * Cc, (j + 1) * Cc))
        rj = D[own][:, own].permute(0, 2, 1).reshape(Cc * L, Cc)
        c_own[j] = _solve(_gram(Rfull, own, L), rj).reshape(Cc, L, Cc)
    return c_all.to(home), c_own.to(home)


def metrics_from_energies(E, metrics=METRICS):
    """{metric: float64 numpy [S, nwin]} from the energies [nwin, S, 8] (host array).  db(a, b) = +inf if b == 0; a window in
    which any source's reference or estimate slice is all zero is NaN for every metric of every source."""
    E = np.asarray(E, np.float64)
    silent = np.any(E[:, :, 0] == 0, axis=1) | np.any(E[:, :, 1] == 0, axis=1)
    out = {}
    for m in metrics:
        a, b = _ENERGY_PAIR[m]
        num, den = E[:, :, a], E[:, :, b]
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.where(den == 0, np.inf, 10.0 * np.log10(num / np.where(den == 0, 1.0, den)))
        v = v.astype(np.float64)
        v[silent, :] = np.nan
        out[m] = np.ascontiguousarray(v.T)
    return out


def bss_eval(references, estimates, sr, window=1.0, hop=1.0, filters_len=512, metrics=METRICS, device=None,
             solve_device="cpu", return_energies=False):
    """BSS Eval v4 of estimates against references: float32 tensors or arrays [S, n, C] at sample rate sr, same source order.
    window, hop in seconds (museval: 1.0 each; frames = int(seconds * sr)); window=None: one window over everything.
    Returns {metric: float64 numpy [S, nwin]} (with return_energies also the [nwin, S, 8] energies).  metrics=("SDR",) computes
    neither correlations nor filters.  Arrays and CPU tensors are uploaded to `device` (default: the inputs' GPU, else cuda:0)."""
    metrics = tuple(metrics)
    for m in metrics:
        if m not in _ENERGY_PAIR:
            raise ValueError("unknown metric %r (have %s)" % (m, ", ".join(METRICS)))
    dev = _pick_device(references, estimates, device)
    if dev.type != "cuda":
        raise RuntimeError("bss_eval runs its kernels on a GPU; there is no CPU fallback (got device %s)" % dev)
    refs, ests = _as_device(references, dev), _as_device(estimates, dev)
    if refs.shape != ests.shape:
        raise ValueError("references %s and estimates %s differ in shape" % (tuple(refs.shape), tuple(ests.shape)))
    S, n, Cc = (int(v) for v in refs.shape)
    if window is None:
        starts, lengths = window_table(n, 0, 0)
    else:
        starts, lengths = window_table(n, int(window * sr), int(hop * sr))
    L = int(filters_len)
    need_filters = any(m != "SDR" for m in metrics)
    if need_filters:
        R, D = correlations(refs, ests, L)
        c_all, c_own = solve_filters(R, D, S, Cc, solve_device)
        E = window_energies(refs, ests, starts, lengths, c_all, c_own)
    else:
        E = window_energies(refs, ests, starts, lengths, filters_len=L)
    E = E.cpu().numpy()
    out = metrics_from_energies(E, metrics)
    return (out, E) if return_energies else out


# ---- museval's JSON layout and the reference's statistics over it ------------------------------
def track_json(source_names, scores, window=1.0, hop=1.0):
    """museval's per-track layout: {"targets": [{"name", "frames": [{"time", "duration", "metrics": {...}}]}]}."""
    targets = []
    for j, name in enumerate(source_names):
        nwin = len(next(iter(scores.values()))[j])
        frames = [{"time": float(k * hop), "duration": float(window),
                   "metrics": {m: float(scores[m][j][k]) for m in METRICS if m in scores}} for k in range(nwin)]
        targets.append({"name": name, "frames": frames})
    return {"targets": targets}


def write_track_json(path, source_names, scores, window=1.0, hop=1.0):
    """NaN / inf are written as the NaN / Infinity literals json.load reads back."""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(track_json(source_names, scores, window, hop), f, indent=2, allow_nan=True)
    return path
