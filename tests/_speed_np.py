"""numpy oracle of wun_gather_snippets_speed (include/wun.h): the contract restated -- the span v of a rated source, u / q / p of
every output frame and the fp32 fused multiply-add chain over the taps, k ascending -- on top of the oracle of the plain gather
(tests/_snippets_np.py).  The filter table is the library's own (wun_resample_design through ctypes, host only: the contract
says the kernel has no table of its own); nothing else is shared with the kernel or with the producers."""
import ctypes as C

import numpy as np

import _snippets_np
from _fma_chain_np import fmaf_np

from wave_u_net_amd import _lib

_TABLES = {}


def table(up, down):
    """wun_resample_design(up, down): fp32 [up, K], K = ceil((2 half + 1) / up), half = 10 max(up, down)."""
    if (up, down) not in _TABLES:
        lib = _lib.load()
        half = 10 * max(up, down)
        K = -(-(2 * half + 1) // up)
        n = int(lib.wun_resample_table_floats(up, down))
        assert n == up * K
        t = np.zeros(n, np.float32)
        assert lib.wun_resample_design(up, down, t.ctypes.data_as(C.POINTER(C.c_float)), n) == 0
        _TABLES[(up, down)] = t.reshape(up, K)
    return _TABLES[(up, down)]


def source_frames(t_in, up, down):
    return ((t_in - 1) * down) // up + 1


def resample_span(v, t_in, up, down):
    """r[t][c] of the contract for the span v [n_src, C] (+0 outside it): float32 [t_in, C]."""
    v = np.asarray(v, dtype=np.float32)
    tab = table(up, down)
    K, half, n_src = tab.shape[1], 10 * max(up, down), v.shape[0]
    u = np.arange(t_in, dtype=np.int64) * down + half
    q, p = u // up, u % up
    acc = np.zeros((t_in, v.shape[1]), np.float32)
    for k in range(K):
        m = q - k
        inside = (m >= 0) & (m < n_src)
        x = np.where(inside[:, None], v[np.where(inside, m, 0)], np.float32(0.0))
        acc = fmaf_np(tab[p, k][:, None], x, acc)
    return acc


def source_window(plane, rec, rate, bank, t_in):
    """a_s of the contract, float32 [t_in, C]; rate 0: the plain gather's window."""
    if rate == 0:
        return _snippets_np.source_window(plane, rec, t_in)
    up, down = bank[rate - 1]
    start, gain, flags = int(rec["start"]), np.float32(rec["gain"]), int(rec["flags"])
    n_src = source_frames(t_in, up, down)
    assert start >= 0 and start + n_src <= plane.shape[0], "span outside the plane"
    v = plane[start:start + n_src, :]
    if flags & _snippets_np.SWAP:
        v = v[:, ::-1]
    r = resample_span(v, t_in, up, down)
    a = r if gain == np.float32(1.0) else (gain * r).astype(np.float32)
    return -a if flags & _snippets_np.NEGATE else a


def gather(planes, table_, rates, bank, t_in, t_out):
    """(mix [B, t_in, C], targets [S, B, t_out, C]) of table_ [B, S] and rates [B, S] with mix_mode 1."""
    B, S = table_.shape
    pad = (t_in - t_out) // 2
    win = np.stack([np.stack([source_window(planes[s], table_[b, s], int(rates[b, s]), bank, t_in) for b in range(B)])
                    for s in range(S)])
    mix = win[0].copy()
    for s in range(1, S):
        mix = (mix + win[s]).astype(np.float32)
    return mix, np.ascontiguousarray(win[:, :, pad:pad + t_out, :])
