"""An exact statement of the accumulation order include/wun.h promises for the 2-D convolutions: one float32
accumulator per output, started at +0, updated by one fused multiply-add per reduction index r = (ky 5 + kx) Cin + ci, r
ascending.  numpy only, so the statement shares no code with the kernels or with the float64 oracle tests/_specunet_np.py.

  fmaf_np(a, b, c)     the correctly rounded float32 of the exact a * b + c, elementwise on float32 arrays: the product is formed
                       in float64 (exact: 24 x 24 bits), c is added with TwoSum, and where the float64 sum is inexact and its last
                       bit is even it is stepped one float64 ulp toward the error term (round to odd), so the final rounding to
                       float32 sees on which side of every float32 tie the exact value lies.  The plain route
                       float32(float64(a) * b + c) rounds twice and is wrong on ties (tests/test_fma_chain_host.py holds a trap).
  chain(A, W)          acc[m][n] = fmaf(A[m][r], W[r][n], acc[m][n]) for r = 0, 1, ..: A [M, R] gathered inputs, W [R, N]
  gather_conv(x)       A of the strided conv, rows (b, y, x) of the output map, all 25 taps, 0 for a tap outside the map
  gather_transpose(x)  A of the transposed conv, rows (b, ty, tx), all 25 taps, 0 outside the map and for the taps that are not
                       of the output's parity class.  The kernels skip those taps instead; fma(0, w, acc) == acc for finite w
                       (acc is never -0 here: it starts at +0 and an exact cancellation gives +0), so the dense chain is the
                       same number.
  conv_weights(w), transpose_weights(w)   W [25 Cin, Cout] of TF's [5, 5, Cin, Cout] / [5, 5, Cout, Cin] kernels
"""
import numpy as np


def fmaf_np(a, b, c):
    a, b, c = (np.asarray(v, dtype=np.float32) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)      # exact
        c = c.astype(np.float64)
        s = p + c                                            # TwoSum: s + err == p + c exactly
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        odd = (s.view(np.int64) & 1) != 0              # (s is a fresh, contiguous result)
        step = np.isfinite(s) & np.isfinite(err) & (err != 0.0) & ~odd
        toward = np.where(err > 0.0, np.inf, -np.inf)
        s = np.where(step, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def chain(A, W):
    A, W = np.asarray(A, dtype=np.float32), np.asarray(W, dtype=np.float32)
    assert A.ndim == 2 and W.ndim == 2 and A.shape[1] == W.shape[0]
    acc = np.zeros((A.shape[0], W.shape[1]), dtype=np.float32)
    for r in range(A.shape[1]):
        acc = fmaf_np(A[:, r, None], W[None, r, :], acc)
    return acc


def _pick(x, iy, oky, ix, okx):
    """x[:, iy[i], ix[j], :] where oky[i] and okx[j], 0 elsewhere.  -> [B, len(iy), len(ix), C]"""
    g = x[:, np.where(oky, iy, 0)][:, :, np.where(okx, ix, 0)]
    return np.where((oky[:, None] & okx[None, :])[None, :, :, None], g, np.float32(0.0))


def gather_conv(x):
    """x [B, H, W, Cin] (H, W even) -> A [B (H / 2) (W / 2), 25 Cin]: A[(b, y, x)][(ky 5 + kx) Cin + ci] = x[b][2y + ky - 1][2x + kx - 1][ci]."""
    x = np.asarray(x, dtype=np.float32)
    B, H, W, ci = x.shape
    y, xx = np.arange(H // 2), np.arange(W // 2)
    taps = []
    for ky in range(5):
        for kx in range(5):
            iy, ix = 2 * y + ky - 1, 2 * xx + kx - 1
            taps.append(_pick(x, iy, (iy >= 0) & (iy < H), ix, (ix >= 0) & (ix < W)))
    return np.stack(taps, axis=3).reshape(B * (H // 2) * (W // 2), 25 * ci)


def gather_transpose(x):
    """x [B, H, W, Cin] -> A [B 2H 2W, 25 Cin]: A[(b, ty, tx)][(ky 5 + kx) Cin + ci] = x[b][jy][jx][ci] where 2 jy + ky - 1 == ty and
    2 jx + kx - 1 == tx have solutions on the map."""
    x = np.asarray(x, dtype=np.float32)
    B, H, W, ci = x.shape
    ty, tx = np.arange(2 * H), np.arange(2 * W)
    taps = []
    for ky in range(5):
        for kx in range(5):
            ny, nx = ty + 1 - ky, tx + 1 - kx
            taps.append(_pick(x, ny // 2, (ny % 2 == 0) & (ny >= 0) & (ny < 2 * H), nx // 2, (nx % 2 == 0) & (nx >= 0) & (nx < 2 * W)))
    return np.stack(taps, axis=3).reshape(B * 4 * H * W, 25 * ci)


def conv_weights(w):
    w = np.asarray(w, dtype=np.float32)
    return w.reshape(25 * w.shape[2], w.shape[3])


def transpose_weights(w):
    w = np.asarray(w, dtype=np.float32)
    return np.ascontiguousarray(w.transpose(0, 1, 3, 2)).reshape(25 * w.shape[3], w.shape[2])
