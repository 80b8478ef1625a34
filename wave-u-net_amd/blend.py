"""Blended separation (include/wun.h: wun_blend_positions, wun_blend_windows, wun_blend_finish): overlapping
hops cross-faded with a trapezoid and several shifted passes averaged, as ONE weighted mean per output frame over every window
that covers it, taken in the order of the window list.

  window_table(Tout, n_frames, V, shifts)   the window list of a separation: int64 [nwin, 3], columns (pos, row, flags), the
                                            passes one behind the other; row counts inside a pass (renumber it per chunk)
  shift_offsets(n, max_shift)               n evenly spread shifts 0 <= s < max_shift, no random numbers
  blend_windows(outputs, windows, V, preds, den)   accumulate the windows of one table, in table order
  blend_finish(preds, den)                  preds /= den, +0 where nothing was accumulated

Device tensors go through the library's kernels.  CPU tensors (numpy stand-in separators) go through the restatement below, which
gives the same bits: the chain of a frame is float32 fused multiply-adds in table order, whichever side runs it.
"""
import numpy as np
import torch

from . import _lib

NO_RISE, NO_FALL = _lib.BLEND_NO_RISE, _lib.BLEND_NO_FALL


def shift_offsets(n, max_shift):
    n, max_shift = int(n), int(max_shift)
    if n < 1 or max_shift < 0:
        raise ValueError("shift_offsets: need n >= 1 and max_shift >= 0, got %d, %d" % (n, max_shift))
    return [j * max_shift // n for j in range(n)]


def window_table(output_frames, n_frames, overlap_frames, shifts):
    lib = _lib.load()
    parts = []
    for s in shifts:
        k = _lib.count(lib.wun_blend_positions(int(output_frames), int(n_frames), int(overlap_frames), int(s), None, 0))
        buf = (_lib.WunBlendWindow * k)()
        _lib.count(lib.wun_blend_positions(int(output_frames), int(n_frames), int(overlap_frames), int(s), buf, k))
        parts.append(np.array([(w.pos, w.row, w.flags) for w in buf], dtype=np.int64).reshape(k, 3))
    if not parts:
        raise ValueError("window_table: no shifts")
    return np.concatenate(parts)


def _windows_arg(windows):
    tab = np.asarray(windows, dtype=np.int64).reshape(-1, 3)
    buf = (_lib.WunBlendWindow * max(1, tab.shape[0]))()
    for i, (pos, row, flags) in enumerate(tab.tolist()):
        buf[i].pos, buf[i].row, buf[i].flags = pos, row, flags
    return tab, buf


def _check_tensors(outputs, preds, den):
    if outputs.dim() != 4 or preds.dim() != 3 or den.dim() != 1:
        raise ValueError("blend: outputs [S, B, Tout, C], preds [S, frames, C] and den [frames] expected")
    for t in (outputs, preds, den):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != preds.device:
            raise ValueError("blend: float32 contiguous tensors on one device expected")
    if outputs.shape[0] != preds.shape[0] or outputs.shape[3] != preds.shape[2] or den.shape[0] != preds.shape[1]:
        raise ValueError("blend: outputs %s, preds %s and den %s do not fit" % (tuple(outputs.shape), tuple(preds.shape),
                                                                                tuple(den.shape)))


def blend_windows(outputs, windows, overlap_frames, preds, den):
    """preds (the accumulator) and den, zeroed by the caller before the first table of a separation, take the windows of
    `windows` ([nwin, 3]: pos, row of outputs, flags) in table order.  outputs [S, B, Tout, C]; returns preds."""
    _check_tensors(outputs, preds, den)
    tab, buf = _windows_arg(windows)
    S, B, tout, ch = (int(v) for v in outputs.shape)
    if preds.device.type != "cpu":
        lib = _lib.load()
        _lib.check(lib.wun_blend_windows(outputs.data_ptr(), S, B, tout, ch, buf, int(tab.shape[0]), int(overlap_frames),
                                         preds.data_ptr(), den.data_ptr(), int(preds.shape[1]), _lib.stream(preds.device)))
        return preds
    _blend_windows_cpu(outputs.numpy(), tab, int(overlap_frames), preds.numpy(), den.numpy())
    return preds


def blend_finish(preds, den):
    if preds.dim() != 3 or den.dim() != 1 or den.shape[0] != preds.shape[1]:
        raise ValueError("blend_finish: preds [S, frames, C] and den [frames] expected")
    for t in (preds, den):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != preds.device:
            raise ValueError("blend_finish: float32 contiguous tensors on one device expected")
    if preds.device.type != "cpu":
        lib = _lib.load()
        _lib.check(lib.wun_blend_finish(preds.data_ptr(), den.data_ptr(), int(preds.shape[0]), int(preds.shape[1]),
                                        int(preds.shape[2]), _lib.stream(preds.device)))
        return preds
    p, d = preds.numpy(), den.numpy()
    live = d != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = p / d[None, :, None]                              # float32 / float32: one correctly rounded division
    p[...] = np.where(live[None, :, None], q, np.float32(0.0))
    return preds


# ---- the CPU restatement ----
def _fma32(a, b, c):
    """The correctly rounded float32 of a * b + c, elementwise.  The product is exact in float64; s = fl64(product + c) and
    the rounding error e of that sum are known exactly (TwoSum).  Rounding s to float32 is the answer unless s lies exactly
    half way between two float32 values and e != 0: then the exact sum lies on e's side of the tie."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)
    r = s.astype(np.float32)
    back = r.astype(np.float64)
    lo = np.where(back <= s, r, np.nextafter(r, np.float32(-np.inf)))
    hi = np.where(back >= s, r, np.nextafter(r, np.float32(np.inf)))
    tie = (lo != hi) & ((s - lo.astype(np.float64)) == (hi.astype(np.float64) - s))
    return np.where(tie & (e > 0), hi, np.where(tie & (e < 0), lo, r)).astype(np.float32)


def _weights(t, tout, v, flags):
    m = np.full(t.shape, v + 1, dtype=np.int64)
    if not flags & NO_RISE:
        m = np.minimum(m, t + 1)
    if not flags & NO_FALL:
        m = np.minimum(m, tout - t)
    return m.astype(np.float32) / np.float32(v + 1)


def _blend_windows_cpu(outputs, tab, v, preds, den):
    S, B, tout, ch = outputs.shape
    frames = preds.shape[1]
    if not 0 <= v <= tout - 1:
        raise ValueError("blend_windows: overlap_frames must be in [0, Tout - 1]")
    for pos, row, flags in tab.tolist():                      # table order: every frame meets its windows in ascending g
        if not 0 <= row < B or flags & ~(NO_RISE | NO_FALL):
            raise ValueError("blend_windows: a window names a row outside [0, B) or has unknown flag bits")
        lo, hi = max(pos, 0), min(pos + tout, frames)
        if lo >= hi:
            continue
        w = _weights(np.arange(lo - pos, hi - pos, dtype=np.int64), tout, v, flags)
        preds[:, lo:hi] = _fma32(w[None, :, None], outputs[:, row, lo - pos:hi - pos], preds[:, lo:hi])
        den[lo:hi] = den[lo:hi] + w
