"""The numpy statement of blended separation (include/wun.h "blended separation"): every output frame is a
weighted mean over every window that covers it, windows taken in the order of the window list.

  pass_windows(Tout, n, V, s)          one pass: [(pos, k, flags)], pos = k (Tout - V) - s, K = 1 + ceil(max(0, n + s - Tout) / H)
  window_list(Tout, n, V, shifts)      the passes one behind the other
  weights(Tout, V, flags)              float32 [Tout]: float32(min(t + 1, Tout - t, V + 1)) / float32(V + 1), no rising ramp with
                                       NO_RISE, no falling ramp with NO_FALL
  accumulate(outputs, windows, V, acc, den)   for g ascending: acc = fmaf(w_g, x_g, acc), den = den + w_g     (in place)
  finish(acc, den)                     acc / den, +0 where den == 0
  blend(outputs, windows, V, frames)   the three together from zeros

A loop over windows, then over the frames of each: every frame meets its covering windows in ascending g.  The chain uses
fmaf_np of tests/_fma_chain_np.py; nothing here comes from the package."""
import numpy as np

from _fma_chain_np import fmaf_np

NO_RISE, NO_FALL = 1, 2


def pass_windows(tout, n_frames, v, shift):
    assert tout >= 1 and n_frames >= 1 and 0 <= v <= tout - 1 and shift >= 0
    h = tout - v
    over = max(0, n_frames + shift - tout)
    k_count = 1 + -(-over // h)
    return [(k * h - shift, k, (NO_RISE if k == 0 else 0) | (NO_FALL if k == k_count - 1 else 0)) for k in range(k_count)]


def window_list(tout, n_frames, v, shifts):
    out = []
    for s in shifts:
        out.extend(pass_windows(tout, n_frames, v, s))
    return out


def weights(tout, v, flags):
    w = np.empty(tout, dtype=np.float32)
    for t in range(tout):
        m = v + 1
        if not flags & NO_RISE:
            m = min(m, t + 1)
        if not flags & NO_FALL:
            m = min(m, tout - t)
        w[t] = np.float32(m) / np.float32(v + 1)
    return w


def accumulate(outputs, windows, v, acc, den):
    """outputs float32 [S, B, Tout, C]; windows [(pos, row, flags)]; acc float32 [S, frames, C]; den float32 [frames]."""
    outputs = np.asarray(outputs, dtype=np.float32)
    tout, frames = outputs.shape[2], acc.shape[1]
    assert acc.dtype == np.float32 and den.dtype == np.float32
    for pos, row, flags in windows:
        w = weights(tout, v, flags)
        t0, t1 = max(0, -pos), min(tout, frames - pos)       # the frames of one window are distinct: all at once
        if t0 >= t1:
            continue
        acc[:, pos + t0:pos + t1, :] = fmaf_np(w[None, t0:t1, None], outputs[:, row, t0:t1, :], acc[:, pos + t0:pos + t1, :])
        den[pos + t0:pos + t1] = den[pos + t0:pos + t1] + w[t0:t1]
    return acc, den


def finish(acc, den):
    live = den != 0
    out = np.zeros_like(acc)
    out[:, live, :] = acc[:, live, :] / den[None, live, None]       # float32 / float32
    return out


def blend(outputs, windows, v, frames):
    outputs = np.asarray(outputs, dtype=np.float32)
    acc = np.zeros((outputs.shape[0], frames, outputs.shape[3]), np.float32)
    den = np.zeros(frames, np.float32)
    accumulate(outputs, windows, v, acc, den)
    return finish(acc, den), den
