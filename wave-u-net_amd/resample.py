"""Sample-rate conversion of the audio boundary (the reference's Utils.resample, Utils.py:94-95): the rational polyphase
resampler of libwun.so (include/wun.h: wun_resample*) for tensors on the GPU, scipy.signal.resample_poly for numpy arrays
and CPU tensors.  Both use scipy's default filter (Kaiser window, beta = 5), NOT the resampy `kaiser_best` table behind
the reference's librosa call: the result is a correct band-limited resampling, not a bit-for-bit copy of librosa's.

Audio is [T, C] (or [T]) float32; the result has ceil(T * new_sr / orig_sr) frames.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

def ratio(orig_sr, new_sr):
    """(up, down) = new_sr / orig_sr reduced by their gcd (wun_resample_ratio)."""
    up, down = C.c_int32(), C.c_int32()
    _lib.check(_lib.load().wun_resample_ratio(int(orig_sr), int(new_sr), C.byref(up), C.byref(down)))
    return up.value, down.value


def frames(n_in, up, down):
    """ceil(n_in * up / down): the length rule of librosa and scipy (wun_resample_frames)."""
    return _lib.count(_lib.load().wun_resample_frames(int(n_in), int(up), int(down)))


def design(up, down):
    """The phase-major fp32 filter table of (up, down) as a numpy array [up, K] (wun_resample_design)."""
    lib = _lib.load()
    n = _lib.count(lib.wun_resample_table_floats(int(up), int(down)))
    table = np.zeros(n, np.float32)
    _lib.check(lib.wun_resample_design(int(up), int(down), table.ctypes.data_as(C.POINTER(C.c_float)), n))
    return table.reshape(int(up), n // int(up))


def _table(up, down, device):
    """The device tensor holding the phase-major fp32 filter table of (up, down), uploaded once per device."""
    return _lib.device_table(("resample", up, down), device, lambda: design(up, down))


def _map_channels_host(x, c_out):
    """The kernel's channel mapping in numpy: equal = per channel, c_out 1 = np.mean, 1 -> 2 = duplicate."""
    c_in = x.shape[1]
    if c_in == c_out:
        return x
    if c_out == 1:
        return np.mean(x, axis=1, keepdims=True)
    if c_in == 1 and c_out == 2:
        return np.tile(x, [1, 2])
    raise ValueError("channels must be equal, c_out = 1 (downmix) or 1 -> 2, got %d -> %d" % (c_in, c_out))


def resample_into(x, y, y_offset, n_out, up, down):
    """y[y_offset : y_offset + n_out] = the first n_out frames of x resampled by up / down, with the channel mapping
    x.shape[1] -> y.shape[1] applied to x first.  x [n_in, c_in] and y [>= y_offset + n_out, c_out] are float32,
    contiguous torch tensors on one device: on a GPU one wun_resample launch on the current stream (no allocation beyond
    the cached filter table, no synchronisation); on the CPU scipy.signal.resample_poly in float64."""
    assert x.dim() == 2 and y.dim() == 2 and x.device == y.device
    assert x.dtype == y.dtype == torch.float32 and x.is_contiguous() and y.is_contiguous()
    n_in, n_out, y_offset = int(x.shape[0]), int(n_out), int(y_offset)
    if not 0 <= n_out <= frames(n_in, up, down) or y_offset < 0 or y_offset + n_out > y.shape[0]:
        raise ValueError("resample_into: %d output frames at offset %d do not fit (%d input frames, %d / %d, y has %d)"
                         % (n_out, y_offset, n_in, up, down, y.shape[0]))
    if n_out == 0:
        return y
    if x.is_cuda:
        tab = _table(up, down, x.device) if up != down else None
        with torch.cuda.device(x.device):
            stream = _lib.stream(x.device)
            _lib.check(_lib.load().wun_resample(x.data_ptr(), n_in, int(x.shape[1]), y.data_ptr(), y_offset, n_out,
                                                int(y.shape[1]), tab.data_ptr() if tab is not None else None,
                                                int(up), int(down), stream))
        return y
    v = _map_channels_host(x.numpy(), int(y.shape[1]))
    if up != down:
        from scipy.signal import resample_poly
        v = resample_poly(v.astype(np.float64), up, down, axis=0).astype(np.float32)
    y[y_offset:y_offset + n_out] = torch.from_numpy(np.ascontiguousarray(v[:n_out], np.float32))
    return y


def resample(audio, orig_sr, new_sr, device=None):
    """Utils.resample (Utils.py:94-95).  A torch tensor on a GPU goes through the HIP kernel and comes back as a tensor
    on that GPU; a numpy array or CPU tensor goes through scipy.signal.resample_poly in float64 and comes back as float32
    of the same kind -- unless `device` names a GPU, in which case it is uploaded, resampled by the kernel and downloaded."""
    up, down = ratio(orig_sr, new_sr)
    is_tensor = torch.is_tensor(audio)
    x = audio if is_tensor else torch.from_numpy(np.ascontiguousarray(np.asarray(audio, dtype=np.float32)))
    squeeze = x.dim() == 1
    if squeeze:
        x = x[:, None]
    if x.dim() != 2:
        raise ValueError("audio must be [frames] or [frames, channels]")
    home = x.device
    if device is not None:
        x = x.to(torch.device(device))
    x = x.to(torch.float32).contiguous()
    y = torch.empty((frames(x.shape[0], up, down), x.shape[1]), dtype=torch.float32, device=x.device)
    resample_into(x, y, 0, y.shape[0], up, down)
    y = y.to(home)
    if squeeze:
        y = y[:, 0]
    return y if is_tensor else y.numpy()
