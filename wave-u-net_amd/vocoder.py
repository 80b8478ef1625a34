"""Time stretching and pitch shifting on the GPU: the phase vocoder of libwun.so (include/wun.h: wun_time_stretch; DESIGN.md
5.24).  time_stretch changes the tempo and keeps the pitch; pitch_shift is a stretch followed by the polyphase resampler at the
same ratio, which brings the length back and moves the pitch.  Every span is one job of a table, so a batch is one call: four
launches per 64 jobs.  There is no CPU path: a tensor that is not on a GPU is an error."""
import ctypes as C

import numpy as np
import torch

from . import _lib, resample, spectral

JOB_DTYPE = np.dtype([("x", "<u8"), ("y", "<u8"), ("n_in", "<i4"), ("n_out", "<i4"), ("num", "<i4"), ("den", "<i4")])
assert JOB_DTYPE.itemsize == C.sizeof(_lib.WunStretchJob)


def frames(n_in, num, den):
    """ceil(n_in * den / num): the longest output of a span of n_in frames at the tempo num / den (wun_time_stretch_frames)."""
    return _lib.count(_lib.load().wun_time_stretch_frames(int(n_in), int(num), int(den)))


def job_table(jobs):
    """The host table of wun_time_stretch from (x_ptr, y_ptr, n_in, n_out, num, den) tuples."""
    t = np.zeros(len(jobs), JOB_DTYPE)
    for i, j in enumerate(jobs):
        t[i] = tuple(int(v) for v in j)
    return t


def scratch_floats(table, channels, n_fft, hop):
    """Floats of scratch for this job table (wun_time_stretch_scratch_floats)."""
    table = np.ascontiguousarray(table, JOB_DTYPE)
    return _lib.count(_lib.load().wun_time_stretch_scratch_floats(table.ctypes.data, len(table), int(channels), int(n_fft),
                                                                  int(hop)))


def run(table, channels, n_fft, hop, scratch, device):
    """wun_time_stretch on a job table (JOB_DTYPE, device pointers) on the current stream of `device`; scratch is a float32
    tensor of at least scratch_floats(...) elements there.  No allocation beyond the cached FFT table, no synchronisation."""
    table = np.ascontiguousarray(table, JOB_DTYPE)
    device = torch.device(device)
    tab = spectral._fft_table(int(n_fft), device)
    with torch.cuda.device(device):
        stream = _lib.stream(device)
        _lib.check(_lib.load().wun_time_stretch(table.ctypes.data, len(table), int(channels), int(n_fft), int(hop), tab.data_ptr(),
                                                scratch.data_ptr(), stream))


def _check_audio(who, x):
    if not torch.is_tensor(x) or not x.is_cuda:
        raise ValueError("%s: x must be a torch tensor on a GPU (there is no CPU path)" % who)
    if x.dim() < 2 or x.dtype != torch.float32:
        raise ValueError("%s: x must be float32 [..., T, C]" % who)


def time_stretch(x, num, den, n_fft=2048, hop=512, length=None):
    """x [..., T, C] on the GPU played at the tempo num / den (above 1: faster and shorter) at constant pitch: [..., length, C],
    length = ceil(T * den / num) unless a shorter one is asked for.  One job per leading index, one call."""
    _check_audio("time_stretch", x)
    x = x.contiguous()
    T, ch = int(x.shape[-2]), int(x.shape[-1])
    full = frames(T, num, den)
    length = full if length is None else int(length)
    if not 1 <= length <= full:
        raise ValueError("time_stretch: length %d outside 1..%d (wun_time_stretch_frames)" % (length, full))
    lead = tuple(x.shape[:-2])
    n_jobs = int(np.prod(lead, dtype=np.int64)) if lead else 1
    y = torch.empty(lead + (length, ch), dtype=torch.float32, device=x.device)
    if n_jobs == 0:
        return y
    table = np.zeros(n_jobs, JOB_DTYPE)
    table["x"] = x.data_ptr() + 4 * T * ch * np.arange(n_jobs, dtype=np.uint64)
    table["y"] = y.data_ptr() + 4 * length * ch * np.arange(n_jobs, dtype=np.uint64)
    table["n_in"], table["n_out"], table["num"], table["den"] = T, length, int(num), int(den)
    scratch = torch.empty(scratch_floats(table, ch, n_fft, hop), dtype=torch.float32, device=x.device)
    run(table, ch, n_fft, hop, scratch, x.device)
    return y


def pitch_shift(x, up, down, n_fft=2048, hop=512):
    """x [..., T, C] on the GPU at the pitch times down / up and the same length T (the speed bank's convention: (18, 17) is
    about a semitone down): time_stretch at up / down to wun_speed_source_frames(T, up, down) frames, then resample by
    up / down to T."""
    _check_audio("pitch_shift", x)
    T, ch = int(x.shape[-2]), int(x.shape[-1])
    n_src = _lib.count(_lib.load().wun_speed_source_frames(T, int(up), int(down)))
    s = time_stretch(x, up, down, n_fft, hop, length=n_src)
    y = torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device)
    sv, yv = s.view(-1, n_src, ch), y.view(-1, T, ch)
    for i in range(sv.shape[0]):
        resample.resample_into(sv[i], yv[i], 0, T, int(up), int(down))
    return y
