"""Integrated loudness (ITU-R BS.1770-4 / EBU R 128) and loudness normalisation on the device, and the recursive filter
underneath it.  DESIGN.md 5.27 holds the definition; the kernels are libwun.so's (include/wun.h: wun_sosfilt, wun_loudness,
wun_loudness_gain, wun_scale_by).  The reference has no counterpart: it feeds a file at whatever level it arrives.

Nothing here reads a device value on the host: the meter, the gain and the scaling are launches on the current stream, and the
factor travels as a device tensor.  There is no CPU fallback: tensors are filtered and metered on a GPU.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib

KEYS = ("target", "max_gain_db", "peak_limit", "restore", "data")
OPTIONAL_KEYS = ("true_peak_limit",)     # in the checked copy only when the caller gave them
REPORT = ("integrated", "range", "max_momentary", "max_short_term", "true_peak", "sample_peak", "blocks_kept", "short_term_kept")
DEFAULTS = {"target": -23.0, "max_gain_db": 30.0, "peak_limit": None, "restore": True, "data": False}


def chunk():
    """Frames per chunk of the filter's parallel schedule (wun_sos_chunk)."""
    return int(_lib.load().wun_sos_chunk())


def tile():
    """Chunks per workgroup and per carry group (wun_sos_tile)."""
    return int(_lib.load().wun_sos_tile())


def kweight_sos(sr):
    """The K-weighting at sr Hz as float64 numpy [2, 6] in scipy's sos layout (wun_kweight_design)."""
    sos = (C.c_double * 12)()
    _lib.check(_lib.load().wun_kweight_design(int(sr), sos))
    return np.array(sos, dtype=np.float64).reshape(2, 6)


def blocks(n, sr):
    """Complete 0.4 s gating blocks of n frames at sr (wun_loudness_blocks)."""
    return _lib.count(_lib.load().wun_loudness_blocks(int(n), int(sr)))


_stream = _lib.stream


def _audio(x, who):
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError("%s runs its kernels on a GPU; there is no CPU fallback (got %s)" % (
            who, "a tensor on %s" % x.device if torch.is_tensor(x) else type(x).__name__))
    if x.dtype != torch.float32 or x.dim() != 2 or not x.is_contiguous():
        raise ValueError("%s: audio must be a contiguous float32 tensor [n, C], got %s %s" % (who, x.dtype, tuple(x.shape)))
    return int(x.shape[0]), int(x.shape[1])


def sosfilt(x, sos, out=None, scratch=None):
    """scipy.signal.sosfilt(sos, x, axis=0) from zero state for a float32 device tensor x [n, C]: float64 arithmetic, one rounding
    to float32 (wun_sosfilt).  sos: [nsec, 6] host floats, a0 == 1, nsec in 1..8."""
    n, Cc = _audio(x, "sosfilt")
    sos = np.ascontiguousarray(np.asarray(sos, dtype=np.float64))
    if sos.ndim != 2 or sos.shape[1] != 6:
        raise ValueError("sos must be [nsec, 6], got %s" % (sos.shape,))
    lib = _lib.load()
    nsec = int(sos.shape[0])
    dev = x.device
    if scratch is None:
        need = _lib.count(lib.wun_sosfilt_scratch_doubles(n, Cc, nsec))
        scratch = torch.empty(need, dtype=torch.float64, device=dev)
    y = torch.empty_like(x) if out is None else out
    with torch.cuda.device(dev):
        _lib.check(lib.wun_sosfilt(x.data_ptr(), n, Cc, sos.ctypes.data_as(C.POINTER(C.c_double)), nsec, y.data_ptr(),
                                   scratch.data_ptr(), _stream(dev)))
    return y


def k_weight(x, sr):
    """x through the K-weighting at sr Hz."""
    return sosfilt(x, kweight_sos(sr))


def scratch_doubles(n, Cc, sr):
    return _lib.count(_lib.load().wun_loudness_scratch_doubles(int(n), int(Cc), int(sr)))


def integrated(x, sr, return_blocks=False, scratch=None):
    """The meter of a float32 device tensor x [n, C] at sr Hz: a float64 device tensor [4] = integrated loudness in LUFS (-inf
    when no block passes the gates, NaN when x holds one), blocks kept, complete blocks, sample peak max |x| (wun_loudness).
    return_blocks: also the momentary loudness of every block, float64 [nb].  No host synchronisation."""
    n, Cc = _audio(x, "integrated")
    dev = x.device
    if scratch is None:
        scratch = torch.empty(scratch_doubles(n, Cc, sr), dtype=torch.float64, device=dev)
    meter = torch.empty(4, dtype=torch.float64, device=dev)
    blk = torch.empty(blocks(n, sr), dtype=torch.float64, device=dev) if return_blocks else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().wun_loudness(x.data_ptr(), n, Cc, int(sr), meter.data_ptr(),
                                            blk.data_ptr() if blk is not None and blk.numel() else None,
                                            scratch.data_ptr(), _stream(dev)))
    return (meter, blk) if return_blocks else meter


def oversampling(sr):
    """The true-peak oversampling factor at sr Hz: the smallest power of two L in 1..32 with L sr >= 176400
    (wun_true_peak_factor)."""
    return _lib.count(_lib.load().wun_true_peak_factor(int(sr)))


def short_term_blocks(n, sr):
    """Complete 3 s short-term blocks of n frames at sr, at the meter's 0.1 s step (wun_loudness_short_term_blocks)."""
    return _lib.count(_lib.load().wun_loudness_short_term_blocks(int(n), int(sr)))


def _peak_table(L, device):
    from . import resample as rs
    return rs._table(L, 1, device) if L > 1 else None


def true_peak(x, sr, scratch=None):
    """float64 device tensor [1 + C]: max |r| over all channels, then per channel, r being bit for bit the resampler's output
    for up = oversampling(sr), down = 1 -- computed without writing r (wun_true_peak).  NaN where x holds one.  This project's
    Kaiser interpolator, not the 48-tap table of BS.1770-4 Annex 2."""
    n, Cc = _audio(x, "true_peak")
    dev = x.device
    L = oversampling(sr)
    lib = _lib.load()
    if scratch is None:
        scratch = torch.empty(int(lib.wun_true_peak_scratch_doubles(n, Cc)), dtype=torch.float64, device=dev)
    tab = _peak_table(L, dev)
    out = torch.empty(1 + Cc, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.wun_true_peak(x.data_ptr(), n, Cc, L, tab.data_ptr() if tab is not None else None, out.data_ptr(),
                                     scratch.data_ptr(), _stream(dev)))
    return out


def r128_scratch_doubles(n, Cc, sr):
    return _lib.count(_lib.load().wun_loudness_r128_scratch_doubles(int(n), int(Cc), int(sr)))


def r128(x, sr, return_short_term=False, scratch=None):
    """The EBU R 128 readings of a float32 device tensor x [n, C] at sr Hz: a float64 device tensor [8] in the order of REPORT
    -- integrated loudness, loudness range (LU), largest momentary and short-term loudness, true peak, sample peak, gating
    blocks kept, short-term blocks kept (wun_loudness_r128; the first, sixth and seventh are integrated()'s bits).
    return_short_term: also the short-term loudness of every 3 s block, float64 [short_term_blocks(n, sr)].  No host
    synchronisation."""
    n, Cc = _audio(x, "r128")
    dev = x.device
    if scratch is None:
        scratch = torch.empty(r128_scratch_doubles(n, Cc, sr), dtype=torch.float64, device=dev)
    tab = _peak_table(oversampling(sr), dev)
    report = torch.empty(8, dtype=torch.float64, device=dev)
    st = torch.empty(short_term_blocks(n, sr), dtype=torch.float64, device=dev) if return_short_term else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().wun_loudness_r128(x.data_ptr(), n, Cc, int(sr), tab.data_ptr() if tab is not None else None,
                                                 report.data_ptr(), st.data_ptr() if st is not None and st.numel() else None,
                                                 scratch.data_ptr(), _stream(dev)))
    return (report, st) if return_short_term else report


def meter_from_r128(report, n, sr):
    """The [L, kept, nb, peak] tensor gain() reads, built on the device from r128()'s report with the TRUE peak in the peak
    slot: gain(.., peak_limit=p) then holds the true peak of the scaled signal under p.  No value reaches the host."""
    nb = torch.full((1,), float(blocks(n, sr)), dtype=torch.float64, device=report.device)
    return torch.cat([report[0:1], report[6:7], nb, report[4:5]])


def meter_for(x, sr, spec):
    """(meter, peak_limit) for gain() under a checked spec: integrated() and the sample-peak limit, or -- with true_peak_limit
    (dBTP) -- r128() with the true peak in the peak slot and the limit 10^(true_peak_limit / 20)."""
    if spec.get("true_peak_limit") is None:
        return integrated(x, sr), spec["peak_limit"]
    return meter_from_r128(r128(x, sr), int(x.shape[0]), sr), 10.0 ** (spec["true_peak_limit"] / 20.0)


def gain(meter, target=-23.0, max_gain_db=30.0, peak_limit=None):
    """float32 device tensor [2] = (g, 1 / g) from a meter of integrated(): g = 10^((target - L) / 20) capped at max_gain_db and,
    with peak_limit, at peak_limit / peak; exactly 1 when L is not finite (wun_loudness_gain)."""
    if not torch.is_tensor(meter) or not meter.is_cuda:
        raise RuntimeError("gain reads the meter on a GPU; there is no CPU fallback")
    if meter.dtype != torch.float64 or meter.numel() != 4 or not meter.is_contiguous():
        raise ValueError("meter must be the float64 [4] tensor of integrated()")
    dev = meter.device
    g = torch.empty(2, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().wun_loudness_gain(meter.data_ptr(), float(target), float(max_gain_db),
                                                 0.0 if peak_limit is None else float(peak_limit), g.data_ptr(), _stream(dev)))
    return g


def scale_(x, factor):
    """x *= factor[0] in place: x a contiguous float32 device tensor of any shape, factor a float32 device tensor (a view of
    gain()'s result: g[0:1] scales, g[1:2] restores).  One launch (wun_scale_by)."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError("scale_ runs on a GPU; there is no CPU fallback")
    if x.dtype != torch.float32 or not x.is_contiguous() or factor.dtype != torch.float32 or factor.device != x.device:
        raise ValueError("scale_: a contiguous float32 tensor and a float32 factor on its device expected")
    if x.numel():
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().wun_scale_by(x.data_ptr(), x.numel(), factor.data_ptr(), _stream(x.device)))
    return x


def normalize(x, sr, target=-23.0, max_gain_db=30.0, peak_limit=None, inplace=False, true_peak_limit=None):
    """(y, gain): x [n, C] scaled to `target` LUFS, and the float32 [2] factor pair of gain().  true_peak_limit (dBTP, instead
    of peak_limit): the ceiling is on the true peak."""
    if true_peak_limit is not None and peak_limit is not None:
        raise ValueError("normalize: peak_limit and true_peak_limit are exclusive")
    meter, limit = meter_for(x, sr, {"peak_limit": peak_limit, "true_peak_limit": true_peak_limit})
    g = gain(meter, target, max_gain_db, limit)
    y = x if inplace else x.clone()
    return scale_(y, g[0:1]), g


def from_config(spec):
    """model_config["loudness"] / separate_track's keyword checked and completed: None stays None; a number is the target; a
    dict may hold target, max_gain_db, peak_limit, restore, data and true_peak_limit (dBTP, a finite number such as -1.0: the
    ceiling is then on the true peak, metered by r128(); not together with peak_limit; the key appears in the result only when
    it was given).  ValueError for anything else."""
    if spec is None:
        return None
    if isinstance(spec, bool):
        raise ValueError("loudness = %r: a target in LUFS or a dict expected" % (spec,))
    if isinstance(spec, (int, float, np.integer, np.floating)):
        spec = {"target": float(spec)}
    if not isinstance(spec, dict):
        raise ValueError("loudness = %r: a target in LUFS or a dict expected" % (spec,))
    unknown = set(spec) - set(KEYS) - set(OPTIONAL_KEYS)
    if unknown:
        raise ValueError("loudness: unknown keys %s (have %s)" % (sorted(unknown), ", ".join(KEYS + OPTIONAL_KEYS)))
    out = dict(DEFAULTS, **spec)
    for k in ("target", "max_gain_db"):
        if isinstance(out[k], bool) or not isinstance(out[k], (int, float, np.integer, np.floating)) or not math.isfinite(out[k]):
            raise ValueError("loudness[%r] = %r must be a finite number" % (k, out[k]))
        out[k] = float(out[k])
    if out["max_gain_db"] < 0:
        raise ValueError("loudness['max_gain_db'] = %r must be >= 0" % out["max_gain_db"])
    pl = out["peak_limit"]
    if pl is not None:
        if isinstance(pl, bool) or not isinstance(pl, (int, float, np.integer, np.floating)) or not math.isfinite(pl) or pl <= 0:
            raise ValueError("loudness['peak_limit'] = %r must be a number > 0 or None" % (pl,))
        out["peak_limit"] = float(pl)
    if "true_peak_limit" in out:
        tp = out["true_peak_limit"]
        if isinstance(tp, bool) or not isinstance(tp, (int, float, np.integer, np.floating)) or not math.isfinite(tp):
            raise ValueError("loudness['true_peak_limit'] = %r must be a finite number of dBTP" % (tp,))
        if pl is not None:
            raise ValueError("loudness: peak_limit and true_peak_limit are exclusive (one ceiling, on the sample or the true peak)")
        out["true_peak_limit"] = float(tp)
    for k in ("restore", "data"):
        if not isinstance(out[k], (bool, np.bool_)):
            raise ValueError("loudness[%r] = %r must be a bool" % (k, out[k]))
        out[k] = bool(out[k])
    return out
