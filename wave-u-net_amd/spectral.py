"""The spectral training loss of libwun.so (include/wun.h: wun_stft_*, wun_spectral_*): the L1 distance
between STFT magnitudes the reference builds from tf.contrib.signal.stft (Training.py:55-60 -- frame 1024, hop 768, periodic
Hann window, no padding), for any number of resolutions up to 8, next to the time-domain MSE.

    stft_magnitude(x, 1024, 768)                       # the magnitude spectrogram [S, B, C, F, K] of audio [S, B, T, C]
    loss = SpectralLoss([(1024, 768), (256, 64)], mse_weight=1.0)
    losses, d_outputs = loss.loss_and_grad(outputs, targets)      # [total, MSE, L_0, L_1], dL / d outputs
    sep.loss_and_gradients(targets, loss=loss)         # the training step's loss (UnetAudioSeparator, Trainer)
    stft_l1(net(mix), targets, loss)                   # under torch.autograd, for users of sep.module()
    loss = SpectralLoss.multi_resolution()             # spectral convergence + log-magnitude L1 at three resolutions (5.14)
    loss = SpectralLoss([(1024, 256)], terms={"mag_l1": 1, "log_mag_l1": 1, "sc": 1, "complex_l1": 0.5})
    loss.term_losses(losses)["sc"]                     # the unweighted term of every resolution, a view of `losses`
    re, im = stft(x, 2048, 512, centered=True)         # the complex STFT [S, B, C, F, K]
    x2 = istft(re, im, x.shape[2], 2048, 512, centered=True)      # and its inverse: x again, to fp32 rounding
    re, im = stft(x, 4096, 1024, centered=True, transform="fft")  # the same definitions through an FFT, n_fft up to 8192 (5.13)
    loss = SpectralLoss([(4096, 1024)], terms={"sc": 1, "log_mag_l1": 1}, log_eps=4.0, transform="fft")    # the loss too (5.16)
    loss = SpectralLoss.multi_resolution(transform="fft")         # the same three resolutions, both frame transforms as FFTs
    loss = SpectralLoss.multi_scale_mel(22050)                    # mel L1 + log-mel L1 at 512 / 1024 / 2048, 40 / 80 / 160 bands (5.19)
    loss = SpectralLoss([(1024, 256)], terms={"sc": 1}, mel={"n_mels": 80, "sample_rate": 22050, "terms": {"log_mel_l1": 1}})
    mel_spectrogram(x, 1024, 256, 80, 22050)                      # [S, B, C, F, n_mels], the floats the mel terms are taken on
    mel_filterbank(1024, 22050, 80)                               # the dense [n_mels, K] weights, rebuilt from the library's table
    y = griffin_lim(mag, 2048, 512, iterations=32, momentum=0.99) # audio [..., T] from magnitudes [..., F, K] (5.21)

Audio is float32 [S, B, T, C] channel-last on the GPU, as get_output stacks its outputs.  There is no CPU path, except for
griffin_lim, whose definition also runs in plain torch on CPU tensors (the tests' stand-in, as postfilter.py's).
"""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib

MAX_RESOLUTIONS = 8
TERMS = ("mag_l1", "log_mag_l1", "sc", "complex_l1")       # the order of the term slots of wun_spectral_loss_terms' losses
MEL_TERMS = ("mel_l1", "log_mel_l1")                         # the order of the mel slots behind them (wun_spectral_loss_mel)
MAX_MELS = 512
TRANSFORMS = ("gemm", "fft")
# (transform, operation) -> the library's entry.  "table": wun_*_table_floats, wun_*_design and the table's leading dimension.
_ENTRIES = {
    "gemm": {"table": ("wun_stft_table_floats", "wun_stft_design", 2), "frames": "wun_stft_frames",
             "centered_frames": "wun_stft_centered_frames", "stft": "wun_stft_complex", "istft": "wun_istft",
             "istft_scratch": "wun_istft_scratch_floats", "istft_tf": "wun_istft_tf",
             "istft_tf_scratch": "wun_istft_tf_scratch_floats", "mask_filter": "wun_mask_filter",
             "mask_filter_scratch": "wun_mask_filter_scratch_floats", "wiener_filter": "wun_wiener_filter",
             "wiener_filter_scratch": "wun_wiener_filter_scratch_floats", "magnitude": "wun_stft_magnitude",
             "loss": "wun_spectral_loss", "loss_scratch": "wun_spectral_scratch_floats", "loss_terms": "wun_spectral_loss_terms",
             "loss_terms_scratch": "wun_spectral_terms_scratch_floats", "loss_mel": "wun_spectral_loss_mel",
             "loss_mel_scratch": "wun_spectral_mel_scratch_floats"},
    "fft": {"table": ("wun_fft_table_floats", "wun_fft_design", 3), "frames": "wun_fft_frames",
            "centered_frames": "wun_fft_centered_frames", "stft": "wun_stft_complex_fft", "istft": "wun_istft_fft",
            "istft_scratch": "wun_istft_fft_scratch_floats", "istft_tf": "wun_istft_tf_fft",
            "istft_tf_scratch": "wun_istft_tf_fft_scratch_floats", "mask_filter": "wun_mask_filter_fft",
            "mask_filter_scratch": "wun_mask_filter_fft_scratch_floats", "wiener_filter": "wun_wiener_filter_fft",
            "wiener_filter_scratch": "wun_wiener_filter_fft_scratch_floats", "magnitude": "wun_stft_magnitude_fft",
            "loss": "wun_spectral_loss_fft", "loss_scratch": "wun_spectral_fft_scratch_floats",
            "loss_terms": "wun_spectral_loss_terms_fft", "loss_terms_scratch": "wun_spectral_terms_fft_scratch_floats",
            "loss_mel": "wun_spectral_loss_mel_fft", "loss_mel_scratch": "wun_spectral_mel_fft_scratch_floats"},
}
_TABLES = _lib._DEVICE_TABLES     # the shared cache: (transform, n_fft, device) -> device tensor holding the transform's table
_MEL_NORMS = {None: 0, "none": 0, 0: 0, "area": 1, 1: 1}


def entry(transform, op):
    """(the library's entry of operation `op` on `transform`, the function (n_fft, device) -> that transform's device table)."""
    if transform not in _ENTRIES:
        raise ValueError("transform must be one of %s, got %r" % (", ".join(TRANSFORMS), transform))
    return getattr(_lib.load(), _ENTRIES[transform][op]), (_fft_table if transform == "fft" else _table)


def _design(transform, n_fft):
    floats, fill, lead = _ENTRIES[transform]["table"]
    lib = _lib.load()
    n = _lib.count(getattr(lib, floats)(int(n_fft)))
    table = np.zeros(n, np.float32)
    _lib.check(getattr(lib, fill)(int(n_fft), table.ctypes.data_as(C.POINTER(C.c_float)), n))
    return table.reshape(lead, int(n_fft), -1) if transform == "gemm" else table.reshape(lead, int(n_fft))


def _device_table(transform, n_fft, device):
    return _lib.device_table((transform, int(n_fft)), device, lambda: _design(transform, n_fft))


def design(n_fft):
    """The fp32 table [2, n_fft, K] as a numpy array: w[n] cos and -w[n] sin of 2 pi n k / n_fft (wun_stft_design)."""
    return _design("gemm", n_fft)


def fft_design(n_fft):
    """The FFT path's fp32 table [3, n_fft] as a numpy array: cos and -sin of 2 pi t / n_fft, then the periodic Hann window
    (wun_fft_design); n_fft a power of two in 64..8192."""
    return _design("fft", n_fft)


def _table(n_fft, device):
    return _device_table("gemm", n_fft, device)


def _fft_table(n_fft, device):
    return _device_table("fft", n_fft, device)


def count(transform, op, *args):
    """A frame or float count of the library; its negative values are error codes."""
    return _lib.count(entry(transform, op)[0](*args))


def frames(n, n_fft, hop, transform="gemm"):
    """Frames of n samples: 1 + (n - n_fft) // hop, no padding (wun_stft_frames; with transform="fft" wun_fft_frames, n_fft up
    to 8192)."""
    return count(transform, "frames", int(n), int(n_fft), int(hop))


def _audio(x, what):
    if not torch.is_tensor(x) or not x.is_cuda:
        raise ValueError("%s must be a tensor on the GPU (there is no CPU path)" % what)
    if x.dim() != 4:
        raise ValueError("%s must be [S, B, T, C], got %s" % (what, tuple(x.shape)))
    return x.to(torch.float32).contiguous()


def stft_magnitude(x, n_fft, hop, transform="gemm"):
    """|STFT| of audio x [S, B, T, C]: float32 [S, B, C, F, K], K = n_fft // 2 + 1 bins, F = frames(T, n_fft, hop) frames of
    the periodic-Hann-windowed signal without padding (wun_stft_magnitude; transform="fft": wun_stft_magnitude_fft, n_fft up
    to 8192).  The floats a SpectralLoss of the same transform takes its signs from.  One launch on the current stream, no sync."""
    fn, table = entry(transform, "magnitude")
    x = _audio(x, "x")
    S, B, T, Cn = (int(v) for v in x.shape)
    F = frames(T, n_fft, hop, transform)
    mags = torch.empty((S, B, Cn, F, int(n_fft) // 2 + 1), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(fn(x.data_ptr(), S, B, T, Cn, int(n_fft), int(hop), table(n_fft, x.device).data_ptr(), mags.data_ptr(),
                      _lib.stream(x.device)))
    return mags


def _mel_key(n_fft, sample_rate, n_mels, fmin, fmax, norm):
    if norm not in _MEL_NORMS:
        raise ValueError("norm must be None or 'area', got %r" % (norm,))
    return int(n_fft), float(sample_rate), int(n_mels), float(fmin), 0.0 if fmax is None else float(fmax), _MEL_NORMS[norm]


def mel_design(n_fft, sample_rate, n_mels, fmin=0.0, fmax=None, norm=None):
    """The mel table's 3 K + 2 n_mels words as an int32 numpy array (wun_mel_design, include/wun.h): b0[K], the bits of the
    float32 w0[K] and w1[K], lo[n_mels], hi[n_mels].  ValueError for what the library refuses -- an empty band among it."""
    key = _mel_key(n_fft, sample_rate, n_mels, fmin, fmax, norm)
    lib = _lib.load()
    n = _lib.count(lib.wun_mel_table_floats(key[0], key[2]))
    table = np.zeros(n, np.float32)
    _lib.check(lib.wun_mel_design(key[0], key[1], key[2], key[3], key[4], key[5], table.ctypes.data_as(C.POINTER(C.c_float)), n))
    return table.view(np.int32)


def mel_table_parts(words, n_fft, n_mels):
    """(b0, w0, w1, lo, hi) views of mel_design's words."""
    K = int(n_fft) // 2 + 1
    return (words[:K], words[K:2 * K].view(np.float32), words[2 * K:3 * K].view(np.float32), words[3 * K:3 * K + n_mels],
            words[3 * K + n_mels:3 * K + 2 * n_mels])


def mel_filterbank(n_fft, sample_rate, n_mels, fmin=0.0, fmax=None, norm=None):
    """The float32 weights W [n_mels, K] of the HTK-scale triangular filterbank (include/wun.h), rebuilt from the library's
    table: fmax=None is sample_rate / 2, norm=None or "area"."""
    b0, w0, w1, _, _ = mel_table_parts(mel_design(n_fft, sample_rate, n_mels, fmin, fmax, norm), n_fft, n_mels)
    W = np.zeros((int(n_mels), b0.size), np.float32)
    k = np.arange(b0.size)
    for b, w in ((b0, w0), (b0 + 1, w1)):
        ok = (w > 0) & (b >= 0) & (b < int(n_mels))
        W[b[ok], k[ok]] = w[ok]
    return W


def _mel_table(n_fft, sample_rate, n_mels, fmin, fmax, norm, device):
    key = ("mel",) + _mel_key(n_fft, sample_rate, n_mels, fmin, fmax, norm)
    return _lib.device_table(key, device, lambda: mel_design(n_fft, sample_rate, n_mels, fmin, fmax, norm))


def mel_spectrogram(x, n_fft, hop, n_mels, sample_rate, fmin=0.0, fmax=None, norm=None, transform="gemm"):
    """The mel magnitudes of audio x [S, B, T, C]: float32 [S, B, C, F, n_mels], stft_magnitude's floats projected onto the
    filterbank (wun_op_mel_project: one ascending fmaf chain per band).  The floats the mel terms of a SpectralLoss with the
    same arguments are taken on.  No sync."""
    table = _mel_table(n_fft, sample_rate, n_mels, fmin, fmax, norm, x.device)       # (refusals before any launch)
    mags = stft_magnitude(x, n_fft, hop, transform)
    out = torch.empty(mags.shape[:4] + (int(n_mels),), dtype=torch.float32, device=mags.device)
    with torch.cuda.device(mags.device):
        _lib.check(_lib.load().wun_op_mel_project(mags.data_ptr(), mags.numel() // mags.shape[4], int(mags.shape[4]), int(n_mels),
                                                  table.data_ptr(), out.data_ptr(), _lib.stream(mags.device)))
    return out


def centered_frames(n, n_fft, hop, transform="gemm"):
    """Frames of n samples in the centred framing: ceil((n + n_fft - hop) / hop) (wun_stft_centered_frames; with
    transform="fft" wun_fft_centered_frames, n_fft up to 8192)."""
    return count(transform, "centered_frames", int(n), int(n_fft), int(hop))


def _framing(T, n_fft, hop, centered, transform="gemm"):
    """(lead, F): centered: lead = n_fft - hop samples of zeros before the track, frames until the track is covered;
    else the framing of the loss, lead = 0 and frames(T, n_fft, hop) whole frames."""
    if centered:
        return int(n_fft) - int(hop), centered_frames(T, n_fft, hop, transform)
    return 0, frames(T, n_fft, hop, transform)


def stft(x, n_fft, hop, centered=False, transform="gemm"):
    """(re, im) of audio x [S, B, T, C]: float32 [S, B, C, F, K] each (wun_stft_complex).  centered=False: the loss's
    framing (no padding, T >= n_fft); centered=True: frame f starts at f hop - (n_fft - hop), zeros outside the track,
    F = centered_frames(T, n_fft, hop), any T >= 1.  transform="gemm" (n_fft up to 2048) or "fft" (wun_stft_complex_fft, up to
    8192): one definition, two summation orders.  One launch on the current stream, no sync."""
    fn, table = entry(transform, "stft")
    x = _audio(x, "x")
    S, B, T, Cn = (int(v) for v in x.shape)
    lead, F = _framing(T, n_fft, hop, centered, transform)
    re = torch.empty((S, B, Cn, F, int(n_fft) // 2 + 1), dtype=torch.float32, device=x.device)
    im = torch.empty_like(re)
    with torch.cuda.device(x.device):
        _lib.check(fn(x.data_ptr(), S, B, T, Cn, int(n_fft), int(hop), lead, F, table(n_fft, x.device).data_ptr(), re.data_ptr(),
                      im.data_ptr(), _lib.stream(x.device)))
    return re, im


def istft(re, im, length, n_fft, hop, centered=False, transform="gemm"):
    """Audio [S, B, length, C] from re, im [S, B, C, F, K] (wun_istft): the windowed overlap-add of the inverse transforms
    of the frames over the overlap-add of the squared window, 0 where that is below 1e-8.  F must be the frame count of
    `length` in the chosen framing.  transform="fft": wun_istft_fft, n_fft up to 8192.  No sync; not differentiable."""
    fn, table = entry(transform, "istft")
    if not (torch.is_tensor(re) and torch.is_tensor(im) and re.is_cuda and im.is_cuda):
        raise ValueError("re and im must be tensors on the GPU (there is no CPU path)")
    if re.dim() != 5 or re.shape != im.shape or re.device != im.device:
        raise ValueError("re and im must be [S, B, C, F, K] of one shape and device, got %s and %s" % (tuple(re.shape), tuple(im.shape)))
    re, im = re.to(torch.float32).contiguous(), im.to(torch.float32).contiguous()
    S, B, Cn, F, K = (int(v) for v in re.shape)
    lead, want = _framing(int(length), n_fft, hop, centered, transform)
    if F != want or K != int(n_fft) // 2 + 1:
        raise ValueError("spectra of %d frames x %d bins, expected %d x %d for length %d" % (F, K, want, int(n_fft) // 2 + 1, length))
    n = count(transform, "istft_scratch", S, B, int(length), Cn, int(n_fft), int(hop), lead, F)
    scratch = torch.empty(n, dtype=torch.float32, device=re.device)
    y = torch.empty((S, B, int(length), Cn), dtype=torch.float32, device=re.device)
    with torch.cuda.device(re.device):
        _lib.check(fn(re.data_ptr(), im.data_ptr(), S, B, int(length), Cn, int(n_fft), int(hop), lead, F,
                      table(n_fft, re.device).data_ptr(), y.data_ptr(), scratch.data_ptr(), _lib.stream(re.device)))
    return y


def istft_tf(re, im, n_fft, hop, transform="gemm"):
    """Audio [S, B, (F - 1) hop + n_fft, C] from re, im [S, B, C, F, K] in the loss's framing, as
    tf.contrib.signal.inverse_stft with inverse_stft_window_fn(hop) gives it (wun_istft_tf): istft's frames over the steady-state
    window-square sum D[t mod hop], at the track's edges too.  NotImplementedError where some D is below 1e-8.
    transform="fft": wun_istft_tf_fft, n_fft up to 8192.  No sync."""
    if not (torch.is_tensor(re) and torch.is_tensor(im) and re.is_cuda and im.is_cuda):
        raise ValueError("re and im must be tensors on the GPU (there is no CPU path)")
    if re.dim() != 5 or re.shape != im.shape or re.device != im.device or int(re.shape[4]) != int(n_fft) // 2 + 1:
        raise ValueError("re and im must be [S, B, C, F, n_fft / 2 + 1] of one shape and device, got %s and %s" % (
            tuple(re.shape), tuple(im.shape)))
    re, im = re.to(torch.float32).contiguous(), im.to(torch.float32).contiguous()
    S, B, Cn, F, _ = (int(v) for v in re.shape)
    T = (F - 1) * int(hop) + int(n_fft)
    fn, table = entry(transform, "istft_tf")
    n = count(transform, "istft_tf_scratch", S, B, T, Cn, int(n_fft), int(hop), F)
    scratch = torch.empty(n, dtype=torch.float32, device=re.device)
    y = torch.empty((S, B, T, Cn), dtype=torch.float32, device=re.device)
    with torch.cuda.device(re.device):
        _lib.check(fn(re.data_ptr(), im.data_ptr(), S, B, T, Cn, int(n_fft), int(hop), F,
                      table(n_fft, re.device).data_ptr(), y.data_ptr(), scratch.data_ptr(), _lib.stream(re.device)))
    return y


class SpectralLoss(object):
    """L = mse_weight * MSE + sum_j weights[j] * L_j at resolutions[j] = (n_fft, hop).  weights=None: 1 for every resolution.
    resolutions=[] is the MSE alone.  ValueError / NotImplementedError for what the library's entry refuses, at the first call
    (the checks need the audio's length).

    terms=None: L_j = mean |M_est - M_tgt| (wun_spectral_loss; losses [2 + nres]).
    terms={name: weight}: L_j = sum_t weight_t * term_t(j) over TERMS (wun_spectral_loss_terms, include/wun.h; a missing name
    is weight 0 and is not computed): "mag_l1" the term above, "log_mag_l1" mean |log(M_est + log_eps) - log(M_tgt + log_eps)|,
    "sc" the spectral convergence sqrt(sum d^2 / (sum M_tgt^2 + sc_eps)) per source, averaged over the sources, "complex_l1"
    mean |STFT_est - STFT_tgt|.  losses is then [2 + 5 nres]: [total, MSE, L_0 .., then mag_l1, log_mag_l1, sc, complex_l1 of
    resolution 0, of resolution 1, ..] (term_losses).  log_eps and sc_eps are choices, not measurements: 1e-3 sits above the
    fp32 transform's error on unit-scale audio at short frames (raise it with n_fft), 1.0 keeps a silent source finite.

    mel=None: nothing below.  mel={"n_mels": int or one per resolution, "sample_rate": Hz, "fmin": 0, "fmax": None, "norm": None,
    "terms": {name: weight} over MEL_TERMS (default both 1), "log_eps": 1e-3}: L_j gains weight * "mel_l1", the mean |Pe - Pt|
    of the mel magnitudes (mel_spectrogram's floats), and weight * "log_mel_l1", the mean |log(Pe + log_eps) - log(Pt + log_eps)|
    (wun_spectral_loss_mel).  losses is then [2 + 7 nres]: the 2 + 5 nres slots above, then mel_l1, log_mel_l1 of
    resolution 0, of resolution 1, ..; with terms=None no linear-frequency term is computed.  The mel log_eps of 1e-3 is a
    choice, not a measurement.  A filterbank with a band that weights no bin is refused (ValueError) at construction.

    transform="gemm": both frame transforms of a resolution as GEMMs against an n_fft^2 table, n_fft up to 2048.  "fft": as
    FFTs (the *_fft entries), n_fft up to 8192 -- the same definitions, slots and summation order, results
    equal to float32 rounding.  ValueError for any other name."""

    def __init__(self, resolutions=((1024, 768),), weights=None, mse_weight=0.0, terms=None, log_eps=1e-3, sc_eps=1.0,
                 transform="gemm", mel=None):
        if transform not in _ENTRIES:
            raise ValueError("transform must be one of %s, got %r" % (", ".join(TRANSFORMS), transform))
        self.transform = transform
        self.resolutions = [(int(n), int(h)) for n, h in resolutions]
        if len(self.resolutions) > MAX_RESOLUTIONS:
            raise ValueError("at most %d resolutions, got %d" % (MAX_RESOLUTIONS, len(self.resolutions)))
        self.weights = [1.0] * len(self.resolutions) if weights is None else [float(w) for w in weights]
        if len(self.weights) != len(self.resolutions):
            raise ValueError("%d weights for %d resolutions" % (len(self.weights), len(self.resolutions)))
        self.mse_weight = float(mse_weight)
        for w in self.weights + [self.mse_weight]:
            if not (w >= 0.0 and np.isfinite(w)):
                raise ValueError("weights must be finite and >= 0, got %r" % (w,))
        self.terms, self.log_eps, self.sc_eps = None, float(log_eps), float(sc_eps)
        self._terms = None       # the entry's wun_spectral_terms (None: wun_spectral_loss)
        self.mel = self._mel = None      # the mel arguments as given (defaults filled in); the entry's wun_mel_terms
        if mel is not None:
            self._init_mel(mel)
            terms = {} if terms is None else terms       # no linear-frequency term unless asked for
        if terms is not None:
            unknown = set(terms) - set(TERMS)
            if unknown:
                raise ValueError("terms: unknown names %s (known: %s)" % (sorted(unknown), ", ".join(TERMS)))
            self.terms = {t: float(terms.get(t, 0.0)) for t in TERMS}
            for w in self.terms.values():
                if not (w >= 0.0 and np.isfinite(w)):
                    raise ValueError("term weights must be finite and >= 0, got %r" % (w,))
            for name, eps in (("log_eps", self.log_eps), ("sc_eps", self.sc_eps)):
                if not (eps > 0.0 and np.isfinite(eps)):
                    raise ValueError("%s must be finite and > 0, got %r" % (name, eps))
            self._terms = _lib.WunSpectralTerms(*([self.terms[t] for t in TERMS] + [self.log_eps, self.sc_eps]))
        n = max(len(self.resolutions), 1)
        self._n_fft = (C.c_int32 * n)(*[r[0] for r in self.resolutions])
        self._hop = (C.c_int32 * n)(*[r[1] for r in self.resolutions])
        self._w = (C.c_float * n)(*self.weights)
        self._scratch = {}       # (shape, device) -> float32 scratch of the entry's *_scratch_floats

    def _init_mel(self, mel):
        known = {"n_mels", "sample_rate", "fmin", "fmax", "norm", "terms", "log_eps"}
        unknown = set(mel) - known
        if unknown:
            raise ValueError("mel: unknown keys %s (known: %s)" % (sorted(unknown), ", ".join(sorted(known))))
        for need in ("n_mels", "sample_rate"):
            if need not in mel:
                raise ValueError("mel: `%s` is required" % need)
        nres = len(self.resolutions)
        n_mels = mel["n_mels"]
        n_mels = [int(n_mels)] * nres if np.isscalar(n_mels) else [int(n) for n in n_mels]
        if len(n_mels) != nres:
            raise ValueError("mel: %d band counts for %d resolutions" % (len(n_mels), nres))
        mterms = mel.get("terms")
        mterms = {t: 1.0 for t in MEL_TERMS} if mterms is None else mterms
        unknown = set(mterms) - set(MEL_TERMS)
        if unknown:
            raise ValueError("mel terms: unknown names %s (known: %s)" % (sorted(unknown), ", ".join(MEL_TERMS)))
        mterms = {t: float(mterms.get(t, 0.0)) for t in MEL_TERMS}
        for w in mterms.values():
            if not (w >= 0.0 and np.isfinite(w)):
                raise ValueError("mel term weights must be finite and >= 0, got %r" % (w,))
        eps = float(mel.get("log_eps", 1e-3))
        if not (eps > 0.0 and np.isfinite(eps)):
            raise ValueError("mel log_eps must be finite and > 0, got %r" % (eps,))
        self.mel = {"n_mels": n_mels, "sample_rate": float(mel["sample_rate"]), "fmin": float(mel.get("fmin", 0.0) or 0.0),
                    "fmax": mel.get("fmax"), "norm": mel.get("norm"), "terms": mterms, "log_eps": eps}
        for (n_fft, _), n in zip(self.resolutions, n_mels):      # the library's refusals now, not at the first step
            mel_design(n_fft, self.mel["sample_rate"], n, self.mel["fmin"], self.mel["fmax"], self.mel["norm"])
        self._mel = _lib.WunMelTerms(mterms["mel_l1"], mterms["log_mel_l1"], eps)
        self._n_mels = (C.c_int32 * max(nres, 1))(*n_mels)

    def _mel_tables(self, device):
        m = self.mel
        return [_mel_table(n_fft, m["sample_rate"], n, m["fmin"], m["fmax"], m["norm"], device)
                for (n_fft, _), n in zip(self.resolutions, m["n_mels"])]

    @classmethod
    def from_config(cls, spec):
        """model_config["spectral_loss"]: None, a SpectralLoss, or a dict with `resolutions`, `weights`, `mse_weight`, `terms`,
        `log_eps`, `sc_eps`, `transform`, `mel` (the dict of the `mel` argument)."""
        if spec is None or isinstance(spec, cls):
            return spec
        unknown = set(spec) - {"resolutions", "weights", "mse_weight", "terms", "log_eps", "sc_eps", "transform", "mel"}
        if unknown:
            raise ValueError("spectral_loss: unknown keys %s" % sorted(unknown))
        return cls(spec.get("resolutions", ((1024, 768),)), spec.get("weights"), spec.get("mse_weight", 0.0), spec.get("terms"),
                   spec.get("log_eps", 1e-3), spec.get("sc_eps", 1.0), spec.get("transform", "gemm"), spec.get("mel"))

    @classmethod
    def multi_scale_mel(cls, sample_rate, transform="gemm"):
        """The usual multi-scale mel loss: mel L1 + log-mel L1 at windows 512 / 1024 / 2048, hop a quarter of each, 40 / 80 / 160
        bands from 0 to sample_rate / 2 -- every band weights a bin at 22 050 Hz; ValueError at a rate where one does not."""
        return cls([(512, 128), (1024, 256), (2048, 512)], transform=transform,
                   mel={"n_mels": [40, 80, 160], "sample_rate": sample_rate, "terms": {t: 1.0 for t in MEL_TERMS}})

    @classmethod
    def multi_resolution(cls, transform="gemm", resolutions=None):
        """The usual multi-resolution STFT loss: spectral convergence + log-magnitude L1 at 512 / 128, 1024 / 256, 2048 / 512
        (or at `resolutions`; transform="fft" admits n_fft up to 8192)."""
        if resolutions is None:
            resolutions = [(512, 128), (1024, 256), (2048, 512)]
        return cls(resolutions, terms={"sc": 1.0, "log_mag_l1": 1.0}, transform=transform)

    @property
    def num_losses(self):
        """Floats of `losses`: 2 + nres, with terms 2 + 5 nres, with mel 2 + 7 nres."""
        return 2 + (7 if self._mel is not None else 1 if self._terms is None else 5) * len(self.resolutions)

    def term_weight(self, name):
        """The weight of a term of term_losses."""
        return self.mel["terms"][name] if name in MEL_TERMS else self.terms[name]

    def term_losses(self, losses):
        """{name: [nres] view of `losses`}: the unweighted terms per resolution (terms= or mel= only; with mel= the two mel
        terms too)."""
        if self._terms is None:
            raise ValueError("term_losses needs a SpectralLoss built with terms=")
        nres = len(self.resolutions)
        per = losses[2 + nres:2 + 5 * nres].view(nres, 4)
        out = {t: per[:, i] for i, t in enumerate(TERMS)}
        if self._mel is not None:
            mper = losses[2 + 5 * nres:2 + 7 * nres].view(nres, 2)
            out.update({t: mper[:, i] for i, t in enumerate(MEL_TERMS)})
        return out

    def scratch_floats(self, shape):
        S, B, T, Cn = (int(v) for v in shape)
        args = (S, B, T, Cn, len(self.resolutions), self._n_fft, self._hop)
        if self._terms is None:
            return count(self.transform, "loss_scratch", *args)
        if self._mel is None:
            return count(self.transform, "loss_terms_scratch", *(args + (C.byref(self._terms),)))
        return count(self.transform, "loss_mel_scratch", *(args + (C.byref(self._terms), C.byref(self._mel), self._n_mels)))

    def _scratch_for(self, x):
        key = (tuple(x.shape), str(x.device))
        if key not in self._scratch:
            self._scratch[key] = torch.empty(self.scratch_floats(x.shape), dtype=torch.float32, device=x.device)
        return self._scratch[key]

    def run(self, outputs, targets, d_outputs, losses, scratch):
        """wun_spectral_loss (with terms: wun_spectral_loss_terms, with mel: wun_spectral_loss_mel; transform="fft": their _fft
        twins) on the caller's buffers
        (contiguous float32 device tensors; losses of num_losses floats; d_outputs may be None)."""
        S, B, T, Cn = (int(v) for v in outputs.shape)
        dev = outputs.device
        nres = len(self.resolutions)
        fn, table = entry(self.transform, "loss" if self._terms is None else "loss_terms" if self._mel is None else "loss_mel")
        tabs = (C.c_void_p * max(nres, 1))(*[table(n, dev).data_ptr() for n, _ in self.resolutions])
        head = (outputs.data_ptr(), targets.data_ptr(), S, B, T, Cn, self.mse_weight, nres, self._n_fft, self._hop, self._w)
        tail = (tabs, d_outputs.data_ptr() if d_outputs is not None else None, losses.data_ptr(), scratch.data_ptr(), _lib.stream(dev))
        with torch.cuda.device(dev):
            if self._terms is None:
                _lib.check(fn(*(head + tail)))
            elif self._mel is None:
                _lib.check(fn(*(head + (C.byref(self._terms),) + tail)))
            else:
                mtabs = self._mel_tables(dev)
                mptr = (C.c_void_p * max(nres, 1))(*[t.data_ptr() for t in mtabs])
                _lib.check(fn(*(head + (C.byref(self._terms),) + tail + (C.byref(self._mel), self._n_mels, mptr))))

    def loss_and_grad(self, outputs, targets, grad=True):
        """(losses, d_outputs): losses float32 [num_losses] on the device = [total, MSE, L_0, ...] (L_j unweighted; with terms
        the per-term slots follow, term_losses), d_outputs = d total / d outputs with the outputs' shape (None with grad=False).
        No host sync."""
        outputs, targets = _audio(outputs, "outputs"), _audio(targets, "targets")
        if outputs.shape != targets.shape or outputs.device != targets.device:
            raise ValueError("outputs %s and targets %s differ in shape or device" % (tuple(outputs.shape), tuple(targets.shape)))
        scratch = self._scratch_for(outputs)
        losses = torch.empty(self.num_losses, dtype=torch.float32, device=outputs.device)
        d_outputs = torch.empty_like(outputs) if grad else None
        self.run(outputs, targets, d_outputs, losses, scratch)
        return losses, d_outputs

    def __call__(self, outputs, targets):
        """The total loss as a 0-dim tensor, differentiable with respect to `outputs` (stft_l1)."""
        return stft_l1(outputs, targets, self)


class _StftL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, outputs, targets, loss):
        losses, d_outputs = loss.loss_and_grad(outputs.detach(), targets.detach(), grad=ctx.needs_input_grad[0])
        if d_outputs is not None:
            ctx.save_for_backward(d_outputs)
        ctx.dtype = outputs.dtype
        return losses[0].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        (d_outputs,) = ctx.saved_tensors
        return (d_outputs * g).to(ctx.dtype), None, None       # (the targets carry no gradient)


def stft_l1(outputs, targets, loss=None, resolutions=((1024, 768),), weights=None, mse_weight=0.0, transform="gemm"):
    """The total of a SpectralLoss (`loss`, or one built from the other arguments) as a 0-dim tensor under torch.autograd:
    backward gives d total / d outputs as wun_spectral_loss computes it; the targets get no gradient."""
    if loss is None:
        loss = SpectralLoss(resolutions, weights, mse_weight, transform=transform)
    return _StftL1.apply(outputs, targets, loss)


# ---------------------------------------------------------------------------------------------------- Griffin-Lim
def _gl_window(n_fft, dtype, device):
    n = torch.arange(int(n_fft), dtype=torch.float64, device=device)
    return (0.5 - 0.5 * torch.cos(2.0 * np.pi * n / int(n_fft))).to(dtype)


def _gl_window_sums(T, n_fft, hop, lead, F, device):
    """float64 [T]: the sum of w^2 over the frames that cover each sample."""
    w2 = _gl_window(n_fft, torch.float64, device) ** 2
    total = max((F - 1) * hop + n_fft, lead + T)
    cols = w2[None, :, None].expand(1, n_fft, F)
    ws = torch.nn.functional.fold(cols, (1, (F - 1) * hop + n_fft), (1, n_fft), stride=(1, hop)).reshape(-1)
    ws = torch.nn.functional.pad(ws, (0, total - ws.numel()))
    return ws[lead:lead + T]


def _gl_stft(y, n_fft, hop, lead, F, w):
    """complex [R, F, K] of y [R, T]: zeros outside [0, T), Im of the bins 0 and n_fft / 2 exactly 0."""
    total = (F - 1) * hop + n_fft
    keep = min(int(y.shape[1]), total - lead)
    pad = torch.zeros((y.shape[0], total), dtype=y.dtype, device=y.device)
    pad[:, lead:lead + keep] = y[:, :keep]
    c = torch.fft.rfft(pad.unfold(1, n_fft, hop)[:, :F] * w, dim=-1)
    c.imag[..., 0] = 0
    c.imag[..., -1] = 0
    return c


def _gl_istft(spec, T, n_fft, hop, lead, w, ws):
    """[R, T] of complex [R, F, K]: the windowed inverse frames overlap-added over the window-square sums, the 1e-8 rule."""
    spec = spec.clone()
    spec.imag[..., 0] = 0
    spec.imag[..., -1] = 0
    R, F = int(spec.shape[0]), int(spec.shape[1])
    fr = torch.fft.irfft(spec, n=n_fft, dim=-1) * w
    y = torch.nn.functional.fold(fr.transpose(1, 2), (1, (F - 1) * hop + n_fft), (1, n_fft), stride=(1, hop)).reshape(R, -1)
    y = torch.nn.functional.pad(y, (0, max(0, lead + T - y.shape[1])))[:, lead:lead + T]
    live = ws >= 1e-8
    return torch.where(live, y / torch.where(live, ws, torch.ones_like(ws)).to(y.dtype), torch.zeros_like(y))


def _gl_unit(t):
    """unit(t) of include/wun.h in t's precision: scaled by max(|Re|, |Im|), unit(0) = 1, NaN stays NaN."""
    re, im = t.real, t.imag
    zero = (re == 0) & (im == 0)
    s = torch.where(zero, torch.ones_like(re), torch.maximum(re.abs(), im.abs()))
    s = torch.where(torch.isnan(re) | torch.isnan(im), torch.full_like(s, float("nan")), s)
    a, b = re / s, im / s
    n = torch.sqrt(a * a + b * b)
    return torch.complex(torch.where(zero, torch.ones_like(a), a / n), torch.where(zero, torch.zeros_like(b), b / n))


def griffin_lim_torch(mag, c0, y0, T, n_fft, hop, lead, iterations, momentum=0.0, dtype=torch.float32):
    """The definition of wun_griffin_lim (include/wun.h) in plain torch, in `dtype`: mag [R, F, K], exactly one of c0 (complex
    [R, F, K]) and y0 ([R, T]).  Returns (y [R, T], inconsistency float64 [iterations, 2]).  What griffin_lim runs on CPU
    tensors, and the tests' float32 stand-in."""
    cdtype = torch.complex64 if dtype == torch.float32 else torch.complex128
    mag = mag.to(dtype)
    R, F, K = (int(v) for v in mag.shape)
    w = _gl_window(n_fft, dtype, mag.device)
    ws = _gl_window_sums(T, n_fft, hop, lead, F, mag.device)
    inc = torch.full((iterations, 2), float("nan"), dtype=torch.float64)
    y = None if y0 is None else y0.to(dtype)
    prev = None
    for i in range(iterations):
        if i == 0 and c0 is not None:
            c = c0.to(cdtype).clone()
            c.imag[..., 0] = 0
            c.imag[..., -1] = 0
        else:
            c = _gl_stft(y, n_fft, hop, lead, F, w)
            m64 = mag.to(torch.float64)
            inc[i, 0] = ((c.to(torch.complex128).abs() - m64) ** 2).sum()
            inc[i, 1] = (m64 * m64).sum()
        t = c if (momentum == 0.0 or prev is None) else c + float(momentum) * (c - prev)
        prev = c
        u = _gl_unit(t)
        y = _gl_istft(torch.complex(mag * u.real, mag * u.imag), T, n_fft, hop, lead, w, ws)
    return y, inc


def griffin_lim_call(mag, init_re, init_im, y_init, T, n_fft, hop, lead, iterations, momentum=0.0, y=None, inconsistency=None,
                     scratch=None):
    """wun_griffin_lim on device tensors: mag (and init_re / init_im) float32 [R, F, K], y_init [R, T]; rows as S = R, B = C = 1.
    y, inconsistency (float64 [iterations, 2] or None) and scratch are the caller's or allocated here.  Returns y [R, T]."""
    lib = _lib.load()
    R, F, K = (int(v) for v in mag.shape)
    dev = mag.device
    if scratch is None:
        n = _lib.count(lib.wun_griffin_lim_scratch_floats(R, 1, int(T), 1, int(n_fft), int(hop), int(lead), F, int(momentum != 0.0)))
        scratch = torch.empty(n, dtype=torch.float32, device=dev)
    if y is None:
        y = torch.empty((R, int(T)), dtype=torch.float32, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    with torch.cuda.device(dev):
        _lib.check(lib.wun_griffin_lim(ptr(mag), ptr(init_re), ptr(init_im), ptr(y_init), R, 1, int(T), 1, int(n_fft), int(hop),
                                       int(lead), F, int(iterations), float(momentum), _fft_table(n_fft, dev).data_ptr(), ptr(y),
                                       ptr(inconsistency), ptr(scratch), _lib.stream(dev)))
    return y


def griffin_lim_default_length(F, n_fft, hop, centered=True):
    """The longest track whose framing has F frames: F hop - (n_fft - hop) centred, (F - 1) hop + n_fft otherwise."""
    return int(F) * int(hop) - (int(n_fft) - int(hop)) if centered else (int(F) - 1) * int(hop) + int(n_fft)


def griffin_lim(mag, n_fft, hop, iterations=10, init=None, length=None, centered=True, momentum=0.0, generator=None,
                return_inconsistency=False):
    """Audio [..., length] whose STFT magnitude approaches mag [..., F, K]: Griffin-Lim's alternating projections
    (wun_griffin_lim, include/wun.h; the reference's Utils.reconPhase), n_fft a power of two in 64..8192.

    init: an (re, im) pair of mag's shape -- the initial spectrum, e.g. a mix's (its phase is what counts) --, an audio tensor
    [..., length], or None: the reference's random start, the spectrum U[0, 1) + i U[-pi, pi) (Utils.py:163 takes its angle),
    drawn with torch on mag's device from `generator`.  length=None: the longest track with F frames in the chosen framing
    (centered as spectral.stft).  momentum in [0, 1): 0 is the plain iteration, 0.99 the usual accelerated one (Perraudin et al.).
    return_inconsistency: also a float64 [iterations, 2] tensor of sum (|STFT(y_{i-1})| - mag)^2 and sum mag^2 per iteration
    (NaN for an iteration that started from a given spectrum); sqrt of their ratio is the spectral convergence.

    On the GPU one library call, no host sync.  On CPU tensors the same definition in plain float32 torch (griffin_lim_torch).
    The inverse is wun_istft's (window-square-normalised).  Not differentiable."""
    if not torch.is_tensor(mag) or mag.dim() < 2:
        raise ValueError("mag must be a tensor [..., F, K]")
    n_fft, hop, iterations, momentum = int(n_fft), int(hop), int(iterations), float(momentum)
    F, K = int(mag.shape[-2]), int(mag.shape[-1])
    if K != n_fft // 2 + 1:
        raise ValueError("mag has %d bins, expected n_fft / 2 + 1 = %d" % (K, n_fft // 2 + 1))
    if iterations < 1:
        raise ValueError("iterations must be at least 1, got %d" % iterations)
    if not (0.0 <= momentum < 1.0):
        raise ValueError("momentum must lie in [0, 1), got %r" % (momentum,))
    T = griffin_lim_default_length(F, n_fft, hop, centered) if length is None else int(length)
    if T < 1:
        raise ValueError("no sample is covered: %d frames of %d / %d" % (F, n_fft, hop))
    lead, want = _framing(T, n_fft, hop, centered, "fft")
    if want != F:
        raise ValueError("mag has %d frames, length %d has %d in this framing" % (F, T, want))
    batch = tuple(mag.shape[:-2])
    dev = mag.device
    m = mag.to(torch.float32).reshape(-1, F, K).contiguous()
    init_re = init_im = y_init = None
    if init is None:
        init_re = torch.rand(m.shape, generator=generator, dtype=torch.float32, device=dev)
        init_im = (torch.rand(m.shape, generator=generator, dtype=torch.float32, device=dev) * 2.0 - 1.0) * float(np.pi)
    elif isinstance(init, (tuple, list)):
        if len(init) != 2 or any((not torch.is_tensor(t)) or t.shape != mag.shape or t.device != dev for t in init):
            raise ValueError("init must be an (re, im) pair of mag's shape and device")
        init_re, init_im = (t.to(torch.float32).reshape(-1, F, K).contiguous() for t in init)
    elif torch.is_tensor(init):
        if tuple(init.shape) != batch + (T,) or init.device != dev:
            raise ValueError("an audio init must be %s on mag's device, got %s" % (list(batch + (T,)), tuple(init.shape)))
        y_init = init.to(torch.float32).reshape(-1, T).contiguous()
    else:
        raise ValueError("init must be None, an (re, im) pair or an audio tensor")
    if m.is_cuda:
        inc = torch.empty((iterations, 2), dtype=torch.float64, device=dev) if return_inconsistency else None
        y = griffin_lim_call(m, init_re, init_im, y_init, T, n_fft, hop, lead, iterations, momentum, inconsistency=inc)
    else:
        c0 = None if init_re is None else torch.complex(init_re, init_im)
        y, inc = griffin_lim_torch(m, c0, y_init, T, n_fft, hop, lead, iterations, momentum)
    y = y.reshape(batch + (T,))
    return (y, inc) if return_inconsistency else y
