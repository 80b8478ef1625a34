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

Audio is float32 [S, B, T, C] channel-last on the GPU, as get_output stacks its outputs.  There is no CPU path.
"""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib

MAX_RESOLUTIONS = 8
TERMS = ("mag_l1", "log_mag_l1", "sc", "complex_l1")       # the order of the term slots of wun_spectral_loss_terms' losses
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
             "loss_terms_scratch": "wun_spectral_terms_scratch_floats"},
    "fft": {"table": ("wun_fft_table_floats", "wun_fft_design", 3), "frames": "wun_fft_frames",
            "centered_frames": "wun_fft_centered_frames", "stft": "wun_stft_complex_fft", "istft": "wun_istft_fft",
            "istft_scratch": "wun_istft_fft_scratch_floats", "istft_tf": "wun_istft_tf_fft",
            "istft_tf_scratch": "wun_istft_tf_fft_scratch_floats", "mask_filter": "wun_mask_filter_fft",
            "mask_filter_scratch": "wun_mask_filter_fft_scratch_floats", "wiener_filter": "wun_wiener_filter_fft",
            "wiener_filter_scratch": "wun_wiener_filter_fft_scratch_floats", "magnitude": "wun_stft_magnitude_fft",
            "loss": "wun_spectral_loss_fft", "loss_scratch": "wun_spectral_fft_scratch_floats",
            "loss_terms": "wun_spectral_loss_terms_fft", "loss_terms_scratch": "wun_spectral_terms_fft_scratch_floats"},
}
_TABLES = {}     # (transform, n_fft, device) -> device tensor holding the transform's table


def entry(transform, op):
    """(the library's entry of operation `op` on `transform`, the function (n_fft, device) -> that transform's device table)."""
    if transform not in _ENTRIES:
        raise ValueError("transform must be one of %s, got %r" % (", ".join(TRANSFORMS), transform))
    return getattr(_lib.load(), _ENTRIES[transform][op]), (_fft_table if transform == "fft" else _table)


def _design(transform, n_fft):
    floats, fill, lead = _ENTRIES[transform]["table"]
    lib = _lib.load()
    n = int(getattr(lib, floats)(int(n_fft)))
    if n < 0:
        _lib.check(n)
    table = np.zeros(n, np.float32)
    _lib.check(getattr(lib, fill)(int(n_fft), table.ctypes.data_as(C.POINTER(C.c_float)), n))
    return table.reshape(lead, int(n_fft), -1) if transform == "gemm" else table.reshape(lead, int(n_fft))


def _device_table(transform, n_fft, device):
    key = (transform, int(n_fft), str(device))
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(_design(transform, n_fft)).to(device)
    return _TABLES[key]


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
    n = int(entry(transform, op)[0](*args))
    if n < 0:
        _lib.check(n)
    return n


def frames(n, n_fft, hop, transform="gemm"):
    """Frames of n samples: 1 + (n - n_fft) // hop, no padding (wun_stft_frames; with transform="fft" wun_fft_frames, n_fft up
    to 8192)."""
    return count(transform, "frames", int(n), int(n_fft), int(hop))


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


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
                      _stream(x.device)))
    return mags


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
                      im.data_ptr(), _stream(x.device)))
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
                      table(n_fft, re.device).data_ptr(), y.data_ptr(), scratch.data_ptr(), _stream(re.device)))
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
                      table(n_fft, re.device).data_ptr(), y.data_ptr(), scratch.data_ptr(), _stream(re.device)))
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

    transform="gemm": both frame transforms of a resolution as GEMMs against an n_fft^2 table, n_fft up to 2048.  "fft": as
    FFTs (the *_fft entries), n_fft up to 8192 -- the same definitions, slots and summation order, results
    equal to float32 rounding.  ValueError for any other name."""

    def __init__(self, resolutions=((1024, 768),), weights=None, mse_weight=0.0, terms=None, log_eps=1e-3, sc_eps=1.0,
                 transform="gemm"):
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

    @classmethod
    def from_config(cls, spec):
        """model_config["spectral_loss"]: None, a SpectralLoss, or a dict with `resolutions`, `weights`, `mse_weight`, `terms`,
        `log_eps`, `sc_eps`, `transform`."""
        if spec is None or isinstance(spec, cls):
            return spec
        unknown = set(spec) - {"resolutions", "weights", "mse_weight", "terms", "log_eps", "sc_eps", "transform"}
        if unknown:
            raise ValueError("spectral_loss: unknown keys %s" % sorted(unknown))
        return cls(spec.get("resolutions", ((1024, 768),)), spec.get("weights"), spec.get("mse_weight", 0.0), spec.get("terms"),
                   spec.get("log_eps", 1e-3), spec.get("sc_eps", 1.0), spec.get("transform", "gemm"))

    @classmethod
    def multi_resolution(cls, transform="gemm", resolutions=None):
        """The usual multi-resolution STFT loss: spectral convergence + log-magnitude L1 at 512 / 128, 1024 / 256, 2048 / 512
        (or at `resolutions`; transform="fft" admits n_fft up to 8192)."""
        if resolutions is None:
            resolutions = [(512, 128), (1024, 256), (2048, 512)]
        return cls(resolutions, terms={"sc": 1.0, "log_mag_l1": 1.0}, transform=transform)

    @property
    def num_losses(self):
        """Floats of `losses`: 2 + nres, with terms 2 + 5 nres."""
        return 2 + (1 if self._terms is None else 5) * len(self.resolutions)

    def term_losses(self, losses):
        """{name: [nres] view of `losses`}: the unweighted terms per resolution (terms= only)."""
        if self._terms is None:
            raise ValueError("term_losses needs a SpectralLoss built with terms=")
        nres = len(self.resolutions)
        per = losses[2 + nres:2 + 5 * nres].view(nres, 4)
        return {t: per[:, i] for i, t in enumerate(TERMS)}

    def scratch_floats(self, shape):
        S, B, T, Cn = (int(v) for v in shape)
        args = (S, B, T, Cn, len(self.resolutions), self._n_fft, self._hop)
        if self._terms is None:
            return count(self.transform, "loss_scratch", *args)
        return count(self.transform, "loss_terms_scratch", *(args + (C.byref(self._terms),)))

    def _scratch_for(self, x):
        key = (tuple(x.shape), str(x.device))
        if key not in self._scratch:
            self._scratch[key] = torch.empty(self.scratch_floats(x.shape), dtype=torch.float32, device=x.device)
        return self._scratch[key]

    def run(self, outputs, targets, d_outputs, losses, scratch):
        """wun_spectral_loss (with terms: wun_spectral_loss_terms; transform="fft": their _fft twins) on the caller's buffers
        (contiguous float32 device tensors; losses of num_losses floats; d_outputs may be None)."""
        S, B, T, Cn = (int(v) for v in outputs.shape)
        dev = outputs.device
        nres = len(self.resolutions)
        fn, table = entry(self.transform, "loss" if self._terms is None else "loss_terms")
        tabs = (C.c_void_p * max(nres, 1))(*[table(n, dev).data_ptr() for n, _ in self.resolutions])
        head = (outputs.data_ptr(), targets.data_ptr(), S, B, T, Cn, self.mse_weight, nres, self._n_fft, self._hop, self._w)
        tail = (tabs, d_outputs.data_ptr() if d_outputs is not None else None, losses.data_ptr(), scratch.data_ptr(), _stream(dev))
        with torch.cuda.device(dev):
            if self._terms is None:
                _lib.check(fn(*(head + tail)))
            else:
                _lib.check(fn(*(head + (C.byref(self._terms),) + tail)))

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
