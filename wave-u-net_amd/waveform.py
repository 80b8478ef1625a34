"""The waveform training losses of libwun.so (include/wun.h: wun_waveform_*): MSE and L1 over all floats, the
scale-invariant SDR and the SNR per excerpt, their weighted total and its gradient with respect to the estimates.

    loss = WaveformLoss({"l1": 1.0, "si_sdr": 0.05})
    losses, d_outputs = loss.loss_and_grad(outputs, targets)     # [total, mse, l1, si_sdr, snr, SI-SDR dB per source, SNR dB per source]
    loss.term_losses(losses)["si_sdr"]                           # the unweighted term, a view of `losses`
    loss.source_metrics(losses)["si_sdr"]                        # [S] dB per source, higher is better
    sep.loss_and_gradients(targets, loss=loss)                   # the training step's loss (UnetAudioSeparator, Trainer)
    waveform_loss(net(mix), targets, loss)                       # under torch.autograd, for users of sep.module()
    both = CombinedLoss(spectral.SpectralLoss.multi_resolution(), loss)      # the sum of the two totals, one gradient

Audio is float32 [S, B, T, C] channel-last on the GPU, as get_output stacks its outputs; a row of the per-excerpt terms is one
(source, excerpt) with all its channels.  There is no CPU path.
"""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .spectral import _audio

TERMS = ("mse", "l1", "si_sdr", "snr")       # the order of the term slots of wun_waveform_loss's losses
METRICS = ("mse", "si_sdr")                  # model_config["validation_metric"]


class WaveformLoss(object):
    """total = sum_t terms[t] * term_t over TERMS (a missing name is weight 0 and is not computed): "mse" and "l1" the means of
    (out - tgt)^2 and |out - tgt| over all floats, "si_sdr" and "snr" minus the mean over the S B excerpts of the scale-invariant
    SDR and of the SNR in dB (include/wun.h has the definitions).  zero_mean removes each excerpt's mean first.  eps = 1e-8 is a
    choice, not a measurement: 80 dB below an excerpt of unit energy, far above the float64 sums' own error.  The protocol is
    spectral.SpectralLoss's: num_losses, scratch_floats, _scratch_for, run, loss_and_grad, term_losses, from_config, __call__."""

    def __init__(self, terms, eps=1e-8, zero_mean=True):
        terms = dict(terms or {})
        unknown = set(terms) - set(TERMS)
        if unknown:
            raise ValueError("terms: unknown names %s (known: %s)" % (sorted(unknown), ", ".join(TERMS)))
        self.terms = {t: float(terms.get(t, 0.0)) for t in TERMS}
        for w in self.terms.values():
            if not (w >= 0.0 and np.isfinite(w)):
                raise ValueError("term weights must be finite and >= 0, got %r" % (w,))
        if not any(w > 0.0 for w in self.terms.values()):
            raise ValueError("terms: at least one of %s needs a weight > 0" % ", ".join(TERMS))
        self.eps, self.zero_mean = float(eps), bool(zero_mean)
        if not (self.eps > 0.0 and np.isfinite(self.eps)):
            raise ValueError("eps must be finite and > 0, got %r" % (eps,))
        self._terms = _lib.WunWaveformTerms(*([self.terms[t] for t in TERMS] + [self.eps, int(self.zero_mean)]))
        self._S = None           # sources of the last run: the layout of `losses`
        self._scratch = {}       # (shape, device) -> float32 scratch of wun_waveform_scratch_floats

    @classmethod
    def from_config(cls, spec):
        """model_config["waveform_loss"]: None, a WaveformLoss, or a dict with `terms`, `eps`, `zero_mean`."""
        if spec is None or isinstance(spec, cls):
            return spec
        unknown = set(spec) - {"terms", "eps", "zero_mean"}
        if unknown:
            raise ValueError("waveform_loss: unknown keys %s" % sorted(unknown))
        return cls(spec.get("terms"), spec.get("eps", 1e-8), spec.get("zero_mean", True))

    def num_losses_for(self, S):
        """Floats of `losses` for S sources: 5 + 2 S."""
        return 5 + 2 * int(S)

    @property
    def num_losses(self):
        """Floats of `losses` for the sources of the last scratch_floats / _scratch_for call: 5 + 2 S."""
        if self._S is None:
            raise ValueError("num_losses depends on the number of sources: call _scratch_for / scratch_floats first")
        return self.num_losses_for(self._S)

    def term_losses(self, losses):
        """{name: 0-dim view of `losses`}: the unweighted terms (0 for a term of weight 0)."""
        return {t: losses[1 + i] for i, t in enumerate(TERMS)}

    def source_metrics(self, losses):
        """{"si_sdr": [S] view, "snr": [S] view} of `losses`: the mean over a source's excerpts, dB, higher is better (0 for a
        term of weight 0)."""
        S = (int(losses.shape[0]) - 5) // 2
        return {"si_sdr": losses[5:5 + S], "snr": losses[5 + S:5 + 2 * S]}

    def scratch_floats(self, shape):
        S, B, T, Cn = (int(v) for v in shape)
        n = _lib.count(_lib.load().wun_waveform_scratch_floats(S, B, T, Cn, C.byref(self._terms)))
        self._S = S
        return n

    def _scratch_for(self, x):
        key = (tuple(x.shape), str(x.device))
        if key not in self._scratch:
            self._scratch[key] = torch.empty(self.scratch_floats(x.shape), dtype=torch.float32, device=x.device)
        self._S = int(x.shape[0])
        return self._scratch[key]

    def run(self, outputs, targets, d_outputs, losses, scratch, accumulate=False):
        """wun_waveform_loss on the caller's buffers (contiguous float32 device tensors; losses of 5 + 2 S floats; d_outputs may
        be None).  accumulate: ADD the gradient to what d_outputs holds (one fp32 add per float)."""
        S, B, T, Cn = (int(v) for v in outputs.shape)
        dev = outputs.device
        with torch.cuda.device(dev):
            _lib.check(_lib.load().wun_waveform_loss(
                outputs.data_ptr(), targets.data_ptr(), S, B, T, Cn, C.byref(self._terms), 1 if accumulate else 0,
                d_outputs.data_ptr() if d_outputs is not None else None, losses.data_ptr(), scratch.data_ptr(), _lib.stream(dev)))

    def loss_and_grad(self, outputs, targets, grad=True):
        """(losses, d_outputs): losses float32 [5 + 2 S] on the device = [total, mse, l1, si_sdr, snr, SI-SDR dB per source, SNR
        dB per source], d_outputs = d total / d outputs with the outputs' shape (None with grad=False).  No host sync."""
        outputs, targets = _audio(outputs, "outputs"), _audio(targets, "targets")
        if outputs.shape != targets.shape or outputs.device != targets.device:
            raise ValueError("outputs %s and targets %s differ in shape or device" % (tuple(outputs.shape), tuple(targets.shape)))
        scratch = self._scratch_for(outputs)
        losses = torch.empty(self.num_losses, dtype=torch.float32, device=outputs.device)
        d_outputs = torch.empty_like(outputs) if grad else None
        self.run(outputs, targets, d_outputs, losses, scratch)
        return losses, d_outputs

    def __call__(self, outputs, targets):
        """The total loss as a 0-dim tensor, differentiable with respect to `outputs` (waveform_loss)."""
        return waveform_loss(outputs, targets, self)


class CombinedLoss(object):
    """The sum of a spectral.SpectralLoss's total and a WaveformLoss's total, same protocol.  losses is [total | the spectral
    loss's losses | the waveform loss's losses] (parts); the spectral entry writes d_outputs and the waveform entry adds its
    gradient to it (accumulate: one fp32 add per float).  No host sync."""

    def __init__(self, spectral, waveform):
        from .spectral import SpectralLoss
        if not isinstance(spectral, SpectralLoss) or not isinstance(waveform, WaveformLoss):
            raise ValueError("CombinedLoss takes a spectral.SpectralLoss and a waveform.WaveformLoss, got %s and %s"
                             % (type(spectral).__name__, type(waveform).__name__))
        self.spectral, self.waveform = spectral, waveform

    @property
    def num_losses(self):
        return 1 + self.spectral.num_losses + self.waveform.num_losses

    def parts(self, losses):
        """(the spectral loss's slice, the waveform loss's slice) of `losses`, views."""
        ns = self.spectral.num_losses
        return losses[1:1 + ns], losses[1 + ns:]

    def scratch_floats(self, shape):
        return self.spectral.scratch_floats(shape), self.waveform.scratch_floats(shape)

    def _scratch_for(self, x):
        return self.spectral._scratch_for(x), self.waveform._scratch_for(x)

    def run(self, outputs, targets, d_outputs, losses, scratch):
        """scratch: the pair _scratch_for returns.  losses[0] = the two totals' sum, formed on the device."""
        sp, wv = self.parts(losses)
        self.spectral.run(outputs, targets, d_outputs, sp, scratch[0])
        self.waveform.run(outputs, targets, d_outputs, wv, scratch[1], accumulate=d_outputs is not None)
        torch.add(sp[0], wv[0], out=losses[0])

    def loss_and_grad(self, outputs, targets, grad=True):
        outputs, targets = _audio(outputs, "outputs"), _audio(targets, "targets")
        if outputs.shape != targets.shape or outputs.device != targets.device:
            raise ValueError("outputs %s and targets %s differ in shape or device" % (tuple(outputs.shape), tuple(targets.shape)))
        scratch = self._scratch_for(outputs)
        losses = torch.empty(self.num_losses, dtype=torch.float32, device=outputs.device)
        d_outputs = torch.empty_like(outputs) if grad else None
        self.run(outputs, targets, d_outputs, losses, scratch)
        return losses, d_outputs

    def __call__(self, outputs, targets):
        return waveform_loss(outputs, targets, self)


class _WaveformLoss(torch.autograd.Function):
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


def waveform_loss(outputs, targets, loss=None, **kw):
    """The total of a WaveformLoss (`loss`, or WaveformLoss(**kw)) as a 0-dim tensor under torch.autograd: backward gives
    d total / d outputs as wun_waveform_loss computes it; the targets get no gradient."""
    if loss is None:
        loss = WaveformLoss(**kw)
    return _WaveformLoss.apply(outputs, targets, loss)


def validation_metric(model_config):
    """model_config["validation_metric"]: "mse" (the default, the reference's) or "si_sdr"; ValueError for anything else."""
    metric = model_config.get("validation_metric", "mse")
    if metric not in METRICS:
        raise ValueError("validation_metric must be one of %s, got %r" % (", ".join(METRICS), metric))
    return metric


def validation_loss(model_config):
    """The WaveformLoss validation scores with under validation_metric = "si_sdr": {"si_sdr": 1} with the eps and zero_mean of
    model_config["waveform_loss"] if there is one, else the defaults."""
    spec = model_config.get("waveform_loss")
    if isinstance(spec, WaveformLoss):
        return WaveformLoss({"si_sdr": 1.0}, spec.eps, spec.zero_mean)
    spec = spec or {}
    return WaveformLoss({"si_sdr": 1.0}, spec.get("eps", 1e-8), spec.get("zero_mean", True))
