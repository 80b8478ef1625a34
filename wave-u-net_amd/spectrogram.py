"""The spectrogram U-Net baseline: the reference's UnetSpectrogramSeparator
(/root/reference/Models/UnetSpectrogramSeparator.py:7-108; configs unet_spectrogram / unet_spectrogram_l1, Config.py:136-161)
on wun_spec_forward (include/wun.h) and, for training on magnitudes, wun_spec_train_forward /
wun_spec_loss_backward / wun_spec_adam_step.

    sep = UnetSpectrogramSeparator(get_config("unet_spectrogram"))
    outs = sep.get_output(mix, False)                              # mix [B, T, 1] -> {source: [B, T, 1]} audio
    mags = sep.get_output(mix, False, return_spectrogram=True)     # {source: [B, F, K]} magnitudes

One U-Net per source over log1p |STFT(mix)| (frame 1024, hop 768, periodic Hann, the last bin dropped): 5 x 5 stride-2
convolutions with inference batch norm and LeakyReLU down, their transposes with ReLU and skip concatenations up, a sigmoid mask
that multiplies the mixture's spectrogram; audio through tf.contrib.signal.inverse_stft's normaliser (wun_istft_tf).  T must be
(F - 1) hop + frame_len with F and frame_len / 2 multiples of 2 ** num_layers.

Training on the magnitude objective (raw_audio_loss=False: Jansson's L1, Training.py:55-63):

    mags = sep.get_output(mix, True, return_spectrogram=True)      # batch statistics, dropout
    loss = sep.loss_and_gradients(targets)                         # targets {source: [B, T, 1]} or stacked [S, B, T, 1] audio
    sep.adam_step(lr)                                              # TF-Adam + the batch norms' moving averages

Any other loss, on magnitudes, audio or both (wun_spec_backward, wun_spec_train_audio):

    audio = sep.audio_output()                                     # {source: [B, T, 1]} of that training forward
    sep.backward(d_mags=..., d_audio=...)                          # dL/d mags [S, B, F, K] and / or dL/d audio [S, B, T, 1] -> sep.grads
    sep.adam_step(lr)                                              # or sep.update_moving_averages() beside another optimizer
    net = sep.module("audio")                                      # SpecUNet, a torch.nn.Module: net(mix) under torch.autograd

Audio from the magnitudes with a refined phase (wun_griffin_lim):

    audio = sep.reconstruct(mags, mix, iterations=10)              # Griffin-Lim from the mix's phase, {source: [B, T, 1]}

Not built (NotImplementedError): get_output's own audio at training=True (ask audio_output() for it), the gradient with respect
to the mix, stereo, any source count but two (the reference asserts both, :24-25) and a bf16 mode.
model_config["spec_frame_len"] / ["spec_hop"] (extension keys, defaults 1024 / 768) let tests run small geometries;
["spec_dropout"] (0.5), ["spec_bn_decay"] (0.999) and ["spec_dropout_seed"] (the separator's seed) are the training step's.
"""
import ctypes as C
import math

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib, spectral
from .config import finalize


class _Table(object):
    """What checkpoint.py reads of a plan: .tensors = [(tf_name, offset, shape)]."""
    def __init__(self, tensors):
        self.tensors = tensors


class UnetSpectrogramSeparator(object):
    """U-Net separator on magnitude spectrograms (UnetSpectrogramSeparator.py:7-12)."""

    def __init__(self, model_config, device=None, seed=1337):
        cfg = finalize(model_config) if "source_names" not in model_config else dict(model_config)
        self.model_config = cfg
        self.num_layers = int(cfg["num_layers"])                 # UnetSpectrogramSeparator.py:19-22
        self.num_initial_filters = int(cfg["num_initial_filters"])
        self.mono = bool(cfg["mono_downmix"])
        self.source_names = list(cfg["source_names"])
        if len(self.source_names) != 2:                          # :24
            raise NotImplementedError("the spectrogram U-Net separates two sources (accompaniment / voice), got %d: "
                                      "other source counts are out of scope" % len(self.source_names))
        if not self.mono:                                        # :25
            raise NotImplementedError("the spectrogram U-Net is mono only (mono_downmix=True): stereo is out of scope")
        if cfg.get("compute_dtype", "f32") != "f32":
            raise NotImplementedError("the spectrogram U-Net has no bf16 mode: out of scope")
        self.num_channels = 1
        self.frame_len = int(cfg.get("spec_frame_len", 1024))    # :28-29
        self.hop = int(cfg.get("spec_hop", 768))

        self._lib = _lib.load()                                  # raises if libwun.so is missing
        self._scfg = _lib.WunSpecConfig(self.num_layers, self.num_initial_filters, len(self.source_names), self.frame_len, self.hop)
        n = _lib.count(self._lib.wun_spec_num_tensors(C.byref(self._scfg)))
        tensors, info = [], _lib.WunTensorInfo()
        for i in range(n):
            _lib.check(self._lib.wun_spec_tensor(C.byref(self._scfg), i, C.byref(info)))
            tensors.append((info.name.decode(), int(info.offset), tuple(int(info.shape[d]) for d in range(info.ndim))))
        self._table = _Table(tensors)
        self.num_params = int(self._lib.wun_spec_param_floats(C.byref(self._scfg)))
        self._seed = seed
        self._device = torch.device(device) if device is not None else None
        self.params = None               # flat float32 buffer, table order
        self.grads = self.adam_m = self.adam_v = None
        self.global_step = 0
        self._tcfg = _lib.WunSpecTrainConfig(float(cfg.get("spec_bn_decay", 0.999)), float(cfg.get("spec_dropout", 0.5)),
                                             int(cfg.get("spec_dropout_seed", seed)))
        self.last_losses = None          # [total, per source] of the last loss_and_gradients (device)
        self._ws = {}                    # (B, T) -> workspace
        self._tws = {}                   # (B, T) -> training workspace
        self._last_train = None          # (B, T) of the last training forward
        self._outs = {}                  # (B, T, return_spectrogram) -> output buffer
        self._tws_gen = {}               # (B, T) -> training forwards that wrote the training workspace
        self._scr = {}                   # (kind, B, T) -> scratch of audio_output / backward

    # ------------------------------------------------------------------ shapes
    def get_padding(self, shape):
        """UnetSpectrogramSeparator.py:31-38: "same" convolutions -- the input shape is the output shape, one channel."""
        s = np.array([int(shape[0]), int(shape[1]), 1], dtype=np.int64)
        return s, s.copy()

    def frames(self, num_samples):
        """F of num_samples samples; ValueError where the network cannot take the length (:69)."""
        return _lib.count(self._lib.wun_spec_frames(C.byref(self._scfg), int(num_samples)))

    # ------------------------------------------------------------------ variables
    def _dev(self):
        if self._device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("wave-u-net_amd needs an MI355X (no CPU fallback)")
            self._device = torch.device("cuda", torch.cuda.current_device())
        return self._device

    @property
    def device(self):
        return self._dev()

    def variable_table(self):
        """[(tf_name, offset, shape)] in TF creation order."""
        return list(self._table.tensors)

    def initial_values(self):
        """The flat float32 host buffer of TF's initial values: glorot-uniform kernels, zero biases, beta and moving_mean,
        unit moving_variance."""
        host = np.zeros(self.num_params, dtype=np.float32)
        rng = np.random.default_rng(self._seed)
        for name, off, shp in self._table.tensors:
            size = int(np.prod(shp))
            if name.endswith("/kernel"):
                rf = int(np.prod(shp[:-2]))
                lim = math.sqrt(6.0 / ((shp[-2] + shp[-1]) * rf))
                host[off:off + size] = rng.uniform(-lim, lim, size=size).astype(np.float32)
            elif name.endswith("/moving_variance"):
                host[off:off + size] = 1.0
        return host

    def _any_plan(self):
        return self._table

    def _ensure_variables(self, plan=None):
        if self.params is not None:
            return
        dev = self._dev()
        self.params = torch.from_numpy(self.initial_values()).to(dev)
        self.adam_m = torch.zeros(self.num_params, dtype=torch.float32, device=dev)
        self.adam_v = torch.zeros(self.num_params, dtype=torch.float32, device=dev)
        self.grads = torch.zeros(self.num_params, dtype=torch.float32, device=dev)

    def variables(self):
        """dict tf_name -> tensor view into the flat buffer."""
        self._ensure_variables()
        return {name: self.params[off:off + int(np.prod(shp))].view(*shp) for name, off, shp in self._table.tensors}

    def load_variables(self, named):
        """named: dict or list of (tf_name, array)."""
        items = named.items() if isinstance(named, dict) else named
        self._ensure_variables()
        index = {name: (off, shp) for name, off, shp in self._table.tensors}
        for name, val in items:
            off, shp = index[name]
            t = torch.as_tensor(np.asarray(val), dtype=torch.float32).reshape(-1)
            assert t.numel() == int(np.prod(shp)), (name, t.shape, shp)
            self.params[off:off + t.numel()].copy_(t)

    def gradients(self):
        """dict tf_name -> gradient view (after loss_and_gradients); the moving statistics' are 0."""
        return {name: self.grads[off:off + int(np.prod(shp))].view(*shp) for name, off, shp in self._table.tensors}

    # ------------------------------------------------------------------ forward
    def get_output(self, input, training, return_spectrogram=False, reuse=True):
        """UnetSpectrogramSeparator.py:40-108.  input: [batch, num_samples, 1] float32 (a tensor, or anything np.asarray
        accepts).  Returns source_name -> [batch, num_samples, 1] audio, or with return_spectrogram
        [batch, F, frame_len / 2 + 1] magnitudes (views of one buffer the next call of the same shape overwrites).
        training=True (batch statistics, dropout keyed by global_step) is built for return_spectrogram=True."""
        if training and not return_spectrogram:
            raise NotImplementedError("the spectrogram U-Net's audio output is built for inference only: at training=True "
                                      "ask for return_spectrogram=True (train with raw_audio_loss=False)")
        if not torch.is_tensor(input):
            input = torch.as_tensor(np.asarray(input, dtype=np.float32))
        if input.dim() != 3 or input.shape[2] != 1:                              # :53
            raise ValueError("input must be [batch, samples, 1] (mono), got %s" % (tuple(input.shape),))
        B, T = int(input.shape[0]), int(input.shape[1])
        F = self.frames(T)                                                       # every refusal before any GPU work
        dev = self._dev()
        mix = input.to(device=dev, dtype=torch.float32).contiguous()
        self._ensure_variables()
        S, K = len(self.source_names), self.frame_len // 2 + 1
        if (B, T) not in self._ws:
            n = _lib.count(self._lib.wun_spec_workspace_floats(C.byref(self._scfg), B, T))
            self._ws[(B, T)] = torch.empty(n, dtype=torch.float32, device=dev)
        key = (B, T, bool(return_spectrogram))
        if key not in self._outs:
            self._outs[key] = torch.empty((S, B, F, K) if return_spectrogram else (S, B, T, 1), dtype=torch.float32, device=dev)
        out = self._outs[key]
        if training:
            with torch.cuda.device(dev):
                _lib.check(self._lib.wun_spec_train_forward(
                    C.byref(self._scfg), C.byref(self._tcfg), self.params.data_ptr(), mix.data_ptr(), B, T,
                    spectral._fft_table(self.frame_len, dev).data_ptr(), self.global_step, out.data_ptr(),
                    self._train_workspace(B, T).data_ptr(), self._stream()))
            self._last_train = (B, T)
            self._tws_gen[(B, T)] = self._tws_gen.get((B, T), 0) + 1
            return {name: out[i] for i, name in enumerate(self.source_names)}
        with torch.cuda.device(dev):
            _lib.check(self._lib.wun_spec_forward(
                C.byref(self._scfg), self.params.data_ptr(), mix.data_ptr(), B, T, spectral._fft_table(self.frame_len, dev).data_ptr(),
                None if return_spectrogram else out.data_ptr(), out.data_ptr() if return_spectrogram else None,
                self._ws[(B, T)].data_ptr(), _lib.stream(dev)))
        return {name: out[i] for i, name in enumerate(self.source_names)}

    # ------------------------------------------------------------------ the training step
    def _stream(self):
        return _lib.stream(self._dev())

    def _train_workspace(self, B, T):
        if (B, T) not in self._tws:
            n = _lib.count(self._lib.wun_spec_train_workspace_floats(C.byref(self._scfg), B, T))
            self._tws[(B, T)] = torch.empty(n, dtype=torch.float32, device=self._dev())
        return self._tws[(B, T)]

    def loss_and_gradients(self, targets):
        """Jansson's L1 on magnitudes (Training.py:55-63) of the last get_output(x, True, return_spectrogram=True) and its
        gradients into self.grads.  targets: {source: [B, T, 1]} or stacked [S, B, T, 1] AUDIO (their STFT magnitudes are taken
        here, in the model's framing).  Returns the loss as a 0-dim device tensor; last_losses holds [loss, per source]."""
        if self._last_train is None:
            raise RuntimeError("loss_and_gradients needs a get_output(x, True, return_spectrogram=True) first")
        B, T = self._last_train
        dev, S = self._dev(), len(self.source_names)
        if isinstance(targets, dict):
            targets = torch.stack([torch.as_tensor(targets[n]) for n in self.source_names])
        tg = torch.as_tensor(targets).to(device=dev, dtype=torch.float32).contiguous()
        if tuple(tg.shape) != (S, B, T, 1):
            raise ValueError("targets must be [%d, %d, %d, 1], got %s" % (S, B, T, tuple(tg.shape)))
        losses = torch.empty(1 + S, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(self._lib.wun_spec_loss_backward(
                C.byref(self._scfg), C.byref(self._tcfg), self.params.data_ptr(), tg.data_ptr(), B, T,
                spectral._fft_table(self.frame_len, dev).data_ptr(), self.grads.data_ptr(), losses.data_ptr(),
                self._train_workspace(B, T).data_ptr(), self._stream()))
        self.last_losses = losses
        return losses[0]

    def adam_step(self, lr, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
        """tf.train.AdamOptimizer(learning_rate=lr) on kernels, biases and betas, the batch norms' moving averages from the last
        training forward (the UPDATE_OPS, Training.py:74-77), global_step += 1."""
        if self._last_train is None:
            raise RuntimeError("adam_step needs a training forward and loss_and_gradients first")
        B, T = self._last_train
        self.global_step += 1
        with torch.cuda.device(self._dev()):
            _lib.check(self._lib.wun_spec_adam_step(
                C.byref(self._scfg), C.byref(self._tcfg), self.params.data_ptr(), self.grads.data_ptr(), self.adam_m.data_ptr(),
                self.adam_v.data_ptr(), self._train_workspace(B, T).data_ptr(), B, T, self.global_step, lr, beta1, beta2, eps,
                grad_scale, self._stream()))

    # ------------------------------------------------------------------ any loss
    def _scratch(self, kind, B, T):
        if (kind, B, T) not in self._scr:
            query = self._lib.wun_spec_train_audio_scratch_floats if kind == "audio" else self._lib.wun_spec_backward_scratch_floats
            n = _lib.count(query(C.byref(self._scfg), B, T))
            self._scr[(kind, B, T)] = torch.empty(n, dtype=torch.float32, device=self._dev())
        return self._scr[(kind, B, T)]

    def _train_audio(self, B, T, out):
        dev = self._dev()
        with torch.cuda.device(dev):
            _lib.check(self._lib.wun_spec_train_audio(
                C.byref(self._scfg), C.byref(self._tcfg), B, T, spectral._fft_table(self.frame_len, dev).data_ptr(), out.data_ptr(),
                self._train_workspace(B, T).data_ptr(), self._scratch("audio", B, T).data_ptr(), self._stream()))
        return out

    def audio_output(self):
        """{source: [B, T, 1]} audio of the last get_output(x, True, return_spectrogram=True): ISTFT_tf(mask X) from what that
        forward retained (a fresh tensor per call; the workspace and the variables are left as they are)."""
        if self._last_train is None:
            raise RuntimeError("audio_output needs a get_output(x, True, return_spectrogram=True) first")
        B, T = self._last_train
        out = self._train_audio(B, T, torch.empty((len(self.source_names), B, T, 1), dtype=torch.float32, device=self._dev()))
        return {name: out[i] for i, name in enumerate(self.source_names)}

    def reconstruct(self, mags, mix, iterations, momentum=0.0):
        """{source: [B, T, 1]} audio from source magnitudes `mags` ({source: [B, F, K]} or stacked [S, B, F, K], e.g. what
        get_output(mix, False, return_spectrogram=True) returned) by `iterations` Griffin-Lim iterations in the network's framing
        (lead 0) from the spectrum of `mix` [B, T, 1] -- the reference's spectrogramToAudioFile(.., phase=mix_phase,
        phaseIterations=N), Utils.py:125-173; spectral.griffin_lim, DESIGN.md 5.21.  mask X with the mix's phase is not the STFT
        of any signal; the iterations move the phase until magnitude and phase agree better.  The mix's spectrum is taken again
        here (one launch of the transform the network ran: the same bits).  The inverse is wun_istft's, normalised by the
        window-square sum over the covering frames -- not inverse_stft_window_fn's steady-state sum, so the audio differs from
        get_output's at the clip's edges even before the phase moves."""
        if isinstance(mags, dict):
            mags = torch.stack([torch.as_tensor(mags[n]) for n in self.source_names])
        if not torch.is_tensor(mix):
            mix = torch.as_tensor(np.asarray(mix, dtype=np.float32))
        if mix.dim() != 3 or mix.shape[2] != 1:
            raise ValueError("mix must be [batch, samples, 1] (mono), got %s" % (tuple(mix.shape),))
        B, T = int(mix.shape[0]), int(mix.shape[1])
        S, K = len(self.source_names), self.frame_len // 2 + 1
        F = self.frames(T)
        dev = self._dev()
        mags = torch.as_tensor(mags).to(device=dev, dtype=torch.float32)
        if tuple(mags.shape) != (S, B, F, K):
            raise ValueError("mags must be [%d, %d, %d, %d], got %s" % (S, B, F, K, tuple(mags.shape)))
        x = mix.to(device=dev, dtype=torch.float32).reshape(1, B, T, 1).contiguous()
        re, im = spectral.stft(x, self.frame_len, self.hop, centered=False, transform="fft")           # [1, B, 1, F, K]
        init = tuple(t.reshape(1, B, F, K).expand(S, B, F, K).contiguous() for t in (re, im))
        y = spectral.griffin_lim(mags, self.frame_len, self.hop, iterations, init=init, length=T, centered=False, momentum=momentum)
        return {name: y[i].unsqueeze(-1) for i, name in enumerate(self.source_names)}

    def _upstream(self, g, what, shape):
        if g is None:
            return None
        if isinstance(g, dict):
            g = torch.stack([torch.as_tensor(g[n]) for n in self.source_names])
        g = torch.as_tensor(g).to(device=self._dev(), dtype=torch.float32).contiguous()
        if tuple(g.shape) != shape:
            raise ValueError("%s must be %s, got %s" % (what, list(shape), tuple(g.shape)))
        return g

    def _backward_into(self, params, grads, d_mags, d_audio, B, T):
        dev = self._dev()
        with torch.cuda.device(dev):
            _lib.check(self._lib.wun_spec_backward(
                C.byref(self._scfg), C.byref(self._tcfg), params.data_ptr(), None if d_mags is None else d_mags.data_ptr(),
                None if d_audio is None else d_audio.data_ptr(), B, T, spectral._fft_table(self.frame_len, dev).data_ptr(),
                grads.data_ptr(), self._train_workspace(B, T).data_ptr(), self._scratch("backward", B, T).data_ptr(), self._stream()))

    def backward(self, d_mags=None, d_audio=None):
        """The gradients of any loss on the last training forward's outputs into self.grads: d_mags = dL/d mags
        ({source: [B, F, K]} or stacked [S, B, F, K]), d_audio = dL/d audio ({source: [B, T, 1]} or [S, B, T, 1]), either or both.
        Afterwards gradients() and adam_step(lr) behave as after loss_and_gradients."""
        if self._last_train is None:
            raise RuntimeError("backward needs a get_output(x, True, return_spectrogram=True) first")
        if d_mags is None and d_audio is None:
            raise ValueError("backward needs d_mags, d_audio or both")
        B, T = self._last_train
        S, K = len(self.source_names), self.frame_len // 2 + 1
        d_mags = self._upstream(d_mags, "d_mags", (S, B, self.frames(T), K))
        d_audio = self._upstream(d_audio, "d_audio", (S, B, T, 1))
        self._backward_into(self.params, self.grads, d_mags, d_audio, B, T)

    def update_moving_averages(self):
        """The batch norms' UPDATE_OPS alone (Training.py:74-75), from the last training forward: what adam_step does after its
        update, for a step whose optimizer is not adam_step.  global_step is left alone."""
        if self._last_train is None:
            raise RuntimeError("update_moving_averages needs a training forward first")
        B, T = self._last_train
        with torch.cuda.device(self._dev()):
            _lib.check(self._lib.wun_spec_update_moving_averages(
                C.byref(self._scfg), C.byref(self._tcfg), self.params.data_ptr(), self._train_workspace(B, T).data_ptr(), B, T,
                self._stream()))

    def module(self, output="audio"):
        """This separator as a torch.nn.Module (SpecUNet) whose forward gives "audio" [S, B, T, 1], "mags" [S, B, F, K] or
        "both" (audio, mags)."""
        return SpecUNet(self, output)

    def activation(self, kind, source, layer):
        """A tensor the last training forward retained (wun_spec_train_tensor), as a view of the workspace.  kind: "z" (pre-norm),
        "mean", "var" (batch statistics), "act" (post-activation; layer 2L-1: the mask [B, F, K-1]) or "dropout" (layer = up level;
        the multipliers 0 and 1 / (1 - rate); None where the level has no dropout).  layer: 0..L-1 down, L..2L-2 up."""
        kinds = {"z": _lib.SPEC_TT_Z, "mean": _lib.SPEC_TT_MEAN, "var": _lib.SPEC_TT_VAR, "act": _lib.SPEC_TT_ACT,
                 "dropout": _lib.SPEC_TT_DROPOUT}
        if self._last_train is None:
            raise RuntimeError("activation needs a training forward first")
        B, T = self._last_train
        off, cnt = C.c_int64(), C.c_int64()
        _lib.check(self._lib.wun_spec_train_tensor(C.byref(self._scfg), B, T, kinds[kind], int(source), int(layer),
                                                   C.byref(off), C.byref(cnt)))
        if cnt.value == 0 or (kind == "dropout" and self._tcfg.dropout_rate == 0.0):
            return None
        flat = self._tws[(B, T)][off.value:off.value + cnt.value]
        L, F, W0 = self.num_layers, self.frames(T), self.frame_len // 2
        if kind in ("mean", "var"):
            return flat
        if kind == "act" and layer == 2 * L - 1:
            return flat.view(B, F, W0)
        if kind == "dropout":
            sh = L - 1 - layer                               # the input map of transposed layer `layer + 1`
            return flat.view(B, F >> sh, W0 >> sh, -1)
        sh = layer + 1 if layer < L else 2 * L - 1 - layer
        return flat.view(B, F >> sh, W0 >> sh, -1)


def make_separator(model_config, device=None):
    """The separator class model_config["network"] names (Test.py:14-19, Evaluate.py, Training.py:31-36)."""
    if model_config["network"] == "unet":
        from .separator import UnetAudioSeparator
        return UnetAudioSeparator(model_config, device=device) if device is not None else UnetAudioSeparator(model_config)
    if model_config["network"] == "unet_spectrogram":
        return UnetSpectrogramSeparator(model_config, device=device)
    raise NotImplementedError(model_config["network"])


# ---------------------------------------------------------------------- torch.autograd
class _TrainOutput(torch.autograd.Function):
    """(audio [S, B, T, 1] and / or mags [S, B, F, K]) of a training forward with the parameters in `arena`; the backward pass is
    wun_spec_backward from the gradients of whichever outputs the loss used."""

    @staticmethod
    def forward(ctx, arena, mix, sep, output, step):
        B, T = int(mix.shape[0]), int(mix.shape[1])
        F, S, K = sep.frames(T), len(sep.source_names), sep.frame_len // 2 + 1
        dev = arena.device
        mags = torch.empty((S, B, F, K), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(sep._lib.wun_spec_train_forward(
                C.byref(sep._scfg), C.byref(sep._tcfg), arena.data_ptr(), mix.data_ptr(), B, T,
                spectral._fft_table(sep.frame_len, dev).data_ptr(), int(step), mags.data_ptr(), sep._train_workspace(B, T).data_ptr(),
                sep._stream()))
        sep._last_train = (B, T)
        sep._tws_gen[(B, T)] = sep._tws_gen.get((B, T), 0) + 1
        ctx.sep, ctx.key, ctx.gen, ctx.output = sep, (B, T), sep._tws_gen[(B, T)], output
        ctx.save_for_backward(arena)
        ctx.set_materialize_grads(False)             # an output the loss did not use gives None: that head is not run
        if output == "mags":
            return mags
        audio = sep._train_audio(B, T, torch.empty((S, B, T, 1), dtype=torch.float32, device=dev))
        return audio if output == "audio" else (audio, mags)

    @staticmethod
    @once_differentiable
    def backward(ctx, *d_outputs):
        (arena,) = ctx.saved_tensors                 # (torch's version check: the arena must not change before backward)
        sep, key = ctx.sep, ctx.key
        if sep._tws_gen.get(key) != ctx.gen:
            raise RuntimeError("wave_u_net_amd: another training forward of shape %s ran on the shared workspace after this "
                               "one; run backward before the next forward of the same shape" % (key,))
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        d_audio = d_outputs[0] if ctx.output != "mags" else None
        d_mags = d_outputs[-1] if ctx.output != "audio" else None
        d_audio, d_mags = (None if g is None else g.to(torch.float32).contiguous() for g in (d_audio, d_mags))
        grads = torch.zeros_like(arena)              # the moving statistics' floats stay 0 for torch optimizers
        if d_audio is not None or d_mags is not None:
            sep._backward_into(arena, grads, d_mags, d_audio, key[0], key[1])
        return grads, None, None, None, None


class SpecUNet(torch.nn.Module):
    """A UnetSpectrogramSeparator as a torch.nn.Module, on the model of autograd.WaveUNet.  forward(mix [B, T, 1]) gives
    output="audio": [S, B, T, 1];  "mags": [S, B, F, K];  "both": (audio, mags) -- fresh tensors per call, source_names order.
    train(): batch statistics, dropout keyed by `dropout_step` (starts at the separator's global_step, advances by one per
    training forward, settable), differentiable w.r.t. `arena`, the ONE nn.Parameter that shares storage with sep.params (the
    moving statistics' floats get gradient 0).  eval(): wun_spec_forward under no_grad.  The separator keeps one training
    workspace per (batch, samples): a second training forward of the same shape before the first one's backward makes that
    backward raise RuntimeError.  Second-order gradients are not supported."""

    def __init__(self, sep, output="audio"):
        super().__init__()
        if output not in ("audio", "mags", "both"):
            raise ValueError('output must be "audio", "mags" or "both", got %r' % (output,))
        self.sep, self.output = sep, output
        sep._ensure_variables()
        self.arena = torch.nn.Parameter(sep.params, requires_grad=True)    # shares storage with sep.params
        assert self.arena.data_ptr() == sep.params.data_ptr()
        self.tensors = list(sep._table.tensors)
        self.dropout_step = int(sep.global_step)

    def forward(self, mix):
        if torch.is_tensor(mix) and mix.requires_grad:
            raise NotImplementedError("the spectrogram U-Net has no gradient with respect to the mix: it would pass through |X|, "
                                      "which has a kink at 0, log1p and the phase; detach the mix")
        if not torch.is_tensor(mix):
            mix = torch.as_tensor(np.asarray(mix, dtype=np.float32))
        if mix.dim() != 3 or mix.shape[2] != 1:
            raise ValueError("input must be [batch, samples, 1] (mono), got %s" % (tuple(mix.shape),))
        sep = self.sep
        sep.frames(int(mix.shape[1]))                # every refusal before any GPU work
        if not self.training:
            with torch.no_grad():
                outs = [torch.stack([o[n] for n in sep.source_names]) for o in
                        (sep.get_output(mix, False, return_spectrogram=r) for r in ((False,) if self.output == "audio" else
                                                                                     (True,) if self.output == "mags" else (False, True)))]
            return outs[0] if len(outs) == 1 else tuple(outs)
        mix = mix.to(device=self.arena.device, dtype=torch.float32).contiguous()
        step = self.dropout_step
        self.dropout_step += 1
        return _TrainOutput.apply(self.arena, mix, sep, self.output, step)

    def update_moving_averages(self):
        """The batch norms' UPDATE_OPS from the last training forward (what a torch optimizer does not do)."""
        with torch.no_grad():
            self.sep.update_moving_averages()

    def named_variables(self):
        """tf_name -> view of the arena."""
        return {name: self.arena[off:off + int(np.prod(shp))].view(*shp) for name, off, shp in self.tensors}

    def variable_grads(self):
        """tf_name -> view of arena.grad (after backward), or None."""
        g = self.arena.grad
        if g is None:
            return None
        return {name: g[off:off + int(np.prod(shp))].view(*shp) for name, off, shp in self.tensors}
