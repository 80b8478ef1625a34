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

Not built (NotImplementedError): the audio output at training=True (the raw-audio objective), stereo, any source count but two
(the reference asserts both, :24-25) and a bf16 mode.
model_config["spec_frame_len"] / ["spec_hop"] (extension keys, defaults 1024 / 768) let tests run small geometries;
["spec_dropout"] (0.5), ["spec_bn_decay"] (0.999) and ["spec_dropout_seed"] (the separator's seed) are the training step's.
"""
import ctypes as C
import math

import numpy as np
import torch

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
        n = int(self._lib.wun_spec_num_tensors(C.byref(self._scfg)))
        if n < 0:
            _lib.check(n)
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

    # ------------------------------------------------------------------ shapes
    def get_padding(self, shape):
        """UnetSpectrogramSeparator.py:31-38: "same" convolutions -- the input shape is the output shape, one channel."""
        s = np.array([int(shape[0]), int(shape[1]), 1], dtype=np.int64)
        return s, s.copy()

    def frames(self, num_samples):
        """F of num_samples samples; ValueError where the network cannot take the length (:69)."""
        F = int(self._lib.wun_spec_frames(C.byref(self._scfg), int(num_samples)))
        if F < 0:
            _lib.check(F)
        return F

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
            n = int(self._lib.wun_spec_workspace_floats(C.byref(self._scfg), B, T))
            if n < 0:
                _lib.check(n)
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
            return {name: out[i] for i, name in enumerate(self.source_names)}
        with torch.cuda.device(dev):
            _lib.check(self._lib.wun_spec_forward(
                C.byref(self._scfg), self.params.data_ptr(), mix.data_ptr(), B, T, spectral._fft_table(self.frame_len, dev).data_ptr(),
                None if return_spectrogram else out.data_ptr(), out.data_ptr() if return_spectrogram else None,
                self._ws[(B, T)].data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return {name: out[i] for i, name in enumerate(self.source_names)}

    # ------------------------------------------------------------------ the training step
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self._dev()).cuda_stream)

    def _train_workspace(self, B, T):
        if (B, T) not in self._tws:
            n = int(self._lib.wun_spec_train_workspace_floats(C.byref(self._scfg), B, T))
            if n < 0:
                _lib.check(n)
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
