"""The spectrogram U-Net baseline in inference mode: the reference's UnetSpectrogramSeparator
(/root/reference/Models/UnetSpectrogramSeparator.py:7-108; configs unet_spectrogram / unet_spectrogram_l1, Config.py:136-161)
on wun_spec_forward (include/wun.h).

    sep = UnetSpectrogramSeparator(get_config("unet_spectrogram"))
    outs = sep.get_output(mix, False)                              # mix [B, T, 1] -> {source: [B, T, 1]} audio
    mags = sep.get_output(mix, False, return_spectrogram=True)     # {source: [B, F, K]} magnitudes

One U-Net per source over log1p |STFT(mix)| (frame 1024, hop 768, periodic Hann, the last bin dropped): 5 x 5 stride-2
convolutions with inference batch norm and LeakyReLU down, their transposes with ReLU and skip concatenations up, a sigmoid mask
that multiplies the mixture's spectrogram; audio through tf.contrib.signal.inverse_stft's normaliser (wun_istft_tf).  T must be
(F - 1) hop + frame_len with F and frame_len / 2 multiples of 2 ** num_layers.

Not built (NotImplementedError): training this model (training=True: batch-statistics batch norm, dropout, the backward of the
2-D convolutions), stereo, any source count but two (the reference asserts both, :24-25) and a bf16 mode.
model_config["spec_frame_len"] / ["spec_hop"] (extension keys, defaults 1024 / 768) let tests run small geometries.
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
    """U-Net separator on magnitude spectrograms (UnetSpectrogramSeparator.py:7-12), inference only."""

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
        self.adam_m = self.adam_v = None # zeros: checkpoints keep their layout; nothing here trains
        self.global_step = 0
        self._ws = {}                    # (B, T) -> workspace
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

    # ------------------------------------------------------------------ forward
    def get_output(self, input, training, return_spectrogram=False, reuse=True):
        """UnetSpectrogramSeparator.py:40-108 at training=False.  input: [batch, num_samples, 1] float32 (a tensor, or
        anything np.asarray accepts).  Returns source_name -> [batch, num_samples, 1] audio, or with return_spectrogram
        [batch, F, frame_len / 2 + 1] magnitudes (views of one buffer the next call of the same shape overwrites)."""
        if training:
            raise NotImplementedError("the spectrogram U-Net is built for inference only: training=True (batch-statistics "
                                      "batch norm, dropout, the 2-D backward) is out of scope")
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
        with torch.cuda.device(dev):
            _lib.check(self._lib.wun_spec_forward(
                C.byref(self._scfg), self.params.data_ptr(), mix.data_ptr(), B, T, spectral._fft_table(self.frame_len, dev).data_ptr(),
                None if return_spectrogram else out.data_ptr(), out.data_ptr() if return_spectrogram else None,
                self._ws[(B, T)].data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return {name: out[i] for i, name in enumerate(self.source_names)}


def make_separator(model_config, device=None):
    """The separator class model_config["network"] names (Test.py:14-19, Evaluate.py, Training.py:31-36)."""
    if model_config["network"] == "unet":
        from .separator import UnetAudioSeparator
        return UnetAudioSeparator(model_config, device=device) if device is not None else UnetAudioSeparator(model_config)
    if model_config["network"] == "unet_spectrogram":
        return UnetSpectrogramSeparator(model_config, device=device)
    raise NotImplementedError(model_config["network"])
