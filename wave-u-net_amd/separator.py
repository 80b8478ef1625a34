"""Host-side mirror of the reference's separator object for the hot path.

Same constructor / get_padding / get_output surface as
/root/reference/Models/UnetAudioSeparator.py:9-144 (what Training.py:29-47, Test.py:15-34 and
Evaluate.py:28-47 call), driving the gfx950 kernels in libwun.so through the C ABI of
include/wun.h.  Because there is no tf.gradients here, the object additionally exposes
`loss_and_gradients` (Training.py:50-63 + the backward implied by :77) and `adam_step`
(tf.train.AdamOptimizer, Training.py:77).

torch is used for device memory, streams and torch.distributed only.
"""
import contextlib
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .config import finalize

_UPS = {"linear": 0, "learned": 1}
_OUT = {"direct": 0, "difference": 1}
_ACT = {"tanh": 0, "linear": 1}
_DTYPE = {"f32": 0, "bf16": 1}      # extension key model_config["compute_dtype"] (no reference counterpart)


def _wun_config(cfg):
    if cfg.get("compute_dtype", "f32") not in _DTYPE:
        raise NotImplementedError("compute_dtype=%r" % (cfg["compute_dtype"],))
    for key, table in (("upsampling", _UPS), ("output_type", _OUT), ("output_activation", _ACT)):
        if cfg[key] not in table:
            raise NotImplementedError("%s=%r" % (key, cfg[key]))   # UnetAudioSeparator.py:136,144
    return _lib.WunConfig(
        cfg["num_layers"], cfg["num_initial_filters"], cfg["filter_size"], cfg["merge_filter_size"],
        cfg["input_filter_size"], cfg["output_filter_size"], _UPS[cfg["upsampling"]],
        _OUT[cfg["output_type"]], 1 if cfg["context"] else 0, len(cfg["source_names"]),
        1 if cfg["mono_downmix"] else 2, _ACT[cfg["output_activation"]], _DTYPE[cfg.get("compute_dtype", "f32")],
        1 if cfg.get("exclusive_streams", False) else 0)      # extension key: scheduling hint (wun.h), set by the Trainer


def check_clip_norm(clip_norm):
    """clip_norm of adam_step / Trainer -> the float wun_adam_step_clip takes: None = +inf (no clipping); ValueError unless
    > 0 (tf.clip_by_global_norm needs a positive clip_norm; NaN is refused)."""
    if clip_norm is None:
        return math.inf
    try:
        c = float(clip_norm)
    except (TypeError, ValueError):
        raise ValueError("clip_norm = %r must be a number > 0" % (clip_norm,))
    if isinstance(clip_norm, bool) or not c > 0:
        raise ValueError("clip_norm = %r must be > 0 (None or inf = no clipping)" % (clip_norm,))
    return c


def check_weight_decay(weight_decay):
    """weight_decay of adam_step / the optimizer dict -> float; ValueError unless a number >= 0 (NaN is refused)."""
    try:
        w = float(weight_decay)
    except (TypeError, ValueError):
        raise ValueError("weight_decay = %r must be a number >= 0" % (weight_decay,))
    if isinstance(weight_decay, bool) or not w >= 0 or math.isinf(w):
        raise ValueError("weight_decay = %r must be a finite number >= 0" % (weight_decay,))
    return w


def check_ema_decay(ema_decay):
    """ema_decay -> float; ValueError unless a number in [0, 1)."""
    try:
        d = float(ema_decay)
    except (TypeError, ValueError):
        raise ValueError("ema_decay = %r must be a number in [0, 1)" % (ema_decay,))
    if isinstance(ema_decay, bool) or not 0 <= d < 1:
        raise ValueError("ema_decay = %r must be in [0, 1)" % (ema_decay,))
    return d


class _Plan(object):
    def __init__(self, lib, wcfg, batch, frames):
        self.lib = lib
        self.handle = C.c_void_p()
        _lib.check(lib.wun_plan_create(C.byref(wcfg), batch, frames, C.byref(self.handle)))
        if wcfg.exclusive_streams:
            if torch.distributed.is_available() and torch.distributed.is_initialized():
                import warnings
                warnings.warn("wun: a plan with exclusive_streams=1 (lowest-priority side streams) was created while a "
                              "process group is initialised -- measured ~40 % slower beside a communication stream; pass "
                              "model_config['exclusive_streams'] = False", RuntimeWarning, stacklevel=3)
            _lib.LOW_PRIORITY_PLANS["created"] += 1
        self.info = _lib.WunPlanInfo()
        _lib.check(lib.wun_plan_query(self.handle, C.byref(self.info)))
        if int(self.info.compute_dtype_effective) != int(wcfg.compute_dtype):
            # (num_initial_filters % 8 != 0, a tap-less conv phase, rows beyond the bf16 kernels' offsets: include/wun.h)
            import warnings
            warnings.warn("wun: compute_dtype='bf16' was requested but this configuration does not qualify for the bf16 "
                          "mode -- the plan runs the exact-fp32 kernels (wun_plan_info.compute_dtype_effective = 0)",
                          RuntimeWarning, stacklevel=3)
        self.tensors = []
        for i in range(self.info.num_tensors):
            ti = _lib.WunTensorInfo()
            _lib.check(lib.wun_plan_tensor(self.handle, i, C.byref(ti)))
            self.tensors.append((ti.name.decode(), int(ti.offset),
                                 tuple(int(ti.shape[k]) for k in range(ti.ndim))))

    def __del__(self):
        try:
            if self.handle:
                self.lib.wun_plan_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class UnetAudioSeparator(object):
    """U-Net separator network on raw waveforms (UnetAudioSeparator.py:9-13)."""

    def __init__(self, model_config, device=None, seed=1337):
        cfg = finalize(model_config) if "source_names" not in model_config else dict(model_config)
        self.model_config = cfg
        self.num_layers = cfg["num_layers"]                      # UnetAudioSeparator.py:20-32
        self.num_initial_filters = cfg["num_initial_filters"]
        self.filter_size = cfg["filter_size"]
        self.merge_filter_size = cfg["merge_filter_size"]
        self.input_filter_size = cfg["input_filter_size"]
        self.output_filter_size = cfg["output_filter_size"]
        self.upsampling = cfg["upsampling"]
        self.output_type = cfg["output_type"]
        self.context = cfg["context"]
        self.padding = "valid" if cfg["context"] else "same"
        self.source_names = list(cfg["source_names"])
        self.num_channels = 1 if cfg["mono_downmix"] else 2
        self.output_activation = cfg["output_activation"]

        self._lib = _lib.load()                                   # raises if libwun.so is missing
        self._wcfg = _wun_config(cfg)
        self._seed = seed
        self._device = torch.device(device) if device is not None else None
        self._plans = {}
        self._active = None          # plan of the last get_output
        self.params = None           # flat float32 arena (TF creation order)
        self.grads = self.adam_m = self.adam_v = None
        self.global_step = 0
        self.ema = None              # EMA of params, an arena like adam_m (created on first use: _ensure_ema)
        self._in_ema = False         # inside ema_weights(): params and ema are exchanged
        self._step_phase = 0         # 1: a training forward is open, 2: gradients are pending (until adam_step)
        self._norm_ws = self._skipped = None     # wun_grad_norm workspace, skipped-step counter (allocated on first use)
        self._ws = {}
        self._ws_gen = {}            # (batch, frames) -> forward passes run on that workspace (autograd's stale-workspace guard)
        self._outs = {}
        self._d_outs = {}            # (batch, frames) -> dL / d outputs of loss_and_gradients(loss=...) (allocated on first use)
        self.last_losses = None      # [total, MSE, L_0, ...] of the last loss_and_gradients(loss=...)
        self._last_mix = None

    # ------------------------------------------------------------------ shapes
    def get_padding(self, shape):
        """UnetAudioSeparator.py:34-83.  shape = [batch, desired_output_frames, *]."""
        fin, fout = C.c_int64(), C.c_int64()
        _lib.check(self._lib.wun_get_padding(C.byref(self._wcfg), int(shape[1]), C.byref(fin),
                                             C.byref(fout)))
        b = int(shape[0])
        return (np.array([b, fin.value, self.num_channels], dtype=np.int64),
                np.array([b, fout.value, self.num_channels], dtype=np.int64))

    # ------------------------------------------------------------------ variables
    def _plan(self, batch, frames):
        key = (int(batch), int(frames))
        if key not in self._plans:
            self._plans[key] = _Plan(self._lib, self._wcfg, key[0], key[1])
        return self._plans[key]

    def _dev(self):
        if self._device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("wave-u-net_amd needs an MI355X (no CPU fallback)")
            self._device = torch.device("cuda", torch.cuda.current_device())
        return self._device

    @property
    def device(self):
        """The GPU the separator's arenas and workspaces live on (evaluate.separate_track keeps the track there)."""
        return self._dev()

    def variable_table(self, batch=1, frames=None):
        """[(tf_name, offset, shape)] in TF creation order."""
        if frames is None:
            frames = int(self.get_padding([batch, 1 if self.context else 2 ** self.num_layers, 0])[0][1])
        return list(self._plan(batch, frames).tensors)

    def _ensure_variables(self, plan):
        if self.params is not None:
            return
        n = int(plan.info.arena_floats)
        host = np.zeros(n, dtype=np.float32)
        rng = np.random.default_rng(self._seed)
        for name, off, shp in plan.tensors:              # glorot-uniform / zero bias (TF defaults)
            size = int(np.prod(shp))
            if name.endswith("/bias"):
                continue
            if len(shp) == 1:
                fan_in = fan_out = shp[0]
            else:
                rf = int(np.prod(shp[:-2]))
                fan_in, fan_out = shp[-2] * rf, shp[-1] * rf
            lim = math.sqrt(6.0 / (fan_in + fan_out))
            host[off:off + size] = rng.uniform(-lim, lim, size=size).astype(np.float32)
        dev = self._dev()
        self.params = torch.from_numpy(host).to(dev)
        self.grads = torch.zeros(n, dtype=torch.float32, device=dev)
        self.adam_m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.adam_v = torch.zeros(n, dtype=torch.float32, device=dev)

    def _any_plan(self):
        """The variable table is the same for every (batch, frames): use any plan, creating a
        minimal one if the separator has not been run yet."""
        if self._active is not None:
            return self._active
        if not self._plans:
            self.variable_table()
        return next(iter(self._plans.values()))

    def variables(self):
        """dict tf_name -> tensor view into the flat arena."""
        plan = self._any_plan()
        self._ensure_variables(plan)
        return {name: self.params[off:off + int(np.prod(shp))].view(*shp)
                for name, off, shp in plan.tensors}

    def gradients(self):
        plan = self._any_plan()
        self._ensure_variables(plan)
        return {name: self.grads[off:off + int(np.prod(shp))].view(*shp)
                for name, off, shp in plan.tensors}

    def load_variables(self, named):
        """named: dict or list of (tf_name, array)."""
        items = named.items() if isinstance(named, dict) else named
        plan = self._any_plan()
        self._ensure_variables(plan)
        index = {name: (off, shp) for name, off, shp in plan.tensors}
        for name, val in items:
            off, shp = index[name]
            t = torch.as_tensor(np.asarray(val), dtype=torch.float32).reshape(-1)
            assert t.numel() == int(np.prod(shp)), (name, t.shape, shp)
            self.params[off:off + t.numel()].copy_(t)

    # ------------------------------------------------------------------ forward
    def _stream(self):
        return _lib.stream(self._dev())

    def get_output(self, input, training, return_spectrogram=False, reuse=True):
        """UnetAudioSeparator.py:85-144.  input: [batch, num_samples, num_channels] float32
        (torch tensor on the GPU, or anything np.asarray accepts).  Returns a dict
        source_name -> [batch, num_out_samples, num_channels] torch tensor (views of one
        buffer that is overwritten by the next call with the same shape)."""
        if training:
            self._refuse_in_ema("get_output(training=True)")
        dev = self._dev()
        if not torch.is_tensor(input):
            input = torch.as_tensor(np.asarray(input, dtype=np.float32))
        mix = input.to(device=dev, dtype=torch.float32).contiguous()
        if mix.dim() != 3 or mix.shape[2] != self.num_channels:
            raise ValueError("input must be [batch, samples, %d]" % self.num_channels)
        plan = self._plan(mix.shape[0], mix.shape[1])
        self._ensure_variables(plan)
        key = (mix.shape[0], mix.shape[1])
        ws, outs = self._buffers(plan, key)
        _lib.check(self._lib.wun_forward(plan.handle, self.params.data_ptr(), mix.data_ptr(),
                                         ws.data_ptr(), outs.data_ptr(), 1 if training else 0,
                                         self._stream()))
        self._ws_gen[key] = self._ws_gen.get(key, 0) + 1
        self._active, self._last_mix, self._last_key = plan, mix, key
        self._last_training = bool(training)
        if training:
            self._step_phase = max(self._step_phase, 1)
        elif self._step_phase == 1:
            self._step_phase = 0
        return {name: outs[i] for i, name in enumerate(self.source_names)}

    # ------------------------------------------------------------------ whole tracks (wun_forward_windows / wun_separate_track)
    def _buffers(self, plan, key):
        """(workspace, outputs [S, B, Tout, C]) of the plan `key` = (batch, input frames), allocated on first use."""
        if key not in self._ws:
            dev = self._dev()
            self._ws[key] = torch.empty(int(plan.info.workspace_floats), dtype=torch.float32, device=dev)
            self._outs[key] = torch.empty((len(self.source_names), key[0], int(plan.info.output_frames), self.num_channels),
                                          dtype=torch.float32, device=dev)
        return self._ws[key], self._outs[key]

    def _default_frames(self):
        return int(self.get_padding([1, self.model_config["num_frames"], 0])[0][1])

    def _track(self, track):
        if not torch.is_tensor(track):
            track = torch.as_tensor(np.asarray(track, dtype=np.float32))
        track = track.to(device=self._dev(), dtype=torch.float32).contiguous()
        if track.dim() != 2 or track.shape[1] != self.num_channels:
            raise ValueError("track must be [frames, %d]" % self.num_channels)
        return track

    @staticmethod
    def _positions_arg(positions):
        pos = np.ascontiguousarray(np.asarray(positions, dtype=np.int64).reshape(-1))
        return pos, pos.ctypes.data_as(C.POINTER(C.c_int64))

    def workspace_floats(self, batch, frames):
        """wun_plan_info.workspace_floats of the plan for `batch` excerpts of `frames` input frames (wun_plan_query)."""
        return int(self._plan(batch, frames).info.workspace_floats)

    def get_output_windows(self, track, positions, training=False, frames=None, batch=None):
        """get_output on the batch whose row b is track[positions[b] : positions[b] + frames], without building that batch
        (wun_forward_windows: the rows are gathered from the track by the forward's first kernel).  track: [track_frames,
        num_channels] float32; frames: input frames of a hop (default: get_padding of model_config["num_frames"]); batch:
        the plan's batch (default len(positions); rows past the positions are zeros).  Returns what get_output returns --
        bit-identical to get_output on the stacked rows with the same batch.  `training` only selects the forward's own
        behaviour (True: no AudioClip): there is no materialised mix, so loss_and_gradients / backward refuse to run
        after this call (RuntimeError) -- use get_output for a training step."""
        track = self._track(track)
        pos, pos_p = self._positions_arg(positions)
        key = (int(batch) if batch is not None else int(pos.size), int(frames) if frames is not None else self._default_frames())
        plan = self._plan(*key)
        self._ensure_variables(plan)
        ws, outs = self._buffers(plan, key)
        _lib.check(self._lib.wun_forward_windows(plan.handle, self.params.data_ptr(), track.data_ptr(), int(track.shape[0]),
                                                 pos_p, int(pos.size), ws.data_ptr(), outs.data_ptr(), 1 if training else 0,
                                                 self._stream()))
        self._ws_gen[key] = self._ws_gen.get(key, 0) + 1
        self._active, self._last_key = plan, key
        self._last_mix, self._last_training = None, False      # (no materialised mix: the backward entries need get_output)
        return {name: outs[i] for i, name in enumerate(self.source_names)}

    def scatter_windows(self, positions, preds, frames=None, batch=None):
        """preds[s, positions[b] : positions[b] + Tout] = the estimates of hop b of the last get_output_windows /
        get_output with the same (batch, frames), hops in index order: where hops overlap the last one wins
        (wun_scatter_windows).  preds: [S, pred_frames, num_channels] float32 on the device, contiguous."""
        pos, pos_p = self._positions_arg(positions)
        key = (int(batch) if batch is not None else int(pos.size), int(frames) if frames is not None else self._default_frames())
        plan = self._plan(*key)
        if key not in self._outs:
            raise RuntimeError("no outputs for batch %d, %d frames: run get_output_windows first" % key)
        assert preds.is_contiguous() and preds.dtype == torch.float32 and preds.dim() == 3
        assert preds.shape[0] == len(self.source_names) and preds.shape[2] == self.num_channels
        _lib.check(self._lib.wun_scatter_windows(plan.handle, self._outs[key].data_ptr(), pos_p, int(pos.size),
                                                 preds.data_ptr(), int(preds.shape[1]), self._stream()))
        return preds

    def separate_padded(self, track, n_frames, batch_hops, frames=None, out=None):
        """The hop loop of Evaluate.predict_track (Evaluate.py:113-143) in one call (wun_separate_track).  track:
        [n_frames + 2 pad, num_channels], the track with pad = (input - output frames) // 2 zero frames on both sides;
        batch_hops: hops per forward pass (the plan's batch; a short last chunk runs on the same plan with zero rows);
        frames: input frames of a hop (default: get_padding of model_config["num_frames"]).  Returns the estimates
        [S, n_frames, num_channels] on the device (`out` when given).  No host synchronisation."""
        track = self._track(track)
        key = (int(batch_hops), int(frames) if frames is not None else self._default_frames())
        plan = self._plan(*key)
        self._ensure_variables(plan)
        ws, outs = self._buffers(plan, key)
        n_frames = int(n_frames)
        pad2 = int(plan.info.input_frames - plan.info.output_frames)
        if track.shape[0] != n_frames + pad2:
            raise ValueError("track has %d frames, expected n_frames + 2 pad = %d" % (track.shape[0], n_frames + pad2))
        if out is None:
            out = torch.empty((len(self.source_names), n_frames, self.num_channels), dtype=torch.float32, device=self._dev())
        assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (len(self.source_names), n_frames,
                                                                                             self.num_channels)
        _lib.check(self._lib.wun_separate_track(plan.handle, self.params.data_ptr(), track.data_ptr(), n_frames,
                                                ws.data_ptr(), outs.data_ptr(), out.data_ptr(), self._stream()))
        self._ws_gen[key] = self._ws_gen.get(key, 0) + 1
        self._active, self._last_key = plan, key
        self._last_mix, self._last_training = None, False
        return out

    def blend_windows(self, windows, preds, den, overlap_frames, frames=None, batch=None):
        """scatter_windows' blending counterpart (blend.blend_windows, wun_blend_windows): the estimates of the last
        get_output_windows / get_output with the same (batch, frames) are accumulated into preds [S, pred_frames,
        num_channels] and den [pred_frames] with the trapezoid weights of `overlap_frames`; windows: [nwin, 3] rows of
        (pos, row of the batch, flags) in the order of the separation's window list.  blend.blend_finish ends it."""
        from . import blend
        tab = np.asarray(windows, dtype=np.int64).reshape(-1, 3)
        key = (int(batch) if batch is not None else int(tab.shape[0]), int(frames) if frames is not None else self._default_frames())
        if key not in self._outs:
            raise RuntimeError("no outputs for batch %d, %d frames: run get_output_windows first" % key)
        return blend.blend_windows(self._outs[key], tab, overlap_frames, preds, den)

    def separate_padded_blend(self, track, n_frames, batch_hops, overlap_frames, shifts, lead, frames=None, out=None):
        """separate_padded with overlapping hops and shifted passes blended (wun_separate_track_blend).
        track: [track_frames, num_channels]: lead + pad zero frames, the track, then zeros for the overhanging last hop of
        every pass (pad = (input - output frames) // 2, lead >= max(shifts)); overlap_frames: frames two neighbouring hops
        share; shifts: the passes' frame offsets.  Returns the estimates [S, n_frames, num_channels] on the device (`out`
        when given).  No host synchronisation."""
        track = self._track(track)
        key = (int(batch_hops), int(frames) if frames is not None else self._default_frames())
        plan = self._plan(*key)
        self._ensure_variables(plan)
        ws, outs = self._buffers(plan, key)
        n_frames = int(n_frames)
        sh = np.ascontiguousarray(np.asarray(list(shifts), dtype=np.int64).reshape(-1))
        if out is None:
            out = torch.empty((len(self.source_names), max(n_frames, 0), self.num_channels), dtype=torch.float32, device=self._dev())
        assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (len(self.source_names), n_frames,
                                                                                             self.num_channels)
        den = torch.empty(max(n_frames, 1), dtype=torch.float32, device=self._dev())
        _lib.check(self._lib.wun_separate_track_blend(plan.handle, self.params.data_ptr(), track.data_ptr(), int(track.shape[0]),
                                                      int(lead), n_frames, int(overlap_frames),
                                                      sh.ctypes.data_as(C.POINTER(C.c_int64)), int(sh.size), ws.data_ptr(),
                                                      outs.data_ptr(), out.data_ptr(), den.data_ptr(), self._stream()))
        self._ws_gen[key] = self._ws_gen.get(key, 0) + 1
        self._active, self._last_key = plan, key
        self._last_mix, self._last_training = None, False
        return out

    # ------------------------------------------------------------------ training step pieces
    def select_mask(self, variables):
        """TF variable names -> the selection of wun_*_select (include/wun.h): a uint8 array with one byte per tensor in
        wun_plan_tensor order, or None for `variables=None` (every tensor).  KeyError for an unknown name."""
        if variables is None:
            return None
        if isinstance(variables, str):
            variables = [variables]
        plan = self._active if self._active is not None else self._any_plan()
        index = {name: k for k, (name, _, _) in enumerate(plan.tensors)}
        mask = np.zeros(len(plan.tensors), dtype=np.uint8)
        for name in variables:
            mask[index[name]] = 1                   # KeyError: not a variable of this separator
        return mask

    @staticmethod
    def _mask_arg(mask):
        if mask is None:
            return None, 0
        return mask.ctypes.data_as(C.POINTER(C.c_uint8)), int(mask.size)

    def loss_and_gradients(self, targets, bucket_starts=None, bucket_events=None, variables=None, accumulate=False, loss=None):
        """MSE loss averaged over sources (Training.py:50-63) and its gradient w.r.t. every
        separator variable.  targets: dict source_name -> [B, Tout, C] or a stacked
        [S, B, Tout, C] tensor.  Must follow get_output(training=True).  Returns the loss as
        a 0-dim GPU tensor (no host sync).

        bucket_starts / bucket_events (optional, data parallel): arena offsets in descending
        order and one torch.cuda.Event per bucket; event k is recorded as soon as all gradients
        at offsets >= bucket_starts[k] are final (see include/wun.h, wun_loss_backward_ex).

        variables: TF variable names whose gradients are wanted (None = all).  The others' floats in self.grads are not
        written, and launches no selected gradient needs are skipped (wun_loss_backward_select).

        accumulate: ADD the gradients to what self.grads holds (wun_loss_backward_accumulate: one fp32 add per float, the
        loss is still written) -- k micro-batches per optimizer step.

        loss: a spectral.SpectralLoss replaces the MSE by mse_weight * MSE + sum_j weight_j * (STFT-magnitude L1 at
        resolution j) (Training.py:55-60): wun_spectral_loss writes the loss and dL / d outputs, then the backward pass runs
        from that gradient (wun_backward_ex / _select / _accumulate), so variables, accumulate and the bucket events mean
        what they mean above.  Returns the total; self.last_losses holds [total, MSE, L_0, ...] (device tensor, L_j
        unweighted; a loss built with terms= adds its per-term slots, SpectralLoss.term_losses).  None: exactly the calls above.

        `loss` is ANY object of this protocol: `_scratch_for(outputs)` -> the scratch it wants (called first), `num_losses` ->
        the floats of its losses, `run(outputs, targets, d_outputs, losses, scratch)` -> writes losses (losses[0] the total)
        and d total / d outputs on the current stream without a host sync.  spectral.SpectralLoss, waveform.WaveformLoss
        (MSE, L1, SI-SDR, SNR; last_losses is then [total, mse, l1, si_sdr, snr, dB per source ...]) and
        waveform.CombinedLoss (the sum of the two) are the package's own."""
        self._refuse_in_ema("loss_and_gradients")
        mask = self.select_mask(variables)
        if self._active is None or not self._last_training:
            raise RuntimeError("call get_output(..., training=True) first")
        tg = self._stacked(targets, "targets")
        self._step_phase = 2
        if loss is not None:
            outs = self._outs[self._last_key]
            if self._last_key not in self._d_outs:
                self._d_outs[self._last_key] = torch.empty_like(outs)
            dout = self._d_outs[self._last_key]
            scratch = loss._scratch_for(outs)              # (first: a loss's num_losses may depend on the shape)
            losses = torch.empty(loss.num_losses, dtype=torch.float32, device=self._dev())
            loss.run(outs, tg, dout, losses, scratch)
            self._run_backward(self._ws[self._last_key], outs, dout, self.grads, None, bucket_starts, bucket_events, mask,
                               accumulate)
            self.last_losses = losses
            return losses[0]
        loss = torch.empty((), dtype=torch.float32, device=self._dev())
        fn, sel = self._backward_entry("wun_loss_backward", mask, accumulate)
        _lib.check(fn(self._active.handle, self.params.data_ptr(), self._last_mix.data_ptr(),
                      self._ws[self._last_key].data_ptr(), self._outs[self._last_key].data_ptr(), tg.data_ptr(),
                      self.grads.data_ptr(), loss.data_ptr(), self._stream(),
                      *self._bucket_args(bucket_starts, bucket_events), *sel))
        return loss

    @staticmethod
    def _bucket_args(bucket_starts, bucket_events):
        """(bucket_starts, bucket_events, nbuckets) of the backward entries: int64 arena offsets and event handles (one
        unused element each when there are no buckets)."""
        nb = len(bucket_starts) if bucket_starts else 0
        starts = (C.c_int64 * max(nb, 1))(*([int(x) for x in bucket_starts] if nb else [0]))
        events = (C.c_void_p * max(nb, 1))(*([int(e.cuda_event) for e in bucket_events] if nb else [0]))
        return starts, events, nb

    def _backward_entry(self, stem, mask, accumulate):
        """The C entry point of a backward pass (stem "wun_loss_backward" or "wun_backward") and its trailing selection
        arguments: <stem>_accumulate when accumulating, <stem>_ex for every variable, else <stem>_select."""
        suffix = "_accumulate" if accumulate else "_ex" if mask is None else "_select"
        return getattr(self._lib, stem + suffix), (() if suffix == "_ex" else self._mask_arg(mask))

    def _stacked(self, x, what):
        """dict source_name -> [B, Tout, C] or [S, B, Tout, C] -> one contiguous float32 [S, B, Tout, C] on the device,
        checked against the outputs of the last get_output."""
        dev = self._dev()
        if isinstance(x, dict):
            x = torch.stack([torch.as_tensor(x[n]).to(dev, torch.float32) for n in self.source_names])
        else:
            x = torch.as_tensor(x).to(dev, torch.float32)
        x = x.contiguous()
        outs = self._outs[self._last_key]
        if tuple(x.shape) != tuple(outs.shape):
            raise ValueError("%s shape %s != outputs shape %s" % (what, tuple(x.shape), tuple(outs.shape)))
        return x

    def backward(self, d_outputs, input_grad=False, bucket_starts=None, bucket_events=None, variables=None, accumulate=False):
        """Backward pass of the last get_output(training=True) from an arbitrary upstream gradient (wun_backward): what
        tf.gradients gives the reference for any loss built on the outputs.  d_outputs: dL/d outputs, as the targets of
        loss_and_gradients (dict source_name -> [B, Tout, C] or a stacked [S, B, Tout, C] tensor).  The parameter gradients
        are written to self.grads (overwritten, as loss_and_gradients does); returns dL/d mix [B, Tin, C] when input_grad,
        else None.  bucket_starts / bucket_events: as for loss_and_gradients.  variables: TF variable names whose gradients
        are wanted (None = all; the others' floats in self.grads are not written); variables=[] with input_grad=True is the
        input-only gradient (wun_backward_select).  accumulate: ADD the parameter gradients to self.grads
        (wun_backward_accumulate); dL/d mix is still written."""
        self._refuse_in_ema("backward")
        mask = self.select_mask(variables)
        if self._active is None or not self._last_training:
            raise RuntimeError("call get_output(..., training=True) first")
        dout = self._stacked(d_outputs, "d_outputs")
        if mask is None or mask.any():
            self._step_phase = 2
        d_mix = torch.empty(tuple(self._last_mix.shape), dtype=torch.float32, device=self._dev()) if input_grad else None
        self._run_backward(self._ws[self._last_key], self._outs[self._last_key], dout, self.grads, d_mix,
                           bucket_starts, bucket_events, mask, accumulate)
        return d_mix

    def _run_backward(self, ws, outs, dout, grads, d_mix, bucket_starts=None, bucket_events=None, mask=None,
                      accumulate=False):
        fn, sel = self._backward_entry("wun_backward", mask, accumulate)
        gp = grads.data_ptr() if (grads is not None and (mask is None or mask.any())) else None   # (input-only: not touched)
        _lib.check(fn(self._active.handle, self.params.data_ptr(), None, ws.data_ptr(), outs.data_ptr(), dout.data_ptr(),
                      gp, d_mix.data_ptr() if d_mix is not None else None, self._stream(),
                      *self._bucket_args(bucket_starts, bucket_events), *sel))

    def module(self):
        """This separator as a torch.nn.Module (wave_u_net_amd.autograd.WaveUNet): get_output under torch.autograd, the
        parameter arena as one nn.Parameter sharing storage with self.params."""
        from .autograd import WaveUNet
        return WaveUNet(self)

    def tune(self, input, targets):
        """Autotune the kernels of this (batch, length) plan on real buffers: one forward +
        backward with per-launch timing of candidate tilings (wun_plan_tune).  Returns the loss."""
        dev = self._dev()
        mix = torch.as_tensor(input).to(device=dev, dtype=torch.float32).contiguous()
        self.get_output(mix, True)                         # allocates plan / workspace / outputs
        tg = self._stacked(targets, "targets")
        loss = torch.empty((), dtype=torch.float32, device=dev)
        _lib.check(self._lib.wun_plan_tune(
            self._active.handle, self.params.data_ptr(), mix.data_ptr(), self._ws[self._last_key].data_ptr(),
            self._outs[self._last_key].data_ptr(), tg.data_ptr(), self.grads.data_ptr(), loss.data_ptr(),
            self._stream()))
        return loss

    def tune_export(self):
        """The tuned per-launch choices of the active plan as text (wun_plan_tune_export)."""
        buf = C.create_string_buffer(1 << 16)
        _lib.check(self._lib.wun_plan_tune_export(self._active.handle, buf, len(buf)))
        return buf.value.decode()

    def tune_import(self, text):
        """Reuse choices exported by a plan of the same config / batch / length (ValueError otherwise)."""
        _lib.check(self._lib.wun_plan_tune_import(self._active.handle, text.encode()))

    # ------------------------------------------------------------------ EMA of the weights (wun_optim_step, wun_ema_update)
    def _ensure_ema(self):
        """The EMA arena, created on first use as a copy of params (TF's shadow variables start at the variable's value)."""
        if self.ema is None:
            self._ensure_variables(self._active if self._active is not None else self._any_plan())
            self.ema = self.params.clone()
        return self.ema

    def ema_variables(self):
        """dict tf_name -> numpy array of the EMA values (RuntimeError when no EMA exists)."""
        if self.ema is None:
            raise RuntimeError("this separator has no EMA of its weights (adam_step(ema_decay=...) / ema_update create one)")
        plan = self._any_plan()
        host = self.ema.cpu().numpy()
        return {name: host[off:off + int(np.prod(shp))].reshape(shp).copy() for name, off, shp in plan.tensors}

    def ema_update(self, decay, warmup=False, variables=None, step=None):
        """ema -= (1 - d_t) * (ema - params) on `variables` (None = all), d_t = decay or, with warmup, min(decay, (1 + step) /
        (10 + step)) -- tf.train.ExponentialMovingAverage.apply; wun_ema_update, the bits of adam_step(ema_decay=...) for the
        same params.  step: default global_step.  For weights updated by another optimizer (torch.optim on module())."""
        self._refuse_in_ema("ema_update")
        decay = check_ema_decay(decay)
        mask = self.select_mask(variables)
        plan = self._active if self._active is not None else self._any_plan()
        ema = self._ensure_ema()
        _lib.check(self._lib.wun_ema_update(plan.handle, ema.data_ptr(), self.params.data_ptr(), decay,
                                            int(self.global_step if step is None else step),
                                            _lib.WUN_OPTIM_EMA_WARMUP if warmup else 0, self._stream(), *self._mask_arg(mask)))

    @contextlib.contextmanager
    def ema_weights(self):
        """Run get_output / separate_padded / validation ... on the EMA values: inside the block the library is handed the EMA
        arena where it takes the parameters (the arenas are exchanged, nothing is copied; whatever a plan derives from the
        weights -- the bf16 mode's packed images, the transposed copies -- is rebuilt from the arena it is handed by every
        forward pass, so it follows).  The trained weights are back on exit, also after an exception.  Refused between a
        training forward and the optimizer step that consumes its gradients (adam_step, or discard_gradients() for gradients
        that were only inspected).  Inside the block the separator infers only: get_output(training=True), loss_and_gradients,
        backward, adam_step and ema_update are refused, so no gradient of the EMA values can reach the trained weights.  The
        autograd module (module()) holds the trained arena itself, so its forward is refused inside the block too."""
        if self.ema is None:
            raise RuntimeError("this separator has no EMA of its weights (adam_step(ema_decay=...) / ema_update create one)")
        if self._step_phase:
            raise RuntimeError("ema_weights() between a training forward pass and its adam_step: %s (adam_step applies, "
                               "discard_gradients() abandons them)" %
                               ("gradients are pending" if self._step_phase == 2 else "a training forward is open"))
        self._refuse_in_ema("ema_weights")
        self.params, self.ema = self.ema, self.params
        self._in_ema = True
        try:
            yield self
        finally:
            self.params, self.ema = self.ema, self.params
            self._in_ema = False

    def _refuse_in_ema(self, what):
        if self._in_ema:
            raise RuntimeError("%s inside ema_weights(): params and ema are exchanged there, the block is for inference" % what)

    def discard_gradients(self):
        """Abandon an open training forward / pending gradients (computed to read grad_norm, to inspect, ...) without an
        optimizer step: self.grads keeps its floats, but loss_and_gradients / backward need a new get_output(training=True),
        and ema_weights() may be entered again."""
        self._step_phase, self._last_training = 0, False

    def decay_mask(self, decay_variables):
        """decay_variables of adam_step -> wun_optim_step's decay_select: None = every conv kernel (tensors of rank > 1) and no
        bias; else the named variables (validated like variables=)."""
        if decay_variables is None:
            plan = self._active if self._active is not None else self._any_plan()
            return np.array([1 if len(shp) > 1 else 0 for _, _, shp in plan.tensors], dtype=np.uint8)
        return self.select_mask(decay_variables)

    def adam_step(self, lr, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, variables=None, clip_norm=None,
                  skip_nonfinite=False, weight_decay=0.0, decay_variables=None, ema_decay=None, ema_warmup=False):
        """tf.train.AdamOptimizer(learning_rate=lr) update (Training.py:77) + global_step += 1.  variables: TF variable names
        to update, as minimize(loss, var_list=...) does (None = all); params, m and v of every other tensor stay as they are.

        clip_norm: tf.clip_by_global_norm(grads, clip_norm) first, the global norm taken over the updated variables' gradients
        (times grad_scale).  skip_nonfinite: when that norm is not finite, params, m and v are left as they are and
        skipped_steps grows by one (global_step still advances, as TF's does per sess.run).  With either set the global
        norm is returned (0-dim GPU tensor, no host sync); otherwise None.

        weight_decay: torch.optim.AdamW's decoupled decay, theta *= 1 - lr * weight_decay before the Adam step, on
        decay_variables (None = every conv kernel -- tensors of rank > 1 -- and no bias) among the updated variables.
        ema_decay: self.ema -= (1 - d_t) (self.ema - new theta) in the same pass (tf.train.ExponentialMovingAverage; the EMA
        arena starts as a copy of params); ema_warmup: d_t = min(ema_decay, (1 + step) / (10 + step)).  A skipped step
        leaves the EMA alone too.

        Every combination is one wun_optim_step call.  With the last four at their defaults params, m and v
        have the same bits as wun_adam_step / wun_adam_step_select / wun_adam_step_clip give: all of them run one kernel."""
        self._refuse_in_ema("adam_step")
        mask = self.select_mask(variables)
        wd = check_weight_decay(weight_decay) if weight_decay else 0.0
        if ema_warmup and ema_decay is None:
            raise ValueError("ema_warmup needs ema_decay")
        dmask = self.decay_mask(decay_variables) if wd or decay_variables is not None else None      # (no decay: no table)
        ema = None
        if ema_decay is not None:
            ema_decay = check_ema_decay(ema_decay)
            ema = self._ensure_ema()
        need_norm = clip_norm is not None or skip_nonfinite
        ws, skipped = self._norm_buffers() if need_norm else (None, None)
        cfg = _lib.WunOptimConfig(beta1, beta2, eps, wd, ema_decay if ema_decay is not None else 0.0,
                                  check_clip_norm(clip_norm),
                                  (_lib.WUN_CLIP_SKIP_NONFINITE if skip_nonfinite else 0) |
                                  (_lib.WUN_OPTIM_EMA_WARMUP if ema_warmup else 0))
        self.global_step += 1
        _lib.check(self._lib.wun_optim_step(
            self._active.handle, self.params.data_ptr(), self.grads.data_ptr(), self.adam_m.data_ptr(),
            self.adam_v.data_ptr(), ema.data_ptr() if ema is not None else None, self.global_step, lr, grad_scale,
            C.byref(cfg), ws.data_ptr() if ws is not None else None, skipped.data_ptr() if skipped is not None else None,
            self._stream(), *self._mask_arg(mask), *self._mask_arg(dmask)))
        self._step_phase = 0                    # (only once the update was accepted: a refused call leaves the gradients pending)
        return ws[len(self._active.tensors)].clone() if need_norm else None

    def _norm_buffers(self):
        """(norm workspace, int64 skip counter) of wun_grad_norm / wun_adam_step_clip, allocated on first use."""
        plan = self._active if self._active is not None else self._any_plan()
        self._ensure_variables(plan)
        n = int(self._lib.wun_grad_norm_workspace_floats(plan.handle))
        if self._norm_ws is None or self._norm_ws.numel() < n:
            self._norm_ws = torch.empty(n, dtype=torch.float32, device=self._dev())
        if self._skipped is None:
            self._skipped = torch.zeros(1, dtype=torch.int64, device=self._dev())
        return self._norm_ws, self._skipped

    def grad_norm(self, grad_scale=1.0, variables=None):
        """L2 norms of grad_scale * self.grads (wun_grad_norm): (global norm over `variables` -- tf.clip_by_global_norm's
        global_norm -- as a 0-dim GPU tensor, per-tensor norms [num_tensors] in variable-table order, 0 for a tensor not in
        `variables`).  None = every variable.  No host sync."""
        mask = self.select_mask(variables)
        ws, _ = self._norm_buffers()
        plan = self._active if self._active is not None else self._any_plan()
        nt = len(plan.tensors)
        _lib.check(self._lib.wun_grad_norm(plan.handle, self.grads.data_ptr(), grad_scale, ws.data_ptr(), self._stream(),
                                           *self._mask_arg(mask)))
        out = ws[:nt + 1].clone()
        return out[nt], out[:nt]

    @property
    def skipped_steps(self):
        """Adam steps skipped for a non-finite gradient norm (adam_step(skip_nonfinite=True)); reads the device counter."""
        return 0 if self._skipped is None else int(self._skipped.item())

    def activation(self, kind, index=0):
        """(tensor view [B, C, frames], t0, tstep) of a forward activation kept in the workspace of the last
        get_output(training=True): kind "dec" / "skip" (down level `index`), "bottleneck", "up" (up conv `index`);
        element j of a row is the post-activation conv output at position t0 + j * tstep (wun_plan_activation).
        After loss_and_gradients also "ups" (upsampled input of up conv `index`), "dz_up", "d_ups", "dz_skip", "dz_dec",
        "dz_bottleneck": the gradient tensors the backward pass left in the workspace (wun.h, kinds 4 - 9)."""
        info = _lib.WunActivationInfo()
        kinds = {"dec": 0, "skip": 1, "bottleneck": 2, "up": 3, "ups": 4, "dz_up": 5, "d_ups": 6, "dz_skip": 7, "dz_dec": 8,
                 "dz_bottleneck": 9}
        _lib.check(self._lib.wun_plan_activation(self._active.handle, kinds[kind], int(index), C.byref(info)))
        B = int(self._active.info.batch)
        ws = self._ws[self._last_key]
        if info.elem_bytes == 2:                                   # bf16 mode: activations live in HBM as bfloat16
            flat = ws[info.offset:].view(torch.bfloat16)[:B * info.batch_stride]
        else:
            flat = ws[info.offset:info.offset + B * info.batch_stride]
        view = flat.view(B, int(info.channels), int(info.pitch))[:, :, :int(info.frames)]
        return view, int(info.t0), int(info.tstep)

    def plan_info(self):
        return self._active.info if self._active is not None else None

    @property
    def effective_dtype(self):
        """'f32' or 'bf16': the arithmetic the active plan really runs (wun_plan_info.compute_dtype_effective) -- a config
        that asks for the bf16 mode without qualifying for it gets the exact-fp32 plan."""
        info = self.plan_info()
        if info is None:
            return None
        return "bf16" if int(info.compute_dtype_effective) == 1 else "f32"
