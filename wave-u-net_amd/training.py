"""Training loop with the shape of the reference's Training.train
(/root/reference/Training.py:24-121): build the separator once, run `epoch_it` steps of
{forward, MSE loss, backward, Adam}, count global_step, return a checkpoint path.

The reference feeds the step from a tf.data pipeline over MUSDB (Datasets.py); here
`batch_source` is any callable returning (mix [B,Tin,C], targets [S,B,Tout,C]) GPU tensors
honouring that pipeline's output contract (float32, mix = sum of sources, targets
centre-cropped): datasets.DeviceSnippetSource for real tracks -- or datasets.FusedSnippetSource, the
same batches from one HIP kernel plus the remix / channel-swap / polarity augmentations, selected
by model_config["data_producer"] = "fused" and model_config["augment"] (validation._train_source)
-- and `synthetic_source` for the benchmark.
"""
import json
import math
import os
import time

import numpy as np
import torch
import torch.distributed as dist

from .parallel import GradAllReducer, OverlappedGradAllReducer, broadcast_parameters, init_distributed
from .checkpoint import load_checkpoint, save_checkpoint
from .separator import UnetAudioSeparator, check_clip_norm, check_ema_decay, check_weight_decay
from .spectral import SpectralLoss
from .waveform import CombinedLoss, WaveformLoss, TERMS as WAVEFORM_TERMS


def synthetic_source(model_config, batch, t_in, t_out, device, seed=1337):
    """Band-limited noise sources (9-tap moving average of U(-1,1)), mix = sum of sources,
    targets = centre crop (Utils.crop_sample, Utils.py:38-42).  Generated once on the GPU and
    reused, so the timed loop has its inputs resident in HBM."""
    S, C = len(model_config["source_names"]), 1 if model_config["mono_downmix"] else 2
    gen = torch.Generator(device="cpu").manual_seed(seed)
    srcs = []
    for _ in range(S):
        w = torch.rand((batch, C, t_in + 8), generator=gen) * 2 - 1
        sm = torch.nn.functional.avg_pool1d(w, 9, stride=1)
        sm = sm * ((0.9 / S) / sm.abs().max().clamp_min(1e-9))
        srcs.append(sm.permute(0, 2, 1).contiguous())
    src = torch.stack(srcs)                           # [S, B, Tin, C]
    mix = src.sum(0).to(device)
    pad = (t_in - t_out) // 2
    targets = src[:, :, pad:t_in - pad, :].contiguous().to(device) if pad > 0 else src.to(device)

    def source():
        return mix, targets
    return source


class Trainer(object):
    """One process per GPU.  step() = sess.run([separator_solver, ...]) of Training.py:105.

    grad_accum_steps = k (or model_config["grad_accum_steps"], default 1): each step runs k micro-batches of batch / k
    excerpts on a plan built for that size, the first overwriting the gradient arena and the rest adding to it
    (wun_loss_backward_accumulate), then one all-reduce and one Adam update on the summed gradient scaled by 1 / k.
    `batch` stays the per-rank batch of one optimizer step.

    clip_grad_norm / skip_nonfinite (or model_config["clip_grad_norm"] / ["skip_nonfinite_steps"], default off): each Adam
    update clips by the global norm of the gradient it applies -- after the all-reduce, times the all-reduce's scale / k, so
    every rank sees the same bits -- and skips the update when that norm is not finite (adam_step's clip_norm /
    skip_nonfinite).  Off: the plain update's bits.

    spectral_loss (or model_config["spectral_loss"], default None): a dict with `resolutions` [[n_fft, hop], ...], `weights`
    and `mse_weight`, or a spectral.SpectralLoss -- the step then minimises mse_weight * MSE + sum_j weight_j * (STFT-magnitude
    L1 at resolution j) (Training.py:55-60; wun_spectral_loss, then the backward pass from its gradient).  step() returns the
    total; last_losses holds [total, MSE, L_0, ...] of the step (device tensor, the mean over the micro-batches).  With
    `terms` (and `log_eps`, `sc_eps`) L_j is the weighted sum of mag_l1, log_mag_l1, sc and complex_l1 (wun_spectral_loss_terms,
    DESIGN.md 5.14), last_losses carries the per-term slots and train.jsonl a `spectral_terms` entry (term_parts).  With
    `"transform": "fft"` the loss's frame transforms are FFTs and n_fft may reach 8192 (`{"resolutions": [[4096, 1024]],
    "transform": "fft", ...}`); "gemm" is the default.  None: exactly the old calls.

    waveform_loss (or model_config["waveform_loss"], default None): a dict with `terms` {"mse" | "l1" | "si_sdr" | "snr": weight},
    `eps` and `zero_mean`, or a waveform.WaveformLoss (wun_waveform_loss).  Alone, the step minimises the
    waveform total -- nothing adds an MSE implicitly, ask for "mse"; with spectral_loss too, the sum of the two totals
    (waveform.CombinedLoss: the spectral entry writes d_outputs, the waveform entry adds to it).  last_waveform_losses holds
    [total, mse, l1, si_sdr, snr, SI-SDR dB per source, SNR dB per source] of the step (the mean over the micro-batches),
    waveform_parts() the weighted terms, train.jsonl a `waveform_terms` entry; last_losses, loss_parts() and term_parts() keep
    their spectral layout and meaning whenever a spectral loss is set.  Validation and early stopping stay the reference's MSE
    unless model_config["validation_metric"] says "si_sdr" (validation.test).

    optimizer (or model_config["optimizer"], default None): {"weight_decay": w, "decay_variables": [...] | None, "ema_decay": d,
    "ema_warmup": bool, "eval_with_ema": bool}, any subset -- decoupled weight decay (torch.optim.AdamW; None = every conv
    kernel, no bias), an EMA of the weights (sep.ema, tf.train.ExponentialMovingAverage; saved in the checkpoints) and
    validation on the EMA values, all in the one update kernel that clips and steps (wun_optim_step).
    lr_schedule (or model_config["lr_schedule"], default None): {"warmup_steps": n, "kind": "constant" | "cosine" | "step" |
    "exponential", "total_steps", "min_factor", "step_size", "gamma"}: each update's lr is float32(init_sup_sep_lr *
    lr_factor(schedule, sep.global_step)); last_lr holds it, train.jsonl gains `lr`.  Unknown keys and inconsistent values raise
    ValueError here.  Both None: exactly the old calls."""

    def __init__(self, model_config, batch_size=None, device=None, seed=1337, bucket_mib=16.0, grad_accum_steps=None,
                 clip_grad_norm=None, skip_nonfinite=None, spectral_loss=None, waveform_loss=None, optimizer=None,
                 lr_schedule=None):
        # (checked before anything touches the device: unknown keys and inconsistent values raise ValueError here)
        self.optimizer = optimizer_settings(optimizer if optimizer is not None else model_config.get("optimizer"))
        self.lr_schedule = schedule_settings(lr_schedule if lr_schedule is not None else model_config.get("lr_schedule"))
        self.rank, self.local_rank, self.world = init_distributed()
        # Scheduling hint of the plan (include/wun.h): low-priority side streams only when no collective shares the
        # device -- with a process group initialised (multi-GPU, or bench.py --force-allreduce) they must stay normal.
        if "exclusive_streams" not in model_config:
            model_config = dict(model_config)
            model_config["exclusive_streams"] = not (dist.is_available() and dist.is_initialized())
        self.cfg = model_config
        if device is None:
            device = "cuda:%d" % (self.local_rank % max(1, torch.cuda.device_count()))
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.sep = UnetAudioSeparator(model_config, device=self.device, seed=seed)
        self.batch = batch_size or model_config["batch_size"]
        k = grad_accum_steps if grad_accum_steps is not None else model_config.get("grad_accum_steps", 1)
        self.accum = int(k)
        if self.accum < 1 or self.batch % self.accum:
            raise ValueError("grad_accum_steps = %r must be >= 1 and divide the batch (%d)" % (k, self.batch))
        self.micro = self.batch // self.accum
        self.clip_norm, self.skip_nonfinite = clip_settings(model_config, clip_grad_norm, skip_nonfinite)
        self.spectral = SpectralLoss.from_config(spectral_loss if spectral_loss is not None
                                                 else model_config.get("spectral_loss"))
        self.waveform = WaveformLoss.from_config(waveform_loss if waveform_loss is not None
                                                 else model_config.get("waveform_loss"))
        if self.spectral is not None and self.waveform is not None:
            self._loss_kw = {"loss": CombinedLoss(self.spectral, self.waveform)}
        elif self.waveform is not None:
            self._loss_kw = {"loss": self.waveform}
        else:
            self._loss_kw = {"loss": self.spectral} if self.spectral is not None else {}
        self.last_losses = None
        self.last_waveform_losses = None
        self.grad_norm = None                  # global norm of the last clipped / checked update (0-dim GPU tensor)
        in_shape, out_shape = self.sep.get_padding(np.array([self.batch, model_config["num_frames"], 0]))
        self.t_in, self.t_out = int(in_shape[1]), int(out_shape[1])
        plan = self.sep._plan(self.micro, self.t_in)
        self.sep._active = plan
        self.sep._ensure_variables(plan)
        broadcast_parameters(self.sep.params)
        self.overlap = self.world > 1 and os.environ.get("WUN_NO_OVERLAP") is None
        if self.overlap:
            self.reducer = OverlappedGradAllReducer(plan.tensors, plan.info.arena_floats, bucket_mib,
                                                    device=self.device)
        else:
            self.reducer = GradAllReducer(plan.tensors, plan.info.arena_floats, bucket_mib)
        self.lr = model_config["init_sup_sep_lr"]
        self.last_lr = self.lr                 # the lr of the last optimizer step (the schedule's value when one is set)
        if self.optimizer is not None:
            self.sep.decay_mask(self.optimizer["decay_variables"])        # KeyError: not a variable of this separator
            if self.optimizer["ema_decay"] is not None:
                self.sep._ensure_ema()

    def tune(self, mix, targets, pinned_table=None):
        """One-off kernel autotuning on a real batch (skipped with WUN_NO_TUNE=1).  Rank 0 decides
        the tilings -- from `pinned_table` (the TEXT of a committed table: read-only, never written
        back), else from WUN_TUNE_CACHE=<file> (a writable cache) if either holds a table for this
        plan and library build, else by measuring (wun_plan_tune) -- and broadcasts the exported
        table; every rank imports that same table, so all replicas run bit-identical kernels
        (per-rank tuning would let replicas differ by fp32 rounding before the gradient all-reduce)
        and nobody reads a cache file that another rank is still writing.  The cache is written
        atomically.  `tune_source` records which of "pinned" / "cache" / "autotuned" / "heuristic"
        happened (decided by whether the import SUCCEEDED, not by comparing files afterwards)."""
        self.tune_source, self.tune_table = "heuristic", None
        if os.environ.get("WUN_NO_TUNE") is not None:
            return
        cache = os.environ.get("WUN_TUNE_CACHE")
        if self.accum > 1:                                # the plan runs micro-batches: tune on the first one
            mix, targets = self._micro_batch(mix, targets, 0)
        self.sep.get_output(mix, True)                    # makes this (batch, length) plan the active one
        table, source = None, None
        if self.rank == 0:
            if pinned_table:
                try:
                    self.sep.tune_import(pinned_table)
                    table, source = pinned_table, "pinned"
                except ValueError:
                    table = None                         # other plan / library build: fall through
            if table is None and cache and os.path.exists(cache):
                try:
                    text = open(cache).read()
                    self.sep.tune_import(text)
                    table, source = text, "cache"
                except ValueError:
                    table = None                         # other plan / library build / truncated: tune afresh
            if table is None:
                self.sep.tune(mix, targets)
                table, source = self.sep.tune_export(), "autotuned"
                if cache:
                    tmp = "%s.tmp.%d" % (cache, os.getpid())
                    with open(tmp, "w") as f:
                        f.write(table)
                    os.replace(tmp, cache)
        box = [table, source]
        if self.world > 1:
            dist.broadcast_object_list(box, src=0)
            if self.rank != 0:
                self.sep.tune_import(box[0])
        self.tune_table, self.tune_source = box[0], box[1]

    def _micro_batch(self, mix, targets, i):
        """Micro-batch i of a step's batch: excerpts [i b, (i + 1) b) -- dim 0 of mix, dim 1 of stacked targets."""
        lo, hi = i * self.micro, (i + 1) * self.micro
        if isinstance(targets, dict):
            return mix[lo:hi], {n: t[lo:hi] for n, t in targets.items()}
        return mix[lo:hi], targets[:, lo:hi]

    def step(self, mix, targets):
        if self.accum > 1:
            return self._accumulated_step(mix, targets)
        self.sep.get_output(mix, True)
        if self.overlap:
            # bucket events are recorded by the backward pass; the all-reduces wait on them
            loss = self.sep.loss_and_gradients(targets, *self.reducer.begin(), **self._loss_kw)
            self.reducer.launch(self.sep.grads)
            self.reducer.finish()
        else:
            loss = self.sep.loss_and_gradients(targets, **self._loss_kw)
            self.reducer.all_reduce(self.sep.grads)
        self._adam(self.reducer.grad_scale)
        if self._loss_kw:
            self._keep_losses(self.sep.last_losses)
        return loss

    def _keep_losses(self, losses):
        """losses of the step's loss object -> last_losses (the spectral loss's own layout) and last_waveform_losses."""
        if self.spectral is not None and self.waveform is not None:
            self.last_losses, self.last_waveform_losses = self._loss_kw["loss"].parts(losses)
        elif self.waveform is not None:
            self.last_waveform_losses = losses
        else:
            self.last_losses = losses

    @property
    def clipping(self):
        return self.clip_norm is not None or self.skip_nonfinite

    @property
    def logs_lr(self):
        """train.jsonl carries `lr` when a schedule or an optimizer dict is set, and only then."""
        return self.optimizer is not None or self.lr_schedule is not None

    def _adam(self, grad_scale):
        lr = self.lr
        if self.lr_schedule is not None:
            # keyed on the separator's global_step: carries across train() epochs and resumes from a checkpoint
            lr = scheduled_lr(self.lr, self.lr_schedule, self.sep.global_step)
        self.last_lr = lr
        kw = {}
        if self.optimizer is not None:
            kw = {k: self.optimizer[k] for k in ("weight_decay", "decay_variables", "ema_decay", "ema_warmup")}
        if self.clipping:
            self.grad_norm = self.sep.adam_step(lr, grad_scale=grad_scale, clip_norm=self.clip_norm,
                                                skip_nonfinite=self.skip_nonfinite, **kw)
        else:
            self.sep.adam_step(lr, grad_scale=grad_scale, **kw)

    def _accumulated_step(self, mix, targets):
        """k micro-batches, one optimizer step.  Only the last backward pass records the bucket events: an event then means
        "the SUM is final" and the overlapped all-reduce starts early as in the one-batch step.  Returns the mean of the
        micro-batch losses (0-dim GPU tensor, no host sync)."""
        if mix.shape[0] != self.batch:
            raise ValueError("step takes the whole batch: %d excerpts, got %d" % (self.batch, mix.shape[0]))
        k = self.accum
        losses, parts = [], []
        for i in range(k):
            m, t = self._micro_batch(mix, targets, i)
            self.sep.get_output(m, True)
            if self.overlap and i == k - 1:
                losses.append(self.sep.loss_and_gradients(t, *self.reducer.begin(), accumulate=i > 0, **self._loss_kw))
            else:
                losses.append(self.sep.loss_and_gradients(t, accumulate=i > 0, **self._loss_kw))
            if self._loss_kw:
                parts.append(self.sep.last_losses)
        if self.overlap:
            self.reducer.launch(self.sep.grads)
            self.reducer.finish()
        else:
            self.reducer.all_reduce(self.sep.grads)
        self._adam(self.reducer.grad_scale / k)
        if self._loss_kw:
            self._keep_losses(torch.stack(parts).mean(0))
        return torch.stack(losses).mean()

    def loss_parts(self):
        """(MSE, weighted sum of the spectral L1 terms) of the last step with a spectral loss, as floats (host sync)."""
        l = self.last_losses.tolist()
        return l[1], sum(w * x for w, x in zip(self.spectral.weights, l[2:]))

    def term_parts(self):
        """{term: sum_j weights[j] * termweight * term(j)} of the last step with a spectral loss built with terms= or mel= (the
        mel terms only with mel=; host sync):
        the parts of loss_parts()' second value."""
        sp = self.spectral
        per = {t: v.tolist() for t, v in sp.term_losses(self.last_losses).items()}
        return {t: sp.term_weight(t) * sum(w * x for w, x in zip(sp.weights, per[t])) for t in per}


    def waveform_parts(self):
        """{term: weight * term} of the last step with a waveform loss -- they sum to its total -- plus "si_sdr_db" and "snr_db":
        the per-source means in dB, higher is better (host sync)."""
        wv = self.waveform
        l = self.last_waveform_losses
        per = {t: v.item() for t, v in wv.term_losses(l).items()}
        parts = {t: wv.terms[t] * per[t] for t in WAVEFORM_TERMS}
        parts.update({k + "_db": v.tolist() for k, v in wv.source_metrics(l).items()})
        return parts


class SpectrogramTrainer(object):
    """The Trainer of the spectrogram U-Net on the magnitude objective (network "unet_spectrogram", raw_audio_loss=False:
    Jansson's L1, Training.py:55-63): step() = training forward on batch statistics with dropout, loss,
    backward, TF-Adam with the batch norms' moving averages.  One GPU; the options of the waveform model's Trainer that are
    not built for this network are refused here, by name."""
    spectral = waveform = None
    clipping = False
    rank, world = 0, 1

    def __init__(self, model_config, batch_size=None, device=None, seed=1337):
        from .spectrogram import UnetSpectrogramSeparator
        if model_config.get("raw_audio_loss", True):
            raise NotImplementedError("unet_spectrogram with raw_audio_loss=True: the spectrogram U-Net's audio output is built "
                                      "for inference only; train with raw_audio_loss=False (cfg.unet_spectrogram_l1)")
        for key, off in (("spectral_loss", None), ("waveform_loss", None), ("clip_grad_norm", None), ("grad_accum_steps", 1),
                         ("skip_nonfinite_steps", False), ("optimizer", None), ("lr_schedule", None)):
            if model_config.get(key, off) not in (off, None):
                raise NotImplementedError("unet_spectrogram: %s is not built for this network (its objective is the magnitude "
                                          "L1 of Training.py:55-63, one batch per step)" % key)
        if int(os.environ.get("WORLD_SIZE", "1")) > 1 or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            raise NotImplementedError("unet_spectrogram: data-parallel training (world > 1) is not built for this network")
        self.cfg = model_config
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        torch.cuda.set_device(self.device)
        self.sep = UnetSpectrogramSeparator(model_config, device=self.device, seed=seed)
        self.batch = batch_size or model_config["batch_size"]
        in_shape, out_shape = self.sep.get_padding(np.array([self.batch, model_config["num_frames"], 0]))
        self.t_in, self.t_out = int(in_shape[1]), int(out_shape[1])
        self.sep.frames(self.t_in)                         # a length the network cannot take is refused here
        self.sep._ensure_variables()
        self.lr = model_config["init_sup_sep_lr"]
        self.last_losses = None
        self.tune_source, self.tune_table = "heuristic", None

    def tune(self, mix, targets, pinned_table=None):
        """Nothing to tune: the 2-D kernels have one tiling."""

    def step(self, mix, targets):
        self.sep.get_output(mix, True, return_spectrogram=True)
        loss = self.sep.loss_and_gradients(targets)
        self.sep.adam_step(self.lr)
        self.last_losses = self.sep.last_losses
        return loss


OPTIMIZER_KEYS = ("weight_decay", "decay_variables", "ema_decay", "ema_warmup", "eval_with_ema")
SCHEDULE_KEYS = ("warmup_steps", "kind", "total_steps", "min_factor", "step_size", "gamma")
SCHEDULE_KINDS = ("constant", "cosine", "step", "exponential")


def optimizer_settings(optimizer):
    """model_config["optimizer"] / Trainer(optimizer=...) -> a checked copy with every key present, or None for None: the
    keyword arguments of UnetAudioSeparator.adam_step plus eval_with_ema (validation.test).  ValueError for an unknown key or
    an inconsistent value."""
    if optimizer is None:
        return None
    if not isinstance(optimizer, dict):
        raise ValueError("optimizer must be a dict or None, got %r" % (optimizer,))
    unknown = sorted(set(optimizer) - set(OPTIMIZER_KEYS))
    if unknown:
        raise ValueError("optimizer: unknown keys %s (known: %s)" % (unknown, list(OPTIMIZER_KEYS)))
    out = {"weight_decay": check_weight_decay(optimizer.get("weight_decay", 0.0)),
           "decay_variables": optimizer.get("decay_variables"),
           "ema_decay": optimizer.get("ema_decay"),
           "ema_warmup": optimizer.get("ema_warmup", False),
           "eval_with_ema": optimizer.get("eval_with_ema", False)}
    if out["ema_decay"] is not None:
        out["ema_decay"] = check_ema_decay(out["ema_decay"])
    for key in ("ema_warmup", "eval_with_ema"):
        if not isinstance(out[key], bool):
            raise ValueError("optimizer: %s = %r must be a bool" % (key, out[key]))
        if out[key] and out["ema_decay"] is None:
            raise ValueError("optimizer: %s needs ema_decay" % key)
    dv = out["decay_variables"]
    if dv is not None:
        if isinstance(dv, str) or not all(isinstance(n, str) for n in dv):
            raise ValueError("optimizer: decay_variables = %r must be a list of variable names or None" % (dv,))
        out["decay_variables"] = list(dv)
    return out


def schedule_settings(schedule):
    """model_config["lr_schedule"] -> a checked copy with every key present, or None for None (constant lr).  ValueError for
    an unknown key or an inconsistent value."""
    if schedule is None:
        return None
    if not isinstance(schedule, dict):
        raise ValueError("lr_schedule must be a dict or None, got %r" % (schedule,))
    unknown = sorted(set(schedule) - set(SCHEDULE_KEYS))
    if unknown:
        raise ValueError("lr_schedule: unknown keys %s (known: %s)" % (unknown, list(SCHEDULE_KEYS)))
    s = {"warmup_steps": schedule.get("warmup_steps", 0), "kind": schedule.get("kind", "constant"),
         "total_steps": schedule.get("total_steps"), "min_factor": schedule.get("min_factor", 0.0),
         "step_size": schedule.get("step_size"), "gamma": schedule.get("gamma")}
    if s["kind"] not in SCHEDULE_KINDS:
        raise ValueError("lr_schedule: kind = %r, expected one of %s" % (s["kind"], list(SCHEDULE_KINDS)))

    def integer(key, least):
        v = s[key]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < least:
            raise ValueError("lr_schedule: %s = %r must be an integer >= %d" % (key, v, least))
        s[key] = int(v)

    def number(key, lo, hi, lo_open):
        v = s[key]
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not (lo <= v <= hi) or (lo_open and v == lo):
            raise ValueError("lr_schedule: %s = %r must be a number in %s%g, %g]" % (key, v, "(" if lo_open else "[", lo, hi))
        s[key] = float(v)

    integer("warmup_steps", 0)
    needs = {"constant": (), "cosine": ("total_steps",), "step": ("step_size", "gamma"), "exponential": ("gamma",)}[s["kind"]]
    for key in ("total_steps", "step_size", "gamma"):
        if key not in needs and s[key] is not None:
            raise ValueError("lr_schedule: %s does not apply to kind %r" % (key, s["kind"]))
        if key in needs and s[key] is None:
            raise ValueError("lr_schedule: kind %r needs %s" % (s["kind"], key))
    if s["min_factor"] is None:
        s["min_factor"] = 0.0
    number("min_factor", 0.0, 1.0, False)
    if s["kind"] != "cosine" and s["min_factor"] != 0.0:           # (0: what a checked copy carries, so checking one again passes)
        raise ValueError("lr_schedule: min_factor does not apply to kind %r" % (s["kind"],))
    if s["kind"] == "cosine":
        integer("total_steps", 1)
        if s["total_steps"] <= s["warmup_steps"]:
            raise ValueError("lr_schedule: total_steps = %d must exceed warmup_steps = %d" % (s["total_steps"], s["warmup_steps"]))
    if s["kind"] == "step":
        integer("step_size", 1)
    if s["kind"] in ("step", "exponential"):
        number("gamma", 0.0, 1.0, True)
    return s


def lr_factor(schedule, global_step):
    """The factor on init_sup_sep_lr of the optimizer step taken at `global_step` (the separator's count BEFORE the step: 0 for
    the first one), in float64; a pure function of its arguments.  schedule: model_config["lr_schedule"] (None = 1).
      warm-up      steps 0 .. warmup_steps - 1: (step + 1) / warmup_steps, linear from 1 / warmup_steps to 1; it multiplies
                   nothing else: the kind starts at t = step - warmup_steps = 0 with factor 1
      constant     1
      cosine       min_factor + (1 - min_factor) (1 + cos(pi t / T)) / 2, T = total_steps - warmup_steps; min_factor from
                   step total_steps on
      step         gamma ** (t // step_size)
      exponential  gamma ** t"""
    s = schedule_settings(schedule)
    if s is None:
        return 1.0
    step = int(global_step)
    if step < 0:
        raise ValueError("global_step = %r must be >= 0" % (global_step,))
    w = s["warmup_steps"]
    if step < w:
        return (step + 1.0) / w
    t = step - w
    if s["kind"] == "cosine":
        T = s["total_steps"] - w
        if t >= T:
            return s["min_factor"]
        return s["min_factor"] + (1.0 - s["min_factor"]) * 0.5 * (1.0 + math.cos(math.pi * t / T))
    if s["kind"] == "step":
        return s["gamma"] ** (t // s["step_size"])
    if s["kind"] == "exponential":
        return s["gamma"] ** t
    return 1.0


def scheduled_lr(base_lr, schedule, global_step):
    """The lr of the step taken at global_step: float32(base_lr * lr_factor), the product in float64, as a Python float."""
    return float(np.float32(float(base_lr) * lr_factor(schedule, global_step)))


def clip_settings(model_config, clip_grad_norm=None, skip_nonfinite=None):
    """(clip_norm or None, skip_nonfinite) of a Trainer: the arguments, else model_config["clip_grad_norm"] /
    ["skip_nonfinite_steps"].  ValueError for a clip_grad_norm that is not > 0 (NaN included)."""
    clip = clip_grad_norm if clip_grad_norm is not None else model_config.get("clip_grad_norm")
    skip = skip_nonfinite if skip_nonfinite is not None else model_config.get("skip_nonfinite_steps", False)
    if clip is not None:
        try:
            clip = check_clip_norm(clip)
        except ValueError:
            raise ValueError("clip_grad_norm = %r must be a number > 0" % (clip,))
    return clip, bool(skip)


def train(model_config, experiment_id, load_model=None, batch_source=None, log_every=None):
    """Training.train(model_config, experiment_id, load_model=None) -> save_path
    (Training.py:24-25,121)."""
    if model_config["network"] not in ("unet", "unet_spectrogram"):
        raise NotImplementedError(model_config["network"])         # Training.py:28-33
    if log_every is None:
        log_every = 100 if model_config["epoch_it"] > 100 else 1
    # the spectrogram U-Net trains on the magnitude objective only (SpectrogramTrainer refuses raw_audio_loss=True)
    tr = SpectrogramTrainer(model_config) if model_config["network"] == "unet_spectrogram" else Trainer(model_config)
    if load_model is not None:
        # rank 0 reads the checkpoint (the only rank that is guaranteed to have the path: train()
        # hands save_path to every rank, but the file system need not be shared); parameters, both
        # Adam slots and global_step are then broadcast so every replica resumes the SAME state
        # (`.npz` of this package, or a TensorFlow V2 checkpoint prefix as the reference's Saver writes: checkpoint.py)
        # Whether an EMA is kept is the CONFIGURATION's word (the Trainer made the arena on every rank when it is), never the
        # file's: every rank then issues the same broadcasts.  A checkpoint's EMA that this run would not update is dropped,
        # with a warning, instead of being carried along stale into the next checkpoint.
        keeps_ema = bool(getattr(tr, "optimizer", None)) and tr.optimizer["ema_decay"] is not None
        if tr.rank == 0:
            load_checkpoint(tr.sep, load_model)
            if not keeps_ema and getattr(tr.sep, "ema", None) is not None:
                import warnings
                warnings.warn("wun: %s carries an EMA of the weights, but this run keeps none (no optimizer['ema_decay']): the "
                              "EMA is dropped and the checkpoints of this run will not contain one" % load_model, RuntimeWarning)
                tr.sep.ema = None
        if tr.world > 1:
            for t in (tr.sep.params, tr.sep.adam_m, tr.sep.adam_v) + ((tr.sep.ema,) if keeps_ema else ()):
                broadcast_parameters(t)
            box = [tr.sep.global_step]
            dist.broadcast_object_list(box, src=0)
            tr.sep.global_step = int(box[0])
    if batch_source is None:
        batch_source = synthetic_source(model_config, tr.batch, tr.t_in, tr.t_out, tr.device,
                                        seed=1337 + tr.rank)
    elif getattr(batch_source, "needs_trainer", False):
        batch_source = batch_source(tr)          # factory: needs the trainer's device / shapes / rank
    log_dir = os.path.join(model_config["log_dir"], str(experiment_id))
    if tr.rank == 0:
        os.makedirs(log_dir, exist_ok=True)
    log = open(os.path.join(log_dir, "train.jsonl"), "a") if tr.rank == 0 else None
    tr.tune(*batch_source())
    t0 = time.time()
    for it in range(model_config["epoch_it"]):                      # Training.py:103-109
        mix, targets = batch_source()
        loss = tr.step(mix, targets)
        if log is not None and (it % log_every == 0 or it == model_config["epoch_it"] - 1):
            line = {"global_step": tr.sep.global_step, "sep_loss": float(loss.item()), "elapsed_s": time.time() - t0}
            if tr.spectral is not None:
                line["mse_loss"], line["spectral_loss"] = tr.loss_parts()
                if tr.spectral.terms is not None:
                    line["spectral_terms"] = tr.term_parts()
            if tr.waveform is not None:
                line["waveform_terms"] = tr.waveform_parts()
            if tr.clipping:
                line["grad_norm"] = float(tr.grad_norm.item())
                line["skipped_steps"] = tr.sep.skipped_steps
            if getattr(tr, "logs_lr", False):
                line["lr"] = tr.last_lr
            log.write(json.dumps(line) + "\n")
            log.flush()
    torch.cuda.synchronize()
    save_path = None
    if tr.rank == 0:                                                # Training.py:113
        ckpt_dir = os.path.join(model_config["model_base_dir"], str(experiment_id))
        os.makedirs(ckpt_dir, exist_ok=True)
        # Training.py:113 saves "<dir>/<id>-<step>" with the V2 Saver; model_config["checkpoint_format"] = "tf" writes
        # exactly that (restorable by the reference), the default is this package's .npz
        if model_config.get("checkpoint_format", "npz") == "tf":
            save_path = save_checkpoint(tr.sep, os.path.join(ckpt_dir, "%s-%d" % (experiment_id, tr.sep.global_step)), "tf")
        else:
            save_path = save_checkpoint(tr.sep, os.path.join(ckpt_dir, "%s-%d.npz" % (experiment_id, tr.sep.global_step)))
        log.close()
    if tr.world > 1:
        # every rank returns the checkpoint path (Training.py:121 has one process; here the callers --
        # optimise()'s next epoch, test() -- run on all ranks and must agree on it)
        box = [save_path]
        dist.broadcast_object_list(box, src=0)
        save_path = box[0]
    return save_path
