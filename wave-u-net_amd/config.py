"""model_config handling: same keys, same named configs as the reference's sacred
ingredient (/root/reference/Config.py:4-161), as a plain dict (sacred is not needed)."""
import copy

BASE_MODEL_CONFIG = {            # Config.py:9-39
    "model_base_dir": "checkpoints",
    "log_dir": "logs",
    "batch_size": 16,
    "init_sup_sep_lr": 1e-4,
    "epoch_it": 2000,
    "cache_size": 4000,
    "num_workers": 4,
    "num_snippets_per_track": 100,
    "num_layers": 12,
    "filter_size": 15,
    "merge_filter_size": 5,
    "input_filter_size": 15,
    "output_filter_size": 1,
    "num_initial_filters": 24,
    "num_frames": 16384,
    "expected_sr": 22050,
    "mono_downmix": True,
    "output_type": "direct",
    "output_activation": "tanh",
    "context": False,
    "network": "unet",
    "upsampling": "linear",
    "task": "voice",
    "augmentation": True,
    "raw_audio_loss": True,
    "worse_epochs": 20,
}

# Keys the reference does not have, with the value a model_config without them means (read with .get(); BASE_MODEL_CONFIG
# stays the reference's dict, key by key).
EXTENSION_DEFAULTS = {
    "grad_accum_steps": 1,            # training.Trainer: micro-batches per optimizer step
    "clip_grad_norm": None,           # training.Trainer: tf.clip_by_global_norm threshold
    "skip_nonfinite_steps": False,    # training.Trainer: skip an update whose gradient norm is not finite
    "checkpoint_format": "npz",       # training.train: "npz" or "tf"
    # training.Trainer: None = the reference's TF-Adam; else {"weight_decay": w, "decay_variables": [...] | None,
    # "ema_decay": d, "ema_warmup": bool, "eval_with_ema": bool} (any subset): decoupled weight decay (AdamW; None = every conv
    # kernel, no bias), an EMA of the weights kept in the checkpoints, and validation / early stopping on the EMA values
    "optimizer": None,
    # training.Trainer / training.lr_factor: None = constant init_sup_sep_lr; else {"warmup_steps": n, "kind": "constant" |
    # "cosine" | "step" | "exponential", "total_steps", "min_factor", "step_size", "gamma"}: the factor on the lr per global_step
    "lr_schedule": None,
    # training.Trainer / spectral.SpectralLoss: None = the reference's MSE; else {"resolutions": [[n_fft, hop], ...],
    # "weights": [...], "mse_weight": w}: the objective becomes w * MSE + sum_j weight_j * STFT-magnitude L1 (Training.py:55-60);
    # with "terms": {"mag_l1" | "log_mag_l1" | "sc" | "complex_l1": weight} (and "log_eps", "sc_eps") the multi-resolution STFT loss;
    # "transform": "gemm" (default, n_fft up to 2048) or "fft" (up to 8192: {"resolutions": [[4096, 1024]], "transform": "fft"})
    "spectral_loss": None,
    # training.Trainer / waveform.WaveformLoss: None, or {"terms": {"mse" | "l1" | "si_sdr" | "snr": weight}, "eps": 1e-8,
    # "zero_mean": True}: the step minimises the weighted sum of those terms (nothing adds an MSE implicitly); with
    # "spectral_loss" too, the sum of the two totals (waveform.CombinedLoss)
    "waveform_loss": None,
    # validation.test: "mse" (the reference's) or "si_sdr": minus the mean SI-SDR in dB, so that lower is still better
    "validation_metric": "mse",
    # evaluate.separate_track / postfilter.SoftMaskFilter: None = the estimates as the network gives them; else
    # {"n_fft": 2048, "hop": 512, "power": 2, "eps": 1e-10} (any subset): the soft-mask filter against the mix's STFT; with
    # "kind": "wiener" (and "iterations": 1, "em_eps": 1e-10) postfilter.WienerFilter, the multichannel Wiener filter
    # "transform": "fft" computes the transforms with an FFT: n_fft up to 8192 instead of 2048
    "postfilter": None,
    # evaluate.separate_track (through produce_source_estimates / evaluate_track / produce_dataset_estimates): None = disjoint
    # hops, one pass; else {"overlap": 0.25, "shifts": 4, "max_shift": 11025} (any subset): neighbouring hops share that
    # fraction of a hop and are cross-faded, and the hop grid is run at that many shifted offsets and averaged
    "separation": None,
    # evaluate.separate_track (through the same callers) / loudness.from_config: None = the mix at the level it
    # arrives; else a target in LUFS or {"target": -23.0, "max_gain_db": 30.0, "peak_limit": None, "restore": True,
    # "data": False} (any subset): the resampled mix is metered (BS.1770-4 integrated loudness) and scaled to the target before
    # the network, the estimates scaled back unless "restore" is False; "data": True makes train / test scale every track's mix
    # and stems by the gain of its mix at load (datasets.normalize_tracks); one more key, "true_peak_limit" (dBTP, e.g. -1.0,
    # instead of "peak_limit"), meters with loudness.r128 and keeps the TRUE peak of the scaled mix under it
    "loudness": None,
    # spectrogram.UnetSpectrogramSeparator: the STFT framing of the spectrogram U-Net (UnetSpectrogramSeparator.py:28-29 fixes
    # 1024 / 768); other values exist so that tests can run small geometries
    "spec_frame_len": 1024,
    "spec_hop": 768,
    # its training step: tf.layers.dropout's rate on the three deepest concatenations (0 = none), the decay of
    # tf.contrib.layers.batch_norm's moving averages; "spec_dropout_seed" (default: the separator's seed) keys the keep bits
    "spec_dropout": 0.5,
    "spec_bn_decay": 0.999,
}

NAMED_CONFIGS = {                # Config.py:52-161
    "baseline": {},
    "baseline_diff": {"output_type": "difference"},
    "baseline_context": {"output_type": "difference", "context": True},
    "baseline_stereo": {"output_type": "difference", "context": True, "mono_downmix": False},
    "full": {"output_type": "difference", "context": True, "upsampling": "learned",
             "mono_downmix": False},
    "full_44KHz": {"output_type": "difference", "context": True, "upsampling": "learned",
                   "mono_downmix": False, "expected_sr": 44100},
    "baseline_context_smallfilter_deep": {"output_type": "difference", "context": True,
                                          "num_layers": 14, "duration": 7, "filter_size": 5,
                                          "merge_filter_size": 1},
    "full_multi_instrument": {"output_type": "difference", "context": True,
                              "upsampling": "linear", "mono_downmix": False,
                              "task": "multi_instrument"},
    "baseline_comparison": {"batch_size": 4, "output_type": "difference", "context": True,
                            "num_frames": 768 * 127 + 1024, "duration": 13,
                            "expected_sr": 8192, "num_initial_filters": 34},   # Config.py:123-134
    # the spectrogram U-Net baseline (spectrogram.UnetSpectrogramSeparator; training: the _l1 objective)
    "unet_spectrogram": {"batch_size": 4, "network": "unet_spectrogram", "num_layers": 6, "expected_sr": 8192,
                         "num_frames": 768 * 127 + 1024, "duration": 13, "num_initial_filters": 16},     # Config.py:136-147
    "unet_spectrogram_l1": {"batch_size": 4, "network": "unet_spectrogram", "num_layers": 6, "expected_sr": 8192,
                            "num_frames": 768 * 127 + 1024, "duration": 13, "num_initial_filters": 16,
                            "raw_audio_loss": False},                                                    # Config.py:149-161
    # BASELINE.json configs[1]: the M1 architecture run with input context (~147k samples in)
    "m1_context": {"context": True},
    # BASELINE.json configs[4]: 16 levels / 48 base channels, stereo, 4 sources, same padding,
    # 589 824-sample excerpts (9 * 2^16; a 16-level context model would need >= 2.1 M input samples)
    "deep_l16_f48": {"num_layers": 16, "num_initial_filters": 48, "mono_downmix": False,
                     "task": "multi_instrument", "output_type": "difference", "num_frames": 589824},
}


def finalize(model_config):
    """Derived keys (Config.py:42-50)."""
    cfg = dict(model_config)
    if cfg["task"] == "multi_instrument":
        cfg.setdefault("source_names", ["bass", "drums", "other", "vocals"])
    elif cfg["task"] == "voice":
        cfg.setdefault("source_names", ["accompaniment", "vocals"])
    else:
        raise NotImplementedError(cfg["task"])
    cfg["num_sources"] = len(cfg["source_names"])
    cfg["num_channels"] = 1 if cfg["mono_downmix"] else 2
    return cfg


def get_config(name="baseline", **overrides):
    cfg = copy.deepcopy(BASE_MODEL_CONFIG)
    cfg.update(NAMED_CONFIGS[name])
    cfg.update(overrides)
    return finalize(cfg)
