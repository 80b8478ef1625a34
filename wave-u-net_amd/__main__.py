"""Command line of the MI355X path, shaped like the reference's sacred CLIs
(`python Training.py with cfg.full_44KHz`, `python Predict.py with cfg.full_44KHz input_path=...`;
/root/reference/Training.py:153-166, Predict.py:1-17, Config.py:52-161):

  python -m wave_u_net_amd train   with cfg.baseline_stereo model_config.epoch_it=200 data_root=DATA
  python -m wave_u_net_amd train   with cfg.m1_context synthetic=1 experiment_id=7
  python -m wave_u_net_amd predict with cfg.full model_path=ckpt.npz input_path=mix.wav output_path=out
  python -m wave_u_net_amd test    with cfg.baseline model_path=ckpt.npz data_root=DATA partition=valid
  python -m wave_u_net_amd evaluate with cfg.full model_path=ckpt.npz data_root=DATA estimates_path=out partition=test
  python -m wave_u_net_amd predict with cfg.unet_spectrogram model_path=ckpt.npz input_path=mix.wav output_path=out
  python -m wave_u_net_amd test    with cfg.unet_spectrogram_l1 model_path=ckpt.npz data_root=DATA
  python -m wave_u_net_amd train   with cfg.unet_spectrogram_l1 data_root=DATA
      (the spectrogram U-Net baseline; `train` takes its magnitude objective, raw_audio_loss=False, on one GPU and refuses
       cfg.unet_spectrogram, whose audio output is built for inference only; hop_frames does not apply)
(model_path / load_model: a .npz of this package or a TensorFlow V2 checkpoint prefix such as checkpoints/full_44KHz/full_44KHz-236118)

`with` arguments: `cfg.<named config>` (any of wave_u_net_amd.NAMED_CONFIGS), `model_config.<key>=<value>`
overrides, and the command's own options as `<name>=<value>`.  data_root holds
train|valid|test/<track>/<source>.wav|.npy (+ optional mix.wav) at expected_sr, or at any rate with the option
`resample=1` (train, test).  `predict` takes a WAV at any rate and writes the estimates at that rate;
`hop_frames=<N|track>` makes its hops N output frames long / one hop over the whole track (default: num_frames).
`postfilter={"n_fft":2048,"hop":512,"power":2,"eps":1e-10}` (predict, evaluate; any subset of the keys, or model_config.postfilter=...)
masks the estimates against the mix's STFT before they are written / scored (postfilter.SoftMaskFilter);
`postfilter={"kind":"wiener","iterations":1,"em_eps":1e-10}` (with any of the keys above) is the multichannel Wiener filter instead
(postfilter.WienerFilter: EM iterations over the channels together; "kind":"softmask" is the default).
`"transform":"fft"` in either spec computes the transforms with an FFT and lifts n_fft's limit from 2048 to 8192
(`postfilter={"n_fft":4096,"hop":1024,"transform":"fft"}`).
`phase_iterations=N` (predict, evaluate; cfg.unet_spectrogram* only) refines the phase of the network's source magnitudes with N
Griffin-Lim iterations from the mix's phase (the reference's spectrogramToAudioFile, Utils.py:125-173) instead of keeping the mix's
phase; the refined audio is normalised by the window-square sum over the covering frames.  Absent or 0: the default audio output.
`overlap=0.25 shifts=4` (predict, evaluate; or model_config.separation={"overlap":0.25,"shifts":4}) lets neighbouring hops share a
quarter of a hop, cross-faded, and averages 4 passes whose hop grids are shifted by 0 .. max_shift frames (max_shift=<frames>,
default expected_sr // 2; shifts=[0,3,700] names the offsets): about shifts / (1 - overlap) times the forward passes.
`loudness=-23` (predict, evaluate; or `loudness={"target":-23,"max_gain_db":30,"peak_limit":0.99,"restore":True}`, with
`"true_peak_limit":-1` instead of peak_limit for a ceiling in dBTP on the oversampled peak, or
model_config.loudness=...) meters the mix at the model's rate (BS.1770-4 integrated loudness, on the GPU), scales it to that
many LUFS before the network and scales the estimates back; `model_config.loudness={"target":-23,"data":True}` makes `train` and
`test` scale every track's mix and stems by the gain of its mix when the tracks are loaded.
`train` takes the spectral objective as `model_config.spectral_loss={"resolutions":[[4096,1024]],"transform":"fft","terms":{"sc":1,
"log_mag_l1":1},"log_eps":4.0}`: `"transform":"fft"` lifts the loss's n_fft limit from 2048 to 8192 in the same way ("gemm" is the default).
`train` and `test` take `model_config.data_producer=fused` to produce their batches with one HIP kernel out of tracks resident in
HBM (datasets.FusedSnippetSource; the default "torch" keeps the torch-operator / host producers -- the batches are the same), and
`train` then takes `model_config.augment={"remix":0.5,"channel_swap":0.5,"polarity":0.5}` (any subset; probabilities) for the
source-level augmentations: stems remixed across songs, channels swapped, polarity inverted, per source; `"speed":p` plays a
snippet faster or slower, `"pitch_shift":p` transposes it at its tempo and `"time_stretch":p` changes its tempo in its key (a
phase vocoder on the GPU in front of the same kernel).
`train` takes `model_config.optimizer={"weight_decay":0.01,"ema_decay":0.999,"ema_warmup":True,"eval_with_ema":True}` (any subset:
decoupled weight decay on the conv kernels, an EMA of the weights kept in the checkpoint and scored by validation) and
`model_config.lr_schedule={"warmup_steps":1000,"kind":"cosine","total_steps":200000}`; `weights=ema` (predict, evaluate) then
separates with the checkpoint's EMA weights instead of the trained ones.
`evaluate` separates every track folder of data_root/<partition>, scores it on the GPU (BSS Eval v4: SDR / ISR / SIR / SAR per
1 s segment, bsseval.py), writes estimates and museval-style JSON under estimates_path and prints the median / MAD / mean / SD per
source.  Multi-GPU: launch `train` with `python -m torch.distributed.run --nproc-per-node N -m wave_u_net_amd train with ...`.
"""
import ast
import os
import random
import sys


def _parse(argv):
    if len(argv) < 1 or argv[0] not in ("train", "predict", "test", "evaluate"):
        raise SystemExit(__doc__)
    cmd, rest = argv[0], argv[1:]
    if rest and rest[0] == "with":
        rest = rest[1:]
    name, overrides, opts = "baseline", {}, {}
    for tok in rest:
        if tok.startswith("cfg."):
            name = tok[4:]
        elif "=" in tok:
            key, val = tok.split("=", 1)
            try:
                val = ast.literal_eval(val)
            except (ValueError, SyntaxError):
                pass
            if key.startswith("model_config."):
                overrides[key[len("model_config."):]] = val
            else:
                opts[key] = val
        else:
            raise SystemExit("cannot parse argument %r" % tok)
    return cmd, name, overrides, opts


def _postfilter(opts, model_config):
    """The postfilter= option, else model_config["postfilter"]: checked here, so that a bad spec ends the command at once."""
    from wave_u_net_amd.postfilter import from_config
    try:
        return from_config(opts.get("postfilter", model_config.get("postfilter")))
    except (ValueError, NotImplementedError, TypeError) as e:
        raise SystemExit("postfilter: %s" % e)


def _loudness(opts, model_config):
    """The loudness= option, else model_config["loudness"]: checked here, so that a bad spec ends the command at once."""
    from wave_u_net_amd.loudness import from_config
    try:
        return from_config(opts.get("loudness", model_config.get("loudness")))
    except (ValueError, TypeError) as e:
        raise SystemExit("loudness: %s" % e)


def _phase_iterations(opts):
    n = opts.get("phase_iterations", 0)
    if isinstance(n, bool) or not isinstance(n, int) or n < 0:
        raise SystemExit("phase_iterations must be an iteration count >= 0, got %r" % (n,))
    return n


def _weights(opts):
    """weights=trained|ema (predict, evaluate): checked here, so that a bad value ends the command at once."""
    from wave_u_net_amd.evaluate import WEIGHTS
    w = opts.get("weights")
    if w is not None and w not in WEIGHTS:
        raise SystemExit("weights must be one of %s, got %r" % (", ".join(WEIGHTS), w))
    return w


def _separation(opts, model_config):
    """overlap= / shifts= / max_shift=, else model_config["separation"]: checked here, so that a bad value ends the command at once."""
    from wave_u_net_amd.evaluate import blend_options, separation_options
    try:
        kw = separation_options(model_config, opts.get("overlap"), opts.get("shifts"), opts.get("max_shift"))
        blend_options(kw["overlap"], kw["shifts"], kw["max_shift"], model_config["expected_sr"])
    except (ValueError, TypeError) as e:
        raise SystemExit("overlap / shifts / max_shift: %s" % e)
    return kw


def main(argv=None):
    cmd, name, overrides, opts = _parse(sys.argv[1:] if argv is None else argv)
    import wave_u_net_amd as wun
    from wave_u_net_amd import training, validation, evaluate
    if name not in wun.NAMED_CONFIGS:
        raise SystemExit("unknown named config %r (have: %s)" % (name, ", ".join(sorted(wun.NAMED_CONFIGS))))
    model_config = wun.get_config(name, **overrides)

    if cmd == "train":
        experiment_id = opts.get("experiment_id", random.randint(0, 1000000))       # Config.py:5 (sacred seed-derived id)
        for d in (model_config["model_base_dir"], model_config["log_dir"]):         # Training.py:158-160
            os.makedirs(d, exist_ok=True)
        if opts.get("synthetic"):
            path = training.train(model_config, experiment_id, load_model=opts.get("load_model"))
            print("Saved model at " + str(path))
        elif opts.get("optimise", True) and "data_root" in opts:
            path, loss = validation.optimise(model_config, experiment_id, data_root=opts["data_root"],
                                             max_epochs=opts.get("max_epochs"), resample=bool(opts.get("resample", False)))
            print("Supervised training finished! Saved model at " + str(path) + ". Performance: " + str(loss))
        else:
            raise SystemExit("train needs data_root=<dir> or synthetic=1")
    elif cmd == "test":
        loss = validation.test(model_config, opts.get("partition", "test"), str(opts.get("experiment_id", "cli")),
                               opts.get("model_path"), data_root=opts["data_root"], resample=bool(opts.get("resample", False)))
        print("Finished testing - Mean MSE: " + str(loss))
    elif cmd == "evaluate":
        for need in ("data_root", "estimates_path"):
            if need not in opts:
                raise SystemExit("evaluate needs %s=<dir>" % need)
        folder = evaluate.produce_dataset_estimates(model_config, opts.get("model_path"), opts["data_root"],
                                                    opts["estimates_path"], partition=opts.get("partition", "test"),
                                                    postfilter=_postfilter(opts, model_config),
                                                    phase_iterations=_phase_iterations(opts), weights=_weights(opts),
                                                    loudness=_loudness(opts, model_config), **_separation(opts, model_config))
        for metric in ("SDR", "ISR", "SIR", "SAR"):
            stats = evaluate.compute_mean_metrics(folder, metric=metric)
            for src, (med, mad, mean, sd) in zip(model_config["source_names"], stats):
                print("%s %s: median %.3f MAD %.3f mean %.3f SD %.3f" % (src, metric, med, mad, mean, sd))
    else:
        if "input_path" not in opts:
            raise SystemExit("predict needs input_path=<mixture.wav>")
        hop = opts.get("hop_frames")                               # hop_frames=<N|track>: evaluate.separate_track's option
        if hop is not None and hop != "track" and (isinstance(hop, bool) or not isinstance(hop, int) or hop < 1):
            raise SystemExit("hop_frames must be a positive frame count or 'track', got %r" % (hop,))
        evaluate.produce_source_estimates(model_config, opts.get("model_path"), opts["input_path"], opts.get("output_path"),
                                          hop_frames=hop, postfilter=_postfilter(opts, model_config),
                                          phase_iterations=_phase_iterations(opts), weights=_weights(opts),
                                          loudness=_loudness(opts, model_config), **_separation(opts, model_config))


if __name__ == "__main__":
    main()
