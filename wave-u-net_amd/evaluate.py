"""Tiled full-track inference: the reference's Evaluate.predict_track
(/root/reference/Evaluate.py:82-145) around the MI355X forward pass.

Semantics kept exactly: mono downmix or mono->stereo duplication (:98-104), zero padding of short
inputs (:108-113), symmetric context padding of (input_frames - output_frames)//2 (:121-122),
hops of `output_frames` with the LAST hop re-aligned to the end of the track (:125-128), removal of
the extra padding (:141-143).  MI355X-first difference: hops are evaluated `batch_hops` at a time in
one get_output call instead of one sess.run per hop (identical results, far fewer launches).
predict_track takes audio that is already at model_config["expected_sr"] and tiles on the host.
separate_track is the whole of Evaluate.predict (:59-80) for a file at ANY rate, on the device the separator lives on:
downmix + resampling + context padding in one kernel (resample.py, wun_resample), the hop loop in one C call
(wun_separate_track: windows gathered from the track by the forward's first kernel, estimates scattered by one kernel
per chunk), resampling back + trim + channel duplication in one kernel per source, one upload and one download per track.
hop_frames lets a hop be longer than the reference's num_frames, up to the whole track.  overlap / shifts blend overlapping hops
and several shifted passes into one weighted mean per output frame (blend.py, wun_separate_track_blend).
"""
import numpy as np
import torch


def predict_track(model_config, separator, mix_audio, mix_sr=None, batch_hops=16):
    """mix_audio: [n_frames, n_channels] float array.  Returns {source_name: float32 [n_frames, C]}."""
    mix_audio = np.asarray(mix_audio, dtype=np.float32)
    assert mix_audio.ndim == 2                                                   # Evaluate.py:97
    if mix_sr is not None and int(mix_sr) != int(model_config["expected_sr"]):
        raise NotImplementedError("resampling is not part of the hot path; provide audio at expected_sr")
    if model_config["mono_downmix"]:
        mix_audio = np.mean(mix_audio, axis=1, keepdims=True)                    # :98-99
    elif mix_audio.shape[1] == 1:
        mix_audio = np.tile(mix_audio, [1, 2])                                   # :101-102

    in_shape, out_shape = separator.get_padding(np.array([1, model_config["num_frames"], 0]))
    input_frames, output_frames = int(in_shape[1]), int(out_shape[1])

    if mix_audio.shape[0] < input_frames:                                        # :108-113
        extra_pad = input_frames - mix_audio.shape[0]
        mix_audio = np.pad(mix_audio, [(0, extra_pad), (0, 0)], mode="constant")
    else:
        extra_pad = 0
    n_frames = mix_audio.shape[0]
    names = list(model_config["source_names"])
    preds = {n: np.zeros(mix_audio.shape, np.float32) for n in names}           # :117

    pad = (input_frames - output_frames) // 2                                    # :121
    padded = np.pad(mix_audio, [(pad, pad), (0, 0)], mode="constant")

    positions = []
    for pos in range(0, n_frames, output_frames):                                # :125-128
        if pos + output_frames > n_frames:
            pos = n_frames - output_frames
        positions.append(pos)

    for k in range(0, len(positions), batch_hops):
        chunk = positions[k:k + batch_hops]
        batch = np.stack([padded[p:p + input_frames, :] for p in chunk])
        outs = separator.get_output(batch, False)                                # training=False: AudioClip active
        for n in names:
            o = outs[n]
            o = o.detach().cpu().numpy() if torch.is_tensor(o) else np.asarray(o)
            for bi, p in enumerate(chunk):
                preds[n][p:p + output_frames] = o[bi]                            # :139
    if extra_pad > 0:                                                            # :141-143
        preds = {n: v[:-extra_pad, :] for n, v in preds.items()}
    return preds


def _hop_positions(n_frames, output_frames):
    positions = []
    for pos in range(0, n_frames, output_frames):                                # Evaluate.py:125-128
        if pos + output_frames > n_frames:
            pos = n_frames - output_frames
        positions.append(pos)
    return positions


def hop_geometry(model_config, separator, n_res, hop_frames=None):
    """(input_frames, output_frames) of one hop.  hop_frames None: get_padding of model_config["num_frames"], the
    reference's hop; an int N: get_padding([1, N, 0]); "track": get_padding of the whole n_res-frame track, one hop.
    For same-padding models N / the track length is first rounded up to a multiple of 2 ** num_layers."""
    if hop_frames is None:
        want = int(model_config["num_frames"])
    elif hop_frames == "track":
        want = max(int(n_res), 1)
    else:
        want = int(hop_frames)
        if isinstance(hop_frames, bool) or want < 1:
            raise ValueError("hop_frames = %r must be a positive frame count, 'track' or None" % (hop_frames,))
    if hop_frames is not None and not model_config["context"]:
        m = 2 ** int(model_config["num_layers"])             # same padding: the length must halve num_layers times
        want = -(-want // m) * m                              # (UnetAudioSeparator.py:121 asserts it)
    in_shape, out_shape = separator.get_padding(np.array([1, want, 0]))
    return int(in_shape[1]), int(out_shape[1])


def budget_batch_hops(separator, batch_hops, n_hops, input_frames, default_input_frames, workspace_bytes=None):
    """Hops per forward pass of a long-hop plan: the largest b <= min(batch_hops, n_hops) with
    b * 4 * workspace_floats(1, input_frames) <= workspace_bytes, at least 1 (one hop cannot be split).  workspace_bytes
    None: 4 * workspace_floats(batch_hops, default_input_frames), the workspace the default tiling takes at batch_hops.
    Both figures are wun_plan_query's (separator.workspace_floats); a separator without that method is not limited."""
    b = max(1, min(int(batch_hops), int(n_hops)))
    query = getattr(separator, "workspace_floats", None)
    if query is None:
        return b
    if workspace_bytes is None:
        workspace_bytes = 4 * query(int(batch_hops), default_input_frames)
    per_hop = 4 * query(1, input_frames)
    return max(1, min(b, int(workspace_bytes) // per_hop))


def blend_options(overlap, shifts, max_shift, expected_sr):
    """separate_track's overlap / shifts / max_shift checked and resolved: (overlap as a float, the list of shift offsets).
    shifts None, 0 or 1: [0]; an int N: blend.shift_offsets(N, max_shift), max_shift defaulting to expected_sr // 2; a list:
    its non-negative frame offsets.  ValueError for anything out of range."""
    from . import blend
    if isinstance(overlap, bool) or not isinstance(overlap, (int, float)) or not 0.0 <= float(overlap) < 1.0:
        raise ValueError("overlap = %r must be a fraction of the hop in [0, 1)" % (overlap,))
    if shifts is None:
        offsets = [0]
    elif isinstance(shifts, bool):
        raise ValueError("shifts = %r must be a count or a list of frame offsets" % (shifts,))
    elif isinstance(shifts, (int, np.integer)):
        if shifts < 0:
            raise ValueError("shifts = %d must be >= 0" % shifts)
        if max_shift is None:
            max_shift = int(expected_sr) // 2
        if isinstance(max_shift, bool) or not isinstance(max_shift, (int, np.integer)) or max_shift < 0:
            raise ValueError("max_shift = %r must be a frame count >= 0" % (max_shift,))
        offsets = blend.shift_offsets(shifts, max_shift) if shifts > 1 else [0]
    else:
        offsets = list(shifts)
        if not offsets or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0 for v in offsets):
            raise ValueError("shifts = %r must be a non-empty list of frame offsets >= 0" % (shifts,))
        offsets = [int(v) for v in offsets]
    return float(overlap), offsets


def separate_track(model_config, separator, mix_audio, mix_sr, batch_hops=16, hop_frames=None, workspace_bytes=None,
                   return_device=False, postfilter=None, phase_iterations=0, overlap=0.0, shifts=None, max_shift=None,
                   loudness=None, loudness_probe=None):
    """Evaluate.predict (Evaluate.py:59-80) around predict_track (:82-145) for audio at any sample rate, without the
    host in the loop.  mix_audio: [n_frames, n_channels] float array or tensor at mix_sr Hz.  Returns {source_name: float32
    numpy [n_frames, channels]} at mix_sr: channels is the input's count, except that a stereo model on a mono file
    gives its two channels, as the reference does.

    Everything between the upload of mix_audio and the download of the estimates runs on `separator.device`: the hop
    windows are read from the padded track and the estimates written into the track-long result by the library (one
    wun_separate_track call when the hops divide into whole chunks, see below) -- no stacked batch, no per-source copies.  (A separator without a device -- a numpy
    stand-in -- runs the same steps on CPU tensors through get_output.)

    hop_frames=None (default): the reference's hops -- same hop positions, chunking and plans as predict_track: at
    mix_sr == expected_sr the estimates are bit-identical to predict_track's (tiled to the input's channels for a mono
    model).  The kernels' split choices depend on a plan's batch, so a last chunk shorter than batch_hops runs on the plan
    of ITS batch, as predict_track's does (chunk by chunk through wun_forward_windows / wun_scatter_windows, the two
    halves of wun_separate_track); every other track is the one call.

    hop_frames=N / "track": hops of get_padding([1, N, 0]) output frames / one hop over the whole resampled track.  A
    context model pays its context (input - output frames) once per hop, so long hops convolve far fewer samples per
    output sample (M1 + context: 9.0 at the default hop, 1.8 at 10 hops' length).  What comes out is the reference's own
    output for a config with that num_frames -- the same network on another alignment of the hop grid -- NOT the output
    of the default tiling: the decimating levels sample other positions, so the two differ as two tilings of the reference
    differ.  For same-padding models a long hop also moves the zero-padded hop edges (fewer of them, elsewhere).  Short
    tracks are zero-padded to one hop's OUTPUT (the default pads to its input, Evaluate.py:108-113).  batch_hops is
    lowered until batch_hops * workspace_floats of the long plan fits workspace_bytes (budget_batch_hops; default: the
    workspace of the default tiling at batch_hops, from wun_plan_query); a last chunk runs on the same plan with zero rows.

    return_device=True: no download -- the float32 tensor [S, n_frames, channels] on the separator's device, sources in
    source_names order (what evaluate_track scores where it lies).

    postfilter (a postfilter.SoftMaskFilter or WienerFilter, or the spec postfilter.from_config takes; default None: no
    filter, today's path): the soft-mask filter, or with {"kind": "wiener", ...} the multichannel Wiener filter, applied at
    the model's rate to the estimates and the resampled mix before the resampling back -- the estimates then share the
    mix's phase and sum to it.

    phase_iterations=N > 0 (network "unet_spectrogram" only; NotImplementedError on the waveform network, whose own magnitudes
    with its own phase are already consistent): every hop's source magnitudes (get_output(.., return_spectrogram=True)) go
    through N Griffin-Lim iterations from the mix's phase (separator.reconstruct, the reference's spectrogramToAudioFile with
    phase=mix_phase) instead of keeping the mix's phase as it is.  The refined audio is normalised by
    wun_istft's window-square sum over the covering frames, not by inverse_stft_window_fn: it differs from the default audio
    output at a hop's edges even before the phase moves.  0 (default) is exactly the path and the bits without the option.

    overlap (a fraction of the hop's output, 0 <= overlap < 1) and shifts (a count N of passes at blend.shift_offsets(N,
    max_shift), max_shift defaulting to expected_sr // 2, or a list of frame offsets at the model's rate): neighbouring
    hops share V = round(overlap * output_frames) frames and are cross-faded over them with a trapezoid, and the hop grid
    is run once per shift, each pass moved back by its offset; every output frame is ONE weighted mean over every window of
    every pass that covers it (blend.py).  The last hop of a pass is not re-aligned: it hangs over the
    track's end and reads zeros there.  The waveform network runs the whole loop in one wun_separate_track_blend call on
    one plan with batch min(batch_hops, windows); any other separator goes chunk by chunk through get_output and
    blend.blend_windows (the same kernel on a device, its restatement on CPU tensors).  About nshifts / (1 - overlap) times
    the forward passes of the plain path; no quality gain is measured or claimed.  overlap == 0 with shifts None, 0, 1 or
    [0] is exactly the path and the bits without the options.

    loudness (a target in LUFS or the spec loudness.from_config takes; default None: the mix at the level it arrives, today's
    path and bits): the n_res frames the network will see are metered at expected_sr with the model's channel count (BS.1770-4
    integrated loudness, loudness.integrated), the gain to the target is computed on the device (loudness.gain) and those
    frames are scaled in place; after the resampling back the estimates are scaled by the reciprocal factor in one launch
    unless the spec's "restore" is False.  A post-filter sees the scaled mix and the scaled estimates.  No value is read on
    the host.  With the spec's "true_peak_limit" (dBTP) the meter is loudness.r128 and the gain is capped so that the TRUE peak
    of the scaled frames stays under it; without the key nothing new is called.  GPU separators only.  loudness_probe (a dict, for tests and tools) receives "meter" and "gain" (the device
    tensors) and "padded" (the scaled track the network read, with its context padding)."""
    from . import resample as rs
    loud = None
    if loudness is not None:
        from . import loudness as ld
        loud = ld.from_config(loudness)
    overlap, offsets = blend_options(overlap, shifts, max_shift, model_config["expected_sr"])
    blended = overlap != 0.0 or offsets != [0]
    phase_iterations = int(phase_iterations)
    if phase_iterations < 0:
        raise ValueError("phase_iterations must be >= 0, got %d" % phase_iterations)
    if phase_iterations and model_config.get("network") != "unet_spectrogram":
        raise NotImplementedError("phase_iterations: Griffin-Lim refines the magnitudes of the spectrogram U-Net "
                                  "(network 'unet_spectrogram'); the waveform network has no magnitude output")
    if model_config.get("network") == "unet_spectrogram" and hop_frames is not None:
        raise NotImplementedError("hop_frames: the spectrogram U-Net separates in hops of num_frames only (its frame count is "
                                  "tied to num_layers); the plan-based long hops are Wave-U-Net only")
    if postfilter is not None:
        from .postfilter import from_config
        postfilter = from_config(postfilter)
    device = torch.device(getattr(separator, "device", None) or "cpu")
    if loud is not None and device.type != "cuda":
        raise RuntimeError("loudness: the meter runs on a GPU; there is no CPU fallback (separator on %s)" % device)
    x = mix_audio if torch.is_tensor(mix_audio) else torch.from_numpy(np.ascontiguousarray(np.asarray(mix_audio, dtype=np.float32)))
    assert x.dim() == 2                                                          # Evaluate.py:97
    x = x.to(device=device, dtype=torch.float32).contiguous()                    # the one upload
    n_in, ch = int(x.shape[0]), int(x.shape[1])
    C = 1 if model_config["mono_downmix"] else max(ch, 2)                        # :98-102
    up, down = rs.ratio(mix_sr, model_config["expected_sr"])
    n_res = rs.frames(n_in, up, down)

    input_frames, output_frames = hop_geometry(model_config, separator, n_res, hop_frames)
    # :108-113 (short inputs: zeros behind)
    n_frames = max(n_res, input_frames if hop_frames is None else output_frames)
    pad = (input_frames - output_frames) // 2                                    # :121-122
    lead, table = 0, None
    track_frames = n_frames + 2 * pad
    if blended:
        from . import blend
        v_frames = min(int(round(overlap * output_frames)), output_frames - 1)
        table = blend.window_table(output_frames, n_frames, v_frames, offsets)
        lead = max(offsets)                                                      # the first window of a pass starts at -shift
        track_frames = max(track_frames + lead, lead + int(table[:, 0].max()) + input_frames)   # ... its last one overhangs
    padded = torch.zeros((track_frames, C), dtype=torch.float32, device=device)
    rs.resample_into(x, padded, lead + pad, n_res, up, down)                     # downmix / duplicate, resample, pad
    gain = None
    if loud is not None:
        seen = padded[lead + pad:lead + pad + n_res]                             # what the network will see of the file
        meter, limit = ld.meter_for(seen, int(model_config["expected_sr"]), loud)     # true_peak_limit: r128, else integrated
        gain = ld.gain(meter, loud["target"], loud["max_gain_db"], limit)
        ld.scale_(seen, gain[0:1])
        if loudness_probe is not None:
            loudness_probe.update(meter=meter, gain=gain, padded=padded, offset=lead + pad, frames=n_res)

    names = list(model_config["source_names"])
    positions = _hop_positions(n_frames, output_frames) if table is None else table[:, 0].tolist()
    if hop_frames is not None:
        batch_hops = budget_batch_hops(separator, batch_hops, len(positions), input_frames,
                                       hop_geometry(model_config, separator, n_res)[0], workspace_bytes)
    if table is not None:
        if device.type != "cpu" and hasattr(separator, "separate_padded_blend"):
            preds = torch.empty((len(names), n_frames, C), dtype=torch.float32, device=device)
            separator.separate_padded_blend(padded, n_frames, min(batch_hops, len(positions)), v_frames, offsets, lead,
                                            frames=input_frames, out=preds)
        else:
            preds = _separate_blend_chunks(separator, padded, table, lead, v_frames, batch_hops, input_frames, names,
                                           n_frames, C, phase_iterations)
    elif device.type != "cpu" and hasattr(separator, "separate_padded"):
        preds = torch.empty((len(names), n_frames, C), dtype=torch.float32, device=device)   # every frame is written
        batch = min(batch_hops, len(positions))
        if hop_frames is not None or len(positions) % batch == 0:
            separator.separate_padded(padded, n_frames, batch, frames=input_frames, out=preds)
        else:
            for k in range(0, len(positions), batch):                            # the last chunk on the plan of its batch
                chunk = positions[k:k + batch]
                separator.get_output_windows(padded, chunk, False, frames=input_frames)
                separator.scatter_windows(chunk, preds, frames=input_frames)
    else:
        preds = _separate_cpu(separator, padded, positions, batch_hops, input_frames, output_frames, names, n_frames, C,
                              phase_iterations)

    if postfilter is not None:                                                   # at the model's rate, without extra_pad
        preds = postfilter.apply(padded[lead + pad:lead + pad + n_res], preds[:, :n_res])

    # back to mix_sr, cut to the input's length, mono estimates duplicated to the input's channels (:64-67)
    c_out = ch if (C == 1 and ch > 1) else C
    c_fused = c_out if c_out <= 2 else C
    n_back = min(rs.frames(n_res, down, up), n_in)
    out = torch.empty((len(names), n_back, c_fused), dtype=torch.float32, device=device)
    for si in range(len(names)):
        rs.resample_into(preds[si, :n_res], out[si], 0, n_back, down, up)        # [:n_res] drops extra_pad (:141-143)
    if gain is not None and loud["restore"]:
        ld.scale_(out, gain[1:2])                                                # back to the file's level
    if c_fused != c_out:
        out = out.repeat(1, 1, c_out)
    if return_device:
        return out
    host = out.cpu().numpy()                                                     # the one download
    return {n: host[si] for si, n in enumerate(names)}


def _separate_cpu(separator, padded, positions, batch_hops, input_frames, output_frames, names, n_frames, C, phase_iterations=0):
    """The hop loop on CPU tensors through separator.get_output (numpy stand-ins).  phase_iterations > 0: the hop's magnitudes
    through separator.reconstruct instead of its audio output."""
    device = padded.device
    preds = torch.zeros((len(names), n_frames, C), dtype=torch.float32, device=device)   # :117
    for k in range(0, len(positions), batch_hops):
        chunk = positions[k:k + batch_hops]
        batch = torch.stack([padded[p:p + input_frames] for p in chunk])         # strided views -> [B, Tin, C]
        if phase_iterations:
            mags = separator.get_output(batch, False, return_spectrogram=True)
            outs = separator.reconstruct(mags, batch, phase_iterations)
        else:
            outs = separator.get_output(batch if device.type != "cpu" else batch.numpy(), False)
        run = 1                                                                  # leading hops at consecutive multiples
        while run < len(chunk) and chunk[run] == chunk[0] + run * output_frames:
            run += 1
        for si, n in enumerate(names):
            o = outs[n]
            o = o if torch.is_tensor(o) else torch.from_numpy(np.ascontiguousarray(np.asarray(o, dtype=np.float32)))
            o = o.to(device)
            preds[si, chunk[0]:chunk[0] + run * output_frames].view(run, output_frames, C).copy_(o[:run])
            for bi in range(run, len(chunk)):                                    # the re-aligned last hop, written last
                preds[si, chunk[bi]:chunk[bi] + output_frames] = o[bi]           # :139
    return preds


def _separate_blend_chunks(separator, padded, table, lead, v_frames, batch_hops, input_frames, names, n_frames, C,
                           phase_iterations=0):
    """The blended hop loop through separator.get_output, for separators without a plan (the spectrogram U-Net, numpy
    stand-ins): the window at pred position p is padded[lead + p : lead + p + input_frames]; every chunk's estimates are
    accumulated by blend.blend_windows where `padded` lives."""
    from . import blend
    device = padded.device
    preds = torch.zeros((len(names), n_frames, C), dtype=torch.float32, device=device)
    den = torch.zeros(n_frames, dtype=torch.float32, device=device)
    for k in range(0, table.shape[0], batch_hops):
        chunk = table[k:k + batch_hops].copy()
        chunk[:, 1] = np.arange(chunk.shape[0])                                  # rows of this chunk's batch
        batch = torch.stack([padded[lead + p:lead + p + input_frames] for p in chunk[:, 0].tolist()])
        if phase_iterations:
            mags = separator.get_output(batch, False, return_spectrogram=True)
            outs = separator.reconstruct(mags, batch, phase_iterations)
        else:
            outs = separator.get_output(batch if device.type != "cpu" else batch.numpy(), False)
        rows = []
        for n in names:
            o = outs[n]
            o = o if torch.is_tensor(o) else torch.from_numpy(np.ascontiguousarray(np.asarray(o, dtype=np.float32)))
            rows.append(o.to(device=device, dtype=torch.float32))
        blend.blend_windows(torch.stack(rows).contiguous(), chunk, v_frames, preds, den)
    return blend.blend_finish(preds, den)


WEIGHTS = ("trained", "ema")


def weights_context(separator, weights):
    """The context predict / evaluate separate under: weights None or "trained" = the separator as it is; "ema" =
    separator.ema_weights(), the EMA of the weights its checkpoint carries.  ValueError for another value,
    RuntimeError when the separator (its checkpoint) has no EMA."""
    import contextlib
    if weights not in (None,) + WEIGHTS:
        raise ValueError("weights = %r, expected one of %s" % (weights, ", ".join(WEIGHTS)))
    if weights != "ema":
        return contextlib.nullcontext()
    if getattr(separator, "ema", None) is None:
        raise RuntimeError("weights='ema': the checkpoint (or the separator given) has no EMA of the weights -- it was "
                           "trained without model_config['optimizer']['ema_decay']")
    return separator.ema_weights()


def produce_source_estimates(model_config, load_model, input_path, output_path=None, separator=None, hop_frames=None,
                             postfilter=None, phase_iterations=0, overlap=None, shifts=None, max_shift=None, *, weights=None,
                             loudness=None):
    """Evaluate.produce_source_estimates (Evaluate.py:160-194): separate one mixture file with a
    checkpoint and write <input file name>_<source>.wav next to it (or into output_path), at the input file's sample rate
    and length.  WAV/NPY input at any rate (an .npy is taken to be at expected_sr; no MP3 decoding here): the separation runs
    through separate_track (hop_frames, postfilter, phase_iterations, overlap, shifts, max_shift: its options of those
    names; overlap / shifts / max_shift None: model_config["separation"]'s, else none; loudness None:
    model_config["loudness"]'s, else none).  weights="ema": separate with the EMA
    of the weights that the checkpoint carries (weights_context; RuntimeError when it has none).  Returns {source: [T, C]}."""
    import os
    from scipy.io import wavfile
    from . import datasets
    from .spectrogram import make_separator
    audio, sr = datasets.read_audio(input_path)                    # Utils.load(input_path, sr=None, mono=False), :172
    if sr is None:
        sr = model_config["expected_sr"]
    sep = separator if separator is not None else make_separator(model_config)
    if load_model is not None:
        from .checkpoint import load_checkpoint
        load_checkpoint(sep, load_model, with_optimizer=False)     # .npz or a TensorFlow V2 checkpoint prefix
    with weights_context(sep, weights):
        preds = separate_track(model_config, sep, audio, sr, hop_frames=hop_frames, postfilter=postfilter,
                               phase_iterations=phase_iterations, loudness=loudness_option(model_config, loudness),
                               **separation_options(model_config, overlap, shifts, max_shift))
    folder, name = os.path.split(input_path)
    if output_path is None:
        output_path = folder
    os.makedirs(output_path or ".", exist_ok=True)
    for source_name, source_audio in preds.items():
        wavfile.write(os.path.join(output_path, name) + "_" + source_name + ".wav", int(sr), np.asarray(source_audio, np.float32))
    return preds


def separation_options(model_config, overlap=None, shifts=None, max_shift=None):
    """The overlap / shifts / max_shift keywords of separate_track: each argument that is None falls back to
    model_config["separation"] = {"overlap": .., "shifts": .., "max_shift": ..} (config.EXTENSION_DEFAULTS: None, no
    blending)."""
    spec = model_config.get("separation") or {}
    if not isinstance(spec, dict) or set(spec) - {"overlap", "shifts", "max_shift"}:
        raise ValueError("model_config['separation'] = %r: a dict with the keys overlap, shifts, max_shift expected" % (spec,))
    return {"overlap": overlap if overlap is not None else spec.get("overlap", 0.0),
            "shifts": shifts if shifts is not None else spec.get("shifts"),
            "max_shift": max_shift if max_shift is not None else spec.get("max_shift")}


def loudness_option(model_config, loudness=None):
    """The loudness keyword of separate_track: the argument, or when it is None model_config["loudness"]
    (config.EXTENSION_DEFAULTS: None, no normalisation)."""
    return loudness if loudness is not None else model_config.get("loudness")


def evaluate_track(model_config, separator, mix_audio, stems, sr, results_dir=None, name=None, hop_frames=None,
                   window=1.0, hop=1.0, filters_len=512, postfilter=None, phase_iterations=0, overlap=None, shifts=None,
                   max_shift=None, *, loudness=None):
    """Evaluate.predict with a results_dir (Evaluate.py:59-80,146-158): separate the mixture (separate_track, estimates kept
    on the device), score them against the stems at the file's rate with bsseval.bss_eval, and write
    <results_dir>/<name>.json in museval's layout.  mix_audio [n, c] at sr; stems {source_name: [n, c]} at sr with the
    channel count of the estimates (a stereo model on a mono file gives two channels: mono stems are duplicated).  Signals
    are cut to the shortest length.  Returns {metric: float64 [S, nwin]}, sources in source_names order."""
    from . import bsseval
    est = separate_track(model_config, separator, mix_audio, sr, hop_frames=hop_frames, return_device=True,
                         postfilter=postfilter, phase_iterations=phase_iterations,
                         loudness=loudness_option(model_config, loudness),
                         **separation_options(model_config, overlap, shifts, max_shift))
    names = list(model_config["source_names"])
    c = int(est.shape[2])
    refs = []
    for k in names:
        a = stems[k]
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float32)
        if a.ndim == 1:
            a = a[:, None]
        if a.shape[1] != c:
            if a.shape[1] == 1:
                a = np.tile(a, [1, c])
            elif c == 1:
                a = np.mean(a, axis=1, keepdims=True)
            else:
                raise ValueError("stem %r has %d channels, the estimates %d" % (k, a.shape[1], c))
        refs.append(a)
    n = min([int(est.shape[1])] + [r.shape[0] for r in refs])
    ref = torch.from_numpy(np.ascontiguousarray(np.stack([r[:n] for r in refs]), dtype=np.float32))
    scores = bsseval.bss_eval(ref.to(est.device), est[:, :n].contiguous(), sr, window=window, hop=hop, filters_len=filters_len)
    if results_dir is not None:
        import os
        bsseval.write_track_json(os.path.join(results_dir, (name or "track") + ".json"), names, scores, window, hop)
    return scores


def compute_mean_metrics(json_folder, compute_averages=True, metric="SDR"):
    """Evaluate.compute_mean_metrics (Evaluate.py:195-232): the per-track JSON files of a folder -> per source
    (median, MAD, mean, SD) of `metric` over all segments, NaN segments (a silent source) ignored; compute_averages=False
    returns the per-source vectors of segment values instead.  A path containing "test.json" is skipped, as there."""
    import glob
    import json
    import os
    files = sorted(glob.glob(os.path.join(json_folder, "*.json")))
    inst_list = None
    for path in files:
        if "test.json" in path:                                                  # :213-215
            continue
        with open(path, "r") as f:
            js = json.load(f)
        if inst_list is None:
            inst_list = [list() for _ in range(len(js["targets"]))]
        for i in range(len(js["targets"])):
            inst_list[i].extend([float(fr["metrics"][metric]) for fr in js["targets"][i]["frames"]])
    inst_list = [np.array(perf, dtype=np.float64) for perf in (inst_list or [])]
    if compute_averages:
        return [(np.nanmedian(perf), np.nanmedian(np.abs(perf - np.nanmedian(perf))), np.nanmean(perf), np.nanstd(perf))
                for perf in inst_list]
    return inst_list


def produce_dataset_estimates(model_config, load_model, data_root, output_path, partition="test", separator=None,
                              hop_frames=None, postfilter=None, phase_iterations=0, overlap=None, shifts=None, max_shift=None,
                              *, weights=None, loudness=None):
    """The reference's produce_musdb_source_estimates (Evaluate.py:147-159) over the track folders of datasets.py:
    data_root/<partition>/<track>/<source>.wav|.npy (+ optional mix.wav|.npy, default: the sum of the stems), every file at
    one rate (an .npy: expected_sr).  Per track: the estimates as <output_path>/<partition>/<track>/<source>.wav and the
    scores as <output_path>/<partition>/<track>.json.  Returns the folder of the JSON files (compute_mean_metrics reads it).
    weights="ema": separate with the EMA of the weights (weights_context)."""
    from .spectrogram import make_separator
    sep = separator if separator is not None else make_separator(model_config)
    if load_model is not None:
        from .checkpoint import load_checkpoint
        load_checkpoint(sep, load_model, with_optimizer=False)
    with weights_context(sep, weights):
        return _dataset_estimates(model_config, sep, data_root, output_path, partition, hop_frames, postfilter, phase_iterations,
                                  dict(separation_options(model_config, overlap, shifts, max_shift),
                                       loudness=loudness_option(model_config, loudness)))


def _dataset_estimates(model_config, sep, data_root, output_path, partition, hop_frames, postfilter, phase_iterations, blend_kw):
    """produce_dataset_estimates on a loaded separator."""
    import os
    from scipy.io import wavfile
    from . import bsseval, datasets
    names = list(model_config["source_names"])
    base = os.path.join(data_root, partition)
    out_dir = os.path.join(output_path, partition)
    os.makedirs(out_dir, exist_ok=True)
    for d in sorted(os.listdir(base)):
        folder = os.path.join(base, d)
        if not os.path.isdir(folder):
            continue
        stems, sr = {}, None
        for k in names + ["mix"]:
            for ext in (".wav", ".npy"):
                f = os.path.join(folder, k + ext)
                if os.path.exists(f):
                    stems[k], r = datasets.read_audio(f)
                    sr = r if r is not None else sr
                    break
            else:
                if k != "mix":
                    raise FileNotFoundError("%s: no %s.wav/.npy" % (folder, k))
        sr = int(sr) if sr is not None else int(model_config["expected_sr"])
        mix = stems.pop("mix") if "mix" in stems else sum(stems[k] for k in names)
        est = separate_track(model_config, sep, mix, sr, hop_frames=hop_frames, return_device=True, postfilter=postfilter,
                             phase_iterations=phase_iterations, **blend_kw)
        c = int(est.shape[2])
        refs = [np.tile(stems[k], [1, c]) if stems[k].shape[1] == 1 and c > 1 else stems[k] for k in names]
        n = min([int(est.shape[1])] + [r.shape[0] for r in refs])
        ref = torch.from_numpy(np.ascontiguousarray(np.stack([r[:n] for r in refs]), dtype=np.float32)).to(est.device)
        scores = bsseval.bss_eval(ref, est[:, :n].contiguous(), sr)
        bsseval.write_track_json(os.path.join(out_dir, d + ".json"), names, scores)
        host = est.cpu().numpy()
        os.makedirs(os.path.join(out_dir, d), exist_ok=True)
        for si, k in enumerate(names):
            wavfile.write(os.path.join(out_dir, d, k + ".wav"), sr, host[si])
    return out_dir
