"""The data contract in front of the hot path: the reference's snippet pipeline
(/root/reference/Datasets.py:16-34,76,188-216 and Utils.py:26-42) without TFRecords/tf.data.

A *track* is a dict {source_name: [T, C] float32, ..., "mix": [T, C]} (what Datasets.write_records
stores per song, :57-90).  get_dataset() reproduces the reference's stream of batches
  pad both ends by (input_frames - output_frames)//2 zeros                    (Datasets.py:49,76)
  train: num_snippets_per_track random snippets per track                      (:16-20,201-202)
  valid/test: every snippet at hop = output_frames                             (:22-27,203-204)
  train + augmentation: per-source gain U(0.7, 1.0), mix := sum of sources     (Utils.py:26-36)
  targets centre-cropped to the output length                                  (Utils.py:38-42)
  train: repeat + shuffle buffer of cache_size snippets                        (Datasets.py:211-213)
  batches of batch_size, remainder dropped                                     (:215)
on the host in numpy.  DeviceSnippetSource is the MI355X-first producer for training: every padded
track lives in HBM (a full MUSDB train set at 22 kHz mono fp32 is ~4 GB of 288 GB), and a batch
is one gather + gain + sum + crop on the GPU, so the input side keeps up with a ~10 ms step.  FusedSnippetSource is
the same producer as ONE HIP kernel per batch (wun_gather_snippets), which also carries the source-level augmentations
the reference lacks: independent remix, channel swap, polarity (augmented_descriptors).

Decoding MUSDB stems (musdb, soundfile in the reference, Datasets.py:119-186) is out of scope: tracks come from WAV
(scipy) or .npy files, at model_config["expected_sr"] or -- with resample=True -- at any rate (resample.py).
"""
import math
import os

import numpy as np


# --------------------------------------------------------------------------------------
# tracks
# --------------------------------------------------------------------------------------
def read_audio(path):
    """([T, C] float32, sample rate) of a .wav (PCM16/32 or float) or .npy file; the rate of an .npy is None (unknown)."""
    if path.endswith(".npy"):
        audio = np.load(path).astype(np.float32)
        sr = None
    else:
        from scipy.io import wavfile
        sr, raw = wavfile.read(path)
        if raw.dtype == np.int16:
            audio = raw.astype(np.float32) / 32768.0
        elif raw.dtype == np.int32:
            audio = raw.astype(np.float32) / 2147483648.0
        elif raw.dtype == np.uint8:
            audio = (raw.astype(np.float32) - 128.0) / 128.0
        else:
            audio = raw.astype(np.float32)
    if audio.ndim == 1:
        audio = audio[:, None]
    return np.ascontiguousarray(audio, dtype=np.float32), sr


def load_audio(path, mono=False, expected_sr=None, resample=False):
    """[T, C] float32 from a .wav (PCM16/32 or float) or .npy file (Utils.load, Utils.py:97-110).  A file at another rate
    than expected_sr is refused unless resample=True: then it is downmixed (mono) and resampled to expected_sr as
    librosa.load does, with resample.py's filter (scipy's Kaiser design on the host, not resampy's)."""
    audio, sr = read_audio(path)
    mismatch = expected_sr is not None and sr is not None and int(sr) != int(expected_sr)
    if mismatch and not resample:
        raise NotImplementedError("%s is at %s Hz, expected %s: pass resample=True (the `resample=1` option of the "
                                  "train / test commands) to convert it" % (path, sr, expected_sr))
    if mono and audio.shape[1] > 1:
        audio = audio.mean(axis=1, keepdims=True)
    if mismatch:
        from .resample import resample as _resample
        audio = _resample(audio, sr, expected_sr)
    return np.ascontiguousarray(audio, dtype=np.float32)


def make_track(sources, model_config, mix=None, resample=False):
    """Validated track dict from {source_name: array-or-path}.  Mono tracks are duplicated when
    the model is stereo (Datasets.py:64-66); all signals must have equal shape (:79-84); the mix
    defaults to the sum of the sources."""
    mono = bool(model_config["mono_downmix"])
    track = {}
    for key in model_config["source_names"]:
        a = sources[key]
        a = load_audio(a, mono, model_config.get("expected_sr"), resample) if isinstance(a, str) else np.asarray(a, np.float32)
        if a.ndim == 1:
            a = a[:, None]
        if mono and a.shape[1] > 1:
            a = a.mean(axis=1, keepdims=True)
        if not mono and a.shape[1] == 1:
            a = np.tile(a, [1, 2])
        track[key] = np.ascontiguousarray(a, np.float32)
    shapes = {a.shape for a in track.values()}
    assert len(shapes) == 1, "all signals of a track must have the same length and channels"
    if mix is None:
        mix = sum(track[k] for k in model_config["source_names"])
    elif isinstance(mix, str):
        mix = load_audio(mix, mono, model_config.get("expected_sr"), resample)
    mix = np.asarray(mix, np.float32)
    if mix.ndim == 1:
        mix = mix[:, None]
    if not mono and mix.shape[1] == 1:
        mix = np.tile(mix, [1, 2])
    track["mix"] = np.ascontiguousarray(mix, np.float32)
    length, channels = track["mix"].shape
    for a in track.values():
        assert a.shape == (length, channels), "all signals of a track must have the same length and channels"
    return track


def load_track_dir(path, model_config, resample=False):
    """A directory holding <source_name>.wav|.npy for every source and optionally mix.wav|.npy.  resample: convert files at
    another rate to expected_sr (load_audio) instead of refusing them."""
    def find(stem):
        for ext in (".wav", ".npy"):
            f = os.path.join(path, stem + ext)
            if os.path.exists(f):
                return f
        return None
    srcs = {}
    for key in model_config["source_names"]:
        f = find(key)
        if f is None:
            raise FileNotFoundError("%s: no %s.wav/.npy" % (path, key))
        srcs[key] = f
    return make_track(srcs, model_config, mix=find("mix"), resample=resample)


def load_partition(root, partition, model_config, resample=False):
    """root/<partition>/<track>/ directories, sorted by name."""
    base = os.path.join(root, partition)
    return [load_track_dir(os.path.join(base, d), model_config, resample)
            for d in sorted(os.listdir(base)) if os.path.isdir(os.path.join(base, d))]


def normalize_tracks(tracks, model_config, device, spec):
    """Loudness-normalised training data: every track's MIX is metered once on `device` at expected_sr
    (loudness.integrated, BS.1770-4), the gain to spec's target is computed there (loudness.gain) and read back -- the one host
    synchronisation per track, at load time -- and that one float32 factor multiplies the mix and every stem (one fp32 product
    per sample, so the stems still sum to the mix as before up to that rounding).  spec: what loudness.from_config takes; with
    its "true_peak_limit" the mix is metered by loudness.r128 and the gain keeps its true peak under the limit (5.28).
    Returns (new track dicts, float32 gains [len(tracks)]); the given tracks are left as they are.  GPU only."""
    import torch
    from . import loudness as ld
    spec = ld.from_config(spec)
    if spec is None:
        raise ValueError("normalize_tracks needs a loudness spec, got None")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("normalize_tracks meters on a GPU; there is no CPU fallback (got device %s)" % device)
    sr = int(model_config["expected_sr"])
    out, gains = [], np.zeros(len(tracks), np.float32)
    for i, track in enumerate(tracks):
        mix = torch.from_numpy(np.ascontiguousarray(track["mix"], np.float32)).to(device)
        meter, limit = ld.meter_for(mix, sr, spec)                              # true_peak_limit: r128, else integrated
        g = ld.gain(meter, spec["target"], spec["max_gain_db"], limit)
        gains[i] = g[0:1].cpu().numpy()[0]                                      # the one sync of this track
        out.append({k: np.ascontiguousarray(np.asarray(v, np.float32) * gains[i]) for k, v in track.items()})
    return out, gains


def loudness_data_spec(model_config):
    """model_config["loudness"] when it asks for normalised training data ("data": True), else None."""
    from . import loudness as ld
    spec = ld.from_config(model_config.get("loudness"))
    return spec if spec is not None and spec["data"] else None


def pad_track(track, pad_frames):
    """Zero padding at both ends (Datasets.py:76)."""
    if pad_frames <= 0:
        return dict(track)
    return {k: np.pad(v, [(pad_frames, pad_frames), (0, 0)], mode="constant") for k, v in track.items()}


# --------------------------------------------------------------------------------------
# snippets
# --------------------------------------------------------------------------------------
def random_positions(length, input_frames, num, rng):
    """tf.random_uniform([num], 0, length - input_frames, int64) (Datasets.py:18)."""
    hi = length - input_frames
    if hi <= 0:
        raise ValueError("track shorter than the network input (%d <= %d)" % (length, input_frames))
    return rng.integers(0, hi, size=num, dtype=np.int64)


def all_positions(length, input_frames, output_frames):
    """tf.range(0, length - input_frames, delta=output_frames) (Datasets.py:24)."""
    return np.arange(0, length - input_frames, output_frames, dtype=np.int64)


def take_snippets_at_pos(track, keys, start_pos, input_frames):
    """{key: [n, input_frames, C]} (Datasets.py:29-34)."""
    return {k: np.stack([track[k][p:p + input_frames, :] for p in start_pos]) if len(start_pos)
            else np.zeros((0, input_frames, track[k].shape[1]), np.float32) for k in keys}


def random_amplify(sample, rng):
    """Per-source scalar gain U(0.7, 1.0); the mix becomes the sum of the amplified sources
    (Utils.py:26-36).  `sample` holds single snippets [T, C]."""
    out = {}
    for key, val in sample.items():
        if key != "mix":
            out[key] = np.float32(rng.uniform(0.7, 1.0)) * val
    out["mix"] = sum(out[k] for k in out)
    return out


def crop_sample(sample, crop_frames):
    """Targets (everything but the mix) lose crop_frames at both ends (Utils.py:38-42)."""
    return {k: (v[crop_frames:-crop_frames, :] if (k != "mix" and crop_frames > 0) else v) for k, v in sample.items()}


def snippet_descriptors(model_config, lengths, input_frames, output_frames, partition, rng):
    """The reference's snippet stream (Datasets.py:188-216) as DESCRIPTORS (track_index, start, gains):
    which snippet of which padded track comes next and, for train + augmentation, the per-source
    gains of Utils.random_amplify (float32 [S], else None).  `lengths` are the padded track lengths.
      train     : endless; per pass the tracks in shuffled order (:195), num_snippets_per_track
                  uniform start positions each (:16-20,201-202), then the shuffle buffer of
                  cache_size elements (:211-213)
      otherwise : one pass, tracks in order, every hop of output_frames (:22-27,203-204)
    Both producers below (host numpy batches, on-GPU gather) consume this one stream, so they
    deliver identical batches for the same seed."""
    train = partition == "train"
    S = len(model_config["source_names"])
    n_tracks = len(lengths)

    def raw():
        while True:
            order = rng.permutation(n_tracks) if train else np.arange(n_tracks)
            for ti in order:
                if train:
                    pos = random_positions(lengths[ti], input_frames, int(model_config["num_snippets_per_track"]), rng)
                else:
                    pos = all_positions(lengths[ti], input_frames, output_frames)
                for p in pos:
                    gains = None
                    if train and model_config["augmentation"]:
                        gains = rng.uniform(0.7, 1.0, size=S).astype(np.float32)
                    yield int(ti), int(p), gains
            if not train:
                return

    def shuffled(stream, buffer_size):
        buf = []
        for s in stream:
            if len(buf) < buffer_size:
                buf.append(s)
                continue
            i = int(rng.integers(0, buffer_size))
            out, buf[i] = buf[i], s
            yield out
        rng.shuffle(buf)                 # (finite streams only; the train stream repeats forever)
        for s in buf:
            yield s

    return shuffled(raw(), int(model_config["cache_size"])) if train else raw()


def materialize(track, keys, source_names, start, input_frames, gains, crop_frames):
    """One snippet {key: [T, C]} from a padded track: cut (Datasets.py:29-34), amplify + re-sum the mix
    (Utils.py:26-36, when gains are given), centre-crop the targets (Utils.py:38-42)."""
    s = {k: track[k][start:start + input_frames, :] for k in keys}
    if gains is not None:
        amp = {k: np.float32(g) * s[k] for k, g in zip(source_names, gains)}
        mix = amp[source_names[0]]
        for k in source_names[1:]:
            mix = mix + amp[k]
        amp["mix"] = mix
        s = amp
    return crop_sample(s, crop_frames)


def get_dataset(model_config, input_shape, output_shape, partition, tracks, seed=1337, rng=None):
    """Generator of batches {source..., "mix"}: mix [B, Tin, C], sources [B, Tout, C]
    (Datasets.get_dataset, Datasets.py:113-218, minus the TFRecord cache).  `tracks` is the list of
    track dicts of this partition.  Train: endless, shuffled; otherwise one pass in order."""
    input_frames, output_frames = int(input_shape[1]), int(output_shape[1])
    assert (input_frames - output_frames) % 2 == 0
    pad = (input_frames - output_frames) // 2
    names = list(model_config["source_names"])
    keys = names + ["mix"]
    batch_size = int(model_config["batch_size"])
    rng = rng if rng is not None else np.random.default_rng(seed)
    padded = [pad_track(t, pad) for t in tracks]
    lengths = [t["mix"].shape[0] for t in padded]
    batch = []
    for ti, pos, gains in snippet_descriptors(model_config, lengths, input_frames, output_frames, partition, rng):
        batch.append(materialize(padded[ti], keys, names, pos, input_frames, gains, pad))
        if len(batch) == batch_size:
            yield {k: np.stack([b[k] for b in batch]) for k in keys}
            batch = []
    # remainder dropped (batch_and_drop_remainder, :215)


def batch_to_device(batch, model_config, device):
    """(mix [B,Tin,C], targets [S,B,Tout,C]) torch tensors in source_names order: the step's inputs."""
    import torch
    mix = torch.from_numpy(np.ascontiguousarray(batch["mix"])).to(device)
    targets = torch.from_numpy(np.stack([batch[k] for k in model_config["source_names"]])).to(device)
    return mix, targets


class DeviceSnippetSource(object):
    """Training batches produced on the GPU from tracks resident in HBM.

    The reference's train pipeline exactly (per pass: shuffled tracks, num_snippets_per_track uniform
    positions per track, per-source gain U(0.7,1.0) and mix = sum when augmentation is on, shuffle
    buffer of cache_size snippets, centre-cropped targets): the snippet stream is the same
    snippet_descriptors() sequence the host pipeline consumes -- only (track, start, gains) triples
    move through the shuffle buffer on the host, a few bytes per snippet -- and a batch is ONE
    gather + gain + sum + crop on the GPU.  For equal seeds the batches are bit-identical to
    get_dataset(..., "train", ...).  Calling the object returns (mix [B,Tin,C], targets [S,B,Tout,C])."""

    def __init__(self, model_config, tracks, input_frames, output_frames, batch_size, device, seed=1337, rng=None):
        import torch
        self.cfg = model_config
        self.names = list(model_config["source_names"])
        self.t_in, self.t_out = int(input_frames), int(output_frames)
        self.pad = (self.t_in - self.t_out) // 2
        self.batch = int(batch_size)
        self.device = torch.device(device)
        starts, lens, cat = [], [], {k: [] for k in self.names + ["mix"]}
        off = 0
        for t in tracks:
            p = pad_track(t, self.pad)
            n = p["mix"].shape[0]
            if n <= self.t_in:
                raise ValueError("track shorter than the network input")
            starts.append(off); lens.append(n); off += n
            for k in cat:
                cat[k].append(p[k])
        self.track_start = np.asarray(starts, dtype=np.int64)
        self.data = {k: torch.from_numpy(np.concatenate(v)).to(self.device) for k, v in cat.items()}
        self.frame = torch.arange(self.t_in, device=self.device, dtype=torch.int64)
        self.stream = snippet_descriptors(model_config, lens, self.t_in, self.t_out, "train",
                                          rng if rng is not None else np.random.default_rng(seed))

    def __call__(self):
        import torch
        B, S = self.batch, len(self.names)
        desc = [next(self.stream) for _ in range(B)]
        base = torch.from_numpy(np.asarray([self.track_start[ti] + pos for ti, pos, _ in desc], dtype=np.int64))
        idx = base.to(self.device)[:, None] + self.frame[None, :]                          # [B, Tin]
        srcs = torch.stack([self.data[k][idx] for k in self.names])                        # [S, B, Tin, C]
        if desc[0][2] is not None:
            gain = torch.from_numpy(np.stack([g for _, _, g in desc], axis=1)).to(self.device)   # [S, B]
            srcs = srcs * gain[:, :, None, None]
            mix = srcs[0]
            for s in range(1, S):                       # same summation order as the host pipeline
                mix = mix + srcs[s]
        else:
            mix = self.data["mix"][idx]
        targets = srcs[:, :, self.pad:self.t_in - self.pad, :] if self.pad > 0 else srcs
        return mix.contiguous(), targets.contiguous()


# --------------------------------------------------------------------------------------
# the fused producer: descriptors with source-level augmentations, one gather kernel per batch
# --------------------------------------------------------------------------------------
# one source of one batch row: wun_snippet_source of include/wun.h (start in frames of the source's plane)
SNIPPET_DTYPE = np.dtype([("start", np.int64), ("gain", np.float32), ("flags", np.uint32)])
SNIPPET_SWAP, SNIPPET_NEGATE = 1, 2
AUGMENT_KEYS = ("remix", "channel_swap", "polarity", "speed")
# the rate bank of wun_gather_snippets_speed (include/wun.h): (up, down) pairs, speed = down / up
SPEED_RATES_DEFAULT = ((10, 9), (20, 19), (20, 21), (10, 11))      # speeds 0.9, 0.95, 1.05, 1.1
SPEED_MAX_RATES, SPEED_MAX_RATIO = 8, 64                           # WUN_SPEED_RATES, WUN_SPEED_MAX_RATIO
# the phase vocoder's augmentations (wun_time_stretch): probabilities, next to AUGMENT_KEYS
VOCODER_KEYS = ("pitch_shift", "time_stretch")
PITCH_SHIFT_RATES_DEFAULT = ((18, 17), (9, 8), (17, 18), (8, 9))   # (up, down): pitch times down / up, about -1, -2, +1, +2 semitones
TIME_STRETCH_RATES_DEFAULT = ((10, 9), (20, 19), (20, 21), (10, 11))   # (num, den): tempo num / den
VOCODER_FFT_DEFAULT = (2048, 512)
_RATE_KEYS = {"speed_rates": "speed", "pitch_shift_rates": "pitch_shift", "time_stretch_rates": "time_stretch"}


def speed_source_frames(input_frames, up, down):
    """Source frames behind a window of input_frames played at speed down / up (wun_speed_source_frames): the smallest n
    with resample.frames(n, up, down) >= input_frames."""
    return ((int(input_frames) - 1) * int(down)) // int(up) + 1


def _check_speed_rates(rates, key="speed_rates"):
    """The bank as a tuple of (up, down) reduced by their gcd; ValueError for what wun_gather_snippets_speed refuses.  The
    ratios of the vocoder's keys obey the same rules (wun_time_stretch has the same ceilings)."""
    if isinstance(rates, (str, bytes, dict)) or not hasattr(rates, "__len__"):
        raise ValueError("augment[%r] must be a list of [up, down] pairs, got %r" % (key, rates))
    if not 1 <= len(rates) <= SPEED_MAX_RATES:
        raise ValueError("augment[%r] holds 1 to %d pairs, got %d" % (key, SPEED_MAX_RATES, len(rates)))
    out = []
    for pair in rates:
        ok = not isinstance(pair, (str, bytes, dict)) and hasattr(pair, "__len__") and len(pair) == 2 and all(
            isinstance(v, (int, np.integer)) and not isinstance(v, bool) and v > 0 for v in pair)
        if not ok:
            raise ValueError("augment[%r]: every pair is [up, down] of positive integers, got %r" % (key, pair))
        g = math.gcd(int(pair[0]), int(pair[1]))
        up, down = int(pair[0]) // g, int(pair[1]) // g
        if up == down:
            raise ValueError("augment[%r]: %r is the unit rate 1/1" % (key, pair))
        if max(up, down) > SPEED_MAX_RATIO or down > 2 * up or up > 2 * down:
            raise ValueError("augment[%r]: %r needs max(up, down) <= %d after reduction and a speed down / up in "
                             "[1/2, 2]" % (key, pair, SPEED_MAX_RATIO))
        if (up, down) in out:
            raise ValueError("augment[%r]: %r occurs twice (after reduction)" % (key, pair))
        out.append((up, down))
    return tuple(out)


def _check_vocoder_fft(res):
    ok = not isinstance(res, (str, bytes, dict)) and hasattr(res, "__len__") and len(res) == 2 and all(
        isinstance(v, (int, np.integer)) and not isinstance(v, bool) and v > 0 for v in res)
    if ok:
        n_fft, hop = int(res[0]), int(res[1])
        ok = 64 <= n_fft <= 8192 and n_fft & (n_fft - 1) == 0 and hop & (hop - 1) == 0 and hop <= n_fft // 4
    if not ok:
        raise ValueError("augment['vocoder_fft'] must be [n_fft, hop]: n_fft a power of two in 64..8192, hop a power of two at "
                         "most n_fft / 4 (wun_time_stretch), got %r" % (res,))
    return n_fft, hop


def check_augment(model_config, augment):
    """{key: probability} of the active augmentations (probability > 0); with an active "speed" also "speed_rates": the bank
    as a tuple of reduced (up, down) pairs (augment["speed_rates"], default SPEED_RATES_DEFAULT).  ValueError for an unknown
    key, a probability outside [0, 1] (NaN included), channel_swap on a mono config, speed_rates without an active speed and
    a bank the library would refuse (1/1, duplicates after reduction, more than 8 pairs, a ratio above 64 or outside [1/2, 2]).
    The vocoder's keys (VOCODER_KEYS) follow the same rules: an active "pitch_shift" / "time_stretch" brings its
    "pitch_shift_rates" / "time_stretch_rates" (defaults PITCH_SHIFT_RATES_DEFAULT / TIME_STRETCH_RATES_DEFAULT), either one
    "vocoder_fft": (n_fft, hop) (default VOCODER_FFT_DEFAULT), and an active pitch_shift "bank_rates": speed_rates followed
    by the pitch_shift_rates not among them -- the resampler's bank, ValueError when it exceeds 8 entries."""
    if augment is None:
        return {}
    if not isinstance(augment, dict):
        raise ValueError("augment must be a dict with the optional keys %s, got %r" % (", ".join(AUGMENT_KEYS), augment))
    active = {}
    for key, p in augment.items():
        if key in _RATE_KEYS or key == "vocoder_fft":
            continue
        if key not in AUGMENT_KEYS and key not in VOCODER_KEYS:
            raise ValueError("unknown augmentation %r (have: %s)" % (key, ", ".join(AUGMENT_KEYS + VOCODER_KEYS)))
        if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)) or not 0.0 <= float(p) <= 1.0:
            raise ValueError("augment[%r] must be a probability in [0, 1], got %r" % (key, p))
        if float(p) > 0.0:
            active[key] = float(p)
    if "channel_swap" in active and model_config["mono_downmix"]:
        raise ValueError("augment['channel_swap'] needs two channels; this config is mono (mono_downmix=True)")
    defaults = {"speed_rates": SPEED_RATES_DEFAULT, "pitch_shift_rates": PITCH_SHIFT_RATES_DEFAULT,
                "time_stretch_rates": TIME_STRETCH_RATES_DEFAULT}
    for rkey, key in _RATE_KEYS.items():
        if key in active:
            active[rkey] = _check_speed_rates(augment.get(rkey, defaults[rkey]), rkey)
        elif rkey in augment:
            raise ValueError("augment[%r] needs an active augment[%r] (a probability > 0)" % (rkey, key))
    if any(k in active for k in VOCODER_KEYS):
        active["vocoder_fft"] = _check_vocoder_fft(augment.get("vocoder_fft", VOCODER_FFT_DEFAULT))
    elif "vocoder_fft" in augment:
        raise ValueError("augment['vocoder_fft'] needs an active augment['pitch_shift'] or augment['time_stretch']")
    if "pitch_shift" in active:
        bank = tuple(active.get("speed_rates", ()))
        bank += tuple(r for r in active["pitch_shift_rates"] if r not in bank)
        if len(bank) > SPEED_MAX_RATES:
            raise ValueError("augment: speed_rates and pitch_shift_rates together need %d entries of the resampler's bank of %d"
                             % (len(bank), SPEED_MAX_RATES))
        active["bank_rates"] = bank
    return active


def _refuse_vocoder(active, who):
    for key in VOCODER_KEYS:
        if key in active:
            raise ValueError("augment[%r] needs the job stream: use datasets.vocoder_descriptors, which yields (rec, mix_mode, "
                             "rate, jobs) -- %s does not carry jobs" % (key, who))


def augmented_descriptors(model_config, lengths, input_frames, output_frames, rng, augment=None, aug_rng=None):
    """snippet_descriptors(..., "train", rng) -- the unchanged stream, shuffle buffer included -- as the tables of
    wun_gather_snippets, with the source-level augmentations drawn on top.  Yields (rec, mix_mode) per snippet: rec is a
    SNIPPET_DTYPE array [S] of (plane offset of the track + start, gain, flags), the planes being the padded tracks one behind
    the other (`lengths` in order); mix_mode 1 = the mix is the sum of the delivered sources, 0 = the track's own mix.
      augment empty : exactly the base stream -- every source at the base (track, start), the base gains (else 1.0), flags 0,
                      mix_mode 1 iff the base stream carried gains (model_config["augmentation"])
      augment       : {"remix": p, "channel_swap": p, "polarity": p}, each optional.  remix -- with probability p every source
                      s >= 1 comes from a track and a start of its own (source 0 keeps the base position): the stems of different
                      songs mixed; channel_swap / polarity -- per source, with probability p the two channels change places / the
                      sign flips.  Next to the reference's per-source gain (Utils.py:26-36).  Any active one makes mix_mode 1.
    The draws come from aug_rng (default np.random.default_rng([1337, 1]); FusedSnippetSource passes [seed, 1]), never from
    rng, so the base stream does not shift.  Only keys with a probability > 0 draw, in this order per snippet: one uniform for
    remix; if taken, per source s >= 1 a track (integers(0, n_tracks)) then a start (integers(0, len - Tin)); one uniform per
    source for the swap; one uniform per source for the polarity.  An active "speed" is refused with a ValueError: its stream
    carries a rate per source (speed_descriptors); so are the vocoder's keys, whose stream carries jobs (vocoder_descriptors)."""
    active = check_augment(model_config, augment)
    if "speed" in active:
        raise ValueError("augment['speed'] needs the rate stream: use datasets.speed_descriptors, which yields (rec, mix_mode, rate)")
    _refuse_vocoder(active, "augmented_descriptors")
    for rec, mix_mode, _, _ in _descriptors(model_config, lengths, input_frames, output_frames, rng, augment, aug_rng):
        yield rec, mix_mode


def speed_descriptors(model_config, lengths, input_frames, output_frames, rng, augment=None, aug_rng=None):
    """augmented_descriptors with speed perturbation: yields (rec, mix_mode, rate) per snippet, rate a uint8 [S] of rate indices
    for wun_gather_snippets_speed (0 = unit rate, i >= 1 = entry i - 1 of the bank check_augment returns as "speed_rates").
    Without an active "speed" (rec, mix_mode) are exactly augmented_descriptors' and rate is zero.
      augment["speed"] = p, augment["speed_rates"] = [[up, down], ...] (optional): with probability p the snippet is played at
      a speed down / up of the bank -- pitch and tempo together.  A remixed snippet draws a rate per source; otherwise all
      sources share one, so the stems of one song stay aligned.  An active speed makes mix_mode 1.
    Draws (aug_rng only, after remix, swap and polarity): one random(); if taken, integers(0, R) per source s = 0..S-1 for a
    remixed snippet, else one integers(0, R) for all.  Placement takes no draws: a rated source reads n_src =
    speed_source_frames(Tin, up, down) frames of its padded track j (length len_j) around the centre of its unit window at
    pos -- it starts at clip(pos + (Tin - n_src) // 2, 0, len_j - n_src) -- and a track shorter than n_src keeps the unit rate.
    The vocoder's keys are refused with a ValueError: their stream carries jobs (vocoder_descriptors)."""
    _refuse_vocoder(check_augment(model_config, augment), "speed_descriptors")
    return _strip_jobs(_descriptors(model_config, lengths, input_frames, output_frames, rng, augment, aug_rng))


def _strip_jobs(stream):
    for rec, mix_mode, rate, _ in stream:
        yield rec, mix_mode, rate


def vocoder_descriptors(model_config, lengths, input_frames, output_frames, rng, augment=None, aug_rng=None):
    """speed_descriptors with the phase vocoder's augmentations (wun_time_stretch): yields (rec, mix_mode, rate,
    jobs) per snippet, jobs an int64 [S, 4] of (span_start, n_span, num, den) -- the span of the source's plane that a job
    stretches at the tempo num / den before the gather reads its output -- with n_span = 0 for a source without a job.  Without
    the vocoder's keys (rec, mix_mode, rate) are exactly speed_descriptors' and jobs is zero.
      augment["pitch_shift"] = p, augment["pitch_shift_rates"] = [[up, down], ...] (optional): with probability p the snippet is
      transposed to the pitch down / up at its own tempo: a job stretches n_span = ceil(n_src up / down) frames to n_src =
      speed_source_frames(Tin, up, down) at num / den = up / down, and the gather resamples those to Tin through the bank entry
      (up, down) of check_augment's "bank_rates" (rate = its index + 1).
      augment["time_stretch"] = p, augment["time_stretch_rates"] = [[num, den], ...] (optional): with probability p the snippet
      is played at the tempo num / den in its own key: a job stretches n_span = ceil(Tin num / den) frames to Tin; rate 0.
    A snippet takes at most one of speed, pitch_shift and time_stretch.  Draws (aug_rng only, after speed's; a snippet that took
    an earlier one draws nothing for the later ones), for pitch_shift then time_stretch: one random(); if taken, integers(0, R)
    per source s = 0..S-1 for a remixed snippet, else one for all, so the stems of one song share the ratio.  Placement takes no
    draws: the span starts at clip(pos + (Tin - n_span) // 2, 0, len_j - n_span) of the source's padded track j, and a track
    shorter than n_span keeps the plain window (no job, rate 0).  rec["start"] of a source with a job is the span's start; the
    consumer points it at the job's output (FusedSnippetSource: a slot behind the planes).  An active key makes mix_mode 1."""
    return _descriptors(model_config, lengths, input_frames, output_frames, rng, augment, aug_rng)


def _descriptors(model_config, lengths, input_frames, output_frames, rng, augment, aug_rng):
    active = check_augment(model_config, augment)
    S = len(model_config["source_names"])
    n_tracks = len(lengths)
    offset = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))[:-1]]).astype(np.int64)
    if active and aug_rng is None:
        aug_rng = np.random.default_rng([1337, 1])
    bank = active.get("speed_rates", ())
    bank_all = active.get("bank_rates", bank)
    vocoder = [k for k in VOCODER_KEYS if k in active]
    unit = np.zeros(S, dtype=np.uint8)                    # shared by every snippet at the unit rate (read-only)
    unit.setflags(write=False)
    no_jobs = np.zeros((S, 4), dtype=np.int64)            # shared by every snippet without a job (read-only)
    no_jobs.setflags(write=False)
    for ti, pos, gains in snippet_descriptors(model_config, lengths, input_frames, output_frames, "train", rng):
        rec = np.zeros(S, dtype=SNIPPET_DTYPE)
        rate, jobs = unit, no_jobs
        rec["start"] = offset[ti] + pos
        rec["gain"] = gains if gains is not None else 1.0
        # (track, start inside it) of every source: speed and the vocoder place by it
        where = [(int(ti), int(pos))] * S if bank or vocoder else None
        remixed = "remix" in active and aug_rng.random() < active["remix"]
        if remixed:
            for s in range(1, S):
                tj = int(aug_rng.integers(0, n_tracks))
                p = int(random_positions(lengths[tj], input_frames, None, aug_rng))
                rec["start"][s] = offset[tj] + p
                if where is not None:
                    where[s] = (tj, p)
        if "channel_swap" in active:
            for s in range(S):
                if aug_rng.random() < active["channel_swap"]:
                    rec["flags"][s] |= SNIPPET_SWAP
        if "polarity" in active:
            for s in range(S):
                if aug_rng.random() < active["polarity"]:
                    rec["flags"][s] |= SNIPPET_NEGATE
        taken = "speed" in active and aug_rng.random() < active["speed"]
        if taken:
            if remixed:
                picks = [int(aug_rng.integers(0, len(bank))) for _ in range(S)]
            else:
                picks = [int(aug_rng.integers(0, len(bank)))] * S
            rate = np.zeros(S, dtype=np.uint8)
            for s in range(S):
                tj, p = where[s]
                n_src = speed_source_frames(input_frames, *bank[picks[s]])
                if lengths[tj] < n_src:
                    continue                              # the track cannot fill the window at this speed: unit rate
                rate[s] = picks[s] + 1
                rec["start"][s] = offset[tj] + min(max(p + (input_frames - n_src) // 2, 0), lengths[tj] - n_src)
        for key in vocoder:
            if taken or not aug_rng.random() < active[key]:
                continue
            taken = True
            ratios = active[key + "_rates"]
            if remixed:
                picks = [int(aug_rng.integers(0, len(ratios))) for _ in range(S)]
            else:
                picks = [int(aug_rng.integers(0, len(ratios)))] * S
            rate, jobs = np.zeros(S, dtype=np.uint8), np.zeros((S, 4), dtype=np.int64)
            for s in range(S):
                tj, p = where[s]
                num, den = ratios[picks[s]]
                n_out = speed_source_frames(input_frames, num, den) if key == "pitch_shift" else input_frames
                n_span = -((-n_out * num) // den)
                if lengths[tj] < n_span:
                    continue                              # the track cannot fill the span: the plain window
                if key == "pitch_shift":
                    rate[s] = bank_all.index((num, den)) + 1
                start = offset[tj] + min(max(p + (input_frames - n_span) // 2, 0), lengths[tj] - n_span)
                rec["start"][s] = start
                jobs[s] = (start, n_span, num, den)
        yield rec, int(gains is not None or bool(active)), rate, jobs


class FusedSnippetSource(object):
    """DeviceSnippetSource's batches from ONE kernel (wun_gather_snippets, csrc/wun_dataset.hip): the same residency -- the
    padded tracks one behind the other, one plane per key, in HBM -- and per batch a table of B x S descriptors (16 bytes
    each) that travels in the kernel arguments: no index tensor, no host-to-device copy, no intermediate.  Calling the object
    returns (mix [B,Tin,C], targets [S,B,Tout,C]) as fresh tensors, written on the current stream.

    partition "train": endless; augmented_descriptors' stream -- without `augment` bit-identical to get_dataset(..., "train",
    ...) and DeviceSnippetSource for equal seeds; with it the remix / channel-swap / polarity / speed augmentations on top
    (draws from np.random.default_rng([seed, 1])); with "speed" the batch comes from wun_gather_snippets_speed, which resamples
    the rated sources inside the same launch (speed_descriptors; rates() shows the next batch's rate indices); with "pitch_shift"
    or "time_stretch" (vocoder_descriptors; jobs() shows the next batch's jobs) every source plane carries a tail of B slots, one
    wun_time_stretch call per batch stretches the jobs' spans into the slots of their rows, and the same gather reads them
    there -- resampling them for pitch_shift.  Any other partition: a finite iterator over every hop of every track in order, the
    remainder dropped -- the batches of get_dataset(..., partition, ...); a call behind the last batch raises StopIteration.
    descriptors() shows the next batch's table without touching the GPU."""

    def __init__(self, model_config, tracks, input_frames, output_frames, batch_size, device, seed=1337, rng=None,
                 augment=None, partition="train"):
        import torch
        self.cfg = model_config
        self.names = list(model_config["source_names"])
        self.t_in, self.t_out = int(input_frames), int(output_frames)
        if self.t_out > self.t_in or (self.t_in - self.t_out) % 2 != 0:
            raise ValueError("input_frames - output_frames must be even and >= 0")
        self.pad = (self.t_in - self.t_out) // 2
        self.batch = int(batch_size)
        self.device = torch.device(device)
        self.partition = partition
        active = check_augment(model_config, augment)
        if active and partition != "train":
            raise ValueError("augment applies to the train partition only")
        if self.device.type != "cuda":
            raise RuntimeError("FusedSnippetSource gathers its batches with a HIP kernel; there is no CPU fallback "
                               "(got device %s)" % self.device)
        from . import _lib
        self._lib_mod, self._lib = _lib, _lib.load()
        lens, cat = [], {k: [] for k in self.names + ["mix"]}
        for t in tracks:
            p = pad_track(t, self.pad)
            n = p["mix"].shape[0]
            if n <= self.t_in:
                raise ValueError("track shorter than the network input")
            lens.append(n)
            for k in cat:
                cat[k].append(p[k])
        self.channels = int(cat["mix"][0].shape[1])
        self.plane_frames = int(sum(lens))
        # the vocoder's slots: B per source plane behind the tracks, each as long as the longest job output (only with its keys)
        self.vocoder_fft = active.get("vocoder_fft")
        self.bank_rates = active.get("bank_rates", active.get("speed_rates", ()))
        self.slot_frames = 0
        if self.vocoder_fft is not None:
            outs = [speed_source_frames(self.t_in, up, down) for up, down in active.get("pitch_shift_rates", ())]
            self.slot_frames = max(outs + [self.t_in] if "time_stretch" in active else outs)
        self.gather_frames = self.plane_frames + self.batch * self.slot_frames      # what the gather may address
        tail = self.batch * self.slot_frames

        def plane(k, parts):
            if tail and k != "mix":
                parts = parts + [np.zeros((tail, self.channels), np.float32)]
            return torch.from_numpy(np.concatenate(parts)).to(self.device)
        self.data = {k: plane(k, v) for k, v in cat.items()}
        self._planes = (_lib.C.c_void_p * len(self.names))(*[self.data[k].data_ptr() for k in self.names])
        rng = rng if rng is not None else np.random.default_rng(seed)
        if partition == "train":
            self.mix_mode = int(bool(model_config["augmentation"]) or bool(active))
            self.stream = vocoder_descriptors(model_config, lens, self.t_in, self.t_out, rng, augment,
                                              np.random.default_rng([seed, 1]))
        else:
            self.mix_mode = 0
            self.stream = self._ordered(snippet_descriptors(model_config, lens, self.t_in, self.t_out, partition, rng), lens)
        self._next = self._next_rates = self._next_jobs = None
        self._no_jobs = np.zeros((self.batch, len(self.names), 4), dtype=np.int64)
        self._no_jobs.setflags(write=False)
        self._scratch = None
        if self.vocoder_fft is not None:                 # allocated once: every source of every row a job of the longest output
            from . import vocoder
            worst = np.zeros(self.batch * len(self.names), vocoder.JOB_DTYPE)
            worst["n_out"], worst["num"], worst["den"] = self.slot_frames, 1, 1
            self._scratch = torch.empty(vocoder.scratch_floats(worst, self.channels, *self.vocoder_fft), dtype=torch.float32,
                                        device=self.device)
        # the rate bank of wun_gather_snippets_speed: one table per ratio, designed and uploaded once
        self.speed_rates = active.get("speed_rates", ())     # (bank_rates: these, then pitch_shift's)
        self._bank = None
        self._unit_rates = np.zeros((self.batch, len(self.names)), dtype=np.uint8)
        self._unit_rates.setflags(write=False)
        if self.bank_rates:
            from . import resample
            self._tables = [resample._table(up, down, self.device) for up, down in self.bank_rates]
            self._bank = _lib.WunSpeedBank()
            self._bank.n = len(self.bank_rates)
            for i, ((up, down), tab) in enumerate(zip(self.bank_rates, self._tables)):
                self._bank.up[i], self._bank.down[i], self._bank.table[i] = up, down, tab.data_ptr()

    def _ordered(self, stream, lens):
        offset = np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))[:-1]])
        for ti, pos, _ in stream:
            rec = np.zeros(len(self.names), dtype=SNIPPET_DTYPE)
            rec["start"] = offset[ti] + pos
            rec["gain"] = 1.0
            yield rec, 0, np.zeros(len(self.names), dtype=np.uint8), self._no_jobs[0]

    def descriptors(self):
        """The next batch's table, SNIPPET_DTYPE [B, S] (host only: nothing is launched).  StopIteration behind the last
        whole batch of a finite partition.  A source with a job (jobs()) starts at its slot: frame plane_frames + b slot_frames
        of its plane, where the job's output lies when the gather runs."""
        if self._next is None:
            rows, rates, jobs = [], [], []
            for rec, _, rate, job in self.stream:
                rows.append(rec)
                rates.append(rate)
                jobs.append(job)
                if len(rows) == self.batch:
                    break
            if len(rows) < self.batch:                   # remainder dropped (batch_and_drop_remainder, Datasets.py:215)
                raise StopIteration
            self._next = np.ascontiguousarray(np.stack(rows))
            # (without a bank every rate is the shared zero row: one table for all batches, nothing stacked)
            self._next_rates = np.ascontiguousarray(np.stack(rates)) if self._bank is not None else self._unit_rates
            self._next_jobs = np.ascontiguousarray(np.stack(jobs)) if self.vocoder_fft is not None else self._no_jobs
            if self.vocoder_fft is not None:
                slot = self.plane_frames + self.slot_frames * np.arange(self.batch, dtype=np.int64)
                self._next["start"] = np.where(self._next_jobs[:, :, 1] > 0, slot[:, None], self._next["start"])
        return self._next

    def rates(self):
        """The next batch's rate indices, uint8 [B, S] (0 = unit rate, i = speed_rates[i - 1]); all zero without an active
        augment["speed"].  Host only, like descriptors(), and about the same batch."""
        self.descriptors()
        return self._next_rates

    def jobs(self):
        """The next batch's vocoder jobs, int64 [B, S, 4] of (span_start, n_span, num, den) in frames of the source's plane
        (n_span = 0: no job); all zero without an active "pitch_shift" / "time_stretch".  Host only, like descriptors(), and
        about the same batch: the job of (b, s) is stretched into slot b of plane s, n_src frames of it for a rated source
        (rates()), Tin otherwise."""
        self.descriptors()
        return self._next_jobs

    def job_table(self, jobs, rates=None):
        """The host table of wun_time_stretch (vocoder.JOB_DTYPE) for an int64 [B, S, 4] table of jobs (jobs()): the span of
        (b, s) in plane s into slot b of that plane, n_src frames of it for a rated source (`rates`, uint8 [B, S]), else Tin."""
        from . import vocoder
        jobs = np.asarray(jobs, dtype=np.int64)
        B, S, C = int(jobs.shape[0]), len(self.names), self.channels
        if jobs.shape != (B, S, 4) or B > self.batch:
            raise ValueError("jobs must be int64 [B <= %d, %d, 4], got %r" % (self.batch, S, jobs.shape))
        bs = np.argwhere(jobs[:, :, 1] > 0)
        if len(bs) and self.vocoder_fft is None:
            raise ValueError("a job needs a source built with augment['pitch_shift'] or augment['time_stretch']")
        table = np.zeros(len(bs), vocoder.JOB_DTYPE)
        for i, (b, s) in enumerate(bs):
            start, n_span, num, den = (int(v) for v in jobs[b, s])
            r = int(rates[b, s]) if rates is not None else 0
            n_out = speed_source_frames(self.t_in, *self.bank_rates[r - 1]) if r else self.t_in
            base = self.data[self.names[s]].data_ptr()
            table[i] = (base + 4 * C * start, base + 4 * C * (self.plane_frames + b * self.slot_frames), n_span, n_out, num, den)
        return table

    def stretch(self, jobs, rates=None):
        """One wun_time_stretch call on the current stream: the jobs of an int64 [B, S, 4] table (jobs()) into the slots of
        their rows.  Nothing is launched for a table without jobs."""
        from . import vocoder
        table = self.job_table(jobs, rates)
        if len(table):
            vocoder.run(table, self.channels, self.vocoder_fft[0], self.vocoder_fft[1], self._scratch, self.device)

    def gather(self, table, mix_mode, rates=None, jobs=None):
        """(mix, targets) of a SNIPPET_DTYPE table [B, S] through wun_gather_snippets, on the current stream; with `rates`
        (uint8 [B, S]) that hold a non-zero, through wun_gather_snippets_speed and this source's rate bank; with `jobs`
        (stretch) the vocoder's call first, on the same stream."""
        import torch
        table = np.ascontiguousarray(table, dtype=SNIPPET_DTYPE)
        B, S, C = int(table.shape[0]), len(self.names), self.channels
        if jobs is not None:
            self.stretch(jobs, rates)
        if rates is not None:
            rates = np.ascontiguousarray(rates, dtype=np.uint8)
            if rates.shape != (B, S):
                raise ValueError("rates must be uint8 [B, S] = %r, got %r" % ((B, S), rates.shape))
            if not rates.any():
                rates = None
            elif self._bank is None:
                raise ValueError("a non-zero rate needs a source built with augment['speed']")
        with torch.cuda.device(self.device):
            mix = torch.empty((B, self.t_in, C), dtype=torch.float32, device=self.device)
            targets = torch.empty((S, B, self.t_out, C), dtype=torch.float32, device=self.device)
            stream = self._lib_mod.stream(self.device)
            if rates is None:
                self._lib_mod.check(self._lib.wun_gather_snippets(
                    self._planes, self.data["mix"].data_ptr(), self.gather_frames, C, S, B, self.t_in, self.t_out,
                    table.ctypes.data, int(mix_mode), mix.data_ptr(), targets.data_ptr(), stream))
            else:
                self._lib_mod.check(self._lib.wun_gather_snippets_speed(
                    self._planes, self.data["mix"].data_ptr(), self.gather_frames, C, S, B, self.t_in, self.t_out,
                    table.ctypes.data, rates.ctypes.data, self._lib_mod.C.addressof(self._bank), int(mix_mode), mix.data_ptr(),
                    targets.data_ptr(), stream))
        return mix, targets

    def __call__(self):
        table = self.descriptors()
        rates = self._next_rates if self._bank is not None else None
        jobs = self._next_jobs if self.vocoder_fft is not None else None
        self._next = self._next_rates = self._next_jobs = None
        return self.gather(table, self.mix_mode, rates, jobs)

    def __iter__(self):
        return self

    def __next__(self):
        return self()
