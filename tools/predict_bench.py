#!/usr/bin/env python3
"""Full-track inference (Evaluate.predict, Evaluate.py:59-145): a synthetic 3-minute track through the M1+context separator,
hops batched 16 at a time, timed in ONE process on the same separator and the same samples:

  predict_track            evaluate.predict_track, host tiling (numpy pad / stack / scatter, one upload and download per batch)
  separate_track           evaluate.separate_track at mix_sr == expected_sr (tiling on the GPU, one upload, one download)
  host_resample+predict    a 44 100 Hz stereo file: scipy resample_poly down, predict_track, resample_poly back (the host path)
  separate_track_44100     the same file through separate_track (wun_resample in, wun_resample out)
  separate_track_stacked   the tiling separate_track used before wun_separate_track: torch.stack of strided views, get_output,
                           one strided copy per source and chunk (kept here only, as the yardstick of the default path)
  hop_x<m> / hop_track     separate_track(hop_frames = m default hops' output / "track"): a context model pays its context
                           once per hop; "convolved_per_output" = hops * input frames / track frames is the arithmetic the
                           measured time is to be read against

The arms are interleaved round by round; each figure is the minimum and the median over the rounds of a host clock around
work that ends in a device synchronise (the returned estimates are host arrays).  The resampler's own kernel time comes from
HIP events around one launch on the same track (bytes = input read once + output written once).  Prints one JSON line.
usage: tools/predict_bench.py [config] [rounds]      kernel-family times: rocprofv3 --kernel-trace --stats -- python tools/predict_bench.py
"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import wave_u_net_amd as wun
from wave_u_net_amd import resample as rs
from wave_u_net_amd.evaluate import _hop_positions, hop_geometry, predict_track, separate_track

name = sys.argv[1] if len(sys.argv) > 1 else "m1_context"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
cfg = wun.get_config(name)
sep = wun.UnetAudioSeparator(cfg, device="cuda:0")
sr = int(cfg["expected_sr"])
seconds = 180
C = 1 if cfg["mono_downmix"] else 2
rng = np.random.default_rng(0)
audio = rng.uniform(-0.5, 0.5, (seconds * sr, C)).astype(np.float32)               # at the model's rate, model's channels
file_sr = 44100 if sr != 44100 else 48000
song = rng.uniform(-0.5, 0.5, (seconds * file_sr, 2)).astype(np.float32)           # an ordinary stereo file


def host_path(x):
    v = np.mean(x, axis=1, keepdims=True) if C == 1 else x
    est = predict_track(cfg, sep, rs.resample(v, file_sr, sr), sr, batch_hops=16)
    out = {}
    for k, e in est.items():
        e = rs.resample(e, sr, file_sr)[:x.shape[0]]
        out[k] = np.tile(e, [1, 2]) if C == 1 else e
    return out


def stacked_path(x, batch_hops=16):
    """separate_track at expected_sr as it ran before wun_separate_track (same results, bit for bit)."""
    dev = sep.device
    x = torch.from_numpy(x).to(dev)
    tin, tout = hop_geometry(cfg, sep, x.shape[0])
    n_frames = max(int(x.shape[0]), tin)
    pad = (tin - tout) // 2
    padded = torch.zeros((n_frames + 2 * pad, C), dtype=torch.float32, device=dev)
    padded[pad:pad + x.shape[0]] = x
    names = list(cfg["source_names"])
    preds = torch.zeros((len(names), n_frames, C), dtype=torch.float32, device=dev)
    positions = _hop_positions(n_frames, tout)
    for k in range(0, len(positions), batch_hops):
        chunk = positions[k:k + batch_hops]
        outs = sep.get_output(torch.stack([padded[p:p + tin] for p in chunk]), False)
        run = 1
        while run < len(chunk) and chunk[run] == chunk[0] + run * tout:
            run += 1
        for si, n in enumerate(names):
            o = outs[n]
            preds[si, chunk[0]:chunk[0] + run * tout].view(run, tout, C).copy_(o[:run])
            for bi in range(run, len(chunk)):
                preds[si, chunk[bi]:chunk[bi] + tout] = o[bi]
    host = preds[:, :x.shape[0]].cpu().numpy()
    return {n: host[si] for si, n in enumerate(names)}


def convolved_per_output(hop):
    tin, tout = hop_geometry(cfg, sep, audio.shape[0], hop)
    n_frames = max(audio.shape[0], tin if hop is None else tout)
    return round(len(_hop_positions(n_frames, tout)) * tin / float(audio.shape[0]), 3)


tout0 = hop_geometry(cfg, sep, audio.shape[0])[1]
long_hops = [("hop_x%d" % m, m * tout0) for m in (2, 4, 10, 32)] + [("hop_track", "track")]
arms = [("predict_track", lambda: predict_track(cfg, sep, audio, sr, batch_hops=16)),
        ("separate_track", lambda: separate_track(cfg, sep, audio, sr, batch_hops=16)),
        ("host_resample+predict", lambda: host_path(song)),
        ("separate_track_44100", lambda: separate_track(cfg, sep, song, file_sr, batch_hops=16)),
        ("separate_track_stacked", lambda: stacked_path(audio))]
arms += [(k, (lambda h: lambda: separate_track(cfg, sep, audio, sr, batch_hops=16, hop_frames=h))(h)) for k, h in long_hops]

for _, fn in arms:                                                                  # warm-up: every plan and kernel of the window
    fn()
torch.cuda.synchronize()
times = {k: [] for k, _ in arms}
for _ in range(rounds):
    for k, fn in arms:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times[k].append(time.perf_counter() - t0)

# results must not change: the device path against the host path on the timed track
a, b = predict_track(cfg, sep, audio, sr, batch_hops=16), separate_track(cfg, sep, audio, sr, batch_hops=16)
same = all(np.array_equal(a[k], b[k]) for k in a)
c = stacked_path(audio)
same_stacked = all(np.array_equal(c[k], b[k]) for k in b)

# the resampler kernel alone: the 44 100 Hz stereo song -> the model's rate and channels
up, down = rs.ratio(file_sr, sr)
x = torch.from_numpy(song).cuda()
y = torch.zeros((rs.frames(song.shape[0], up, down), C), device="cuda")
rs.resample_into(x, y, 0, y.shape[0], up, down)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
kt = []
for _ in range(20):
    ev[0].record(); rs.resample_into(x, y, 0, y.shape[0], up, down); ev[1].record()
    torch.cuda.synchronize()
    kt.append(ev[0].elapsed_time(ev[1]))
nbytes = x.numel() * 4 + y.numel() * 4

res = {"tool": "predict_bench", "config": name, "seconds_of_audio": seconds, "expected_sr": sr, "file_sr": file_sr,
       "model_channels": C, "batch_hops": 16, "rounds": rounds,
       "ms": {k: {"min": round(min(v) * 1e3, 2), "median": round(float(np.median(v)) * 1e3, 2)} for k, v in times.items()},
       "separate_track_bit_equal_to_predict_track": bool(same),
       "separate_track_bit_equal_to_stacked_path": bool(same_stacked),
       "convolved_per_output": dict([("separate_track", convolved_per_output(None))] + [(k, convolved_per_output(h)) for k, h in long_hops]),
       "resample_kernel": {"up": up, "down": down, "c_in": 2, "c_out": C, "frames_in": int(song.shape[0]),
                           "event_ms_min": round(min(kt), 4), "event_ms_median": round(float(np.median(kt)), 4),
                           "algorithmic_bytes": nbytes, "GBps_at_min": round(nbytes / (min(kt) * 1e-3) / 1e9, 1)}}
print(json.dumps(res))
