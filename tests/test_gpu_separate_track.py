"""GPU tests of evaluate.separate_track -- Evaluate.predict (Evaluate.py:59-80) around predict_track (:82-145) on the device,
for audio at any sample rate: bit-equal to predict_track at the model's rate, the documented composition
resample -> predict_track -> resample back at 44 100 -> 22 050 -> 44 100 Hz, and the `predict` command end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile
from scipy.signal import firwin, resample_poly

from oracle import shapes, waveunet_torch as wt
from oracle.golden_params import GOLDEN_CASES, golden_params
from oracle.predict_np import predict_track_ref

import wave_u_net_amd as wun
from wave_u_net_amd import resample as rs
from wave_u_net_amd.evaluate import predict_track, separate_track

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _separator(name):
    from wave_u_net_amd.separator import UnetAudioSeparator
    case = GOLDEN_CASES[name]
    ocfg = shapes.finalize_config(dict(shapes.BASE_MODEL_CONFIG, **case["cfg"]))
    frames = case["frames"]
    cfg = wun.get_config("baseline", num_frames=frames, **case["cfg"])
    params = golden_params(ocfg, case["seed"])
    sep = UnetAudioSeparator(cfg, device="cuda:0")
    i, o = shapes.get_padding(ocfg, [1, frames, 0])
    sep._plan(1, i[1]); sep._active = sep._plans[(1, i[1])]
    sep.load_variables(params)
    return cfg, ocfg, sep, params, i, o


@pytest.mark.parametrize("length", ["long", "short"])
@pytest.mark.parametrize("chan", [1, 2])
@pytest.mark.parametrize("name", ["baseline_context_small", "linear_act_eval_small", "baseline_small"])
def test_equals_predict_track_at_expected_sr(name, chan, length):
    cfg, ocfg, sep, params, i, o = _separator(name)
    frames = GOLDEN_CASES[name]["frames"]
    n_frames = 5 * int(o[1]) + 17 if length == "long" else int(i[1]) - 7     # short: below input_frames
    audio = np.random.default_rng(3).uniform(-1.5, 1.5, (n_frames, chan)).astype(np.float32)
    want = predict_track(cfg, sep, audio, cfg["expected_sr"], batch_hops=3)
    got = separate_track(cfg, sep, audio, cfg["expected_sr"], batch_hops=3)
    tp = wt.params_to_torch(params, torch.float32)

    def run(part):
        outs = wt.get_output(ocfg, tp, torch.from_numpy(np.ascontiguousarray(part)), False)
        return {k: v.numpy() for k, v in outs.items()}
    ref = predict_track_ref(dict(ocfg, num_frames=frames), run, audio, i, o)
    c_model = 1 if cfg["mono_downmix"] else 2
    c_out = chan if c_model == 1 else 2
    assert list(got.keys()) == list(ocfg["source_names"])
    for n in ocfg["source_names"]:
        w, r = want[n], ref[n]
        if c_model == 1 and chan > 1:                                         # Evaluate.py:66-67
            w, r = np.tile(w, [1, chan]), np.tile(r, [1, chan])
        assert got[n].dtype == np.float32 and got[n].shape == w.shape == (n_frames, c_out)
        assert np.array_equal(got[n], w)
        assert np.abs(got[n] - r).max() <= 2e-4


@pytest.mark.parametrize("chan", [1, 2])
@pytest.mark.parametrize("name", ["baseline_context_small", "baseline_stereo_small"])        # mono_downmix True / False
def test_44100_file_is_the_three_step_composition(name, chan):
    """separate_track on a 44 100 Hz file with a 22 050 Hz model against (a) resample() of the channel-mapped input on the
    device, (b) predict_track on the downloaded result, (c) resample() of every estimate back, trimmed to the input.
    (a): the kernel's 2 -> 1 / 1 -> 2 mapping is bit-equal to the 1 -> 1 / 2 -> 2 call on the host-mapped fp32 signal
    (tests/test_gpu_resample.py), so (b) sees the same samples in both paths and is compared bit for bit on them.
    (c): both paths resample the same estimate with the same kernel; each lies within the bound of the kernel test
    of the float64 oracle, so they differ by at most twice that bound: 2 ((K + 2) 2^-24 (|h| * |v|) + 2^-24 |y64|)."""
    cfg, ocfg, sep, params, i, o = _separator(name)
    assert cfg["expected_sr"] == 22050
    mono = bool(cfg["mono_downmix"])
    n = 2 * (5 * int(o[1]) + 17) + 1                                          # odd: the way back yields one frame more
    audio = np.random.default_rng(6).uniform(-1.0, 1.0, (n, chan)).astype(np.float32)
    got = separate_track(cfg, sep, audio, 44100, batch_hops=3)

    if mono:
        mapped = audio if chan == 1 else ((audio[:, 0] + audio[:, 1]) / np.float32(2))[:, None]
    else:
        mapped = audio if chan == 2 else np.tile(audio, [1, 2])
    mid_in = rs.resample(torch.from_numpy(mapped).cuda(), 44100, 22050).cpu().numpy()          # (a)
    assert mid_in.shape[0] == (n + 1) // 2
    mid = predict_track(cfg, sep, mid_in, 22050, batch_hops=3)                                 # (b)
    same = separate_track(cfg, sep, mid_in, 22050, batch_hops=3)                               # (b) bit for bit
    up, down = rs.ratio(22050, 44100)
    K = rs.design(up, down).shape[1]
    habs = np.abs(firwin(20 * max(up, down) + 1, 1.0 / max(up, down), window=("kaiser", 5.0)))
    c_out = chan if mono else 2                        # a stereo model on a mono file keeps its two channels (reference)
    assert list(got.keys()) == list(cfg["source_names"])
    for s in cfg["source_names"]:
        assert np.array_equal(same[s], mid[s])
        back = rs.resample(torch.from_numpy(mid[s]).cuda(), 22050, 44100).cpu().numpy()[:n]    # (c)
        if mono and chan > 1:
            back = np.tile(back, [1, chan])
        assert got[s].dtype == np.float32 and got[s].shape == back.shape == (n, c_out)
        v = mid[s].astype(np.float64)
        y64 = resample_poly(v, up, down, axis=0)[:n]
        mag = resample_poly(np.abs(v), up, down, axis=0, window=habs)[:n]
        bound = 2.0 * ((K + 2) * 2.0 ** -24 * mag + 2.0 ** -24 * np.abs(y64))
        if bound.shape[1] != c_out:
            bound, y64 = np.tile(bound, [1, c_out]), np.tile(y64, [1, c_out])
        err = np.abs(got[s].astype(np.float64) - back.astype(np.float64))
        print("%s, %d ch, %s: max |fused - composed| = %.3g (bit-equal: %s), max |fused - float64 resampling| = %.3g"
              % (name, chan, s, err.max(), np.array_equal(got[s], back), np.abs(got[s] - y64).max()))
        assert np.all(err <= bound)
        assert np.all(np.abs(got[s] - y64) <= 0.5 * bound)                     # and the way back is a correct resampling


def test_predict_command_on_a_44100_wav(tmp_path):
    n = 30011
    pcm = (np.random.default_rng(0).uniform(-0.5, 0.5, (n, 2)) * 32767).astype(np.int16)
    src = os.path.join(str(tmp_path), "song.wav")
    out = os.path.join(str(tmp_path), "out")
    wavfile.write(src, 44100, pcm)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "wave_u_net_amd", "predict", "with", "cfg.baseline", "model_config.num_layers=4",
           "model_config.num_initial_filters=8", "model_config.num_frames=2048", "input_path=" + src, "output_path=" + out]
    res = subprocess.run(cmd, cwd=ROOT, env=env, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert res.returncode == 0, res.stdout.decode("utf-8", "replace")[-2000:]
    cfg = wun.get_config("baseline")
    assert cfg["expected_sr"] == 22050
    assert sorted(os.listdir(out)) == sorted("song.wav_%s.wav" % s for s in cfg["source_names"])
    for s in cfg["source_names"]:
        sr, est = wavfile.read(os.path.join(out, "song.wav_%s.wav" % s))
        assert sr == 44100 and est.shape == (n, 2) and est.dtype == np.float32
        assert np.all(np.isfinite(est)) and np.array_equal(est[:, 0], est[:, 1])       # mono model: duplicated estimate
