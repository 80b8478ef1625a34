"""GPU tests of whole-track separation through the C ABI (include/wun.h: wun_forward_windows, wun_scatter_windows,
wun_separate_track) and of what the package builds on it: get_output_windows against get_output on the stacked batch (bit for
bit), scatter_windows against a numpy loop, separate_track at the default hops against predict_track (bit for bit), long hops
against the float64 oracle on the same windows, a plain C caller against the Python path, and run-to-run reproducibility."""
import os
import subprocess

import numpy as np
import pytest
import torch

from _observed import record
from oracle import shapes, waveunet_torch as wt
from oracle.golden_params import GOLDEN_CASES, golden_params

import wave_u_net_amd as wun
from wave_u_net_amd import resample as rs
from wave_u_net_amd.evaluate import _hop_positions, hop_geometry, predict_track, separate_track
from wave_u_net_amd.separator import UnetAudioSeparator

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_TOL = 5e-6       # absolute, network outputs against the float64 oracle (tests/test_gpu_parity.py)


def _small(chan, mode="f32", **over):
    cfg = wun.get_config("baseline", num_layers=3, num_initial_filters=8, context=True, output_type="difference",
                         mono_downmix=(chan == 1), num_frames=40, compute_dtype=mode, **over)
    sep = UnetAudioSeparator(cfg, device="cuda:0")
    i, o = sep.get_padding(np.array([1, 40, 0]))
    return cfg, sep, int(i[1]), int(o[1])


def _shifted_track(frames, chan, shift, seed):
    """[frames, chan] random track whose first float sits `shift` floats past a 16-byte boundary."""
    flat = torch.from_numpy(np.random.default_rng(seed).uniform(-1.5, 1.5, frames * chan + 8).astype(np.float32)).cuda()
    base = (flat.data_ptr() // 4) % 4
    k = (shift - base) % 4
    track = flat[k:k + frames * chan].view(frames, chan)
    assert (track.data_ptr() // 4) % 4 == shift and track.is_contiguous()
    return track


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("chan", [1, 2])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_forward_windows_is_forward_on_the_stacked_batch(mode, chan, shift):
    """Row b read from the track at any alignment of positions[b] * C (0 .. 3 floats past a 16-byte boundary, here through
    the positions AND the track's own address), a window that ends exactly at track_frames, and npos < batch (zero rows)."""
    cfg, sep, tin, tout = _small(chan, mode)
    frames = 3 * tin + 5
    track = _shifted_track(frames, chan, shift, 10 * shift + chan)
    positions = [0, 1, 2, 3, tin + 7, frames - tin]
    seen = {((track.data_ptr() // 4) + p * chan) % 4 for p in positions}
    assert seen == ({0, 1, 2, 3} if chan == 1 else {shift % 2, shift % 2 + 2})
    B = len(positions)
    batch = torch.stack([track[p:p + tin] for p in positions])
    want = {k: v.clone() for k, v in sep.get_output(batch, False).items()}
    assert sep.effective_dtype == mode
    got = sep.get_output_windows(track, positions, False, frames=tin)
    for k in want:
        assert got[k].shape == (B, tout, chan)
        assert torch.equal(got[k], want[k]), (k, (got[k] - want[k]).abs().max().item())
    # training = True (no AudioClip) goes the same way
    want = {k: v.clone() for k, v in sep.get_output(batch, True).items()}
    got = sep.get_output_windows(track, positions, True, frames=tin)
    assert all(torch.equal(got[k], want[k]) for k in want)
    # npos < batch: rows past the positions are zeros and give what zeros give
    short = torch.zeros_like(batch)
    short[:4] = batch[:4]
    want = {k: v.clone() for k, v in sep.get_output(short, False).items()}
    got = sep.get_output_windows(track, positions[:4], False, frames=tin, batch=B)
    assert all(torch.equal(got[k], want[k]) for k in want)
    with pytest.raises(ValueError):
        sep.get_output_windows(track, [frames - tin + 1], False, frames=tin)


def _numpy_scatter(outs, positions, preds, tout):
    for b, p in enumerate(positions):                                            # hops in order: written last wins
        preds[:, p:p + tout] = outs[:, b]
    return preds


@pytest.mark.parametrize("chan", [1, 2])
def test_scatter_windows_is_the_numpy_loop(chan):
    """Known estimates are planted in the separator's own output buffer (sep._outs, its cache of per-plan buffers: the only
    way to give the kernel bit-exact inputs that no network produced)."""
    cfg, sep, tin, tout = _small(chan)
    S = len(cfg["source_names"])
    cases = [
        ("regular hops, overlapping last hop", [0, tout, 2 * tout, 3 * tout - 5], 3 * tout + tout - 5),
        ("track of whole hops", [0, tout, 2 * tout], 3 * tout),
        ("last hop coincides with a regular hop", [0, tout, tout], 2 * tout + 9),
        ("one hop", [3], tout + 11),
        ("unordered, overlapping, with gaps", [50, 0, 30, 4 * tout + 1, 33, 4 * tout - 2], 6 * tout + 3),
        ("later hop covers an earlier one's middle", [10, 10 + tout // 3, 10 + tout // 2, 10], 3 * tout),
    ]
    rng = np.random.default_rng(chan)
    for what, positions, pred_frames in cases:
        B = len(positions)
        track = torch.zeros((pred_frames + tin, chan), device="cuda:0")
        sep.get_output_windows(track, [0] * B, False, frames=tin)               # the plan's output buffer
        outs = rng.uniform(-1, 1, (S, B, tout, chan)).astype(np.float32)
        sep._outs[(B, tin)].copy_(torch.from_numpy(outs))
        preds = torch.full((S, pred_frames, chan), -7.0, device="cuda:0")
        sep.scatter_windows(positions, preds, frames=tin)
        want = _numpy_scatter(outs, positions, np.full((S, pred_frames, chan), -7.0, np.float32), tout)
        assert np.array_equal(preds.cpu().numpy(), want), what
    with pytest.raises(ValueError):
        sep.scatter_windows([pred_frames - tout + 1] * B, preds, frames=tin)


def _golden_separator(name):
    case = GOLDEN_CASES[name]
    ocfg = shapes.finalize_config(dict(shapes.BASE_MODEL_CONFIG, **case["cfg"]))
    cfg = wun.get_config("baseline", num_frames=case["frames"], **case["cfg"])
    params = golden_params(ocfg, case["seed"])
    sep = UnetAudioSeparator(cfg, device="cuda:0")
    i, o = shapes.get_padding(ocfg, [1, case["frames"], 0])
    sep._plan(1, i[1]); sep._active = sep._plans[(1, i[1])]
    sep.load_variables(params)
    return cfg, ocfg, sep, params, int(i[1]), int(o[1])


@pytest.mark.parametrize("batch_hops", [3, 4, 16])
@pytest.mark.parametrize("chan", [1, 2])
@pytest.mark.parametrize("name", ["baseline_context_small", "linear_act_eval_small", "baseline_small", "baseline_stereo_small"])
def test_default_hops_equal_predict_track(name, chan, batch_hops):
    """8 hops: chunks of 3 + 3 + 2 (a short last chunk: the plan of its batch, chunk by chunk), 4 + 4 and 8 (one
    wun_separate_track call)."""
    cfg, ocfg, sep, params, tin, tout = _golden_separator(name)
    n = 7 * tout + 17
    audio = np.random.default_rng(3).uniform(-1.5, 1.5, (n, chan)).astype(np.float32)
    want = predict_track(cfg, sep, audio, cfg["expected_sr"], batch_hops=batch_hops)
    got = separate_track(cfg, sep, audio, cfg["expected_sr"], batch_hops=batch_hops)
    c_model = 1 if cfg["mono_downmix"] else 2
    for s in cfg["source_names"]:
        w = np.tile(want[s], [1, chan]) if (c_model == 1 and chan > 1) else want[s]
        assert got[s].shape == w.shape and np.array_equal(got[s], w), s


@pytest.mark.parametrize("name", ["baseline_context_small", "baseline_stereo_small"])
def test_default_hops_equal_predict_track_from_44100(name):
    """A 44 100 Hz file and a 22 050 Hz model: the track separate_track tiles is the device-resampled one, and on it the
    estimates equal predict_track's bit for bit -- before and after the way back to 44 100 Hz."""
    cfg, ocfg, sep, params, tin, tout = _golden_separator(name)
    chan = 1 if cfg["mono_downmix"] else 2
    n = 2 * (7 * tout + 17) + 1
    audio = np.random.default_rng(6).uniform(-1.0, 1.0, (n, chan)).astype(np.float32)
    mid_in = rs.resample(torch.from_numpy(audio).cuda(), 44100, 22050).cpu().numpy()
    mid = predict_track(cfg, sep, mid_in, 22050, batch_hops=3)
    same = separate_track(cfg, sep, mid_in, 22050, batch_hops=3)
    got = separate_track(cfg, sep, audio, 44100, batch_hops=3)
    for s in cfg["source_names"]:
        assert np.array_equal(same[s], mid[s]), s
        back = rs.resample(torch.from_numpy(mid[s]).cuda(), 22050, 44100).cpu().numpy()[:n]
        assert got[s].shape == back.shape == (n, chan) and np.array_equal(got[s], back), s


def _oracle_tiling(ocfg, params, audio, tin, tout):
    """predict_track's loop with one float64 oracle evaluation per hop window."""
    tp = wt.params_to_torch(params, torch.float64)
    n_frames = max(audio.shape[0], tout)
    x = np.zeros((n_frames, audio.shape[1]), np.float64)
    x[:audio.shape[0]] = audio
    pad = (tin - tout) // 2
    padded = np.pad(x, [(pad, pad), (0, 0)])
    preds = {s: np.zeros((n_frames, audio.shape[1])) for s in ocfg["source_names"]}
    positions = _hop_positions(n_frames, tout)
    for p in positions:
        outs = wt.get_output(ocfg, tp, torch.from_numpy(np.ascontiguousarray(padded[None, p:p + tin])), False)
        for s in preds:
            preds[s][p:p + tout] = outs[s][0].detach().numpy()
    return {s: v[:audio.shape[0]] for s, v in preds.items()}, len(positions)


@pytest.mark.parametrize("hop", ["mid", "track"])
@pytest.mark.parametrize("name", ["baseline_context_small", "baseline_small"])                 # context / same padding
def test_long_hops_against_the_float64_oracle(name, hop):
    cfg, ocfg, sep, params, tin, tout = _golden_separator(name)
    chan = 1 if cfg["mono_downmix"] else 2
    n = 7 * tout + 17
    audio = np.random.default_rng(12).uniform(-1.0, 1.0, (n, chan)).astype(np.float32)
    hop_frames = "track" if hop == "track" else 3 * tout
    lin, lout = hop_geometry(cfg, sep, n, hop_frames)
    assert lout >= (n if hop == "track" else 3 * tout) and lin - lout == tin - tout
    got = separate_track(cfg, sep, audio, cfg["expected_sr"], batch_hops=2, hop_frames=hop_frames)
    ref, hops = _oracle_tiling(ocfg, params, audio, lin, lout)
    assert hops == (1 if hop == "track" else -(-n // lout))
    for s in cfg["source_names"]:
        err = np.abs(got[s].astype(np.float64) - ref[s]).max()
        record("long_hops_vs_float64_oracle", "%s/%s/%s" % (name, hop, s), err, OUT_TOL)
        assert got[s].shape == (n, chan) and err <= OUT_TOL, (s, err)


def _pattern(n, mul):
    """tests/track_smoke.c pattern(): 16 bits of a multiplicative hash, every step exact in float32."""
    i = np.arange(n, dtype=np.uint64)
    h = (((i * np.uint64(mul)) & np.uint64(0xFFFFFFFF)) >> np.uint64(8)) & np.uint64(0xFFFF)
    return (h.astype(np.float32) / np.float32(65536.0) - np.float32(0.5)) * np.float32(0.25)


def test_c_program_separates_a_track(tmp_path):
    """tests/track_smoke.c -- hipMalloc + the C ABI, no Python -- against separate_padded with the same parameter pattern.
    Both sides run wun_separate_track: this checks the CALLER (a C program can drive the entry with its own buffers and gets
    the Python path's bits); what the entry computes is anchored by the tests above and below."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    libdir = os.path.join(ROOT, "wave-u-net_amd")
    exe, out = os.path.join(str(tmp_path), "track_smoke"), os.path.join(str(tmp_path), "preds.f32")
    cmd = [hipcc, "-x", "c", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "track_smoke.c"), "-L" + libdir, "-lwun", "-Wl,-rpath," + libdir, "-o", exe]
    res = subprocess.run(cmd, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert res.returncode == 0, res.stdout.decode("utf-8", "replace")[-2000:]
    res = subprocess.run(["timeout", "-k", "10", "120", exe, out], timeout=150, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert res.returncode == 0, res.stdout.decode("utf-8", "replace")[-2000:]
    assert b"track_smoke: ok" in res.stdout

    cfg = wun.get_config("baseline", num_layers=3, num_initial_filters=8, context=True, mono_downmix=False, num_frames=40)
    sep = UnetAudioSeparator(cfg, device="cuda:0")
    i, o = sep.get_padding(np.array([1, 40, 0]))
    tin, tout = int(i[1]), int(o[1])
    plan = sep._plan(3, tin)
    sep._ensure_variables(plan)
    sep.params.copy_(torch.from_numpy(_pattern(int(plan.info.arena_floats), 2654435761)))
    n_frames, pad = 7 * tout + 17, (tin - tout) // 2
    track = np.zeros((n_frames + 2 * pad, 2), np.float32)
    track[pad:pad + n_frames] = (np.float32(4.0) * _pattern(n_frames * 2, 40503)).reshape(n_frames, 2)
    want = sep.separate_padded(torch.from_numpy(track), n_frames, 3, frames=tin).cpu().numpy()
    got = np.fromfile(out, dtype=np.float32)
    assert got.size == want.size and np.all(np.isfinite(got))
    assert np.array_equal(got.reshape(want.shape), want)
    assert np.abs(want).max() > 1e-3                                             # not a trivially silent network


def test_separate_track_is_reproducible_on_fresh_workspaces():
    """(Fresh workspaces: the separator's cached buffers -- sep._ws / sep._outs -- are taken out and kept alive, so the second
    run allocates new memory.)"""
    cfg, ocfg, sep, params, tin, tout = _golden_separator("baseline_stereo_small")
    n_frames, pad = 7 * tout + 17, (tin - tout) // 2
    track = torch.zeros((n_frames + 2 * pad, 2), device="cuda:0")
    track[pad:pad + n_frames] = torch.from_numpy(np.random.default_rng(4).uniform(-1, 1, (n_frames, 2)).astype(np.float32)).cuda()
    first = sep.separate_padded(track, n_frames, 3, frames=tin).clone()
    held = (sep._ws.pop((3, tin)), sep._outs.pop((3, tin)))                      # kept alive: the next ones are new memory
    second = sep.separate_padded(track, n_frames, 3, frames=tin)
    assert sep._ws[(3, tin)].data_ptr() != held[0].data_ptr()
    assert torch.equal(first, second)
    # ... and the one call is the chunk-by-chunk composition of its two halves
    third = torch.full_like(first, float("nan"))
    positions = _hop_positions(n_frames, tout)
    for k in range(0, len(positions), 3):
        sep.get_output_windows(track, positions[k:k + 3], False, frames=tin, batch=3)
        sep.scatter_windows(positions[k:k + 3], third, frames=tin, batch=3)
    assert torch.equal(first, third)
