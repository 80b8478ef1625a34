"""GPU tests of blended separation end to end (include/wun.h: wun_separate_track_blend; UnetAudioSeparator.separate_padded_blend;
evaluate.separate_track(overlap=.., shifts=..)) on the smallest models the track tests use: the one call against
the forward pass per chunk followed by the numpy statement tests/_blend_np.py (bit for bit), two batch sizes against each other,
the untouched plain path, the post-filter on top, and the spectrogram U-Net through get_output + blend.blend_windows."""
import numpy as np
import pytest
import torch

import _blend_np as bn
import _postfilter_np as pf_np
from oracle import shapes
from oracle.golden_params import GOLDEN_CASES, golden_params

import wave_u_net_amd as wun
from wave_u_net_amd import blend, postfilter, spectral
from wave_u_net_amd.evaluate import predict_track, separate_track
from wave_u_net_amd.separator import UnetAudioSeparator

pytestmark = pytest.mark.gpu
MODELS = ["baseline_context_small", "baseline_stereo_small", "baseline_small"]     # context mono / context stereo / same padding


def _separator(name):
    case = GOLDEN_CASES[name]
    ocfg = shapes.finalize_config(dict(shapes.BASE_MODEL_CONFIG, **case["cfg"]))
    cfg = wun.get_config("baseline", num_frames=case["frames"], **case["cfg"])
    sep = UnetAudioSeparator(cfg, device="cuda:0")
    i, o = shapes.get_padding(ocfg, [1, case["frames"], 0])
    sep._plan(1, i[1]); sep._active = sep._plans[(1, i[1])]
    sep.load_variables(golden_params(ocfg, case["seed"]))
    return cfg, sep, int(i[1]), int(o[1])


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def _track(audio, tin, tout, v, offsets):
    """The zero-padded device track separate_track builds for a track at the model's rate, and its window list."""
    n, chan = audio.shape
    pad = (tin - tout) // 2
    wins = bn.window_list(tout, n, v, offsets)
    lead = max(offsets)
    frames = max(lead + n + 2 * pad, lead + max(p for p, _, _ in wins) + tin)
    track = torch.zeros((frames, chan), device="cuda:0")
    track[lead + pad:lead + pad + n] = torch.from_numpy(audio).cuda()
    return track, wins, lead


def _chunked_statement(sep, track, wins, lead, v, B, tin, n):
    """get_output_windows on the plan of batch B per chunk, then the numpy statement on what it returned."""
    S, chan = len(sep.source_names), track.shape[1]
    acc, den = np.zeros((S, n, chan), np.float32), np.zeros(n, np.float32)
    for k in range(0, len(wins), B):
        chunk = wins[k:k + B]
        outs = sep.get_output_windows(track, [lead + p for p, _, _ in chunk], False, frames=tin, batch=B)
        x = np.stack([outs[name].cpu().numpy() for name in sep.source_names])
        bn.accumulate(x, [(p, b, f) for b, (p, _, f) in enumerate(chunk)], v, acc, den)
    return bn.finish(acc, den)


@pytest.mark.parametrize("overlap, shifts", [(0.25, None), (0, [0, 3, 700]), (0.5, 2)])
@pytest.mark.parametrize("name", MODELS)
def test_one_call_is_forward_per_chunk_then_the_statement(name, overlap, shifts):
    cfg, sep, tin, tout = _separator(name)
    chan = 1 if cfg["mono_downmix"] else 2
    n, B = 7 * tout + 17, 3                       # longer than one hop's input: no extra zero padding
    audio = np.random.default_rng(3).uniform(-1.0, 1.0, (n, chan)).astype(np.float32)
    v = min(int(round(overlap * tout)), tout - 1)
    offsets = [0] if shifts is None else (blend.shift_offsets(shifts, tout + 5) if isinstance(shifts, int) else shifts)
    track, wins, lead = _track(audio, tin, tout, v, offsets)
    got = sep.separate_padded_blend(track, n, B, v, offsets, lead, frames=tin)
    want = _chunked_statement(sep, track, wins, lead, v, B, tin, n)
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want))
    assert np.abs(want).max() > 1e-3
    # ... and evaluate.separate_track is that call on that track
    kw = {"shifts": shifts, "max_shift": tout + 5} if isinstance(shifts, int) else {"shifts": shifts}
    dev = separate_track(cfg, sep, audio, cfg["expected_sr"], batch_hops=B, return_device=True, overlap=overlap, **kw)
    assert np.array_equal(_bits(dev), _bits(got))
    with pytest.raises(ValueError):
        sep.separate_padded_blend(track, n, B, v, offsets, lead - 1 if lead else -1, frames=tin)
    with pytest.raises(ValueError):
        sep.separate_padded_blend(track[:-1], n, B, v, offsets, lead, frames=tin)      # the last hop would leave the track


@pytest.mark.parametrize("name", MODELS)
def test_two_batch_sizes_agree(name):
    """batch_hops 2 and 5 on one track.  The forward's tilings depend on the plan's batch, so the bits may differ; the existing
    tests/test_gpu_separate_track.py compares across batches nowhere (its comparisons share a batch), so the bound is the
    issue's fallback: 1e-5 max |pred|."""
    cfg, sep, tin, tout = _separator(name)
    chan = 1 if cfg["mono_downmix"] else 2
    audio = np.random.default_rng(5).uniform(-1.0, 1.0, (7 * tout + 17, chan)).astype(np.float32)
    a = separate_track(cfg, sep, audio, cfg["expected_sr"], batch_hops=2, return_device=True, overlap=0.25, shifts=[0, 7])
    b = separate_track(cfg, sep, audio, cfg["expected_sr"], batch_hops=5, return_device=True, overlap=0.25, shifts=[0, 7])
    err, scale = (a - b).abs().max().item(), a.abs().max().item()
    print("%s: max |batch 2 - batch 5| = %.3g, bound %.3g" % (name, err, 1e-5 * scale))
    assert scale > 1e-3 and err <= 1e-5 * scale


@pytest.mark.parametrize("name", MODELS)
def test_plain_options_keep_the_plain_path_and_bits(name):
    cfg, sep, tin, tout = _separator(name)
    chan = 1 if cfg["mono_downmix"] else 2
    n = 7 * tout + 17
    audio = np.random.default_rng(3).uniform(-1.5, 1.5, (n, chan)).astype(np.float32)
    want = predict_track(cfg, sep, audio, cfg["expected_sr"], batch_hops=3)
    for kw in ({"overlap": 0, "shifts": None}, {"overlap": 0.0, "shifts": [0]}, {"shifts": 1}):
        got = separate_track(cfg, sep, audio, cfg["expected_sr"], batch_hops=3, **kw)
        assert all(np.array_equal(_bits(got[k]), _bits(want[k])) for k in want), kw
    # One pass without overlap through the blend entry: the grid differs from the plain one in the last hop only (it hangs
    # over the end instead of being re-aligned to n - Tout, where the plain path lets it overwrite the hop before it), and
    # with the same batch the frames before the plain path's last hop are its values (fmaf(1, x, +0) / 1 == x; compared as
    # values, since a -0 would come out as +0).
    pad = (tin - tout) // 2
    track = torch.zeros((n + 2 * pad + tout, chan), device="cuda:0")
    track[pad:pad + n] = torch.from_numpy(audio).cuda()
    plain = sep.separate_padded(track[:n + 2 * pad].contiguous(), n, 3, frames=tin).clone()
    one = sep.separate_padded_blend(track, n, 3, 0, [0], 0, frames=tin)
    last = n - tout
    assert last % tout != 0 and torch.equal(one[:, :last], plain[:, :last])
    assert not torch.equal(one[:, last:], plain[:, last:])                            # behind it the two grids differ


@pytest.mark.parametrize("name", ["baseline_context_small", "baseline_stereo_small"])
def test_postfilter_and_return_device_compose(name):
    cfg, sep, tin, tout = _separator(name)
    chan = 1 if cfg["mono_downmix"] else 2
    n = 7 * tout + 17
    audio = np.random.default_rng(8).uniform(-1.0, 1.0, (n, chan)).astype(np.float32)
    sr = cfg["expected_sr"]
    kw = dict(batch_hops=3, overlap=0.25, shifts=2, max_shift=tout // 2)
    plain = separate_track(cfg, sep, audio, sr, return_device=True, **kw)
    n_fft, hop = 64, 16
    f = postfilter.SoftMaskFilter(n_fft, hop)
    got = separate_track(cfg, sep, audio, sr, return_device=True, postfilter=f, **kw)
    mix = torch.from_numpy(audio).cuda()
    assert got.shape == plain.shape and torch.equal(got, f.apply(mix, plain)) and not torch.equal(got, plain)
    host = separate_track(cfg, sep, audio, sr, postfilter={"n_fft": n_fft, "hop": hop}, **kw)
    for si, k in enumerate(cfg["source_names"]):
        assert np.array_equal(host[k], got[si].cpu().numpy())
    # the soft-mask estimates still sum to the device's istft(stft(mix)), within that filter's own tolerance
    # (tests/test_gpu_postfilter.py test_filter_exact_cases: S 2^-22 max |mix| plus the inverse's bound)
    rt = spectral.istft(*spectral.stft(mix.view(1, 1, n, chan), n_fft, hop, centered=True), n, n_fft, hop, centered=True)[0, 0]
    lead, F = pf_np.framing(n, n_fft, hop, True)
    re, im = pf_np.stft(audio.T, n_fft, hop, lead, F)
    bound = pf_np.istft_bound(re, im, pf_np.istft(re, im, n, n_fft, hop, lead), n, n_fft, hop, lead).T
    err = (got.double().sum(0) - rt.double()).abs().cpu().numpy()
    assert (err <= got.shape[0] * 2.0 ** -22 * np.abs(audio).max() + bound).all()


def test_spectrogram_unet_blends_through_get_output():
    """The spectrogram U-Net has no plan: separate_track goes chunk by chunk through get_output and blend.blend_windows (the
    library's kernel on the device).  Its smallest legal frame count: the `skip` geometry of tests/test_gpu_specunet.py."""
    import _specunet_np as so
    from wave_u_net_amd import UnetSpectrogramSeparator
    n_fft, hop, L, nif, F, B = 64, 48, 2, 3, 8, 2
    T = (F - 1) * hop + n_fft
    cfg = wun.get_config("unet_spectrogram", num_layers=L, num_initial_filters=nif, spec_frame_len=n_fft, spec_hop=hop,
                         num_frames=T, batch_size=B)
    sep = UnetSpectrogramSeparator(cfg, device="cuda:0")
    sep.load_variables(so.random_variables(L, nif, seed=23 + L))
    tin, tout = (int(s[1]) for s in sep.get_padding(np.array([1, T, 0])))
    n = int(2.5 * T)
    audio = (0.3 * np.random.RandomState(4).randn(n, 1)).astype(np.float32)
    overlap, offsets = 0.25, [0, 5]
    v = int(round(overlap * tout))
    got = separate_track(cfg, sep, audio, cfg["expected_sr"], batch_hops=B, return_device=True, overlap=overlap, shifts=offsets)
    track, wins, lead = _track(audio, tin, tout, v, offsets)
    acc, den = np.zeros((len(sep.source_names), n, 1), np.float32), np.zeros(n, np.float32)
    for k in range(0, len(wins), B):
        chunk = wins[k:k + B]
        outs = sep.get_output(torch.stack([track[lead + p:lead + p + tin] for p, _, _ in chunk]), False)
        x = np.stack([outs[name].cpu().numpy() for name in sep.source_names])
        bn.accumulate(x, [(p, b, f) for b, (p, _, f) in enumerate(chunk)], v, acc, den)
    want = bn.finish(acc, den)
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want))
    assert np.abs(want).max() > 0
