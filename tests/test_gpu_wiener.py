"""GPU tests of the multichannel Wiener post-filter (include/wun.h: wun_wiener_filter; wave_u_net_amd.postfilter.WienerFilter;
DESIGN.md 5.12) against the float64 oracle tests/_wiener_np.py, whose docstring quotes the definition.

Shapes: 64 / 16 with n = 1500 (97 frames: one block, 7 chunks of 16 frames, the last one short), 64 / 16 with n = 4800 (303
frames: the statistics and the inverse cross a block boundary at frame 256; K = 33 is one bin past a 32-bin tile), 2048 / 512
with n = 6000 (15 frames: less than one chunk, 65 tiles of bins); (S, C) in {(2, 2), (3, 2), (2, 1), (1, 2)}: both channel
counts, one source alone, an odd source count.  n = 5 (shorter than a frame) goes through the exact cases.

Against the oracle the rule is DESIGN.md 5.11's for the mask filter: the device's error is at most 8 x the distance of the CPU
float32 WienerFilter from the same oracle (the algebra is float64 on both sides; the transforms differ in their summation
order)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _postfilter_np as ora  # noqa: E402
import _wiener_np as wie  # noqa: E402
from _observed import record  # noqa: E402

from wave_u_net_amd import _lib, postfilter, spectral  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(64, 16, 1500), (64, 16, 4800), (2048, 512, 6000)]
CASES = [(2, 2), (3, 2), (2, 1), (1, 2)]                          # (S, C)
_CACHE = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def _fixture(S, C, n_fft, hop, n, power, iterations):
    """(mix, est, the oracle's output, the CPU float32 filter's distance from it, the oracle's max |Cxx^-1 X|), computed
    once."""
    key = (S, C, n_fft, hop, n, power, iterations)
    if key not in _CACHE:
        mix, est, want, zmax = wie.fixture(11, S, n, C, n_fft, hop, power, iterations, details=True)
        cpu = postfilter.WienerFilter(n_fft, hop, power, iterations=iterations).apply(torch.from_numpy(mix), torch.from_numpy(est))
        _CACHE[key] = (mix, est, want, np.abs(cpu.numpy() - want).max(), zmax)
    return _CACHE[key]


def _check_against_float64(S, C, n_fft, hop, n, power, iterations):
    mix, est, want, e_cpu, _ = _fixture(S, C, n_fft, hop, n, power, iterations)
    f = postfilter.WienerFilter(n_fft, hop, power, iterations=iterations)
    out = f.apply(torch.from_numpy(mix).cuda(), torch.from_numpy(est).cuda())
    assert out.is_cuda and tuple(out.shape) == (S, n, C) and out.dtype == torch.float32
    e_gpu = np.abs(out.cpu().numpy() - want).max()
    tag = "test_wiener_filter_against_float64[%d-%d-%d-S%d-C%d-I%d-p%d]" % (n_fft, hop, n, S, C, iterations, power)
    record(tag, "cpu fp32 max err", e_cpu, 1.0)
    record(tag, "gpu max err", e_gpu, 8 * e_cpu)
    assert e_gpu <= 8 * e_cpu


# ---------------------------------------------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("iterations", [1, 2])
@pytest.mark.parametrize("S, C", CASES)
@pytest.mark.parametrize("n_fft, hop, n", SHAPES)
def test_wiener_filter_against_float64(lib, n_fft, hop, n, S, C, iterations):
    _check_against_float64(S, C, n_fft, hop, n, 2, iterations)


def test_wiener_filter_against_float64_power_one(lib):
    _check_against_float64(3, 2, 64, 16, 4800, 1, 1)


# ---------------------------------------------------------------------------------------------------- 2. exact cases
def _inputs(S, C, n, seed):
    rng = np.random.RandomState(seed)
    mix = torch.from_numpy((0.3 * rng.randn(n, C)).astype(np.float32)).cuda()
    est = torch.from_numpy((0.25 * rng.randn(S, n, C)).astype(np.float32)).cuda()
    return mix, est


@pytest.mark.parametrize("C", [2, 1])
@pytest.mark.parametrize("n_fft, hop, n", [(64, 16, 4800), (2048, 512, 1000), (64, 32, 5)])
def test_zero_iterations_is_the_mask_filter(lib, n_fft, hop, n, C):
    mix, est = _inputs(3, C, n, 1)
    for power in (2, 1):
        got = postfilter.WienerFilter(n_fft, hop, power, iterations=0).apply(mix, est)
        assert torch.equal(got, postfilter.SoftMaskFilter(n_fft, hop, power).apply(mix, est))


@pytest.mark.parametrize("C", [2, 1])
@pytest.mark.parametrize("n_fft, hop, n", [(64, 16, 4800), (2048, 512, 1000), (64, 32, 5)])
def test_exact_cases(lib, n_fft, hop, n, C):
    mix, est = _inputs(2, C, n, n + hop)
    f = postfilter.WienerFilter(n_fft, hop, iterations=2)
    assert bool((f.apply(torch.zeros_like(mix), est) == 0).all())              # a zero mix gives zeros
    out = f.apply(mix, torch.zeros_like(est))                                  # zero estimates: both sources alike
    assert torch.equal(out[0], out[1]) and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("n_fft, hop, n", [(64, 16, 4800), (2048, 512, 1000), (64, 32, 5)])
def test_bits_do_not_depend_on_scratch_or_the_run(lib, n_fft, hop, n):
    S, C = 3, 2
    mix, est = _inputs(S, C, n, 5)
    f = postfilter.WienerFilter(n_fft, hop, iterations=2)
    floats = f.scratch_floats(S, n, C)
    outs = []
    for fill in (float("nan"), 0.0, float("nan")):                             # NaN-filled, zeroed, and a second NaN run
        scratch = torch.full((floats,), fill, dtype=torch.float32, device="cuda")
        out = torch.full_like(est, float("nan"))
        f.run(mix, est, out, scratch)
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and bool(torch.isfinite(outs[0]).all())
    assert torch.equal(f.apply(mix, est), outs[0]) and torch.equal(f.apply(mix, est), outs[0])     # the cached scratch, twice
    # the scratch handed over 4 bytes off an 8-byte boundary: the float64 statistics find their own alignment
    scratch = torch.full((floats + 1,), float("nan"), dtype=torch.float32, device="cuda")[1:]
    out = torch.empty_like(est)
    f.run(mix, est, out, scratch)
    assert torch.equal(out, outs[0])


# ---------------------------------------------------------------------------------------------------- 3. sum to the mix
@pytest.mark.parametrize("S, C", [(2, 2), (3, 1)])
@pytest.mark.parametrize("n_fft, hop, n", SHAPES)
def test_outputs_sum_to_the_mix(lib, n_fft, hop, n, S, C):
    """The y_s sum to X - sqrt(eps) Cxx^-1 X.  Against the device's own istft(stft(mix)): the regulariser's share
    (_wiener_np.regulariser_bound at the oracle's largest |Cxx^-1 X|) plus DESIGN.md 5.11's bound for the mask filter's sum,
    S 2^-22 max |mix| and the inverse's bound."""
    mix_h, est_h, _, _, zmax = _fixture(S, C, n_fft, hop, n, 2, 1)
    mix = torch.from_numpy(mix_h).cuda()
    rt = spectral.istft(*spectral.stft(mix.view(1, 1, n, C), n_fft, hop, centered=True), n, n_fft, hop, centered=True)[0, 0]
    lead, F = ora.framing(n, n_fft, hop, True)
    re, im = ora.stft(mix_h.T, n_fft, hop, lead, F)
    y64 = ora.istft(re, im, n, n_fft, hop, lead)
    reg = wie.regulariser_bound(zmax, n, n_fft, hop)
    tol = reg + S * 2.0 ** -22 * np.abs(mix_h).max() + ora.istft_bound(re, im, y64, n, n_fft, hop, lead).T       # [n, C]
    total = postfilter.WienerFilter(n_fft, hop).apply(mix, torch.from_numpy(est_h).cuda()).double().sum(0)
    err = (total - rt.double()).abs().cpu().numpy()
    tag = "test_outputs_sum_to_the_mix[%d-%d-%d-S%d-C%d]" % (n_fft, hop, n, S, C)
    record(tag, "regulariser's share of the tolerance", reg / tol.min(), 1.0)
    record(tag, "max (sum - rt) / tol", (err / tol).max(), 1.0)
    assert (err <= tol).all()


# ---------------------------------------------------------------------------------------------------- 4. what it is for
@pytest.mark.parametrize("seed", [0, 1])
def test_panned_sources(lib, seed):
    """_wiener_np.panned_fixture on the device: one EM iteration brings the RMS error against the true sources to at most 0.9
    of the device's own soft mask's."""
    mix, est, src = wie.panned_fixture(seed)
    mix, est = torch.from_numpy(mix).cuda(), torch.from_numpy(est).cuda()
    soft = wie.rms(postfilter.SoftMaskFilter(64, 16).apply(mix, est).cpu().numpy() - src)
    one = wie.rms(postfilter.WienerFilter(64, 16).apply(mix, est).cpu().numpy() - src)
    record("test_gpu_wiener.test_panned_sources[%d]" % seed, "rms error / soft mask's", one / soft, 0.9)
    assert one <= 0.9 * soft


# ---------------------------------------------------------------------------------------------------- 5. separate_track
def test_separate_track_with_the_filter(lib):
    from test_gpu_separate_track import _separator
    from wave_u_net_amd.evaluate import separate_track
    cfg, ocfg, sep, params, i, o = _separator("baseline_stereo_small")
    assert not cfg["mono_downmix"]
    n = 5 * int(o[1]) + 17
    audio = np.random.default_rng(8).uniform(-1.0, 1.0, (n, 2)).astype(np.float32)
    sr = cfg["expected_sr"]
    plain = separate_track(cfg, sep, audio, sr, batch_hops=3, return_device=True)
    spec = {"kind": "wiener", "n_fft": 64, "hop": 16}
    got = separate_track(cfg, sep, audio, sr, batch_hops=3, return_device=True, postfilter=spec)
    want = postfilter.WienerFilter(64, 16).apply(torch.from_numpy(audio).cuda(), plain)
    soft = separate_track(cfg, sep, audio, sr, batch_hops=3, return_device=True, postfilter={"n_fft": 64, "hop": 16})
    assert got.shape == plain.shape and torch.equal(got, want) and not torch.equal(got, plain) and not torch.equal(got, soft)
    host = separate_track(cfg, sep, audio, sr, batch_hops=3, postfilter=postfilter.WienerFilter(64, 16))
    for si, k in enumerate(cfg["source_names"]):
        assert np.array_equal(host[k], got[si].cpu().numpy())
