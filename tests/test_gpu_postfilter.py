"""GPU tests of the complex STFT, the inverse STFT and the soft-mask filter (include/wun.h: wun_stft_complex, wun_istft,
wun_mask_filter; wave_u_net_amd.spectral.stft / istft, wave_u_net_amd.postfilter) against the float64 oracle
tests/_postfilter_np.py, whose docstring quotes the definitions and derives the bounds (beta for a Re or Im, istft_bound for
an output sample; both are tried on an fp32 numpy stand-in in tests/test_postfilter_host.py).

Shapes: (n_fft, hop) in {(64, 32), (64, 16), (2048, 512)} -- K = 33 is one bin past a 32-bin tile, 2048 has 65 tiles of bins;
T in {5, 1000, 5000} -- shorter than a frame, no multiple of a hop, every frame count off the 64-row tile; T = 5000 at hop 16 has
316 frames, two of the blocks of 256 the inverse works in.  The filter's float64 comparison runs at T in {1000, 5000}: its
fixtures must keep every bin of the summed estimates above 1e-4 (the oracle asserts it), which a 5-sample track seen through
the edge of a window cannot; T = 5 goes through the filter in the exact cases, which need no conditioning."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _postfilter_np as ora  # noqa: E402
import _spectral_np as sp  # noqa: E402
from _observed import record  # noqa: E402
from _unaligned import _offset_copy  # noqa: E402

from wave_u_net_amd import _lib, postfilter, spectral  # noqa: E402

pytestmark = pytest.mark.gpu

SQRT2 = np.sqrt(2.0)
RES = [(64, 32), (64, 16), (2048, 512)]
LENGTHS = [5, 1000, 5000]
SHAPES = [(2, 1, 2), (3, 3, 1)]            # (S, B, C): C in {1, 2}, S in {2, 3}, B in {1, 3}
_CACHE = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def _signal(n_fft, hop, T, shape, centered=True):
    """Audio [S, B, T, C] of amplitude 0.3 and its float64 transform, computed once."""
    key = (n_fft, hop, T, shape, centered)
    if key not in _CACHE:
        S, B, C = shape
        rng = np.random.RandomState(n_fft + hop + T + 7 * S)
        x = (0.3 * rng.randn(S, B, T, C)).astype(np.float32)
        lead, F = ora.framing(T, n_fft, hop, centered)
        xr = sp.rows(x)
        re, im = ora.stft(xr, n_fft, hop, lead, F)
        _CACHE[key] = {"x": x, "xr": xr, "lead": lead, "F": F, "re": re, "im": im, "beta": ora.beta(xr, n_fft, hop, lead, F)}
    return _CACHE[key]


def _rows(t):
    """Device [S, B, C, F, K] -> float64 [R, F, K]."""
    return t.reshape(-1, t.shape[-2], t.shape[-1]).cpu().numpy().astype(np.float64)


def _spectra(re, im, shape):
    """float [R, F, K] -> device float32 [S, B, C, F, K]."""
    S, B, C = shape
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).reshape(S, B, C, *a.shape[1:]).cuda() for a in (re, im))


# ---------------------------------------------------------------------------------------------------- 1. complex STFT
@pytest.mark.parametrize("shape", SHAPES, ids=["S2B1C2", "S3B3C1"])
@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("n_fft, hop", RES)
def test_stft_complex_against_float64(lib, n_fft, hop, T, shape):
    ref = _signal(n_fft, hop, T, shape)
    re, im = spectral.stft(torch.from_numpy(ref["x"]).cuda(), n_fft, hop, centered=True)
    assert tuple(re.shape) == shape[:2] + (shape[2], ref["F"], n_fft // 2 + 1) == tuple(im.shape)
    b = ref["beta"][:, :, None]
    for what, got, want in (("Re", _rows(re), ref["re"]), ("Im", _rows(im), ref["im"])):
        ratio = (np.abs(got - want) / np.maximum(b, 1e-300)).max()
        record("test_stft_complex_against_float64[%d-%d-%d]" % (n_fft, hop, T), "%s max err / beta" % what, ratio, 1.0)
        assert np.isfinite(got).all() and (np.abs(got - want) <= b).all()


@pytest.mark.parametrize("n_fft, hop, T", [(64, 32, 1000), (64, 16, 5000), (2048, 512, 5000)])
def test_stft_complex_in_the_loss_framing(lib, n_fft, hop, T):
    """lead = 0 with F = wun_stft_frames: sqrt(re^2 + im^2) within the bound test_gpu_spectral uses for wun_stft_magnitude."""
    ref = _signal(n_fft, hop, T, (2, 1, 2), centered=False)
    x = torch.from_numpy(ref["x"]).cuda()
    re, im = spectral.stft(x, n_fft, hop)
    assert re.shape[3] == spectral.frames(T, n_fft, hop) == ref["F"]
    want = np.sqrt(ref["re"] ** 2 + ref["im"] ** 2)
    got = np.sqrt(_rows(re) ** 2 + _rows(im) ** 2)
    bound = SQRT2 * ref["beta"][:, :, None] + 2.0 ** -22 * want
    ratio = (np.abs(got - want) / bound).max()
    record("test_stft_complex_in_the_loss_framing[%d-%d-%d]" % (n_fft, hop, T), "max err / bound", ratio, 1.0)
    assert ratio <= 1.0
    assert (np.abs(_rows(re) - ref["re"]) <= ref["beta"][:, :, None]).all()


# ---------------------------------------------------------------------------------------------------- 2. inverse STFT
@pytest.mark.parametrize("shape", SHAPES, ids=["S2B1C2", "S3B3C1"])
@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("n_fft, hop", RES)
def test_istft_of_given_spectra_against_float64(lib, n_fft, hop, T, shape):
    S, B, C = shape
    lead, F = ora.framing(T, n_fft, hop, True)
    rng = np.random.RandomState(T + n_fft + hop + S)
    re = rng.randn(S * B * C, F, n_fft // 2 + 1).astype(np.float32)
    im = rng.randn(S * B * C, F, n_fft // 2 + 1).astype(np.float32)
    want = ora.istft(re.astype(np.float64), im.astype(np.float64), T, n_fft, hop, lead)
    bound = ora.istft_bound(re, im, want, T, n_fft, hop, lead)
    y = spectral.istft(*_spectra(re, im, shape), T, n_fft, hop, centered=True)
    assert tuple(y.shape) == (S, B, T, C)
    got = sp.rows(y.cpu().numpy())
    ratio = (np.abs(got - want) / bound).max()
    record("test_istft_of_given_spectra_against_float64[%d-%d-%d]" % (n_fft, hop, T), "max err / bound", ratio, 1.0)
    assert np.isfinite(got).all() and (np.abs(got - want) <= bound).all()


def test_istft_is_zero_where_no_window_weight_lies(lib):
    """lead = 0, hop = n_fft: sample 0 of every frame has w^2 = 0 -- below 1e-8, so exactly 0; so is a tail no frame covers."""
    n_fft, T, shape = 64, 64 * 3 + 9, (2, 1, 2)
    F = spectral.frames(T, n_fft, n_fft)
    rng = np.random.RandomState(3)
    re, im = rng.randn(4, F, 33).astype(np.float32), rng.randn(4, F, 33).astype(np.float32)
    y = spectral.istft(*_spectra(re, im, shape), T, n_fft, n_fft)
    got = sp.rows(y.cpu().numpy())
    want = ora.istft(re.astype(np.float64), im.astype(np.float64), T, n_fft, n_fft, 0)
    ws = ora.window_sums(T, F, n_fft, n_fft, 0)
    dead = ws < 1e-8
    assert dead[0] and dead[64] and dead[128] and dead[192:].all() and dead.sum() == 3 + 9
    assert (got[:, dead] == 0).all() and (want[:, dead] == 0).all()
    assert (np.abs(got - want) <= ora.istft_bound(re, im, want, T, n_fft, n_fft, 0)).all()


# ---------------------------------------------------------------------------------------------------- 3. round trip
@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("n_fft, hop", RES)
def test_round_trip(lib, n_fft, hop, T):
    """istft(stft(x)) = x in the centred framing: within istft_bound at the float64 spectra plus the propagated beta."""
    shape = (2, 1, 2)
    ref = _signal(n_fft, hop, T, shape)
    x = torch.from_numpy(ref["x"]).cuda()
    y = spectral.istft(*spectral.stft(x, n_fft, hop, centered=True), T, n_fft, hop, centered=True)
    y64 = ora.istft(ref["re"], ref["im"], T, n_fft, hop, ref["lead"])
    assert np.abs(y64 - ref["xr"]).max() < 1e-14
    bound = ora.istft_bound(ref["re"], ref["im"], y64, T, n_fft, hop, ref["lead"], fwd_beta=ref["beta"])
    got = sp.rows(y.cpu().numpy())
    record("test_round_trip[%d-%d-%d]" % (n_fft, hop, T), "max |y - x|", np.abs(got - ref["xr"]).max(), bound.max())
    record("test_round_trip[%d-%d-%d]" % (n_fft, hop, T), "max err / bound", (np.abs(got - y64) / bound).max(), 1.0)
    assert (np.abs(got - y64) <= bound).all()


# ---------------------------------------------------------------------------------------------------- 4. the filter
@pytest.mark.parametrize("power", [2, 1])
@pytest.mark.parametrize("S, n, C, n_fft, hop", [(2, 1000, 2, 64, 32), (3, 5000, 1, 64, 32), (3, 1000, 1, 64, 16), (2, 5000, 2, 64, 16),
                                                 (2, 1000, 1, 2048, 512), (3, 5000, 2, 2048, 512)])
def test_mask_filter_against_float64(lib, S, n, C, n_fft, hop, power):
    """Within 8 x the distance of the CPU fp32 SoftMaskFilter from the same oracle (max over the track).  Ratios seen on an
    MI355X: see DESIGN.md 5.11."""
    mix, est, want = ora.filter_fixture(11, S, n, C, n_fft, hop, power)
    f = postfilter.SoftMaskFilter(n_fft, hop, power)
    e_cpu = np.abs(f.apply(torch.from_numpy(mix), torch.from_numpy(est)).numpy() - want).max()
    out = f.apply(torch.from_numpy(mix).cuda(), torch.from_numpy(est).cuda())
    assert out.is_cuda and tuple(out.shape) == (S, n, C) and out.dtype == torch.float32
    e_gpu = np.abs(out.cpu().numpy() - want).max()
    tag = "test_mask_filter_against_float64[%d-%d-%d-S%d-p%d]" % (n_fft, hop, n, S, power)
    record(tag, "cpu fp32 max err", e_cpu, 1.0)
    record(tag, "gpu max err", e_gpu, 8 * e_cpu)
    assert e_gpu <= 8 * e_cpu


# ---------------------------------------------------------------------------------------------------- 5. exact cases
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("n_fft, hop", RES)
def test_filter_exact_cases(lib, n_fft, hop, n):
    C = 2
    rng = np.random.RandomState(n + hop)
    mix_h = (0.3 * rng.randn(n, C)).astype(np.float32)
    mix = torch.from_numpy(mix_h).cuda()
    f = postfilter.SoftMaskFilter(n_fft, hop)
    x4 = mix.view(1, 1, n, C)
    rt = spectral.istft(*spectral.stft(x4, n_fft, hop, centered=True), n, n_fft, hop, centered=True)[0, 0]
    # zero estimates, S = 2: mask = 0.5 exactly
    out = f.apply(mix, torch.zeros((2, n, C), device="cuda"))
    assert torch.equal(out[0], out[1]) and torch.equal(out[0], 0.5 * rt)
    # the outputs sum to the device's own istft(stft(mix)): S 2^-22 max |mix| plus the inverse's bound
    lead, F = ora.framing(n, n_fft, hop, True)
    re, im = ora.stft(mix_h.T, n_fft, hop, lead, F)
    y64 = ora.istft(re, im, n, n_fft, hop, lead)
    bound = ora.istft_bound(re, im, y64, n, n_fft, hop, lead).T                      # [n, C]
    for S in (2, 3):
        est = torch.from_numpy((0.25 * rng.randn(S, n, C)).astype(np.float32)).cuda()
        total = f.apply(mix, est).double().sum(0)
        err = (total - rt.double()).abs().cpu().numpy()
        tol = S * 2.0 ** -22 * np.abs(mix_h).max() + bound
        record("test_filter_exact_cases[%d-%d-%d]" % (n_fft, hop, n), "S = %d: max (sum - rt) / tol" % S, (err / tol).max(), 1.0)
        assert (err <= tol).all()
        # a zero mix gives outputs of exactly 0
        assert bool((f.apply(torch.zeros_like(mix), est) == 0).all())


# ---------------------------------------------------------------------------------------------------- 6. determinism
@pytest.mark.parametrize("n_fft, hop, n", [(64, 16, 5000), (2048, 512, 1000), (64, 32, 5)])
def test_filter_bits_do_not_depend_on_scratch_or_alignment(lib, n_fft, hop, n):
    S, C = 3, 2
    rng = np.random.RandomState(5)
    mix = torch.from_numpy((0.3 * rng.randn(n, C)).astype(np.float32)).cuda()
    est = torch.from_numpy((0.25 * rng.randn(S, n, C)).astype(np.float32)).cuda()
    f = postfilter.SoftMaskFilter(n_fft, hop)
    floats = f.scratch_floats(S, n, C)
    outs = []
    for fill in (float("nan"), 0.0):
        scratch = torch.full((floats,), fill, dtype=torch.float32, device="cuda")
        out = torch.full_like(est, float("nan"))
        f.run(mix, est, out, scratch)
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())
    assert torch.equal(f.apply(mix, est), outs[0])
    # every pointer 4 bytes off
    out = torch.empty(est.numel() + 1, dtype=torch.float32, device="cuda")[1:].view(est.shape)
    scratch = torch.full((floats + 1,), float("nan"), dtype=torch.float32, device="cuda")[1:]
    f.run(_offset_copy(mix), _offset_copy(est), out, scratch)
    assert torch.equal(out, outs[0])


def test_transform_bits_do_not_depend_on_the_batch_or_alignment(lib):
    """A row's spectra and samples do not depend on the rows around it (other tiles, other blocks of frames), nor on a
    pointer 4 bytes off."""
    n_fft, hop, T = 64, 16, 5000
    ref = _signal(n_fft, hop, T, (3, 3, 1))
    x = torch.from_numpy(ref["x"]).cuda()
    re, im = spectral.stft(x, n_fft, hop, centered=True)
    r1, i1 = spectral.stft(x[1:2, 2:3].contiguous(), n_fft, hop, centered=True)
    assert torch.equal(r1, re[1:2, 2:3]) and torch.equal(i1, im[1:2, 2:3])
    r2, i2 = spectral.stft(_offset_copy(x), n_fft, hop, centered=True)
    assert torch.equal(r2, re) and torch.equal(i2, im)
    y = spectral.istft(re, im, T, n_fft, hop, centered=True)
    assert torch.equal(spectral.istft(r1.contiguous(), i1.contiguous(), T, n_fft, hop, centered=True), y[1:2, 2:3])
    assert torch.equal(spectral.istft(_offset_copy(re), _offset_copy(im), T, n_fft, hop, centered=True), y)


# ---------------------------------------------------------------------------------------------------- 7. separate_track
@pytest.mark.parametrize("name", ["baseline_context_small", "baseline_stereo_small"])
def test_separate_track_with_the_filter(lib, name):
    from test_gpu_separate_track import _separator
    from wave_u_net_amd.evaluate import separate_track
    cfg, ocfg, sep, params, i, o = _separator(name)
    chan = 1 if cfg["mono_downmix"] else 2
    n = 5 * int(o[1]) + 17
    audio = np.random.default_rng(8).uniform(-1.0, 1.0, (n, chan)).astype(np.float32)
    sr = cfg["expected_sr"]
    plain = separate_track(cfg, sep, audio, sr, batch_hops=3, return_device=True)
    none = separate_track(cfg, sep, audio, sr, batch_hops=3, return_device=True, postfilter=None)
    assert torch.equal(plain, none)                                            # postfilter=None: the parent's path and bits
    f = postfilter.SoftMaskFilter(64, 16)
    got = separate_track(cfg, sep, audio, sr, batch_hops=3, return_device=True, postfilter=f)
    want = f.apply(torch.from_numpy(audio).cuda(), plain)
    assert got.shape == plain.shape and torch.equal(got, want) and not torch.equal(got, plain)
    host = separate_track(cfg, sep, audio, sr, batch_hops=3, postfilter={"n_fft": 64, "hop": 16})
    for si, k in enumerate(cfg["source_names"]):
        assert np.array_equal(host[k], got[si].cpu().numpy())
