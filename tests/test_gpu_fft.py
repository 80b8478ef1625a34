"""GPU tests of the FFT path (include/wun.h: wun_stft_complex_fft, wun_istft_fft, wun_mask_filter_fft, wun_wiener_filter_fft;
wave_u_net_amd.spectral.stft / istft and wave_u_net_amd.postfilter with transform="fft") against the float64
oracle tests/_fft_np.py (numpy.fft on the frames of _postfilter_np, whose bounds beta and istft_bound hold for any float32
summation order).

Shapes (n_fft, hop, T): (64, 16, 5000) is the smallest transform, 316 frames -- two blocks of 256, 32 frames to a workgroup;
(64, 32, 5) a track shorter than a frame; (256, 64, 1000); (2048, 512, 5000) overlaps the GEMM path; (4096, 1024, 9000) is
the first size the GEMM refuses; (8192, 2048, 20000) the largest; (8192, 1024, 5) the largest with a short track.  log2 of the
complex length is odd at 64, 256, 1024 and 4096 (a radix-2 stage last) and even at 2048 and 8192.

Two rules per transform: the derived hard bound, and a measured one -- at most 8 x the max-abs error of scipy's float32 FFT on
the same windowed frames (the project's margin for another summation order and once-rounded tables).
Ratios seen on an MI355X: DESIGN.md 5.13."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from wave_u_net_amd import _lib, postfilter, spectral  # noqa: E402

_lib.load().wun_stft_complex_fft                     # the feature: an AttributeError without it

import _fft_np as fo  # noqa: E402
import _spectral_np as sp  # noqa: E402
from _observed import record  # noqa: E402
from _unaligned import _offset_copy  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(64, 16, 5000), (64, 32, 5), (256, 64, 1000), (2048, 512, 5000), (4096, 1024, 9000), (8192, 2048, 20000), (8192, 1024, 5)]
SHAPES = [(2, 1, 2), (3, 3, 1)]                      # (S, B, C)
IDS = ["S2B1C2", "S3B3C1"]
FILTER_SIZES = [(64, 16, 4800), (4096, 1024, 9000), (8192, 2048, 20000)]
FILTER_CASES = [(2, 2), (4, 2), (3, 1)]              # (S, C)
_CACHE = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def _signal(n_fft, hop, T, shape):
    """Audio [S, B, T, C] of amplitude 0.3, its float64 transform, beta and the float32 stand-in's error, computed once."""
    key = ("sig", n_fft, hop, T, shape)
    if key not in _CACHE:
        S, B, Cn = shape
        rng = np.random.RandomState(n_fft + hop + T + 7 * S)
        x = (0.3 * rng.randn(S, B, T, Cn)).astype(np.float32)
        lead, F = fo.framing(T, n_fft, hop, True)
        xr = sp.rows(x)
        re, im = fo.stft(xr, n_fft, hop, lead, F)
        r32, i32 = fo.stft_fp32(xr, n_fft, hop, lead, F)
        _CACHE[key] = {"x": x, "xr": xr, "lead": lead, "F": F, "re": re, "im": im, "beta": fo.beta(xr, n_fft, hop, lead, F),
                       "e32": max(np.abs(r32 - re).max(), np.abs(i32 - im).max())}
    return _CACHE[key]


def _given_spectra(n_fft, hop, T, shape):
    """Random spectra [R, F, K], their float64 inverse, its bound and the float32 stand-in's error, computed once."""
    key = ("spec", n_fft, hop, T, shape)
    if key not in _CACHE:
        S, B, Cn = shape
        lead, F = fo.framing(T, n_fft, hop, True)
        rng = np.random.RandomState(T + n_fft + hop + S)
        re = rng.randn(S * B * Cn, F, n_fft // 2 + 1).astype(np.float32)
        im = rng.randn(S * B * Cn, F, n_fft // 2 + 1).astype(np.float32)
        want = fo.istft(re, im, T, n_fft, hop, lead)
        ref_re, ref_im = re.astype(np.float64), im.astype(np.float64).copy()
        ref_im[..., 0] = ref_im[..., -1] = 0.0           # (the definition does not read them; the bound must not count them)
        _CACHE[key] = {"re": re, "im": im, "lead": lead, "F": F, "want": want,
                       "bound": fo.istft_bound(ref_re, ref_im, want, T, n_fft, hop, lead),
                       "e32": np.abs(fo.istft_fp32(re, im, T, n_fft, hop, lead) - want).max()}
    return _CACHE[key]


def _rows(t):
    """Device [S, B, C, F, K] -> float64 [R, F, K]."""
    return t.reshape(-1, t.shape[-2], t.shape[-1]).cpu().numpy().astype(np.float64)


def _dev_spectra(re, im, shape):
    S, B, Cn = shape
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).reshape(S, B, Cn, *a.shape[1:]).cuda() for a in (re, im))


# ---------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("n_fft, hop, T", CASES)
def test_stft_fft_against_float64(lib, n_fft, hop, T, shape):
    ref = _signal(n_fft, hop, T, shape)
    re, im = spectral.stft(torch.from_numpy(ref["x"]).cuda(), n_fft, hop, centered=True, transform="fft")
    assert tuple(re.shape) == shape[:2] + (shape[2], ref["F"], n_fft // 2 + 1) == tuple(im.shape)
    assert bool((im[..., 0] == 0).all()) and bool((im[..., -1] == 0).all())              # exactly 0 at the bins 0 and n_fft / 2
    b = ref["beta"][:, :, None]
    tag = "test_stft_fft_against_float64[%d-%d-%d-%s]" % (n_fft, hop, T, IDS[SHAPES.index(shape)])
    gre, gim = _rows(re), _rows(im)
    worst = 0.0
    for what, got, want in (("Re", gre, ref["re"]), ("Im", gim, ref["im"])):
        err = np.abs(got - want)
        worst = max(worst, err.max())
        record(tag, "%s max err / beta" % what, (err / np.maximum(b, 1e-300)).max(), 1.0)
        assert np.isfinite(got).all() and (err <= b).all()
    record(tag, "fp32 FFT stand-in max err / max beta", ref["e32"] / ref["beta"].max(), 1.0)
    record(tag, "max err / stand-in's", worst / ref["e32"], 8.0)
    assert worst <= 8 * ref["e32"]


@pytest.mark.parametrize("n_fft, hop, T", [(64, 48, 1000), (4096, 1024, 9000), (8192, 8192, 20000)])
def test_the_framing_without_padding(lib, n_fft, hop, T):
    """centered=False: lead = 0 and F = wun_fft_frames whole frames (the loss's framing), past the GEMM's 2048 too.  Forward
    under the two rules above; the inverse of those spectra gives the samples back wherever window weight lies (hop = n_fft
    leaves every frame's sample 0 and the tail behind the last frame at exactly 0)."""
    shape = (2, 1, 2)
    rng = np.random.RandomState(n_fft + T)
    x = (0.3 * rng.randn(2, 1, T, 2)).astype(np.float32)
    F = spectral.frames(T, n_fft, hop, transform="fft")
    assert F == 1 + (T - n_fft) // hop
    xr = sp.rows(x)
    want_re, want_im = fo.stft(xr, n_fft, hop, 0, F)
    b = fo.beta(xr, n_fft, hop, 0, F)[:, :, None]
    r32, i32 = fo.stft_fp32(xr, n_fft, hop, 0, F)
    e32 = max(np.abs(r32 - want_re).max(), np.abs(i32 - want_im).max())
    re, im = spectral.stft(torch.from_numpy(x).cuda(), n_fft, hop, transform="fft")
    assert tuple(re.shape) == (2, 1, 2, F, n_fft // 2 + 1)
    err = np.maximum(np.abs(_rows(re) - want_re), np.abs(_rows(im) - want_im))
    record("test_the_framing_without_padding[%d-%d-%d]" % (n_fft, hop, T), "max err / stand-in's", err.max() / e32, 8.0)
    assert (err <= b).all() and err.max() <= 8 * e32
    y = spectral.istft(re, im, T, n_fft, hop, transform="fft")
    y64 = fo.istft(want_re, want_im, T, n_fft, hop, 0)
    live = fo.window_sums(T, F, n_fft, hop, 0) >= 1e-8
    assert np.abs(y64 - xr)[:, live].max() < 1e-9 and (y64[:, ~live] == 0).all()
    # (hop = n_fft divides by window squares down to 1e-8: there y64 = x only to 1e-9, and the bound carries the division)
    bound = fo.istft_bound(want_re, want_im, y64, T, n_fft, hop, 0, fwd_beta=fo.beta(xr, n_fft, hop, 0, F))
    got = sp.rows(y.cpu().numpy())
    assert (got[:, ~live] == 0).all() and (np.abs(got - y64) <= bound).all()


# ---------------------------------------------------------------------------------------------------- 2. inverse
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("n_fft, hop, T", CASES)
def test_istft_fft_of_given_spectra_against_float64(lib, n_fft, hop, T, shape):
    S, B, Cn = shape
    ref = _given_spectra(n_fft, hop, T, shape)
    dre, dim = _dev_spectra(ref["re"], ref["im"], shape)
    y = spectral.istft(dre, dim, T, n_fft, hop, centered=True, transform="fft")
    assert tuple(y.shape) == (S, B, T, Cn)
    got = sp.rows(y.cpu().numpy())
    err = np.abs(got - ref["want"])
    tag = "test_istft_fft_of_given_spectra_against_float64[%d-%d-%d-%s]" % (n_fft, hop, T, IDS[SHAPES.index(shape)])
    record(tag, "max err / bound", (err / ref["bound"]).max(), 1.0)
    record(tag, "max err / stand-in's", err.max() / ref["e32"], 8.0)
    assert np.isfinite(got).all() and (err <= ref["bound"]).all()
    assert err.max() <= 8 * ref["e32"]
    # garbage in Im of the bins 0 and n_fft / 2 does not change a bit
    dim2 = dim.clone()
    dim2[..., 0] = float("nan")
    dim2[..., -1] = 1e30
    assert torch.equal(spectral.istft(dre, dim2, T, n_fft, hop, centered=True, transform="fft"), y)


def test_istft_fft_is_zero_where_no_window_weight_lies(lib):
    """lead = 0, hop = n_fft: sample 0 of every frame has w^2 = 0 -- below 1e-8, so exactly 0; so is a tail no frame covers."""
    n_fft, T, shape = 64, 64 * 3 + 9, (2, 1, 2)
    F = spectral.frames(T, n_fft, n_fft)
    rng = np.random.RandomState(3)
    re, im = rng.randn(4, F, 33).astype(np.float32), rng.randn(4, F, 33).astype(np.float32)
    y = spectral.istft(*_dev_spectra(re, im, shape), T, n_fft, n_fft, transform="fft")
    got = sp.rows(y.cpu().numpy())
    want = fo.istft(re, im, T, n_fft, n_fft, 0)
    dead = fo.window_sums(T, F, n_fft, n_fft, 0) < 1e-8
    assert dead[0] and dead[64] and dead[128] and dead[192:].all() and dead.sum() == 3 + 9
    assert (got[:, dead] == 0).all() and (want[:, dead] == 0).all()
    im0 = im.astype(np.float64).copy()
    im0[..., 0] = im0[..., -1] = 0.0
    assert (np.abs(got - want) <= fo.istft_bound(re.astype(np.float64), im0, want, T, n_fft, n_fft, 0)).all()


# ---------------------------------------------------------------------------------------------------- 3. round trip
@pytest.mark.parametrize("n_fft, hop, T", CASES)
def test_round_trip(lib, n_fft, hop, T):
    """istft(stft(x)) = x in the centred framing: test_gpu_postfilter's bound, istft_bound at the float64 spectra plus the
    propagated beta."""
    ref = _signal(n_fft, hop, T, (2, 1, 2))
    x = torch.from_numpy(ref["x"]).cuda()
    y = spectral.istft(*spectral.stft(x, n_fft, hop, centered=True, transform="fft"), T, n_fft, hop, centered=True, transform="fft")
    y64 = fo.istft(ref["re"], ref["im"], T, n_fft, hop, ref["lead"])
    assert np.abs(y64 - ref["xr"]).max() < 1e-13
    bound = fo.istft_bound(ref["re"], ref["im"], y64, T, n_fft, hop, ref["lead"], fwd_beta=ref["beta"])
    got = sp.rows(y.cpu().numpy())
    record("test_gpu_fft.test_round_trip[%d-%d-%d]" % (n_fft, hop, T), "max |y - x|", np.abs(got - ref["xr"]).max(), bound.max())
    record("test_gpu_fft.test_round_trip[%d-%d-%d]" % (n_fft, hop, T), "max err / bound", (np.abs(got - y64) / bound).max(), 1.0)
    assert (np.abs(got - y64) <= bound).all()


# ---------------------------------------------------------------------------------------------------- 4. the GEMM path
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("n_fft, hop, T", [c for c in CASES if c[0] <= 2048])
def test_agreement_with_the_gemm_path(lib, n_fft, hop, T, shape):
    """Both paths lie within their bound of the float64 value: they differ by at most the sum, 2 beta and 2 istft_bound."""
    ref = _signal(n_fft, hop, T, shape)
    x = torch.from_numpy(ref["x"]).cuda()
    fre, fim = spectral.stft(x, n_fft, hop, centered=True, transform="fft")
    gre, gim = spectral.stft(x, n_fft, hop, centered=True)
    b = 2 * ref["beta"][:, :, None]
    assert (np.abs(_rows(fre) - _rows(gre)) <= b).all() and (np.abs(_rows(fim) - _rows(gim)) <= b).all()
    spec = _given_spectra(n_fft, hop, T, shape)
    dre, dim = _dev_spectra(spec["re"], spec["im"], shape)
    yf = spectral.istft(dre, dim, T, n_fft, hop, centered=True, transform="fft")
    yg = spectral.istft(dre, dim, T, n_fft, hop, centered=True, transform="gemm")
    # (the GEMM's bound counts Im of the edge bins, which it multiplies by Sb = 0)
    gb = fo.istft_bound(spec["re"], spec["im"], spec["want"], T, n_fft, hop, spec["lead"])
    d = np.abs(sp.rows(yf.cpu().numpy()) - sp.rows(yg.cpu().numpy()))
    record("test_agreement_with_the_gemm_path[%d-%d-%d]" % (n_fft, hop, T), "max |fft - gemm| / sum of bounds",
           (d / (spec["bound"] + gb)).max(), 1.0)
    assert (d <= spec["bound"] + gb).all()


# ---------------------------------------------------------------------------------------------------- 5. the filters
def _filter(n_fft, hop, iterations, **kw):
    if iterations is None:
        return postfilter.SoftMaskFilter(n_fft, hop, transform="fft", **kw)
    return postfilter.WienerFilter(n_fft, hop, iterations=iterations, transform="fft", **kw)


def _fixture(S, Cn, n_fft, hop, n, iterations):
    """(mix, est, the oracle's output, the CPU class's distance from it), computed once."""
    key = ("filt", S, Cn, n_fft, hop, n, iterations)
    if key not in _CACHE:
        mix, est, want = fo.fixture(11, S, n, Cn, n_fft, hop, 2, iterations or 0)
        cpu = _filter(n_fft, hop, iterations).apply(torch.from_numpy(mix), torch.from_numpy(est))
        _CACHE[key] = (mix, est, want, np.abs(cpu.numpy() - want).max())
    return _CACHE[key]


def _check_filter(tag, f, mix, est, want, e_cpu):
    out = f.apply(torch.from_numpy(mix).cuda(), torch.from_numpy(est).cuda())
    assert out.is_cuda and tuple(out.shape) == est.shape and out.dtype == torch.float32
    e_gpu = np.abs(out.cpu().numpy() - want).max()
    record(tag, "cpu fp32 max err", e_cpu, 1.0)
    record(tag, "gpu max err", e_gpu, 8 * e_cpu)
    assert np.isfinite(e_gpu) and e_gpu <= 8 * e_cpu


@pytest.mark.parametrize("iterations", [None, 1, 2], ids=["mask", "I1", "I2"])
@pytest.mark.parametrize("S, Cn", FILTER_CASES)
@pytest.mark.parametrize("n_fft, hop, n", FILTER_SIZES)
def test_filters_against_float64(lib, n_fft, hop, n, S, Cn, iterations):
    """At most 8 x the distance of the CPU class (torch.fft in float32) from the same oracle."""
    mix, est, want, e_cpu = _fixture(S, Cn, n_fft, hop, n, iterations)
    tag = "test_gpu_fft.test_filters_against_float64[%d-%d-%d-S%d-C%d-%s]" % (n_fft, hop, n, S, Cn, iterations)
    _check_filter(tag, _filter(n_fft, hop, iterations), mix, est, want, e_cpu)


def test_wiener_on_a_loud_tonal_track_at_8192(lib):
    """DESIGN.md 5.13, the conditioning above 2048: 0.9-amplitude sines, hard-panned, plus 1e-3 noise.  The same rule."""
    n_fft, hop, n = 8192, 2048, 20000
    mix, est, want = fo.loud_fixture(5, n, n_fft, hop)
    f = _filter(n_fft, hop, 1)
    e_cpu = np.abs(f.apply(torch.from_numpy(mix), torch.from_numpy(est)).numpy() - want).max()
    _check_filter("test_wiener_on_a_loud_tonal_track_at_8192", f, mix, est, want, e_cpu)


# ---------------------------------------------------------------------------------------------------- 6. exact cases
def _inputs(S, Cn, n, seed):
    rng = np.random.RandomState(seed)
    mix = torch.from_numpy((0.3 * rng.randn(n, Cn)).astype(np.float32)).cuda()
    est = torch.from_numpy((0.25 * rng.randn(S, n, Cn)).astype(np.float32)).cuda()
    return mix, est


EXACT = [(64, 16, 4800), (4096, 1024, 9000), (8192, 1024, 5)]


@pytest.mark.parametrize("Cn", [2, 1])
@pytest.mark.parametrize("n_fft, hop, n", EXACT)
def test_exact_cases(lib, n_fft, hop, n, Cn):
    mix, est = _inputs(2, Cn, n, n + hop)
    for f in (_filter(n_fft, hop, None), _filter(n_fft, hop, 2)):
        assert bool((f.apply(torch.zeros_like(mix), est) == 0).all())              # a zero mix gives zeros
        out = f.apply(mix, torch.zeros_like(est))                                  # zero estimates: both sources alike
        assert torch.equal(out[0], out[1]) and bool(torch.isfinite(out).all())
    mix3, est3 = _inputs(3, Cn, n, 1)
    for power in (2, 1):                                                           # I = 0 is wun_mask_filter_fft
        got = _filter(n_fft, hop, 0, power=power).apply(mix3, est3)
        assert torch.equal(got, _filter(n_fft, hop, None, power=power).apply(mix3, est3))


@pytest.mark.parametrize("iterations", [None, 2], ids=["mask", "I2"])
@pytest.mark.parametrize("n_fft, hop, n", EXACT)
def test_bits_do_not_depend_on_scratch_alignment_or_the_run(lib, n_fft, hop, n, iterations):
    S, Cn = 3, 2
    mix, est = _inputs(S, Cn, n, 5)
    f = _filter(n_fft, hop, iterations)
    floats = f.scratch_floats(S, n, Cn)
    outs = []
    for fill in (float("nan"), 0.0, float("nan")):                                 # NaN-filled, zeroed, and a second NaN run
        scratch = torch.full((floats,), fill, dtype=torch.float32, device="cuda")
        out = torch.full_like(est, float("nan"))
        f.run(mix, est, out, scratch)
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and bool(torch.isfinite(outs[0]).all())
    assert torch.equal(f.apply(mix, est), outs[0]) and torch.equal(f.apply(mix, est), outs[0])
    out = torch.empty(est.numel() + 1, dtype=torch.float32, device="cuda")[1:].view(est.shape)      # every pointer 4 bytes off
    scratch = torch.full((floats + 1,), float("nan"), dtype=torch.float32, device="cuda")[1:]
    f.run(_offset_copy(mix), _offset_copy(est), out, scratch)
    assert torch.equal(out, outs[0])


def _one_frame(lib, x, n_fft, hop, f):
    """Frame f of the centred transform of x [S, B, T, C], computed alone: F = 1, the lead (or the start of the audio) moved."""
    S, B, T, Cn = (int(v) for v in x.shape)
    t0 = f * hop - (n_fft - hop)
    lead = 0
    if t0 < 0:
        lead, t0 = -t0, 0
    xs = x[:, :, t0:].contiguous()
    re = torch.empty((S, B, Cn, 1, n_fft // 2 + 1), dtype=torch.float32, device=x.device)
    im = torch.empty_like(re)
    _lib.check(lib.wun_stft_complex_fft(xs.data_ptr(), S, B, T - t0, Cn, n_fft, hop, lead, 1,
                                        spectral._fft_table(n_fft, x.device).data_ptr(), re.data_ptr(), im.data_ptr(),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return re, im


def test_a_frames_bits_do_not_depend_on_its_neighbours(lib):
    """A frame alone (F = 1, one frame slot of a workgroup in use) has the bits it has inside the 316-frame call; so has a row
    computed alone, and a transform from a pointer 4 bytes off.  The inverse likewise."""
    n_fft, hop, T = 64, 16, 5000
    ref = _signal(n_fft, hop, T, (3, 3, 1))
    x = torch.from_numpy(ref["x"]).cuda()
    re, im = spectral.stft(x, n_fft, hop, centered=True, transform="fft")
    assert re.shape[3] == 316
    for f in (0, 2, 3, 4, 31, 32, 100, 255, 256, 315):
        r1, i1 = _one_frame(lib, x, n_fft, hop, f)
        assert torch.equal(r1[..., 0, :], re[..., f, :]) and torch.equal(i1[..., 0, :], im[..., f, :]), f
    r1, i1 = spectral.stft(x[1:2, 2:3].contiguous(), n_fft, hop, centered=True, transform="fft")
    assert torch.equal(r1, re[1:2, 2:3]) and torch.equal(i1, im[1:2, 2:3])
    r2, i2 = spectral.stft(_offset_copy(x), n_fft, hop, centered=True, transform="fft")
    assert torch.equal(r2, re) and torch.equal(i2, im)
    y = spectral.istft(re, im, T, n_fft, hop, centered=True, transform="fft")
    assert torch.equal(spectral.istft(r1.contiguous(), i1.contiguous(), T, n_fft, hop, centered=True, transform="fft"), y[1:2, 2:3])
    assert torch.equal(spectral.istft(_offset_copy(re), _offset_copy(im), T, n_fft, hop, centered=True, transform="fft"), y)


def test_without_the_opt_in_4096_is_still_refused(lib):
    x = torch.zeros((1, 1, 9000, 1), device="cuda")
    with pytest.raises(NotImplementedError):
        spectral.stft(x, 4096, 1024, centered=True)
    with pytest.raises(NotImplementedError):
        postfilter.SoftMaskFilter(n_fft=4096, hop=1024)
