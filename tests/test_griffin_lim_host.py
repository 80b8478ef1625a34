"""CPU-only checks of Griffin-Lim phase reconstruction (include/wun.h: wun_griffin_lim, wun_griffin_lim_scratch_floats;
wave_u_net_amd.spectral.griffin_lim): the float64 oracle tests/_griffin_lim_np.py against an independent
torch.fft computation, the CPU float32 path against the oracle under the one-step rule, the two properties that hold only for the
least-squares inverse (the inconsistency never increases; a consistent spectrogram with its own phase is a fixed point), every
refusal of the C entry in its documented order, the scratch formula, and the Python surface.  The device path is checked in
tests/test_gpu_griffin_lim.py."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fft_np as fo  # noqa: E402
import _griffin_lim_np as gl  # noqa: E402
from _observed import record  # noqa: E402
from test_postfilter_host import FakeSeparator  # noqa: E402

import wave_u_net_amd as wun  # noqa: E402
from wave_u_net_amd import _lib, spectral  # noqa: E402
from wave_u_net_amd.evaluate import separate_track  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wun_griffin_lim_scratch_floats", "wun_griffin_lim")
INVALID, UNSUPPORTED = -1, -2
P, Q, R3, R4, R5, R6 = 0x100000, 0x40000000, 0x80000000, 0xC0000000, 0x100000000, 0x140000000   # "device pointers": never read
BAD_N_FFT = (0, 32, 96, 100, 16384)
# (n_fft, hop, T, centred): the sizes the one-step bound was tried on before the device was judged by it
STEP_CASES = [(64, 16, 592, True), (128, 32, 700, True), (1024, 256, 3000, True), (1024, 768, 4864, False)]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_declared_exported_and_documented(lib):
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert "`%s`" % name in doc, name


# ---- the oracle ----------------------------------------------------------------------------------------
def _torch_step(y, mag, n_fft, hop, lead, F):
    """One plain step in float64 with torch.fft and an explicit overlap-add loop: nothing shared with the oracle's code."""
    y = torch.from_numpy(np.asarray(y, np.float64))
    R, T = y.shape
    n = torch.arange(n_fft, dtype=torch.float64)
    w = 0.5 - 0.5 * torch.cos(2 * math.pi * n / n_fft)
    total = max((F - 1) * hop + n_fft, lead + T)
    pad = torch.zeros(R, total, dtype=torch.float64)
    pad[:, lead:lead + T] = y
    frames = torch.stack([pad[:, f * hop:f * hop + n_fft] for f in range(F)], 1) * w
    c = torch.fft.rfft(frames, dim=-1)
    a = c.abs()
    u = torch.where(a == 0, torch.ones_like(c), c / torch.where(a == 0, torch.ones_like(a), a))
    s = torch.from_numpy(np.asarray(mag, np.float64)) * u
    s[..., 0] = s[..., 0].real + 0j
    s[..., -1] = s[..., -1].real + 0j
    fr = torch.fft.irfft(s, n=n_fft, dim=-1) * w
    num, den = torch.zeros(R, total, dtype=torch.float64), torch.zeros(total, dtype=torch.float64)
    for f in range(F):
        num[:, f * hop:f * hop + n_fft] += fr[:, f]
        den[f * hop:f * hop + n_fft] += w * w
    out = torch.where(den >= 1e-8, num / torch.where(den >= 1e-8, den, torch.ones_like(den)), torch.zeros_like(num))
    return out[:, lead:lead + T].numpy(), c.numpy()


@pytest.mark.parametrize("n_fft, hop, T, centered", STEP_CASES)
def test_oracle_step_against_torch_fft(n_fft, hop, T, centered):
    lead, F = fo.framing(T, n_fft, hop, centered)
    mag, y0 = gl.fixture(3, 2, T, n_fft, hop, lead, F)
    want, c_want = _torch_step(y0, mag, n_fft, hop, lead, F)
    got, c, inc = gl.step(y0, mag, n_fft, hop, lead)
    assert np.abs(c - c_want).max() < 1e-10 and np.abs(got - want).max() < 1e-10
    assert np.allclose(inc, [((np.abs(c_want) - mag) ** 2).sum(), (mag.astype(np.float64) ** 2).sum()], rtol=1e-12)


def test_unit():
    c = np.array([0, 3 + 4j, -2.0, 1e-300j, 1e300 - 1e300j])
    u = gl.unit(c)
    assert u[0] == 1 and np.allclose(u[1:], [0.6 + 0.8j, -1, 1j, (1 - 1j) / np.sqrt(2)], rtol=1e-15)
    t = torch.complex(torch.tensor([0.0, -0.0, 3.0, 1e-30, 1e30, float("nan"), 0.0]),
                      torch.tensor([0.0, 0.0, 4.0, -1e-30, 1e30, 0.0, float("nan")]))
    u32 = spectral._gl_unit(t)
    assert u32[0] == 1 and u32[1] == 1
    assert torch.allclose(torch.view_as_real(u32[2:5]), torch.tensor([[0.6, 0.8], [2 ** -0.5, -2 ** -0.5], [2 ** -0.5, 2 ** -0.5]]),
                          rtol=4 * 2.0 ** -24, atol=0)
    assert torch.isnan(torch.view_as_real(u32[5])).any() and torch.isnan(torch.view_as_real(u32[6])).any()


# ---- the CPU float32 path under the one-step rule ------------------------------------------------------
def one_step_check(tag, prev_audio, got_steps, mag, n_fft, hop, lead, stand_in_steps=None, first_c=None):
    """DESIGN.md 5.21's one-step rule for got_steps[i] = a float32 evaluation of step i taken from prev_audio[i] (its own previous
    audio, teacher-forced; step 0 from the spectrum first_c when that is given): the a priori pointwise bound, and -- with
    stand_in_steps, the CPU float32 path's steps from the same audio -- rms(err) <= 8 x rms(stand-in err), floored at 2^-20 of
    rms(y_64).  Returns the worst err / bound and err-rms / allowed-rms."""
    T, F = got_steps[0].shape[1], mag.shape[1]
    worst, worst_rms = 0.0, 0.0
    for i, got in enumerate(got_steps):
        if i == 0 and first_c is not None:
            c, fb = first_c, None
        else:
            c = gl.forward(prev_audio[i], n_fft, hop, lead, F)
            fb = gl.beta(prev_audio[i], n_fft, hop, lead, F)
        y64 = gl.project_invert(c, mag, T, n_fft, hop, lead)
        bound, saturated = gl.step_bound(c, mag, y64, T, n_fft, hop, lead, fb)
        # the condition on the inputs: a usable bound, few ill-conditioned bins
        assert bound.max() <= 1e-2 * np.abs(y64).max(), (tag, i, bound.max() / np.abs(y64).max())
        assert saturated <= 0.01, (tag, i, saturated)
        err = np.abs(np.asarray(got, np.float64) - y64)
        assert np.isfinite(got).all()
        ratio = (err / np.maximum(bound, 1e-300))[bound > 0].max()
        assert (err[bound == 0] == 0).all()
        worst = max(worst, ratio)
        assert (err <= bound).all(), (tag, i, ratio)
        if stand_in_steps is not None:
            allowed = max(8.0 * gl.rms(np.asarray(stand_in_steps[i], np.float64) - y64), 2.0 ** -20 * gl.rms(y64))
            worst_rms = max(worst_rms, gl.rms(err) / allowed)
            assert gl.rms(err) <= allowed, (tag, i, gl.rms(err) / allowed)
    record(tag, "worst err / bound", worst, 1.0)
    if stand_in_steps is not None:
        record(tag, "worst rms err / allowed", worst_rms, 1.0)
    return worst, worst_rms


def cpu_step(prev, mag, n_fft, hop, lead, T, c0=None):
    """One float32 step of the CPU path from audio `prev` [R, T] (or, with prev None, the complex64 spectrum c0)."""
    y, _ = spectral.griffin_lim_torch(torch.from_numpy(mag), None if c0 is None else torch.from_numpy(c0),
                                      None if prev is None else torch.from_numpy(np.ascontiguousarray(prev, dtype=np.float32)),
                                      T, n_fft, hop, lead, 1)
    return y.numpy()


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("n_fft, hop, T, centered", STEP_CASES)
def test_cpu_path_obeys_the_one_step_rule(n_fft, hop, T, centered, seed):
    lead, F = fo.framing(T, n_fft, hop, centered)
    mag, y0 = gl.fixture(seed, 2, T, n_fft, hop, lead, F)
    prev, steps = [y0], []
    for _ in range(8):
        steps.append(cpu_step(prev[-1], mag, n_fft, hop, lead, T))
        prev.append(steps[-1])
    one_step_check("test_cpu_path_obeys_the_one_step_rule[%d-%d-%d]" % (n_fft, hop, seed), prev, steps, mag, n_fft, hop, lead)
    # the whole iteration in one call is the chain of its steps
    y, inc = spectral.griffin_lim_torch(torch.from_numpy(mag), None, torch.from_numpy(y0), T, n_fft, hop, lead, 8)
    assert np.array_equal(y.numpy(), steps[-1])
    _, inc64, _ = gl.iterate(mag, T, n_fft, hop, lead, 8, y0=y0)
    assert np.allclose(inc.numpy(), inc64, rtol=1e-3)


# ---- properties of the least-squares inverse -----------------------------------------------------------
@pytest.mark.parametrize("n_fft, hop, T, centered", [(64, 16, 592, True), (128, 96, 900, False), (256, 64, 1500, True)])
def test_inconsistency_never_increases(n_fft, hop, T, centered):
    """Griffin & Lim's theorem for the window-square-normalised inverse; another normaliser (the steady-state sum at the edges,
    or none) breaks it."""
    lead, F = fo.framing(T, n_fft, hop, centered)
    mag, _ = gl.fixture(5, 1, T, n_fft, hop, lead, F)
    rng = np.random.RandomState(6)
    c0 = gl.given(rng.rand(1, F, n_fft // 2 + 1), rng.uniform(-np.pi, np.pi, (1, F, n_fft // 2 + 1)))
    _, inc, _ = gl.iterate(mag, T, n_fft, hop, lead, 33, c0=c0)
    assert np.isnan(inc[0]).all() and np.isfinite(inc[1:]).all()
    d = inc[1:, 0]
    assert (d[1:] <= d[:-1] * (1 + 1e-12)).all() and d[-1] < 0.9 * d[0]
    # the same in the package's torch implementation at float64
    y, tinc = spectral.griffin_lim_torch(torch.from_numpy(mag), torch.from_numpy(c0), None, T, n_fft, hop, lead, 33, dtype=torch.float64)
    assert np.allclose(tinc.numpy()[1:], inc[1:], rtol=1e-9)


def test_consistent_spectrogram_is_a_fixed_point():
    n_fft, hop, T = 128, 32, 800
    lead, F = fo.framing(T, n_fft, hop, True)
    x = 0.3 * np.random.RandomState(8).randn(2, T)
    c = gl.forward(x, n_fft, hop, lead, F)
    y, inc, _ = gl.iterate(np.abs(c), T, n_fft, hop, lead, 3, c0=c)
    assert np.abs(y - x).max() < 1e-12 and inc[1:, 0].max() < 1e-20
    y, _, _ = gl.iterate(np.abs(c), T, n_fft, hop, lead, 3, y0=x, momentum=0.99)
    assert np.abs(y - x).max() < 1e-12


def test_momentum_is_the_accelerated_iteration():
    """t_i = c_i + momentum (c_i - c_{i-1}): equal to the plain path at the first step, different afterwards, and further along
    after 32 iterations on this input."""
    n_fft, hop, T = 64, 16, 592
    lead, F = fo.framing(T, n_fft, hop, True)
    mag, y0 = gl.fixture(9, 1, T, n_fft, hop, lead, F)
    _, plain, ys_p = gl.iterate(mag, T, n_fft, hop, lead, 32, y0=y0)
    _, fast, ys_f = gl.iterate(mag, T, n_fft, hop, lead, 32, y0=y0, momentum=0.99)
    assert np.array_equal(ys_p[0], ys_f[0]) and not np.array_equal(ys_p[1], ys_f[1])
    assert fast[-1, 0] < plain[-1, 0]
    y32, inc32 = spectral.griffin_lim_torch(torch.from_numpy(mag), None, torch.from_numpy(y0), T, n_fft, hop, lead, 4, momentum=0.99)
    assert np.abs(y32.numpy() - ys_f[3]).max() < 1e-3 * np.abs(ys_f[3]).max()


# ---- refusals of the C entry (no device is touched: every call must return from its checks) -----------
def _call(lib, mag=P, init_re=None, init_im=None, y_init=Q, S=2, B=3, T=200, Cn=2, n_fft=64, hop=16, lead=48, F=16, iterations=4,
          momentum=0.0, table=R3, y=R4, inconsistency=None, scratch=R5):
    return lib.wun_griffin_lim(mag, init_re, init_im, y_init, S, B, T, Cn, n_fft, hop, lead, F, iterations, momentum, table, y,
                               inconsistency, scratch, None)


def test_argument_errors_and_their_order(lib):
    for name in ("mag", "table", "y", "scratch"):
        assert _call(lib, **{name: None}) == INVALID and b"null" in lib.wun_last_error(), name
    for kw in ({"S": 0}, {"B": 0}, {"Cn": 0}, {"Cn": 3}, {"T": 0}, {"hop": 0}, {"hop": 65}, {"lead": -1}, {"lead": 64}, {"F": 0},
               {"F": -3}):
        assert _call(lib, **kw) == INVALID, kw
    for bad in BAD_N_FFT:
        assert _call(lib, n_fft=bad) == UNSUPPORTED, bad
    assert _call(lib, F=1 << 30) == UNSUPPORTED
    # the order: pointers, the audio shape, n_fft, hop, lead, F -- then this entry's own
    assert _call(lib, mag=None, n_fft=100) == INVALID and _call(lib, S=0, n_fft=100) == INVALID
    assert _call(lib, n_fft=100, hop=0) == UNSUPPORTED and _call(lib, n_fft=100, iterations=0) == UNSUPPORTED
    assert _call(lib, hop=0, iterations=0) == INVALID and b"hop" in lib.wun_last_error()
    assert _call(lib, F=0, iterations=0) == INVALID and b"F < 1" in lib.wun_last_error()
    for it in (0, -1):
        assert _call(lib, iterations=it) == INVALID and b"iterations" in lib.wun_last_error()
    assert _call(lib, iterations=0, momentum=2.0) == INVALID and b"iterations" in lib.wun_last_error()
    for m in (-0.01, 1.0, 1.5, float("nan"), float("inf"), -float("inf")):
        assert _call(lib, momentum=m) == INVALID and b"momentum" in lib.wun_last_error(), m
    assert _call(lib, momentum=1.0, y_init=None) == INVALID and b"momentum" in lib.wun_last_error()
    for kw in ({"y_init": None}, {"init_re": R6, "init_im": R6 + (1 << 24)}, {"init_re": R6}, {"init_im": R6},
               {"init_re": R6, "y_init": None}, {"init_im": R6, "y_init": None}):
        assert _call(lib, **kw) == INVALID and b"exactly one" in lib.wun_last_error(), kw
    assert _call(lib, y_init=None, y=P) == INVALID and b"exactly one" in lib.wun_last_error()      # before the overlap check
    E, NT = 12 * 16 * 33, 12 * 200                                                            # floats of a spectrum, of the audio
    for kw in ({"y": P}, {"y": P + 4 * (E - 1)}, {"mag": R4 + 4 * (NT - 1)}):
        assert _call(lib, **kw) == INVALID and b"overlaps" in lib.wun_last_error(), kw
    given = {"y_init": None, "init_re": R6, "init_im": R6 + (1 << 24)}
    for kw in ({"y": R6 + 4 * (E - 1)}, {"y": R6 + (1 << 24) - 4 * (NT - 1)}):
        assert _call(lib, **dict(given, **kw)) == INVALID and b"overlaps" in lib.wun_last_error(), kw
    # (legal neighbours of the refused layouts pass every check -- and would launch, so they are not called here)


def test_scratch_formula(lib):
    f = lib.wun_griffin_lim_scratch_floats
    for (S, B, T, Cn, n_fft, hop, lead, F) in [(2, 3, 200, 2, 64, 16, 48, 16), (1, 1, 5000, 1, 64, 16, 48, 316),
                                               (1, 2, 20000, 1, 8192, 2048, 6144, 13), (3, 1, 4864, 1, 1024, 768, 0, 6),
                                               (1, 1, 100000, 2, 256, 1, 255, 100255)]:
        R, K = S * B * Cn, n_fft // 2 + 1
        nb = min(F, 256 + -(-n_fft // hop) - 1)
        plain = R * nb * n_fft + R * T + 2 * n_fft + 4 * R * F + 2
        assert f(S, B, T, Cn, n_fft, hop, lead, F, 0) == plain
        assert f(S, B, T, Cn, n_fft, hop, lead, F, 1) == plain + 2 * R * F * K == f(S, B, T, Cn, n_fft, hop, lead, F, 7)
        # the frames of one block are wun_istft_fft's: the rest does not depend on the blocking
        assert plain - lib.wun_istft_fft_scratch_floats(S, B, T, Cn, n_fft, hop, lead, F) == R * T + 4 * R * F
    assert f(0, 1, 200, 1, 64, 16, 48, 16, 0) == INVALID and f(1, 1, 200, 1, 100, 16, 48, 16, 0) == UNSUPPORTED
    assert f(1, 1, 200, 1, 64, 0, 48, 16, 0) == INVALID and f(1, 1, 200, 1, 64, 16, 64, 16, 0) == INVALID
    assert f(1, 1, 200, 1, 64, 16, 48, 0, 0) == INVALID


# ---- the Python surface --------------------------------------------------------------------------------
def test_python_refusals_and_shapes():
    n_fft, hop = 64, 16
    F = 12
    mag = torch.rand(2, 3, F, 33)
    T = spectral.griffin_lim_default_length(F, n_fft, hop)
    assert T == F * hop - 48 and spectral.centered_frames(T, n_fft, hop, "fft") == F
    assert spectral.centered_frames(T + 1, n_fft, hop, "fft") == F + 1
    assert spectral.griffin_lim_default_length(F, n_fft, hop, centered=False) == (F - 1) * hop + n_fft
    g = torch.Generator().manual_seed(5)
    y = spectral.griffin_lim(mag, n_fft, hop, iterations=3, generator=g)
    assert tuple(y.shape) == (2, 3, T) and y.dtype == torch.float32 and bool(torch.isfinite(y).all())
    again = spectral.griffin_lim(mag, n_fft, hop, iterations=3, generator=torch.Generator().manual_seed(5))
    assert torch.equal(y, again)
    y2, inc = spectral.griffin_lim(mag, n_fft, hop, iterations=3, init=y, return_inconsistency=True)
    assert tuple(inc.shape) == (3, 2) and inc.dtype == torch.float64 and bool(torch.isfinite(inc).all())
    _, inc0 = spectral.griffin_lim(mag, n_fft, hop, iterations=2, init=(mag, torch.zeros_like(mag)), return_inconsistency=True)
    assert bool(torch.isnan(inc0[0]).all()) and bool(torch.isfinite(inc0[1]).all())
    short = spectral.griffin_lim(mag, n_fft, hop, iterations=1, init=(mag, mag), length=T - 5)
    assert tuple(short.shape) == (2, 3, T - 5)
    y3 = spectral.griffin_lim(mag[0, 0], n_fft, hop, iterations=1, init=(mag[0, 0], mag[0, 0]), centered=False)
    assert tuple(y3.shape) == ((F - 1) * hop + n_fft,)
    for kw in ({"iterations": 0}, {"momentum": 1.0}, {"momentum": -0.1}, {"momentum": float("nan")}, {"length": T + 1},
               {"length": T - hop}, {"init": (mag,)}, {"init": (mag, mag[0])}, {"init": torch.zeros(2, 3, T + 1)}, {"init": 3.0}):
        with pytest.raises(ValueError):
            spectral.griffin_lim(mag, n_fft, hop, **kw)
    with pytest.raises(ValueError):
        spectral.griffin_lim(mag, 128, 32)                                                    # 33 bins are not 128 / 2 + 1
    with pytest.raises(ValueError):
        spectral.griffin_lim(torch.rand(3, 65), 128, 32)                                      # 3 centred frames cover no sample
    with pytest.raises(NotImplementedError):
        spectral.griffin_lim(torch.rand(4, 51), 100, 25)                                      # no kernel for this n_fft


def test_phase_iterations_option():
    """phase_iterations=0 is the call without the option, bit for bit; N > 0 is the spectrogram U-Net's alone."""
    cfg = wun.get_config("baseline", mono_downmix=True)
    sr = cfg["expected_sr"]
    audio = np.random.default_rng(11).uniform(-1, 1, (1033, 2)).astype(np.float32)
    plain = separate_track(cfg, FakeSeparator(cfg, 1324, 300), audio, sr, batch_hops=4)
    zero = separate_track(cfg, FakeSeparator(cfg, 1324, 300), audio, sr, batch_hops=4, phase_iterations=0)
    assert all(np.array_equal(plain[k], zero[k]) for k in cfg["source_names"])
    with pytest.raises(NotImplementedError):
        separate_track(cfg, FakeSeparator(cfg, 1324, 300), audio, sr, batch_hops=4, phase_iterations=3)
    with pytest.raises(ValueError):
        separate_track(cfg, FakeSeparator(cfg, 1324, 300), audio, sr, batch_hops=4, phase_iterations=-1)
    from wave_u_net_amd import config
    assert "phase_iterations" not in config.EXTENSION_DEFAULTS                                 # a keyword only
    from wave_u_net_amd.__main__ import _phase_iterations
    assert _phase_iterations({}) == 0 and _phase_iterations({"phase_iterations": 10}) == 10
    for bad in (-1, 2.5, "ten", True):
        with pytest.raises(SystemExit):
            _phase_iterations({"phase_iterations": bad})
