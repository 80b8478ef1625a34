"""GPU tests of Griffin-Lim phase reconstruction (include/wun.h: wun_griffin_lim; wave_u_net_amd.spectral.griffin_lim,
UnetSpectrogramSeparator.reconstruct, evaluate.separate_track(phase_iterations=N)) against the float64 oracle
tests/_griffin_lim_np.py.

Cases (n_fft / hop, T, rows, framing), the smallest shapes at which the mapping can go wrong:
    64 / 16     592   1  centred   odd log2 of the complex length, 32 frames per workgroup, two workgroups, the last partly filled
    128 / 32    700   3  centred   even log2, 16 frames per workgroup, three rows
    1024 / 768  4864  2  lead 0    the network's hop, no power of two; 2 frames per workgroup
    1024 / 256  3000  2  centred
    2048 / 512  5000  1  centred   one frame per workgroup, one butterfly per lane
    4096 / 1024 9000  1  centred   two butterflies per lane, odd log2
    8192 / 2048 24576 1  centred   four butterflies per lane, the LDS full (64 KB)
    64 / 16     5000  1  centred   316 frames: two blocks of 256, the second recomputes 3 frames of the first ("blocks")
    512 / 1     700   1  centred   1211 frames, 511 recomputed per block: more than a block's own 256 ("dense"; bit checks and momentum)

One-step rule: every iteration is judged against a float64 step of the oracle taken from the DEVICE's own previous audio
(teacher-forced): the phase of a bin is ill-conditioned where |c| is small, so errors are not comparable across iterations.
Pointwise the a priori bound of _griffin_lim_np.step_bound; over each tensor rms(err) <= 8 x the CPU float32 path's from the same
audio, floored at 2^-20 rms(y) (DESIGN.md 5.17's rule and margin).  Ratios seen on an MI355X: DESIGN.md 5.21."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from wave_u_net_amd import _lib, evaluate, spectral  # noqa: E402

_lib.load().wun_griffin_lim                          # the feature: an AttributeError without it

import _fft_np as fo  # noqa: E402
import _griffin_lim_np as gl  # noqa: E402
from _observed import record  # noqa: E402
from _unaligned import _offset_copy  # noqa: E402
from test_griffin_lim_host import cpu_step, one_step_check  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {"64": (64, 16, 592, 1, True), "128": (128, 32, 700, 3, True), "1024net": (1024, 768, 4864, 2, False),
         "1024": (1024, 256, 3000, 2, True), "2048": (2048, 512, 5000, 1, True), "4096": (4096, 1024, 9000, 1, True),
         "8192": (8192, 2048, 3 * 8192, 1, True), "blocks": (64, 16, 5000, 1, True), "dense": (512, 1, 700, 1, True)}
ONE_STEP = [c for c in sorted(CASES) if c != "dense"]
BITS = ["64", "1024net", "2048", "blocks", "dense"]          # the bit-for-bit checks: every frames-per-workgroup regime and two blocks
U = 2.0 ** -24
_CACHE = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def _case(name):
    """The inputs of a case on the host and the device, computed once and left unchanged."""
    if name not in _CACHE:
        n_fft, hop, T, R, centered = CASES[name]
        lead, F = fo.framing(T, n_fft, hop, centered)
        mag, y0 = gl.fixture(n_fft + hop + R, R, T, n_fft, hop, lead, F)
        rng = np.random.RandomState(T)
        c0 = (rng.rand(R, F, n_fft // 2 + 1) + 1j * rng.uniform(-np.pi, np.pi, (R, F, n_fft // 2 + 1))).astype(np.complex64)
        _CACHE[name] = {"n_fft": n_fft, "hop": hop, "T": T, "R": R, "lead": lead, "F": F, "mag": mag, "y0": y0, "c0": c0,
                        "dmag": torch.from_numpy(mag).cuda(), "dy0": torch.from_numpy(y0).cuda(),
                        "dre": torch.from_numpy(np.ascontiguousarray(c0.real)).cuda(),
                        "dim": torch.from_numpy(np.ascontiguousarray(c0.imag)).cuda()}
    return _CACHE[name]


def _run(k, iterations=1, start="audio", momentum=0.0, y_init=None, **kw):
    """wun_griffin_lim on a case's device inputs -> y [R, T] (device)."""
    if start == "audio":
        return spectral.griffin_lim_call(k["dmag"], None, None, k["dy0"] if y_init is None else y_init, k["T"], k["n_fft"], k["hop"],
                                         k["lead"], iterations, momentum, **kw)
    return spectral.griffin_lim_call(k["dmag"], k["dre"], k["dim"], None, k["T"], k["n_fft"], k["hop"], k["lead"], iterations,
                                     momentum, **kw)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------ 1. the one-step rule
@pytest.mark.parametrize("start", ["audio", "spectrum"])
@pytest.mark.parametrize("name", ONE_STEP)
def test_one_step_rule(lib, name, start):
    k = _case(name)
    n_fft, hop, T, lead, F, mag = k["n_fft"], k["hop"], k["T"], k["lead"], k["F"], k["mag"]
    steps_n = 4
    inc = torch.zeros((steps_n, 2), dtype=torch.float64, device="cuda")
    prev, steps, stand_in = [k["y0"] if start == "audio" else None], [], []
    for i in range(steps_n):
        if i == 0:
            y = _run(k, 1, start, inconsistency=inc[0:1])
            stand_in.append(cpu_step(prev[0], mag, n_fft, hop, lead, T, c0=None if start == "audio" else k["c0"]))
        else:
            y = _run(k, 1, "audio", y_init=steps[-1], inconsistency=inc[i:i + 1])
            stand_in.append(cpu_step(prev[i], mag, n_fft, hop, lead, T))
        steps.append(y)
        prev.append(y.cpu().numpy())
    got = [s.cpu().numpy() for s in steps]
    tag = "test_one_step_rule[%s-%s]" % (name, start)
    first_c = None if start == "audio" else gl.given(k["c0"].real, k["c0"].imag)
    # the condition on the inputs, with the CPU stand-in, before the device is judged
    one_step_check(tag + " stand-in", prev, stand_in, mag, n_fft, hop, lead, first_c=first_c)
    one_step_check(tag, prev, got, mag, n_fft, hop, lead, stand_in_steps=stand_in, first_c=first_c)
    # the inconsistency of every step that ran a forward transform: relative 32 u, floored by the conditioning of |c|
    inc = inc.cpu().numpy()
    worst = 0.0
    for i in range(steps_n):
        if i == 0 and start == "spectrum":
            assert np.isnan(inc[0]).all()
            continue
        c = gl.forward(prev[i], n_fft, hop, lead, F)
        want = gl.inconsistency(c, mag)
        b = gl.beta(prev[i], n_fft, hop, lead, F)[:, :, None]
        floor = (2.0 * np.sqrt(2.0) * b * np.abs(np.abs(c) - mag) + 2.0 * b * b).sum()
        tol = 32 * U * want + np.array([floor, 0.0])
        worst = max(worst, (np.abs(inc[i] - want) / tol).max())
        assert (np.abs(inc[i] - want) <= tol).all(), (i, inc[i], want, tol)
    record(tag, "inconsistency err / tolerance", worst, 1.0)


@pytest.mark.parametrize("name", BITS)
def test_momentum_first_step_is_the_plain_one(lib, name):
    k = _case(name)
    assert _same(_run(k, 1, momentum=0.99), _run(k, 1)) and _same(_run(k, 1, "spectrum", momentum=0.5), _run(k, 1, "spectrum"))


@pytest.mark.parametrize("name", ["64", "1024", "2048", "blocks", "dense"])
def test_momentum_step(lib, name):
    """The second accelerated step against the oracle's, taken from the device's first audio: t_1 = c_1 + m (c_1 - c_0) carries
    (1 + m) beta_1 + m beta_0.  (Centred cases: at lead 0 the first samples divide by window squares near 1e-8 and the tripled
    bound misses the condition on the inputs.)"""
    k = _case(name)
    n_fft, hop, T, lead, F, mag, m = k["n_fft"], k["hop"], k["T"], k["lead"], k["F"], k["mag"], 0.99
    y0_dev = _run(k, 1)
    y1 = _run(k, 2, momentum=m).cpu().numpy()
    assert not np.array_equal(y1, _run(k, 2).cpu().numpy())
    c0 = gl.forward(k["y0"], n_fft, hop, lead, F)
    c1 = gl.forward(y0_dev.cpu().numpy(), n_fft, hop, lead, F)
    t1 = c1 + float(np.float32(m)) * (c1 - c0)
    want = gl.project_invert(t1, mag, T, n_fft, hop, lead)
    fb = (1 + m) * gl.beta(y0_dev.cpu().numpy(), n_fft, hop, lead, F) + m * gl.beta(k["y0"], n_fft, hop, lead, F)
    bound, saturated = gl.step_bound(t1, mag, want, T, n_fft, hop, lead, fb)
    assert bound.max() <= 1e-2 * np.abs(want).max() and saturated <= 0.01
    err = np.abs(y1 - want)
    record("test_momentum_step[%s]" % name, "worst err / bound", (err / np.maximum(bound, 1e-300)).max(), 1.0)
    assert np.isfinite(y1).all() and (err <= bound).all()


# ------------------------------------------------------------------------------------------ 2. bit for bit
@pytest.mark.parametrize("name", BITS)
def test_one_call_is_the_chain_of_its_steps(lib, name):
    k = _case(name)
    inc_chain = torch.zeros((5, 2), dtype=torch.float64, device="cuda")
    chain = [_run(k, 1, inconsistency=inc_chain[0:1])]
    for i in range(1, 5):
        chain.append(_run(k, 1, y_init=chain[-1], inconsistency=inc_chain[i:i + 1]))
    for n in (4, 5):                                     # both parities of the ping-pong
        inc = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
        assert _same(_run(k, n, inconsistency=inc), chain[n - 1])
        assert np.array_equal(inc.cpu().numpy(), inc_chain[:n].cpu().numpy())
        y = k["dy0"].clone()                             # y_init may be y itself
        assert _same(_run(k, n, y_init=y, y=y), chain[n - 1])
    spec = [_run(k, 1, "spectrum")]
    for i in range(1, 3):
        spec.append(_run(k, 1, y_init=spec[-1]))
    assert _same(_run(k, 3, "spectrum"), spec[2])
    # momentum: carried inside one call; with the inconsistency asked for or not, the same audio
    inc = torch.zeros((5, 2), dtype=torch.float64, device="cuda")
    fast = _run(k, 5, momentum=0.5)
    assert _same(_run(k, 5, momentum=0.5, inconsistency=inc), fast) and not _same(fast, chain[4])
    assert np.array_equal(inc[:2].cpu().numpy(), inc_chain[:2].cpu().numpy())      # (the first two steps start from the same audio)
    assert bool(torch.isfinite(fast).all()) and bool(torch.isfinite(inc).all())


@pytest.mark.parametrize("momentum", [0.0, 0.99])
@pytest.mark.parametrize("name", BITS)
def test_scratch_alignment_stream_and_guards(lib, name, momentum):
    k = _case(name)
    n_fft, hop, T, R, lead, F = k["n_fft"], k["hop"], k["T"], k["R"], k["lead"], k["F"]
    K = n_fft // 2 + 1
    want = _run(k, 3, momentum=momentum)
    assert _same(_run(k, 3, momentum=momentum), want)                              # a repeated call
    n_small = lib.wun_griffin_lim_scratch_floats(R, 1, T, 1, n_fft, hop, lead, F, 0)
    n_big = lib.wun_griffin_lim_scratch_floats(R, 1, T, 1, n_fft, hop, lead, F, 1)
    assert n_small + 2 * R * F * K == n_big
    n = n_big if momentum else n_small                   # momentum 0 never needs (or touches) the c_{i-1} buffer
    G = 64
    for fill in (float("nan"), 0.0):
        buf = torch.full((n + 2 * G,), fill, dtype=torch.float32, device="cuda")
        buf[:G] = 7.0
        buf[G + n:] = 7.0
        ybuf = torch.full((R * T + 2 * G,), 7.0, dtype=torch.float32, device="cuda")
        y = ybuf[G:G + R * T].view(R, T)
        _run(k, 3, momentum=momentum, y=y, scratch=buf[G:G + n])
        assert _same(y, want)
        assert bool((buf[:G] == 7.0).all()) and bool((buf[G + n:] == 7.0).all())
        assert bool((ybuf[:G] == 7.0).all()) and bool((ybuf[G + R * T:] == 7.0).all())
    # every buffer one float off 8- and 16-byte alignment
    off = [_offset_copy(k[t]) for t in ("dmag", "dy0", "dre", "dim")]
    table = _offset_copy(spectral._fft_table(n_fft, torch.device("cuda", torch.cuda.current_device())))
    y = _offset_copy(torch.zeros(R, T, device="cuda"))
    scratch = _offset_copy(torch.zeros(n, device="cuda"))
    inc = torch.zeros((3, 2), dtype=torch.float64, device="cuda")
    for start in ("audio", "spectrum"):
        rc = lib.wun_griffin_lim(off[0].data_ptr(), *((None, None, off[1].data_ptr()) if start == "audio" else
                                                      (off[2].data_ptr(), off[3].data_ptr(), None)),
                                 R, 1, T, 1, n_fft, hop, lead, F, 3, momentum, table.data_ptr(), y.data_ptr(), inc.data_ptr(),
                                 scratch.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, lib.wun_last_error()
        assert _same(y, want if start == "audio" else _run(k, 3, "spectrum", momentum=momentum))
    # a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y_side = _run(k, 3, momentum=momentum)
    side.synchronize()
    assert _same(y_side, want)


def _direct(lib, mag, y_init, S, B, T, Cn, n_fft, hop, lead, F, iterations=1):
    """The C call on audio [S, B, T, Cn] with the caller's own framing."""
    n = lib.wun_griffin_lim_scratch_floats(S, B, T, Cn, n_fft, hop, lead, F, 0)
    assert n > 0
    scratch = torch.empty(n, dtype=torch.float32, device="cuda")
    y = torch.full((S, B, T, Cn), float("nan"), dtype=torch.float32, device="cuda")
    rc = lib.wun_griffin_lim(mag.data_ptr(), None, None, y_init.data_ptr(), S, B, T, Cn, n_fft, hop, lead, F, iterations, 0.0,
                             spectral._fft_table(n_fft, mag.device).data_ptr(), y.data_ptr(), None, scratch.data_ptr(),
                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.wun_last_error()
    return y


def test_rows_are_channel_last_audio(lib):
    """Rows r = (s B + b) C + c of audio [S, B, T, C]: the stereo call is the row call on the transposed audio, bit for bit."""
    k = _case("128")
    n_fft, hop, T, lead, F = k["n_fft"], k["hop"], k["T"], k["lead"], k["F"]
    rng = np.random.RandomState(4)
    S, B, Cn = 2, 1, 2
    mag = torch.from_numpy(np.abs(rng.randn(S * B * Cn, F, n_fft // 2 + 1)).astype(np.float32)).cuda()
    x = torch.from_numpy((0.3 * rng.randn(S, B, T, Cn)).astype(np.float32)).cuda()
    got = _direct(lib, mag, x, S, B, T, Cn, n_fft, hop, lead, F, 2)
    rows = x.permute(0, 1, 3, 2).reshape(S * B * Cn, T).contiguous()
    want = spectral.griffin_lim_call(mag, None, None, rows, T, n_fft, hop, lead, 2)
    assert _same(got.permute(0, 1, 3, 2).reshape(S * B * Cn, T).contiguous(), want)


def test_a_frame_does_not_depend_on_its_neighbours(lib):
    """64 / 16, lead 0: frame 0 alone in its workgroup (F = 1) and with 31 others (F = 37) -- the samples only frame 0 covers."""
    n_fft, hop = 64, 16
    rng = np.random.RandomState(12)
    x = (0.3 * rng.randn(1, 1, 36 * hop + n_fft, 1)).astype(np.float32)
    mag = np.abs(rng.randn(1, 37, 33)).astype(np.float32)
    many = _direct(lib, torch.from_numpy(mag).cuda(), torch.from_numpy(x).cuda(), 1, 1, x.shape[2], 1, n_fft, hop, 0, 37)
    one = _direct(lib, torch.from_numpy(mag[:, :1].copy()).cuda(), torch.from_numpy(x[:, :, :n_fft].copy()).cuda(), 1, 1, n_fft, 1,
                  n_fft, hop, 0, 1)
    assert bool(torch.isfinite(many).all()) and _same(many[0, 0, :hop, 0], one[0, 0, :hop, 0])
    assert bool((one[0, 0, 0, 0] == 0).all())                                       # w[0] = 0: below the 1e-8 rule


@pytest.mark.parametrize("name", ["64", "2048"])
def test_a_nan_magnitude_stays_in_its_frame(lib, name):
    k = _case(name)
    n_fft, hop, T, lead, F = k["n_fft"], k["hop"], k["T"], k["lead"], k["F"]
    f = F // 2
    mag = k["dmag"].clone()
    mag[0, f, 5] = float("nan")
    y = spectral.griffin_lim_call(mag, None, None, k["dy0"], T, n_fft, hop, lead, 1).cpu().numpy()
    lo, hi = max(0, f * hop - lead), min(T, f * hop - lead + n_fft)
    want = np.zeros(y.shape, bool)
    want[0, lo:hi] = True
    assert np.array_equal(np.isnan(y), want)
    clean = _run(k, 1).cpu().numpy()
    assert np.array_equal(y[~want].view(np.uint32), clean[~want].view(np.uint32))


@pytest.mark.parametrize("name", ["64", "1024net", "2048", "8192"])
def test_unit_of_zero_tiny_and_huge(lib, name):
    """A zero spectrum gives S = mag exactly: the audio is wun_istft_fft's of (mag, 0), bit for bit -- the inverse half IS that
    entry's.  Spectra of modulus 1e-30 and 1e30 give what modulus 1 gives, each unit within 4 u of the true one."""
    k = _case(name)
    n_fft, hop, T, R, lead, F, mag = k["n_fft"], k["hop"], k["T"], k["R"], k["lead"], k["F"], k["mag"]
    zero = torch.zeros_like(k["dmag"])
    got = spectral.griffin_lim_call(k["dmag"], zero, zero, None, T, n_fft, hop, lead, 1)
    centred = lead != 0
    want = spectral.istft(k["dmag"].view(R, 1, 1, F, -1), zero.view(R, 1, 1, F, -1), T, n_fft, hop, centered=centred, transform="fft")
    assert _same(got, want.reshape(R, T))
    u = k["c0"] / np.abs(k["c0"])
    c64 = gl.given(u.real, u.imag)
    y64 = gl.project_invert(c64, mag, T, n_fft, hop, lead)
    bound, _ = gl.step_bound(c64, mag, y64, T, n_fft, hop, lead, delta=8 * U)          # 4 u for the scaled float32 input's own
    for scale in (1.0, 1e-30, 1e30):                                                  # rounding, 4 u for the unit
        re, im = (torch.from_numpy(np.ascontiguousarray((p * scale).astype(np.float32))).cuda() for p in (u.real, u.imag))
        y = spectral.griffin_lim_call(k["dmag"], re, im, None, T, n_fft, hop, lead, 1).cpu().numpy()
        err = np.abs(y - y64)
        record("test_unit_of_zero_tiny_and_huge[%s]" % name, "scale %g: worst err / bound" % scale,
               (err / np.maximum(bound, 1e-300))[bound > 0].max(), 1.0)
        assert np.isfinite(y).all() and (err <= bound).all()


# ------------------------------------------------------------------------------------------ 3. through Python
def test_python_entry(lib):
    k = _case("128")
    n_fft, hop, T, R, F = k["n_fft"], k["hop"], k["T"], k["R"], k["F"]
    mag = k["dmag"].view(R, 1, F, -1)
    g = torch.Generator(device="cuda").manual_seed(7)
    y, inc = spectral.griffin_lim(mag, n_fft, hop, iterations=6, length=T, generator=g, return_inconsistency=True)
    assert tuple(y.shape) == (R, 1, T) and tuple(inc.shape) == (6, 2) and inc.dtype == torch.float64
    again = spectral.griffin_lim(mag, n_fft, hop, iterations=6, length=T, generator=torch.Generator(device="cuda").manual_seed(7))
    assert _same(y, again)
    g = torch.Generator(device="cuda").manual_seed(7)                               # the same draw, handed to the C call
    re = torch.rand(k["dmag"].shape, generator=g, dtype=torch.float32, device="cuda")
    im = (torch.rand(k["dmag"].shape, generator=g, dtype=torch.float32, device="cuda") * 2.0 - 1.0) * float(np.pi)
    assert bool((re >= 0).all()) and bool((im.abs() <= np.pi).all())
    direct = spectral.griffin_lim_call(k["dmag"], re, im, None, T, n_fft, hop, k["lead"], 6)
    assert _same(y.reshape(R, T), direct)
    inc = inc.cpu().numpy()
    assert np.isnan(inc[0]).all() and (np.diff(inc[1:, 0]) < 0).all() and (inc[1:, 1] == inc[1, 1]).all()
    # an audio start, the default length, momentum
    T0 = spectral.griffin_lim_default_length(F, n_fft, hop)
    y0 = spectral.griffin_lim(mag, n_fft, hop, iterations=2, init=torch.zeros(R, 1, T0, device="cuda"), momentum=0.99)
    assert tuple(y0.shape) == (R, 1, T0) and bool(torch.isfinite(y0).all())
    # the CPU path computes the same definition: close, not equal
    cpu = spectral.griffin_lim(mag.cpu(), n_fft, hop, iterations=1, init=(re.view_as(mag).cpu(), im.view_as(mag).cpu()), length=T)
    dev = spectral.griffin_lim(mag, n_fft, hop, iterations=1, init=(re.view_as(mag), im.view_as(mag)), length=T)
    assert float((cpu - dev.cpu()).abs().max()) <= 1e-4 * float(cpu.abs().max())


def _spec_separator():
    import _specunet_np as so
    import wave_u_net_amd as wun
    from wave_u_net_amd import UnetSpectrogramSeparator
    n_fft, hop, L, nif, F, B = 64, 48, 2, 3, 8, 2                                   # the `skip` geometry of test_gpu_specunet.py
    T = (F - 1) * hop + n_fft
    cfg = wun.get_config("unet_spectrogram", num_layers=L, num_initial_filters=nif, spec_frame_len=n_fft, spec_hop=hop,
                         num_frames=T, batch_size=B)
    sep = UnetSpectrogramSeparator(cfg, device="cuda:0")
    sep.load_variables(so.random_variables(L, nif, seed=23 + L))
    mix = (0.3 * np.random.RandomState(17 + L + F).randn(B, T, 1)).astype(np.float32)
    return cfg, sep, mix, (n_fft, hop, F, B, T)


def test_reconstruct_from_the_mix_phase(lib):
    cfg, sep, mix, (n_fft, hop, F, B, T) = _spec_separator()
    dmix = torch.from_numpy(mix).cuda()
    outs = sep.get_output(dmix, False, return_spectrogram=True)
    mags = torch.stack([outs[n] for n in sep.source_names]).clone()                 # [S, B, F, K]
    S, K = 2, n_fft // 2 + 1
    y = sep.reconstruct(outs, dmix, 1)
    assert sorted(y) == sorted(sep.source_names) and all(tuple(v.shape) == (B, T, 1) for v in y.values())
    got = torch.stack([y[n] for n in sep.source_names]).reshape(S * B, T).cpu().numpy()
    re, im = spectral.stft(dmix.view(1, B, T, 1), n_fft, hop, transform="fft")      # the spectrum the device started from
    c0 = np.tile((re.cpu().numpy() + 1j * im.cpu().numpy()).reshape(B, F, K).astype(np.complex64), (S, 1, 1))
    mag = mags.reshape(S * B, F, K).cpu().numpy()
    stand_in = cpu_step(None, mag, n_fft, hop, 0, T, c0=c0)
    one_step_check("test_reconstruct_from_the_mix_phase", [None], [got], mag, n_fft, hop, 0, stand_in_steps=[stand_in],
                   first_c=gl.given(c0.real, c0.imag))
    # eight iterations are more consistent than one (measured by the oracle on the device's audio)
    y8 = sep.reconstruct(mags, dmix, 8)
    got8 = torch.stack([y8[n] for n in sep.source_names]).reshape(S * B, T).cpu().numpy()
    d1 = gl.inconsistency(gl.forward(got, n_fft, hop, 0, F), mag)[0]
    d8 = gl.inconsistency(gl.forward(got8, n_fft, hop, 0, F), mag)[0]
    record("test_reconstruct_from_the_mix_phase", "inconsistency after 8 / after 1", d8 / d1, 1.0)
    assert d8 < d1


def test_separate_track_phase_iterations(lib):
    cfg, sep, _, (n_fft, hop, F, B, T) = _spec_separator()
    audio = (0.3 * np.random.RandomState(4).randn(int(2.5 * T), 1)).astype(np.float32)
    plain = evaluate.separate_track(cfg, sep, audio, cfg["expected_sr"])
    zero = evaluate.separate_track(cfg, sep, audio, cfg["expected_sr"], phase_iterations=0)
    assert all(np.array_equal(plain[n].view(np.uint32), zero[n].view(np.uint32)) for n in cfg["source_names"])
    refined = evaluate.separate_track(cfg, sep, audio, cfg["expected_sr"], phase_iterations=3)
    for n in cfg["source_names"]:
        assert refined[n].shape == plain[n].shape and np.isfinite(refined[n]).all() and not np.array_equal(refined[n], plain[n])
