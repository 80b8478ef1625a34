"""GPU sweep of the FFT family (wun_fft.hip): each of its eight kernel bodies -- forward, magnitude, the
spectrogram U-Net's head, inverse, adjoint, Griffin-Lim from audio and from a given spectrum, the vocoder's analysis -- at each of
its eight transform sizes, n_fft = 64 .. 8192, on the cases of tests/_fft_sweep_np.py (A: three rows that cross workgroups, B:
stereo at hop = 3 n_fft / 4, C: one frame, D: a centred track of 5 samples), against the float64 references the family tests use.

No bound of its own: every rule is the family test's, imported (beta / istft_bound and 8 x the float32 stand-in from
test_gpu_fft, the magnitude bound and the pinned-sign gradient of test_gpu_spectral_fft, `_rule` of test_gpu_specunet_backward,
the one-step rule of test_griffin_lim_host, TOL_ORACLE / TOL_IDENTITY of test_gpu_vocoder).  tests/test_fft_sweep_host.py shows
without a GPU that these rules refuse a dropped bin, a missing conjugate, a neighbour row's samples, a shifted window, doubled
edge bins and a wrong scale on these very cases.

Outputs live in NaN-filled arenas 1 to 3 floats past a 16-byte boundary (test_gpu_vocoder._Arena): afterwards every float of an
output is finite and every float outside is still NaN.  The module resets the library's launch ledger first and reads it last:
all 64 kernels (8 bodies x 8 sizes) must have run.  Ratios seen on an MI355X: profiles/fft_sweep_parity_observed.json."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from wave_u_net_amd import _lib, spectral, vocoder  # noqa: E402

_lib.load().wun_fft_launch_counts                    # the feature: an AttributeError without it

import _fft_sweep_np as sw  # noqa: E402
import _griffin_lim_np as gl  # noqa: E402
import _specunet_backward_np as bo  # noqa: E402
import _specunet_np as suo  # noqa: E402
import _spectral_np as sp  # noqa: E402
import _vocoder_np as vnp  # noqa: E402
import test_gpu_fft as family_fft  # noqa: E402
from _observed import record  # noqa: E402
from test_gpu_spectral_fft import _check_gradient, _loss, _pinned_signs  # noqa: E402
from test_gpu_specunet_backward import DOMAINS, _rule  # noqa: E402
from test_gpu_vocoder import TOL_IDENTITY, TOL_ORACLE, _Arena, _bits, _signal  # noqa: E402
from test_griffin_lim_host import cpu_step, one_step_check  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = sw.SIZES
FAMILIES = ["forward", "magnitude", "spec_head", "inverse", "adjoint", "griffin_lim", "griffin_lim_given", "voc_analysis"]
CELLS = _lib.FFT_FAMILY_COUNT * _lib.FFT_SIZE_COUNT


def _counts(lib):
    buf = (C.c_int64 * CELLS)()
    _lib.check(lib.wun_fft_launch_counts(buf, CELLS))
    return np.array(list(buf), dtype=np.int64).reshape(_lib.FFT_FAMILY_COUNT, _lib.FFT_SIZE_COUNT)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    lib = _lib.load()
    lib.wun_fft_launch_counts_reset()                    # the module's ledger starts at 0 (test_every_fft_kernel_was_exercised)
    assert not _counts(lib).any()
    return lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _table(n_fft):
    return spectral._fft_table(n_fft, torch.device(DEV))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _arena(*sizes):
    """An arena for outputs of these sizes and its views, the k-th at 1 + k mod 3 floats past a 16-byte boundary."""
    a = _Arena(sum(n + 12 for n in sizes) + 64)
    return a, [a.take(n, 1 + k % 3) for k, n in enumerate(sizes)]


def _footprint(arena, *views):
    """Every float of an output finite, every float outside still NaN."""
    torch.cuda.synchronize()
    assert arena.guards_intact()
    assert all(bool(torch.isfinite(v).all()) for v in views)


def _tag(test, n_fft, name, *more):
    return "fft_sweep::%s[%d-%s]" % (test, n_fft, "-".join((name,) + tuple(str(m) for m in more)))


def _judge(tag, verdict):
    ok, figs = verdict
    for what, (observed, tolerance) in sorted(figs.items()):
        record(tag, what, observed, tolerance)
    assert ok, (tag, figs)


def _forward(lib, x, c, re, im, F=None, T=None, lead=None):
    S, B, Cn = (int(v) for v in (x.shape[0], x.shape[1], x.shape[3]))
    _lib.check(lib.wun_stft_complex_fft(x.data_ptr(), S, B, int(x.shape[2]) if T is None else T, Cn, c["n_fft"], c["hop"],
                                        c["lead"] if lead is None else lead, c["F"] if F is None else F,
                                        _table(c["n_fft"]).data_ptr(), re.data_ptr(), im.data_ptr(), _stream()))


def _inverse(lib, re, im, shape, c, y, T=None, F=None, hop=None):
    S, B, Cn = shape
    T, F, hop = (c["T"] if T is None else T), (c["F"] if F is None else F), (c["hop"] if hop is None else hop)
    n = _lib.count(lib.wun_istft_fft_scratch_floats(S, B, T, Cn, c["n_fft"], hop, c["lead"], F))
    scratch = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(lib.wun_istft_fft(re.data_ptr(), im.data_ptr(), S, B, T, Cn, c["n_fft"], hop, c["lead"], F,
                                 _table(c["n_fft"]).data_ptr(), y.data_ptr(), scratch.data_ptr(), _stream()))


def _audio_rows(y, c, T=None):
    """An arena view holding [S, B, T, C] -> float64 rows [R, T]."""
    S, B, Cn = c["shape"]
    return sp.rows(y.cpu().numpy().reshape(S, B, c["T"] if T is None else T, Cn))


# ---------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("name", sw.CASE_NAMES)
@pytest.mark.parametrize("n_fft", SIZES)
def test_forward(lib, n_fft, name):
    c = sw.case(n_fft, name)
    ref = sw.signal(c)
    n = c["R"] * c["F"] * (n_fft // 2 + 1)
    arena, (re, im) = _arena(n, n)
    _forward(lib, _dev(ref["x"]), c, re, im)
    _footprint(arena, re, im)
    shape = (c["R"], c["F"], n_fft // 2 + 1)
    _judge(_tag("forward", n_fft, name), sw.forward_verdict(re.cpu().numpy().reshape(shape), im.cpu().numpy().reshape(shape), ref))


# ---------------------------------------------------------------------------------------------------- 2. inverse
@pytest.mark.parametrize("name", sw.CASE_NAMES)
@pytest.mark.parametrize("n_fft", SIZES)
def test_inverse(lib, n_fft, name):
    c = sw.case(n_fft, name)
    ref = sw.spectra(c)
    arena, (y, y2) = _arena(c["R"] * c["T"], c["R"] * c["T"])
    re, im = _dev(ref["re"]), _dev(ref["im"])
    _inverse(lib, re, im, c["shape"], c, y)
    im[..., 0] = float("nan")                            # garbage in Im of the bins 0 and n_fft / 2 changes no bit
    im[..., -1] = 1e30
    _inverse(lib, re, im, c["shape"], c, y2)
    _footprint(arena, y, y2)
    assert np.array_equal(_bits(y), _bits(y2))
    _judge(_tag("inverse", n_fft, name), sw.inverse_verdict(_audio_rows(y, c), ref))


# ---------------------------------------------------------------------------------------------------- 3. magnitude and adjoint
@pytest.mark.parametrize("name", sw.CASE_NAMES[:3])
@pytest.mark.parametrize("n_fft", SIZES)
def test_magnitude_and_adjoint(lib, n_fft, name):
    """wun_stft_magnitude_fft under the magnitude bound; then the one-term wun_spectral_loss_fft gradient at the signs of those
    very magnitudes (they may differ from float64's only where the reference's magnitudes tie within their bounds:
    _pinned_signs asserts that on the reference), 8 x the float32 yardstick."""
    c = sw.case(n_fft, name)
    ref = sw.loss_pair(c)
    S, B, Cn = c["shape"]
    shape = (c["R"], c["F"], n_fft // 2 + 1)
    n = int(np.prod(shape))
    arena, (me, mt, d_out) = _arena(n, n, c["R"] * c["T"])
    out, tgt = _dev(ref["out"]), _dev(ref["tgt"])
    for x, m in ((out, me), (tgt, mt)):
        _lib.check(lib.wun_stft_magnitude_fft(x.data_ptr(), S, B, c["T"], Cn, n_fft, c["hop"], _table(n_fft).data_ptr(),
                                              m.data_ptr(), _stream()))
    loss = _loss(ref, None)
    losses = torch.empty(loss.num_losses, dtype=torch.float32, device=DEV)
    scratch = torch.full((loss.scratch_floats(out.shape),), float("nan"), dtype=torch.float32, device=DEV)
    loss.run(out, tgt, d_out.view(out.shape), losses, scratch)
    _footprint(arena, me, mt, d_out)
    tag = _tag("magnitude", n_fft, name)
    for what, x, m in (("estimates", ref["out"], me), ("targets", ref["tgt"], mt)):
        ok, figs = sw.magnitude_verdict(m.cpu().numpy().reshape(shape), x, n_fft, c["hop"])
        record(tag, "%s err / bound" % what, figs["err / bound"][0], 1.0)
        assert ok, (tag, what, figs)
    ref["gpu_mags"] = [(me.cpu().numpy().reshape(shape), mt.cpu().numpy().reshape(shape))]
    tag = _tag("adjoint", n_fft, name)
    signs = _pinned_signs(ref, tag)
    _check_gradient(tag, ref, "mag_l1", d_out.view(out.shape), signs)


# ---------------------------------------------------------------------------------------------------- 4. the head
def _head_operands(c):
    """test_gpu_specunet_backward's operands on the case's rows (B = rows; the head's audio is mono), computed once."""
    key = ("head", c["n_fft"], c["name"])
    if key not in sw._CACHE:
        n_fft, hop, F, B, T = c["n_fft"], c["hop"], c["F"], c["R"], c["T"]
        K = n_fft // 2 + 1
        assert T == (F - 1) * hop + n_fft
        rng = np.random.RandomState(sw._seed(c, 4))
        X = suo.stft(torch.tensor(0.5 * rng.randn(B, T)), n_fft, hop)
        op = {"re": X.real.numpy().astype(np.float32), "im": X.imag.numpy().astype(np.float32),
              "mask": (1.0 / (1.0 + np.exp(-rng.randn(B, F, K - 1)))).astype(np.float32),
              "d_mags": (rng.randn(B, F, K) / (B * F * K)).astype(np.float32), "d_audio": (rng.randn(B, T) / (B * T)).astype(np.float32)}
        op["mag"] = np.sqrt(op["re"].astype(np.float64) ** 2 + op["im"].astype(np.float64) ** 2).astype(np.float32)
        sw._CACHE[key] = op
    return sw._CACHE[key]


def _head_want(c, domain, dtype):
    op = _head_operands(c)
    t = lambda a: torch.tensor(a, dtype=dtype)           # noqa: E731
    dz, scale = bo.head(torch.complex(t(op["re"]), t(op["im"])), t(op["mag"]), t(op["mask"]),
                        op["d_mags"] if domain != "audio" else None, op["d_audio"] if domain != "mags" else None, c["n_fft"], c["hop"])
    return dz.numpy(), scale


@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("name", sw.CASE_NAMES[:3])
@pytest.mark.parametrize("n_fft", SIZES)
def test_head(lib, n_fft, name, domain):
    """wun_op_spec_head_backward in its three domains under test_gpu_specunet_backward's rule.  The dropped bin K - 1 reaches
    nothing and is never written: d_mags, X and M hold NaN there, dz has no slot for it, and the arena around dz stays NaN."""
    c = sw.case(n_fft, name)
    op = _head_operands(c)
    B, F, T, K = c["R"], c["F"], c["T"], n_fft // 2 + 1
    poisoned = {}
    for k in ("re", "im", "mag", "d_mags"):
        a = op[k].copy()
        a[..., K - 1] = np.nan
        poisoned[k] = _dev(a)
    mask = _dev(op["mask"])
    dm = poisoned["d_mags"] if domain != "audio" else None
    da = _dev(op["d_audio"]) if domain != "mags" else None
    ns = _lib.count(lib.wun_op_spec_head_backward_scratch(B, T, n_fft, c["hop"]))
    arena, (dz, scratch) = _arena(B * F * (K - 1), ns)
    _lib.check(lib.wun_op_spec_head_backward(poisoned["re"].data_ptr(), poisoned["im"].data_ptr(), poisoned["mag"].data_ptr(),
                                             mask.data_ptr(), None if dm is None else dm.data_ptr(),
                                             None if da is None else da.data_ptr(), B, T, n_fft, c["hop"], _table(n_fft).data_ptr(),
                                             dz.data_ptr(), scratch.data_ptr(), _stream()))
    _footprint(arena, dz)
    got = dz.cpu().numpy().reshape(B, F, K - 1)
    want64, scale = _head_want(c, domain, torch.float64)
    want32, _ = _head_want(c, domain, torch.float32)
    err, bound = _rule(got, want64, want32, floor_scale=scale)
    record(_tag("spec_head", n_fft, name, domain), "err / bound", err / bound, 1.0)
    assert float(np.abs(want64).max()) > 0 and err <= bound, (err, bound)


# ---------------------------------------------------------------------------------------------------- 5. Griffin-Lim
def _gl_fixture(c):
    key = ("gl", c["n_fft"], c["name"])
    if key not in sw._CACHE:
        n_fft, hop, R, T, lead, F = c["n_fft"], c["hop"], c["R"], c["T"], c["lead"], c["F"]
        mag, y0 = gl.fixture(n_fft + hop + R, R, T, n_fft, hop, lead, F)
        rng = np.random.RandomState(T + n_fft)
        c0 = (rng.rand(R, F, n_fft // 2 + 1) + 1j * rng.uniform(-np.pi, np.pi, (R, F, n_fft // 2 + 1))).astype(np.complex64)
        sw._CACHE[key] = (mag, y0, c0)
    return sw._CACHE[key]


def _griffin_lim(lib, c, mag, y, iterations, y_init=None, c0=None):
    S, B, Cn = c["shape"]
    n = _lib.count(lib.wun_griffin_lim_scratch_floats(S, B, c["T"], Cn, c["n_fft"], c["hop"], c["lead"], c["F"], 0))
    scratch = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    start = (None, None, y_init.data_ptr()) if c0 is None else (c0[0].data_ptr(), c0[1].data_ptr(), None)
    _lib.check(lib.wun_griffin_lim(mag.data_ptr(), *start, S, B, c["T"], Cn, c["n_fft"], c["hop"], c["lead"], c["F"], iterations, 0.0,
                                   _table(c["n_fft"]).data_ptr(), y.data_ptr(), None, scratch.data_ptr(), _stream()))


@pytest.mark.parametrize("start", ["audio", "spectrum"])
@pytest.mark.parametrize("name", sw.CASE_NAMES)
@pytest.mark.parametrize("n_fft", SIZES)
def test_griffin_lim(lib, n_fft, name, start):
    """One and two iterations from audio and from given phases (the GIVEN body), under the one-step rule: the second step is
    judged from the device's own first audio."""
    c = sw.gl_case(sw.case(n_fft, name))
    S, B, Cn = c["shape"]
    mag, y0, c0 = _gl_fixture(c)
    hop, lead, T = c["hop"], c["lead"], c["T"]
    arena, (y1, y2) = _arena(c["R"] * T, c["R"] * T)
    dmag = _dev(mag)
    if start == "audio":
        kw = {"y_init": _dev(sp.unrows(y0, (S, B, T, Cn)))}
    else:
        kw = {"c0": (_dev(c0.real), _dev(c0.imag))}
    _griffin_lim(lib, c, dmag, y1, 1, **kw)
    _griffin_lim(lib, c, dmag, y2, 2, **kw)
    _footprint(arena, y1, y2)
    got = [_audio_rows(y1, c), _audio_rows(y2, c)]
    prev = [y0 if start == "audio" else None, got[0]]
    stand_in = [cpu_step(prev[0], mag, n_fft, hop, lead, T, c0=None if start == "audio" else c0),
                cpu_step(prev[1], mag, n_fft, hop, lead, T)]
    first_c = None if start == "audio" else gl.given(c0.real, c0.imag)
    one_step_check(_tag("griffin_lim", n_fft, name, start), prev, got, mag, n_fft, hop, lead, stand_in_steps=stand_in, first_c=first_c)


# ---------------------------------------------------------------------------------------------------- 6. the vocoder
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("n_fft", SIZES)
def test_vocoder(lib, n_fft, ch):
    """wun_time_stretch at 10/9, 1/2 and 1/1 in one call, hop = n_fft / 4: two analysis transforms per frame."""
    hop = n_fft // 4
    n_in = max(2 * n_fft + 37, 701)
    ratios = [(10, 9), (1, 2), (1, 1)]
    n_outs = [vnp.stretch_frames(n_in, num, den) for num, den in ratios]
    yarena, ys = _arena(*[n * ch for n in n_outs])
    hosts, jobs = [], []
    for i, ((num, den), n_out) in enumerate(zip(ratios, n_outs)):
        h = _signal(n_in, ch, seed=1000 * n_fft + 10 * i + ch)
        hosts.append(h)
        jobs.append((_dev(h).reshape(-1), ys[i], n_in, n_out, num, den))
    table = vocoder.job_table([(x.data_ptr(), y.data_ptr(), a, b, num, den) for x, y, a, b, num, den in jobs])
    scratch = torch.full((vocoder.scratch_floats(table, ch, n_fft, hop),), float("nan"), dtype=torch.float32, device=DEV)
    vocoder.run(table, ch, n_fft, hop, scratch, DEV)
    _footprint(yarena, *ys)
    tag = _tag("voc_analysis", n_fft, "C%d" % ch)
    for (xv, yv, _, n_out, num, den), h in zip(jobs, hosts):
        got = yv.cpu().numpy().reshape(n_out, ch).astype(np.float64)
        if (num, den) == (1, 1):
            err, tol = np.abs(got - h).max() / np.abs(h).max(), TOL_IDENTITY
        else:
            want = vnp.time_stretch(h, num, den, n_fft, hop, n_out)
            err, tol = np.abs(got - want).max() / np.abs(want).max(), TOL_ORACLE
        record(tag, "ratio %d/%d max err / max" % (num, den), err, tol)
        assert err < tol, (num, den, err, tol)


# ---------------------------------------------------------------------------------------------------- 7. the GEMM path
@pytest.mark.parametrize("n_fft", [128, 512, 1024])
def test_agreement_with_the_gemm_path_at_the_sizes_the_family_test_skips(lib, n_fft):
    """test_gpu_fft.test_agreement_with_the_gemm_path itself (both paths within their bounds of the float64 value: they differ
    by at most the sum), on case A's rows, hop and length in the centred framing both paths take."""
    c = sw.case(n_fft, "A")
    family_fft.test_agreement_with_the_gemm_path(lib, n_fft, c["hop"], c["T"], c["shape"])
    counts = _counts(lib)
    assert counts[_lib.FFT_FAMILY_FORWARD, SIZES.index(n_fft)] > 0 and counts[_lib.FFT_FAMILY_INVERSE, SIZES.index(n_fft)] > 0


# ---------------------------------------------------------------------------------------------------- 8. neighbours
@pytest.mark.parametrize("n_fft", SIZES)
def test_a_frame_alone_has_the_bits_it_has_among_its_neighbours(lib, n_fft):
    """Case A's 15 frame rows, each computed alone (one valid slot of a workgroup) against the call that holds them all.  The
    inverse at hop = n_fft, where an output sample belongs to one frame: 15 spectra at once and one at a time."""
    c = sw.case(n_fft, "A")
    ref, spec = sw.signal(c), sw.spectra(c)
    R, F, hop, K = c["R"], c["F"], c["hop"], n_fft // 2 + 1
    x = _dev(ref["x"])                                   # [1, 3, T, 1]
    re, im = torch.empty((R, F, K), dtype=torch.float32, device=DEV), torch.empty((R, F, K), dtype=torch.float32, device=DEV)
    _forward(lib, x, c, re, im)
    r1, i1 = torch.empty(K, dtype=torch.float32, device=DEV), torch.empty(K, dtype=torch.float32, device=DEV)
    for r in range(R):
        for f in range(F):
            one = x[:, r:r + 1, f * hop:f * hop + n_fft].contiguous()
            _forward(lib, one, c, r1, i1, F=1)
            assert np.array_equal(_bits(r1), _bits(re[r, f])) and np.array_equal(_bits(i1), _bits(im[r, f])), (r, f)
    sre, sim = _dev(spec["re"]), _dev(spec["im"])
    y = torch.empty((R, F * n_fft), dtype=torch.float32, device=DEV)
    _inverse(lib, sre, sim, (1, R, 1), c, y, T=F * n_fft, hop=n_fft)
    y1 = torch.empty(n_fft, dtype=torch.float32, device=DEV)
    for r in range(R):
        for f in range(F):
            _inverse(lib, sre[r, f].contiguous(), sim[r, f].contiguous(), (1, 1, 1), c, y1, T=n_fft, F=1, hop=n_fft)
            assert np.array_equal(_bits(y1), _bits(y[r, f * n_fft:(f + 1) * n_fft])), (r, f)
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- 9. coverage (last)
def test_every_fft_kernel_was_exercised(lib):
    """The ledger since the module's reset: each of the 8 x 8 kernels has run; an n_fft without a kernel is refused and adds
    nothing."""
    counts = _counts(lib)
    assert counts.shape == (len(FAMILIES), len(SIZES)) == (8, 8)
    for f, fam in enumerate(FAMILIES):
        print("[fft ledger] %-18s %s" % (fam, " ".join("%5d" % v for v in counts[f])))
    missing = [(fam, n) for f, fam in enumerate(FAMILIES) for j, n in enumerate(SIZES) if counts[f, j] == 0]
    record("fft_sweep::test_every_fft_kernel_was_exercised", "cells never launched (count)", len(missing), 0.0)
    assert not missing, missing
    # behind the table there is no cell: a longer buffer keeps what it held
    buf = (C.c_int64 * (CELLS + 8))(*([-7] * (CELLS + 8)))
    _lib.check(lib.wun_fft_launch_counts(buf, CELLS + 8))
    assert list(buf)[CELLS:] == [-7] * 8 and list(buf)[:CELLS] == list(counts.reshape(-1))
    x = torch.zeros((1, 1, 40000, 1), dtype=torch.float32, device=DEV)
    out = torch.full((1 << 16,), float("nan"), dtype=torch.float32, device=DEV)
    table = _table(64)
    for bad in (32, 16384):
        K, hop = bad // 2 + 1, bad // 4
        rcs = [lib.wun_stft_complex_fft(x.data_ptr(), 1, 1, 40000, 1, bad, hop, 0, 1, table.data_ptr(), out.data_ptr(),
                                        out[K:].data_ptr(), _stream()),
               lib.wun_stft_magnitude_fft(x.data_ptr(), 1, 1, 40000, 1, bad, hop, table.data_ptr(), out.data_ptr(), _stream()),
               lib.wun_istft_fft(out.data_ptr(), out.data_ptr(), 1, 1, bad, 1, bad, hop, 0, 1, table.data_ptr(), out.data_ptr(),
                                 out.data_ptr(), _stream())]
        assert rcs == [-2, -2, -2], (bad, rcs, lib.wun_last_error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and np.array_equal(_counts(lib), counts)
