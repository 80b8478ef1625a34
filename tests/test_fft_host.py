"""CPU-only checks of the FFT path (include/wun.h: wun_fft_*, wun_stft_complex_fft, wun_istft_fft, wun_mask_filter_fft,
wun_wiener_filter_fft; wave_u_net_amd.spectral / postfilter with transform="fft"): the host-designed table,
every argument error of the new entries before any GPU work and their scratch sizes, the CPU transform="fft" path of both
filter classes against the float64 oracle tests/_fft_np.py, and the Python surface.  The device path is checked in
tests/test_gpu_fft.py.

Tolerance of the CPU filters against the oracle: test_wiener_host.py's rule, 8 x the distance of a float32 stand-in
(_fft_np.wiener_filter_fp32: scipy's float32 FFTs, float32 spectra) from the same oracle on the same inputs."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fft_np as fo  # noqa: E402
import _postfilter_np as ora  # noqa: E402
from _observed import record  # noqa: E402
from test_postfilter_host import FakeSeparator  # noqa: E402

import wave_u_net_amd as wun  # noqa: E402
from wave_u_net_amd import _lib, postfilter, spectral  # noqa: E402
from wave_u_net_amd.evaluate import separate_track  # noqa: E402

INVALID, UNSUPPORTED = -1, -2
P, Q, R3, R4 = 0x100000, 0x40000000, 0x80000000, 0xC0000000      # non-null "device pointers" far apart: never read
BAD_N_FFT = (0, 32, 96, 100, 16384)
SIZES = (64, 128, 256, 512, 1024, 2048, 4096, 8192)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---- the table ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", SIZES)
def test_table_is_the_float64_design_rounded_once(lib, n_fft):
    """Half an ulp of float32 at the entry's size, plus 2^-52: the float64 recomputation (numpy's cos / sin of a rounded
    angle) is itself only good to about 1e-16, which matters where the exact value is 0."""
    assert lib.wun_fft_table_floats(n_fft) == 3 * n_fft
    tab = spectral.fft_design(n_fft)
    assert tab.shape == (3, n_fft) and tab.dtype == np.float32
    ang = 2.0 * np.pi * np.arange(n_fft) / n_fft
    want = np.stack([np.cos(ang), -np.sin(ang), 0.5 - 0.5 * np.cos(ang)])
    half_ulp = 0.5 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(tab.astype(np.float64) - want)
    record("test_table_is_the_float64_design_rounded_once[%d]" % n_fft, "max err / (half ulp + 2^-52)",
           (err / (half_ulp + 2.0 ** -52)).max(), 1.0)
    assert (err <= half_ulp + 2.0 ** -52).all()
    q = n_fft // 4                                                # exact at the multiples of pi / 2
    assert [tab[0, 0], tab[0, q], tab[0, 2 * q], tab[0, 3 * q]] == [1.0, 0.0, -1.0, 0.0]
    assert [tab[1, 0], tab[1, q], tab[1, 2 * q], tab[1, 3 * q]] == [0.0, -1.0, 0.0, 1.0]
    assert tab[2, 0] == 0.0 and tab[2, 2 * q] == 1.0
    assert np.array_equal(tab[2, 1:], tab[2, :0:-1])              # the periodic Hann window is symmetric about n_fft / 2


def test_table_errors(lib):
    import ctypes as C
    buf = np.zeros(3 * 64, np.float32)
    ptr = buf.ctypes.data_as(C.POINTER(C.c_float))
    for bad in BAD_N_FFT:
        assert lib.wun_fft_table_floats(bad) == UNSUPPORTED and lib.wun_fft_design(bad, ptr, 1 << 20) == UNSUPPORTED
        assert lib.wun_fft_centered_frames(1000, bad, 16) == UNSUPPORTED
    assert lib.wun_fft_design(64, None, 192) == INVALID and lib.wun_fft_design(64, ptr, 191) == INVALID
    assert lib.wun_fft_design(64, ptr, 192) == 0
    assert lib.wun_fft_centered_frames(1000, 8192, 2048) == ora.centered_frames(1000, 8192, 2048)
    assert lib.wun_fft_centered_frames(5, 64, 0) == INVALID and lib.wun_fft_centered_frames(0, 64, 16) == INVALID
    assert lib.wun_fft_centered_frames(0, 100, 0) == UNSUPPORTED
    # the framing without padding: wun_stft_frames' rule and check order (n_fft, then the hop, then T < n_fft)
    for bad in BAD_N_FFT:
        assert lib.wun_fft_frames(100000, bad, 16) == UNSUPPORTED
    assert lib.wun_fft_frames(9000, 4096, 1024) == 1 + (9000 - 4096) // 1024 == 5 and lib.wun_fft_frames(8192, 8192, 8192) == 1
    assert lib.wun_fft_frames(1000, 64, 48) == lib.wun_stft_frames(1000, 64, 48) == 20
    assert lib.wun_fft_frames(4095, 4096, 1024) == INVALID and lib.wun_fft_frames(9000, 4096, 0) == INVALID
    assert lib.wun_fft_frames(9000, 4096, 4097) == INVALID and lib.wun_fft_frames(10, 100, 0) == UNSUPPORTED
    assert lib.wun_fft_frames(10, 64, 0) == INVALID and b"hop" in lib.wun_last_error()
    assert spectral.frames(9000, 4096, 1024, transform="fft") == 5
    with pytest.raises(NotImplementedError):
        spectral.frames(9000, 4096, 1024)
    with pytest.raises(ValueError):
        spectral.frames(4000, 4096, 1024, transform="fft")
    with pytest.raises(ValueError):
        spectral.frames(9000, 4096, 1024, transform="dft")
    with pytest.raises(NotImplementedError):
        spectral.fft_design(16384)


# ---- refusals of the device entries (no device is touched: every call must return from its checks) ----
def _complex(lib, x=P, S=2, B=3, T=200, Cn=2, n_fft=64, hop=16, lead=48, F=16, table=Q, re=R3, im=R4):
    return lib.wun_stft_complex_fft(x, S, B, T, Cn, n_fft, hop, lead, F, table, re, im, None)


def _istft(lib, re=R3, im=R4, S=2, B=3, T=200, Cn=2, n_fft=64, hop=16, lead=48, F=16, table=Q, y=P, scratch=0x10000):
    return lib.wun_istft_fft(re, im, S, B, T, Cn, n_fft, hop, lead, F, table, y, scratch, None)


def _mask(lib, mix=P, ests=Q, S=2, n=200, Cn=2, n_fft=64, hop=16, power=2, eps=1e-10, table=0x10000, out=R3, scratch=R4):
    return lib.wun_mask_filter_fft(mix, ests, S, n, Cn, n_fft, hop, power, eps, table, out, scratch, None)


def _wiener(lib, mix=P, ests=Q, S=2, n=200, Cn=2, n_fft=64, hop=16, power=2, eps=1e-10, iterations=1, em_eps=1e-10, table=0x10000,
            out=R3, scratch=R4):
    return lib.wun_wiener_filter_fft(mix, ests, S, n, Cn, n_fft, hop, power, eps, iterations, em_eps, table, out, scratch, None)


def test_transform_argument_errors_and_their_order(lib):
    for call, ptrs in ((_complex, ("x", "table", "re", "im")), (_istft, ("re", "im", "table", "y", "scratch"))):
        for name in ptrs:
            assert call(lib, **{name: None}) == INVALID, name
        for kw in ({"S": 0}, {"B": 0}, {"Cn": 0}, {"Cn": 3}, {"T": 0}, {"hop": 0}, {"hop": 65}, {"lead": -1}, {"lead": 64},
                   {"F": 0}, {"F": -3}):
            assert call(lib, **kw) == INVALID, kw
        for bad in BAD_N_FFT:
            assert call(lib, n_fft=bad) == UNSUPPORTED, bad
        assert call(lib, **{ptrs[0]: None, "n_fft": 100}) == INVALID
        assert call(lib, S=0, n_fft=100) == INVALID
        assert call(lib, n_fft=100, hop=0, lead=-1) == UNSUPPORTED and b"8192" in lib.wun_last_error()
        assert call(lib, hop=0, lead=-1) == INVALID and b"hop" in lib.wun_last_error()
        assert call(lib, lead=64, F=0) == INVALID and b"lead" in lib.wun_last_error()
        assert call(lib, F=1 << 29) == UNSUPPORTED
        assert call(lib, n_fft=8192, hop=8193, lead=0) == INVALID and call(lib, n_fft=8192, hop=2048, lead=8192) == INVALID
    assert _complex(lib, re=P + 16) == INVALID and _complex(lib, im=P) == INVALID and _complex(lib, re=R3, im=R3 + 4) == INVALID
    assert _istft(lib, y=R3 + 64) == INVALID and _istft(lib, y=R4) == INVALID

    def scratch(S=2, B=3, T=200, Cn=2, n_fft=64, hop=16, lead=48, F=16):
        return lib.wun_istft_fft_scratch_floats(S, B, T, Cn, n_fft, hop, lead, F)
    assert scratch(S=0) == INVALID and scratch(hop=0) == INVALID and scratch(lead=64) == INVALID and scratch(F=0) == INVALID
    for bad in BAD_N_FFT:
        assert scratch(n_fft=bad) == UNSUPPORTED
    assert scratch() == lib.wun_istft_scratch_floats(2, 3, 200, 2, 64, 16, 48, 16) == 12 * 16 * 64 + 2 * 64 + 2
    assert scratch(T=100000, F=6253) == 12 * (256 + 3) * 64 + 2 * 64 + 2
    assert scratch(T=100000, n_fft=8192, hop=2048, lead=6144, F=52) == 12 * 52 * 8192 + 2 * 8192 + 2


def test_filter_argument_errors_and_their_order(lib):
    for call in (_mask, _wiener):
        for name in ("mix", "ests", "table", "out", "scratch"):
            assert call(lib, **{name: None}) == INVALID, name
        for kw in ({"S": 0}, {"Cn": 0}, {"Cn": 3}, {"n": 0}, {"hop": 0}, {"hop": 65}, {"hop": 24}, {"hop": 64}, {"power": 0},
                   {"power": 3}, {"eps": 0.0}, {"eps": -1e-10}, {"eps": float("nan")}, {"eps": float("inf")}):
            assert call(lib, **kw) == INVALID, kw
        for bad in BAD_N_FFT:
            assert call(lib, n_fft=bad) == UNSUPPORTED, bad
        assert call(lib, S=9) == UNSUPPORTED
        assert call(lib, mix=None, n_fft=100) == INVALID and call(lib, S=0, n_fft=100) == INVALID
        assert call(lib, n_fft=100, hop=24, power=3) == UNSUPPORTED
        assert call(lib, hop=24, power=3) == INVALID and b"hop" in lib.wun_last_error()
        assert call(lib, power=3, eps=0.0) == INVALID and b"power" in lib.wun_last_error()
        assert call(lib, out=P + 4) == INVALID and b"overlap" in lib.wun_last_error()
        assert call(lib, n_fft=8192, hop=8192) == INVALID and call(lib, n_fft=8192, hop=3000) == INVALID
    for kw in ({"iterations": -1}, {"iterations": 5}, {"em_eps": 0.0}, {"em_eps": float("nan")}, {"em_eps": float("inf")}):
        assert _wiener(lib, **kw) == INVALID, kw
    assert _wiener(lib, iterations=5, em_eps=0.0) == INVALID and b"iterations" in lib.wun_last_error()

    def ms(S=2, n=200, Cn=2, n_fft=64, hop=16):
        return lib.wun_mask_filter_fft_scratch_floats(S, n, Cn, n_fft, hop)

    def ws(S=2, n=200, Cn=2, n_fft=64, hop=16, iterations=1):
        return lib.wun_wiener_filter_fft_scratch_floats(S, n, Cn, n_fft, hop, iterations)
    assert ms(S=0) == INVALID and ms(hop=24) == INVALID and ms(n_fft=100) == UNSUPPORTED and ms(S=9) == UNSUPPORTED
    assert ws(S=0) == INVALID and ws(hop=24) == INVALID and ws(n_fft=16384) == UNSUPPORTED and ws(iterations=5) == INVALID
    # the twins' formulas
    assert ms() == lib.wun_mask_filter_scratch_floats(2, 200, 2, 64, 16)
    assert ws(iterations=2) == lib.wun_wiener_filter_scratch_floats(2, 200, 2, 64, 16, 2) and ws(iterations=0) == ms()
    n, nb = 3 * 60 * 44100, 256 + 3
    for n_fft, hop in ((4096, 1024), (8192, 2048)):
        K = n_fft // 2 + 1
        assert ms(n=n, n_fft=n_fft, hop=hop) == 2 * 3 * 2 * nb * K + 2 * 2 * nb * n_fft + 2 * n_fft + 2
        assert ws(n=n, n_fft=n_fft, hop=hop) == ms(n=n, n_fft=n_fft, hop=hop) + 2 * (1 + 16) * 2 * 5 * K


def test_the_gemm_entries_still_refuse_4096(lib):
    assert lib.wun_mask_filter(P, Q, 2, 200, 2, 4096, 1024, 2, 1e-10, 0x10000, R3, R4, None) == UNSUPPORTED
    assert b"64..2048" in lib.wun_last_error()
    assert lib.wun_stft_centered_frames(1000, 4096, 1024) == UNSUPPORTED
    for F in (postfilter.SoftMaskFilter, postfilter.WienerFilter):
        with pytest.raises(NotImplementedError):
            F(n_fft=4096, hop=1024)
        with pytest.raises(NotImplementedError):
            F(n_fft=16384, hop=1024, transform="fft")
        with pytest.raises(ValueError):
            F(transform="dct")


# ---- the CPU "fft" path against the oracle -------------------------------------------------------------
@pytest.mark.parametrize("iterations", [0, 1, 2])
@pytest.mark.parametrize("S, C, n_fft, hop, n", [(2, 2, 64, 16, 1500), (3, 1, 64, 16, 1500), (2, 2, 4096, 1024, 9000),
                                                 (3, 1, 4096, 1024, 9000)])
def test_cpu_filters_against_float64(S, C, n_fft, hop, n, iterations):
    mix, est, want = fo.fixture(7, S, n, C, n_fft, hop, 2, iterations)
    tol = 8 * np.abs(fo.wiener_filter_fp32(mix, est, n_fft, hop, iterations=iterations) - want).max()
    f = (postfilter.WienerFilter(n_fft, hop, iterations=iterations, transform="fft") if iterations
         else postfilter.SoftMaskFilter(n_fft, hop, transform="fft"))
    got = f.apply(torch.from_numpy(mix), torch.from_numpy(est))
    assert got.dtype == torch.float32 and tuple(got.shape) == (S, n, C)
    err = np.abs(got.numpy() - want).max()
    record("test_fft_host.test_cpu_filters_against_float64[%d-%d-S%d-C%d-I%d]" % (n_fft, hop, S, C, iterations), "max err", err, tol)
    assert err <= tol
    if n_fft == 64:                                              # and the same definition as the "gemm" CPU path
        g = (postfilter.WienerFilter(n_fft, hop, iterations=iterations) if iterations else postfilter.SoftMaskFilter(n_fft, hop))
        other = np.abs(g.apply(torch.from_numpy(mix), torch.from_numpy(est)).numpy() - want).max()
        assert np.abs(got.numpy() - g.apply(torch.from_numpy(mix), torch.from_numpy(est)).numpy()).max() <= err + other


def test_cpu_exact_cases():
    rng = np.random.RandomState(2)
    mix = torch.from_numpy((0.3 * rng.randn(300, 2)).astype(np.float32))
    est = torch.from_numpy(rng.randn(2, 300, 2).astype(np.float32))
    for f in (postfilter.SoftMaskFilter(128, 32, transform="fft"), postfilter.WienerFilter(128, 32, iterations=2, transform="fft")):
        out = f.apply(mix, torch.zeros(2, 300, 2))
        assert torch.equal(out[0], out[1]) and bool(torch.isfinite(out).all())
        assert bool((f.apply(torch.zeros(300, 2), est) == 0).all())
    a = postfilter.WienerFilter(128, 32, iterations=0, transform="fft").apply(mix, est)
    assert torch.equal(a, postfilter.SoftMaskFilter(128, 32, transform="fft").apply(mix, est))


# ---- the surface -----------------------------------------------------------------------------------------
def test_spec_and_from_config_round_trip():
    S, W = postfilter.SoftMaskFilter, postfilter.WienerFilter
    assert S().spec() == {"n_fft": 2048, "hop": 512, "power": 2, "eps": 1e-10}             # the default spec is unchanged
    assert "transform" not in W().spec() and "transform" not in S(transform="gemm").spec()
    f = S(4096, 1024, transform="fft")
    assert f.spec() == {"n_fft": 4096, "hop": 1024, "power": 2, "eps": 1e-10, "transform": "fft"}
    g = postfilter.from_config(f.spec())
    assert type(g) is S and g.spec() == f.spec() and g.transform == "fft"
    w = W(8192, 2048, iterations=2, transform="fft")
    assert w.spec() == {"n_fft": 8192, "hop": 2048, "power": 2, "eps": 1e-10, "kind": "wiener", "iterations": 2, "em_eps": 1e-10,
                        "transform": "fft"}
    w2 = postfilter.from_config(w.spec())
    assert type(w2) is W and w2.spec() == w.spec()
    assert postfilter.from_config({"transform": "gemm"}).spec() == S().spec()
    with pytest.raises(NotImplementedError):
        postfilter.from_config({"n_fft": 4096, "hop": 1024})
    with pytest.raises(ValueError):
        postfilter.from_config({"n_fft": 4096, "hop": 1024, "transform": "FFT"})
    from wave_u_net_amd.__main__ import _parse, _postfilter
    _, name, over, opts = _parse(["predict", "with", "cfg.full", "input_path=/x.wav",
                                  'postfilter={"n_fft":4096,"hop":1024,"transform":"fft"}'])
    assert _postfilter(opts, wun.get_config(name, **over)).spec()["transform"] == "fft"
    cfg = wun.get_config("full", postfilter={"kind": "wiener", "n_fft": 4096, "hop": 1024, "transform": "fft"})
    assert type(postfilter.from_config(cfg["postfilter"])) is W


def test_spectral_refuses_without_a_gpu_or_with_a_bad_transform():
    with pytest.raises(ValueError):
        spectral.stft(torch.zeros(1, 1, 100, 1), 64, 16, centered=True, transform="fft")   # no CPU path, as for "gemm"
    with pytest.raises(ValueError):
        spectral.centered_frames(100, 64, 16, transform="dft")
    assert spectral.centered_frames(100, 8192, 2048, transform="fft") == ora.centered_frames(100, 8192, 2048)
    with pytest.raises(NotImplementedError):
        spectral.centered_frames(100, 8192, 2048)


def test_separate_track_with_the_filter():
    cfg = wun.get_config("baseline", mono_downmix=False, task="multi_instrument")
    sr, n = cfg["expected_sr"], 9001
    audio = np.random.default_rng(n).uniform(-1, 1, (n, 2)).astype(np.float32)
    spec = {"n_fft": 4096, "hop": 1024, "transform": "fft"}
    plain = separate_track(cfg, FakeSeparator(cfg, 1324, 300), audio, sr, batch_hops=4)
    got = separate_track(cfg, FakeSeparator(cfg, 1324, 300), audio, sr, batch_hops=4, postfilter=spec)
    est = np.stack([plain[k] for k in cfg["source_names"]])
    want = postfilter.from_config(spec).apply(audio, est).numpy()
    total = np.zeros_like(audio, dtype=np.float64)
    for i, k in enumerate(cfg["source_names"]):
        assert got[k].dtype == np.float32 and np.array_equal(got[k], want[i]) and not np.array_equal(got[k], plain[k])
        total += got[k]
    assert np.abs(total - audio).max() <= 4096 * 2.0 ** -24 * np.abs(audio).max()          # test_postfilter_host._cpu_tol's rule
    with pytest.raises(NotImplementedError):
        separate_track(cfg, FakeSeparator(cfg, 1324, 300), audio, sr, batch_hops=4, postfilter={"n_fft": 4096, "hop": 1024})
