"""CPU-only checks of the multichannel Wiener post-filter (include/wun.h: wun_wiener_filter*; wave_u_net_amd.postfilter
.WienerFilter, postfilter.from_config): the CPU WienerFilter against the float64 oracle tests/_wiener_np.py,
iterations = 0 against the soft mask, the spec dispatch on `kind`, every argument error of the library before any GPU work
and its scratch sizes, separate_track(postfilter={"kind": "wiener"}) on a numpy stand-in separator, and what the filter is
for: panned sources, from the oracle alone.  The device path is checked in tests/test_gpu_wiener.py.

Tolerance against the oracle: 8 x the distance of _wiener_np.wiener_filter_fp32 from it -- the same definition on float32
numpy transforms with float32 spectra, i.e. what the number format costs on these very inputs, conditioning of the gains
included.  Two float32 implementations differ by their summation orders; 8 x is the allowance DESIGN.md 5.11 gives for that.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _postfilter_np as ora  # noqa: E402
import _wiener_np as wie  # noqa: E402
from _observed import record  # noqa: E402

import wave_u_net_amd as wun  # noqa: E402
from wave_u_net_amd import _lib, postfilter  # noqa: E402
from wave_u_net_amd.evaluate import separate_track  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wun_wiener_filter_scratch_floats", "wun_wiener_filter")
INVALID, UNSUPPORTED = -1, -2
P, Q, R3, R4 = 0x100000, 0x40000000, 0x80000000, 0xC0000000      # non-null "device pointers" far apart: never read
CASES = [(2, 2), (3, 2), (2, 1), (1, 2)]                          # (S, C)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_declared_exported_and_documented(lib):
    hdr = open(os.path.join(ROOT, "include", "wun.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in doc, name
    for line in ("v_s[f,k]  = (1 / C) sum_c |y_s[f,k,c]|^2", "R_s[k]    = (sum_f y_s[f,k] y_s[f,k]^H) / (eps + sum_f v_s[f,k])",
                 "Cxx[f,k]  = sum_s v_s[f,k] R_s[k] + sqrt(eps) I", "y_s[f,k] <- v_s[f,k] R_s[k] Cxx[f,k]^-1 X[f,k]",
                 "2 (iterations + 16) S (C^2 + 1) K"):
        assert line in hdr, line
        if "iterations" not in line:
            assert line in wie.__doc__, line                     # the oracle quotes the header's definition


# ---- the CPU filter against the oracle ---------------------------------------------------------------
@pytest.mark.parametrize("iterations", [1, 2])
@pytest.mark.parametrize("S, C", CASES)
def test_cpu_filter_against_float64(S, C, iterations):
    n, n_fft, hop = 1500, 64, 16
    mix, est, want = wie.fixture(7, S, n, C, n_fft, hop, 2, iterations)
    f = postfilter.WienerFilter(n_fft, hop, iterations=iterations)
    got = f.apply(torch.from_numpy(mix), torch.from_numpy(est))
    assert got.dtype == torch.float32 and tuple(got.shape) == (S, n, C) and not got.is_cuda
    tol = 8 * np.abs(wie.wiener_filter_fp32(mix, est, n_fft, hop, iterations=iterations) - want).max()
    err = np.abs(got.numpy() - want).max()
    record("test_wiener_host.test_cpu_filter_against_float64[S%d-C%d-I%d]" % (S, C, iterations), "max err", err, tol)
    assert err <= tol
    assert np.array_equal(f.apply(mix, est).numpy(), got.numpy())                                 # arrays are taken too
    # the filter does something: the soft mask is further from this oracle than the tolerance
    soft = postfilter.SoftMaskFilter(n_fft, hop).apply(mix, est).numpy()
    if S > 1:
        assert np.abs(soft - want).max() > 100 * tol


def test_oracle_sums_to_the_mix_and_power_one():
    """The y_s sum to (Cxx - sqrt(eps) I) Cxx^-1 X: the oracle's outputs sum to the mix within _wiener_np.regulariser_bound,
    and miss it by more than float64 rounding (the regulariser is there).  power = 1 on the CPU filter, once."""
    n, n_fft, hop = 1500, 64, 16
    mix, est, out, zmax = wie.fixture(3, 3, n, 2, n_fft, hop, 1, 1, details=True)
    gap = np.abs(out.sum(0) - mix).max()
    assert 1e-12 < gap <= wie.regulariser_bound(zmax, n, n_fft, hop) + 1e-12
    got = postfilter.WienerFilter(n_fft, hop, power=1).apply(mix, est).numpy()
    assert np.abs(got - out).max() <= 8 * np.abs(wie.wiener_filter_fp32(mix, est, n_fft, hop, 1) - out).max()


@pytest.mark.parametrize("S, C", CASES)
def test_zero_iterations_is_the_soft_mask(S, C):
    mix, est, _ = wie.fixture(5, S, 1500, C, 64, 16, 2, 0)
    mix, est = torch.from_numpy(mix), torch.from_numpy(est)
    for power in (2, 1):
        got = postfilter.WienerFilter(64, 16, power, iterations=0).apply(mix, est)
        assert torch.equal(got, postfilter.SoftMaskFilter(64, 16, power)._apply_cpu(mix, est))


def test_cpu_filter_exact_cases():
    rng = np.random.RandomState(2)
    mix = torch.from_numpy((0.3 * rng.randn(300, 2)).astype(np.float32))
    f = postfilter.WienerFilter(64, 16, iterations=2)
    out = f.apply(mix, torch.zeros(2, 300, 2))
    assert torch.equal(out[0], out[1]) and bool(torch.isfinite(out).all())
    assert bool((f.apply(torch.zeros(300, 2), torch.from_numpy(rng.randn(2, 300, 2).astype(np.float32))) == 0).all())


# ---- the spec ---------------------------------------------------------------------------------------------
def test_spec_dispatch():
    fc, W, M = postfilter.from_config, postfilter.WienerFilter, postfilter.SoftMaskFilter
    assert fc(None) is None
    m, w = M(64, 16), W(64, 16)
    assert fc(m) is m and fc(w) is w
    got = fc({"n_fft": 1024, "hop": 256})                                        # no kind: today's object
    assert type(got) is M and got.spec() == {"n_fft": 1024, "hop": 256, "power": 2, "eps": 1e-10}
    assert type(fc(True)) is M and type(fc({})) is M
    got = fc({"kind": "softmask", "power": 1})
    assert type(got) is M and got.power == 1
    got = fc({"kind": "wiener"})
    assert type(got) is W and got.spec() == {"kind": "wiener", "n_fft": 2048, "hop": 512, "power": 2, "eps": 1e-10,
                                             "iterations": 1, "em_eps": 1e-10}
    spec = {"kind": "wiener", "n_fft": 256, "hop": 64, "power": 1, "eps": 1e-8, "iterations": 3, "em_eps": 1e-6}
    got = fc(spec)
    assert got.spec() == spec and spec["kind"] == "wiener"                      # the caller's dict is left alone
    assert fc(got.spec()).spec() == spec
    for bad in ({"kind": "norbert"}, {"kind": None}, {"kind": "wiener", "window": "hann"}, {"iterations": 1},
                {"kind": "softmask", "em_eps": 1e-10}, {"kind": "wiener", "iterations": 5}, {"kind": "wiener", "iterations": -1},
                {"kind": "wiener", "iterations": 1.5}, {"kind": "wiener", "iterations": True}, {"kind": "wiener", "em_eps": 0.0},
                {"kind": "wiener", "em_eps": -1e-10}, {"kind": "wiener", "em_eps": float("nan")},
                {"kind": "wiener", "em_eps": float("inf")}, {"kind": "wiener", "em_eps": 1e-60}, {"kind": "wiener", "hop": 24}):
        with pytest.raises(ValueError):
            fc(bad)
    with pytest.raises(ValueError):
        fc("wiener")
    with pytest.raises(NotImplementedError):
        fc({"kind": "wiener", "n_fft": 100})
    assert type(W.from_config({"iterations": 2})) is W and W.from_config(None) is None
    # SoftMaskFilter.from_config itself is what it was: kind is an unknown key to it
    with pytest.raises(ValueError):
        M.from_config({"kind": "wiener"})
    from wave_u_net_amd.__main__ import _parse, _postfilter
    _, name, over, opts = _parse(["predict", "with", "cfg.full", "input_path=/x.wav", 'postfilter={"kind":"wiener","iterations":2}'])
    got = _postfilter(opts, wun.get_config(name, **over))
    assert type(got) is W and got.iterations == 2
    _, name, over, opts = _parse(["evaluate", "with", "cfg.full", 'model_config.postfilter={"kind":"wiener"}', "data_root=/d"])
    cfg = wun.get_config(name, **over)
    assert type(_postfilter(opts, cfg)) is W and type(_postfilter({"postfilter": {"hop": 256}}, cfg)) is M
    with pytest.raises(SystemExit):
        _postfilter({"postfilter": {"kind": "wiener", "iterations": 9}}, cfg)


# ---- the library's argument checks, before any GPU work -------------------------------------------------
def _filter(lib, mix=P, ests=Q, S=2, n=200, Cn=2, n_fft=64, hop=16, power=2, mask_eps=1e-10, iterations=1, eps=1e-10, table=0x10000,
            out=R3, scratch=R4):
    return lib.wun_wiener_filter(mix, ests, S, n, Cn, n_fft, hop, power, mask_eps, iterations, eps, table, out, scratch, None)


def test_argument_errors_and_their_order(lib):
    """No device is touched: the pointers are not device memory and there may be no device at all (so no call here is
    valid: every one must return from its checks).  wun_mask_filter's errors in its order, then iterations, then eps."""
    for name in ("mix", "ests", "table", "out", "scratch"):
        assert _filter(lib, **{name: None}) == INVALID, name
    for kw in ({"S": 0}, {"Cn": 0}, {"Cn": 3}, {"n": 0}, {"hop": 0}, {"hop": 65}, {"hop": 24}, {"hop": 64}, {"power": 0},
               {"power": 3}, {"mask_eps": 0.0}, {"mask_eps": -1e-10}, {"mask_eps": float("nan")}, {"mask_eps": float("inf")},
               {"iterations": -1}, {"iterations": 5}, {"eps": 0.0}, {"eps": -1e-10}, {"eps": float("nan")}, {"eps": float("inf")}):
        assert _filter(lib, **kw) == INVALID, kw
    for bad in (0, 32, 96, 4096):
        assert _filter(lib, n_fft=bad) == UNSUPPORTED, bad
    assert _filter(lib, S=9) == UNSUPPORTED
    assert _filter(lib, mix=None, n_fft=100) == INVALID and _filter(lib, S=0, n_fft=100) == INVALID
    assert _filter(lib, n_fft=100, hop=24, power=3, iterations=9) == UNSUPPORTED
    assert _filter(lib, hop=24, power=3) == INVALID and b"hop" in lib.wun_last_error()
    assert _filter(lib, power=3, mask_eps=0.0) == INVALID and b"power" in lib.wun_last_error()
    assert _filter(lib, mask_eps=0.0, iterations=9) == INVALID and b"mask_eps" in lib.wun_last_error()
    assert _filter(lib, out=P + 4, iterations=9) == INVALID and b"overlap" in lib.wun_last_error()       # out over the mix
    assert _filter(lib, out=Q + 4 * (2 * 200 * 2 - 1)) == INVALID                                        # ... the last estimate float
    assert _filter(lib, iterations=9, eps=0.0) == INVALID and b"iterations" in lib.wun_last_error()
    assert _filter(lib, eps=0.0) == INVALID and b"eps" in lib.wun_last_error()


def test_scratch_sizes(lib):
    def scratch(S=2, n=200, Cn=2, n_fft=64, hop=16, iterations=1):
        return lib.wun_wiener_filter_scratch_floats(S, n, Cn, n_fft, hop, iterations)
    assert scratch(S=0) == INVALID and scratch(hop=24) == INVALID and scratch(n_fft=100) == UNSUPPORTED and scratch(S=9) == UNSUPPORTED
    assert scratch(iterations=-1) == INVALID and scratch(iterations=5) == INVALID and scratch(S=9, iterations=5) == UNSUPPORTED
    for kw in ({}, {"S": 3, "Cn": 1}, {"n": 3 * 60 * 22050, "n_fft": 2048, "hop": 512}, {"S": 8, "n": 100000, "n_fft": 256, "hop": 64}):
        S, Cn, K = kw.get("S", 2), kw.get("Cn", 2), kw.get("n_fft", 64) // 2 + 1
        base = lib.wun_mask_filter_scratch_floats(S, kw.get("n", 200), Cn, kw.get("n_fft", 64), kw.get("hop", 16))
        assert base > 0 and scratch(iterations=0, **kw) == base                  # no iterations: the mask filter's scratch
        for it in (1, 2, 4):                                                    # the header's formula; bounded in n
            assert scratch(iterations=it, **kw) == base + 2 * (it + 16) * S * (Cn * Cn + 1) * K
    f = postfilter.WienerFilter(64, 16, iterations=2)
    assert f.scratch_floats(2, 200, 2) == scratch(iterations=2)
    with pytest.raises(NotImplementedError):
        f.scratch_floats(9, 200, 2)


# ---- separate_track -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mono, chan, n", [(False, 2, 4099), (True, 2, 1033)])
def test_separate_track_with_the_filter(mono, chan, n):
    from test_postfilter_host import FakeSeparator
    cfg = wun.get_config("baseline", mono_downmix=mono, task="multi_instrument")
    sr = cfg["expected_sr"]
    audio = np.random.default_rng(n).uniform(-1, 1, (n, chan)).astype(np.float32)
    plain = separate_track(cfg, FakeSeparator(cfg, 1324, 300), audio, sr, batch_hops=4)
    spec = {"kind": "wiener", "n_fft": 64, "hop": 16}
    got = separate_track(cfg, FakeSeparator(cfg, 1324, 300), audio, sr, batch_hops=4, postfilter=spec)
    mapped = audio.mean(1, keepdims=True) if mono else audio
    est = np.stack([plain[k][:, :mapped.shape[1]] for k in cfg["source_names"]])
    want = postfilter.WienerFilter(64, 16).apply(mapped, est).numpy()
    soft = separate_track(cfg, FakeSeparator(cfg, 1324, 300), audio, sr, batch_hops=4, postfilter={"n_fft": 64, "hop": 16})
    for i, k in enumerate(cfg["source_names"]):
        assert got[k].dtype == np.float32 and got[k].shape == plain[k].shape
        assert np.array_equal(got[k][:, :mapped.shape[1]], want[i])
        assert not np.array_equal(got[k], plain[k]) and not np.array_equal(got[k], soft[k])
    same = separate_track(cfg, FakeSeparator(cfg, 1324, 300), audio, sr, batch_hops=4, postfilter=postfilter.WienerFilter(64, 16))
    assert all(np.array_equal(same[k], got[k]) for k in cfg["source_names"])
    # model_config["postfilter"] carries the spec through the config
    assert wun.get_config("baseline", postfilter=spec)["postfilter"] == spec


# ---- what it is for --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
def test_panned_sources_from_the_oracle(seed):
    """Two overlapping noise sources at pans [1, 0.2] and [0.3, 1], estimates = true + 0.5 x the other + 0.05 noise: one EM
    iteration brings the RMS error against the true sources to at most 0.9 of the soft mask's (float64 oracle alone)."""
    mix, est, src = wie.panned_fixture(seed)
    soft = wie.rms(ora.mask_filter(mix, est, 64, 16)[0] - src)
    one = wie.rms(wie.wiener_filter(mix, est, 64, 16, iterations=1) - src)
    record("test_wiener_host.test_panned_sources_from_the_oracle[%d]" % seed, "rms error / soft mask's", one / soft, 0.9)
    assert one <= 0.9 * soft
