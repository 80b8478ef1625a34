"""CPU-only checks of the rest of the EBU R 128 meter (include/wun.h: wun_true_peak_factor, wun_true_peak,
wun_loudness_short_term_blocks, wun_loudness_r128; wave_u_net_amd.loudness): the float64 oracle
(tests/_r128_np.py) against the figures EBU Tech 3342 asks of a loudness-range meter and against the inter-sample peak of a
quarter-rate sine, the host entries, the argument errors before any GPU work, and the true_peak_limit key of the configuration.
The device path is compared with this oracle in tests/test_gpu_r128.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _loudness_np as ora  # noqa: E402
import _r128_np as r128o  # noqa: E402
from wave_u_net_amd import _lib, loudness  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wun_true_peak_factor", "wun_true_peak_scratch_doubles", "wun_true_peak", "wun_loudness_short_term_blocks",
         "wun_loudness_r128_scratch_doubles", "wun_loudness_r128")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_declared_exported_and_documented(lib):
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in doc, name


# ---- the oracle against the standards' figures ------------------------------------------------------
def _tone(sr, seconds, dbfs):
    t = np.arange(int(seconds * sr)) / float(sr)
    return np.tile((10.0 ** (dbfs / 20.0) * np.sin(2 * np.pi * 1000.0 * t))[:, None], [1, 2]).astype(np.float32)


@pytest.mark.parametrize("levels, want", [((-20, -30), 10.0), ((-40, -20), 20.0), ((-50, -35, -20, -35, -50), 15.0)])
def test_tech_3342_sequences(levels, want):
    """EBU Tech 3342 minimum requirement cases 1 - 3: stereo 1 kHz tones, 20 s per level, LRA within 1 LU of the figure (here at
    8 kHz, where the oracle reads them to four decimals)."""
    sr = 8000
    x = np.concatenate([_tone(sr, 20, d) for d in levels])
    z3, s = r128o.short_term(x, sr)
    lra = r128o.loudness_range(z3, s)[0]
    assert abs(lra - want) <= 1.0, lra
    assert abs(lra - want) <= 1e-3, lra                                   # float32 samples of exact level steps


def _sine45(n):
    return np.sin(2 * np.pi * 0.25 * np.arange(n) + np.pi / 4)[:, None].astype(np.float32)


@pytest.mark.parametrize("sr", [48000, 8000])                            # L = 4 and L = 32
def test_inter_sample_peak_of_the_quarter_rate_sine(sr):
    x = _sine45(2000)
    assert abs(float(np.max(np.abs(x))) - 0.70711) < 1e-5                 # every sample at +-sin(45 deg)
    tp, per = r128o.true_peak(x, sr)
    assert r128o.oversampling(sr) == (4 if sr == 48000 else 32)
    assert 1.00 <= tp <= 1.03 and abs(tp - 1.0134) < 1e-3 and per.shape == (1,) and per[0] == tp
    assert r128o.true_peak(x, 192000)[0] == float(np.max(np.abs(x)))     # L = 1: the sample peak


def test_oracle_range_rule():
    """The ranks in integers, ties by index, the strict gates, and the empty and NaN cases."""
    assert [r128o.ranks(m) for m in (1, 2, 11, 90, 100)] == [(0, 0), (0, 1), (1, 10), (9, 85), (10, 94)]
    z = lambda s: 10.0 ** ((np.asarray(s, np.float64) + 0.691) / 10.0)    # noqa: E731
    s = np.array([-20.0, -30.0, -25.0, -80.0, -20.0])
    lra, keep, gate, sel = r128o.loudness_range(z(s), s)
    assert keep.tolist() == [True, True, True, False, True] and sel == (1, 4) and abs(lra - 10.0) < 1e-12      # ranks (0, 3): -30 and the later -20
    s = np.array([-20.0, -45.0, -80.0])                                   # -45 is under the relative gate: -20 - 3.0 - 20
    lra, keep, gate, sel = r128o.loudness_range(z(s), s)
    assert keep.tolist() == [True, False, False] and lra == 0.0 and sel == (0, 0) and abs(gate + 43.0) < 0.01
    assert r128o.loudness_range(z([-75.0]), np.array([-75.0]))[0] == 0.0
    assert r128o.loudness_range(np.zeros(0), np.zeros(0))[0] == 0.0
    assert np.isnan(r128o.loudness_range(np.array([1.0, np.nan]), np.array([-0.691, np.nan]))[0])


# ---- host entries -----------------------------------------------------------------------------
def test_oversampling_factor(lib):
    want = {8000: 32, 8192: 32, 22050: 8, 44100: 4, 48000: 4, 96000: 2, 192000: 1}
    for sr, L in want.items():
        assert loudness.oversampling(sr) == L == lib.wun_true_peak_factor(sr) == r128o.oversampling(sr), sr
        assert L == 32 or L * sr >= 176400 and (L == 1 or (L // 2) * sr < 176400)
    for sr in (0, 3999, 384001):
        assert lib.wun_true_peak_factor(sr) == -1
        with pytest.raises(ValueError):
            loudness.oversampling(sr)


def test_short_term_block_count_rule(lib):
    for sr in (8000, 11025, 44100, 48000):
        N3, step = (30 * sr + 5) // 10, (sr + 5) // 10
        for n, want in ((N3 - 1, 0), (N3, 1), (N3 + step - 1, 1), (N3 + step, 2)):
            assert lib.wun_loudness_short_term_blocks(n, sr) == want == loudness.short_term_blocks(n, sr), (sr, n)
            assert r128o.short_term_geometry(n, sr) == (N3, step, want)
    assert lib.wun_loudness_short_term_blocks(0, 8000) == -1 and lib.wun_loudness_short_term_blocks(100, 3999) == -1


def test_scratch_queries(lib):
    n, sr = 100000, 8000
    chunks, tiles = -(-n // 256), -(-n // 1024)
    nb3 = (n - 24000) // 800 + 1
    for Cc in (1, 2):
        assert lib.wun_true_peak_scratch_doubles(n, Cc) == Cc * tiles
        base = lib.wun_loudness_scratch_doubles(n, Cc, sr)
        assert lib.wun_loudness_r128_scratch_doubles(n, Cc, sr) == base + 3 * Cc * chunks + 2 * nb3 + 10 + Cc * tiles
        assert loudness.r128_scratch_doubles(n, Cc, sr) == lib.wun_loudness_r128_scratch_doubles(n, Cc, sr)
    for bad in ((0, 1), (n, 0), (n, 3)):
        assert lib.wun_true_peak_scratch_doubles(*bad) == -1, bad
        assert lib.wun_loudness_r128_scratch_doubles(bad[0], bad[1], sr) == -1, bad
    assert lib.wun_loudness_r128_scratch_doubles(n, 2, 3999) == -1
    assert lib.wun_true_peak_scratch_doubles((1 << 40) + 1, 1) == -2


def test_entries_refuse_bad_arguments_before_gpu_work(lib):
    buf = (C.c_double * 64)()
    base = C.addressof(buf)
    p = C.c_void_p(base)                               # a non-null (host) pointer: never dereferenced by a refused call
    far = C.c_void_p(base + 256)
    odd = C.c_void_p(base + 4)

    def peak(x=p, n=16, Cc=2, L=4, tab=p, out=far, scratch=p):
        return lib.wun_true_peak(x, n, Cc, L, tab, out, scratch, None)

    for kw in (dict(x=None), dict(out=None), dict(scratch=None), dict(tab=None), dict(n=0), dict(n=-3), dict(Cc=0), dict(Cc=3),
               dict(L=0), dict(L=3), dict(L=-4), dict(L=64), dict(L=12), dict(scratch=odd), dict(out=odd)):
        assert peak(**kw) == -1, kw
        assert lib.wun_last_error()
    assert peak(n=(1 << 40) + 1) == -2

    def meter(x=p, n=16, Cc=2, sr=8000, tab=p, report=far, st=None, scratch=p):
        return lib.wun_loudness_r128(x, n, Cc, sr, tab, report, st, scratch, None)

    for kw in (dict(x=None), dict(report=None), dict(scratch=None), dict(tab=None), dict(n=0), dict(Cc=0), dict(Cc=3),
               dict(sr=3999), dict(sr=384001), dict(scratch=odd), dict(report=odd), dict(st=odd)):
        assert meter(**kw) == -1, kw
    assert meter(n=(1 << 40) + 1) == -2


def test_module_refuses_cpu_tensors():
    import torch
    x = torch.zeros(100, 1)
    for call in (lambda: loudness.true_peak(x, 8000), lambda: loudness.r128(x, 8000),
                 lambda: loudness.normalize(x, 8000, true_peak_limit=-1.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ---- configuration ---------------------------------------------------------------------------
def test_from_config_true_peak_limit():
    five = {"target": -23.0, "max_gain_db": 30.0, "peak_limit": None, "restore": True, "data": False}
    assert loudness.from_config({}) == five and loudness.from_config(-23) == five           # absent unless given
    assert loudness.from_config({"peak_limit": 0.9}) == dict(five, peak_limit=0.9)
    got = loudness.from_config({"target": -16, "true_peak_limit": -1})
    assert got == dict(five, target=-16.0, true_peak_limit=-1.0) and isinstance(got["true_peak_limit"], float)
    assert loudness.from_config({"true_peak_limit": np.float32(0.5)})["true_peak_limit"] == 0.5
    assert loudness.from_config({"true_peak_limit": -1, "peak_limit": None})["true_peak_limit"] == -1.0
    for bad in (float("nan"), float("inf"), -float("inf"), "-1", True, None, [-1]):
        with pytest.raises(ValueError):
            loudness.from_config({"true_peak_limit": bad})
    with pytest.raises(ValueError, match="exclusive"):
        loudness.from_config({"true_peak_limit": -1.0, "peak_limit": 0.9})
    main = __import__("wave_u_net_amd.__main__", fromlist=["main"])
    assert main._loudness({"loudness": {"target": -23, "true_peak_limit": -1}}, {})["true_peak_limit"] == -1.0
    with pytest.raises(SystemExit):
        main._loudness({"loudness": {"true_peak_limit": -1, "peak_limit": 0.5}}, {})
