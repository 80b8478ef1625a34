"""CPU-only checks of the recursive filter and the loudness meter (include/wun.h: wun_sosfilt, wun_kweight_design,
wun_loudness, wun_loudness_gain, wun_scale_by; wave_u_net_amd.loudness): the K-weighting design against the
standard's table, argument errors before any GPU work, the config handling, and the float64 oracle (tests/_loudness_np.py)
against the readings the definition must give -- the sine levels and the EBU Tech 3341 cases.  The device path is compared
with this oracle in tests/test_gpu_loudness.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _loudness_np as ora  # noqa: E402
from wave_u_net_amd import _lib, config, evaluate, loudness  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wun_sos_chunk", "wun_sos_tile", "wun_sosfilt_scratch_doubles", "wun_sosfilt", "wun_kweight_design",
         "wun_loudness_blocks", "wun_loudness_scratch_doubles", "wun_loudness", "wun_loudness_gain", "wun_scale_by")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_declared_exported_and_documented(lib):
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in doc, name
    assert lib.wun_sos_chunk() == 256 == loudness.chunk() and lib.wun_sos_tile() == 64 == loudness.tile()


# ---- the design ------------------------------------------------------------------------------
def test_kweight_design_reproduces_the_table_at_48k():
    """The table prints 14 decimals: an entry is known to half a unit of the 14th, 5e-15, and the design's own float64
    round-off (a dozen operations on values below 3) is below 3e-15: bound 1e-14."""
    got = loudness.kweight_sos(48000)
    assert got.shape == (2, 6) and got.dtype == np.float64
    assert np.max(np.abs(got - ora.TABLE_48K)) <= 1e-14
    assert np.max(np.abs(ora.kweight_sos(48000) - ora.TABLE_48K)) <= 1e-14
    assert got[1, 0] == 1.0 and got[1, 1] == -2.0 and got[1, 2] == 1.0 and got[0, 3] == 1.0 and got[1, 3] == 1.0


@pytest.mark.parametrize("sr", [4000, 8000, 22050, 44100, 96000, 384000])
def test_kweight_design_matches_the_oracle(sr):
    # the same formulas in C and numpy: a few units of round-off on coefficients below 4
    assert np.max(np.abs(loudness.kweight_sos(sr) - ora.kweight_sos(sr))) <= 4e-15


@pytest.mark.parametrize("sr", [0, -1, 3999, 384001])
def test_refused_sample_rates(lib, sr):
    sos = (C.c_double * 12)()
    assert lib.wun_kweight_design(sr, sos) == -1
    assert lib.wun_loudness_blocks(1000, sr) == -1
    assert lib.wun_loudness_scratch_doubles(1000, 1, sr) == -1
    with pytest.raises(ValueError):
        loudness.kweight_sos(sr)


def test_block_count_rule(lib):
    for sr in (8000, 11025, 44100, 48000):
        Nb, step = (4 * sr + 5) // 10, (sr + 5) // 10                    # 11025 Hz: a step of 1102.5 frames rounds up
        for n in (1, Nb - 1, Nb, Nb + step - 1, Nb + step, 10 * sr + 7):
            want = (n - Nb) // step + 1 if n >= Nb else 0
            assert lib.wun_loudness_blocks(n, sr) == want == ora.block_geometry(n, sr)[2], (sr, n)
    assert lib.wun_loudness_blocks(0, 8000) == -1


# ---- ABI argument errors: all before any GPU work (there is no GPU here) ----------------------------
def test_scratch_queries(lib):
    n = 100000
    chunks = -(-n // 256)
    groups = -(-chunks // 64)
    for Cc in (1, 2):
        for nsec in (1, 2, 8):
            assert lib.wun_sosfilt_scratch_doubles(n, Cc, nsec) == 2 * nsec * Cc * (chunks + groups)
        nb = (n - 3200) // 800 + 1
        assert lib.wun_loudness_scratch_doubles(n, Cc, 8000) == 4 * Cc * (chunks + groups) + 4 * Cc * chunks + nb
    for bad in ((0, 1, 2), (n, 0, 2), (n, 3, 2), (n, 1, 0), (n, 1, 9)):
        assert lib.wun_sosfilt_scratch_doubles(*bad) == -1, bad
    for bad in ((0, 1, 8000), (n, 0, 8000), (n, 3, 8000)):
        assert lib.wun_loudness_scratch_doubles(*bad) == -1, bad
    assert lib.wun_sosfilt_scratch_doubles((1 << 40) + 1, 1, 2) == -2


def test_entries_refuse_bad_arguments_before_gpu_work(lib):
    buf = (C.c_double * 64)()
    base = C.addressof(buf)
    p = C.c_void_p(base)                               # a non-null (host) pointer: never dereferenced by a refused call
    far = C.c_void_p(base + 256)
    sos_ok = (C.c_double * 12)(*ora.kweight_sos(48000).ravel())

    def filt(x=p, n=16, Cc=2, sos=sos_ok, nsec=2, y=far, scratch=p):
        return lib.wun_sosfilt(x, n, Cc, sos, nsec, y, scratch, None)

    a0 = (C.c_double * 12)(*ora.kweight_sos(48000).ravel())
    a0[9] = 2.0
    nonfinite = (C.c_double * 12)(*ora.kweight_sos(48000).ravel())
    nonfinite[1] = float("nan")
    for kw in (dict(x=None), dict(y=None), dict(scratch=None), dict(sos=None), dict(nsec=0), dict(nsec=9), dict(n=0), dict(n=-5),
               dict(Cc=0), dict(Cc=3), dict(sos=a0), dict(sos=nonfinite),
               dict(y=p),                                               # in place
               dict(y=C.c_void_p(base + 64)),                           # y starts inside x (16 frames x 2 x 4 bytes = 128)
               dict(x=far, y=C.c_void_p(base + 256 - 4)),               # y ends inside x
               dict(scratch=C.c_void_p(base + 4))):                     # misaligned scratch
        assert filt(**kw) == -1, kw
        assert lib.wun_last_error()
    assert filt(n=(1 << 40) + 1) == -2

    def meter(x=p, n=16, Cc=2, sr=8000, m=far, blocks=None, scratch=p):
        return lib.wun_loudness(x, n, Cc, sr, m, blocks, scratch, None)

    for kw in (dict(x=None), dict(m=None), dict(scratch=None), dict(n=0), dict(Cc=0), dict(Cc=3), dict(sr=3999), dict(sr=384001),
               dict(scratch=C.c_void_p(base + 4)), dict(m=C.c_void_p(base + 260)), dict(blocks=C.c_void_p(base + 4))):
        assert meter(**kw) == -1, kw

    def gain(m=p, target=-23.0, max_db=30.0, peak=0.0, g=far):
        return lib.wun_loudness_gain(m, target, max_db, peak, g, None)

    for kw in (dict(m=None), dict(g=None), dict(target=float("nan")), dict(target=float("inf")), dict(max_db=-1.0),
               dict(max_db=float("nan")), dict(peak=-0.5), dict(peak=float("inf"))):
        assert gain(**kw) == -1, kw

    for args in ((None, 4, p), (p, 4, None), (p, 0, p), (p, -1, p)):
        assert lib.wun_scale_by(args[0], args[1], args[2], None) == -1, args


def test_module_refuses_cpu_tensors():
    import torch
    x = torch.zeros(100, 1)
    for call in (lambda: loudness.sosfilt(x, ora.kweight_sos(8000)), lambda: loudness.k_weight(x, 8000),
                 lambda: loudness.integrated(x, 8000), lambda: loudness.normalize(x, 8000),
                 lambda: loudness.gain(torch.zeros(4, dtype=torch.float64)), lambda: loudness.scale_(x, torch.ones(1))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ---- configuration ---------------------------------------------------------------------------
def test_from_config():
    assert loudness.from_config(None) is None
    want = {"target": -23.0, "max_gain_db": 30.0, "peak_limit": None, "restore": True, "data": False}
    assert loudness.from_config({}) == want
    assert loudness.from_config(-16) == dict(want, target=-16.0)
    assert loudness.from_config(-14.5) == dict(want, target=-14.5)
    got = loudness.from_config({"target": -20, "peak_limit": 0.9, "restore": False, "data": True, "max_gain_db": 0})
    assert got == {"target": -20.0, "max_gain_db": 0.0, "peak_limit": 0.9, "restore": False, "data": True}
    for bad in ({"targt": -23}, {"target": float("nan")}, {"target": float("inf")}, {"target": "loud"}, {"max_gain_db": -1},
                {"peak_limit": 0}, {"peak_limit": -1.0}, {"restore": 1}, {"data": "yes"}, True, "quiet", [-23]):
        with pytest.raises(ValueError):
            loudness.from_config(bad)


def test_config_default_and_keyword():
    import inspect
    assert config.EXTENSION_DEFAULTS["loudness"] is None and "loudness" not in config.BASE_MODEL_CONFIG
    for fn in (evaluate.separate_track, evaluate.produce_source_estimates, evaluate.evaluate_track,
               evaluate.produce_dataset_estimates):
        assert inspect.signature(fn).parameters["loudness"].default is None, fn.__name__
    assert evaluate.loudness_option({"loudness": -20}) == -20 and evaluate.loudness_option({"loudness": -20}, -30) == -30
    assert evaluate.loudness_option({}) is None


def test_cli_checks_the_spec_at_once():
    main = __import__("wave_u_net_amd.__main__", fromlist=["main"])
    assert main._loudness({"loudness": -20}, {})["target"] == -20.0
    assert main._loudness({}, {"loudness": {"target": -18, "restore": False}})["restore"] is False
    assert main._loudness({}, {}) is None
    with pytest.raises(SystemExit):
        main._loudness({"loudness": {"level": 3}}, {})


def test_cpu_separators_are_refused():
    class Stub(object):
        device = None

        def get_padding(self, shape):
            return np.array([1, 64, 1]), np.array([1, 64, 1])
    cfg = config.get_config("baseline", num_frames=64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluate.separate_track(cfg, Stub(), np.zeros((100, 1), np.float32), cfg["expected_sr"], loudness=-23)


# ---- the oracle against what the definition must read ----------------------------------------------
def test_serial_recurrence_against_lfilter_and_the_chunked_schedule():
    """Serial direct form I against scipy.signal.lfilter (the transposed direct form II): the two orders of the same
    sums.  Measured 2e-13 of max |y| for the K-weighting on noise; the high-pass has a near-double pole at radius 0.995, which
    amplifies round-off by about (1 - r)^-2 = 4e4 ulps: bound 1e-11."""
    rng = np.random.RandomState(0)
    x = rng.randn(3000, 2)
    for sr in (48000, 8000):
        sos = ora.kweight_sos(sr)
        a, b = ora.sosfilt_serial(sos, x), ora.sosfilt_fast(sos, x)
        assert np.max(np.abs(a - b)) <= 1e-11 * np.max(np.abs(a))
        c = ora.sosfilt_chunked(sos, x, 256)
        err = np.max(np.abs(c - a)) / np.max(np.abs(a))
        assert err <= 1e-8                                # measured 4e-11 - 3e-10 at 48 kHz (the companion-form carry of the high-pass)
        d = ora.sosfilt_chunked(sos, x, 256, drop_carry=True)
        assert np.max(np.abs(d - a)) / np.max(np.abs(a)) > 1e-3


@pytest.mark.parametrize("kind", ora.INPUT_KINDS)
@pytest.mark.parametrize("case", sorted(ora.filter_cases()))
def test_a_lost_carry_cannot_pass_the_device_tolerance(case, kind):
    """The tolerance tests/test_gpu_loudness.py holds the device to, on the emulation of the device's schedule WITHOUT its
    carries (every chunk from zero state): missed by at least 1000 times on every case, so a kernel that loses a carry fails."""
    chunk = loudness.chunk()
    sos = ora.filter_cases()[case]
    x = ora.filter_input(kind, 3 * chunk + 37, 2, chunk)
    serial = ora.sosfilt_serial(sos, x)
    tol = ora.filter_tolerance(serial, ora.sosfilt_chunked(sos, x, chunk))
    lost = np.max(np.abs(ora.sosfilt_chunked(sos, x, chunk, drop_carry=True) - serial))
    assert lost >= 1000.0 * tol, (lost, tol)
    # and the serial loop is the recurrence scipy runs (another order of the same sums)
    assert np.max(np.abs(serial - ora.sosfilt_fast(sos, x))) <= 1e-11 * np.max(np.abs(serial))


def _sine(sr, seconds, freq, amp_db, C):
    t = np.arange(int(seconds * sr)) / float(sr)
    return np.tile((10.0 ** (amp_db / 20.0) * np.sin(2 * np.pi * freq * t))[:, None], [1, C]).astype(np.float32)


@pytest.mark.parametrize("sr, C, want", [(48000, 1, -3.0103), (48000, 2, 0.0000), (44100, 1, -3.0075), (44100, 2, 0.0028)])
def test_full_scale_sine_readings(sr, C, want):
    L = ora.loudness(_sine(sr, 20, 997.0, 0.0, C), sr)[0]
    assert abs(L - want) <= 1e-3, L                      # the table's four printed decimals, and float32 samples


def test_ebu_tech_3341_cases():
    """EBU Tech 3341 minimum requirement cases, stereo 1 kHz sines, +-0.1 LU."""
    for sr, fine in ((8000, -23.001), (48000, -23.014)):
        x = np.concatenate([_sine(sr, 10, 1000.0, -36.0, 2), _sine(sr, 60, 1000.0, -23.0, 2), _sine(sr, 10, 1000.0, -36.0, 2)])
        L = ora.loudness(x, sr)[0]
        assert abs(L + 23.0) <= 0.1 and abs(L - fine) <= 5e-3, (sr, L)      # the relative gate drops the quiet ends
    a = ora.loudness(_sine(48000, 3, 1000.0, -23.0, 2), 48000)[0]
    assert abs(a + 23.0) <= 0.1 and abs(a + 22.99) <= 5e-3, a
    b = ora.loudness(_sine(48000, 3, 1000.0, -33.0, 2), 48000)[0]
    assert abs((a - b) - 10.0) <= 1e-4, (a, b)                               # float32 samples: 10 dB to a few 1e-6
    L, kept, nb, peak, l = ora.loudness(np.zeros((48000, 2), np.float32), 48000)
    assert L == -np.inf and kept == 0 and nb == 7 and peak == 0.0 and np.all(l == -np.inf)
    L, kept, nb, _, l = ora.loudness(np.ones((100, 2), np.float32), 48000)
    assert L == -np.inf and kept == 0 and nb == 0 and l.shape == (0,)


def test_oracle_gain_rule():
    g, r = ora.gain(-33.0, 0.1)
    assert g == np.float32(10.0 ** 0.5) and r == np.float32(1.0 / np.float64(g))
    assert ora.gain(-80.0, 0.001)[0] == np.float32(10.0 ** 1.5)             # the cap at 30 dB
    assert ora.gain(-33.0, 0.5, peak_limit=0.9)[0] == np.float32(0.9 / 0.5)
    assert ora.gain(-np.inf, 0.0)[0] == 1.0 and ora.gain(np.nan, 0.3)[0] == 1.0
