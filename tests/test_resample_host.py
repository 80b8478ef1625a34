"""CPU-only checks of the resampler (include/wun.h: wun_resample_ratio / _frames / _table_floats / _design / wun_resample) and
of what is built on it without a GPU: resample() on numpy, datasets.load_audio(resample=True), evaluate.separate_track on CPU
tensors against predict_track.  The oracle is scipy.signal (resample_poly, firwin): the filter is scipy's default design."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy.io import wavfile
from scipy.signal import firwin, resample_poly

import wave_u_net_amd as wun
from wave_u_net_amd import _lib, datasets
from wave_u_net_amd import resample as rs
from wave_u_net_amd.evaluate import predict_track, separate_track

WUN_ERR_INVALID, WUN_ERR_UNSUPPORTED = -1, -2
RATES = [((44100, 22050), (1, 2)), ((22050, 44100), (2, 1)), ((48000, 22050), (147, 320)), ((44100, 8192), (2048, 11025))]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("rates,want", RATES)
def test_ratio_and_frames(lib, rates, want):
    up, down = C.c_int32(), C.c_int32()
    assert lib.wun_resample_ratio(rates[0], rates[1], C.byref(up), C.byref(down)) == 0
    assert (up.value, down.value) == want == rs.ratio(*rates)
    for n in (0, 1, 2, 149822, 7938000):
        got = lib.wun_resample_frames(n, up.value, down.value)
        assert got == -(-n * up.value // down.value)
        assert got == len(resample_poly(np.zeros(n), up.value, down.value)) == rs.frames(n, *want)


@pytest.mark.parametrize("rates,want", RATES)
def test_design_matches_scipy_firwin(lib, rates, want):
    """Both are float64 designs rounded once to fp32: at most 1 fp32 ulp of the largest tap per element."""
    up, down = want
    mx = max(up, down)
    half = 10 * mx
    h = firwin(2 * half + 1, 1.0 / mx, window=("kaiser", 5.0)) * up
    n = lib.wun_resample_table_floats(up, down)
    K = -(-(2 * half + 1) // up)
    assert n == up * K
    table = np.full(n, np.nan, np.float32)
    assert lib.wun_resample_design(up, down, table.ctypes.data_as(C.POINTER(C.c_float)), n) == 0
    table = table.reshape(up, K)
    idx = np.arange(up)[:, None] + np.arange(K)[None, :] * up                # phase-major: taps[p][k] = h[p + k * up]
    inside = idx < h.size
    assert np.all(table[~inside] == 0.0)
    got = np.zeros(h.size, np.float64)
    got[idx[inside]] = table[inside]                                           # un-permuted
    assert np.bincount(idx[inside], minlength=h.size).min() == 1              # every tap exactly once
    ulp = float(np.spacing(np.float32(np.abs(h).max())))
    err = np.abs(got - h.astype(np.float32).astype(np.float64)).max()
    print("up %d down %d: max |table - firwin| = %.3g (1 ulp of the largest tap = %.3g)" % (up, down, err, ulp))
    assert err <= ulp
    assert np.array_equal(rs.design(up, down), table)


_FAKE = C.c_void_p(0x1000)          # non-null, never dereferenced: every call below fails its argument check first


def _call(lib, x=_FAKE, n_in=1000, c_in=2, y=_FAKE, y_offset=0, n_out=500, c_out=2, table=_FAKE, up=1, down=2):
    return lib.wun_resample(x, n_in, c_in, y, y_offset, n_out, c_out, table, up, down, None)


def test_argument_errors_without_a_device(lib):
    up, down = C.c_int32(), C.c_int32()
    assert lib.wun_resample_ratio(0, 22050, C.byref(up), C.byref(down)) == WUN_ERR_INVALID
    assert lib.wun_resample_ratio(44100, -1, C.byref(up), C.byref(down)) == WUN_ERR_INVALID
    assert lib.wun_resample_ratio(44100, 22050, None, C.byref(down)) == WUN_ERR_INVALID
    assert lib.wun_resample_ratio(44100, 22050, C.byref(up), None) == WUN_ERR_INVALID
    # the ceiling on max(up, down): 16384
    assert lib.wun_resample_ratio(44100, 16411, C.byref(up), C.byref(down)) == WUN_ERR_UNSUPPORTED      # 16411 is prime
    assert lib.wun_resample_frames(10, 16385, 1) == WUN_ERR_UNSUPPORTED
    assert lib.wun_resample_table_floats(1, 16385) == WUN_ERR_UNSUPPORTED
    assert lib.wun_resample_table_floats(16384, 1) == 16384 * 21
    assert lib.wun_resample_frames(-1, 1, 2) == WUN_ERR_INVALID
    assert lib.wun_resample_frames(10, 0, 2) == WUN_ERR_INVALID
    assert lib.wun_resample_frames(10, 2, 4) == WUN_ERR_INVALID                # not reduced
    buf = (C.c_float * 41)()
    assert lib.wun_resample_design(1, 2, None, 41) == WUN_ERR_INVALID
    assert lib.wun_resample_design(1, 2, buf, 40) == WUN_ERR_INVALID           # short cap
    assert "cap" in lib.wun_last_error().decode()
    assert lib.wun_resample_design(1, 2, buf, 41) == 0

    assert _call(lib, x=None) == WUN_ERR_INVALID
    assert _call(lib, y=None) == WUN_ERR_INVALID
    assert _call(lib, table=None) == WUN_ERR_INVALID
    for c_in, c_out in ((2, 3), (3, 3), (3, 2), (1, 3), (0, 1), (1, 0), (9, 1), (2, 4)):
        assert _call(lib, c_in=c_in, c_out=c_out) == WUN_ERR_INVALID, (c_in, c_out)
        assert "channels" in lib.wun_last_error().decode()
    assert _call(lib, n_out=501) == WUN_ERR_INVALID                            # beyond ceil(1000 / 2)
    assert "n_out" in lib.wun_last_error().decode()
    assert _call(lib, n_in=999, n_out=501) == WUN_ERR_INVALID
    assert _call(lib, n_in=-1, n_out=0) == WUN_ERR_INVALID
    assert _call(lib, y_offset=-1) == WUN_ERR_INVALID
    assert _call(lib, up=0) == WUN_ERR_INVALID
    assert _call(lib, up=2, down=4, n_out=500) == WUN_ERR_INVALID
    assert _call(lib, up=1, down=16385, n_out=1) == WUN_ERR_UNSUPPORTED
    assert _call(lib, up=1, down=4096, n_out=1) == WUN_ERR_UNSUPPORTED         # window of 256 outputs beyond 64 KB
    # nothing to do is not an error (and launches nothing)
    assert _call(lib, n_out=0) == 0
    assert _call(lib, n_in=0, n_out=0, up=1, down=1, table=None) == 0


@pytest.mark.parametrize("rates,want", RATES)
def test_resample_numpy_is_scipy(rates, want):
    x = np.random.default_rng(5).uniform(-1, 1, (4099, 2)).astype(np.float32)
    got = rs.resample(x, *rates)
    ref = resample_poly(x.astype(np.float64), want[0], want[1], axis=0).astype(np.float32)
    assert got.dtype == np.float32 and got.shape == ref.shape == (rs.frames(4099, *want), 2)
    assert np.array_equal(got, ref)
    assert np.array_equal(rs.resample(x[:, 0], *rates), ref[:, 0])            # [T] in, [T] out
    assert np.array_equal(rs.resample(x, 22050, 22050), x)


def test_load_audio_resample_is_opt_in(tmp_path):
    rng = np.random.default_rng(2)
    n = 4411
    pcm = (rng.uniform(-0.5, 0.5, (n, 2)) * 32767).astype(np.int16)
    path = os.path.join(str(tmp_path), "song.wav")
    wavfile.write(path, 44100, pcm)
    with pytest.raises(NotImplementedError):
        datasets.load_audio(path, expected_sr=22050)
    with pytest.raises(NotImplementedError):
        datasets.load_audio(path, expected_sr=22050, resample=False)
    got = datasets.load_audio(path, expected_sr=22050, resample=True)
    assert got.shape == (-(-n // 2), 2) and got.dtype == np.float32
    x = pcm.astype(np.float32) / 32768.0
    assert np.array_equal(got, resample_poly(x.astype(np.float64), 1, 2, axis=0).astype(np.float32))
    mono = datasets.load_audio(path, mono=True, expected_sr=22050, resample=True)
    assert mono.shape == (-(-n // 2), 1)
    assert np.array_equal(datasets.load_audio(path, expected_sr=44100, resample=True), x)     # same rate: untouched
    audio, sr = datasets.read_audio(path)
    assert sr == 44100 and np.array_equal(audio, x)
    # the partition loaders pass the option through
    cfg = wun.get_config("baseline")
    d = os.path.join(str(tmp_path), "valid", "t0")
    os.makedirs(d)
    for name in cfg["source_names"]:
        wavfile.write(os.path.join(d, name + ".wav"), 44100, pcm)
    with pytest.raises(NotImplementedError):
        datasets.load_partition(str(tmp_path), "valid", cfg)
    tr = datasets.load_partition(str(tmp_path), "valid", cfg, resample=True)
    assert tr[0]["mix"].shape == (-(-n // 2), 1)


def test_cli_resample_option_is_parsed():
    from wave_u_net_amd.__main__ import _parse
    _, _, _, opts = _parse(["test", "with", "cfg.baseline", "data_root=/x", "resample=1"])
    assert bool(opts.get("resample", False)) is True


class FakeSeparator(object):
    """Deterministic stand-in with the separator surface: output = centre crop * per-source gain."""

    def __init__(self, cfg, t_in, t_out):
        self.cfg, self.t_in, self.t_out = cfg, t_in, t_out
        self.calls = 0
        self.batches = []

    def get_padding(self, shape):
        c = 1 if self.cfg["mono_downmix"] else 2
        return np.array([shape[0], self.t_in, c]), np.array([shape[0], self.t_out, c])

    def get_output(self, batch, training):
        assert training is False
        self.calls += 1
        self.batches.append(np.array(batch, copy=True))
        pad = (self.t_in - self.t_out) // 2
        core = np.asarray(batch)[:, pad:pad + self.t_out, :]
        return {n: core * (i + 1) + 0.01 * i for i, n in enumerate(self.cfg["source_names"])}


@pytest.mark.parametrize("n_frames", [50, 1000, 1024, 1033, 4099])
@pytest.mark.parametrize("mono,chan", [(True, 2), (False, 1), (False, 2)])
def test_separate_track_equals_predict_track_at_expected_sr(n_frames, mono, chan):
    cfg = wun.get_config("baseline", mono_downmix=mono, task="multi_instrument")
    t_in, t_out = 1324, 300
    audio = np.random.default_rng(n_frames).uniform(-1, 1, (n_frames, chan)).astype(np.float32)
    ref_sep, sep = FakeSeparator(cfg, t_in, t_out), FakeSeparator(cfg, t_in, t_out)
    want = predict_track(cfg, ref_sep, audio, cfg["expected_sr"], batch_hops=4)
    if mono and chan > 1:
        want = {k: np.tile(v, [1, chan]) for k, v in want.items()}           # as produce_source_estimates did
    got = separate_track(cfg, sep, audio, cfg["expected_sr"], batch_hops=4)
    assert list(got.keys()) == cfg["source_names"]
    assert sep.calls == ref_sep.calls
    for a, b in zip(sep.batches, ref_sep.batches):                            # same chunking, same batches
        assert np.array_equal(a, b)
    for n in cfg["source_names"]:
        assert got[n].dtype == np.float32 and got[n].shape == want[n].shape == (n_frames, 2)
        assert np.array_equal(got[n], want[n])


@pytest.mark.parametrize("mono,chan", [(True, 2), (True, 1), (False, 1), (False, 2)])
def test_separate_track_resamples_on_the_host_path(mono, chan):
    """44 100 Hz file, 22 050 Hz model, CPU stand-in: the composition resample -> predict_track -> resample back, trimmed."""
    cfg = wun.get_config("baseline", mono_downmix=mono)
    n = 4099
    audio = np.random.default_rng(1).uniform(-1, 1, (n, chan)).astype(np.float32)
    got = separate_track(cfg, FakeSeparator(cfg, 1324, 300), audio, 44100, batch_hops=4)
    x = np.mean(audio, axis=1, keepdims=True) if mono else (np.tile(audio, [1, 2]) if chan == 1 else audio)
    mid = predict_track(cfg, FakeSeparator(cfg, 1324, 300), rs.resample(x, 44100, 22050), 22050, batch_hops=4)
    for name in cfg["source_names"]:
        back = rs.resample(mid[name], 22050, 44100)[:n]
        if mono and chan > 1:
            back = np.tile(back, [1, chan])
        # a stereo model on a mono file keeps its two channels, as the reference does
        assert got[name].shape == back.shape == (n, 2 if not mono else chan)
        assert np.array_equal(got[name], back)
