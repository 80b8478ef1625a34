"""CPU-only checks of the spectral loss (include/wun.h: wun_stft_*, wun_spectral_*; wave_u_net_amd.spectral):
the host-designed table against float64 numpy, the frame rule, every argument error before any GPU work, the bindings and the
documentation, and the float64 oracle's own gradient (tests/_spectral_np.py) against central differences.  The device path is
checked against that oracle in tests/test_gpu_spectral.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _spectral_np as ora  # noqa: E402
from _observed import record  # noqa: E402
from wave_u_net_amd import _lib, spectral  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wun_stft_frames", "wun_stft_table_floats", "wun_stft_design", "wun_stft_magnitude", "wun_spectral_scratch_floats",
         "wun_spectral_loss")
INVALID, UNSUPPORTED = -1, -2
P = 0x1000                  # a non-null "device pointer": every call below must fail before any GPU work reads it


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_declared_exported_and_documented(lib):
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in doc, name


@pytest.mark.parametrize("n_fft", [64, 1024, 2048])
def test_design_against_float64(n_fft):
    """Every entry within 2^-24: one rounding of a value of modulus <= 1."""
    tab = spectral.design(n_fft)
    K = n_fft // 2 + 1
    assert tab.shape == (2, n_fft, K) and tab.dtype == np.float32
    assert tab.size == _lib.load().wun_stft_table_floats(n_fft)
    cb, sb = ora.basis(n_fft)
    err = max(np.abs(tab[0].astype(np.float64) - cb).max(), np.abs(tab[1].astype(np.float64) - sb).max())
    record("test_design_against_float64[%d]" % n_fft, "max |table - float64|", err, 2.0 ** -24)
    assert err <= 2.0 ** -24
    assert np.all(tab[1][:, 0] == 0) and np.all(tab[:, 0, :] == 0)          # sin(0) and w[0] are exact zeros


def test_oracle_transform_is_the_direct_dft():
    """torch.stft(center=False, periodic Hann) in float64 is the definition's direct DFT."""
    rng = np.random.RandomState(5)
    x = rng.randn(3, 1024 + 2 * 768 + 3)
    re, im = ora.stft(x, 1024, 768)
    cb, sb = ora.basis(1024)
    fr = ora.frame_view(x, 1024, 768)
    err = max(np.abs(fr @ cb - re).max(), np.abs(fr @ sb - im).max())
    record("test_oracle_transform_is_the_direct_dft", "max |stft - dft|", err, 1e-10)
    assert re.shape == (3, 3, 513) and err < 1e-10


@pytest.mark.parametrize("n_fft, hop", [(64, 48), (64, 1), (64, 64), (1024, 768), (2048, 37)])
def test_frames_rule(lib, n_fft, hop):
    for T in (n_fft, n_fft + hop - 1, n_fft + hop, n_fft + 7 * hop + 3):
        want = 1 + (T - n_fft) // hop
        assert lib.wun_stft_frames(T, n_fft, hop) == want == spectral.frames(T, n_fft, hop) == ora.num_frames(T, n_fft, hop)
    assert lib.wun_stft_frames(n_fft, n_fft, hop) == 1
    assert lib.wun_stft_frames(n_fft + hop - 1, n_fft, hop) == 1
    assert lib.wun_stft_frames(n_fft + hop, n_fft, hop) == 2


def test_host_entry_errors(lib):
    assert lib.wun_stft_frames(63, 64, 16) == INVALID                      # fewer samples than a frame
    assert lib.wun_stft_frames(100, 64, 0) == INVALID
    assert lib.wun_stft_frames(100, 64, 65) == INVALID
    for bad in (0, 32, 96, 1000, 4096, -64):
        assert lib.wun_stft_frames(10000, bad, 16) == UNSUPPORTED, bad
        assert lib.wun_stft_table_floats(bad) == UNSUPPORTED, bad
    buf = (C.c_float * 16)()
    assert lib.wun_stft_design(64, None, 1 << 20) == INVALID
    assert lib.wun_stft_design(64, buf, 16) == INVALID                      # cap below the table
    assert lib.wun_stft_design(48, buf, 16) == UNSUPPORTED
    with pytest.raises(ValueError):
        spectral.frames(10, 64, 16)
    with pytest.raises(NotImplementedError):
        spectral.design(100)


def _loss(lib, outputs=P, targets=P, S=2, B=3, T=200, Cn=2, mse_weight=0.0, res=((64, 48),), weights=(1.0,), tables=None,
          d_outputs=P, losses=P, scratch=P, nres=None, null_tables=False):
    n = max(len(res), 1)
    n_fft = (C.c_int32 * n)(*[r[0] for r in res])
    hop = (C.c_int32 * n)(*[r[1] for r in res])
    w = (C.c_float * n)(*weights)
    tabs = (C.c_void_p * n)(*(tables if tables is not None else [P] * len(res)))
    return lib.wun_spectral_loss(outputs, targets, S, B, T, Cn, mse_weight, len(res) if nres is None else nres, n_fft, hop, w,
                                 None if null_tables else tabs, d_outputs, losses, scratch, None)


def test_loss_argument_errors(lib):
    """Every refusal comes before any GPU work: the pointers are not device memory and there may be no device at all."""
    for kw in ({"outputs": None}, {"targets": None}, {"losses": None}, {"scratch": None}, {"null_tables": True},
               {"tables": [None]}):
        assert _loss(lib, **kw) == INVALID, kw
    for kw in ({"S": 0}, {"B": 0}, {"Cn": 0}, {"Cn": 3}, {"S": -1}):
        assert _loss(lib, **kw) == INVALID, kw
    assert _loss(lib, T=63) == INVALID                                      # Tout < n_fft
    assert _loss(lib, res=((64, 48), (1024, 768)), weights=(1.0, 1.0), T=1023) == INVALID
    assert _loss(lib, res=((64, 0),)) == INVALID
    assert _loss(lib, res=((64, 65),)) == INVALID
    assert _loss(lib, nres=-1) == INVALID
    assert _loss(lib, res=((64, 48),) * 9, weights=(1.0,) * 9) == INVALID   # nres outside 0..8
    for bad in (-1.0, float("nan"), float("inf")):
        assert _loss(lib, weights=(bad,)) == INVALID, bad
        assert _loss(lib, mse_weight=bad) == INVALID, bad
        assert _loss(lib, res=(), weights=(1.0,), mse_weight=bad) == INVALID, bad
    for bad in (32, 96, 4096, 0):
        assert _loss(lib, res=((bad, 16),), T=10000) == UNSUPPORTED, bad
    assert b"n_fft" in lib.wun_last_error()


def test_magnitude_and_scratch_argument_errors(lib):
    def mag(x=P, S=2, B=3, T=200, Cn=2, n_fft=64, hop=48, table=P, mags=P):
        return lib.wun_stft_magnitude(x, S, B, T, Cn, n_fft, hop, table, mags, None)
    for kw in ({"x": None}, {"table": None}, {"mags": None}, {"S": 0}, {"B": 0}, {"Cn": 3}, {"T": 63}, {"hop": 0}, {"hop": 65}):
        assert mag(**kw) == INVALID, kw
    assert mag(n_fft=100) == UNSUPPORTED and mag(n_fft=32) == UNSUPPORTED and mag(n_fft=4096, T=10000) == UNSUPPORTED

    def scratch(S=2, B=3, T=200, Cn=2, res=((64, 48),), nres=None):
        n = max(len(res), 1)
        return lib.wun_spectral_scratch_floats(S, B, T, Cn, len(res) if nres is None else nres,
                                               (C.c_int32 * n)(*[r[0] for r in res]), (C.c_int32 * n)(*[r[1] for r in res]))
    assert scratch(S=0) == INVALID and scratch(T=63) == INVALID and scratch(nres=9) == INVALID
    assert scratch(res=((100, 10),)) == UNSUPPORTED
    # the documented size: R F (4 K + n_fft) floats per resolution, one float64 per 1024 elements, 2 floats of room
    R, F, K = 12, 3, 33
    parts = -(-(R * 200) // 1024) + -(-(R * F * K) // 1024)
    assert scratch() == R * F * (4 * K + 64) + 2 * parts + 2
    assert scratch(res=()) == 2 * -(-(R * 200) // 1024) + 2


def test_python_front_end_refuses_bad_settings():
    with pytest.raises(ValueError):
        spectral.SpectralLoss([(64, 48)], weights=[1.0, 2.0])
    with pytest.raises(ValueError):
        spectral.SpectralLoss([(64, 48)], weights=[-1.0])
    with pytest.raises(ValueError):
        spectral.SpectralLoss([(64, 48)], mse_weight=float("nan"))
    with pytest.raises(ValueError):
        spectral.SpectralLoss([(64, 48)] * 9)
    with pytest.raises(ValueError):
        spectral.SpectralLoss.from_config({"resolutions": [[64, 48]], "hop": 3})
    loss = spectral.SpectralLoss.from_config({"resolutions": [[64, 48], [128, 32]], "weights": [1.0, 0.5], "mse_weight": 1.0})
    assert loss.resolutions == [(64, 48), (128, 32)] and loss.weights == [1.0, 0.5] and loss.mse_weight == 1.0
    assert spectral.SpectralLoss.from_config(None) is None and spectral.SpectralLoss.from_config(loss) is loss
    assert spectral.SpectralLoss().resolutions == [(1024, 768)]             # the reference's setting
    from wave_u_net_amd import config
    assert config.EXTENSION_DEFAULTS["spectral_loss"] is None and "spectral_loss" not in config.BASE_MODEL_CONFIG


def test_oracle_gradient_against_central_differences():
    """The float64 oracle's analytic gradient on R = 1, n_fft = 64, hop = 48, T = 165 (three frames and a tail)."""
    rng = np.random.RandomState(11)
    out, tgt = rng.randn(1, 1, 165, 1), rng.randn(1, 1, 165, 1)
    res, w, mw = [(64, 48)], [0.7], 0.3
    losses, g = ora.loss_and_grad(out, tgt, res, w, mw)
    assert abs(losses[0] - (mw * losses[1] + w[0] * losses[2])) < 1e-15
    h, worst = 1e-6, 0.0
    for t in range(165):
        p, m = out.copy(), out.copy()
        p[0, 0, t, 0] += h
        m[0, 0, t, 0] -= h
        num = (ora.loss_and_grad(p, tgt, res, w, mw)[0][0] - ora.loss_and_grad(m, tgt, res, w, mw)[0][0]) / (2 * h)
        worst = max(worst, abs(num - g[0, 0, t, 0]))
    scale = np.abs(g).max()
    record("test_oracle_gradient_against_central_differences", "max |numeric - analytic| / max |g|", worst / scale, 1e-6)
    assert worst / scale < 1e-6           # h^2 truncation and 1e-16 / h cancellation, far from any sign flip at this seed
    # samples behind the last frame (t >= 64 + 2 * 48) carry the MSE term alone
    tail = mw * 2.0 * (out - tgt)[0, 0, 160:, 0] / 165
    assert np.array_equal(g[0, 0, 160:, 0], tail)
