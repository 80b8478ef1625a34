"""CPU-only checks of the mel-scale terms of the spectral loss (include/wun.h: wun_mel_design, wun_op_mel_project*,
wun_spectral_loss_mel; wave_u_net_amd.spectral.SpectralLoss(mel=...)): the library's table against the float64
oracle tests/_mel_np.py, the table's two structural properties, the refusal of an empty band and of every bad argument before any
GPU work, the scratch formula, the bindings, the Python front end, and the oracle itself against torch.autograd.  The device path
is checked against that oracle in tests/test_gpu_mel.py.

The table is compared after its one rounding to float32 with a tolerance of one float32 unit in the last place plus 1e-10: the
two builders call different libms (log10 and a power of ten), whose float64 results may differ in the last bits -- about 1e-11 Hz
on a corner frequency, over a band edge at least 1 Hz long -- and such a difference can move the rounding by one step."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mel_np as mel  # noqa: E402
import _mrstft_np as mr  # noqa: E402
from wave_u_net_amd import _lib, spectral, training  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wun_mel_table_floats", "wun_mel_design", "wun_op_mel_project", "wun_op_mel_project_transpose", "wun_mel_abi_size",
         "wun_spectral_mel_scratch_floats", "wun_spectral_loss_mel", "wun_spectral_mel_fft_scratch_floats",
         "wun_spectral_loss_mel_fft")
INVALID, UNSUPPORTED = -1, -2
P = 0x1000                  # a non-null "device pointer": every call below must fail before any GPU work reads it
NON_EMPTY = [(64, 8192, 8), (128, 8192, 16), (256, 8192, 20), (512, 22050, 40), (1024, 22050, 40), (2048, 22050, 160),
             (4096, 44100, 128)]
# the seven configurations, some with fmin > 0, fmax < sr / 2 and the area norm
VARIANTS = [{}, {"fmin": 100.0}, {"fmax": 3500.0}, {"norm": "area"}, {"fmin": 60.0, "fmax": 10000.0, "norm": "area"}, {"norm": "area"},
            {"fmin": 30.0, "fmax": 20000.0}]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_declared_exported_and_documented(lib):
    hdr = open(os.path.join(ROOT, "include", "wun.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in NAMES:
        assert name in doc and name in design, name
    assert "wun_mel_terms" in hdr and C.sizeof(_lib.WunMelTerms) == 12 == lib.wun_mel_abi_size()
    assert spectral.MEL_TERMS == mel.MEL_TERMS == tuple(n for n, _ in _lib.WunMelTerms._fields_[:2])
    assert spectral.TERMS == mr.TERMS and C.sizeof(_lib.WunSpectralTerms) == 24          # the old struct is untouched


# ---------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("i", range(len(NON_EMPTY)))
def test_table_against_the_float64_filterbank(lib, i):
    (n_fft, sr, n_mels), kw = NON_EMPTY[i], VARIANTS[i]
    K = n_fft // 2 + 1
    assert lib.wun_mel_table_floats(n_fft, n_mels) == 3 * K + 2 * n_mels
    words = spectral.mel_design(n_fft, sr, n_mels, **kw)
    assert words.dtype == np.int32 and words.shape == (3 * K + 2 * n_mels,)
    b0, w0, w1, lo, hi = spectral.mel_table_parts(words, n_fft, n_mels)
    got = spectral.mel_filterbank(n_fft, sr, n_mels, **kw)
    want = mel.filterbank32(n_fft, sr, n_mels, **kw)
    assert got.dtype == np.float32 and got.shape == want.shape == (n_mels, K)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert (err <= 2.0 ** -23 * np.abs(want) + 1e-10).all(), err.max()
    assert ((got > 0) == (want > 0)).all()
    # every bin: at most two bands, adjacent, the lower one first; every band: one contiguous, non-empty run [lo, hi)
    pos = got > 0
    assert pos.sum(0).max() <= 2
    for k in np.nonzero(pos.sum(0) == 2)[0]:
        b = np.nonzero(pos[:, k])[0]
        assert b[1] == b[0] + 1 and b0[k] == b[0]
    for k in np.nonzero(pos.sum(0) == 1)[0]:
        assert b0[k] == np.nonzero(pos[:, k])[0][0] and w1[k] == 0
    for k in np.nonzero(pos.sum(0) == 0)[0]:
        assert w0[k] == 0 and w1[k] == 0
    assert (w0 >= 0).all() and (w1 >= 0).all()
    for b in range(n_mels):
        ks = np.nonzero(pos[b])[0]
        assert ks.size > 0 and lo[b] == ks[0] and hi[b] == ks[-1] + 1 and ks.size == hi[b] - lo[b], b
    # the float64 filterbank itself has both properties and the triangles' peaks
    W = mel.filterbank(n_fft, sr, n_mels, **kw)
    assert ((W > 0).sum(0) <= 2).all()
    if "norm" not in kw:
        assert W.max() <= 1.0 and got.max() <= 1.0


def test_an_empty_band_is_refused(lib):
    want = mel.filterbank32(64, 8192, 24)
    empty = np.nonzero((want > 0).sum(1) == 0)[0]
    assert empty.size >= 1                                          # the oracle agrees: some band weights no bin
    buf = (C.c_float * 400)()
    assert lib.wun_mel_design(64, 8192.0, 24, 0.0, 0.0, 0, buf, 400) == INVALID
    msg = lib.wun_last_error().decode()
    assert "band %d" % empty[0] in msg, msg                         # named
    with pytest.raises(ValueError):
        spectral.mel_filterbank(64, 8192, 24)
    with pytest.raises(ValueError):
        spectral.SpectralLoss([(64, 48)], mel={"n_mels": 24, "sample_rate": 8192})
    # the preset: non-empty at 22 050 Hz, refused where a band is empty (512 points, 40 bands up to 48 kHz)
    ms = spectral.SpectralLoss.multi_scale_mel(22050)
    assert ms.resolutions == [(512, 128), (1024, 256), (2048, 512)] and ms.mel["n_mels"] == [40, 80, 160]
    assert ms.mel["terms"] == {"mel_l1": 1.0, "log_mel_l1": 1.0} and ms.num_losses == 2 + 7 * 3 and ms.transform == "gemm"
    assert ms.terms == {t: 0.0 for t in spectral.TERMS}            # no linear-frequency term
    for (n_fft, _), n in zip(ms.resolutions, ms.mel["n_mels"]):
        assert ((mel.filterbank32(n_fft, 22050, n) > 0).sum(1) > 0).all()
    assert spectral.SpectralLoss.multi_scale_mel(22050, transform="fft").transform == "fft"
    with pytest.raises(ValueError):
        spectral.SpectralLoss.multi_scale_mel(96000)


def _design(lib, n_fft=64, sr=8192.0, n_mels=8, fmin=0.0, fmax=0.0, norm=0, null=False, cap=None):
    n = 3 * 4097 + 2 * 512
    buf = (C.c_float * n)()
    return lib.wun_mel_design(n_fft, sr, n_mels, fmin, fmax, norm, None if null else buf, n if cap is None else cap)


def test_design_argument_errors(lib):
    assert _design(lib) == 0
    for bad in (32, 96, 16384, 0):
        assert _design(lib, n_fft=bad) == UNSUPPORTED and lib.wun_mel_table_floats(bad, 8) == UNSUPPORTED
    for bad in (0, -1, 513):
        assert _design(lib, n_mels=bad) == INVALID and lib.wun_mel_table_floats(64, bad) == INVALID
    for bad in (0.0, -8192.0, float("nan"), float("inf")):
        assert _design(lib, sr=bad) == INVALID, bad
    for kw in ({"fmin": -1.0}, {"fmin": 5000.0}, {"fmin": 100.0, "fmax": 100.0}, {"fmin": 200.0, "fmax": 100.0}, {"fmax": 4097.0},
               {"fmin": float("nan")}, {"fmax": float("nan")}, {"fmax": float("inf")}, {"fmax": -1.0}):
        assert _design(lib, **kw) == INVALID, kw
    for bad in (-1, 2):
        assert _design(lib, norm=bad) == INVALID
    assert _design(lib, null=True) == INVALID
    assert _design(lib, cap=3 * 33 + 2 * 8 - 1) == INVALID and _design(lib, cap=3 * 33 + 2 * 8) == 0
    assert _design(lib, n_fft=96, n_mels=0) == UNSUPPORTED          # the n_fft first
    assert _design(lib, fmax=4096.0) == 0                           # fmax = sr / 2 itself is legal
    with pytest.raises(ValueError):
        spectral.mel_filterbank(64, 8192, 8, norm="slaney")


def test_single_operator_argument_errors(lib):
    for fn in (lib.wun_op_mel_project, lib.wun_op_mel_project_transpose):
        assert fn(None, 4, 33, 8, P, P, None) == INVALID and fn(P, 4, 33, 8, None, P, None) == INVALID
        assert fn(P, 4, 33, 8, P, None, None) == INVALID
        for M in (0, -1, 2 ** 30 + 1):
            assert fn(P, M, 33, 8, P, P, None) == INVALID
        for K in (0, 1, 17, 32, 34, 8193):
            assert fn(P, 4, K, 8, P, P, None) == INVALID, K
        for n in (0, -1, 513):
            assert fn(P, 4, 33, n, P, P, None) == INVALID


# ---------------------------------------------------------------------------------------------------- the loss entries
def _sterms(mag_l1=1.0, log_mag_l1=0.0, sc=0.0, complex_l1=0.0, log_eps=1e-3, sc_eps=1.0):
    return _lib.WunSpectralTerms(mag_l1, log_mag_l1, sc, complex_l1, log_eps, sc_eps)


def _mterms(mel_l1=1.0, log_mel_l1=1.0, log_eps=1e-3):
    return _lib.WunMelTerms(mel_l1, log_mel_l1, log_eps)


def _loss(lib, fft=False, outputs=P, targets=P, S=2, B=3, T=200, Cn=2, mse_weight=0.0, res=((64, 48),), weights=(1.0,), tables=None,
          losses=P, scratch=P, nres=None, null_tables=False, terms=None, null_terms=False, mel=None, null_mel=False, n_mels=(8,),
          null_n_mels=False, mel_tables=None, null_mel_tables=False):
    n = max(len(res), 1)
    n_fft = (C.c_int32 * n)(*[r[0] for r in res])
    hop = (C.c_int32 * n)(*[r[1] for r in res])
    w = (C.c_float * n)(*weights)
    tabs = (C.c_void_p * n)(*(tables if tables is not None else [P] * len(res)))
    tw = None if null_terms else C.byref(terms if terms is not None else _sterms())
    mw = None if null_mel else C.byref(mel if mel is not None else _mterms())
    nm = None if null_n_mels else (C.c_int32 * n)(*n_mels)
    mt = None if null_mel_tables else (C.c_void_p * n)(*(mel_tables if mel_tables is not None else [P] * len(res)))
    fn = lib.wun_spectral_loss_mel_fft if fft else lib.wun_spectral_loss_mel
    return fn(outputs, targets, S, B, T, Cn, mse_weight, len(res) if nres is None else nres, n_fft, hop, w, tw,
              None if null_tables else tabs, P, losses, scratch, None, mw, nm, mt)


BAD_MEL = [{"mel_l1": -1.0}, {"mel_l1": float("nan")}, {"log_mel_l1": float("inf")}, {"log_mel_l1": -0.5},
           {"log_eps": 0.0}, {"log_eps": -1e-3}, {"log_eps": float("nan")}, {"log_eps": float("inf")}]


@pytest.mark.parametrize("fft", [False, True])
def test_loss_argument_errors(lib, fft):
    """Every refusal comes before any GPU work: the pointers are not device memory and there may be no device at all.  The
    sibling's refusals first (tests/test_mrstft_host.py), in its order, then those of the mel arguments."""
    for kw in ({"outputs": None}, {"targets": None}, {"losses": None}, {"scratch": None}, {"null_tables": True}, {"tables": [None]}):
        assert _loss(lib, fft, **kw) == INVALID, kw
    for kw in ({"S": 0}, {"B": 0}, {"Cn": 0}, {"Cn": 3}, {"S": -1}, {"T": 63}, {"res": ((64, 0),)}, {"res": ((64, 65),)}, {"nres": -1},
               {"res": ((64, 48),) * 9, "weights": (1.0,) * 9, "n_mels": (8,) * 9}):
        assert _loss(lib, fft, **kw) == INVALID, kw
    for bad in (-1.0, float("nan"), float("inf")):
        assert _loss(lib, fft, weights=(bad,)) == INVALID and _loss(lib, fft, mse_weight=bad) == INVALID
    for bad in (32, 96, 0, 16384) + (() if fft else (4096,)):
        assert _loss(lib, fft, res=((bad, 16),), T=20000) == UNSUPPORTED, bad
    assert _loss(lib, fft, null_terms=True) == INVALID and b"terms" in lib.wun_last_error()
    assert _loss(lib, fft, terms=_sterms(log_eps=0.0)) == INVALID and _loss(lib, fft, terms=_sterms(sc=-1.0)) == INVALID
    # the mel arguments
    assert _loss(lib, fft, null_mel=True) == INVALID and b"mel" in lib.wun_last_error()
    for kw in BAD_MEL:
        assert _loss(lib, fft, mel=_mterms(**kw)) == INVALID, kw
        assert _loss(lib, fft, res=(), mel=_mterms(**kw)) == INVALID, kw
    assert _loss(lib, fft, null_n_mels=True) == INVALID and _loss(lib, fft, null_mel_tables=True) == INVALID
    for bad in (0, -1, 513):
        assert _loss(lib, fft, n_mels=(bad,)) == INVALID and b"n_mels" in lib.wun_last_error()
    assert _loss(lib, fft, mel_tables=[None]) == INVALID and b"mel table" in lib.wun_last_error()
    assert _loss(lib, fft, mel=_mterms(0.0, 0.0), mel_tables=[None]) == INVALID     # ... with both mel weights 0 too
    # the sibling's checks come first
    assert _loss(lib, fft, res=((96, 16),), T=10000, null_mel=True) == UNSUPPORTED
    assert _loss(lib, fft, outputs=None, null_mel=True) == INVALID and b"null argument" in lib.wun_last_error()
    assert _loss(lib, fft, terms=_sterms(log_eps=0.0), null_mel=True) == INVALID and b"log_eps" in lib.wun_last_error()


def _scratch(lib, fft=False, S=2, B=3, T=200, Cn=2, res=((64, 48),), nres=None, terms=None, mel=None, null_mel=False, n_mels=(8,),
             null_n_mels=False):
    n = max(len(res), 1)
    fn = lib.wun_spectral_mel_fft_scratch_floats if fft else lib.wun_spectral_mel_scratch_floats
    return fn(S, B, T, Cn, len(res) if nres is None else nres, (C.c_int32 * n)(*[r[0] for r in res]),
              (C.c_int32 * n)(*[r[1] for r in res]), C.byref(terms if terms is not None else _sterms()),
              None if null_mel else C.byref(mel if mel is not None else _mterms()), None if null_n_mels else (C.c_int32 * n)(*n_mels))


@pytest.mark.parametrize("fft", [False, True])
def test_scratch_argument_errors_and_size(lib, fft):
    assert _scratch(lib, fft, S=0) == INVALID and _scratch(lib, fft, T=63) == INVALID and _scratch(lib, fft, nres=9) == INVALID
    assert _scratch(lib, fft, res=((100, 10),)) == UNSUPPORTED and _scratch(lib, fft, res=((100, 10),), null_mel=True) == UNSUPPORTED
    assert _scratch(lib, fft, null_mel=True) == INVALID and _scratch(lib, fft, null_n_mels=True) == INVALID
    for kw in BAD_MEL:
        assert _scratch(lib, fft, mel=_mterms(**kw)) == INVALID, kw
    for bad in (0, 513):
        assert _scratch(lib, fft, n_mels=(bad,)) == INVALID
    # the documented size.  R = 12 rows, F = 3, K = 33: M = 36 frames, 8 bands: 288 mel values, one partial per term
    n_fft, hop = (C.c_int32 * 1)(64), (C.c_int32 * 1)(48)
    sib = lib.wun_spectral_terms_fft_scratch_floats if fft else lib.wun_spectral_terms_scratch_floats
    for st in (_sterms(), _sterms(1, 1, 1, 1), _sterms(0, 0, 0, 0)):
        old = sib(2, 3, 200, 2, 1, n_fft, hop, C.byref(st))
        assert _scratch(lib, fft, terms=st) == old + 2 * 36 * 8 + 2 * 2
        assert _scratch(lib, fft, terms=st, mel=_mterms(1.0, 0.0)) == old + 2 * 36 * 8 + 2 * 1
        assert _scratch(lib, fft, terms=st, mel=_mterms(0.0, 0.0)) == old
    big = _scratch(lib, fft, T=64 + 48 * 99, n_mels=(24,), terms=_sterms(0, 0, 0, 0))     # M = 1200 frames: 28800 mel values
    assert big == 1200 * (4 * 33 + 64) + 2 * 1200 * 24 + 2 * (-(-(12 * (64 + 48 * 99)) // 1024) + 2 * -(-28800 // 1024)) + 2
    # the Python front end follows the entry in use
    loss = spectral.SpectralLoss([(64, 48)], terms={"mag_l1": 1}, mel={"n_mels": 8, "sample_rate": 8192}, transform="fft" if fft else "gemm")
    assert loss.scratch_floats((2, 3, 200, 2)) == _scratch(lib, fft)


# ---------------------------------------------------------------------------------------------------- the Python front end
def test_mel_none_is_todays_object():
    for kw in ({}, {"terms": {"sc": 1.0, "log_mag_l1": 1.0}}):
        a = spectral.SpectralLoss([(64, 48), (128, 32)], **kw)
        b = spectral.SpectralLoss([(64, 48), (128, 32)], mel=None, **kw)
        assert a.mel is None and b.mel is None and a._mel is None and b._mel is None
        assert a.num_losses == b.num_losses == (2 + 5 * 2 if kw else 2 + 2) and a.terms == b.terms
        assert (a._terms is None) == (b._terms is None) == (not kw)
        if kw:
            assert sorted(b.term_losses(torch.zeros(12))) == sorted(spectral.TERMS)
            assert bytes(a._terms) == bytes(b._terms)
        else:
            with pytest.raises(ValueError):
                b.term_losses(torch.zeros(4))
    assert spectral.TERMS == ("mag_l1", "log_mag_l1", "sc", "complex_l1") and spectral.MEL_TERMS == ("mel_l1", "log_mel_l1")


def test_python_front_end_mel():
    M = {"n_mels": 8, "sample_rate": 8192}
    for bad in ({"bands": 8}, dict(M, terms={"mel": 1.0}), dict(M, terms={"mel_l1": -1.0}), dict(M, terms={"mel_l1": float("nan")}),
                dict(M, log_eps=0.0), dict(M, log_eps=float("inf")), dict(M, n_mels=[8, 8]), {"n_mels": 8}, {"sample_rate": 8192},
                dict(M, norm="slaney"), dict(M, n_mels=0), dict(M, fmin=5000.0), dict(M, sample_rate=0.0), dict(M, eps=1.0)):
        with pytest.raises(ValueError):
            spectral.SpectralLoss([(64, 48)], mel=bad)
    with pytest.raises(ValueError):
        spectral.SpectralLoss.from_config({"resolutions": [[64, 48]], "mel": dict(M, bands=3)})
    with pytest.raises(ValueError):
        spectral.SpectralLoss.from_config({"resolutions": [[64, 48]], "mels": M})
    spec = {"resolutions": [[64, 48], [128, 32]], "mse_weight": 1.0, "terms": {"sc": 1},
            "mel": {"n_mels": [8, 16], "sample_rate": 8192, "fmin": 50.0, "fmax": 4000.0, "norm": "area",
                    "terms": {"log_mel_l1": 2.0}, "log_eps": 1e-2}}
    loss = spectral.SpectralLoss.from_config(spec)
    assert loss.mel == {"n_mels": [8, 16], "sample_rate": 8192.0, "fmin": 50.0, "fmax": 4000.0, "norm": "area",
                        "terms": {"mel_l1": 0.0, "log_mel_l1": 2.0}, "log_eps": 1e-2}
    assert loss.terms == {"mag_l1": 0.0, "log_mag_l1": 0.0, "sc": 1.0, "complex_l1": 0.0} and loss.num_losses == 2 + 7 * 2
    m = loss._mel
    assert (m.mel_l1, m.log_mel_l1) == (0.0, 2.0) and m.log_eps == np.float32(1e-2) and list(loss._n_mels) == [8, 16]
    again = spectral.SpectralLoss.from_config(dict(spec, mel=loss.mel))            # the stored dict round-trips
    assert again.mel == loss.mel and spectral.SpectralLoss.from_config(loss) is loss
    # defaults: both mel terms at weight 1, log_eps 1e-3, one band count for every resolution, no linear-frequency term
    d = spectral.SpectralLoss([(64, 48), (128, 32)], mel={"n_mels": 8, "sample_rate": 8192})
    assert d.mel["terms"] == {"mel_l1": 1.0, "log_mel_l1": 1.0} and d.mel["log_eps"] == 1e-3 and d.mel["n_mels"] == [8, 8]
    assert d.terms == {t: 0.0 for t in spectral.TERMS} and d.term_weight("mel_l1") == 1.0 and d.term_weight("sc") == 0.0
    # term_losses: the four views, then the two mel views behind the 2 + 5 nres slots
    losses = torch.arange(16, dtype=torch.float32)
    per = loss.term_losses(losses)
    assert sorted(per) == sorted(spectral.TERMS + spectral.MEL_TERMS)
    assert per["mag_l1"].tolist() == [4.0, 8.0] and per["complex_l1"].tolist() == [7.0, 11.0]
    assert per["mel_l1"].tolist() == [12.0, 14.0] and per["log_mel_l1"].tolist() == [13.0, 15.0]
    losses[13] = -1.0
    assert per["log_mel_l1"][0].item() == -1.0
    assert hasattr(training.Trainer, "term_parts")


# ---------------------------------------------------------------------------------------------------- the oracle itself
def test_oracle_adjoint_against_torch_autograd():
    rng = np.random.RandomState(31)
    W = mel.filterbank32(128, 8192, 16, fmin=40.0, norm="area").astype(np.float64)
    M, g = rng.rand(7, 65), rng.randn(7, 16)
    tm = torch.from_numpy(M).requires_grad_(True)
    p = tm @ torch.from_numpy(W).T
    assert np.abs(p.detach().numpy() - mel.project(W, M)).max() <= 1e-12 * np.abs(p.detach().numpy()).max()
    (p * torch.from_numpy(g)).sum().backward()
    q = mel.adjoint(W, g)
    assert q.shape == M.shape and np.abs(q - tm.grad.numpy()).max() <= 1e-12 * np.abs(q).max()


@pytest.mark.parametrize("terms", [{}, {"sc": 1.0, "log_mag_l1": 1.0}])
def test_oracle_loss_against_torch_autograd(terms):
    """Losses and gradient of the oracle against autograd on a float64 torch restatement: the linear-frequency part of
    tests/_mrstft_np.py plus the mel terms on |torch.stft| @ W^T, two resolutions, S = 2, stereo."""
    rng = np.random.RandomState(32)
    out, tgt = rng.randn(2, 2, 200, 2), rng.randn(2, 2, 200, 2)
    res, w, mw, le, se = [(64, 48), (128, 32)], [1.0, 0.5], 0.3, 1e-3, 1.0
    m = {"W": [mel.filterbank32(64, 8192, 8), mel.filterbank32(128, 8192, 16)], "terms": {"mel_l1": 0.7, "log_mel_l1": 0.4}, "log_eps": 1e-2}
    losses, g = mel.loss_and_grad(out, tgt, res, w, mw, terms, le, se, m)
    to, tt = torch.from_numpy(out).requires_grad_(True), torch.from_numpy(tgt)
    tl, total = mr.torch_total(to, tt, res, w, mw, terms, le, se)
    rows = lambda x: x.permute(0, 1, 3, 2).reshape(-1, x.shape[2])  # noqa: E731
    want = np.zeros(2 + 7 * 2)
    want[:12] = tl.detach().numpy()
    for j, (n_fft, hop) in enumerate(res):
        win = torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
        W = torch.from_numpy(m["W"][j].astype(np.float64))
        pe, pt = (torch.stft(rows(x), n_fft, hop_length=hop, win_length=n_fft, window=win, center=False, onesided=True,
                             return_complex=True).abs().transpose(1, 2) @ W.T for x in (to, tt))
        l1, ll = (pe - pt).abs().mean(), (torch.log(pe + 1e-2) - torch.log(pt + 1e-2)).abs().mean()
        total = total + w[j] * (0.7 * l1 + 0.4 * ll)
        want[12 + 2 * j], want[13 + 2 * j] = l1.item(), ll.item()
        want[2 + j] += 0.7 * l1.item() + 0.4 * ll.item()
    want[0] = total.item()
    total.backward()
    assert losses.shape == (16,) and np.abs(losses - want).max() <= 1e-9 * np.abs(want).max()
    tg = to.grad.numpy()
    assert np.abs(g - tg).max() <= 1e-9 * np.abs(tg).max()
    # the fp32 stand-in is the same formula: close to float64, not equal to it
    signs = [np.sign(mel.sp.magnitude(out, n, h) - mel.sp.magnitude(tgt, n, h)) for n, h in res]
    msigns = [np.sign(mel.project(W, mel.sp.magnitude(out, n, h)) - mel.project(W, mel.sp.magnitude(tgt, n, h)))
              for (n, h), W in zip(res, m["W"])]
    l32, g32 = mel.loss_and_grad_fp32(out.astype(np.float32), tgt.astype(np.float32), res, w, mw, terms, le, se, m, signs, msigns)
    l64, g64 = mel.loss_and_grad(out.astype(np.float32), tgt.astype(np.float32), res, w, mw, terms, le, se, m, signs, msigns)
    assert l32.dtype == g32.dtype == np.float32
    assert 0 < np.abs(g32 - g64).max() / np.abs(g64).max() < 1e-4 and 0 < np.abs(l32 - l64).max() / np.abs(l64).max() < 1e-4
