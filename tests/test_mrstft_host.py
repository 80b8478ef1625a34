"""CPU-only checks of the four-term spectral loss (include/wun.h: wun_spectral_terms_scratch_floats, wun_spectral_loss_terms;
wave_u_net_amd.spectral.SpectralLoss(terms=...)): the float64 oracle tests/_mrstft_np.py against torch.autograd
on a float64 torch restatement of the definitions, its fp32 stand-in, every refusal of the two entries and of the new
SpectralLoss arguments before any GPU work, the scratch formula, the bindings and the documentation.  The device path is
checked against that oracle in tests/test_gpu_mrstft.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mrstft_np as mr  # noqa: E402
import _spectral_np as ora  # noqa: E402
from _observed import record  # noqa: E402
from wave_u_net_amd import _lib, spectral, training  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wun_spectral_terms_scratch_floats", "wun_spectral_loss_terms")
INVALID, UNSUPPORTED = -1, -2
P = 0x1000                  # a non-null "device pointer": every call below must fail before any GPU work reads it
ALL = {"mag_l1": 0.7, "log_mag_l1": 0.4, "sc": 1.3, "complex_l1": 0.6}
TERM_SETS = {"mag_l1": {"mag_l1": 1.0}, "log_mag_l1": {"log_mag_l1": 1.0}, "sc": {"sc": 1.0}, "complex_l1": {"complex_l1": 1.0},
             "sc_log": {"sc": 1.0, "log_mag_l1": 1.0}, "all": ALL}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _terms(mag_l1=1.0, log_mag_l1=0.0, sc=0.0, complex_l1=0.0, log_eps=1e-3, sc_eps=1.0):
    return _lib.WunSpectralTerms(mag_l1, log_mag_l1, sc, complex_l1, log_eps, sc_eps)


def test_declared_exported_and_documented(lib):
    hdr = open(os.path.join(ROOT, "include", "wun.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in NAMES:
        assert name in doc and name in design, name
    assert "wun_spectral_terms" in hdr and C.sizeof(_lib.WunSpectralTerms) == 24
    assert spectral.TERMS == mr.TERMS == tuple(n for n, _ in _lib.WunSpectralTerms._fields_[:4])


# ---------------------------------------------------------------------------------------------------- the oracle itself
@pytest.mark.parametrize("name", sorted(TERM_SETS))
def test_oracle_against_torch_autograd(name):
    """Losses and gradient of the numpy oracle against autograd on the float64 torch restatement, two resolutions, S = 2, stereo.
    Random inputs: no |d| or |E - T| is an exact 0, where sgn and autograd's abs would have to agree on a convention."""
    rng = np.random.RandomState(21)
    out, tgt = rng.randn(2, 2, 200, 2), rng.randn(2, 2, 200, 2)
    res, w, mw, le, se = [(64, 48), (128, 32)], [1.0, 0.5], 0.3, 1e-3, 1.0
    terms = TERM_SETS[name]
    losses, g = mr.loss_and_grad(out, tgt, res, w, mw, terms, le, se)
    to = torch.from_numpy(out).requires_grad_(True)
    tl, total = mr.torch_total(to, torch.from_numpy(tgt), res, w, mw, terms, le, se)
    total.backward()
    tl, tg = tl.detach().numpy(), to.grad.numpy()
    assert losses.shape == (2 + 5 * len(res),)
    el = np.abs(losses - tl).max() / np.abs(tl).max()
    eg = np.abs(g - tg).max() / np.abs(tg).max()
    record("test_oracle_against_torch_autograd[%s]" % name, "losses relative", el, 1e-9)
    record("test_oracle_against_torch_autograd[%s]" % name, "gradient relative", eg, 1e-9)
    assert el <= 1e-9 and eg <= 1e-9
    absent = [2 + len(res) + 4 * j + t for j in range(len(res)) for t, n in enumerate(mr.TERMS) if terms.get(n, 0.0) == 0.0]
    assert np.all(losses[absent] == 0.0)                        # a term whose weight is 0 is reported as 0
    for j in range(len(res)):
        lj = sum(terms.get(n, 0.0) * losses[2 + len(res) + 4 * j + t] for t, n in enumerate(mr.TERMS))
        assert abs(lj - losses[2 + j]) <= 1e-15 * max(lj, 1.0)
    assert abs(losses[0] - (mw * losses[1] + sum(wj * losses[2 + j] for j, wj in enumerate(w)))) <= 1e-14


def test_oracle_mag_l1_is_the_one_term_oracle():
    rng = np.random.RandomState(22)
    out, tgt = rng.randn(2, 1, 165, 2), rng.randn(2, 1, 165, 2)
    l0, g0 = ora.loss_and_grad(out, tgt, [(64, 48)], [0.7], 0.3)
    l1, g1 = mr.loss_and_grad(out, tgt, [(64, 48)], [0.7], 0.3, {"mag_l1": 1.0}, 1e-3, 1.0)
    assert np.allclose(l1[:3], l0, rtol=1e-14, atol=0) and l1[3] == l1[2] and np.allclose(g1, g0, rtol=1e-12, atol=1e-18)


@pytest.mark.parametrize("name", ["sc_log", "all"])
def test_fp32_stand_in_is_close_to_float64(name):
    """grad_fp32 is the same formula in fp32: its distance from float64 is fp32 rounding, far below the gradient's scale."""
    rng = np.random.RandomState(23)
    out, tgt = rng.randn(2, 2, 165, 1).astype(np.float32), rng.randn(2, 2, 165, 1).astype(np.float32)
    res, w = [(64, 48)], [0.5]
    signs = [np.sign(ora.magnitude(out, 64, 48) - ora.magnitude(tgt, 64, 48))]
    _, g64 = mr.loss_and_grad(out, tgt, res, w, 0.25, TERM_SETS[name], 1e-3, 1.0, signs=signs)
    g32 = mr.grad_fp32(out, tgt, res, w, 0.25, TERM_SETS[name], 1e-3, 1.0, signs)
    e = np.abs(g32.astype(np.float64) - g64).max() / np.abs(g64).max()
    record("test_fp32_stand_in_is_close_to_float64[%s]" % name, "max err / max |g64|", e, 1e-4)
    assert g32.dtype == np.float32 and 0 < e < 1e-4


def test_silent_source_and_equal_signals_in_the_oracle():
    rng = np.random.RandomState(24)
    out, tgt = rng.randn(2, 1, 165, 1), rng.randn(2, 1, 165, 1)
    tgt[1] = 0.0
    losses, g = mr.loss_and_grad(out, tgt, [(64, 48)], [1.0], 0.0, {"sc": 1.0}, 1e-3, 0.5)
    me = ora.magnitude(out, 64, 48)
    D1 = (me[1:] ** 2).sum()
    _, _, _, scs = mr.mag_terms(me, ora.magnitude(tgt, 64, 48), 2, 1e-3, 0.5)
    assert np.isfinite(losses).all() and np.isfinite(g).all() and abs(scs[1] - np.sqrt(D1 / 0.5)) <= 1e-12 * scs[1]
    losses, g = mr.loss_and_grad(out, out, [(64, 48)], [1.0], 1.0, ALL, 1e-3, 1.0)
    assert np.all(losses == 0) and np.all(g == 0)


# ---------------------------------------------------------------------------------------------------- refusals
def _loss(lib, outputs=P, targets=P, S=2, B=3, T=200, Cn=2, mse_weight=0.0, res=((64, 48),), weights=(1.0,), tables=None,
          d_outputs=P, losses=P, scratch=P, nres=None, null_tables=False, terms=None, null_terms=False):
    n = max(len(res), 1)
    n_fft = (C.c_int32 * n)(*[r[0] for r in res])
    hop = (C.c_int32 * n)(*[r[1] for r in res])
    w = (C.c_float * n)(*weights)
    tabs = (C.c_void_p * n)(*(tables if tables is not None else [P] * len(res)))
    tw = None if null_terms else C.byref(terms if terms is not None else _terms())
    return lib.wun_spectral_loss_terms(outputs, targets, S, B, T, Cn, mse_weight, len(res) if nres is None else nres, n_fft, hop,
                                       w, tw, None if null_tables else tabs, d_outputs, losses, scratch, None)


BAD_TERMS = [{"mag_l1": -1.0}, {"log_mag_l1": float("nan")}, {"sc": float("inf")}, {"complex_l1": -0.5},
             {"log_eps": 0.0}, {"log_eps": -1e-3}, {"log_eps": float("nan")}, {"log_eps": float("inf")},
             {"sc_eps": 0.0}, {"sc_eps": -1.0}, {"sc_eps": float("nan")}, {"sc_eps": float("inf")}]


def test_loss_terms_argument_errors(lib):
    """Every refusal comes before any GPU work: the pointers are not device memory and there may be no device at all.  The
    refusals of wun_spectral_loss first (tests/test_spectral_host.py), then those of `terms`."""
    for kw in ({"outputs": None}, {"targets": None}, {"losses": None}, {"scratch": None}, {"null_tables": True},
               {"tables": [None]}):
        assert _loss(lib, **kw) == INVALID, kw
    for kw in ({"S": 0}, {"B": 0}, {"Cn": 0}, {"Cn": 3}, {"S": -1}):
        assert _loss(lib, **kw) == INVALID, kw
    assert _loss(lib, T=63) == INVALID
    assert _loss(lib, res=((64, 48), (1024, 768)), weights=(1.0, 1.0), T=1023) == INVALID
    assert _loss(lib, res=((64, 0),)) == INVALID
    assert _loss(lib, res=((64, 65),)) == INVALID
    assert _loss(lib, nres=-1) == INVALID
    assert _loss(lib, res=((64, 48),) * 9, weights=(1.0,) * 9) == INVALID
    for bad in (-1.0, float("nan"), float("inf")):
        assert _loss(lib, weights=(bad,)) == INVALID, bad
        assert _loss(lib, mse_weight=bad) == INVALID, bad
        assert _loss(lib, res=(), weights=(1.0,), mse_weight=bad) == INVALID, bad
    for bad in (32, 96, 4096, 0):
        assert _loss(lib, res=((bad, 16),), T=10000) == UNSUPPORTED, bad
    assert b"n_fft" in lib.wun_last_error()
    assert _loss(lib, null_terms=True) == INVALID and b"terms" in lib.wun_last_error()
    for kw in BAD_TERMS:
        assert _loss(lib, terms=_terms(**kw)) == INVALID, kw
        assert _loss(lib, res=(), terms=_terms(**kw)) == INVALID, kw
    # the existing checks come first: a bad n_fft beside bad terms is UNSUPPORTED, a null pointer beside them names the pointer
    assert _loss(lib, res=((96, 16),), T=10000, terms=_terms(log_eps=0.0)) == UNSUPPORTED
    assert _loss(lib, outputs=None, null_terms=True) == INVALID and b"null argument" in lib.wun_last_error()


def _scratch(lib, S=2, B=3, T=200, Cn=2, res=((64, 48),), nres=None, terms=None, null_terms=False):
    n = max(len(res), 1)
    tw = None if null_terms else C.byref(terms if terms is not None else _terms())
    return lib.wun_spectral_terms_scratch_floats(S, B, T, Cn, len(res) if nres is None else nres,
                                                 (C.c_int32 * n)(*[r[0] for r in res]), (C.c_int32 * n)(*[r[1] for r in res]), tw)


def test_scratch_argument_errors_and_size(lib):
    assert _scratch(lib, S=0) == INVALID and _scratch(lib, T=63) == INVALID and _scratch(lib, nres=9) == INVALID
    assert _scratch(lib, Cn=3) == INVALID and _scratch(lib, res=((64, 65),)) == INVALID
    assert _scratch(lib, res=((100, 10),)) == UNSUPPORTED
    assert _scratch(lib, null_terms=True) == INVALID
    assert _scratch(lib, res=((100, 10),), null_terms=True) == UNSUPPORTED          # the existing checks first
    for kw in BAD_TERMS:
        assert _scratch(lib, terms=_terms(**kw)) == INVALID, kw
    # the documented size.  R = 12 rows, F = 3, K = 33, S = 2: E = 1188 bins, 594 per source
    R, F, K, S = 12, 3, 33, 2
    E = R * F * K
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    mse_parts, parts, src_parts = cdiv(R * 200, 1024), cdiv(E, 1024), cdiv(E // S, 1024)
    base = R * F * (4 * K + 64)
    n_fft, hop = (C.c_int32 * 1)(64), (C.c_int32 * 1)(48)
    old = lib.wun_spectral_scratch_floats(2, 3, 200, 2, 1, n_fft, hop)
    assert _scratch(lib) == base + 2 * (mse_parts + parts) + 2 == old              # mag_l1 alone: wun_spectral_loss's scratch
    assert _scratch(lib, terms=_terms(1, 1, 0, 0)) == base + 2 * (mse_parts + 2 * parts) + 2
    assert _scratch(lib, terms=_terms(0, 0, 0, 1)) == base + 2 * E + 2 * (mse_parts + parts) + 2
    assert _scratch(lib, terms=_terms(0, 0, 1, 0)) == base + 2 * (mse_parts + 2 * S * src_parts + 3 * S) + 2
    assert _scratch(lib, terms=_terms(1, 1, 1, 1)) == base + 2 * E + 2 * (mse_parts + 3 * parts + 2 * S * src_parts + 3 * S) + 2
    assert _scratch(lib, res=(), terms=_terms(1, 1, 1, 1)) == 2 * mse_parts + 2
    # the Python front end follows the entry in use
    shape = (2, 3, 200, 2)
    assert spectral.SpectralLoss([(64, 48)]).scratch_floats(shape) == old
    assert spectral.SpectralLoss([(64, 48)], terms={"sc": 1, "complex_l1": 1}).scratch_floats(shape) == \
        _scratch(lib, terms=_terms(0, 0, 1, 1))
    with pytest.raises(ValueError):
        spectral.SpectralLoss([(64, 48)], terms={"sc": 1}).scratch_floats((2, 3, 63, 2))
    with pytest.raises(NotImplementedError):
        spectral.SpectralLoss([(96, 48)], terms={"sc": 1}).scratch_floats(shape)


# ---------------------------------------------------------------------------------------------------- the Python front end
def test_python_front_end_terms():
    with pytest.raises(ValueError):
        spectral.SpectralLoss([(64, 48)], terms={"mag": 1.0})                       # an unknown name
    with pytest.raises(ValueError):
        spectral.SpectralLoss([(64, 48)], terms={"sc": -1.0})
    with pytest.raises(ValueError):
        spectral.SpectralLoss([(64, 48)], terms={"sc": float("nan")})
    for kw in ({"log_eps": 0.0}, {"log_eps": float("inf")}, {"sc_eps": -1.0}, {"sc_eps": float("nan")}):
        with pytest.raises(ValueError):
            spectral.SpectralLoss([(64, 48)], terms={"sc": 1.0}, **kw)
    with pytest.raises(ValueError):
        spectral.SpectralLoss.from_config({"resolutions": [[64, 48]], "terms": {"sc": 1}, "eps": 1.0})
    loss = spectral.SpectralLoss.from_config({"resolutions": [[64, 48], [128, 32]], "mse_weight": 1.0,
                                              "terms": {"sc": 1, "log_mag_l1": 2}, "log_eps": 1e-2, "sc_eps": 0.5})
    assert loss.terms == {"mag_l1": 0.0, "log_mag_l1": 2.0, "sc": 1.0, "complex_l1": 0.0}     # a missing name is weight 0
    assert loss.log_eps == 1e-2 and loss.sc_eps == 0.5 and loss.num_losses == 2 + 5 * 2
    t = loss._terms
    assert (t.mag_l1, t.log_mag_l1, t.sc, t.complex_l1) == (0.0, 2.0, 1.0, 0.0)
    assert t.log_eps == np.float32(1e-2) and t.sc_eps == 0.5
    # term_losses: views of the losses vector, [nres] each, in the entry's order
    losses = torch.arange(12, dtype=torch.float32)
    per = loss.term_losses(losses)
    assert sorted(per) == sorted(spectral.TERMS)
    assert per["mag_l1"].tolist() == [4.0, 8.0] and per["log_mag_l1"].tolist() == [5.0, 9.0]
    assert per["sc"].tolist() == [6.0, 10.0] and per["complex_l1"].tolist() == [7.0, 11.0]
    losses[6] = -1.0
    assert per["sc"][0].item() == -1.0
    # terms=None is the old object
    old = spectral.SpectralLoss([(64, 48)])
    assert old.terms is None and old._terms is None and old.num_losses == 3 and old.log_eps == 1e-3 and old.sc_eps == 1.0
    with pytest.raises(ValueError):
        old.term_losses(torch.zeros(3))
    mr3 = spectral.SpectralLoss.multi_resolution()
    assert mr3.resolutions == [(512, 128), (1024, 256), (2048, 512)] and mr3.weights == [1.0, 1.0, 1.0]
    assert mr3.terms == {"mag_l1": 0.0, "log_mag_l1": 1.0, "sc": 1.0, "complex_l1": 0.0} and mr3.mse_weight == 0.0
    assert hasattr(training.Trainer, "term_parts")
