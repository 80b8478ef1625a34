"""CPU-only checks of the waveform losses (include/wun.h: wun_waveform_*; wave_u_net_amd.waveform): the float64
oracle's closed-form gradient (tests/_waveform_np.py) against central differences and against torch float64 autograd of the same
formulas written independently, the scratch formula, every argument error before any GPU work, and the Python front end's
argument errors.  The device path is checked against that oracle in tests/test_gpu_waveform.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _waveform_np as ora  # noqa: E402
from _observed import record  # noqa: E402
from wave_u_net_amd import _lib, config, spectral, waveform  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wun_waveform_scratch_floats", "wun_waveform_loss")
INVALID = -1
P = 0x1000                  # a non-null "device pointer": every call below must fail before any GPU work reads it
ALL = {"mse": 0.7, "l1": 0.4, "si_sdr": 0.05, "snr": 0.03}
TERM_SETS = {"mse": {"mse": 1.0}, "l1": {"l1": 1.0}, "si_sdr": {"si_sdr": 1.0}, "snr": {"snr": 1.0}, "all": ALL}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _inputs(seed=7, shape=(2, 2, 37, 2)):
    """Estimates = targets + noise, with a mean per row so that zero_mean matters."""
    rng = np.random.RandomState(seed)
    tgt = rng.randn(*shape) + 0.3
    out = tgt * 0.8 + 0.5 * rng.randn(*shape) - 0.1
    return out, tgt


def test_declared_exported_and_documented(lib):
    hdr = open(os.path.join(ROOT, "include", "wun.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in NAMES:
        assert name in doc and name in design, name
    assert "wun_waveform_terms" in hdr and C.sizeof(_lib.WunWaveformTerms) == 24
    assert [f[0] for f in _lib.WunWaveformTerms._fields_] == ["mse", "l1", "si_sdr", "snr", "eps", "zero_mean"]


@pytest.mark.parametrize("zero_mean", [True, False])
@pytest.mark.parametrize("tname", sorted(TERM_SETS))
def test_oracle_gradient_against_central_differences(tname, zero_mean):
    """h = 1e-6 on unit-scale data: h^2 truncation and 1e-16 / h cancellation both sit near 1e-10 of the loss's scale; the l1
    term is linear between its kinks and no |d| of this seed is within h of one."""
    out, tgt = _inputs()
    terms = TERM_SETS[tname]
    losses, g = ora.loss_and_grad(out, tgt, terms, 1e-8, zero_mean)
    assert abs(losses[0] - sum(terms.get(t, 0.0) * losses[1 + i] for i, t in enumerate(ora.TERMS))) < 1e-14
    assert np.abs(out - tgt).min() > 1e-5
    h, worst = 1e-6, 0.0
    flat = out.reshape(-1)
    for i in range(flat.size):
        p, m = flat.copy(), flat.copy()
        p[i] += h
        m[i] -= h
        num = (ora.loss_and_grad(p.reshape(out.shape), tgt, terms, 1e-8, zero_mean)[0][0]
               - ora.loss_and_grad(m.reshape(out.shape), tgt, terms, 1e-8, zero_mean)[0][0]) / (2 * h)
        worst = max(worst, abs(num - g.reshape(-1)[i]))
    scale = np.abs(g).max()
    record("waveform::test_oracle_gradient_against_central_differences[%s-%s]" % (tname, zero_mean),
           "max |numeric - analytic| / max |g|", worst / scale, 1e-6)
    assert worst / scale < 1e-6


def _torch_total(out, tgt, terms, eps, zero_mean):
    """The same losses written from the textbook forms, not the oracle's sums: projection and residual, explicit centring."""
    S, B = out.shape[:2]
    e, t = out.reshape(S * B, -1), tgt.reshape(S * B, -1)
    total = 0.0
    if terms.get("mse", 0) > 0:
        total = total + terms["mse"] * torch.mean((out - tgt) ** 2)
    if terms.get("l1", 0) > 0:
        total = total + terms["l1"] * torch.mean(torch.abs(out - tgt))
    if zero_mean:
        e, t = e - e.mean(1, keepdim=True), t - t.mean(1, keepdim=True)
    if terms.get("si_sdr", 0) > 0:
        dot, tt = (e * t).sum(1), (t * t).sum(1)
        P = dot ** 2 / (tt + eps)                             # the energy of the projection of e on t
        Nn = (e * e).sum(1) - P                               # and of the residual
        si = 10.0 * torch.log10((P + eps) / (Nn + eps))
        total = total - terms["si_sdr"] * si.mean()
    if terms.get("snr", 0) > 0:
        snr = 10.0 * torch.log10(((t * t).sum(1) + eps) / (((e - t) ** 2).sum(1) + eps))
        total = total - terms["snr"] * snr.mean()
    return total


@pytest.mark.parametrize("zero_mean", [True, False])
@pytest.mark.parametrize("tname", sorted(TERM_SETS))
def test_oracle_gradient_against_torch_autograd(tname, zero_mean):
    out, tgt = _inputs(seed=8, shape=(3, 2, 41, 1))
    terms = TERM_SETS[tname]
    losses, g = ora.loss_and_grad(out, tgt, terms, 1e-8, zero_mean)
    x = torch.from_numpy(out).requires_grad_(True)
    total = _torch_total(x, torch.from_numpy(tgt), terms, 1e-8, zero_mean)
    total.backward()
    err = np.abs(x.grad.numpy() - g).max() / np.abs(g).max()
    lerr = abs(total.item() - losses[0]) / abs(losses[0])
    tag = "waveform::test_oracle_gradient_against_torch_autograd[%s-%s]" % (tname, zero_mean)
    record(tag, "max |autograd - closed form| / max |g|", err, 1e-9)
    record(tag, "|total - oracle| / |oracle|", lerr, 1e-9)
    assert err <= 1e-9 and lerr <= 1e-9


def test_oracle_layout_and_consequences():
    out, tgt = _inputs(shape=(2, 3, 29, 2))
    losses, g = ora.loss_and_grad(out, tgt, ALL)
    st = ora.row_stats(out, tgt, 1e-8, True)
    assert losses.shape == (9,) and g.shape == out.shape
    assert np.allclose(losses[5:7], st["SI"].reshape(2, 3).mean(1)) and np.allclose(losses[7:9], st["SNR"].reshape(2, 3).mean(1))
    assert abs(losses[3] + losses[5:7].mean()) < 1e-12 and abs(losses[4] + losses[7:9].mean()) < 1e-12
    # a term of weight 0 is reported as 0
    l1, _ = ora.loss_and_grad(out, tgt, {"l1": 1.0})
    assert l1[1] == 0 and l1[3] == 0 and l1[4] == 0 and np.all(l1[5:] == 0) and l1[0] == l1[2]
    # zero estimates: the si_sdr gradient is exactly 0; a silent target row stays finite
    _, g0 = ora.loss_and_grad(np.zeros_like(out), tgt, {"si_sdr": 1.0})
    assert np.all(g0 == 0)
    silent = tgt.copy()
    silent[1, 2] = 0
    ls, gs = ora.loss_and_grad(out, silent, {"si_sdr": 1.0}, zero_mean=False)
    See = (out[1, 2] ** 2).sum()
    assert np.all(np.isfinite(ls)) and np.all(np.isfinite(gs))
    assert abs(ora.row_stats(out, silent, 1e-8, False)["SI"][5] - 10 * np.log10(1e-8 / (See + 1e-8))) < 1e-9
    # estimates equal to the targets: about 10 log10(Stt / 2 eps), not infinity
    le, _ = ora.loss_and_grad(tgt, tgt, {"si_sdr": 1.0})
    Stt = ora.row_stats(tgt, tgt, 1e-8, True)["Stt"]
    assert np.all(np.isfinite(le)) and abs(-le[3] - np.mean(10 * np.log10(Stt / 2e-8))) < 1e-3


def _terms(mse=0.0, l1=0.0, si_sdr=0.0, snr=0.0, eps=1e-8, zero_mean=1):
    return _lib.WunWaveformTerms(mse, l1, si_sdr, snr, eps, zero_mean)


def test_scratch_formula(lib):
    """2 ceil(N / 1024) flat partials, 6 R ceil(n / 1024) row partials and 8 R row scalars as float64, plus 2 floats."""
    for S, B, T, Cn in ((2, 3, 165, 2), (2, 3, 700, 2), (1, 2, 512, 2), (3, 2, 2049, 1), (2, 2, 5000, 2), (1, 1, 1, 1), (2, 16, 16389, 1)):
        R, n = S * B, T * Cn
        want = 2 * (2 * -(-(R * n) // 1024) + 6 * R * -(-n // 1024) + 8 * R) + 2
        for t in (_terms(mse=1.0), _terms(si_sdr=1.0, snr=2.0), _terms(1.0, 1.0, 1.0, 1.0, zero_mean=0)):
            assert lib.wun_waveform_scratch_floats(S, B, T, Cn, C.byref(t)) == want, (S, B, T, Cn)
        assert waveform.WaveformLoss({"l1": 1}).scratch_floats((S, B, T, Cn)) == want
    for kw in ({"S": 0}, {"B": 0}, {"T": 0}, {"Cn": 3}, {"Cn": 0}):
        a = dict(S=2, B=3, T=100, Cn=2)
        a.update(kw)
        assert lib.wun_waveform_scratch_floats(a["S"], a["B"], a["T"], a["Cn"], C.byref(_terms(mse=1.0))) == INVALID, kw
    assert lib.wun_waveform_scratch_floats(2, 3, 100, 2, None) == INVALID
    assert lib.wun_waveform_scratch_floats(2, 3, 100, 2, C.byref(_terms(mse=-1.0))) == INVALID
    assert lib.wun_waveform_scratch_floats(2, 3, 100, 2, C.byref(_terms(mse=1.0, eps=0.0))) == INVALID


def _loss(lib, outputs=P, targets=P, S=2, B=3, T=200, Cn=2, terms="default", accumulate=0, d_outputs=P, losses=P, scratch=P):
    t = _terms(mse=1.0, si_sdr=1.0) if terms == "default" else terms
    return lib.wun_waveform_loss(outputs, targets, S, B, T, Cn, None if t is None else C.byref(t), accumulate, d_outputs, losses,
                                 scratch, None)


def test_loss_argument_errors(lib):
    """Every refusal comes before any GPU work: the pointers are not device memory and there may be no device at all."""
    for kw in ({"outputs": None}, {"targets": None}, {"losses": None}, {"scratch": None}, {"terms": None}):
        assert _loss(lib, **kw) == INVALID, kw
    for kw in ({"S": 0}, {"S": -1}, {"B": 0}, {"T": 0}, {"T": -5}, {"Cn": 0}, {"Cn": 3}):
        assert _loss(lib, **kw) == INVALID, kw
    for bad in (-1.0, float("nan"), float("inf")):
        for name in ("mse", "l1", "si_sdr", "snr"):
            assert _loss(lib, terms=_terms(**{name: bad})) == INVALID, (name, bad)
    for bad in (0.0, -1e-8, float("nan"), float("inf")):
        assert _loss(lib, terms=_terms(mse=1.0, eps=bad)) == INVALID, bad
    assert b"eps" in lib.wun_last_error()
    for bad in (2, -1):
        assert _loss(lib, accumulate=bad) == INVALID, bad
    assert _loss(lib, accumulate=1, d_outputs=None) == INVALID
    assert b"accumulate" in lib.wun_last_error()


def test_abi_sizes_still_reports_three_structs(lib):
    sizes = (C.c_int64 * 4)(0, 0, 0, -7)
    lib.wun_abi_sizes(sizes, 4)
    assert sizes[3] == -7


def test_python_front_end_refuses_bad_settings():
    W = waveform.WaveformLoss
    for bad in ({}, {"mse": 0.0, "l1": 0}, {"sdr": 1.0}, {"mse": -1.0}, {"l1": float("nan")}, {"snr": float("inf")}):
        with pytest.raises(ValueError):
            W(bad)
    with pytest.raises(ValueError):
        W.from_config({"terms": {}})
    with pytest.raises(ValueError):
        W.from_config({"terms": {"mse": 1}, "epsilon": 1e-8})
    with pytest.raises(ValueError):
        W.from_config({"terms": {"mse": 1, "sisdr": 1}})
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            W({"mse": 1}, eps=bad)
    loss = W.from_config({"terms": {"l1": 1, "si_sdr": 0.05}, "eps": 1e-6, "zero_mean": False})
    assert loss.terms == {"mse": 0.0, "l1": 1.0, "si_sdr": 0.05, "snr": 0.0} and loss.eps == 1e-6 and loss.zero_mean is False
    assert W.from_config(None) is None and W.from_config(loss) is loss
    assert W({"mse": 1}).eps == 1e-8 and W({"mse": 1}).zero_mean is True
    assert waveform.TERMS == ("mse", "l1", "si_sdr", "snr") == ora.TERMS
    assert loss.num_losses_for(3) == 11
    with pytest.raises(ValueError):
        waveform.CombinedLoss(loss, loss)
    with pytest.raises(ValueError):
        waveform.CombinedLoss(spectral.SpectralLoss([(64, 48)]), {"terms": {"mse": 1}})
    both = waveform.CombinedLoss(spectral.SpectralLoss([(64, 48)], mse_weight=1.0), loss)
    assert both.spectral.resolutions == [(64, 48)] and both.waveform is loss
    with pytest.raises(ValueError):
        waveform.waveform_loss(torch.zeros(1, 1, 8, 1), torch.zeros(1, 1, 8, 1), loss)          # there is no CPU path


def test_config_keys_and_validation_metric():
    assert config.EXTENSION_DEFAULTS["waveform_loss"] is None and config.EXTENSION_DEFAULTS["validation_metric"] == "mse"
    assert "waveform_loss" not in config.BASE_MODEL_CONFIG and "validation_metric" not in config.BASE_MODEL_CONFIG
    assert waveform.validation_metric({}) == "mse" and waveform.validation_metric({"validation_metric": "si_sdr"}) == "si_sdr"
    for bad in ("sdr", "snr", None, 1):
        with pytest.raises(ValueError):
            waveform.validation_metric({"validation_metric": bad})
    v = waveform.validation_loss({"waveform_loss": {"terms": {"l1": 1}, "eps": 1e-6, "zero_mean": False}})
    assert v.terms == {"mse": 0.0, "l1": 0.0, "si_sdr": 1.0, "snr": 0.0} and v.eps == 1e-6 and v.zero_mean is False
    d = waveform.validation_loss({})
    assert d.eps == 1e-8 and d.zero_mean is True
    # validation.test refuses the value before it touches data or a device
    from wave_u_net_amd import validation
    import wave_u_net_amd as wun
    with pytest.raises(ValueError):
        validation.test(wun.get_config("baseline", validation_metric="sdr"), "valid", "x", None, tracks=[])
