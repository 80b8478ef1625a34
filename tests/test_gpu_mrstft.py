"""GPU tests of the four-term spectral loss (include/wun.h: wun_spectral_loss_terms; spectral.SpectralLoss(terms=...); DESIGN.md
5.14) against the float64 oracle tests/_mrstft_np.py.

Bounds (tests/test_gpu_spectral.py has the first two).  beta[r][f] = n_fft 2^-24 sum_n |w[n] x[f hop + n]| bounds the error of Re
and of Im; a magnitude carries delta = sqrt(2) beta + 2^-22 M.  From these:
    mag_l1      mean(sqrt(2) (beta_e + beta_t)) + 2^-22 term
    complex_l1  the same: a and b each carry beta_e + beta_t, the modulus sqrt(2) times that, plus its own rounding
    log_mag_l1  mean(delta_e / (Me + e - delta_e) + delta_t / (Mt + e - delta_t)) -- log's slope at the near end of the interval --
                plus the fp32 evaluation itself: mean(2^-21 (|log(Me + e)| + |log(Mt + e)|)) + 2^-22 (logf, the two additions of
                e, one subtraction)
    sc          per source (||delta_e + delta_t||_2 + SC_s ||delta_t||_2) / sqrt(N_s + sc_eps) + 1e-6 SC_s -- the triangle
                inequality on sqrt(D_s) and on sqrt(N_s + sc_eps) -- then the mean over s
L_j carries the term-weighted sum, the total the weighted sum over the resolutions plus the MSE's 1e-6 relative.  The cases keep
delta <= log_eps / 4 (log_eps 1e-3 at n_fft 64, 1.0 at n_fft 1024), so the log bound is finite and not vacuous.  The gradient is
compared as there: at the signs the GPU took, against a second fp32 computation (grad_fp32) as the yardstick, 8 x its error.

The shapes make the per-source sums of sc meet every boundary case: 594 bins per source (below one 1024-bin block), 1386 (a
1024-bin block of the whole array straddles the two sources), 3078 (several blocks per source), three sources inside one block."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mrstft_np as mr  # noqa: E402
import _spectral_np as ora  # noqa: E402
from _observed import record  # noqa: E402
from _unaligned import _offset_copy  # noqa: E402

import wave_u_net_amd as wun  # noqa: E402
from wave_u_net_amd import _lib, spectral, training  # noqa: E402

pytestmark = pytest.mark.gpu

SQRT2 = np.sqrt(2.0)
T_SMALL = 64 + 2 * 48 + 5
CASES = {   # name -> (S, B, C, Tout, resolutions, weights, log_eps)
    "64_48": (2, 3, 2, T_SMALL, [(64, 48)], [1.0], 1e-3),                         # 594 bins per source
    "64_16": (2, 3, 2, T_SMALL, [(64, 16)], [1.0], 1e-3),                         # 1386 bins per source
    "1024_768": (2, 2, 1, 1024 + 2 * 768 + 3, [(1024, 768)], [1.0], 1.0),         # 3078 bins per source
    "two_resolutions": (2, 3, 2, T_SMALL, [(64, 48), (64, 16)], [1.0, 0.5], 1e-3),
    "three_sources": (3, 3, 1, T_SMALL, [(64, 48)], [1.0], 1e-3),                 # 297 bins per source: three in one block
}
MSE_W = 0.25
SC_EPS = 1.0
ALL = {"mag_l1": 0.7, "log_mag_l1": 0.4, "sc": 1.3, "complex_l1": 0.6}
TERM_SETS = {"mag_l1": {"mag_l1": 1.0}, "log_mag_l1": {"log_mag_l1": 1.0}, "sc": {"sc": 1.0}, "complex_l1": {"complex_l1": 1.0},
             "sc_log": {"sc": 1.0, "log_mag_l1": 1.0}, "all": ALL}
_CACHE = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def _f32(x):
    """The float the entry receives (wun_spectral_terms holds floats), as a Python float."""
    return float(np.float32(x))


def _case(name):
    """Inputs of a case and what depends on them alone, computed once."""
    if name not in _CACHE:
        S, B, C, T, res, w, le = CASES[name]
        rng = np.random.RandomState(2000 + sorted(CASES).index(name))
        out = rng.randn(S, B, T, C).astype(np.float32)
        tgt = rng.randn(S, B, T, C).astype(np.float32)
        _CACHE[name] = {"out": out, "tgt": tgt, "res": res, "w": w, "log_eps": le, "S": S, "oracle": {}, "gpu_mags": None}
    return _CACHE[name]


def _oracle(ref, tname, signs=None):
    """(losses, gradient) of the float64 oracle for a term set; without pinned signs computed once per case."""
    args = (ref["out"], ref["tgt"], ref["res"], ref["w"], MSE_W, TERM_SETS[tname], _f32(ref["log_eps"]), SC_EPS)
    if signs is not None:
        return mr.loss_and_grad(*args, signs=signs)
    if tname not in ref["oracle"]:
        ref["oracle"][tname] = mr.loss_and_grad(*args)
    return ref["oracle"][tname]


def _loss(ref, terms, mse_w=MSE_W, sc_eps=SC_EPS):
    return spectral.SpectralLoss(ref["res"], ref["w"], mse_w, terms=terms, log_eps=ref["log_eps"], sc_eps=sc_eps)


def _dev(ref):
    return torch.from_numpy(ref["out"]).cuda(), torch.from_numpy(ref["tgt"]).cuda()


def _gpu_mags(ref):
    """Per resolution (Me, Mt) float32 [R, F, K] as spectral.stft_magnitude returns them."""
    if ref["gpu_mags"] is None:
        out, tgt = _dev(ref)
        mags = []
        for n_fft, hop in ref["res"]:
            pair = []
            for x in (out, tgt):
                m = spectral.stft_magnitude(x, n_fft, hop)
                pair.append(m.reshape(-1, m.shape[3], m.shape[4]).cpu().numpy())
            mags.append(tuple(pair))
        ref["gpu_mags"] = mags
    return ref["gpu_mags"]


def _log_rounding(me, mt, e):
    """The fp32 evaluation of the log term on given magnitudes: logf, the additions of e, one subtraction."""
    me, mt = np.asarray(me, np.float64), np.asarray(mt, np.float64)
    return (2.0 ** -21 * (np.abs(np.log(me + e)) + np.abs(np.log(mt + e)))).mean() + 2.0 ** -22


def term_bounds(out, tgt, n_fft, hop, S, log_eps, sc_eps):
    """[mag_l1, log_mag_l1, sc, complex_l1] bounds of one resolution (the module docstring), from float64 audio."""
    re, im = ora.stft(ora.rows(out), n_fft, hop)
    tre, tim = ora.stft(ora.rows(tgt), n_fft, hop)
    me, mt = np.sqrt(re * re + im * im), np.sqrt(tre * tre + tim * tim)
    be, bt = ora.beta(out, n_fft, hop)[:, :, None], ora.beta(tgt, n_fft, hop)[:, :, None]
    de, dt = SQRT2 * be + 2.0 ** -22 * me, SQRT2 * bt + 2.0 ** -22 * mt
    assert max(de.max(), dt.max()) <= log_eps / 4, (de.max(), dt.max(), log_eps)        # the log bound is not vacuous
    mag, lg, sc, scs = mr.mag_terms(me, mt, S, log_eps, sc_eps)
    cx = np.sqrt((re - tre) ** 2 + (im - tim) ** 2).mean()
    b_mag = SQRT2 * (be.mean() + bt.mean()) + 2.0 ** -22 * mag
    b_cx = SQRT2 * (be.mean() + bt.mean()) + 2.0 ** -22 * cx
    b_log = (de / (me + log_eps - de) + dt / (mt + log_eps - dt)).mean() + _log_rounding(me, mt, log_eps)
    _, N = mr.source_sums(me, mt, S)
    n_sum = np.sqrt(((de + dt) ** 2).reshape(S, -1).sum(1))
    n_t = np.sqrt((dt ** 2).reshape(S, -1).sum(1))
    b_scs = (n_sum + scs * n_t) / np.sqrt(N + sc_eps) + 1e-6 * scs
    return np.array([b_mag, b_log, b_scs.mean(), b_cx]), b_scs, scs


def loss_bounds(out, tgt, res, weights, mse_w, terms, log_eps, sc_eps, mse):
    """Bounds of the whole losses vector [2 + 5 nres]."""
    S, nres, tw = out.shape[0], len(res), mr.term_weights(terms)
    b = np.zeros(2 + 5 * nres)
    b[1] = 1e-6 * mse
    b[0] = mse_w * b[1]
    for j, (n_fft, hop) in enumerate(res):
        tb, _, _ = term_bounds(out, tgt, n_fft, hop, S, log_eps, sc_eps)
        tb = np.where(np.array(tw) > 0, tb, 0.0)
        b[2 + nres + 4 * j:2 + nres + 4 * j + 4] = tb
        b[2 + j] = float(np.dot(tw, tb))
        b[0] += weights[j] * b[2 + j]
    return b


def _slot_names(nres):
    return ["total", "MSE"] + ["L_%d" % j for j in range(nres)] + ["%s_%d" % (t, j) for j in range(nres) for t in mr.TERMS]


# ---------------------------------------------------------------------------------------------------- 1. the old entry's bits
@pytest.mark.parametrize("name", sorted(CASES))
def test_mag_l1_alone_is_the_old_entry(lib, name, monkeypatch):
    ref = _case(name)
    out, tgt = _dev(ref)
    nres = len(ref["res"])
    old = spectral.SpectralLoss(ref["res"], ref["w"], MSE_W)
    l0, g0 = old.loss_and_grad(out, tgt)
    assert l0.shape == (2 + nres,)
    for terms in ({"mag_l1": 1.0}, {"mag_l1": 1, "sc": 0}):
        l1, g1 = _loss(ref, terms).loss_and_grad(out, tgt)
        assert l1.shape == (2 + 5 * nres,)
        assert torch.equal(l1[:2 + nres], l0) and torch.equal(g1, g0)
        assert g1.view(torch.int32).eq(g0.view(torch.int32)).all()                  # (bit for bit: the sign of a zero too)
        per = l1[2 + nres:].view(nres, 4)
        assert torch.equal(per[:, 0], l0[2:]) and bool((per[:, 1:] == 0).all())
    # terms=None still calls the old entry: the new one is not reached
    def boom(*a):
        raise AssertionError("terms=None must use wun_spectral_loss")
    monkeypatch.setattr(lib, "wun_spectral_loss_terms", boom)
    monkeypatch.setattr(lib, "wun_spectral_terms_scratch_floats", boom)
    l2, g2 = spectral.SpectralLoss(ref["res"], ref["w"], MSE_W, terms=None).loss_and_grad(out, tgt)
    assert torch.equal(l2, l0) and torch.equal(g2, g0)


# ---------------------------------------------------------------------------------------------------- 2. the device's magnitudes
@pytest.mark.parametrize("name", sorted(CASES))
def test_terms_at_the_devices_magnitudes(lib, name):
    """log_mag_l1 and sc are functions of the floats stft_magnitude returns: float64 formulas on those floats."""
    ref = _case(name)
    out, tgt = _dev(ref)
    loss = _loss(ref, TERM_SETS["sc_log"])
    losses, _ = loss.loss_and_grad(out, tgt, grad=False)
    per = {t: v.cpu().numpy().astype(np.float64) for t, v in loss.term_losses(losses).items()}
    e = _f32(ref["log_eps"])
    for j, (me, mt) in enumerate(_gpu_mags(ref)):
        _, lg, sc, _ = mr.mag_terms(me, mt, ref["S"], e, SC_EPS)
        tol = _log_rounding(me, mt, e) + 2.0 ** -24 * lg                            # (and the slot's own rounding to fp32)
        tag = "mrstft::test_terms_at_the_devices_magnitudes[%s]" % name
        record(tag, "log_mag_l1_%d err / bound" % j, abs(per["log_mag_l1"][j] - lg) / tol, 1.0)
        record(tag, "sc_%d relative" % j, abs(per["sc"][j] - sc) / sc, 1e-6)
        assert abs(per["log_mag_l1"][j] - lg) <= tol
        assert abs(per["sc"][j] - sc) <= 1e-6 * sc
        assert per["mag_l1"][j] == 0 and per["complex_l1"][j] == 0                  # not computed, reported as 0


# ---------------------------------------------------------------------------------------------------- 3. the float64 oracle
@pytest.mark.parametrize("tname", ["sc_log", "all"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_losses_against_float64(lib, name, tname):
    ref = _case(name)
    out, tgt = _dev(ref)
    losses, _ = _loss(ref, TERM_SETS[tname]).loss_and_grad(out, tgt)
    got = losses.cpu().numpy().astype(np.float64)
    want, _ = _oracle(ref, tname)
    e = _f32(ref["log_eps"])
    tol = loss_bounds(ref["out"].astype(np.float64), ref["tgt"].astype(np.float64), ref["res"], ref["w"], MSE_W, TERM_SETS[tname],
                      e, SC_EPS, want[1])
    assert got.shape == want.shape and np.isfinite(got).all()
    for i, what in enumerate(_slot_names(len(ref["res"]))):
        if tol[i] == 0.0:
            assert got[i] == 0.0 and want[i] == 0.0, what                           # a term that is not in the set
            continue
        record("mrstft::test_losses_against_float64[%s-%s]" % (name, tname), "%s err / bound" % what, abs(got[i] - want[i]) / tol[i], 1.0)
        assert abs(got[i] - want[i]) <= tol[i], (what, got[i], want[i], tol[i])


# ---------------------------------------------------------------------------------------------------- 4. gradient, signs pinned
def _pinned_signs(ref, tag):
    """sgn(Me - Mt) of the device's magnitudes; it may differ from float64's only where the magnitudes tie within their bounds."""
    signs = []
    for j, ((n_fft, hop), (me, mt)) in enumerate(zip(ref["res"], _gpu_mags(ref))):
        sg = np.sign(me - mt).astype(np.float64)
        m_e, m_t = ora.magnitude(ref["out"], n_fft, hop), ora.magnitude(ref["tgt"], n_fft, hop)
        d64 = m_e - m_t
        tie = np.abs(d64) <= (SQRT2 * (ora.beta(ref["out"], n_fft, hop) + ora.beta(ref["tgt"], n_fft, hop))[:, :, None]
                              + 2.0 ** -22 * (m_e + m_t))
        flipped = sg != np.sign(d64)
        record(tag, "signs differing from float64 (count)", flipped.sum(), sg.size)
        assert not (flipped & ~tie).any()
        signs.append(sg)
    return signs


def _check_gradient(tag, ref, tname, d_out, signs, mse_w=MSE_W, out=None):
    o = ref["out"] if out is None else out
    args = (o, ref["tgt"], ref["res"], ref["w"], mse_w, TERM_SETS[tname], _f32(ref["log_eps"]), SC_EPS)
    _, g64 = mr.loss_and_grad(*args, signs=signs)
    g32 = mr.grad_fp32(*args, signs)
    scale = np.abs(g64).max()
    e32 = np.abs(g32.astype(np.float64) - g64).max() / scale
    egpu = np.abs(d_out.cpu().numpy().astype(np.float64) - g64).max() / scale
    record(tag, "cpu fp32 e32", e32, 1.0)
    record(tag, "gpu err / max |g64|", egpu, 8 * e32)
    assert scale > 0 and egpu <= 8 * e32, (egpu, e32)


@pytest.mark.parametrize("tname", sorted(TERM_SETS))
@pytest.mark.parametrize("name", sorted(CASES))
def test_gradient_with_pinned_signs(lib, name, tname):
    ref = _case(name)
    tag = "mrstft::test_gradient_with_pinned_signs[%s-%s]" % (name, tname)
    signs = _pinned_signs(ref, tag)
    out, tgt = _dev(ref)
    loss = _loss(ref, TERM_SETS[tname])
    l0, d_out = loss.loss_and_grad(out, tgt)
    assert torch.isfinite(d_out).all()
    _check_gradient(tag, ref, tname, d_out, signs)
    if name == "two_resolutions" and tname == "all":
        # every pointer 4 bytes off an 8-byte boundary: the same bits
        o1, t1 = _offset_copy(out), _offset_copy(tgt)
        g1 = torch.empty(out.numel() + 1, dtype=torch.float32, device="cuda")[1:].view(out.shape)
        scratch = torch.empty(loss.scratch_floats(out.shape) + 1, dtype=torch.float32, device="cuda")[1:]
        l1 = torch.empty(loss.num_losses + 1, dtype=torch.float32, device="cuda")[1:]
        assert all(t.data_ptr() % 8 == 4 for t in (o1, t1, g1, scratch, l1))
        loss.run(o1, t1, g1, l1, scratch)
        assert torch.equal(g1, d_out) and torch.equal(l1, l0)


# ---------------------------------------------------------------------------------------------------- 5. exact and edge cases
@pytest.mark.parametrize("name", ["64_16", "1024_768", "two_resolutions"])
def test_exact_cases(lib, name):
    ref = _case(name)
    out, tgt = _dev(ref)
    # estimates bit-equal to the targets: every slot and the gradient exactly 0, for all four terms
    losses, g = _loss(ref, ALL, 1.0).loss_and_grad(tgt.clone(), tgt)
    assert bool((losses == 0).all()) and bool((g == 0).all())
    # zero estimates without complex_l1 and without the MSE: every coefficient has Me == 0
    losses, g = _loss(ref, {"mag_l1": 1, "log_mag_l1": 1, "sc": 1}, 0.0).loss_and_grad(torch.zeros_like(tgt), tgt)
    assert torch.isfinite(losses).all() and bool((g == 0).all())
    # ... with complex_l1 alone the gradient is -T / |T|: not zero, and as good as check 4 asks
    losses, g = _loss(ref, TERM_SETS["complex_l1"], 0.0).loss_and_grad(torch.zeros_like(tgt), tgt)
    assert torch.isfinite(losses).all() and bool((g != 0).any())
    zsigns = [-np.ones_like(me, dtype=np.float64) for me, _ in _gpu_mags(ref)]      # (complex_l1 takes no sign)
    _check_gradient("mrstft::test_exact_cases[%s] zero estimates, complex_l1" % name, ref, "complex_l1", g, zsigns, mse_w=0.0,
                    out=np.zeros_like(ref["out"]))
    # samples behind the last frame hold exactly the MSE term
    loss = _loss(ref, ALL, 0.5)
    losses, g = loss.loss_and_grad(out, tgt)
    covered = max(n + (ora.num_frames(out.shape[2], n, h) - 1) * h for n, h in ref["res"])
    cm = np.float32(np.float64(np.float32(0.5)) * 2.0 / out.numel())
    assert covered < out.shape[2] and torch.equal(g[:, :, covered:], (out - tgt)[:, :, covered:] * float(cm))
    assert not torch.equal(g[:, :, :covered], (out - tgt)[:, :, :covered] * float(cm))
    # d_outputs = NULL leaves the same losses
    l2, none = loss.loss_and_grad(out, tgt, grad=False)
    assert none is None and torch.equal(l2, losses)


@pytest.mark.parametrize("name", ["64_48", "64_16", "1024_768"])
def test_a_silent_source(lib, name):
    """The targets of source 0 all zero (N_0 == 0): everything finite, SC_0 = sqrt(D_0 / sc_eps).  The per-source values are
    read through runs with S = 1 on one source alone (the losses hold only the mean over the sources): source 1's sums -- and so
    its coefficients -- do not depend on source 0 being there, so its gradient is, bit for bit, HALF its gradient alone (every
    mean's 1 / S, a power of two), and the sc slot is the mean of the two sources' own."""
    ref = _case(name)
    out, tgt = _dev(ref)
    tgt = tgt.clone()
    tgt[0] = 0.0
    sc_eps = 0.5
    e = _f32(ref["log_eps"])
    loss = _loss(ref, ALL, MSE_W, sc_eps=sc_eps)
    losses, g = loss.loss_and_grad(out, tgt)
    assert torch.isfinite(losses).all() and torch.isfinite(g).all()
    alone = [loss.loss_and_grad(out[s:s + 1], tgt[s:s + 1]) for s in (0, 1)]
    assert torch.equal(g[1:2], alone[1][1] * 0.5)
    assert torch.equal(g[0:1], alone[0][1] * 0.5)
    sc2 = loss.term_losses(losses)["sc"].cpu().numpy().astype(np.float64)
    sc1 = [loss.term_losses(l)["sc"].cpu().numpy().astype(np.float64) for l, _ in alone]
    o64, t64 = ref["out"].astype(np.float64), ref["tgt"].astype(np.float64).copy()
    t64[0] = 0.0
    for j, (n_fft, hop) in enumerate(ref["res"]):
        assert abs(sc2[j] - 0.5 * (sc1[0][j] + sc1[1][j])) <= 2.0 ** -22 * sc2[j]   # three roundings to fp32
        _, b_scs, scs = term_bounds(o64, t64, n_fft, hop, 2, e, sc_eps)
        me0 = ora.magnitude(o64[0:1], n_fft, hop)
        assert abs(scs[0] - np.sqrt((me0 ** 2).sum() / sc_eps)) <= 1e-12 * scs[0]   # the oracle's own SC_0
        for s in (0, 1):
            record("mrstft::test_a_silent_source[%s]" % name, "SC_%d (res %d) err / bound" % (s, j), abs(sc1[s][j] - scs[s]) / b_scs[s], 1.0)
            assert abs(sc1[s][j] - scs[s]) <= b_scs[s]


# ---------------------------------------------------------------------------------------------------- 6. reproducibility
@pytest.mark.parametrize("name", ["64_16", "1024_768", "two_resolutions", "three_sources"])
def test_reproducible_bits(lib, name):
    ref = _case(name)
    out, tgt = _dev(ref)
    loss = _loss(ref, ALL)
    l0, g0 = loss.loss_and_grad(out, tgt)
    l1, g1 = loss.loss_and_grad(out, tgt)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    for fill in (float("nan"), 0.0):
        scratch = torch.full((loss.scratch_floats(out.shape),), fill, dtype=torch.float32, device="cuda")
        g2, l2 = torch.full_like(out, float("nan")), torch.full_like(l0, float("nan"))
        loss.run(out, tgt, g2, l2, scratch)
        assert torch.equal(l0, l2) and torch.equal(g0, g2)


# ---------------------------------------------------------------------------------------------------- 7. through the layers
def test_autograd_wrapper(lib):
    ref = _case("two_resolutions")
    out, tgt = _dev(ref)
    out.requires_grad_(True)
    loss = _loss(ref, ALL)
    l0, g0 = loss.loss_and_grad(out.detach(), tgt)
    total = spectral.stft_l1(out, tgt, loss)
    (3.0 * total).backward()
    assert total.item() == l0[0].item() and torch.equal(out.grad, g0 * 3.0)
    assert loss(out.detach(), tgt).item() == l0[0].item()


_E2E_RES = [(64, 48)]
_E2E_TERMS = {"sc": 1, "log_mag_l1": 1}
_E2E_SPEC = {"resolutions": [[64, 48]], "mse_weight": 1.0, "terms": _E2E_TERMS, "log_eps": 1e-3}


def _e2e_cfg(tmp, **over):
    return wun.get_config("full", num_layers=3, num_initial_filters=8, num_frames=200, batch_size=4, epoch_it=3,
                          model_base_dir=os.path.join(tmp, "ckpt"), log_dir=os.path.join(tmp, "logs"),
                          init_sup_sep_lr=1e-3, **over)


def _oracle_parts(cfg, sep, mix, targets):
    """[total, MSE, spectral, sc, log_mag_l1] of _E2E_SPEC and their bounds, from the float64 oracle forward on the
    separator's weights."""
    from oracle import waveunet_torch as wt
    names = [n for n, _, _ in sep._active.tensors]
    v = sep.variables()
    tp = [(n, v[n].detach().cpu().double()) for n in names]
    o = wt.get_output(cfg, tp, mix.cpu().double(), True)
    out = torch.stack([o[n] for n in cfg["source_names"]]).numpy()
    tgt = targets.cpu().numpy().astype(np.float64)
    e = _f32(1e-3)
    l, _ = mr.loss_and_grad(out, tgt, _E2E_RES, [1.0], 1.0, _E2E_TERMS, e, 1.0)
    b = loss_bounds(out, tgt, _E2E_RES, [1.0], 1.0, _E2E_TERMS, e, 1.0, l[1])
    return np.array([l[0], l[1], l[2], l[5], l[4]]), np.array([b[0], b[1], b[2], b[5], b[4]])


def _check_logged(tag, tr, first, want, tol):
    mse, spec = tr.loss_parts()
    parts = tr.term_parts()
    got = (first, mse, spec, parts["sc"], parts["log_mag_l1"])
    for i, what in enumerate(("total", "mse", "spectral", "sc", "log_mag_l1")):
        record(tag, "%s err / bound" % what, abs(got[i] - want[i]) / tol[i], 1.0)
        assert abs(got[i] - want[i]) <= tol[i], (what, got[i], want[i], tol[i])
    assert parts["mag_l1"] == 0 and parts["complex_l1"] == 0


def test_trainer_end_to_end(lib, tmp_path, monkeypatch):
    monkeypatch.setenv("WUN_NO_TUNE", "1")
    cfg = _e2e_cfg(str(tmp_path))
    tr = training.Trainer(cfg, spectral_loss=_E2E_SPEC)
    assert tr.t_out >= 64 + 48 and tr.spectral.terms["sc"] == 1.0 and tr.spectral.num_losses == 7
    mix, targets = training.synthetic_source(cfg, tr.batch, tr.t_in, tr.t_out, tr.device)()
    want, tol = _oracle_parts(cfg, tr.sep, mix, targets)
    first = tr.step(mix, targets).item()
    assert tr.last_losses.shape == (7,)
    _check_logged("mrstft::test_trainer_end_to_end", tr, first, want, tol)
    for _ in range(19):
        last = tr.step(mix, targets).item()
    assert np.isfinite(last) and last < first and tr.sep.global_step == 20

    # gradient accumulation: the first step's loss is the mean of the two micro-batches' losses
    ta = training.Trainer(cfg, spectral_loss=_E2E_SPEC, grad_accum_steps=2)
    halves = [_oracle_parts(cfg, ta.sep, mix[lo:lo + 2], targets[:, lo:lo + 2]) for lo in (0, 2)]
    first = ta.step(mix, targets).item()
    _check_logged("mrstft::test_trainer_end_to_end[accum2]", ta, first, (halves[0][0] + halves[1][0]) / 2, (halves[0][1] + halves[1][1]) / 2)


def test_train_log_carries_the_terms(lib, tmp_path, monkeypatch):
    monkeypatch.setenv("WUN_NO_TUNE", "1")
    training.train(_e2e_cfg(str(tmp_path), spectral_loss=_E2E_SPEC), "terms")
    log = [json.loads(l) for l in open(os.path.join(str(tmp_path), "logs", "terms", "train.jsonl"))]
    assert len(log) == 3
    for line in log:
        parts = line["spectral_terms"]
        assert sorted(parts) == sorted(spectral.TERMS) and parts["sc"] > 0 and parts["log_mag_l1"] > 0
        assert abs(sum(parts.values()) - line["spectral_loss"]) <= 1e-6 * line["spectral_loss"]
        assert abs(line["sep_loss"] - (line["mse_loss"] + line["spectral_loss"])) <= 1e-6 * line["sep_loss"]
    # a run without `terms` has no such key
    training.train(_e2e_cfg(str(tmp_path), spectral_loss={"resolutions": [[64, 48]], "mse_weight": 1.0}), "one_term")
    old = [json.loads(l) for l in open(os.path.join(str(tmp_path), "logs", "one_term", "train.jsonl"))]
    assert len(old) == 3 and all("spectral_terms" not in line and "spectral_loss" in line for line in old)
