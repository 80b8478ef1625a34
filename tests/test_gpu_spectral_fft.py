"""GPU tests of the spectral loss's FFT path (include/wun.h: wun_stft_magnitude_fft, wun_spectral_loss_fft,
wun_spectral_loss_terms_fft; spectral.SpectralLoss(transform="fft")) against the float64 oracle
tests/_mrstft_fft_np.py, which holds the cases too.

The bounds are tests/test_gpu_mrstft.py's (term_bounds, loss_bounds, imported): beta[r][f] = n_fft 2^-24 sum_n |w[n] x[f hop + n]|
bounds the error of Re and of Im of ANY float32 evaluation of the n_fft-term sums, whatever its order -- an FFT's included -- and a
magnitude carries delta = sqrt(2) beta + 2^-22 M.  The gradient is compared as there: at the signs the device took, against a
second float32 computation (grad_fp32_fft: scipy's float32 FFTs) as the yardstick, 8 x its error.

    case             S, B, C   T       log_eps   reaches
    64_16            2, 3, 2   165     1e-3      84 frame rows: three 32-frame workgroups, the last part-filled; radix-2 last stage
    64_48            2, 3, 2   165     1e-3      few frames per row
    512_128          2, 1, 2   771     2^-4      4 frames per workgroup, pure radix 4
    1024_768         2, 2, 1   2563    2^-2      the reference's resolution; 2 frames per workgroup
    2048_512         2, 1, 1   3077    1         one frame per workgroup
    4096_1024        2, 1, 2   6149    4         2 butterflies per lane, radix-2 last stage
    8192_2048        2, 1, 1   12293   16        4 butterflies per lane, 64 KB of LDS
    two_resolutions  2, 3, 2   6149    4         64 / 48 and 4096 / 1024, weights 1 and 0.5: two kernel forms in one call
    three_sources    3, 3, 1   165     1e-3      three sources in one 1024-bin block

log_eps is the smallest power of two (1e-3 at n_fft 64) for which term_bounds' own assertion delta <= log_eps / 4 holds on the
case's randn audio: max delta is 1.8e-4, 9.6e-3, 3.7e-2, 0.147, 0.578 and 2.29 at n_fft 64 .. 8192
(tests/test_spectral_fft_host.py::test_log_eps_of_the_cases recomputes it without a GPU)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mrstft_fft_np as fo  # noqa: E402
import _spectral_np as ora  # noqa: E402
from _observed import record  # noqa: E402
from _unaligned import _offset_copy  # noqa: E402
from test_gpu_mrstft import ALL, MSE_W, SC_EPS, TERM_SETS, _e2e_cfg, _f32, _log_rounding, _slot_names, loss_bounds  # noqa: E402

import wave_u_net_amd as wun  # noqa: E402,F401
from wave_u_net_amd import _lib, spectral, training  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = fo.CASES
SMALL = [n for n in sorted(CASES) if max(r[0] for r in CASES[n][4]) <= 2048]       # the cases the GEMM entries accept
EXACT = ["64_16", "4096_1024", "two_resolutions"]
SQRT2 = np.sqrt(2.0)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def _oracle(ref, tname):
    """(losses, gradient) of the float64 oracle for a term set with float64's own signs, computed once per case."""
    if tname not in ref["oracle"]:
        ref["oracle"][tname] = fo.loss_and_grad(ref["out"], ref["tgt"], ref["res"], ref["w"], MSE_W, TERM_SETS[tname],
                                                _f32(ref["log_eps"]), SC_EPS)
    return ref["oracle"][tname]


def _loss(ref, terms, mse_w=MSE_W, sc_eps=SC_EPS, transform="fft"):
    return spectral.SpectralLoss(ref["res"], ref["w"], mse_w, terms=terms, log_eps=ref["log_eps"], sc_eps=sc_eps, transform=transform)


def _dev(ref):
    return torch.from_numpy(ref["out"]).cuda(), torch.from_numpy(ref["tgt"]).cuda()


def _gpu_mags(ref):
    """Per resolution (Me, Mt) float32 [R, F, K] as spectral.stft_magnitude(transform="fft") returns them."""
    if ref["gpu_mags"] is None:
        out, tgt = _dev(ref)
        mags = []
        for n_fft, hop in ref["res"]:
            pair = []
            for x in (out, tgt):
                m = spectral.stft_magnitude(x, n_fft, hop, transform="fft")
                pair.append(m.reshape(-1, m.shape[3], m.shape[4]).cpu().numpy())
            mags.append(tuple(pair))
        ref["gpu_mags"] = mags
    return ref["gpu_mags"]


def _bounds(ref, terms, want_mse, mse_w=MSE_W):
    return loss_bounds(ref["out"].astype(np.float64), ref["tgt"].astype(np.float64), ref["res"], ref["w"], mse_w, terms,
                       _f32(ref["log_eps"]), SC_EPS, want_mse)


# ---------------------------------------------------------------------------------------------------- 1. magnitudes
@pytest.mark.parametrize("name", sorted(CASES))
def test_magnitudes_against_float64(lib, name):
    ref = fo.case(name)
    for j, ((n_fft, hop), pair) in enumerate(zip(ref["res"], _gpu_mags(ref))):
        for what, x, got in (("estimates", ref["out"], pair[0]), ("targets", ref["tgt"], pair[1])):
            x64 = x.astype(np.float64)
            want = ora.magnitude(x64, n_fft, hop)
            assert got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all()
            tol = fo.magnitude_bound(x64, n_fft, hop, want)
            ratio = (np.abs(got.astype(np.float64) - want) / tol).max()
            record("spectral_fft::test_magnitudes_against_float64[%s]" % name, "%s res %d err / bound" % (what, j), ratio, 1.0)
            assert ratio <= 1.0


# ---------------------------------------------------------------------------------------------------- 2. losses
@pytest.mark.parametrize("tname", ["sc_log", "all"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_losses_against_float64(lib, name, tname):
    ref = fo.case(name)
    out, tgt = _dev(ref)
    losses, _ = _loss(ref, TERM_SETS[tname]).loss_and_grad(out, tgt)
    got = losses.cpu().numpy().astype(np.float64)
    want, _ = _oracle(ref, tname)
    tol = _bounds(ref, TERM_SETS[tname], want[1])
    assert got.shape == want.shape and np.isfinite(got).all()
    tag = "spectral_fft::test_losses_against_float64[%s-%s]" % (name, tname)
    for i, what in enumerate(_slot_names(len(ref["res"]))):
        if tol[i] == 0.0:
            assert got[i] == 0.0 and want[i] == 0.0, what                           # a term that is not in the set
            continue
        record(tag, "%s err / bound" % what, abs(got[i] - want[i]) / tol[i], 1.0)
        assert abs(got[i] - want[i]) <= tol[i], (what, got[i], want[i], tol[i])
    record(tag, "MSE relative", abs(got[1] - want[1]) / want[1], 1e-6)
    assert abs(got[1] - want[1]) <= 1e-6 * want[1]


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_term_losses_against_float64(lib, name):
    """terms=None (wun_spectral_loss_fft): [total, MSE, L_j] against _spectral_np's float64 magnitudes."""
    ref = fo.case(name)
    out, tgt = _dev(ref)
    losses, _ = _loss(ref, None).loss_and_grad(out, tgt)
    got = losses.cpu().numpy().astype(np.float64)
    nres = len(ref["res"])
    o64, t64 = ref["out"].astype(np.float64), ref["tgt"].astype(np.float64)
    want = np.zeros(2 + nres)
    want[1] = np.mean((o64 - t64) ** 2)
    for j, (n_fft, hop) in enumerate(ref["res"]):
        want[2 + j] = np.abs(ora.magnitude(o64, n_fft, hop) - ora.magnitude(t64, n_fft, hop)).mean()
    want[0] = MSE_W * want[1] + float(np.dot(ref["w"], want[2:]))
    tol = _bounds(ref, TERM_SETS["mag_l1"], want[1])[:2 + nres]
    assert got.shape == want.shape
    for i, what in enumerate(_slot_names(nres)[:2 + nres]):
        record("spectral_fft::test_one_term_losses_against_float64[%s]" % name, "%s err / bound" % what, abs(got[i] - want[i]) / tol[i], 1.0)
        assert abs(got[i] - want[i]) <= tol[i], (what, got[i], want[i], tol[i])
    assert abs(got[1] - want[1]) <= 1e-6 * want[1]


# ---------------------------------------------------------------------------------------------------- 3. the device's magnitudes
@pytest.mark.parametrize("name", sorted(CASES))
def test_terms_at_the_devices_magnitudes(lib, name):
    """log_mag_l1 and sc are the float64 formulas on the floats stft_magnitude(transform="fft") returns: the loss and the
    magnitude entry share one forward."""
    ref = fo.case(name)
    out, tgt = _dev(ref)
    loss = _loss(ref, TERM_SETS["sc_log"])
    losses, _ = loss.loss_and_grad(out, tgt, grad=False)
    per = {t: v.cpu().numpy().astype(np.float64) for t, v in loss.term_losses(losses).items()}
    e = _f32(ref["log_eps"])
    for j, (me, mt) in enumerate(_gpu_mags(ref)):
        _, lg, sc, _ = fo.mag_terms(me, mt, ref["S"], e, SC_EPS)
        tol = _log_rounding(me, mt, e) + 2.0 ** -24 * lg                            # (and the slot's own rounding to fp32)
        tag = "spectral_fft::test_terms_at_the_devices_magnitudes[%s]" % name
        record(tag, "log_mag_l1_%d err / bound" % j, abs(per["log_mag_l1"][j] - lg) / tol, 1.0)
        record(tag, "sc_%d relative" % j, abs(per["sc"][j] - sc) / sc, 1e-6)
        assert abs(per["log_mag_l1"][j] - lg) <= tol
        assert abs(per["sc"][j] - sc) <= 1e-6 * sc
        assert per["mag_l1"][j] == 0 and per["complex_l1"][j] == 0                  # not computed, reported as 0


# ---------------------------------------------------------------------------------------------------- 4. gradient, signs pinned
def _pinned_signs(ref, tag):
    """sgn(Me - Mt) of the device's FFT magnitudes; it may differ from float64's only where the magnitudes tie within their bounds."""
    signs = []
    for (n_fft, hop), (me, mt) in zip(ref["res"], _gpu_mags(ref)):
        sg = np.sign(me - mt).astype(np.float64)
        d64, tie = fo.tie(ref["out"].astype(np.float64), ref["tgt"].astype(np.float64), n_fft, hop)
        flipped = sg != np.sign(d64)
        record(tag, "signs differing from float64 (count)", flipped.sum(), sg.size)
        assert not (flipped & ~tie).any()
        signs.append(sg)
    return signs


def _check_gradient(tag, ref, tname, d_out, signs, mse_w=MSE_W):
    args = (ref["out"], ref["tgt"], ref["res"], ref["w"], mse_w, TERM_SETS[tname], _f32(ref["log_eps"]), SC_EPS)
    _, g64 = fo.loss_and_grad(*args, signs=signs)
    g32 = fo.grad_fp32_fft(*args, signs)
    scale = np.abs(g64).max()
    e32 = np.abs(g32.astype(np.float64) - g64).max() / scale
    egpu = np.abs(d_out.cpu().numpy().astype(np.float64) - g64).max() / scale
    record(tag, "cpu fp32 e32", e32, 1.0)
    record(tag, "gpu err / max |g64|", egpu, 8 * e32)
    assert scale > 0 and egpu <= 8 * e32, (egpu, e32)


@pytest.mark.parametrize("tname", sorted(TERM_SETS))
@pytest.mark.parametrize("name", sorted(CASES))
def test_gradient_with_pinned_signs(lib, name, tname):
    ref = fo.case(name)
    tag = "spectral_fft::test_gradient_with_pinned_signs[%s-%s]" % (name, tname)
    signs = _pinned_signs(ref, tag)
    out, tgt = _dev(ref)
    _, d_out = _loss(ref, TERM_SETS[tname]).loss_and_grad(out, tgt)
    assert torch.isfinite(d_out).all()
    _check_gradient(tag, ref, tname, d_out, signs)


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_term_gradient_with_pinned_signs(lib, name):
    """wun_spectral_loss_fft's gradient (terms=None) by the same rule."""
    ref = fo.case(name)
    tag = "spectral_fft::test_one_term_gradient_with_pinned_signs[%s]" % name
    signs = _pinned_signs(ref, tag)
    out, tgt = _dev(ref)
    _, d_out = _loss(ref, None).loss_and_grad(out, tgt)
    _check_gradient(tag, ref, "mag_l1", d_out, signs)


# ---------------------------------------------------------------------------------------------------- 5. against the GEMM path
@pytest.mark.parametrize("name", SMALL)
def test_against_the_gemm_path(lib, name):
    """Both paths lie within the bounds of the same float64 values: their losses differ by at most the sum of both bounds."""
    ref = fo.case(name)
    out, tgt = _dev(ref)
    want, _ = _oracle(ref, "all")
    tol = 2.0 * _bounds(ref, ALL, want[1])
    lf, _ = _loss(ref, ALL).loss_and_grad(out, tgt, grad=False)
    lg, _ = _loss(ref, ALL, transform="gemm").loss_and_grad(out, tgt, grad=False)
    lf, lg = lf.cpu().numpy().astype(np.float64), lg.cpu().numpy().astype(np.float64)
    for i, what in enumerate(_slot_names(len(ref["res"]))):
        record("spectral_fft::test_against_the_gemm_path[%s]" % name, "%s |fft - gemm| / bound" % what, abs(lf[i] - lg[i]) / tol[i], 1.0)
        assert abs(lf[i] - lg[i]) <= tol[i], (what, lf[i], lg[i], tol[i])
    f1, _ = _loss(ref, None).loss_and_grad(out, tgt, grad=False)
    g1, _ = _loss(ref, None, transform="gemm").loss_and_grad(out, tgt, grad=False)
    nres = len(ref["res"])
    tol1 = 2.0 * _bounds(ref, TERM_SETS["mag_l1"], want[1])[:2 + nres]
    assert bool((torch.abs(f1 - g1).cpu().double() <= torch.from_numpy(tol1)).all())


# ---------------------------------------------------------------------------------------------------- 6. exact and edge cases
@pytest.mark.parametrize("name", EXACT)
def test_exact_cases(lib, name):
    ref = fo.case(name)
    out, tgt = _dev(ref)
    nres = len(ref["res"])
    # estimates bit-equal to the targets: every slot and the gradient exactly 0, for all four terms and for the one-term entry
    for terms in (ALL, None):
        losses, g = _loss(ref, terms, 1.0).loss_and_grad(tgt.clone(), tgt)
        assert bool((losses == 0).all()) and bool((g == 0).all())
    # zero estimates without complex_l1 and without the MSE: every coefficient has Me == 0
    losses, g = _loss(ref, {"mag_l1": 1, "log_mag_l1": 1, "sc": 1}, 0.0).loss_and_grad(torch.zeros_like(tgt), tgt)
    assert torch.isfinite(losses).all() and bool((g == 0).all())
    losses, g = _loss(ref, None, 0.0).loss_and_grad(torch.zeros_like(tgt), tgt)
    assert torch.isfinite(losses).all() and bool((g == 0).all())
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
    # mag_l1 alone through wun_spectral_loss_terms_fft: wun_spectral_loss_fft's bits in the shared slots and the gradient
    l0, g0 = _loss(ref, None).loss_and_grad(out, tgt)
    for terms in ({"mag_l1": 1.0}, {"mag_l1": 1, "sc": 0}):
        l1, g1 = _loss(ref, terms).loss_and_grad(out, tgt)
        assert l0.shape == (2 + nres,) and l1.shape == (2 + 5 * nres,)
        assert torch.equal(l1[:2 + nres], l0) and g1.view(torch.int32).eq(g0.view(torch.int32)).all()
        per = l1[2 + nres:].view(nres, 4)
        assert torch.equal(per[:, 0], l0[2:]) and bool((per[:, 1:] == 0).all())


@pytest.mark.parametrize("name", EXACT)
def test_a_silent_source(lib, name):
    """tests/test_gpu_mrstft.py::test_a_silent_source's identity on the FFT path: with the targets of source 0 all zero, either
    source's gradient inside the S = 2 call is, bit for bit, HALF its gradient alone (every mean's 1 / S, a power of two): a
    source's sums, coefficients and frame gradients do not depend on the other source being there."""
    ref = fo.case(name)
    out, tgt = _dev(ref)
    tgt = tgt.clone()
    tgt[0] = 0.0
    loss = _loss(ref, ALL, MSE_W, sc_eps=0.5)
    losses, g = loss.loss_and_grad(out, tgt)
    assert torch.isfinite(losses).all() and torch.isfinite(g).all()
    alone = [loss.loss_and_grad(out[s:s + 1], tgt[s:s + 1]) for s in (0, 1)]
    assert torch.equal(g[1:2], alone[1][1] * 0.5)
    assert torch.equal(g[0:1], alone[0][1] * 0.5)


# ---------------------------------------------------------------------------------------------------- 7. reproducibility
@pytest.mark.parametrize("terms", [None, ALL], ids=["one_term", "all"])
@pytest.mark.parametrize("name", ["64_16", "1024_768", "4096_1024", "8192_2048", "two_resolutions", "three_sources"])
def test_reproducible_bits(lib, name, terms):
    ref = fo.case(name)
    out, tgt = _dev(ref)
    loss = _loss(ref, terms)
    l0, g0 = loss.loss_and_grad(out, tgt)
    l1, g1 = loss.loss_and_grad(out, tgt)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    for fill in (float("nan"), 0.0):
        scratch = torch.full((loss.scratch_floats(out.shape),), fill, dtype=torch.float32, device="cuda")
        g2, l2 = torch.full_like(out, float("nan")), torch.full_like(l0, float("nan"))
        loss.run(out, tgt, g2, l2, scratch)
        assert torch.equal(l0, l2) and torch.equal(g0, g2)
    # every pointer 4 bytes off an 8-byte boundary: the same bits
    o1, t1 = _offset_copy(out), _offset_copy(tgt)
    g3 = torch.empty(out.numel() + 1, dtype=torch.float32, device="cuda")[1:].view(out.shape)
    scratch = torch.empty(loss.scratch_floats(out.shape) + 1, dtype=torch.float32, device="cuda")[1:]
    l3 = torch.empty(loss.num_losses + 1, dtype=torch.float32, device="cuda")[1:]
    assert all(t.data_ptr() % 8 == 4 for t in (o1, t1, g3, scratch, l3))
    loss.run(o1, t1, g3, l3, scratch)
    assert torch.equal(g3, g0) and torch.equal(l3, l0)
    if terms is None:
        m0 = [spectral.stft_magnitude(out, n, h, transform="fft") for n, h in ref["res"]]
        m1 = [spectral.stft_magnitude(o1, n, h, transform="fft") for n, h in ref["res"]]
        assert all(torch.equal(a, b) for a, b in zip(m0, m1))


# ---------------------------------------------------------------------------------------------------- 8. row independence
@pytest.mark.parametrize("n_fft, hop, T", [(64, 16, fo.T_SMALL), (4096, 1024, 4096 + 2 * 1024 + 5)])
def test_rows_do_not_depend_on_the_batch(lib, n_fft, hop, T):
    """Row r's magnitudes from a B = 3 call are those of a B = 1 call on that row alone, bit for bit.  At 64 / 16 a row has 7
    frames and a workgroup 32: frames of different rows share workgroups, and the same frame sits in different lanes in the two
    calls."""
    x = torch.from_numpy(np.random.RandomState(77).randn(2, 3, T, 2).astype(np.float32)).cuda()
    whole = spectral.stft_magnitude(x, n_fft, hop, transform="fft")
    assert whole.shape[:3] == (2, 3, 2)
    for s in range(2):
        for b in range(3):
            alone = spectral.stft_magnitude(x[s:s + 1, b:b + 1].contiguous(), n_fft, hop, transform="fft")
            assert torch.equal(whole[s:s + 1, b:b + 1], alone), (s, b)


# ---------------------------------------------------------------------------------------------------- 9. through the layers
def test_autograd_wrapper(lib):
    ref = fo.case("two_resolutions")
    out, tgt = _dev(ref)
    out.requires_grad_(True)
    loss = _loss(ref, ALL)
    l0, g0 = loss.loss_and_grad(out.detach(), tgt)
    total = spectral.stft_l1(out, tgt, loss)
    (3.0 * total).backward()
    assert total.item() == l0[0].item() and torch.equal(out.grad, g0 * 3.0)
    assert loss(out.detach(), tgt).item() == l0[0].item()
    # the keyword of stft_l1 itself builds the one-term loss on the chosen transform
    o2 = out.detach().clone().requires_grad_(True)
    t2 = spectral.stft_l1(o2, tgt, resolutions=ref["res"], weights=ref["w"], mse_weight=MSE_W, transform="fft")
    t2.backward()
    l1, g1 = _loss(ref, None).loss_and_grad(out.detach(), tgt)
    assert t2.item() == l1[0].item() and torch.equal(o2.grad, g1)
    with pytest.raises(NotImplementedError):
        spectral.stft_l1(o2, tgt, resolutions=ref["res"], weights=ref["w"])           # "gemm" is the default: 4096 is refused


_E2E_RES = [(64, 48)]
_E2E_TERMS = {"sc": 1, "log_mag_l1": 1}
_E2E_SPEC = {"resolutions": [[64, 48]], "transform": "fft", "terms": _E2E_TERMS, "mse_weight": 1.0, "log_eps": 1e-3}


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
    l, _ = fo.loss_and_grad(out, tgt, _E2E_RES, [1.0], 1.0, _E2E_TERMS, e, 1.0)
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
    assert tr.t_out >= 64 + 48 and tr.spectral.transform == "fft" and tr.spectral.num_losses == 7
    mix, targets = training.synthetic_source(cfg, tr.batch, tr.t_in, tr.t_out, tr.device)()
    want, tol = _oracle_parts(cfg, tr.sep, mix, targets)
    first = tr.step(mix, targets).item()
    assert tr.last_losses.shape == (7,)
    _check_logged("spectral_fft::test_trainer_end_to_end", tr, first, want, tol)
    for _ in range(19):
        last = tr.step(mix, targets).item()
    assert np.isfinite(last) and last < first and tr.sep.global_step == 20

    # gradient accumulation: the first step's loss is the mean of the two micro-batches' losses
    ta = training.Trainer(cfg, spectral_loss=_E2E_SPEC, grad_accum_steps=2)
    halves = [_oracle_parts(cfg, ta.sep, mix[lo:lo + 2], targets[:, lo:lo + 2]) for lo in (0, 2)]
    first = ta.step(mix, targets).item()
    _check_logged("spectral_fft::test_trainer_end_to_end[accum2]", ta, first, (halves[0][0] + halves[1][0]) / 2,
                  (halves[0][1] + halves[1][1]) / 2)


def test_trainer_step_at_4096(lib, tmp_path, monkeypatch):
    """One step against a 4096 / 1024 resolution, through model_config["spectral_loss"]: num_frames 5118 is the smallest that
    get_padding turns into an output of at least 4096 + 1024 frames (5125; 5117 gives 5117)."""
    monkeypatch.setenv("WUN_NO_TUNE", "1")
    spec = {"resolutions": [[4096, 1024]], "transform": "fft", "terms": _E2E_TERMS, "mse_weight": 1.0, "log_eps": 4.0}
    cfg = lambda n, **kw: dict(_e2e_cfg(str(tmp_path)), num_frames=n, **kw)  # noqa: E731
    short = training.Trainer(cfg(5117, spectral_loss=spec))
    assert short.t_out < 4096 + 1024
    tr = training.Trainer(cfg(5118, spectral_loss=spec))
    assert tr.t_out >= 4096 + 1024 and tr.spectral.transform == "fft" and tr.spectral.resolutions == [(4096, 1024)]
    mix, targets = training.synthetic_source(tr.cfg, tr.batch, tr.t_in, tr.t_out, tr.device)()
    total = tr.step(mix, targets).item()
    assert np.isfinite(total) and torch.isfinite(tr.last_losses).all() and tr.sep.global_step == 1
    parts = tr.term_parts()
    assert parts["sc"] > 0 and parts["log_mag_l1"] > 0
    # the same spec without the keyword is refused at the first step: "gemm" stays the default
    old = training.Trainer(cfg(5118), spectral_loss={k: v for k, v in spec.items() if k != "transform"})
    with pytest.raises(NotImplementedError):
        old.step(mix, targets)
