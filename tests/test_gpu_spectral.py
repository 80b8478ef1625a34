"""GPU tests of the spectral loss (include/wun.h: wun_stft_magnitude, wun_spectral_loss; wave_u_net_amd.spectral; DESIGN.md
5.10) against the float64 oracle tests/_spectral_np.py.

Bounds.  beta[r][f] = n_fft 2^-24 sum_n |w[n] x[f hop + n]| bounds the error of an fp32 dot product of the windowed frame with
factors of modulus <= 1 in any order; Re and Im each carry at most beta, so a magnitude carries sqrt(2) beta plus the rounding
of the square root and the two squares (2^-22 relative).  A loss, being a mean of |M_est - M_tgt|, carries the mean of both
signals' bounds.  The L1 sign is discontinuous: the gradient is compared with the oracle's gradient AT THE SIGNS THE GPU TOOK
(as _gpu_pins does for LeakyReLU branches), the yardstick being a second fp32 computation of the same formula on the CPU, and a
pinned sign may differ from float64's only where the two magnitudes tie within their bounds."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _spectral_np as ora  # noqa: E402
from _observed import record  # noqa: E402
from _unaligned import _offset_copy  # noqa: E402

import wave_u_net_amd as wun  # noqa: E402
from wave_u_net_amd import _lib, spectral, training  # noqa: E402
from wave_u_net_amd.separator import UnetAudioSeparator  # noqa: E402

pytestmark = pytest.mark.gpu

SQRT2 = np.sqrt(2.0)
T_SMALL = 64 + 2 * 48 + 5
CASES = {   # name -> (S, B, C, Tout, resolutions, weights)
    "64_48": (2, 3, 2, T_SMALL, [(64, 48)], [1.0]),                       # three frames and a tail
    "64_16": (2, 3, 2, T_SMALL, [(64, 16)], [1.0]),                       # four frames per sample
    "64_37": (2, 3, 2, T_SMALL, [(64, 37)], [1.0]),                       # an odd hop
    "64_64": (2, 3, 2, T_SMALL, [(64, 64)], [1.0]),                       # no overlap
    "1024_768": (2, 2, 1, 1024 + 2 * 768 + 3, [(1024, 768)], [1.0]),      # the reference's setting
    "1024_one_frame": (2, 2, 1, 1024, [(1024, 768)], [1.0]),              # one frame, no tail
    "two_resolutions": (2, 3, 2, T_SMALL, [(64, 48), (64, 16)], [1.0, 0.5]),
}
MSE_W = 0.25
_CACHE = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def _case(name):
    """Inputs and the float64 references of a case, computed once."""
    if name not in _CACHE:
        S, B, C, T, res, w = CASES[name]
        rng = np.random.RandomState(1000 + sorted(CASES).index(name))
        out = rng.randn(S, B, T, C).astype(np.float32)
        tgt = rng.randn(S, B, T, C).astype(np.float32)
        ref = {"out": out, "tgt": tgt, "res": res, "w": w}
        ref["m_est"] = [ora.magnitude(out, n, h) for n, h in res]
        ref["m_tgt"] = [ora.magnitude(tgt, n, h) for n, h in res]
        ref["b_est"] = [ora.beta(out, n, h) for n, h in res]
        ref["b_tgt"] = [ora.beta(tgt, n, h) for n, h in res]
        ref["losses"], _ = ora.loss_and_grad(out, tgt, res, w, MSE_W)
        _CACHE[name] = ref
    return _CACHE[name]


def _gpu_mags(x, n_fft, hop):
    m = spectral.stft_magnitude(x, n_fft, hop)
    S, B, C, F, K = m.shape
    assert F == ora.num_frames(x.shape[2], n_fft, hop) and K == n_fft // 2 + 1
    return m.reshape(S * B * C, F, K)


def _loss_bound(ref, j):
    return SQRT2 * (ref["b_est"][j].mean() + ref["b_tgt"][j].mean()) + 2.0 ** -22 * ref["losses"][2 + j]


# ---------------------------------------------------------------------------------------------------- 1. magnitudes
@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset1"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_magnitudes_against_float64(lib, name, offset):
    ref = _case(name)
    for key, mk, bk in (("out", "m_est", "b_est"), ("tgt", "m_tgt", "b_tgt")):
        x = torch.from_numpy(ref[key]).cuda()
        if offset:
            x = _offset_copy(x)
        for j, (n_fft, hop) in enumerate(ref["res"]):
            got = _gpu_mags(x, n_fft, hop).cpu().numpy().astype(np.float64)
            bound = SQRT2 * ref[bk][j][:, :, None] + 2.0 ** -22 * ref[mk][j]
            ratio = (np.abs(got - ref[mk][j]) / bound).max()
            record("test_magnitudes_against_float64[%s]" % name, "%s %d/%d max err / bound" % (key, n_fft, hop), ratio, 1.0)
            assert np.isfinite(got).all() and ratio <= 1.0
            if offset:
                assert np.array_equal(got, _gpu_mags(torch.from_numpy(ref[key]).cuda(), n_fft, hop).cpu().numpy())


# ---------------------------------------------------------------------------------------------------- 2. loss
@pytest.mark.parametrize("name", sorted(CASES))
def test_losses_against_float64(lib, name):
    ref = _case(name)
    loss = spectral.SpectralLoss(ref["res"], ref["w"], MSE_W)
    losses, _ = loss.loss_and_grad(torch.from_numpy(ref["out"]).cuda(), torch.from_numpy(ref["tgt"]).cuda())
    got, want = losses.cpu().numpy().astype(np.float64), ref["losses"]
    assert got.shape == (2 + len(ref["res"]),)
    mse_tol = 1e-6 * want[1]
    record("test_losses_against_float64[%s]" % name, "MSE relative", abs(got[1] - want[1]) / want[1], 1e-6)
    assert abs(got[1] - want[1]) <= mse_tol
    total_tol = MSE_W * mse_tol
    for j in range(len(ref["res"])):
        tol = _loss_bound(ref, j)
        record("test_losses_against_float64[%s]" % name, "L_%d err / bound" % j, abs(got[2 + j] - want[2 + j]) / tol, 1.0)
        assert abs(got[2 + j] - want[2 + j]) <= tol
        total_tol += ref["w"][j] * tol
    record("test_losses_against_float64[%s]" % name, "total err / bound", abs(got[0] - want[0]) / total_tol, 1.0)
    assert abs(got[0] - want[0]) <= total_tol


# ---------------------------------------------------------------------------------------------------- 3. gradient, signs pinned
@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset1"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_gradient_with_pinned_signs(lib, name, offset):
    ref = _case(name)
    out, tgt = torch.from_numpy(ref["out"]).cuda(), torch.from_numpy(ref["tgt"]).cuda()
    if offset:
        out, tgt = _offset_copy(out), _offset_copy(tgt)
    signs = []
    for j, (n_fft, hop) in enumerate(ref["res"]):
        sg = torch.sign(_gpu_mags(out, n_fft, hop) - _gpu_mags(tgt, n_fft, hop)).cpu().numpy().astype(np.float64)
        d64 = ref["m_est"][j] - ref["m_tgt"][j]
        flipped = sg != np.sign(d64)
        tie = np.abs(d64) <= SQRT2 * (ref["b_est"][j] + ref["b_tgt"][j])[:, :, None]
        record("test_gradient_with_pinned_signs[%s]" % name, "signs differing from float64 (count)", flipped.sum(), sg.size)
        assert not (flipped & ~tie).any()
        signs.append(sg)
    loss = spectral.SpectralLoss(ref["res"], ref["w"], MSE_W)
    if offset:
        N = out.numel()
        d_out = torch.empty(N + 1, dtype=torch.float32, device="cuda")[1:].view(out.shape)
        scratch = torch.empty(loss.scratch_floats(out.shape) + 1, dtype=torch.float32, device="cuda")[1:]
        losses = torch.empty(2 + len(ref["res"]) + 1, dtype=torch.float32, device="cuda")[1:]
        loss.run(out, tgt, d_out, losses, scratch)
        l0, g0 = loss.loss_and_grad(torch.from_numpy(ref["out"]).cuda(), torch.from_numpy(ref["tgt"]).cuda())
        assert torch.equal(d_out, g0) and torch.equal(losses, l0)          # the bits do not depend on the alignment
    else:
        _, d_out = loss.loss_and_grad(out, tgt)
    _, g64 = ora.loss_and_grad(ref["out"], ref["tgt"], ref["res"], ref["w"], MSE_W, signs=signs)
    g32 = ora.grad_fp32(ref["out"], ref["tgt"], ref["res"], ref["w"], MSE_W, signs)
    scale = np.abs(g64).max()
    e32 = np.abs(g32.astype(np.float64) - g64).max() / scale
    egpu = np.abs(d_out.cpu().numpy().astype(np.float64) - g64).max() / scale
    record("test_gradient_with_pinned_signs[%s]" % name, "cpu fp32 e32", e32, 1.0)
    record("test_gradient_with_pinned_signs[%s]" % name, "gpu err / max |g64|", egpu, 8 * e32)
    assert egpu <= 8 * e32


# ---------------------------------------------------------------------------------------------------- 4. exact cases
@pytest.mark.parametrize("name", ["64_48", "1024_768", "two_resolutions"])
def test_exact_cases(lib, name):
    ref = _case(name)
    tgt = torch.from_numpy(ref["tgt"]).cuda()
    out = torch.from_numpy(ref["out"]).cuda()
    res, w = ref["res"], ref["w"]
    # estimates all zero, no MSE term: no gradient anywhere (the term of a bin with M_est = 0 is 0)
    losses, g = spectral.SpectralLoss(res, w, 0.0).loss_and_grad(torch.zeros_like(tgt), tgt)
    assert torch.isfinite(losses).all() and bool((g == 0).all())
    for j in range(len(res)):
        want = ref["m_tgt"][j].mean()
        tol = SQRT2 * ref["b_tgt"][j].mean() + 2.0 ** -22 * want
        record("test_exact_cases[%s]" % name, "zero estimates L_%d err / bound" % j, abs(losses[2 + j].item() - want) / tol, 1.0)
        assert abs(losses[2 + j].item() - want) <= tol
    # estimates bit-equal to the targets: sgn(0) = 0
    losses, g = spectral.SpectralLoss(res, w, 1.0).loss_and_grad(tgt.clone(), tgt)
    assert bool((losses == 0).all()) and bool((g == 0).all())
    # samples behind the last frame hold exactly the MSE term
    loss = spectral.SpectralLoss(res, w, 0.5)
    losses, g = loss.loss_and_grad(out, tgt)
    covered = max(n + (ora.num_frames(out.shape[2], n, h) - 1) * h for n, h in res)
    cm = np.float32(np.float64(np.float32(0.5)) * 2.0 / out.numel())
    assert torch.equal(g[:, :, covered:], (out - tgt)[:, :, covered:] * float(cm))
    if covered < out.shape[2]:
        assert not torch.equal(g[:, :, :covered], (out - tgt)[:, :, :covered] * float(cm))
    # d_outputs = NULL leaves the same losses
    l2, none = loss.loss_and_grad(out, tgt, grad=False)
    assert none is None and torch.equal(l2, losses)


# ---------------------------------------------------------------------------------------------------- 5. MSE alone
def test_mse_alone_matches_loss_and_gradients(lib):
    from test_gpu_backward import MSE_EQ_TOL, _per_tensor_equal, _setup
    sep, ocfg, params, mix, tg = _setup("baseline_small")
    sep.get_output(mix, True)
    want = sep.loss_and_gradients(tg).item()
    g_ref = sep.grads.clone()
    sep.grads.fill_(float("nan"))
    got = sep.loss_and_gradients(tg, loss=spectral.SpectralLoss([], mse_weight=1.0))
    torch.cuda.synchronize()
    record("test_mse_alone_matches_loss_and_gradients", "loss relative", abs(got.item() - want) / want, 1e-6)
    assert abs(got.item() - want) <= 1e-6 * want
    assert sep.last_losses.shape == (2,) and sep.last_losses[0].item() == sep.last_losses[1].item()
    _per_tensor_equal(sep, g_ref, sep.grads, MSE_EQ_TOL, "mse_alone")


# ---------------------------------------------------------------------------------------------------- 6. reproducibility
@pytest.mark.parametrize("name", ["64_37", "1024_768", "two_resolutions"])
def test_reproducible_bits(lib, name):
    ref = _case(name)
    out, tgt = torch.from_numpy(ref["out"]).cuda(), torch.from_numpy(ref["tgt"]).cuda()
    loss = spectral.SpectralLoss(ref["res"], ref["w"], MSE_W)
    l0, g0 = loss.loss_and_grad(out, tgt)
    l1, g1 = loss.loss_and_grad(out, tgt)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    scratch = torch.full((loss.scratch_floats(out.shape),), float("nan"), dtype=torch.float32, device="cuda")
    g2 = torch.full_like(out, float("nan"))
    l2 = torch.full_like(l0, float("nan"))
    loss.run(out, tgt, g2, l2, scratch)
    assert torch.equal(l0, l2) and torch.equal(g0, g2)
    # a row's magnitudes do not depend on the batch around it: slices of S and of B land in other tiles of the GEMM
    for n_fft, hop in ref["res"]:
        full = spectral.stft_magnitude(out, n_fft, hop)
        assert torch.equal(spectral.stft_magnitude(out[1:2], n_fft, hop), full[1:2])
        assert torch.equal(spectral.stft_magnitude(out[:, 1:2], n_fft, hop), full[:, 1:2])
        assert torch.equal(spectral.stft_magnitude(out[:, -1:], n_fft, hop), full[:, -1:])


def test_autograd_wrapper(lib):
    ref = _case("two_resolutions")
    out = torch.from_numpy(ref["out"]).cuda().requires_grad_(True)
    tgt = torch.from_numpy(ref["tgt"]).cuda()
    loss = spectral.SpectralLoss(ref["res"], ref["w"], MSE_W)
    l0, g0 = loss.loss_and_grad(out.detach(), tgt)
    total = spectral.stft_l1(out, tgt, loss)
    (3.0 * total).backward()
    assert total.item() == l0[0].item() and torch.equal(out.grad, g0 * 3.0)
    assert spectral.stft_l1(out.detach(), tgt, resolutions=ref["res"], weights=ref["w"], mse_weight=MSE_W).item() == l0[0].item()


# ---------------------------------------------------------------------------------------------------- 7. end to end
_E2E_RES, _E2E_SPEC = [(64, 48)], {"resolutions": [[64, 48]], "mse_weight": 1.0}


def _e2e_cfg(tmp, **over):
    return wun.get_config("full", num_layers=3, num_initial_filters=8, num_frames=200, batch_size=4, epoch_it=3,
                          model_base_dir=os.path.join(tmp, "ckpt"), log_dir=os.path.join(tmp, "logs"),
                          init_sup_sep_lr=1e-3, **over)


def _oracle_losses(cfg, sep, mix, targets):
    """[total, MSE, L_0] of _E2E_SPEC and its bounds, from the float64 oracle forward on the separator's weights."""
    from oracle import waveunet_torch as wt
    names = [n for n, _, _ in sep._active.tensors]
    v = sep.variables()
    tp = [(n, v[n].detach().cpu().double()) for n in names]
    o = wt.get_output(cfg, tp, mix.cpu().double(), True)
    out = torch.stack([o[n] for n in cfg["source_names"]]).numpy()
    tgt = targets.cpu().numpy()
    losses, _ = ora.loss_and_grad(out, tgt, _E2E_RES, [1.0], 1.0)
    l_tol = SQRT2 * (ora.beta(out, 64, 48).mean() + ora.beta(tgt, 64, 48).mean()) + 2.0 ** -22 * losses[2]
    return losses, np.array([1e-6 * losses[1] + l_tol, 1e-6 * losses[1], l_tol])


def _check_logged(tag, got, want, tol):
    for i, what in enumerate(("total", "mse", "spectral")):
        record(tag, "%s err / bound" % what, abs(got[i] - want[i]) / tol[i], 1.0)
        assert abs(got[i] - want[i]) <= tol[i], (what, got[i], want[i], tol[i])


def test_trainer_end_to_end(lib, tmp_path, monkeypatch):
    monkeypatch.setenv("WUN_NO_TUNE", "1")
    cfg = _e2e_cfg(str(tmp_path))
    tr = training.Trainer(cfg, spectral_loss=_E2E_SPEC)
    assert tr.t_out >= 64 + 48
    mix, targets = training.synthetic_source(cfg, tr.batch, tr.t_in, tr.t_out, tr.device)()
    want, tol = _oracle_losses(cfg, tr.sep, mix, targets)
    first = tr.step(mix, targets).item()
    mse, spec = tr.loss_parts()
    _check_logged("test_trainer_end_to_end", (first, mse, spec), want, tol)
    for _ in range(19):
        last = tr.step(mix, targets).item()
    assert np.isfinite(last) and last < first and tr.sep.global_step == 20

    # gradient accumulation: the first step's loss is the mean of the two micro-batches' losses
    ta = training.Trainer(cfg, spectral_loss=_E2E_SPEC, grad_accum_steps=2)
    halves = [_oracle_losses(cfg, ta.sep, mix[lo:lo + 2], targets[:, lo:lo + 2]) for lo in (0, 2)]
    first = ta.step(mix, targets).item()
    _check_logged("test_trainer_end_to_end[accum2]", (first,) + ta.loss_parts(),
                  (halves[0][0] + halves[1][0]) / 2, (halves[0][1] + halves[1][1]) / 2)

    # spectral_loss=None is the parent's step, bit for bit
    t0, t1 = training.Trainer(cfg), training.Trainer(cfg, spectral_loss=None)
    assert t1.spectral is None
    for _ in range(2):
        a, b = t0.step(mix, targets), t1.step(mix, targets)
        assert a.item() == b.item()
    assert torch.equal(t0.sep.params, t1.sep.params) and torch.equal(t0.sep.adam_v, t1.sep.adam_v)


def test_train_log_carries_the_loss_parts(lib, tmp_path, monkeypatch):
    monkeypatch.setenv("WUN_NO_TUNE", "1")
    cfg = _e2e_cfg(str(tmp_path), spectral_loss=_E2E_SPEC)
    training.train(cfg, "spec")
    log = [json.loads(l) for l in open(os.path.join(str(tmp_path), "logs", "spec", "train.jsonl"))]
    assert len(log) == 3
    for line in log:
        assert abs(line["sep_loss"] - (line["mse_loss"] + line["spectral_loss"])) <= 1e-6 * line["sep_loss"]
        assert line["spectral_loss"] > 0 and line["mse_loss"] > 0
    training.train(_e2e_cfg(str(tmp_path)), "plain")
    plain = [json.loads(l) for l in open(os.path.join(str(tmp_path), "logs", "plain", "train.jsonl"))]
    assert all("mse_loss" not in line and "spectral_loss" not in line for line in plain)
