"""GPU tests of the mel-scale terms of the spectral loss (include/wun.h: wun_op_mel_project, wun_op_mel_project_transpose,
wun_spectral_loss_mel[_fft]; spectral.SpectralLoss(mel=...)) against the float64 oracle tests/_mel_np.py and the
exact fmaf chain of tests/_fma_chain_np.py.

Single operators.  The projection is ONE ascending fmaf chain per band: it must equal the chain bit for bit (a bin the band does
not weight contributes fmaf(0, M, acc) == acc to the dense chain: the magnitudes are finite and acc is never -0).  Against float64
on the float32 table a chain of n_b fused steps with non-negative terms is off by at most (n_b + 1) 2^-24 sum_k W M (n_b roundings
of partial sums that never exceed the final one, first order, with one more for the slack), n_b the band's support.  The adjoint
is fmaf(w1, g1, w0 * g0), two operations, bit for bit.

The loss.  Every slot of `losses` and d_outputs against the float64 oracle under the project's rule for the spectral losses: the
same formulas in float32 on the CPU (tests/_mel_np.py loss_and_grad_fp32, float32 means) are the yardstick; with scale = max |x64|
over the tensor, err(x) = max |x - x64| / scale, the device must have err <= 8 err(float32 stand-in), for the losses vector and
for the gradient, the gradient taken at the signs the device took.  The fixtures keep every |Pe - Pt| at least 64 float32 spacings
of the larger of the two from 0 (asserted on the device's floats), so the mel signs are not at stake."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fma_chain_np as fc  # noqa: E402
import _mel_np as mel  # noqa: E402
import _spectral_np as ora  # noqa: E402
from _observed import record  # noqa: E402
from _unaligned import _offset_copy  # noqa: E402

import wave_u_net_amd as wun  # noqa: E402
from wave_u_net_amd import _lib, spectral, training  # noqa: E402

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------- single operators
OPS = {   # name -> (M, (n_fft, sample_rate, n_mels), filterbank arguments): K = 33, 65, 513 and 4097 bins
    "5_33_8": (5, (64, 8192, 8), {}),
    "37_65_16": (37, (128, 8192, 16), {"fmin": 100.0, "norm": "area"}),
    "300_513_40": (300, (1024, 22050, 40), {}),                  # more frames than one workgroup stages: 100 workgroups of 3
    "3_4097_128": (3, (8192, 44100, 128), {"fmax": 20000.0}),    # one frame per workgroup
}
GUARD = 8
_OPS = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def _op(name):
    if name not in _OPS:
        M, (n_fft, sr, n_mels), kw = OPS[name]
        rng = np.random.RandomState(3100 + sorted(OPS).index(name))
        words = spectral.mel_design(n_fft, sr, n_mels, **kw)
        W = spectral.mel_filterbank(n_fft, sr, n_mels, **kw)
        mags = np.abs(rng.randn(M, n_fft // 2 + 1)).astype(np.float32)
        g = rng.randn(M, n_mels).astype(np.float32)
        _OPS[name] = {"M": M, "K": n_fft // 2 + 1, "n_mels": n_mels, "words": words, "W": W, "mags": mags, "g": g,
                      "chain": fc.chain(mags, np.ascontiguousarray(W.T)), "parts": spectral.mel_table_parts(words, n_fft, n_mels)}
    return _OPS[name]


def _guarded(n, shift):
    """(buffer, view of n floats behind GUARD + shift sentinel floats)."""
    buf = torch.full((n + 2 * GUARD + shift,), -777.0, dtype=torch.float32, device="cuda")
    return buf, buf[GUARD + shift:GUARD + shift + n]


def _run_op(lib, fn, ref, src, n_out, shift):
    """fn on `src` [M, .] with every operand `shift` floats off its allocation; the output between guard floats."""
    x = torch.from_numpy(src).cuda()
    table = torch.from_numpy(ref["words"]).cuda()
    if shift:
        x, table = _offset_copy(x), _offset_copy(table)
        assert x.data_ptr() % 16 == 4 and table.data_ptr() % 16 == 4
    buf, out = _guarded(ref["M"] * n_out, shift)
    assert out.data_ptr() % 16 == (4 * shift) % 16
    _lib.check(fn(x.data_ptr(), ref["M"], ref["K"], ref["n_mels"], table.data_ptr(), out.data_ptr(), None))
    torch.cuda.synchronize()
    lo, hi = buf[:GUARD + shift], buf[GUARD + shift + out.numel():]
    assert bool((lo == -777.0).all()) and bool((hi == -777.0).all())               # the guard floats
    return out.cpu().numpy().reshape(ref["M"], n_out)


@pytest.mark.parametrize("name", sorted(OPS))
def test_project_is_the_ascending_chain(lib, name):
    ref = _op(name)
    got = _run_op(lib, lib.wun_op_mel_project, ref, ref["mags"], ref["n_mels"], 0)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), ref["chain"].view(np.int32))
    got1 = _run_op(lib, lib.wun_op_mel_project, ref, ref["mags"], ref["n_mels"], 1)   # every operand one float off 16 bytes
    assert np.array_equal(got1.view(np.int32), got.view(np.int32))
    # float64 on the float32 table, the derived bound
    want = mel.project(ref["W"], ref["mags"])
    n_b = (ref["W"] > 0).sum(1)
    tol = (n_b + 1)[None, :] * 2.0 ** -24 * want
    ratio = (np.abs(got.astype(np.float64) - want) / tol).max()
    record("mel::test_project_is_the_ascending_chain[%s]" % name, "err / bound", ratio, 1.0)
    assert (tol > 0).all() and ratio <= 1.0
    # the Python front end's floats are the operator's on the device's magnitudes
    _, (n_fft, sr, n_mels), kw = OPS[name]
    if n_fft <= 1024:
        x = torch.from_numpy(np.random.RandomState(5).randn(1, 2, n_fft + 3 * (n_fft // 4) + 1, 1).astype(np.float32)).cuda()
        ms = spectral.mel_spectrogram(x, n_fft, n_fft // 4, n_mels, sr, **kw)
        mg = spectral.stft_magnitude(x, n_fft, n_fft // 4)
        assert ms.shape == mg.shape[:4] + (n_mels,)
        want = fc.chain(mg.reshape(-1, mg.shape[4]).cpu().numpy(), np.ascontiguousarray(ref["W"].T))
        assert np.array_equal(ms.reshape(-1, n_mels).cpu().numpy().view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("name", sorted(OPS))
def test_project_transpose_is_two_operations(lib, name):
    ref = _op(name)
    b0, w0, w1, _, _ = ref["parts"]
    g, n = ref["g"], ref["n_mels"]
    pick = lambda b, w: np.where(((w != 0) & (b >= 0) & (b < n))[None, :], g[:, np.clip(b, 0, n - 1)], np.float32(0))  # noqa: E731
    want = fc.fmaf_np(w1[None, :], pick(b0 + 1, w1), w0[None, :] * pick(b0, w0))
    assert want.dtype == np.float32
    got = _run_op(lib, lib.wun_op_mel_project_transpose, ref, g, ref["K"], 0)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    got1 = _run_op(lib, lib.wun_op_mel_project_transpose, ref, g, ref["K"], 1)
    assert np.array_equal(got1.view(np.int32), got.view(np.int32))
    # it is the adjoint: float64 g W to float32 rounding of two terms
    q = mel.adjoint(ref["W"], g)
    assert np.abs(got - q).max() <= 2.0 ** -22 * np.abs(g).max() * ref["W"].max() * 2


@pytest.mark.parametrize("name", sorted(OPS))
def test_project_footprint_of_one_nan(lib, name):
    ref = _op(name)
    clean = _run_op(lib, lib.wun_op_mel_project, ref, ref["mags"], ref["n_mels"], 0)
    weighted = np.nonzero((ref["W"] > 0).sum(0) == 2)[0]
    for m, k in ((0, int(weighted[0])), (ref["M"] - 1, int(weighted[-1])), (ref["M"] // 2, int(weighted[len(weighted) // 2]))):
        bad = ref["mags"].copy()
        bad[m, k] = np.nan
        got = _run_op(lib, lib.wun_op_mel_project, ref, bad, ref["n_mels"], 0)
        hit = np.zeros(got.shape, bool)
        hit[m] = ref["W"][:, k] > 0
        assert hit.sum() == 2 and np.isnan(got[hit]).all()                          # exactly the bands that weight the bin
        assert np.array_equal(got[~hit].view(np.int32), clean[~hit].view(np.int32))


# ---------------------------------------------------------------------------------------------------- the loss
T64 = 64 + 2 * 48 + 5
CASES = {   # name -> (S, B, C, Tout, resolutions, weights, n_mels, sample_rate, log_eps of the linear-frequency log term)
    "64_48": (2, 3, 2, T64, [(64, 48)], [1.0], [8], 8192, 1e-3),
    "128_32": (1, 2, 1, 128 + 5 * 32 + 3, [(128, 32)], [1.0], [16], 8192, 1e-3),
    "1024_768": (3, 1, 1, 1024 + 2 * 768 + 3, [(1024, 768)], [1.0], [40], 22050, 1.0),
    "two_resolutions": (3, 2, 2, 128 + 3 * 32 + 7, [(64, 48), (128, 32)], [1.0, 0.5], [8, 16], 8192, 1e-3),
    "4096_1024": (1, 1, 1, 4096 + 1024 + 5, [(4096, 1024)], [1.0], [128], 44100, 4.0),    # fft only: one short row
}
RUNS = [(n, t) for n in sorted(CASES) for t in ("gemm", "fft") if not (n == "4096_1024" and t == "gemm")]
MSE_W, SC_EPS, MEL_EPS = 0.25, 1.0, 1e-3
MEL_W = {"mel_l1": 0.7, "log_mel_l1": 0.4}
TERM_SETS = {"mel": None, "all": {"mag_l1": 0.7, "log_mag_l1": 0.4, "sc": 1.3, "complex_l1": 0.6}}
_CACHE = {}


def _f32(x):
    return float(np.float32(x))


def _case(name):
    if name not in _CACHE:
        S, B, C, T, res, w, n_mels, sr, le = CASES[name]
        rng = np.random.RandomState(4000 + sorted(CASES).index(name))
        out = rng.randn(S, B, T, C).astype(np.float32)
        tgt = rng.randn(S, B, T, C).astype(np.float32)
        W = [mel.filterbank32(n_fft, sr, n) for (n_fft, _), n in zip(res, n_mels)]
        _CACHE[name] = {"out": out, "tgt": tgt, "res": res, "w": w, "n_mels": n_mels, "sr": sr, "log_eps": le, "W": W, "ref": {}}
    return _CACHE[name]


def _loss(ref, transform, terms, mel_terms=MEL_W, mse_w=MSE_W):
    return spectral.SpectralLoss(ref["res"], ref["w"], mse_w, terms=terms, log_eps=ref["log_eps"], sc_eps=SC_EPS, transform=transform,
                                 mel={"n_mels": ref["n_mels"], "sample_rate": ref["sr"], "terms": mel_terms, "log_eps": MEL_EPS})


def _dev(ref):
    return torch.from_numpy(ref["out"]).cuda(), torch.from_numpy(ref["tgt"]).cuda()


def _device_signs(ref, transform):
    """(signs of Me - Mt, signs of Pe - Pt) per resolution from the device's own floats; asserts the fixture's margin."""
    out, tgt = _dev(ref)
    signs, msigns = [], []
    for (n_fft, hop), n in zip(ref["res"], ref["n_mels"]):
        me, mt = (spectral.stft_magnitude(x, n_fft, hop, transform) for x in (out, tgt))
        pe, pt = (spectral.mel_spectrogram(x, n_fft, hop, n, ref["sr"], transform=transform) for x in (out, tgt))
        F = me.shape[3]
        me, mt, pe, pt = (v.reshape(-1, F, v.shape[4]).cpu().numpy() for v in (me, mt, pe, pt))
        margin = np.abs(pe - pt) / (2.0 ** -23 * np.maximum(pe, pt))
        assert margin.min() >= 64, margin.min()                                     # no mel sign is at stake
        signs.append(np.sign(me - mt))
        msigns.append(np.sign(pe - pt))
    return signs, msigns


def _reference(ref, transform, tname):
    """(l64, g64, l32, g32) at the device's signs, once per (case, transform, term set)."""
    key = (transform, tname)
    if key not in ref["ref"]:
        signs, msigns = _device_signs(ref, transform)
        m = {"W": ref["W"], "terms": MEL_W, "log_eps": _f32(MEL_EPS)}
        args = (ref["out"], ref["tgt"], ref["res"], ref["w"], MSE_W, TERM_SETS[tname] or {}, _f32(ref["log_eps"]), SC_EPS, m)
        l64, g64 = mel.loss_and_grad(*args, signs=signs, mel_signs=msigns)
        l32, g32 = mel.loss_and_grad_fp32(*args, signs, msigns)
        ref["ref"][key] = (l64, g64, l32, g32)
    return ref["ref"][key]


def _slot_names(nres):
    return (["total", "MSE"] + ["L_%d" % j for j in range(nres)] + ["%s_%d" % (t, j) for j in range(nres) for t in spectral.TERMS]
            + ["%s_%d" % (t, j) for j in range(nres) for t in spectral.MEL_TERMS])


@pytest.mark.parametrize("tname", sorted(TERM_SETS))
@pytest.mark.parametrize("name, transform", RUNS)
def test_losses_and_gradient_against_float64(lib, name, transform, tname):
    ref = _case(name)
    nres = len(ref["res"])
    l64, g64, l32, g32 = _reference(ref, transform, tname)
    out, tgt = _dev(ref)
    loss = _loss(ref, transform, TERM_SETS[tname])
    losses, d_out = loss.loss_and_grad(out, tgt)
    assert losses.shape == (2 + 7 * nres,) == l64.shape and torch.isfinite(losses).all() and torch.isfinite(d_out).all()
    tag = "mel::test_losses_and_gradient_against_float64[%s-%s-%s]" % (name, transform, tname)
    got = losses.cpu().numpy().astype(np.float64)
    scale = np.abs(l64).max()
    e32 = np.abs(l32.astype(np.float64) - l64).max() / scale
    record(tag, "losses: cpu fp32 e32", e32, 1.0)
    for i, what in enumerate(_slot_names(nres)):
        if l64[i] == 0.0:
            assert got[i] == 0.0, what                                              # a term that is not in the set
            continue
        e = abs(got[i] - l64[i]) / scale
        print("[mel] %s %s gpu %.9g f64 %.9g" % (tag, what, got[i], l64[i]))
        record(tag, "%s err / (8 e32)" % what, e / (8 * e32), 1.0)
        assert e <= 8 * e32, (what, got[i], l64[i], e, e32)
    gs = np.abs(g64).max()
    eg32 = np.abs(g32.astype(np.float64) - g64).max() / gs
    eg = np.abs(d_out.cpu().numpy().astype(np.float64) - g64).max() / gs
    record(tag, "gradient: cpu fp32 e32", eg32, 1.0)
    record(tag, "gradient err / (8 e32)", eg / (8 * eg32), 1.0)
    assert gs > 0 and eg <= 8 * eg32, (eg, eg32)
    # the mel slots are functions of the floats mel_spectrogram returns: float64 formulas on those floats
    per = {t: v.cpu().numpy().astype(np.float64) for t, v in loss.term_losses(losses).items()}
    for j, ((n_fft, hop), n) in enumerate(zip(ref["res"], ref["n_mels"])):
        pe, pt = (spectral.mel_spectrogram(x, n_fft, hop, n, ref["sr"], transform=transform).cpu().numpy() for x in (out, tgt))
        l1, ll = mel.mel_terms(pe, pt, _f32(MEL_EPS))
        e = _f32(MEL_EPS)
        log_tol = (2.0 ** -21 * (np.abs(np.log(pe.astype(np.float64) + e)) + np.abs(np.log(pt.astype(np.float64) + e)))).mean() + 2.0 ** -22
        assert abs(per["mel_l1"][j] - l1) <= 2.0 ** -23 * l1                         # float64 sums, one rounding of the slot
        assert abs(per["log_mel_l1"][j] - ll) <= log_tol + 2.0 ** -24 * ll          # (logf, two additions of e, one subtraction)


@pytest.mark.parametrize("name, transform", RUNS)
def test_zero_mel_weights_are_the_terms_entry(lib, name, transform):
    ref = _case(name)
    out, tgt = _dev(ref)
    nres = len(ref["res"])
    terms = TERM_SETS["all"]
    old = spectral.SpectralLoss(ref["res"], ref["w"], MSE_W, terms=terms, log_eps=ref["log_eps"], sc_eps=SC_EPS, transform=transform)
    l0, g0 = old.loss_and_grad(out, tgt)
    new = _loss(ref, transform, terms, mel_terms={})
    assert new.num_losses == 2 + 7 * nres and new.scratch_floats(out.shape) == old.scratch_floats(out.shape)
    l1, g1 = new.loss_and_grad(out, tgt)
    assert l1.shape == (2 + 7 * nres,)
    assert l1[:2 + 5 * nres].view(torch.int32).eq(l0.view(torch.int32)).all()
    assert g1.view(torch.int32).eq(g0.view(torch.int32)).all()
    assert bool((l1[2 + 5 * nres:] == 0).all())
    l2, none = new.loss_and_grad(out, tgt, grad=False)
    assert none is None and torch.equal(l2, l1)


@pytest.mark.parametrize("name, transform", RUNS)
def test_exact_cases(lib, name, transform):
    ref = _case(name)
    out, tgt = _dev(ref)
    nres = len(ref["res"])
    # estimates bit-equal to the targets: every slot and the gradient exactly 0
    for tname in sorted(TERM_SETS):
        losses, g = _loss(ref, transform, TERM_SETS[tname], mse_w=1.0).loss_and_grad(tgt.clone(), tgt)
        assert bool((losses == 0).all()) and bool((g == 0).all())
    # samples behind the last frame hold exactly the MSE term
    loss = _loss(ref, transform, None, mse_w=0.5)
    losses, g = loss.loss_and_grad(out, tgt)
    covered = max(n + (ora.num_frames(out.shape[2], n, h) - 1) * h for n, h in ref["res"])
    cm = np.float32(np.float64(np.float32(0.5)) * 2.0 / out.numel())
    assert covered < out.shape[2] and torch.equal(g[:, :, covered:], (out - tgt)[:, :, covered:] * float(cm))
    assert not torch.equal(g[:, :, :covered], (out - tgt)[:, :, :covered] * float(cm))
    # d_outputs = NULL leaves the same losses; one mel term alone reports the other as 0
    l2, none = loss.loss_and_grad(out, tgt, grad=False)
    assert none is None and torch.equal(l2, losses)
    l3, _ = _loss(ref, transform, None, mel_terms={"log_mel_l1": 1.0}, mse_w=0.5).loss_and_grad(out, tgt)
    per = l3[2 + 5 * nres:].view(nres, 2)
    assert bool((per[:, 0] == 0).all()) and torch.equal(per[:, 1], losses[2 + 5 * nres:].view(nres, 2)[:, 1])
    assert bool((l3[2 + nres:2 + 5 * nres] == 0).all())                             # no linear-frequency term


@pytest.mark.parametrize("name, transform", RUNS)
def test_reproducible_bits(lib, name, transform, monkeypatch):
    ref = _case(name)
    out, tgt = _dev(ref)
    loss = _loss(ref, transform, TERM_SETS["all"])
    l0, g0 = loss.loss_and_grad(out, tgt)
    l1, g1 = loss.loss_and_grad(out, tgt)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    for fill in (float("nan"), 0.0):
        scratch = torch.full((loss.scratch_floats(out.shape),), fill, dtype=torch.float32, device="cuda")
        g2, l2 = torch.full_like(out, float("nan")), torch.full_like(l0, float("nan"))
        loss.run(out, tgt, g2, l2, scratch)
        assert torch.equal(l0, l2) and torch.equal(g0, g2)
    # every buffer one float off 16 bytes, the tables too
    o1, t1 = _offset_copy(out), _offset_copy(tgt)
    g3 = torch.empty(out.numel() + 1, dtype=torch.float32, device="cuda")[1:].view(out.shape)
    scratch = torch.empty(loss.scratch_floats(out.shape) + 1, dtype=torch.float32, device="cuda")[1:]
    l3 = torch.empty(loss.num_losses + 1, dtype=torch.float32, device="cuda")[1:]
    mtabs = [_offset_copy(t) for t in loss._mel_tables(out.device)]
    monkeypatch.setattr(loss, "_mel_tables", lambda dev: mtabs)
    for n_fft, _ in ref["res"]:
        key = (transform, n_fft, str(out.device))
        monkeypatch.setitem(spectral._TABLES, key, _offset_copy(spectral._TABLES[key]))
    assert all(t.data_ptr() % 16 == 4 for t in [o1, t1, g3, scratch, l3] + mtabs + [spectral._TABLES[(transform, n, str(out.device))]
                                                                                     for n, _ in ref["res"]])
    loss.run(o1, t1, g3, l3, scratch)
    assert torch.equal(g3, g0) and torch.equal(l3, l0)


# ---------------------------------------------------------------------------------------------------- through the layers
def test_autograd_wrapper(lib):
    ref = _case("two_resolutions")
    out, tgt = _dev(ref)
    out.requires_grad_(True)
    loss = _loss(ref, "gemm", TERM_SETS["all"])
    l0, g0 = loss.loss_and_grad(out.detach(), tgt)
    total = spectral.stft_l1(out, tgt, loss)
    (3.0 * total).backward()
    assert total.item() == l0[0].item() and torch.equal(out.grad, g0 * 3.0)
    assert loss(out.detach(), tgt).item() == l0[0].item()


_E2E_SPEC = {"resolutions": [[64, 48]], "mse_weight": 1.0, "terms": {"sc": 1},
             "mel": {"n_mels": 8, "sample_rate": 8192, "terms": {"mel_l1": 1.0, "log_mel_l1": 0.5}}}


def _e2e_cfg(tmp, **over):
    return wun.get_config("full", num_layers=3, num_initial_filters=8, num_frames=200, batch_size=4, epoch_it=3,
                          model_base_dir=os.path.join(tmp, "ckpt"), log_dir=os.path.join(tmp, "logs"),
                          init_sup_sep_lr=1e-3, **over)


def test_trainer_end_to_end(lib, tmp_path, monkeypatch):
    monkeypatch.setenv("WUN_NO_TUNE", "1")
    cfg = _e2e_cfg(str(tmp_path))
    tr = training.Trainer(cfg, spectral_loss=_E2E_SPEC)
    assert tr.t_out >= 64 + 48 and tr.spectral.num_losses == 2 + 7 and tr.spectral.mel["n_mels"] == [8]
    mix, targets = training.synthetic_source(cfg, tr.batch, tr.t_in, tr.t_out, tr.device)()
    first = tr.step(mix, targets).item()
    assert tr.last_losses.shape == (2 + 7,)
    l = tr.last_losses.tolist()
    parts = tr.term_parts()
    assert sorted(parts) == sorted(spectral.TERMS + spectral.MEL_TERMS)
    assert parts["mel_l1"] == l[7] > 0 and parts["log_mel_l1"] == 0.5 * l[8] > 0 and parts["sc"] == l[5] > 0
    assert parts["mag_l1"] == 0 and parts["log_mag_l1"] == 0 and parts["complex_l1"] == 0
    mse, spec = tr.loss_parts()
    assert abs(sum(parts.values()) - spec) <= 1e-6 * spec and abs(first - (mse + spec)) <= 1e-6 * first
    for _ in range(19):
        last = tr.step(mix, targets).item()
    assert np.isfinite(last) and last < first and tr.sep.global_step == 20           # one repeated batch: the loss goes down


def test_train_log_carries_the_mel_terms(lib, tmp_path, monkeypatch):
    monkeypatch.setenv("WUN_NO_TUNE", "1")
    training.train(_e2e_cfg(str(tmp_path), spectral_loss=_E2E_SPEC), "mel")
    log = [json.loads(l) for l in open(os.path.join(str(tmp_path), "logs", "mel", "train.jsonl"))]
    assert len(log) == 3
    for line in log:
        parts = line["spectral_terms"]
        assert sorted(parts) == sorted(spectral.TERMS + spectral.MEL_TERMS) and parts["mel_l1"] > 0 and parts["log_mel_l1"] > 0
        assert abs(sum(parts.values()) - line["spectral_loss"]) <= 1e-6 * line["spectral_loss"]
    # a run without `mel` has the four terms only
    training.train(_e2e_cfg(str(tmp_path), spectral_loss={"resolutions": [[64, 48]], "mse_weight": 1.0, "terms": {"sc": 1}}), "no_mel")
    old = [json.loads(l) for l in open(os.path.join(str(tmp_path), "logs", "no_mel", "train.jsonl"))]
    assert len(old) == 3 and all(sorted(line["spectral_terms"]) == sorted(spectral.TERMS) for line in old)
