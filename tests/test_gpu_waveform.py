"""GPU tests of the waveform losses (include/wun.h: wun_waveform_loss; wave_u_net_amd.waveform) against the
float64 oracle tests/_waveform_np.py.

Bounds.  The device forms the row sums in float64 from exact products, so they err by at most n 2^-52 of the sums of absolute
values: the row scalars are exact for these tests except through the cancellation in Nn = See - P and Dd.  With k = 10 / ln 10:
    mse, l1      2^-22 relative: d formed in fp32 (2^-24 of |d|, twice for the square) and the final rounding
    SI_r, SNR_r  per source, and the si_sdr / snr terms: 2^-23 |value| + the mean over the rows of
                 cond_r = k n 2^-50 (See + P) / (Nn + eps); for SNR the denominator is Dd + eps
    total        2^-23 |total| + sum_t weight_t bound_t
    gradient     per element C_ROUND 2^-24 (|mse part| + |l1 part| + |v|) + (cond_si_r + cond_snr_r) |v|.
                 C_ROUND = 6: the fp32 roundings of the expression the header fixes are cm = (float)(mse 2 / N), d = e - t,
                 cm d, the add of the l1 part, (float)v and the add of (float)v -- six.  (cl = (float)(l1 / N) is a seventh,
                 of a constant; no path through the expression carries more than five of them, so 6 also covers the second-order
                 terms.)  The sign of the l1 part needs no pinning: the sign of an fp32 difference of two floats is the sign of
                 the exact difference.
The weights and eps given to the oracle are the floats the entry receives.

Shapes (S, B, Tout, C): (2, 3, 165, 2) a row has 330 floats, several rows share one flat 1024-block; (2, 3, 700, 2) n = 1400, the
second chunk of each row is partial and flat blocks straddle rows and the two sources; (1, 2, 512, 2) n = 1024 exactly;
(3, 2, 2049, 1) a one-float last chunk, S = 3; (2, 2, 5000, 2) several chunks per row.  Estimates = targets + noise, the noise
scaled per row so that SI_r spans about -10 .. +40 dB."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _waveform_np as ora  # noqa: E402
from _observed import record  # noqa: E402
from _unaligned import _offset_copy  # noqa: E402

import wave_u_net_amd as wun  # noqa: E402
from wave_u_net_amd import _lib, datasets, spectral, training, validation, waveform  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {"330": (2, 3, 165, 2), "1400": (2, 3, 700, 2), "1024": (1, 2, 512, 2), "2049": (3, 2, 2049, 1), "10000": (2, 2, 5000, 2)}
ALL = {"mse": 0.7, "l1": 0.4, "si_sdr": 0.05, "snr": 0.03}
TERM_SETS = {"mse": {"mse": 1.0}, "l1": {"l1": 1.0}, "si_sdr": {"si_sdr": 1.0}, "snr": {"snr": 1.0}, "all": ALL}
EPS = 1e-8
C_ROUND = 6
_CACHE = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def _f32(x):
    """The float the entry receives (wun_waveform_terms holds floats), as a Python float."""
    return float(np.float32(x))


def _case(name):
    """Inputs of a case, computed once: targets randn + 0.1, estimates = targets + noise at -10 .. +40 dB per row."""
    if name not in _CACHE:
        S, B, T, C = CASES[name]
        rng = np.random.RandomState(3000 + sorted(CASES).index(name))
        tgt = (rng.randn(S, B, T, C) + 0.1).astype(np.float32)
        db = np.linspace(-10.0, 40.0, S * B).reshape(S, B, 1, 1)
        out = (tgt + rng.randn(S, B, T, C) * 10.0 ** (-db / 20.0)).astype(np.float32)
        _CACHE[name] = {"out": out, "tgt": tgt, "oracle": {}}
    return _CACHE[name]


def _oracle(ref, tname, zero_mean=True):
    """(losses, gradient, parts) of the float64 oracle for a term set, computed once per case."""
    key = (tname, zero_mean)
    if key not in ref["oracle"]:
        terms = {t: _f32(w) for t, w in TERM_SETS[tname].items()}
        ref["oracle"][key] = ora.loss_and_grad(ref["out"], ref["tgt"], terms, _f32(EPS), zero_mean, parts=True)
    return ref["oracle"][key]


def _dev(ref):
    return torch.from_numpy(ref["out"]).cuda(), torch.from_numpy(ref["tgt"]).cuda()


def _cond(st, eps):
    """(cond_si, cond_snr) per row from the oracle's row statistics."""
    c = ora.K * st["n"] * 2.0 ** -50 * (st["See"] + st["P"])
    return c / (st["Nn"] + eps), c / (st["Dd"] + eps)


def loss_bounds(want, st, terms, S, B, eps):
    """The bound of every slot of `losses` (module docstring)."""
    csi, csn = _cond(st, eps)
    b = np.zeros_like(want)
    b[1], b[2] = 2.0 ** -22 * want[1], 2.0 ** -22 * want[2]
    if terms.get("si_sdr", 0) > 0:
        b[5:5 + S] = 2.0 ** -23 * np.abs(want[5:5 + S]) + csi.reshape(S, B).mean(1)
        b[3] = 2.0 ** -23 * abs(want[3]) + csi.mean()
    if terms.get("snr", 0) > 0:
        b[5 + S:] = 2.0 ** -23 * np.abs(want[5 + S:]) + csn.reshape(S, B).mean(1)
        b[4] = 2.0 ** -23 * abs(want[4]) + csn.mean()
    b[0] = 2.0 ** -23 * abs(want[0]) + sum(_f32(terms.get(t, 0.0)) * b[1 + i] for i, t in enumerate(ora.TERMS))
    return b


def grad_bound(parts, terms, shape, eps):
    S, B = shape[:2]
    csi, csn = _cond(parts["rows"], eps)
    cond = (csi if terms.get("si_sdr", 0) > 0 else 0.0) + (csn if terms.get("snr", 0) > 0 else 0.0)
    cond = np.broadcast_to(np.asarray(cond, np.float64).reshape(-1, 1), (S * B, parts["v"].size // (S * B))).reshape(shape)
    return C_ROUND * 2.0 ** -24 * (np.abs(parts["mse"]) + np.abs(parts["l1"]) + np.abs(parts["v"])) + cond * np.abs(parts["v"])


def _check_losses(tag, got, want, bound):
    got = np.asarray(got, np.float64)
    for i in range(len(want)):
        if bound[i] == 0:
            assert got[i] == want[i] == 0, (tag, i, got[i], want[i])
            continue
        record(tag, "slot %d err / bound" % i, abs(got[i] - want[i]) / bound[i], 1.0)
        assert abs(got[i] - want[i]) <= bound[i], (tag, i, got[i], want[i], bound[i])


# ---------------------------------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("zero_mean", [True, False])
@pytest.mark.parametrize("tname", sorted(TERM_SETS))
@pytest.mark.parametrize("name", sorted(CASES))
def test_values_and_gradient_against_float64(lib, name, tname, zero_mean):
    ref = _case(name)
    S, B = CASES[name][:2]
    want, g_want, parts = _oracle(ref, tname, zero_mean)
    out, tgt = _dev(ref)
    losses, g = waveform.WaveformLoss(TERM_SETS[tname], EPS, zero_mean).loss_and_grad(out, tgt)
    tag = "waveform::test_values_and_gradient_against_float64[%s-%s-%s]" % (name, tname, zero_mean)
    assert losses.shape == (5 + 2 * S,)
    _check_losses(tag, losses.cpu().numpy(), want, loss_bounds(want, parts["rows"], TERM_SETS[tname], S, B, _f32(EPS)))
    err = np.abs(g.cpu().numpy().astype(np.float64) - g_want)
    bound = grad_bound(parts, TERM_SETS[tname], ref["out"].shape, _f32(EPS))
    live = bound > 0
    assert np.all(err[~live] == 0)
    record(tag, "gradient max err / bound", (err[live] / bound[live]).max(), 1.0)
    assert np.all(err <= bound)
    # d_outputs = NULL leaves the same losses
    l2, none = waveform.WaveformLoss(TERM_SETS[tname], EPS, zero_mean).loss_and_grad(out, tgt, grad=False)
    assert none is None and torch.equal(l2, losses)


# ---------------------------------------------------------------------------------------------------- 2. bit ties
@pytest.mark.parametrize("w", [1.0, 0.37])
@pytest.mark.parametrize("name", sorted(CASES))
def test_mse_alone_is_the_spectral_entry(lib, name, w):
    out, tgt = _dev(_case(name))
    ls, gs = spectral.SpectralLoss([], mse_weight=w).loss_and_grad(out, tgt)
    lw, gw = waveform.WaveformLoss({"mse": w}).loss_and_grad(out, tgt)
    assert torch.equal(lw[:2], ls[:2]) and torch.equal(gw, gs)
    assert ls[0].item() != 0


@pytest.mark.parametrize("tname", ["mse", "all"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_accumulate_is_one_fp32_add(lib, name, tname):
    out, tgt = _dev(_case(name))
    loss = waveform.WaveformLoss(TERM_SETS[tname])
    l0, fresh = loss.loss_and_grad(out, tgt)
    old = torch.randn(out.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    acc, l1 = old.clone(), torch.empty_like(l0)
    loss.run(out, tgt, acc, l1, loss._scratch_for(out), accumulate=True)
    assert torch.equal(acc, old + fresh) and torch.equal(l0, l1)


# ---------------------------------------------------------------------------------------------------- 3. independence
@pytest.mark.parametrize("name", sorted(CASES))
def test_reproducible_bits(lib, name):
    out, tgt = _dev(_case(name))
    loss = waveform.WaveformLoss(ALL)
    l0, g0 = loss.loss_and_grad(out, tgt)
    l1, g1 = loss.loss_and_grad(out, tgt)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    for fill in (float("nan"), 0.0):
        scratch = torch.full((loss.scratch_floats(out.shape),), fill, dtype=torch.float32, device="cuda")
        g2, l2 = torch.full_like(out, float("nan")), torch.full_like(l0, float("nan"))
        loss.run(out, tgt, g2, l2, scratch)
        assert torch.equal(l0, l2) and torch.equal(g0, g2)
    # every buffer 4 bytes off an 8-byte boundary
    g3, l3 = _offset_copy(torch.full_like(out, float("nan"))), _offset_copy(torch.full_like(l0, float("nan")))
    scratch = _offset_copy(torch.full((loss.scratch_floats(out.shape),), float("nan"), dtype=torch.float32, device="cuda"))
    loss.run(_offset_copy(out), _offset_copy(tgt), g3, l3, scratch)
    assert torch.equal(l0, l3) and torch.equal(g0, g3)


@pytest.mark.parametrize("tname", ["si_sdr", "snr"])
def test_a_row_does_not_depend_on_the_others(lib, tname):
    """R = 4 is a power of two: the 1 / R of the row coefficients scales a row's gradient exactly."""
    out, tgt = _dev(_case("10000"))
    loss = waveform.WaveformLoss(TERM_SETS[tname])
    lf, gf = loss.loss_and_grad(out, tgt)
    for s in range(2):
        for b in range(2):
            l1, g1 = loss.loss_and_grad(out[s:s + 1, b:b + 1].contiguous(), tgt[s:s + 1, b:b + 1].contiguous())
            assert torch.equal(gf[s, b], g1[0, 0] * 0.25), (s, b)
    # and a source's dB is the mean of its rows' alone
    alone = [[loss.loss_and_grad(out[s:s + 1, b:b + 1].contiguous(), tgt[s:s + 1, b:b + 1].contiguous())[0] for b in range(2)]
             for s in range(2)]
    slot = 5 if tname == "si_sdr" else 6
    for s in range(2):
        want = (alone[s][0][slot].double() + alone[s][1][slot].double()) / 2
        got = loss.source_metrics(lf)[tname][s].double()
        assert abs(got.item() - want.item()) <= 2.0 ** -22 * abs(want.item())


# ---------------------------------------------------------------------------------------------------- 4. exact cases
@pytest.mark.parametrize("name", ["330", "2049", "10000"])
def test_exact_cases(lib, name):
    ref = _case(name)
    S, B = CASES[name][:2]
    out, tgt = _dev(ref)
    eps = _f32(EPS)
    tag = "waveform::test_exact_cases[%s]" % name
    # estimates bit-equal to the targets
    l, g = waveform.WaveformLoss({"mse": 1.0, "l1": 1.0}).loss_and_grad(tgt.clone(), tgt)
    assert l[0].item() == 0 and l[1].item() == 0 and l[2].item() == 0 and not g.any()
    l, g = waveform.WaveformLoss({"si_sdr": 1.0, "snr": 1.0}).loss_and_grad(tgt.clone(), tgt)
    assert torch.isfinite(l).all() and torch.isfinite(g).all()
    st = ora.row_stats(ref["tgt"], ref["tgt"], eps, True)
    csi, csn = _cond(st, eps)
    got = l.cpu().numpy().astype(np.float64)
    want_si = (10 * np.log10(st["Stt"] / (2 * eps))).reshape(S, B).mean(1)
    want_snr = (10 * np.log10((st["Stt"] + eps) / eps)).reshape(S, B).mean(1)
    b_si = 2.0 ** -23 * np.abs(want_si) + csi.reshape(S, B).mean(1)
    b_snr = 2.0 ** -23 * np.abs(want_snr) + csn.reshape(S, B).mean(1)
    record(tag, "equal inputs: SI err / bound", (np.abs(got[5:5 + S] - want_si) / b_si).max(), 1.0)
    record(tag, "equal inputs: SNR err / bound", (np.abs(got[5 + S:] - want_snr) / b_snr).max(), 1.0)
    assert np.all(np.abs(got[5:5 + S] - want_si) <= b_si) and np.all(np.abs(got[5 + S:] - want_snr) <= b_snr)
    # zero estimates: the si_sdr gradient is exactly 0
    for zm in (True, False):
        l, g = waveform.WaveformLoss({"si_sdr": 1.0}, zero_mean=zm).loss_and_grad(torch.zeros_like(tgt), tgt)
        assert torch.isfinite(l).all() and not g.any()
    # a row whose target is all zero: every slot finite and the oracle's
    silent = ref["tgt"].copy()
    silent[-1, -1] = 0
    for zm in (True, False):
        terms = {t: _f32(w) for t, w in ALL.items()}
        want, g_want, parts = ora.loss_and_grad(ref["out"], silent, terms, eps, zm, parts=True)
        l, g = waveform.WaveformLoss(ALL, EPS, zm).loss_and_grad(out, torch.from_numpy(silent).cuda())
        assert torch.isfinite(l).all() and torch.isfinite(g).all()
        _check_losses(tag + "[silent-%s]" % zm, l.cpu().numpy(), want, loss_bounds(want, parts["rows"], ALL, S, B, eps))
        assert np.all(np.abs(g.cpu().numpy().astype(np.float64) - g_want) <= grad_bound(parts, ALL, silent.shape, eps))
        if not zm:                                          # the header's closed form of a silent target row
            See = (ref["out"][-1, -1].astype(np.float64) ** 2).sum()
            assert abs(parts["rows"]["SI"][-1] - 10 * np.log10(eps / (See + eps))) < 1e-9
    # a term of weight 0 reports 0, and the other slots do not change by a bit whether it is 0 or absent -- nor when another
    # term joins: the slots of si_sdr are the same bits with snr beside it
    la, ga = waveform.WaveformLoss({"l1": 1.0, "si_sdr": 0.05}).loss_and_grad(out, tgt)
    lb, gb = waveform.WaveformLoss({"mse": 0.0, "l1": 1.0, "si_sdr": 0.05, "snr": 0.0}).loss_and_grad(out, tgt)
    assert torch.equal(la, lb) and torch.equal(ga, gb)
    assert la[1].item() == 0 and la[4].item() == 0 and not la[5 + S:].any()
    lc, _ = waveform.WaveformLoss({"l1": 1.0, "si_sdr": 0.05, "snr": 0.5}).loss_and_grad(out, tgt)
    assert torch.equal(lc[2:4], la[2:4]) and torch.equal(lc[5:5 + S], la[5:5 + S]) and lc[4].item() != 0


# ---------------------------------------------------------------------------------------------------- 5. through the layers
def _e2e_cfg(tmp, **over):
    """The smallest model config of the spectral Trainer tests."""
    return wun.get_config("full", num_layers=3, num_initial_filters=8, num_frames=200, batch_size=4, epoch_it=3,
                          model_base_dir=os.path.join(tmp, "ckpt"), log_dir=os.path.join(tmp, "logs"),
                          init_sup_sep_lr=1e-3, **over)


def _sep_and_batch(tmp):
    cfg = _e2e_cfg(tmp)
    sep = wun.UnetAudioSeparator(cfg, device="cuda:0", seed=5)
    i, o = sep.get_padding(np.array([4, cfg["num_frames"], 0]))
    mix, targets = training.synthetic_source(cfg, 4, int(i[1]), int(o[1]), torch.device("cuda:0"))()
    return cfg, sep, mix, targets


def _ranges_equal(sep, a, b):
    for name, off, shp in sep._active.tensors:
        n = int(np.prod(shp))
        assert torch.equal(a[off:off + n], b[off:off + n]), name


def test_loss_and_gradients_is_backward_from_the_gradient(lib, tmp_path):
    cfg, sep, mix, targets = _sep_and_batch(str(tmp_path))
    loss = waveform.WaveformLoss({"l1": 1.0, "si_sdr": 0.05})
    outs = sep.get_output(mix, True)
    stacked = torch.stack([outs[n] for n in cfg["source_names"]])
    losses, d_out = loss.loss_and_grad(stacked, targets)
    for kw in ({}, {"variables": ["separator/conv1d/kernel", "separator/conv1d/bias"]}):
        sep.grads.zero_()
        sep.get_output(mix, True)                           # (every backward pass follows a forward pass of its own)
        total = sep.loss_and_gradients(targets, loss=loss, **kw)
        got = sep.grads.clone()
        assert total.item() == losses[0].item() and torch.equal(sep.last_losses, losses)
        sep.get_output(mix, True)
        total = sep.loss_and_gradients(targets, loss=loss, accumulate=True, **kw)
        got2 = sep.grads.clone()
        sep.grads.zero_()
        sep.get_output(mix, True)
        sep.backward(d_out, **kw)
        _ranges_equal(sep, got, sep.grads)
        sep.get_output(mix, True)
        sep.backward(d_out, accumulate=True, **kw)
        _ranges_equal(sep, got2, sep.grads)
    # under autograd through module()
    sep.get_output(mix, True)
    sep.backward(d_out)
    want = sep.grads.clone()
    net = sep.module()
    y = net(mix)
    total = waveform.waveform_loss(y, targets, loss)
    (ga,) = torch.autograd.grad(total, [net.arena])
    assert total.item() == losses[0].item()
    _ranges_equal(sep, ga, want)
    assert loss(y.detach(), targets).item() == losses[0].item()
    assert waveform.waveform_loss(y.detach(), targets, terms={"l1": 1.0, "si_sdr": 0.05}).item() == losses[0].item()


def test_combined_loss(lib):
    out, tgt = _dev(_case("1400"))
    sp = spectral.SpectralLoss([(64, 48), (256, 64)], mse_weight=0.5, terms={"sc": 1.0, "log_mag_l1": 1.0})
    wv = waveform.WaveformLoss(ALL)
    both = waveform.CombinedLoss(sp, wv)
    ls, gs = sp.loss_and_grad(out, tgt)
    lw, gw = wv.loss_and_grad(out, tgt)
    l, g = both.loss_and_grad(out, tgt)
    assert both.num_losses == 1 + sp.num_losses + wv.num_losses == l.numel()
    a, b = both.parts(l)
    assert torch.equal(a, ls) and torch.equal(b, lw)
    assert torch.equal(l[0], ls[0] + lw[0]) and torch.equal(g, gs + gw)
    l2, none = both.loss_and_grad(out, tgt, grad=False)
    assert none is None and torch.equal(l2, l)
    x = out.clone().requires_grad_(True)
    both(x, tgt).backward()
    assert torch.equal(x.grad, g)


_WAVE_SPEC = {"terms": {"l1": 1, "si_sdr": 0.05}}
_SPEC_SPEC = {"resolutions": [[64, 48]], "mse_weight": 1.0, "terms": {"sc": 1, "log_mag_l1": 1}, "log_eps": 1e-3}


def test_trainer_waveform_loss(lib, tmp_path, monkeypatch):
    monkeypatch.setenv("WUN_NO_TUNE", "1")
    cfg = _e2e_cfg(str(tmp_path))
    tr = training.Trainer(cfg, waveform_loss=_WAVE_SPEC)
    assert tr.spectral is None and tr.waveform.terms["si_sdr"] == 0.05
    mix, targets = training.synthetic_source(cfg, tr.batch, tr.t_in, tr.t_out, tr.device)()
    first = tr.step(mix, targets).item()
    S = len(cfg["source_names"])
    assert tr.last_losses is None and tr.last_waveform_losses.shape == (5 + 2 * S,)
    parts = tr.waveform_parts()
    assert sorted(parts) == ["l1", "mse", "si_sdr", "si_sdr_db", "snr", "snr_db"] and parts["mse"] == 0 and parts["snr"] == 0
    assert abs(parts["l1"] + parts["si_sdr"] - first) <= 2.0 ** -21 * (abs(parts["l1"]) + abs(parts["si_sdr"]))
    assert len(parts["si_sdr_db"]) == S and abs(-0.05 * np.mean(parts["si_sdr_db"]) - parts["si_sdr"]) <= 1e-6 * abs(parts["si_sdr"])
    for _ in range(19):
        last = tr.step(mix, targets).item()
    assert np.isfinite(last) and last < first and tr.sep.global_step == 20

    # gradient accumulation reports the mean of the micro-batch slots
    ta = training.Trainer(cfg, waveform_loss=_WAVE_SPEC, grad_accum_steps=2)
    halves = []
    for lo in (0, 2):
        outs = ta.sep.get_output(mix[lo:lo + 2], True)
        halves.append(ta.waveform.loss_and_grad(torch.stack([outs[n] for n in cfg["source_names"]]), targets[:, lo:lo + 2])[0])
    got = ta.step(mix, targets)
    assert torch.equal(ta.last_waveform_losses, torch.stack(halves).mean(0)) and got.item() == ta.last_waveform_losses[0].item()

    # with a spectral loss too: the sum of the two totals; loss_parts() / term_parts() stay the spectral slice's
    tb = training.Trainer(cfg, spectral_loss=_SPEC_SPEC, waveform_loss=_WAVE_SPEC)
    ts = training.Trainer(cfg, spectral_loss=_SPEC_SPEC)
    total = tb.step(mix, targets)
    ts.step(mix, targets)
    assert torch.equal(tb.last_losses, ts.last_losses) and tb.loss_parts() == ts.loss_parts() and tb.term_parts() == ts.term_parts()
    assert tb.last_losses.shape == (7,) and tb.last_waveform_losses.shape == (5 + 2 * S,)
    assert torch.equal(total, tb.last_losses[0] + tb.last_waveform_losses[0])


def test_train_log_carries_the_waveform_terms(lib, tmp_path, monkeypatch):
    monkeypatch.setenv("WUN_NO_TUNE", "1")
    training.train(_e2e_cfg(str(tmp_path), waveform_loss=_WAVE_SPEC), "wave")
    log = [json.loads(l) for l in open(os.path.join(str(tmp_path), "logs", "wave", "train.jsonl"))]
    assert len(log) == 3
    for line in log:
        parts = line["waveform_terms"]
        assert "mse_loss" not in line and "spectral_loss" not in line
        assert abs(parts["l1"] + parts["si_sdr"] - line["sep_loss"]) <= 1e-6 * (abs(parts["l1"]) + abs(parts["si_sdr"]))
    training.train(_e2e_cfg(str(tmp_path)), "plain")
    plain = [json.loads(l) for l in open(os.path.join(str(tmp_path), "logs", "plain", "train.jsonl"))]
    assert all("waveform_terms" not in line for line in plain)


def test_validation_metric_si_sdr(lib, tmp_path):
    cfg = wun.get_config("baseline_stereo", num_layers=3, num_initial_filters=8, num_frames=40, batch_size=4,
                         num_snippets_per_track=6, cache_size=8, model_base_dir=os.path.join(str(tmp_path), "ckpt"),
                         log_dir=os.path.join(str(tmp_path), "logs"), validation_metric="si_sdr",
                         waveform_loss={"terms": {"l1": 1.0}, "eps": 1e-6})
    sep = wun.UnetAudioSeparator(cfg, seed=11)
    rng = np.random.default_rng(3)
    tracks = [datasets.make_track({k: (rng.uniform(-0.4, 0.4, (n, 2))).astype(np.float32) for k in cfg["source_names"]}, cfg)
              for n in (700, 900)]
    got = validation.test(cfg, "valid", "exp", None, tracks=tracks, separator=sep)
    in_shape, out_shape = sep.get_padding(np.array([cfg["batch_size"], cfg["num_frames"], 0]))
    names, eps = list(cfg["source_names"]), _f32(1e-6)
    total, bound, per, k = 0.0, 0.0, np.zeros(len(names)), 1
    for b in datasets.get_dataset(cfg, in_shape, out_shape, "valid", tracks):
        outs = sep.get_output(b["mix"], False)
        est = np.stack([outs[n].cpu().numpy() for n in names])
        real = np.stack([np.asarray(b[n]) for n in names])
        want, _, parts = ora.loss_and_grad(est, real, {"si_sdr": 1.0}, eps, True, parts=True)
        bnd = loss_bounds(want, parts["rows"], {"si_sdr": 1.0}, est.shape[0], est.shape[1], eps)
        total += (want[0] - total) / k
        bound += (bnd[0] - bound) / k
        per += (want[5:5 + len(names)] - per) / k
        k += 1
    assert k > 2
    record("waveform::test_validation_metric_si_sdr", "err / bound", abs(got - total) / bound, 1.0)
    assert abs(got - total) <= bound and abs(got + per.mean()) <= 1e-4 * abs(got) + bound
    line = json.loads(open(os.path.join(cfg["log_dir"], "exp", "test.jsonl")).read().splitlines()[-1])
    assert line["metric"] == "si_sdr" and line["test_loss"] == got and sorted(line["si_sdr_db"]) == sorted(names)
    for i, n in enumerate(names):
        assert abs(line["si_sdr_db"][n] - per[i]) <= 2.0 ** -22 * abs(per[i]) + bound
    # "mse" keeps today's record
    mse = validation.test(dict(cfg, validation_metric="mse"), "valid", "exp", None, tracks=tracks, separator=sep)
    line = json.loads(open(os.path.join(cfg["log_dir"], "exp", "test.jsonl")).read().splitlines()[-1])
    assert sorted(line) == ["global_step", "partition", "test_loss"] and line["test_loss"] == mse and mse > 0
