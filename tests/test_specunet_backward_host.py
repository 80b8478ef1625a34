"""CPU-only checks of the spectrogram U-Net's backward pass from any upstream gradient: the float64 oracle
tests/_specunet_backward_np.py against torch.autograd -- through torch.fft.irfft, an overlap-add, the division by D and
test_specunet_train_host.py's differentiable network -- against _specunet_train_np.loss_and_gradients for Jansson's L1, the scratch
formulas, and every refusal of the new entries and of the Python surfaces, each before any GPU work."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _specunet_np as ora  # noqa: E402
import _specunet_train_np as tro  # noqa: E402
import _specunet_backward_np as bo  # noqa: E402

import wave_u_net_amd as wun  # noqa: E402
from wave_u_net_amd import _lib, spectrogram, training  # noqa: E402
from wave_u_net_amd.spectrogram import UnetSpectrogramSeparator  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("wun_spec_train_audio_scratch_floats", "wun_spec_train_audio", "wun_spec_backward_scratch_floats", "wun_spec_backward",
               "wun_spec_update_moving_averages", "wun_op_spec_head_backward_scratch", "wun_op_spec_head_backward")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the oracle against autograd
def _istft_tf_autograd(z, n_fft, hop):
    """ISTFT_tf written independently of _specunet_np.istft_tf: irfft, the window, an overlap-add by index_add, then the division
    by D[t mod hop]."""
    B, F, K = z.shape
    T = (F - 1) * hop + n_fft
    frames = torch.fft.irfft(z, n=n_fft, dim=-1) * ora.hann(n_fft)
    idx = (torch.arange(F)[:, None] * hop + torch.arange(n_fft)[None, :]).reshape(-1)
    y = torch.zeros((B, T), dtype=torch.float64).index_add(1, idx, frames.reshape(B, -1))
    w2 = ora.hann(n_fft) ** 2
    D = torch.stack([w2[p::hop].sum() for p in range(hop)])
    return y / D[torch.arange(T) % hop]


def _autograd_outputs(fx, masks):
    """(variables with requires_grad, mags [S, B, F, K], audio [S, B, T]) under torch.autograd: the network of
    test_specunet_train_host.py::_autograd, the library's batch norm."""
    Fn = torch.nn.functional
    L, n_fft, hop = fx["L"], fx["n_fft"], fx["hop"]
    v = {k: torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=not k.split("/")[-1].startswith("moving"))
         for k, a in fx["variables"].items()}
    X = ora.stft(torch.tensor(fx["mix"], dtype=torch.float64), n_fft, hop)
    M = X.abs()
    B, F, K = M.shape
    a0 = torch.log1p(M[:, :, :-1, None])

    def bn(z, beta):
        return Fn.batch_norm(z.permute(0, 3, 1, 2), None, None, None, beta, True, 0.0, ora.BN_EPS).permute(0, 2, 3, 1)

    mags, audio = [], []
    for s in range(2):
        down, up = tro.names(L, s)
        cur, enc = a0, []
        for i in range(L):
            cur = Fn.leaky_relu(bn(ora.conv2d_s2(cur, v[down[i][0] + "/kernel"]) + v[down[i][0] + "/bias"], v[down[i][1] + "/beta"]), 0.2)
            enc.append(cur)
        for i in range(L):
            if i > 0:
                cur = torch.cat([enc[L - 1 - i], cur], dim=3)
                if masks is not None and (s, i - 1) in masks:
                    cur = cur * torch.tensor(masks[(s, i - 1)], dtype=torch.float64)
            z = ora.conv2d_transpose_s2(cur, v[up[i][0] + "/kernel"]) + v[up[i][0] + "/bias"]
            cur = torch.relu(bn(z, v[up[i][1] + "/beta"])) if i < L - 1 else torch.sigmoid(z)[..., 0]
        mask = torch.cat([cur, torch.full((B, F, 1), 0.5, dtype=torch.float64)], dim=2)
        mags.append(M * mask)
        audio.append(_istft_tf_autograd(mask * X, n_fft, hop))
    return v, torch.stack(mags), torch.stack(audio)


def _same(grads, floors, want, tol=1e-10):
    for k, g in want.items():
        scale = max(float(g.abs().max()), floors[k])
        assert grads[k].shape == g.shape, k
        assert float((grads[k] - g).abs().max()) <= tol * scale, (k, float((grads[k] - g).abs().max()), scale)
    for k in grads:
        if k.split("/")[-1].startswith("moving"):
            assert float(grads[k].abs().max()) == 0.0


def _forward64(fx, rate):
    masks = tro.fixture_masks(fx, rate)
    return masks, tro.train_forward(fx["mix"], fx["variables"], fx["L"], fx["nif"], fx["n_fft"], fx["hop"], masks)


@pytest.mark.parametrize("domain", ["mags", "audio", "both"])
@pytest.mark.parametrize("name", ["skip", "flat", "five", "flat_b1"])
def test_oracle_is_autograd(name, domain):
    """Random upstream gradients: sum(d_mags mags) + sum(d_audio audio) differentiated by autograd."""
    fx = tro.fixture(name)
    masks, fw = _forward64(fx, 0.5)
    v, mags, audio = _autograd_outputs(fx, masks)
    rng = np.random.RandomState(3)
    d_mags = torch.tensor(rng.randn(*mags.shape)) if domain != "audio" else None
    d_audio = torch.tensor(rng.randn(*audio.shape)) if domain != "mags" else None
    got_audio = torch.stack(bo.audio_output(fw, fx["mix"], fx["n_fft"], fx["hop"]))
    assert float((got_audio - audio.detach()).abs().max()) <= 1e-12 * float(audio.detach().abs().max())
    assert float((torch.stack(fw["mags"]) - mags.detach()).abs().max()) <= 1e-12 * float(mags.detach().abs().max())
    obj = (0 if d_mags is None else (d_mags * mags).sum()) + (0 if d_audio is None else (d_audio * audio).sum())
    names = [k for k in v if v[k].requires_grad]
    want = dict(zip(names, torch.autograd.grad(obj, [v[k] for k in names])))
    grads, floors, _ = bo.gradients(fw, fx["mix"], fx["n_fft"], fx["hop"], d_mags=d_mags, d_audio=d_audio)
    assert set(grads) == set(fx["variables"])
    _same(grads, floors, want)


@pytest.mark.parametrize("n_fft, hop, F", [(64, 48, 8), (64, 16, 33), (256, 64, 5), (1024, 768, 3)])
def test_head_is_autograd(n_fft, hop, F):
    """The head alone at the GPU test's resolutions: dz against autograd through the sigmoid, M mask and ISTFT_tf(mask X)."""
    rng = np.random.RandomState(n_fft + hop)
    B, K, T = 2, n_fft // 2 + 1, (F - 1) * hop + n_fft
    X = ora.stft(torch.tensor(rng.randn(B, T)), n_fft, hop)
    M = X.abs()
    z = torch.tensor(rng.randn(B, F, K - 1), requires_grad=True)
    mask = torch.sigmoid(z)
    full = torch.cat([mask, torch.full((B, F, 1), 0.5, dtype=torch.float64)], dim=2)
    d_mags, d_audio = torch.tensor(rng.randn(B, F, K)), torch.tensor(rng.randn(B, T))
    for dm, da in ((d_mags, None), (None, d_audio), (d_mags, d_audio)):
        obj = (0 if dm is None else (dm * M * full).sum()) + (0 if da is None else (da * _istft_tf_autograd(full * X, n_fft, hop)).sum())
        (want,) = torch.autograd.grad(obj, z, retain_graph=True)
        dz, scale = bo.head(X, M, mask.detach(), dm, da, n_fft, hop)
        assert scale > 0 and float((dz - want).abs().max()) <= 1e-10 * max(float(want.abs().max()), scale)


@pytest.mark.parametrize("name", ["skip", "five", "flat_b1"])
def test_l1_upstream_gives_the_magnitude_objective(name):
    fx = tro.fixture(name)
    _, fw = _forward64(fx, 0.5)
    _, _, want, floors, _ = tro.loss_and_gradients(fw, fx["targets"], fx["n_fft"], fx["hop"])
    grads, floors2, _ = bo.gradients(fw, fx["mix"], fx["n_fft"], fx["hop"], d_mags=bo.l1_upstream(fw, fx["targets"], fx["n_fft"], fx["hop"]))
    assert set(grads) == set(want)
    for k, g in want.items():
        if k in floors:
            assert float((grads[k] - g).abs().max()) <= 1e-14 * floors[k] and abs(floors2[k] - floors[k]) <= 1e-12 * floors[k], k
        else:                                                # the moving statistics
            assert float(grads[k].abs().max()) == 0.0 and float(g.abs().max()) == 0.0, k


@pytest.mark.parametrize("name", ["skip", "flat"])
def test_mse_upstream_is_the_raw_audio_objective(name):
    """Training.py:62-63: the mean over the sources of the MSE through inverse_stft, differentiated by autograd."""
    fx = tro.fixture(name)
    masks, fw = _forward64(fx, 0.5)
    v, _, audio = _autograd_outputs(fx, masks)
    tg = torch.tensor(fx["targets"], dtype=torch.float64)
    want_loss = sum(((audio[s] - tg[s]) ** 2).mean() for s in range(2)) / 2.0
    names = [k for k in v if v[k].requires_grad]
    want = dict(zip(names, torch.autograd.grad(want_loss, [v[k] for k in names])))
    loss, d_audio = bo.mse_upstream(bo.audio_output(fw, fx["mix"], fx["n_fft"], fx["hop"]), fx["targets"])
    assert abs(loss - float(want_loss.detach())) <= 1e-12 * float(want_loss.detach())
    grads, floors, _ = bo.gradients(fw, fx["mix"], fx["n_fft"], fx["hop"], d_audio=d_audio)
    _same(grads, floors, want)


# ------------------------------------------------------------------------------------------------ the C ABI, host side
def test_new_symbols_are_declared_bound_documented_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "wun.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert "`%s`" % name in doc, name
    assert "DIVIDES by the rounded D" in hdr              # the statement the oracle follows


def _spec(L=2, nif=3, S=2, n_fft=64, hop=48):
    return _lib.WunSpecConfig(L, nif, S, n_fft, hop)


def _tc(decay=0.999, rate=0.5, seed=1):
    return _lib.WunSpecTrainConfig(decay, rate, seed)


def _ceil4(n):
    return (n + 3) // 4 * 4


@pytest.mark.parametrize("L, n_fft, hop, F, B", [(2, 64, 48, 8, 2), (1, 64, 48, 2, 1), (5, 64, 48, 32, 2), (2, 64, 16, 36, 3),
                                                 (2, 1024, 768, 4, 1)])
def test_scratch_formulas(lib, L, n_fft, hop, F, B):
    c, T, K = _spec(L=L, n_fft=n_fft, hop=hop), (F - 1) * hop + n_fft, n_fft // 2 + 1
    assert lib.wun_spec_backward_scratch_floats(C.byref(c), B, T) == _ceil4(hop) + B * T
    inverse = lib.wun_istft_tf_fft_scratch_floats(2, B, T, 1, n_fft, hop, F)
    assert inverse > 0
    assert lib.wun_spec_train_audio_scratch_floats(C.byref(c), B, T) == 2 * _ceil4(2 * B * F * K) + inverse
    assert lib.wun_op_spec_head_backward_scratch(B, T, n_fft, hop) == _ceil4(hop) + B * T


def test_scratch_queries_refuse(lib):
    c, T = _spec(), 7 * 48 + 64
    for q in (lib.wun_spec_backward_scratch_floats, lib.wun_spec_train_audio_scratch_floats):
        assert q(None, 2, T) == -1 and q(C.byref(c), 0, T) == -1 and q(C.byref(c), 2, T - 48) == -1 and q(C.byref(c), 2, T + 1) == -1
        assert q(C.byref(_spec(n_fft=96)), 2, 7 * 48 + 96) in (-1, -2)                   # n_fft outside the list
        assert q(C.byref(_spec(hop=64)), 2, 3 * 64 + 64) == -2                           # D[0] = w[0]^2 = 0: wun_istft_tf_fft refuses
        assert b"window-square" in lib.wun_last_error()
    op = lib.wun_op_spec_head_backward_scratch
    assert op(0, T, 64, 48) == -1 and op(2, T + 1, 64, 48) == -1 and op(2, 32, 64, 48) == -1
    assert op(2, 96 + 48, 96, 48) == -2 and op(2, 16384 + 48, 16384, 48) == -2           # n_fft outside 64..8192
    assert op(2, 128, 64, 0) == -1 and op(2, 128, 64, 65) == -1                          # hop outside 1..n_fft
    assert op(2, 128, 64, 64) == -2


def test_entries_refuse_before_any_gpu_work(lib):
    """Every refusal below returns before the first launch, so the fake (never dereferenced) pointers are safe without a GPU."""
    c, T, B = _spec(), 7 * 48 + 64, 1
    ws_n = lib.wun_spec_train_workspace_floats(C.byref(c), B, T)
    sc_n = max(lib.wun_spec_backward_scratch_floats(C.byref(c), B, T), lib.wun_spec_train_audio_scratch_floats(C.byref(c), B, T))
    ws = C.c_void_p(256)
    sc = C.c_void_p(256 + 4 * (ws_n + 64))
    q = [C.c_void_p(sc.value + 4 * (sc_n + 64) + (i + 1) * (1 << 24)) for i in range(6)]
    t, cr, tr = _tc(), C.byref(c), C.byref(_tc())
    params, dm, da, table, grads, audio = q

    bwd = lib.wun_spec_backward
    ok = [cr, tr, params, dm, da, B, T, table, grads, ws, sc, None]
    for i in (0, 1, 2, 7, 8, 9, 10):                                                     # null arguments
        a = list(ok)
        a[i] = None
        assert bwd(*a) == -1 and b"null" in lib.wun_last_error(), i
    a = list(ok); a[3] = a[4] = None
    assert bwd(*a) == -1 and b"both null" in lib.wun_last_error()
    for bad_T in (T + 1, T - 48, 32):                                                    # the shape conditions
        a = list(ok); a[6] = bad_T
        assert bwd(*a) == -1
    a = list(ok); a[5] = 0
    assert bwd(*a) == -1
    for bad in (_tc(rate=1.0), _tc(rate=float("nan")), _tc(decay=1.5), _tc(decay=float("nan"))):
        a = list(ok); a[1] = C.byref(bad)
        assert bwd(*a) == -1
        assert lib.wun_spec_train_audio(cr, C.byref(bad), B, T, table, audio, ws, sc, None) == -1
        assert lib.wun_spec_update_moving_averages(cr, C.byref(bad), params, ws, B, T, None) == -1
    # each overlap: (argument index, the buffer it is put on)
    for i, j in ((2, 9), (3, 9), (4, 9), (8, 9), (10, 9), (2, 10), (3, 10), (4, 10), (8, 10), (8, 2), (3, 8), (4, 8)):
        a = list(ok); a[i] = ok[j]
        assert bwd(*a) == -1 and b"overlap" in lib.wun_last_error(), (i, j)
    for only in (3, 4):                                                                  # one gradient alone: the same checks
        a = list(ok); a[only] = None; a[7 - only] = ws
        assert bwd(*a) == -1 and b"overlap" in lib.wun_last_error()
    a = list(ok); a[0] = C.byref(_spec(n_fft=96)); a[6] = 7 * 48 + 96
    assert bwd(*a) in (-1, -2)
    a = list(ok); a[0] = C.byref(_spec(hop=64)); a[6] = 3 * 64 + 64
    assert bwd(*a) == -2

    aud = lib.wun_spec_train_audio
    ok = [cr, tr, B, T, table, audio, ws, sc, None]
    for i in (0, 1, 4, 5, 6, 7):
        a = list(ok); a[i] = None
        assert aud(*a) == -1, i
    a = list(ok); a[3] = T + 1
    assert aud(*a) == -1
    for i, j in ((5, 6), (7, 6), (5, 7)):
        a = list(ok); a[i] = ok[j]
        assert aud(*a) == -1 and b"overlap" in lib.wun_last_error(), (i, j)
    assert aud(C.byref(_spec(hop=64)), tr, B, 3 * 64 + 64, table, audio, ws, sc, None) == -2

    mov = lib.wun_spec_update_moving_averages
    assert mov(None, tr, params, ws, B, T, None) == -1 and mov(cr, None, params, ws, B, T, None) == -1
    assert mov(cr, tr, None, ws, B, T, None) == -1 and mov(cr, tr, params, None, B, T, None) == -1
    assert mov(cr, tr, params, ws, B, T + 1, None) == -1 and mov(cr, tr, ws, ws, B, T, None) == -1

    op = lib.wun_op_spec_head_backward
    re_, im_, mag, mask, dz = q[0], q[1], q[2], q[3], q[4]
    dmo, dao = C.c_void_p(q[5].value + (1 << 24)), C.c_void_p(q[5].value + (2 << 24))
    ok = [re_, im_, mag, mask, dmo, dao, B, T, 64, 48, table_far(q), dz, sc, None]
    for i in (0, 1, 2, 3, 10, 11, 12):
        a = list(ok); a[i] = None
        assert op(*a) == -1, i
    a = list(ok); a[4] = a[5] = None
    assert op(*a) == -1 and b"both null" in lib.wun_last_error()
    a = list(ok); a[7] = T + 1
    assert op(*a) == -1
    a = list(ok); a[8] = 96; a[7] = 7 * 48 + 96
    assert op(*a) == -2
    a = list(ok); a[9] = 64; a[7] = 3 * 64 + 64
    assert op(*a) == -2
    for i in (0, 1, 2, 3, 4, 5):                                                         # an operand on the scratch, then on dz
        for j in (12, 11):
            a = list(ok); a[i] = ok[j]
            assert op(*a) == -1 and b"overlap" in lib.wun_last_error(), (i, j)
    a = list(ok); a[11] = ok[12]
    assert op(*a) == -1 and b"overlap" in lib.wun_last_error()


def table_far(q):
    return C.c_void_p(q[5].value + (3 << 24))


# ------------------------------------------------------------------------------------------------ the Python side
def _cfg(**kw):
    base = dict(num_layers=2, num_initial_filters=3, spec_frame_len=64, spec_hop=48, num_frames=7 * 48 + 64, batch_size=2)
    base.update(kw)
    return wun.get_config("unet_spectrogram_l1", **base)


def test_python_refusals():
    T = 7 * 48 + 64
    sep = UnetSpectrogramSeparator(_cfg(), device="cpu")       # (a host-side separator: every refusal comes before any GPU work)
    for call in (sep.audio_output, lambda: sep.backward(d_audio=np.zeros((2, 2, T, 1), np.float32)), sep.update_moving_averages):
        with pytest.raises(RuntimeError, match="first"):
            call()
    with pytest.raises(ValueError, match='"audio", "mags" or "both"'):
        sep.module(output="x")
    sep._last_train = (2, T)                                  # as after a training forward
    with pytest.raises(ValueError, match="d_mags, d_audio or both"):
        sep.backward()
    with pytest.raises(ValueError, match="d_audio must be"):
        sep.backward(d_audio=np.zeros((2, 2, T), np.float32))
    with pytest.raises(ValueError, match="d_mags must be"):
        sep.backward(d_mags=np.zeros((2, 2, 8, 32), np.float32))
    with pytest.raises(ValueError, match="d_mags must be"):
        sep.backward(d_mags={k: np.zeros((2, 9, 33), np.float32) for k in sep.source_names})
    net = sep.module("both")
    assert isinstance(net, spectrogram.SpecUNet) and net.arena.data_ptr() == sep.params.data_ptr() and net.dropout_step == 0
    assert set(net.named_variables()) == {n for n, _, _ in sep.variable_table()} and net.variable_grads() is None
    with pytest.raises(NotImplementedError, match="gradient with respect to the mix"):
        net(torch.zeros((2, T, 1), requires_grad=True))
    with pytest.raises(ValueError, match="mono"):
        net(torch.zeros((2, T, 2)))
    with pytest.raises(ValueError):
        net(torch.zeros((2, T + 1, 1)))


def test_the_pinned_refusals_are_still_raised(monkeypatch):
    """This pull request delivers training on any loss through new surfaces; the four earlier refusals stay as they were."""
    T = 7 * 48 + 64
    sep = UnetSpectrogramSeparator(_cfg())
    with pytest.raises(NotImplementedError, match="inference only"):                     # 1: get_output's own audio at training
        sep.get_output(np.zeros((1, T, 1), np.float32), True)
    with pytest.raises(NotImplementedError, match="inference only"):                     # 2: the trainer's raw-audio objective
        training.train(dict(_cfg(), raw_audio_loss=True), 1)
    for key, value in (("spectral_loss", {"resolutions": [[64, 16]], "weights": [1.0], "mse_weight": 0.0}),
                       ("waveform_loss", {"terms": {"l1": 1.0}}), ("grad_accum_steps", 2), ("clip_grad_norm", 1.0),
                       ("skip_nonfinite_steps", True)):                                  # 4: the trainer's other keys
        with pytest.raises(NotImplementedError, match=key):
            training.train(dict(_cfg(), **{key: value}), 1)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="world > 1"):
        training.train(_cfg(), 1)


def test_the_cli_still_refuses_the_raw_audio_config(tmp_path):
    """3: python -m wave_u_net_amd train with cfg.unet_spectrogram, as a child process."""
    cmd = [sys.executable, "-m", "wave_u_net_amd", "train", "with", "cfg.unet_spectrogram", "synthetic=1", "experiment_id=7",
           "model_config.num_layers=2", "model_config.num_initial_filters=3", "model_config.spec_frame_len=64",
           "model_config.spec_hop=48", "model_config.num_frames=%d" % (7 * 48 + 64), "model_config.batch_size=2",
           "model_config.epoch_it=1", "model_config.log_dir=%s" % (tmp_path / "logs"), "model_config.model_base_dir=%s" % (tmp_path / "ck")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "inference only" in r.stderr
