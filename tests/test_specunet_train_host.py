"""CPU-only checks of the spectrogram U-Net's training step: the float64 oracle tests/_specunet_train_np.py
against torch.autograd and independent restatements, the fixtures' distance from the kinks, and the host side of the new
entries -- symbols, struct sizes and every refusal, each before any GPU work."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _specunet_np as ora  # noqa: E402
import _specunet_train_np as tro  # noqa: E402

import wave_u_net_amd as wun  # noqa: E402
from wave_u_net_amd import _lib, training  # noqa: E402
from wave_u_net_amd.spectrogram import UnetSpectrogramSeparator  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the oracle against autograd
def _autograd(fx, masks):
    """loss and gradients by torch.autograd over _specunet_np.py's differentiable convs and the library's batch norm."""
    Fn = torch.nn.functional
    L, n_fft, hop = fx["L"], fx["n_fft"], fx["hop"]
    v = {k: torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=not k.split("/")[-1].startswith("moving"))
         for k, a in fx["variables"].items()}
    x = torch.tensor(fx["mix"], dtype=torch.float64)
    tg = torch.tensor(fx["targets"], dtype=torch.float64)
    M = ora.stft(x, n_fft, hop).abs()
    B, F, K = M.shape
    a0 = torch.log1p(M[:, :, :-1, None])

    def bn(z, beta):
        return Fn.batch_norm(z.permute(0, 3, 1, 2), None, None, None, beta, True, 0.0, ora.BN_EPS).permute(0, 2, 3, 1)

    loss = 0
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
        loss = loss + (ora.stft(tg[s], n_fft, hop).abs() - M * mask).abs().mean()
    loss = loss / 2.0
    names = [k for k in v if v[k].requires_grad]
    return loss, dict(zip(names, torch.autograd.grad(loss, [v[k] for k in names])))


@pytest.mark.parametrize("rate", [0.0, 0.5])
@pytest.mark.parametrize("name", ["skip", "flat", "five", "flat_b1"])
def test_oracle_is_autograd(name, rate):
    fx = tro.fixture(name)
    masks = tro.fixture_masks(fx, rate)
    fw = tro.train_forward(fx["mix"], fx["variables"], fx["L"], fx["nif"], fx["n_fft"], fx["hop"], masks)
    loss, per, grads, floors, _ = tro.loss_and_gradients(fw, fx["targets"], fx["n_fft"], fx["hop"])
    want_loss, want = _autograd(fx, masks)
    want_loss = want_loss.detach()
    assert abs(float(loss) - float(want_loss)) <= 1e-12 * float(want_loss)
    assert abs(float(sum(per)) / 2 - float(loss)) <= 1e-15
    assert set(want) | {k for k in fx["variables"] if k.split("/")[-1].startswith("moving")} == set(grads) == set(fx["variables"])
    for k, g in want.items():
        scale = max(float(g.abs().max()), floors[k])
        assert grads[k].shape == g.shape, k
        assert float((grads[k] - g).abs().max()) <= 1e-10 * scale, (k, float((grads[k] - g).abs().max()), scale)
    for k in grads:
        if k.split("/")[-1].startswith("moving"):
            assert float(grads[k].abs().max()) == 0.0
    if rate > 0 and fx["L"] > 1:                             # the masks did something
        fw0 = tro.train_forward(fx["mix"], fx["variables"], fx["L"], fx["nif"], fx["n_fft"], fx["hop"], None)
        assert float((fw0["mags"][0] - fw["mags"][0]).abs().max()) > 1e-6


def test_the_conv_bias_gradient_under_a_batch_norm_is_zero_but_its_floor_is_not():
    fx = tro.fixture("skip")
    fw = tro.train_forward(fx["mix"], fx["variables"], fx["L"], fx["nif"], fx["n_fft"], fx["hop"], None)
    _, _, grads, floors, _ = tro.loss_and_gradients(fw, fx["targets"], fx["n_fft"], fx["hop"])
    g, f = grads["separator/conv2d/bias"], floors["separator/conv2d/bias"]
    assert float(g.abs().max()) <= 1e-12 * f and f > 0
    assert float(grads["separator/conv2d_transpose_1/bias"].abs().max()) > 1e-3 * floors["separator/conv2d_transpose_1/bias"]


def test_wgrad_form_is_the_gradient_of_both_conv_oracles():
    rng = np.random.RandomState(3)
    x = torch.tensor(rng.randn(2, 4, 6, 3), dtype=torch.float64)
    w = torch.tensor(rng.randn(5, 5, 3, 4), dtype=torch.float64, requires_grad=True)
    g = torch.tensor(rng.randn(2, 2, 3, 4), dtype=torch.float64)
    (want,) = torch.autograd.grad((ora.conv2d_s2(x, w) * g).sum(), w)
    assert float((tro.wgrad(x, g) - want).abs().max()) <= 1e-12
    a = torch.tensor(rng.randn(2, 2, 3, 5), dtype=torch.float64)
    wt = torch.tensor(rng.randn(5, 5, 2, 5), dtype=torch.float64, requires_grad=True)
    gt = torch.tensor(rng.randn(2, 4, 6, 2), dtype=torch.float64)
    (want,) = torch.autograd.grad((ora.conv2d_transpose_s2(a, wt) * gt).sum(), wt)
    assert float((tro.wgrad(gt, a) - want).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------------ moving averages
def _assign_moving_average_literal(variable, value, decay):
    """tensorflow/python/training/moving_averages.py, zero_debias=False, transcribed:
         decay = 1 - decay;  update_delta = (variable - value) * decay;  return assign_sub(variable, update_delta)"""
    decay = 1.0 - decay
    update_delta = (variable - value) * decay
    return variable - update_delta


@pytest.mark.parametrize("n", [1, 2, 16, 4096])
def test_moving_average_rule(n):
    rng = np.random.RandomState(n)
    mm, mv, mu, var = rng.randn(5), rng.rand(5) + 0.5, rng.randn(5), rng.rand(5)
    assert np.array_equal(tro.moving_average(mm, mu, 0.999), _assign_moving_average_literal(mm, mu, 0.999))
    want = _assign_moving_average_literal(mv, var * n / (n - 1) if n > 1 else var, 0.999)
    assert np.abs(tro.moving_average(mv, tro.unbiased(var, n), 0.999) - want).max() <= 1e-15
    assert tro.unbiased(1.0, 1) == 1.0 and tro.unbiased(1.0, 2) == 2.0


# ------------------------------------------------------------------------------------------------ dropout keep bits
def _keep_literal(seed, step, source, level, e, rate):
    """include/wun.h's rule in Python integers."""
    m = (1 << 64) - 1

    def mix(z):
        z = (z + 0x9E3779B97F4A7C15) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        return z ^ (z >> 31)

    key = mix((mix((mix(seed & m) + step) & m) + ((source << 8) | level)) & m)
    u = mix((key + e) & m) >> 40
    return np.float32(u) * np.float32(2.0 ** -24) >= np.float32(rate)


def test_dropout_keep_function():
    base = (1337, 5, 1, 2)
    got = tro.dropout_keep(*base, 300, 0.5)
    assert [bool(x) for x in got] == [bool(_keep_literal(*base, e, 0.5)) for e in range(300)]
    assert np.array_equal(got, tro.dropout_keep(*base, 300, 0.5))                         # deterministic
    assert np.array_equal(tro.dropout_keep(-3, 5, 1, 2, 8, 0.5), [_keep_literal(-3, 5, 1, 2, e, 0.5) for e in range(8)])
    for other in ((1338, 5, 1, 2), (1337, 6, 1, 2), (1337, 5, 0, 2), (1337, 5, 1, 1)):    # every argument matters
        assert not np.array_equal(got, tro.dropout_keep(*other, 300, 0.5))
    assert not np.array_equal(got[1:], got[:-1])                                          # (and so does the element index)
    n = 1 << 16
    frac = tro.dropout_keep(*base, n, 0.5).mean()
    assert abs(frac - 0.5) <= 4 * 0.5 / np.sqrt(n)
    frac = tro.dropout_keep(*base, n, 0.25).mean()
    assert abs(frac - 0.75) <= 4 * np.sqrt(0.25 * 0.75 / n)
    assert tro.dropout_keep(*base, 1000, 0.0).all()
    m = tro.dropout_multipliers(*base, (4, 5), 0.5)
    assert set(np.unique(m)) <= {0.0, 2.0} and m.shape == (4, 5)


# ------------------------------------------------------------------------------------------------ the kink condition
@pytest.mark.parametrize("rate", [0.0, 0.5])
@pytest.mark.parametrize("name", sorted(tro.GEOMETRIES))
def test_fixtures_stay_away_from_the_kinks(name, rate):
    """Gradient parity in float32 means something only away from the kinks of abs, ReLU and LeakyReLU: every loss difference
    R - M mask (k < K - 1) and every zhat of the float64 oracle is farther from 0 than 64 times the float32 oracle's deviation
    at that element.  tro.SEEDS was chosen so that this holds."""
    fx = tro.fixture(name)
    masks = tro.fixture_masks(fx, rate)
    args = (fx["mix"], fx["variables"], fx["L"], fx["nif"], fx["n_fft"], fx["hop"], masks)
    f64, f32 = tro.train_forward(*args), tro.train_forward(*args, dtype=torch.float32)
    d64 = tro.loss_and_gradients(f64, fx["targets"], fx["n_fft"], fx["hop"])[4]
    d32 = tro.loss_and_gradients(f32, fx["targets"], fx["n_fft"], fx["hop"])[4]
    worst = np.inf
    for s in range(2):
        pairs = [(d64[s], d32[s])] + [(a, b) for a, b in zip(f64["src"][s]["zhat"], f32["src"][s]["zhat"])]
        for a, b in pairs:
            dev = (a - b.double()).abs()
            margin = a.abs() / (64.0 * dev).clamp_min(1e-300)
            worst = min(worst, float(margin.min()))
    print("%s rate %.1f: smallest |value| / (64 deviation) = %.3g" % (name, rate, worst))
    assert worst > 1.0


# ------------------------------------------------------------------------------------------------ the C ABI, host side
def _spec(L=2, nif=3, S=2, n_fft=64, hop=48):
    return _lib.WunSpecConfig(L, nif, S, n_fft, hop)


def _tc(decay=0.999, rate=0.5, seed=1):
    return _lib.WunSpecTrainConfig(decay, rate, seed)


def test_workspace_and_accessor(lib):
    c, T = _spec(), 7 * 48 + 64
    n = lib.wun_spec_train_workspace_floats(C.byref(c), 2, T)
    assert n > lib.wun_spec_workspace_floats(C.byref(c), 2, T) > 0
    assert lib.wun_spec_train_workspace_floats(C.byref(c), 0, T) == -1
    assert lib.wun_spec_train_workspace_floats(C.byref(c), 2, T - 48) == -1
    assert lib.wun_spec_train_workspace_floats(None, 2, T) == -1
    off, cnt = C.c_int64(), C.c_int64()
    get = lambda kind, s, layer: (lib.wun_spec_train_tensor(C.byref(c), 2, T, kind, s, layer, C.byref(off), C.byref(cnt)), off.value, cnt.value)
    spans = []
    for s in range(2):
        for layer, (H, W, ch) in enumerate([(4, 16, 3), (2, 8, 6), (4, 16, 3)]):
            for kind, want in ((0, 2 * H * W * ch), (1, ch), (2, ch), (3, 2 * H * W * ch)):
                rc, o, k = get(kind, s, layer)
                assert rc == 0 and k == want and 0 <= o and o + k <= n
                spans.append((o, o + k))
        rc, o, k = get(3, s, 3)                              # the mask
        assert rc == 0 and k == 2 * 8 * 32
        spans.append((o, o + k))
        rc, o, k = get(4, s, 0)                              # the one dropout level: [2, 4, 16, 6]
        assert rc == 0 and k == 2 * 4 * 16 * 6
        spans.append((o, o + k))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))                   # no two retained tensors share a float
    assert get(0, 2, 0)[0] == -1 and get(0, 0, 3)[0] == -1 and get(9, 0, 0)[0] == -1 and get(4, 0, 1)[0] == -1
    assert lib.wun_spec_train_tensor(C.byref(c), 2, T, 0, 0, 0, None, C.byref(cnt)) == -1
    five = _spec(L=5, nif=2)
    T5 = 31 * 48 + 64
    assert lib.wun_spec_train_tensor(C.byref(five), 2, T5, 4, 0, 2, C.byref(off), C.byref(cnt)) == 0 and cnt.value > 0
    assert lib.wun_spec_train_tensor(C.byref(five), 2, T5, 4, 0, 3, C.byref(off), C.byref(cnt)) == 0 and cnt.value == 0


def test_entries_refuse_before_any_gpu_work(lib):
    """Every refusal below returns before the first launch, so the fake (never dereferenced) pointers are safe without a GPU."""
    c, T = _spec(), 7 * 48 + 64
    ws_n = lib.wun_spec_train_workspace_floats(C.byref(c), 1, T)
    p, far = C.c_void_p(256), C.c_void_p(256 + 4 * (ws_n + 64))
    q = [C.c_void_p(far.value + (i + 1) * (1 << 24)) for i in range(6)]
    fwd, bwd, adam = lib.wun_spec_train_forward, lib.wun_spec_loss_backward, lib.wun_spec_adam_step
    t = _tc()
    assert fwd(C.byref(c), None, q[0], q[1], 1, T, q[2], 0, q[3], p, None) == -1                    # null training config
    assert fwd(C.byref(c), C.byref(t), None, q[1], 1, T, q[2], 0, q[3], p, None) == -1
    assert fwd(C.byref(c), C.byref(t), q[0], q[1], 1, T, q[2], 0, None, p, None) == -1              # mags are required
    assert fwd(C.byref(c), C.byref(t), q[0], q[1], 1, T, q[2], 0, q[3], None, None) == -1
    assert fwd(C.byref(c), C.byref(t), q[0], q[1], 1, T + 1, q[2], 0, q[3], p, None) == -1
    assert fwd(C.byref(c), C.byref(t), q[0], q[1], 1, T, q[2], -1, q[3], p, None) == -1             # step below 0
    assert fwd(C.byref(c), C.byref(t), q[0], q[1], 1, T, q[2], 0, p, p, None) == -1                 # mags inside the workspace
    assert b"overlaps" in lib.wun_last_error()
    assert fwd(C.byref(c), C.byref(t), p, q[1], 1, T, q[2], 0, q[3], p, None) == -1                 # params inside it
    for bad in (_tc(rate=1.0), _tc(rate=-0.1), _tc(rate=float("nan")), _tc(decay=1.5), _tc(decay=-0.1), _tc(decay=float("nan"))):
        assert fwd(C.byref(c), C.byref(bad), q[0], q[1], 1, T, q[2], 0, q[3], p, None) == -1
        assert bwd(C.byref(c), C.byref(bad), q[0], q[1], 1, T, q[2], q[3], q[4], p, None) == -1
        assert adam(C.byref(c), C.byref(bad), q[0], q[1], q[2], q[3], p, 1, T, 1, 1e-3, 0.9, 0.999, 1e-8, 1.0, None) == -1
    assert b"bn_decay" in lib.wun_last_error()
    assert bwd(C.byref(c), C.byref(t), q[0], None, 1, T, q[2], q[3], q[4], p, None) == -1
    assert bwd(C.byref(c), C.byref(t), q[0], q[1], 1, T, q[2], None, q[4], p, None) == -1
    assert bwd(C.byref(c), C.byref(t), q[0], q[1], 1, T, q[2], q[3], None, p, None) == -1
    assert bwd(C.byref(c), C.byref(t), q[0], q[1], 1, T, q[2], p, q[4], p, None) == -1              # grads inside the workspace
    assert bwd(C.byref(c), C.byref(t), q[0], q[1], 1, T, q[2], q[0], q[4], p, None) == -1           # grads on params
    assert bwd(C.byref(c), C.byref(t), q[0], q[1], 0, T, q[2], q[3], q[4], p, None) == -1
    assert adam(C.byref(c), C.byref(t), None, q[1], q[2], q[3], p, 1, T, 1, 1e-3, 0.9, 0.999, 1e-8, 1.0, None) == -1
    assert adam(C.byref(c), C.byref(t), q[0], q[1], q[2], q[3], p, 1, T, 0, 1e-3, 0.9, 0.999, 1e-8, 1.0, None) == -1   # 1-based
    assert adam(C.byref(c), C.byref(t), q[0], q[1], q[2], q[2], p, 1, T, 1, 1e-3, 0.9, 0.999, 1e-8, 1.0, None) == -1   # m is v
    assert adam(C.byref(c), C.byref(t), q[0], q[1], q[2], q[3], q[0], 1, T, 1, 1e-3, 0.9, 0.999, 1e-8, 1.0, None) == -1
    # the single operators
    sw, tw, st = lib.wun_op_conv2d_s2_wgrad, lib.wun_op_conv2d_transpose_s2_wgrad, lib.wun_op_bn2d_stats
    assert lib.wun_op_conv2d_s2_wgrad_scratch(1, 4, 4, 2, 3) == 25 * 2 * 3 + 4 * 3 + 2
    assert lib.wun_op_conv2d_s2_wgrad_scratch(1, 3, 4, 2, 3) == -1 and lib.wun_op_conv2d_s2_wgrad_scratch(1, 4, 4, 0, 3) == -1
    assert lib.wun_op_conv2d_s2_wgrad_scratch(2, 64, 64, 2, 3) == 8 * 25 * 2 * 3 + 4 * 2 * 3 + 2      # 2048 pixels: 8 chunks, 2 sum blocks
    assert lib.wun_op_conv2d_transpose_s2_wgrad_scratch(1, 2, 2, 5, 3) == 25 * 3 * 5 + 4 * 3 + 2
    assert lib.wun_op_conv2d_transpose_s2_wgrad_scratch(0, 2, 2, 5, 3) == -1
    assert sw(None, q[1], q[2], None, p, 1, 4, 4, 2, 3, None) == -1
    assert sw(q[0], q[1], q[2], None, None, 1, 4, 4, 2, 3, None) == -1
    assert sw(q[0], q[1], q[2], None, p, 1, 4, 5, 2, 3, None) == -1                                  # odd W
    assert sw(q[0], q[1], p, None, p, 1, 4, 4, 2, 3, None) == -1                                     # dw inside the scratch
    assert tw(q[0], 2, None, 3, q[1], q[2], None, p, 1, 2, 2, 3, None) == -1                         # c1 without x1
    assert tw(q[0], 0, None, 0, q[1], q[2], None, p, 1, 2, 2, 3, None) == -1
    assert tw(q[0], 2, None, 0, q[1], q[2], p, p, 1, 2, 2, 3, None) == -1                            # db inside the scratch
    assert lib.wun_op_bn2d_stats_scratch(1, 1, 1, 1) == 6 and lib.wun_op_bn2d_stats_scratch(1, 0, 1, 1) == -1
    assert st(None, q[1], q[2], p, 1, 1, 1, 1, None) == -1
    assert st(q[0], q[1], q[1], p, 1, 1, 1, 1, None) == -1                                           # mean is var
    assert st(q[0], p, q[2], p, 1, 1, 1, 1, None) == -1


# ------------------------------------------------------------------------------------------------ the Python side
def _cfg(**kw):
    base = dict(num_layers=2, num_initial_filters=3, spec_frame_len=64, spec_hop=48, num_frames=7 * 48 + 64, batch_size=2)
    base.update(kw)
    return wun.get_config("unet_spectrogram_l1", **base)


def test_the_two_pinned_refusals_still_say_inference_only():
    sep = UnetSpectrogramSeparator(_cfg())
    with pytest.raises(NotImplementedError, match="inference only"):
        sep.get_output(np.zeros((1, 7 * 48 + 64, 1), np.float32), True)
    with pytest.raises(NotImplementedError, match="inference only"):
        training.train(dict(_cfg(), raw_audio_loss=True), 1)
    assert sep.params is None


@pytest.mark.parametrize("key, value", [("spectral_loss", {"resolutions": [[64, 16]], "weights": [1.0], "mse_weight": 0.0}),
                                        ("waveform_loss", {"terms": {"l1": 1.0}}), ("grad_accum_steps", 2), ("clip_grad_norm", 1.0),
                                        ("skip_nonfinite_steps", True)])
def test_trainer_refuses_what_is_not_built_for_this_network(key, value):
    with pytest.raises(NotImplementedError, match=key):
        training.train(dict(_cfg(), **{key: value}), 1)


def test_trainer_refuses_data_parallel_training(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="world > 1"):
        training.train(_cfg(), 1)


def test_training_settings_are_extension_keys():
    sep = UnetSpectrogramSeparator(_cfg(), seed=5)
    assert (sep._tcfg.dropout_rate, sep._tcfg.dropout_seed) == (0.5, 5) and abs(sep._tcfg.bn_decay - 0.999) < 1e-7
    sep = UnetSpectrogramSeparator(_cfg(spec_dropout=0.0, spec_bn_decay=0.9, spec_dropout_seed=11))
    assert (sep._tcfg.dropout_rate, sep._tcfg.dropout_seed) == (0.0, 11) and abs(sep._tcfg.bn_decay - 0.9) < 1e-7
    assert wun.config.EXTENSION_DEFAULTS["spec_dropout"] == 0.5 and wun.config.EXTENSION_DEFAULTS["spec_bn_decay"] == 0.999
    with pytest.raises(RuntimeError, match="training forward|get_output"):
        sep.loss_and_gradients(np.zeros((2, 1, 400, 1), np.float32))
