"""CPU-only checks of the spectrogram U-Net: the float64 oracle tests/_specunet_np.py against independent
statements of the same definitions, and the host side of the feature -- the variable table, the named configurations, the
shapes and every refusal.  No GPU work: each refusal must come before any."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _specunet_np as ora  # noqa: E402

import wave_u_net_amd as wun  # noqa: E402
from wave_u_net_amd import _lib, config, training, validation  # noqa: E402
from wave_u_net_amd.spectrogram import UnetSpectrogramSeparator, make_separator  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _cfg(**kw):
    base = dict(num_layers=2, num_initial_filters=3, spec_frame_len=64, spec_hop=48, num_frames=7 * 48 + 64, batch_size=2)
    base.update(kw)
    return wun.get_config("unet_spectrogram", **base)


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("N, M", [(3, 5), (4, 2), (1, 1), (2, 7)])
def test_transposed_oracle_is_the_gradient_of_the_conv_oracle(N, M):
    """d/dx <conv2d_s2(x, w), g> = conv2d_transpose_s2(g, w^T): a conv kernel [5, 5, Ci, Co] read as a transposed-conv kernel
    [5, 5, out = Ci, in = Co].  Input maps of the transposed conv with odd and even sizes."""
    rng = np.random.RandomState(N * 10 + M)
    ci, co = 3, 4
    x = torch.tensor(rng.randn(2, 2 * N, 2 * M, ci), dtype=torch.float64, requires_grad=True)
    w = torch.tensor(rng.randn(5, 5, ci, co), dtype=torch.float64)
    g = torch.tensor(rng.randn(2, N, M, co), dtype=torch.float64)
    (grad,) = torch.autograd.grad((ora.conv2d_s2(x, w) * g).sum(), x)
    got = ora.conv2d_transpose_s2(g, w)
    assert got.shape == grad.shape
    assert float((got - grad).abs().max()) <= 1e-12 * max(1.0, float(grad.abs().max()))


def test_conv_oracle_is_tf_same_padding():
    """out[y][x] = sum A[2y + ky - 1][2x + kx - 1] W[ky][kx], written as loops."""
    rng = np.random.RandomState(0)
    x, w = rng.randn(1, 4, 6, 2), rng.randn(5, 5, 2, 3)
    want = np.zeros((1, 2, 3, 3))
    for y in range(2):
        for xx in range(3):
            for ky in range(5):
                for kx in range(5):
                    iy, ix = 2 * y + ky - 1, 2 * xx + kx - 1
                    if 0 <= iy < 4 and 0 <= ix < 6:
                        want[0, y, xx] += x[0, iy, ix] @ w[ky, kx]
    got = ora.conv2d_s2(torch.tensor(x), torch.tensor(w)).numpy()
    assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize("B, N, M, ci, co", [(2, 3, 5, 3, 4), (1, 1, 1, 1, 1), (1, 4, 1, 2, 5), (2, 1, 6, 5, 2)])
def test_both_conv_oracles_are_the_library_convolutions(B, N, M, ci, co):
    """An implementation nobody here wrote: torch.nn.functional.conv2d on the (1, 2, 1, 2)-padded input, and
    conv_transpose2d(stride=2, padding=1) cut to [2N, 2M] (its output has 2N + 1 rows: out[t] = sum over 2 j + k - 1 == t)."""
    Fn = torch.nn.functional
    rng = np.random.RandomState(B + 10 * N + 100 * M)
    x = torch.tensor(rng.randn(B, 2 * N, 2 * M, ci), dtype=torch.float64)
    w = torch.tensor(rng.randn(5, 5, ci, co), dtype=torch.float64)
    want = Fn.conv2d(Fn.pad(x.permute(0, 3, 1, 2), (1, 2, 1, 2)), w.permute(3, 2, 0, 1), stride=2).permute(0, 2, 3, 1)
    got = ora.conv2d_s2(x, w)
    assert got.shape == want.shape == (B, N, M, co)
    assert float((got - want).abs().max()) <= 1e-12
    a = torch.tensor(rng.randn(B, N, M, ci), dtype=torch.float64)
    wt = torch.tensor(rng.randn(5, 5, co, ci), dtype=torch.float64)
    want = Fn.conv_transpose2d(a.permute(0, 3, 1, 2), wt.permute(3, 2, 0, 1), stride=2, padding=1)[..., :2 * N, :2 * M].permute(0, 2, 3, 1)
    got = ora.conv2d_transpose_s2(a, wt)
    assert got.shape == want.shape == (B, 2 * N, 2 * M, co)
    assert float((got - want).abs().max()) <= 1e-12


def _inverse_stft_window_literal(frame_length, frame_step):
    """tf.contrib.signal.inverse_stft_window_fn, transcribed: pad the squared window to overlaps * frame_step, reshape to
    [overlaps, frame_step], sum over the overlaps, tile back, divide the forward window by it."""
    n = np.arange(frame_length, dtype=np.float64)
    forward_window = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / frame_length)           # hann_window(periodic=True)
    denom = np.square(forward_window)
    overlaps = -(-frame_length // frame_step)
    denom = np.pad(denom, [(0, overlaps * frame_step - frame_length)], mode="constant")
    denom = np.reshape(denom, [overlaps, frame_step])
    denom = np.sum(denom, 0, keepdims=True)
    denom = np.tile(denom, [overlaps, 1])
    denom = np.reshape(denom, [overlaps * frame_step])
    return forward_window / denom[:frame_length]


@pytest.mark.parametrize("n_fft, hop", [(1024, 768), (64, 48), (64, 16)])
def test_istft_tf_normaliser_is_inverse_stft_window_fn(n_fft, hop):
    D = ora.steady_denominator(n_fft, hop).numpy()
    got = ora.hann(n_fft).numpy() / D[np.arange(n_fft) % hop]
    want = _inverse_stft_window_literal(n_fft, hop)
    assert np.abs(got - want).max() <= 1e-14
    if (n_fft, hop) == (1024, 768):
        # the smallest denominator at the model's framing: p = 128, where w^2[128] + w^2[896] = 2 sin^4(pi / 8) -- far above
        # the 1e-8 below which a resolution is refused (D[0] = w^2[768] = 0.25 is not the minimum)
        assert abs(D.min() - 2.0 * np.sin(np.pi / 8) ** 4) < 1e-12 and abs(D[0] - 0.25) < 1e-12


@pytest.mark.parametrize("n_fft, hop, F", [(1024, 768, 4), (64, 48, 8), (64, 16, 9)])
def test_istft_tf_inverts_the_stft_where_the_track_is_fully_covered(n_fft, hop, F):
    T = (F - 1) * hop + n_fft
    x = torch.tensor(np.random.RandomState(F).randn(2, T), dtype=torch.float64)
    y = ora.istft_tf(ora.stft(x, n_fft, hop), n_fft, hop).numpy()
    w2 = (ora.hann(n_fft) ** 2).numpy()
    cover = np.zeros(T)
    for f in range(F):
        cover[f * hop:f * hop + n_fft] += w2
    D = ora.steady_denominator(n_fft, hop).numpy()[np.arange(T) % hop]
    full = np.abs(cover - D) <= 1e-12                        # both normalisers agree: the steady state is reached
    assert full.sum() >= T - 2 * n_fft and full.sum() > 0
    assert np.abs(y[:, full] - x.numpy()[:, full]).max() <= 1e-12
    assert not full[0]                                       # (the edges are NOT inverted: w^2 / D < 1 there)


# ------------------------------------------------------------------------------------------------ the variable table
L2_TABLE = [
    ("separator/conv2d/kernel", (5, 5, 1, 3)), ("separator/conv2d/bias", (3,)),
    ("separator/BatchNorm/beta", (3,)), ("separator/BatchNorm/moving_mean", (3,)), ("separator/BatchNorm/moving_variance", (3,)),
    ("separator/conv2d_1/kernel", (5, 5, 3, 6)), ("separator/conv2d_1/bias", (6,)),
    ("separator/BatchNorm_1/beta", (6,)), ("separator/BatchNorm_1/moving_mean", (6,)), ("separator/BatchNorm_1/moving_variance", (6,)),
    ("separator/conv2d_transpose/kernel", (5, 5, 3, 6)), ("separator/conv2d_transpose/bias", (3,)),
    ("separator/BatchNorm_2/beta", (3,)), ("separator/BatchNorm_2/moving_mean", (3,)), ("separator/BatchNorm_2/moving_variance", (3,)),
    ("separator/conv2d_transpose_1/kernel", (5, 5, 1, 6)), ("separator/conv2d_transpose_1/bias", (1,)),
    ("separator/conv2d_2/kernel", (5, 5, 1, 3)), ("separator/conv2d_2/bias", (3,)),
    ("separator/BatchNorm_3/beta", (3,)), ("separator/BatchNorm_3/moving_mean", (3,)), ("separator/BatchNorm_3/moving_variance", (3,)),
    ("separator/conv2d_3/kernel", (5, 5, 3, 6)), ("separator/conv2d_3/bias", (6,)),
    ("separator/BatchNorm_4/beta", (6,)), ("separator/BatchNorm_4/moving_mean", (6,)), ("separator/BatchNorm_4/moving_variance", (6,)),
    ("separator/conv2d_transpose_2/kernel", (5, 5, 3, 6)), ("separator/conv2d_transpose_2/bias", (3,)),
    ("separator/BatchNorm_5/beta", (3,)), ("separator/BatchNorm_5/moving_mean", (3,)), ("separator/BatchNorm_5/moving_variance", (3,)),
    ("separator/conv2d_transpose_3/kernel", (5, 5, 1, 6)), ("separator/conv2d_transpose_3/bias", (1,)),
]


def test_variable_table_l2_written_out():
    sep = UnetSpectrogramSeparator(_cfg())
    assert [(n, s) for n, _, s in sep.variable_table()] == L2_TABLE == ora.variable_shapes(2, 3)
    off = 0
    for _, o, s in sep.variable_table():                     # packed, in table order
        assert o == off
        off += int(np.prod(s))
    assert off == sep.num_params


@pytest.mark.parametrize("L, nif", [(6, 16), (2, 3), (1, 5)])
def test_variable_table_follows_the_naming_rule(L, nif):
    sep = UnetSpectrogramSeparator(_cfg(num_layers=L, num_initial_filters=nif, spec_frame_len=1024, spec_hop=768))
    table = [(n, s) for n, _, s in sep.variable_table()]
    assert table == ora.variable_shapes(L, nif)
    assert len(table) == 2 * (5 * L + 5 * (L - 1) + 2)
    names = [n for n, _ in table]
    assert len(set(names)) == len(names) and all(len(n) < 64 for n in names)
    if L == 6:                                               # the last conv of source 1, the mask layer, the last batch norm
        assert "separator/conv2d_11/kernel" in names and "separator/conv2d_transpose_11/bias" in names
        assert "separator/BatchNorm_21/moving_variance" in names and "separator/BatchNorm_22/beta" not in names
        assert dict(table)["separator/conv2d_transpose_6/kernel"] == (5, 5, 256, 512)
        assert dict(table)["separator/conv2d_transpose_7/kernel"] == (5, 5, 128, 512)
        assert dict(table)["separator/conv2d_transpose_5/kernel"] == (5, 5, 1, 32)


def test_initial_values_are_tfs():
    sep = UnetSpectrogramSeparator(_cfg())
    host = sep.initial_values()
    for name, off, shp in sep.variable_table():
        v = host[off:off + int(np.prod(shp))]
        if name.endswith("/kernel"):
            lim = np.sqrt(6.0 / (25 * (shp[2] + shp[3])))
            assert np.abs(v).max() <= lim and np.abs(v).max() > 0.5 * lim
        elif name.endswith("/moving_variance"):
            assert (v == 1.0).all()
        else:
            assert (v == 0.0).all()


# ------------------------------------------------------------------------------------------------ configs, shapes, refusals
def test_named_configs_are_the_references():
    base = dict(config.BASE_MODEL_CONFIG)
    u7 = dict(base, batch_size=4, network="unet_spectrogram", num_layers=6, expected_sr=8192, num_frames=768 * 127 + 1024,
              duration=13, num_initial_filters=16)                               # Config.py:136-147
    for name, want in (("unet_spectrogram", u7), ("unet_spectrogram_l1", dict(u7, raw_audio_loss=False))):   # :149-161
        got = wun.get_config(name)
        for k, v in want.items():
            assert got[k] == v, (name, k)
        assert got["source_names"] == ["accompaniment", "vocals"] and got["num_channels"] == 1
        assert set(got) == set(want) | {"source_names", "num_sources", "num_channels"}
    assert config.EXTENSION_DEFAULTS["spec_frame_len"] == 1024 and config.EXTENSION_DEFAULTS["spec_hop"] == 768
    assert "spec_hop" not in config.BASE_MODEL_CONFIG
    sep = make_separator(wun.get_config("unet_spectrogram"))
    assert isinstance(sep, UnetSpectrogramSeparator) and (sep.frame_len, sep.hop) == (1024, 768)
    assert sep.frames(98560) == 128
    assert isinstance(make_separator(wun.get_config("baseline")), wun.UnetAudioSeparator)
    with pytest.raises(NotImplementedError):
        make_separator(dict(wun.get_config("baseline"), network="gan"))


def test_get_padding_returns_the_shape_twice():
    sep = UnetSpectrogramSeparator(_cfg())
    i, o = sep.get_padding(np.array([4, 400, 0]))
    assert list(i) == [4, 400, 1] == list(o)                  # UnetSpectrogramSeparator.py:38


def test_constructor_refusals_say_what_is_out_of_scope():
    with pytest.raises(NotImplementedError, match="mono"):
        UnetSpectrogramSeparator(_cfg(mono_downmix=False))
    with pytest.raises(NotImplementedError, match="two sources"):
        UnetSpectrogramSeparator(_cfg(task="multi_instrument"))
    with pytest.raises(NotImplementedError, match="bf16"):
        UnetSpectrogramSeparator(_cfg(compute_dtype="bf16"))
    with pytest.raises(NotImplementedError):                 # n_fft outside the FFT's list
        UnetSpectrogramSeparator(_cfg(spec_frame_len=16384, spec_hop=4096))
    with pytest.raises(NotImplementedError):
        UnetSpectrogramSeparator(_cfg(spec_frame_len=96, spec_hop=48))
    with pytest.raises(ValueError):
        UnetSpectrogramSeparator(_cfg(spec_hop=0))


def test_get_output_refuses_before_any_gpu_work():
    sep = UnetSpectrogramSeparator(_cfg())
    ok = np.zeros((1, 7 * 48 + 64, 1), np.float32)
    with pytest.raises(NotImplementedError, match="inference only"):
        sep.get_output(ok, True)
    for T in (3 * 48 + 64 + 1,                               # not (F - 1) hop + n_fft
              6 * 48 + 64,                                   # F = 7: no multiple of 4
              10):                                           # shorter than a frame
        with pytest.raises(ValueError):
            sep.get_output(np.zeros((1, T, 1), np.float32), False)
    with pytest.raises(ValueError, match="mono"):
        sep.get_output(np.zeros((1, 400, 2), np.float32), False)
    # n_fft / 2 = 32 halves 5 times, not 6
    deep = UnetSpectrogramSeparator(_cfg(num_layers=6))
    with pytest.raises(ValueError):
        deep.frames(63 * 48 + 64)
    assert sep.params is None                                # nothing was allocated on the way


def test_training_refuses_the_network_with_a_plain_message():
    with pytest.raises(NotImplementedError, match="inference only"):
        training.train(_cfg(), 1)
    with pytest.raises(NotImplementedError):
        validation.test(dict(_cfg(), network="gan"), "valid", "x", None, tracks=[])
    with pytest.raises(ValueError, match="magnitudes"):
        validation.test(dict(_cfg(), raw_audio_loss=False, validation_metric="si_sdr"), "valid", "x", None, tracks=[])


# ------------------------------------------------------------------------------------------------ the C ABI, host side
def _spec(L=2, nif=3, S=2, n_fft=64, hop=48):
    return _lib.WunSpecConfig(L, nif, S, n_fft, hop)


def test_shape_conditions_and_counts(lib):
    c = _spec()
    assert lib.wun_spec_frames(C.byref(c), 7 * 48 + 64) == 8
    assert lib.wun_spec_frames(C.byref(c), 7 * 48 + 65) == -1
    assert lib.wun_spec_frames(C.byref(c), 6 * 48 + 64) == -1
    assert lib.wun_spec_frames(C.byref(_spec(L=6)), 63 * 48 + 64) == -1          # 32 bins do not halve six times
    assert lib.wun_spec_frames(C.byref(_spec(n_fft=100)), 400) == -2
    assert lib.wun_spec_frames(None, 400) == -1
    assert lib.wun_spec_num_tensors(C.byref(c)) == 34
    assert lib.wun_spec_param_floats(C.byref(c)) == sum(int(np.prod(s)) for _, s in L2_TABLE)
    assert lib.wun_spec_workspace_floats(C.byref(c), 2, 7 * 48 + 64) > 0
    assert lib.wun_spec_workspace_floats(C.byref(c), 0, 7 * 48 + 64) == -1
    assert lib.wun_spec_workspace_floats(C.byref(c), 2, 6 * 48 + 64) == -1
    info = _lib.WunTensorInfo()
    assert lib.wun_spec_tensor(C.byref(c), 34, C.byref(info)) == -1 and lib.wun_spec_tensor(C.byref(c), 0, None) == -1
    u7 = _spec(L=6, nif=16, n_fft=1024, hop=768)
    assert lib.wun_spec_frames(C.byref(u7), 98560) == 128


@pytest.mark.parametrize("L, nif", [(2, 3), (1, 5)])
@pytest.mark.parametrize("S", [1, 3])
def test_table_through_the_c_abi_for_other_source_counts(lib, S, L, nif):
    """wun_spec_tensor allows 1..8 sources; the separator class only ever asks for two.  The index arithmetic s L + i and
    s (2L - 1) + j of the names, the packing and the two counts, against the oracle's table."""
    c = _spec(L=L, nif=nif, S=S)
    n = lib.wun_spec_num_tensors(C.byref(c))
    want = ora.variable_shapes(L, nif, S)
    assert n == len(want) == S * (5 * L + 5 * (L - 1) + 2)
    info, off, names = _lib.WunTensorInfo(), 0, []
    for i in range(n):
        assert lib.wun_spec_tensor(C.byref(c), i, C.byref(info)) == 0
        shape = tuple(int(info.shape[d]) for d in range(info.ndim))
        assert (info.name.decode(), shape) == want[i]
        assert info.offset == off                            # packed, in table order
        off += int(np.prod(shape))
        names.append(info.name.decode())
    assert lib.wun_spec_param_floats(C.byref(c)) == off
    assert len(set(names)) == n
    assert lib.wun_spec_tensor(C.byref(c), n, C.byref(info)) == -1
    last = S * L - 1
    assert names[-1] == "separator/conv2d_transpose%s/bias" % ("_%d" % last if last else "")
    assert lib.wun_spec_num_tensors(C.byref(_spec(S=9))) == -2 and lib.wun_spec_num_tensors(C.byref(_spec(S=0))) == -1


def test_istft_tf_refuses_a_resolution_with_a_vanishing_denominator(lib):
    """hop == n_fft: D[0] = w[0]^2 = 0."""
    assert lib.wun_istft_tf_scratch_floats(1, 1, 256, 1, 64, 64, 4) == -2
    assert b"1e-8" in lib.wun_last_error()
    assert lib.wun_istft_tf_fft_scratch_floats(1, 1, 256, 1, 64, 64, 4) == -2
    assert lib.wun_istft_tf_fft_scratch_floats(1, 1, 3 * 3072 + 4096, 1, 4096, 3072, 4) > 0 > lib.wun_istft_tf_scratch_floats(
        1, 1, 3 * 3072 + 4096, 1, 4096, 3072, 4)
    assert lib.wun_istft_tf_scratch_floats(1, 1, 7 * 48 + 64, 1, 64, 48, 8) > 0
    assert lib.wun_istft_tf_scratch_floats(1, 1, 98560, 1, 1024, 768, 128) == lib.wun_istft_scratch_floats(1, 1, 98560, 1, 1024, 768, 0, 128)


def test_forward_and_operators_refuse_before_any_gpu_work(lib):
    """Every refusal below returns before the first launch, so the fake (never dereferenced) pointers are safe without a GPU."""
    p = C.c_void_p(256)
    c = _spec()
    T = 7 * 48 + 64
    assert lib.wun_spec_forward(C.byref(c), None, p, 1, T, p, p, None, p, None) == -1
    assert lib.wun_spec_forward(C.byref(c), p, p, 1, T, p, None, None, p, None) == -1           # no output asked for
    assert lib.wun_spec_forward(C.byref(c), p, p, 1, T + 1, p, p, None, p, None) == -1
    assert lib.wun_spec_forward(C.byref(c), p, p, 1, T, p, p, None, p, None) == -1              # everything overlaps
    assert b"overlaps" in lib.wun_last_error()
    conv, tr = lib.wun_op_conv2d_s2, lib.wun_op_conv2d_transpose_s2
    assert conv(None, p, None, None, None, None, p, 1, 2, 2, 1, 1, 0, None) == -1
    assert conv(p, p, None, None, None, None, p, 1, 3, 2, 1, 1, 0, None) == -1                   # odd H
    assert conv(p, p, None, None, None, None, p, 1, 2, 5, 1, 1, 0, None) == -1                   # odd W
    assert conv(p, p, None, None, None, None, p, 1, 2, 2, 1, 1, 4, None) == -1                   # unknown act
    assert conv(p, p, None, p, None, None, p, 1, 2, 2, 1, 1, 0, None) == -1                      # a partial batch norm
    assert conv(p, p, None, None, None, None, p, 0, 2, 2, 1, 1, 0, None) == -1
    assert tr(p, 1, None, 0, p, None, None, None, None, None, 1, 1, 1, 1, 0, None) == -1         # null y
    assert tr(p, 1, None, 2, p, None, None, None, None, p, 1, 1, 1, 1, 0, None) == -1            # c1 without x1
    assert tr(p, 1, p, 0, p, None, None, None, None, p, 1, 1, 1, 1, 0, None) == -1               # x1 without c1
    assert tr(p, 0, None, 0, p, None, None, None, None, p, 1, 1, 1, 1, 0, None) == -1
