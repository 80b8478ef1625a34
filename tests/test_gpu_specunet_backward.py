"""GPU tests of the spectrogram U-Net's backward pass from any upstream gradient (include/wun.h: wun_spec_backward,
wun_spec_train_audio, wun_spec_update_moving_averages, wun_op_spec_head_backward; UnetSpectrogramSeparator.audio_output / backward /
update_moving_averages / module, spectrogram.SpecUNet) against the float64 oracle tests/_specunet_backward_np.py.

Bounds: test_gpu_specunet_train.py's `_rule`, 8 x the float32-CPU oracle's own error on that tensor, floored at
2^-20 of the tensor's sum |terms| at its largest output.  For the head's dz the terms are |d_mags| M and, per bin, the n_fft
products of the transform, c_k (|Re X| + |Im X|) sum_n |w[n] u[f hop + n]|, times mask (1 - mask); for the gradients the oracle's
`floors`; for the audio the largest value.  Bit-for-bit claims are checked on the uint32 patterns."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _specunet_np as ora  # noqa: E402
import _specunet_train_np as tro  # noqa: E402
import _specunet_backward_np as bo  # noqa: E402
from _observed import record  # noqa: E402
from _unaligned import _offset_copy  # noqa: E402

import wave_u_net_amd as wun  # noqa: E402
from wave_u_net_amd import _lib, spectral, waveform  # noqa: E402
from wave_u_net_amd.spectrogram import SpecUNet, UnetSpectrogramSeparator  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
_CACHE = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _guarded(n, fill, off=0):
    """(buffer, view of n floats with GUARD sentinel floats on both sides, `off` floats further in)."""
    buf = torch.full((n + 2 * GUARD + off,), 12345.0, dtype=torch.float32, device="cuda")
    view = buf[GUARD + off:GUARD + off + n]
    view.fill_(fill)
    return buf, view


def _guards_intact(buf, n, off=0):
    b = buf.cpu().numpy()
    return bool((b[:GUARD + off] == 12345.0).all() and (b[GUARD + off + n:] == 12345.0).all())


def _rule(got, want64, want32, floor_scale=None):
    """DESIGN.md 5.17's rule -> (error, bound), as tests/test_gpu_specunet_train.py defines it."""
    want64, want32 = np.asarray(want64, np.float64), np.asarray(want32, np.float64)
    stand_in = np.abs(want32 - want64).max()
    scale = np.abs(want64).max() if floor_scale is None else floor_scale
    return float(np.abs(np.asarray(got, np.float64) - want64).max()), max(8.0 * stand_in, 2.0 ** -20 * scale)


def _bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ================================================================================================ the operator
# (n_fft, hop, F), B = 2: FftGeom's three mappings and their partial last workgroup
HEAD_CASES = [
    (64, 48, 8),          # 32 frames per workgroup, one partial workgroup (16 frame rows)
    (64, 16, 33),         # 32 frames per workgroup, a second, partial workgroup (66 frame rows)
    (1024, 768, 3),       # 2 frames per workgroup, an odd row count per excerpt
    (4096, 1024, 3),      # one frame per workgroup, several butterflies per lane
]
DOMAINS = ["mags", "audio", "both"]


def _head_operands(case):
    """float32 operands of one source (numpy) -- computed once per case, never changed."""
    if case not in _CACHE:
        n_fft, hop, F = case
        B, K, T = 2, n_fft // 2 + 1, (F - 1) * hop + n_fft
        rng = np.random.RandomState(n_fft + hop + F)
        X = ora.stft(torch.tensor(0.5 * rng.randn(B, T)), n_fft, hop)
        op = {"re": X.real.numpy().astype(np.float32), "im": X.imag.numpy().astype(np.float32), "B": B, "T": T, "K": K,
              "mask": (1.0 / (1.0 + np.exp(-rng.randn(B, F, K - 1)))).astype(np.float32),
              "d_mags": (rng.randn(B, F, K) / (B * F * K)).astype(np.float32), "d_audio": (rng.randn(B, T) / (B * T)).astype(np.float32)}
        op["mag"] = np.sqrt(op["re"].astype(np.float64) ** 2 + op["im"].astype(np.float64) ** 2).astype(np.float32)
        _CACHE[case] = op
    return _CACHE[case]


def _head_want(case, domain, dtype, d_mags=None, d_audio=None):
    n_fft, hop, F = case
    op = _head_operands(case)
    t = lambda a: torch.tensor(a, dtype=dtype)
    X = torch.complex(t(op["re"]), t(op["im"]))
    dm = (op["d_mags"] if d_mags is None else d_mags) if domain != "audio" else None
    da = (op["d_audio"] if d_audio is None else d_audio) if domain != "mags" else None
    dz, scale = bo.head(X, t(op["mag"]), t(op["mask"]), dm, da, n_fft, hop)
    return dz.numpy(), scale


def run_head(lib, case, domain, d_mags=None, d_audio=None, off=(), scratch_fill=float("nan")):
    """-> dz [B, F, K - 1] numpy; dz and the scratch sit between guard floats, which are checked."""
    n_fft, hop, F = case
    op = _head_operands(case)
    B, T, K = op["B"], op["T"], op["K"]
    place = lambda name, a: _offset_copy(_dev(a)) if name in off else _dev(a)
    re, im, mag, mask = (place(k, op[k]) for k in ("re", "im", "mag", "mask"))
    dm = place("d_mags", op["d_mags"] if d_mags is None else d_mags) if domain != "audio" else None
    da = place("d_audio", op["d_audio"] if d_audio is None else d_audio) if domain != "mags" else None
    ns = lib.wun_op_spec_head_backward_scratch(B, T, n_fft, hop)
    assert ns == (hop + 3) // 4 * 4 + B * T
    so, zo = (1 if "scratch" in off else 0), (1 if "dz" in off else 0)
    sbuf, scratch = _guarded(ns, scratch_fill, so)
    zbuf, dz = _guarded(B * F * (K - 1), float("nan"), zo)
    _lib.check(lib.wun_op_spec_head_backward(re.data_ptr(), im.data_ptr(), mag.data_ptr(), mask.data_ptr(),
                                             None if dm is None else dm.data_ptr(), None if da is None else da.data_ptr(), B, T, n_fft,
                                             hop, spectral._fft_table(n_fft, re.device).data_ptr(), dz.data_ptr(), scratch.data_ptr(),
                                             _stream()))
    torch.cuda.synchronize()
    assert _guards_intact(sbuf, ns, so) and _guards_intact(zbuf, B * F * (K - 1), zo)
    return dz.cpu().numpy().reshape(B, F, K - 1)


@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_head_against_float64(lib, case, domain):
    got = run_head(lib, case, domain)
    want64, scale = _head_want(case, domain, torch.float64)
    want32, _ = _head_want(case, domain, torch.float32)
    err, bound = _rule(got, want64, want32, floor_scale=scale)
    record("test_head_against_float64[%s-%s]" % ("x".join(map(str, case)), domain), "err / bound", err / bound, 1.0)
    assert np.isfinite(got).all() and float(np.abs(want64).max()) > 0 and err <= bound, (err, bound)


@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_head_footprint_by_one_nan(lib, case):
    n_fft, hop, F = case
    op = _head_operands(case)
    K, T = op["K"], op["T"]
    clean = run_head(lib, case, "both")
    # one sample of d_audio: exactly the frames that cover it, every bin of them
    for t in (0, T - 1, (F // 2) * hop + n_fft // 3):
        da = op["d_audio"].copy()
        da[1, t] = np.nan
        got = run_head(lib, case, "both", d_audio=da)
        hit = np.zeros(clean.shape, bool)
        for f in range(F):
            if f * hop <= t < f * hop + n_fft:
                hit[1, f, :] = True
        assert hit.any() and np.array_equal(np.isnan(got), hit), t
        assert np.array_equal(got[~hit].view(np.uint32), clean[~hit].view(np.uint32)), t
    # one bin of d_mags: exactly that bin; the dropped bin K - 1 reaches nothing
    for k, reaches in ((0, True), (K - 2, True), (K - 1, False)):
        dm = op["d_mags"].copy()
        dm[0, F - 1, k] = np.nan
        got = run_head(lib, case, "both", d_mags=dm)
        hit = np.zeros(clean.shape, bool)
        if reaches:
            hit[0, F - 1, k] = True
        assert np.array_equal(np.isnan(got), hit), k
        assert np.array_equal(got[~hit].view(np.uint32), clean[~hit].view(np.uint32)), k
    got = run_head(lib, case, "mags", d_mags=dm)             # (the mags-only kernel: the dropped bin again)
    assert not np.isnan(got).any()


@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_head_bits_depend_on_nothing_but_the_operands(lib, case, domain):
    ref = run_head(lib, case, domain)
    assert _same_bits(ref, run_head(lib, case, domain))                                   # repetition
    assert _same_bits(ref, run_head(lib, case, domain, scratch_fill=0.0))                 # what the scratch held
    every = ("re", "im", "mag", "mask", "d_mags", "d_audio", "scratch", "dz")
    assert _same_bits(ref, run_head(lib, case, domain, off=every))                        # every operand one float off 16 bytes
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = run_head(lib, case, domain)
    assert _same_bits(ref, got)


# ================================================================================================ the model
def _cfg(geo, **kw):
    n_fft, hop, L, nif, F, B = tro.GEOMETRIES[geo]
    base = dict(num_layers=L, num_initial_filters=nif, spec_frame_len=n_fft, spec_hop=hop, num_frames=(F - 1) * hop + n_fft,
                batch_size=B, spec_dropout_seed=tro.DROPOUT_SEED)
    base.update(kw)
    return wun.get_config("unet_spectrogram_l1", **base)


def _separator(geo, fx=None, **kw):
    sep = UnetSpectrogramSeparator(_cfg(geo, **kw), device="cuda:0")
    sep.load_variables((fx or tro.fixture(geo))["variables"])
    return sep


def _mix(fx):
    return torch.from_numpy(fx["mix"][:, :, None]).cuda()


def _targets(fx):
    return torch.from_numpy(fx["targets"][..., None]).cuda()


def _forward(sep, fx):
    outs = sep.get_output(_mix(fx), True, return_spectrogram=True)
    return torch.stack([outs[k] for k in sep.source_names])


def _oracles(geo, rate):
    """(fixture, the float64 and the float32 training forward) -- computed once, never changed."""
    key = (geo, rate)
    if key not in _CACHE:
        fx = tro.fixture(geo)
        args = (fx["mix"], fx["variables"], fx["L"], fx["nif"], fx["n_fft"], fx["hop"], tro.fixture_masks(fx, rate))
        _CACHE[key] = (fx, tro.train_forward(*args), tro.train_forward(*args, dtype=torch.float32))
    return _CACHE[key]


def _l1_upstream(sep, fx, mags):
    """d_mags [S, B, F, K] of Jansson's L1, the sign taken in float32 from the GPU's own mags and target magnitudes."""
    R = spectral.stft_magnitude(_targets(fx), fx["n_fft"], fx["hop"], transform="fft")[:, :, 0]
    cm = np.float32(1.0 / float(mags.numel()))
    return (-torch.sign(R - mags)) * cm


def _mse_upstream(audio, fx):
    return 2.0 * (audio - _targets(fx)) / float(audio.numel())


def _audio(sep):
    a = sep.audio_output()
    return torch.stack([a[k] for k in sep.source_names])


def _check_gradients(name, sep, fx, f64, f32, d_mags=None, d_audio=None):
    """sep.grads against the oracle, which is given the GPU's own upstream gradients."""
    cpu = lambda g: None if g is None else g.detach().cpu().numpy().astype(np.float64)
    dm, da = cpu(d_mags), None if d_audio is None else cpu(d_audio)[..., 0]
    g64, floors, _ = bo.gradients(f64, fx["mix"], fx["n_fft"], fx["hop"], d_mags=dm, d_audio=da)
    g32, _, _ = bo.gradients(f32, fx["mix"], fx["n_fft"], fx["hop"], d_mags=dm, d_audio=da)
    grads = sep.gradients()
    worst = 0.0
    for k, want in g64.items():
        got = grads[k].cpu().numpy()
        assert got.shape == tuple(want.shape), k
        if k.split("/")[-1].startswith("moving"):
            assert (got == 0.0).all(), k
            continue
        err, bound = _rule(got, want.numpy(), g32[k].numpy(), floor_scale=floors[k])
        print("[grad] %-44s err %.3e bound %.3e max|g| %.3e floor scale %.3e" % (k, err, bound, float(want.abs().max()), floors[k]))
        worst = max(worst, err / bound)
        assert np.isfinite(got).all() and err <= bound, (k, err, bound)
    assert any(float(g64[k].abs().max()) > 0 for k in g64)
    record(name, "worst gradient err / bound", worst, 1.0)


@pytest.mark.parametrize("geo", ["skip", "five", "flat_b1"])
def test_l1_upstream_gives_the_bits_of_loss_and_gradients(geo):
    fx = tro.fixture(geo)
    sep = _separator(geo, fx)                                # dropout 0.5
    mags = _forward(sep, fx)
    sep.loss_and_gradients(_targets(fx))
    ref = sep.grads.clone()
    assert float(ref.abs().max()) > 0
    sep.grads.fill_(float("nan"))
    sep.backward(d_mags=_l1_upstream(sep, fx, mags))
    assert _same_bits(ref, sep.grads)
    for k, g in sep.gradients().items():                     # every gradient tensor, by name
        if not k.split("/")[-1].startswith("moving"):
            assert float(g.abs().max()) > 0, k


@pytest.mark.parametrize("rate", [0.0, 0.5])
@pytest.mark.parametrize("geo", ["skip", "five"])
def test_audio_output_against_float64(geo, rate):
    fx, f64, f32 = _oracles(geo, rate)
    sep = _separator(geo, fx, spec_dropout=rate)
    _forward(sep, fx)
    ws = sep._tws[(fx["B"], fx["T"])]
    ws0, p0 = ws.clone(), sep.params.clone()
    got = _audio(sep)
    assert got.shape == (2, fx["B"], fx["T"], 1)
    assert torch.equal(ws.view(torch.int32), ws0.view(torch.int32)) and torch.equal(sep.params.view(torch.int32), p0.view(torch.int32))
    want64 = torch.stack(bo.audio_output(f64, fx["mix"], fx["n_fft"], fx["hop"])).numpy()
    want32 = torch.stack(bo.audio_output(f32, fx["mix"], fx["n_fft"], fx["hop"])).numpy()
    err, bound = _rule(got[..., 0].cpu().numpy(), want64, want32)
    record("test_audio_output_against_float64[%s-%.1f]" % (geo, rate), "err / bound", err / bound, 1.0)
    assert err <= bound, (err, bound)
    assert _same_bits(got, _audio(sep)) and got.data_ptr() != _audio(sep).data_ptr()     # repeatable, fresh tensors


@pytest.mark.parametrize("geo", ["skip", "flat", "five", "flat_b1"])
def test_raw_audio_step_against_float64(geo):
    """Training.py:62-63: forward, the audio, d_audio = 2 (audio - target) / (S B T) on the device, backward, Adam."""
    fx, f64, f32 = _oracles(geo, 0.5)
    sep = _separator(geo, fx)
    _forward(sep, fx)
    d_audio = _mse_upstream(_audio(sep), fx)
    sep.backward(d_audio=d_audio)
    _check_gradients("test_raw_audio_step_against_float64[%s]" % geo, sep, fx, f64, f32, d_audio=d_audio)
    p0 = sep.params.clone()
    sep.adam_step(1e-3)
    torch.cuda.synchronize()
    assert sep.global_step == 1 and not torch.equal(p0, sep.params) and bool(torch.isfinite(sep.params).all())


def test_both_domains_at_once_against_float64():
    fx, f64, f32 = _oracles("five", 0.5)
    sep = _separator("five", fx)
    mags = _forward(sep, fx)
    d_mags, d_audio = _l1_upstream(sep, fx, mags), _mse_upstream(_audio(sep), fx)
    sep.backward(d_mags={k: d_mags[i] for i, k in enumerate(sep.source_names)}, d_audio=d_audio)      # a dict and a stacked tensor
    _check_gradients("test_both_domains_at_once_against_float64", sep, fx, f64, f32, d_mags=d_mags, d_audio=d_audio)
    both = sep.grads.clone()
    sep.backward(d_audio=d_audio)
    assert not _same_bits(both, sep.grads)                   # (the magnitude term was in it)


@pytest.mark.parametrize("geo", ["skip", "five"])
def test_backward_repeats_its_bits(lib, geo):
    fx = tro.fixture(geo)
    sep = _separator(geo, fx)
    B, T, S = fx["B"], fx["T"], 2
    mags = _forward(sep, fx)
    d_mags, d_audio, tg = _l1_upstream(sep, fx, mags), _mse_upstream(_audio(sep), fx), _targets(fx)
    sep.backward(d_mags=d_mags, d_audio=d_audio)
    ref = sep.grads.clone()
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
    sep.backward(d_mags=d_mags, d_audio=d_audio)             # twice
    assert _same_bits(ref, sep.grads)
    sep.loss_and_gradients(tg)                               # after loss_and_gradients ...
    l1 = sep.grads.clone()
    sep.backward(d_mags=d_mags, d_audio=d_audio)
    assert _same_bits(ref, sep.grads)
    sep.loss_and_gradients(tg)                               # ... and before it
    assert _same_bits(l1, sep.grads)
    # what the scratch held, guard floats around the scratch and the gradients
    ns = int(lib.wun_spec_backward_scratch_floats(C.byref(sep._scfg), B, T))
    for fill in (float("nan"), 0.0):
        sbuf, sep._scr[("backward", B, T)] = _guarded(ns, fill)
        gbuf, sep.grads = _guarded(sep.num_params, fill)
        sep.backward(d_mags=d_mags, d_audio=d_audio)
        torch.cuda.synchronize()
        assert _same_bits(ref, sep.grads) and _guards_intact(sbuf, ns) and _guards_intact(gbuf, sep.num_params)
    # every buffer one float off 16 bytes, on a side stream, through the C ABI
    nw = int(lib.wun_spec_train_workspace_floats(C.byref(sep._scfg), B, T))
    wbuf, ws = _guarded(nw, 0.0, 1)
    ws.copy_(sep._tws[(B, T)])
    sbuf, scratch = _guarded(ns, float("nan"), 1)
    gbuf, grads = _guarded(sep.num_params, float("nan"), 1)
    params, dm, da = _offset_copy(sep.params), _offset_copy(d_mags.contiguous()), _offset_copy(d_audio.contiguous())
    assert all(t.data_ptr() % 8 == 4 for t in (ws, scratch, grads, params, dm, da))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _lib.check(lib.wun_spec_backward(C.byref(sep._scfg), C.byref(sep._tcfg), params.data_ptr(), dm.data_ptr(), da.data_ptr(), B, T,
                                         spectral._fft_table(fx["n_fft"], ws.device).data_ptr(), grads.data_ptr(), ws.data_ptr(),
                                         scratch.data_ptr(), C.c_void_p(side.cuda_stream)))
    torch.cuda.synchronize()
    assert _same_bits(ref, grads)
    assert _guards_intact(wbuf, nw, 1) and _guards_intact(sbuf, ns, 1) and _guards_intact(gbuf, sep.num_params, 1)


def test_update_moving_averages_is_adam_steps_update():
    fx = tro.fixture("skip")
    a, b = _separator("skip", fx), _separator("skip", fx)
    for sep in (a, b):
        _forward(sep, fx)
        sep.backward(d_audio=_mse_upstream(_audio(sep), fx))
    p0 = a.params.clone()
    a.adam_step(0.0)
    b.update_moving_averages()
    assert _same_bits(a.params, b.params) and not _same_bits(a.params, p0)
    assert a.global_step == 1 and b.global_step == 0
    moved = [n for n, off, shp in a.variable_table() if not torch.equal(a.params[off:off + int(np.prod(shp))], p0[off:off + int(np.prod(shp))])]
    assert len(moved) == 2 * 2 * 3 and all(n.split("/")[-1].startswith("moving") for n in moved)


# ------------------------------------------------------------------------------------------------ the module
def test_module_gradient_is_backwards_bits():
    fx = tro.fixture("skip")
    sep = _separator("skip", fx)
    net = sep.module("audio")
    assert isinstance(net, SpecUNet) and net.training and net.arena.data_ptr() == sep.params.data_ptr()
    assert [p.data_ptr() for p in net.parameters()] == [sep.params.data_ptr()]
    mix, tg = _mix(fx), _targets(fx)
    y = net(mix)
    assert y.shape == (2, fx["B"], fx["T"], 1) and y.requires_grad
    y.retain_grad()
    loss = ((y - tg) ** 2).mean()
    loss.backward()
    assert net.arena.grad is not None and float(net.arena.grad.abs().max()) > 0
    assert _same_bits(y, _audio(sep))                        # the separator's accessors read the same forward
    want = 2.0 * (y.detach() - tg) / float(y.numel())
    assert float((y.grad - want).abs().max()) <= 4 * 2.0 ** -24 * float(want.abs().max())
    sep.backward(d_audio=y.grad)
    assert _same_bits(net.arena.grad, sep.grads)
    vg = net.variable_grads()
    for name, off, shp in sep.variable_table():
        assert vg[name].shape == tuple(shp)
        assert (float(vg[name].abs().max()) == 0.0) == name.split("/")[-1].startswith("moving"), name
    assert net(mix).data_ptr() != y.data_ptr()               # fresh output tensors

    both = sep.module("both")
    audio, mags = both(mix)
    assert audio.shape == y.shape and mags.shape == (2, fx["B"], fx["F"], fx["n_fft"] // 2 + 1)
    audio.retain_grad(), mags.retain_grad()
    R = spectral.stft_magnitude(tg, fx["n_fft"], fx["hop"], transform="fft")[:, :, 0]
    (((audio - tg) ** 2).mean() + (R - mags).abs().mean()).backward()
    sep.backward(d_mags=mags.grad, d_audio=audio.grad)
    assert _same_bits(both.arena.grad, sep.grads)
    only = sep.module("both")                                # a loss on one of the two outputs
    audio, mags = only(mix)
    mags.retain_grad()
    (R - mags).abs().mean().backward()
    sep.backward(d_mags=mags.grad)
    assert _same_bits(only.arena.grad, sep.grads)


def test_module_refuses_a_stale_workspace_and_a_mix_that_requires_grad():
    fx = tro.fixture("skip")
    net = _separator("skip", fx).module("audio")
    mix = _mix(fx)
    y1 = net(mix)
    y2 = net(mix)
    with pytest.raises(RuntimeError, match="another training forward"):
        y1.sum().backward()
    y2.sum().backward()                                      # the latest forward's backward runs
    assert net.arena.grad is not None
    with pytest.raises(NotImplementedError, match="gradient with respect to the mix"):
        net(mix.clone().requires_grad_(True))


def test_module_eval_is_inference():
    fx = tro.fixture("skip")
    sep = _separator("skip", fx)
    mix = _mix(fx)
    for output in ("audio", "mags", "both"):
        net = sep.module(output).eval()
        got = net(mix)
        got = got if isinstance(got, tuple) else (got,)
        want = [torch.stack([o[k] for k in sep.source_names]).clone() for o in
                (sep.get_output(mix, False, return_spectrogram=r) for r in {"audio": (False,), "mags": (True,), "both": (False, True)}[output])]
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert _same_bits(g, w) and not g.requires_grad and g.grad_fn is None
        assert net.dropout_step == 0                         # eval does not advance the counter


def test_module_dropout_step_keys_the_masks():
    fx = tro.fixture("skip")
    sep = _separator("skip", fx)
    sep.global_step = 3
    net = sep.module("mags")
    assert net.dropout_step == 3
    shape = tro.dropout_shapes(fx)[0]
    mix = _mix(fx)
    for step in (3, 4):
        net(mix)
        assert net.dropout_step == step + 1
        assert np.array_equal(sep.activation("dropout", 1, 0).cpu().numpy(), tro.dropout_multipliers(tro.DROPOUT_SEED, step, 1, 0, shape, 0.5))
    net.dropout_step = 9                                     # settable
    net(mix)
    assert np.array_equal(sep.activation("dropout", 0, 0).cpu().numpy(), tro.dropout_multipliers(tro.DROPOUT_SEED, 9, 0, 0, shape, 0.5))
    assert sep.global_step == 3


def test_a_project_loss_through_the_module():
    """waveform.WaveformLoss (SI-SDR) on the module's audio: its autograd wrapper takes [S, B, T, 1]."""
    fx = tro.fixture("skip")
    sep = _separator("skip", fx)
    net = sep.module("audio")
    loss = waveform.WaveformLoss({"si_sdr": 1.0})(net(_mix(fx)), _targets(fx))
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(net.arena.grad).all())
    for name, g in net.variable_grads().items():
        if name.endswith("/kernel"):
            assert float(g.abs().max()) > 0, name


def test_it_learns_through_the_module():
    """200 steps of torch.optim.Adam(lr=1e-3) on the MSE of the module's audio, on _specunet_train_np.learn_fixture() without
    dropout.  The float32 CPU restatement of the same steps (_specunet_backward_np.mse_learning_curve: the oracle plus
    _specunet_train_np.adam) goes from 0.07336 to 0.01423, a ratio r = 0.1940; the test asks for at most sqrt(r) = 0.4404, halfway
    to 1 on a log scale."""
    fx = tro.learn_fixture()
    sep = _separator("skip", fx, spec_dropout=0.0)
    net = sep.module("audio")
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    mix, tg = _mix(fx), _targets(fx)
    losses = []
    for _ in range(200):
        opt.zero_grad()
        loss = ((net(mix) - tg) ** 2).mean()
        loss.backward()
        opt.step()
        net.update_moving_averages()
        losses.append(loss.detach())
    first, last = float(losses[0].item()), float(losses[-1].item())
    record("test_it_learns_through_the_module", "loss at step 199 / loss at step 0", last / first, 0.1940 ** 0.5)
    assert abs(first - 0.07336) < 1e-4 and np.isfinite(last) and last <= 0.1940 ** 0.5 * first
    assert net.dropout_step == 200
