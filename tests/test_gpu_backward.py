"""GPU tests of wun_backward (include/wun.h) -- get_output differentiated from an arbitrary upstream gradient, w.r.t. the
variables and the input mix -- and of the torch.autograd module built on it (wave_u_net_amd/autograd.py).

  * MSE equivalence: d_outputs = 2 / (S B Tout C) (y - target) gives wun_loss_backward's gradients (both modes);
  * a loss that is not MSE against the float64 oracle, evaluated on the kernels' own LeakyReLU branches (_gpu_pins):
    every variable's gradient and d loss / d mix (fp32 mode, every STEP_CASES entry and the benchmarked plan);
  * the bf16 mode's d_mix launch by launch: a float64 computation from the tensors mix_grad_kernel read;
  * torch.autograd through WaveUNet, its stale-workspace and version guards, and bitwise determinism."""
import os

import numpy as np
import pytest
import torch

from oracle import shapes, waveunet_torch as wt
from oracle.golden_params import GOLDEN_CASES, golden_params
from _observed import record
from test_gpu_parity import GRAD_TOL_PINNED, STEP_CASES, _gpu_pins, _grad_check

import wave_u_net_amd as wun
from wave_u_net_amd import _lib
from wave_u_net_amd.separator import UnetAudioSeparator

pytestmark = pytest.mark.gpu

MSE_EQ_TOL = 1e-6        # x max|g| per tensor: wun_backward vs wun_loss_backward, same plan, same forward pass
BF16_MIX_TOL = 2e-6      # x max|ref|: the bf16 mode's d_mix vs float64 from the tensors the launch read (as the emulation checks)
_W_SRC = [1.0, 0.5, 2.0, 0.25]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def _custom_loss(y, t, scale=1.0):
    """sum_s w_s mean(log cosh(3 (y_s - t_s))) + 0.1 mean(y_0^3) on stacked [S, B, T, C] -- not MSE, and smooth (an L1 term's
    sign would differ between the fp32 outputs and the float64 oracle's wherever y == t within rounding)."""
    loss = 0
    for s in range(y.shape[0]):
        d = 3.0 * (y[s] - t[s])
        loss = loss + _W_SRC[s] * (torch.logaddexp(d, -d) - np.log(2.0)).mean()
    return (loss + 0.1 * (y[0] ** 3).mean()) * scale


def _setup(name, B=3, **over):
    case = GOLDEN_CASES[name]
    ocfg = shapes.finalize_config(dict(shapes.BASE_MODEL_CONFIG, **case["cfg"]))
    params = golden_params(ocfg, case["seed"])
    sep = UnetAudioSeparator(wun.get_config("baseline", **dict(case["cfg"], **over)), device="cuda:0")
    i, o = shapes.get_padding(ocfg, [B, case["frames"], 0])
    mix, targets = wt.synthetic_batch(ocfg, B, i[1], o[1], seed=case["seed"] + 100)
    sep._plan(B, i[1]); sep._active = sep._plans[(B, i[1])]
    sep.load_variables(params)
    tg = torch.stack([torch.from_numpy(targets[n]) for n in ocfg["source_names"]]).cuda()
    return sep, ocfg, params, torch.from_numpy(mix).cuda(), tg


def _upstream(outs, names, tg):
    """d_outputs of _custom_loss at the GPU's outputs (torch autograd on the stacked outputs)."""
    y = torch.stack([outs[n] for n in names]).clone().requires_grad_(True)
    _custom_loss(y, tg).backward()
    return y.grad.detach()


def _oracle_custom(ocfg, params, mix, tg, pins, chunk=None):
    """float64 oracle of _custom_loss on the kernels' LeakyReLU branches: (tp, parameter grads, d loss / d mix), one chunk
    of excerpts at a time (the means over the batch split into per-chunk means weighted chunk / B)."""
    B = mix.shape[0]
    chunk = chunk or B
    tp = wt.params_to_torch(params, torch.float64, requires_grad=True)
    dmix = torch.zeros(tuple(mix.shape), dtype=torch.float64)
    hmix, htg = mix.cpu().double(), tg.cpu().double()
    for lo in range(0, B, chunk):
        m = hmix[lo:lo + chunk].clone().requires_grad_(True)
        cp = {k: (v[0][lo:lo + chunk], v[1][lo:lo + chunk]) for k, v in pins.items()}
        o = wt.get_output(ocfg, tp, m, True, pins=cp)
        y = torch.stack([o[n] for n in ocfg["source_names"]])
        _custom_loss(y, htg[:, lo:lo + chunk], m.shape[0] / B).backward()
        dmix[lo:lo + chunk] = m.grad
    return tp, [p.grad for _, p in tp], dmix


def _mix_check(got, ref, tag, tol=GRAD_TOL_PINNED):
    got = got.cpu().double()
    assert torch.isfinite(got).all()
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    record("d_mix_vs_float64_oracle", tag, err / max(scale, 1e-30), tol)
    assert err <= tol * scale + 1e-7, (err, scale)


def _mse_upstream(outs, tg):
    S, B, T, C = outs.shape
    return (2.0 / (S * B * T * C)) * (outs - tg)


def _per_tensor_equal(sep, g_ref, g_new, tol, tag):
    for name, off, shp in sep._active.tensors:
        n = int(np.prod(shp))
        a, b = g_ref[off:off + n].double(), g_new[off:off + n].double()
        scale = a.abs().max().item()
        assert (a - b).abs().max().item() <= tol * scale, (tag, name, (a - b).abs().max().item(), scale)


def _mse_equivalence(sep, mix, tg, tag):
    outs = sep.get_output(mix, True)
    sep.loss_and_gradients(tg)
    g_ref = sep.grads.clone()
    stacked = sep._outs[sep._last_key]
    sep.grads.fill_(float("nan"))
    assert sep.backward(_mse_upstream(stacked, tg)) is None
    torch.cuda.synchronize()
    _per_tensor_equal(sep, g_ref, sep.grads, MSE_EQ_TOL, tag)
    return outs


# ---------------------------------------------------------------------------------------------------- MSE equivalence
@pytest.mark.parametrize("name", STEP_CASES)
def test_mse_upstream_matches_loss_backward_fp32(lib, name):
    sep, ocfg, params, mix, tg = _setup(name)
    _mse_equivalence(sep, mix, tg, name)


BF16_CASES = {   # (golden case, overrides): small M4- / M5-shaped configs and one shaped like deep_l16_f48 (same padding)
    "m4_shaped": ("baseline_stereo_small", {}),
    "m5_shaped": ("full_small", {}),
    "deep_l16_f48_shaped": ("baseline_small", dict(num_layers=4, num_initial_filters=48, mono_downmix=False,
                                                   task="multi_instrument", output_type="difference")),
}


def _setup_bf16(key, B=2):
    name, over = BF16_CASES[key]
    case = GOLDEN_CASES[name]
    cfg_over = dict(case["cfg"], **over)
    ocfg = shapes.finalize_config(dict(shapes.BASE_MODEL_CONFIG, **cfg_over))
    params = golden_params(ocfg, case["seed"])
    sep = UnetAudioSeparator(wun.get_config("baseline", compute_dtype="bf16", **cfg_over), device="cuda:0")
    frames = 160 if not ocfg["context"] else case["frames"]
    i, o = shapes.get_padding(ocfg, [B, frames, 0])
    mix, targets = wt.synthetic_batch(ocfg, B, i[1], o[1], seed=case["seed"] + 200)
    sep._plan(B, i[1]); sep._active = sep._plans[(B, i[1])]
    sep.load_variables(params)
    assert sep.effective_dtype == "bf16"
    tg = torch.stack([torch.from_numpy(targets[n]) for n in ocfg["source_names"]]).cuda()
    return sep, ocfg, params, torch.from_numpy(mix).cuda(), tg


@pytest.mark.parametrize("key", sorted(BF16_CASES))
def test_mse_upstream_matches_loss_backward_bf16(lib, key):
    sep, ocfg, params, mix, tg = _setup_bf16(key)
    assert sep.model_config["num_initial_filters"] % 8 == 0
    _mse_equivalence(sep, mix, tg, "bf16_" + key)
    assert sep.effective_dtype == "bf16"


# ------------------------------------------------------------------------------ arbitrary loss vs the float64 oracle
@pytest.mark.parametrize("name", STEP_CASES)
def test_custom_loss_gradients_and_mix_gradient_vs_oracle(lib, name):
    sep, ocfg, params, mix, tg = _setup(name)
    names = ocfg["source_names"]
    outs = sep.get_output(mix, True)
    dout = _upstream(outs, names, tg)
    pins = _gpu_pins(sep, ocfg)
    d_mix = sep.backward(dout, input_grad=True)
    torch.cuda.synchronize()
    tp, ograds, odmix = _oracle_custom(ocfg, params, mix, tg, pins)
    _grad_check(sep, tp, ograds, tol=GRAD_TOL_PINNED, tag="custom_loss_" + name)
    assert tuple(d_mix.shape) == tuple(mix.shape)
    _mix_check(d_mix, odmix, "custom_loss_" + name)


def test_benchmarked_configuration_custom_loss_vs_oracle(lib):
    """The plan bench.py times -- configs[1], M1 with context, B = 16, 147443 -> 16389, the pinned tuning table when it
    matches this build -- differentiated from _custom_loss: every gradient and d_mix against the branch-pinned float64 oracle."""
    from wave_u_net_amd.training import Trainer, synthetic_source
    cfg = wun.get_config("m1_context")
    table = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "round6_tune_table.txt")
    text = open(table).read() if os.path.exists(table) else None
    tr = Trainer(cfg, batch_size=16)
    assert (tr.t_in, tr.t_out) == (147443, 16389)
    mix, targets = synthetic_source(cfg, 16, tr.t_in, tr.t_out, tr.device, seed=1337)()
    tr.tune(mix, targets, pinned_table=text)
    sep = tr.sep
    assert sep.tune_export().startswith("wun-tune 2 ")
    names = cfg["source_names"]
    outs = sep.get_output(mix, True)
    tg = torch.stack([targets[k] for k in range(len(names))]).to(torch.float32) if not torch.is_tensor(targets) \
        else targets.to(torch.float32)
    dout = _upstream(outs, names, tg)
    d_mix = sep.backward(dout, input_grad=True)
    torch.cuda.synchronize()
    ocfg = shapes.finalize_config(dict(shapes.BASE_MODEL_CONFIG, context=True))
    pins = _gpu_pins(sep, ocfg)
    var = sep.variables()
    params = [(n, var[n].detach().cpu().numpy()) for n, _, _ in sep._active.tensors]
    tp, ograds, odmix = _oracle_custom(ocfg, params, mix, tg, pins, chunk=1)
    _grad_check(sep, tp, ograds, tol=GRAD_TOL_PINNED, tag="custom_loss_bench_config_B16_tuned")
    _mix_check(d_mix, odmix, "custom_loss_bench_config_B16_tuned")


# ------------------------------------------------------------------------------------ bf16 mode: d_mix launch-level
def _bf16_mix_reference(sep, ocfg, params, mix, outs, dout):
    """float64 d_mix from what mix_grad_kernel read: level 0's stored d(pre-activation) (dz_skip / dz_dec), the head's dpre
    recomputed from d_outputs and the outputs, the fp32 mix geometry and weights."""
    same = not ocfg["context"]
    names = ocfg["source_names"]
    S, C = len(names), ocfg["num_channels"]
    L = ocfg["num_layers"]
    prm = dict(params)
    B, Tin = mix.shape[0], mix.shape[1]
    x = torch.zeros(B, C, Tin, dtype=torch.float64, requires_grad=True)
    # down conv 0: its full-rate conv-output gradient assembled from the stored parts (both parts add where both exist)
    W0 = torch.tensor(prm[[n for n, _ in params if n.endswith("/kernel")][0]], dtype=torch.float64)
    z = wt.conv1d_tf(x, W0, None, same)
    G = torch.zeros(z.shape, dtype=torch.float64)
    for kind in (("dz_skip",) if same else ("dz_skip", "dz_dec")):
        v, t0, ts = sep.activation(kind, 0)
        G[:, :, t0:t0 + v.shape[2] * ts:ts] += v.cpu().double()
    total = (z * G).sum()
    # head: dpre from the upstream gradient, the mix-channel rows of every source's output kernel
    outs = outs.cpu().double()
    d = dout.cpu().double()
    diff = ocfg["output_type"] == "difference"
    Sh = S - 1 if diff else S
    feat_len = sep.activation("up", L - 1)[0].shape[2]
    xc = wt.crop(x, feat_len)
    heads = [n for n, _ in params if n.endswith("/kernel")][-Sh:]
    for s in range(Sh):
        g = d[s] - (d[S - 1] if diff else 0)
        if ocfg["output_activation"] == "tanh":
            g = g * (1 - outs[s] ** 2)
        Wh = torch.tensor(prm[heads[s]], dtype=torch.float64)[:, :C, :]
        pre = wt.conv1d_tf(xc, Wh, None, same)                            # [B, C, Tout]
        total = total + (pre * g.permute(0, 2, 1)).sum()
    if diff:
        last = wt.crop(xc, outs.shape[2])
        total = total + (last * d[S - 1].permute(0, 2, 1)).sum()
    total.backward()
    return x.grad.permute(0, 2, 1)


@pytest.mark.parametrize("key", sorted(BF16_CASES))
def test_bf16_mix_gradient_launch_level(lib, key):
    sep, ocfg, params, mix, tg = _setup_bf16(key)
    outs = sep.get_output(mix, True)
    dout = _upstream(outs, ocfg["source_names"], tg)
    d_mix = sep.backward(dout, input_grad=True)
    torch.cuda.synchronize()
    ref = _bf16_mix_reference(sep, ocfg, params, mix, sep._outs[sep._last_key], dout)
    _mix_check(d_mix, ref, "bf16_launch_level_" + key, tol=BF16_MIX_TOL)


# --------------------------------------------------------------------------------------------------------- autograd
def test_autograd_module_matches_backward_and_oracle(lib):
    name = "full_multi_small"
    sep, ocfg, params, mix, tg = _setup(name)
    net = sep.module()
    assert net.arena.data_ptr() == sep.params.data_ptr()
    m = mix.clone().requires_grad_(True)
    y = net(m)
    assert y.requires_grad and tuple(y.shape) == (len(ocfg["source_names"]),) + tuple(tg.shape[1:])
    pins = _gpu_pins(sep, ocfg)
    ga, gm = torch.autograd.grad(_custom_loss(y, tg), [net.arena, m])
    # the same through separator.backward (same forward, bitwise)
    outs = sep.get_output(mix, True)
    assert torch.equal(torch.stack([outs[n] for n in ocfg["source_names"]]), y.detach())
    d_mix = sep.backward(_upstream(outs, ocfg["source_names"], tg), input_grad=True)
    torch.cuda.synchronize()
    assert torch.equal(ga, sep.grads) and torch.equal(gm, d_mix)
    tp, ograds, odmix = _oracle_custom(ocfg, params, mix, tg, pins)
    _grad_check(sep, tp, ograds, tol=GRAD_TOL_PINNED, tag="autograd_" + name)
    _mix_check(gm, odmix, "autograd_" + name)


def test_autograd_bf16_mix_gradient(lib):
    sep, ocfg, params, mix, tg = _setup_bf16("m4_shaped")
    net = sep.module()
    m = mix.clone().requires_grad_(True)
    y = net(m)
    ga, gm = torch.autograd.grad(_custom_loss(y, tg), [net.arena, m])
    yd = y.detach()
    dout = _upstream({n: yd[k] for k, n in enumerate(ocfg["source_names"])}, ocfg["source_names"], tg)
    ref = _bf16_mix_reference(sep, ocfg, params, mix, yd, dout)
    _mix_check(gm, ref, "autograd_bf16_m4_shaped", tol=BF16_MIX_TOL)


def test_autograd_adam_padding_and_no_input_grad(lib):
    sep, ocfg, params, mix, tg = _setup("baseline_context_small")
    net = sep.module()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    y = net(mix)                                            # mix does not require grad
    _custom_loss(y, tg).backward()
    g = net.arena.grad
    covered = torch.zeros(g.numel(), dtype=torch.bool)
    for _, off, shp in net.tensors:
        covered[off:off + int(np.prod(shp))] = True
    assert (g.cpu()[~covered] == 0).all()                   # padding floats 0
    assert torch.isfinite(g).all() and g.abs().max().item() > 0
    before = net.arena.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(before, net.arena.detach())
    assert torch.equal(sep.params, net.arena.detach())      # the separator sees the update (shared storage)
    m = mix.clone()
    y = net(m)
    assert torch.autograd.grad(_custom_loss(y, tg), [net.arena])[0].shape == net.arena.shape
    assert m.grad is None
    # eval(): AudioClip, no grad
    net.eval()
    ye = net(mix)
    assert not ye.requires_grad
    ref = sep.get_output(mix, False)
    assert torch.equal(ye, torch.stack([ref[n] for n in ocfg["source_names"]]))


def test_autograd_stale_workspace_and_version_guards(lib):
    sep, ocfg, params, mix, tg = _setup("baseline_small")
    net = sep.module()
    ya = net(mix)
    yb = net(mix + 0.01)                                    # same shape: overwrites the shared workspace
    with pytest.raises(RuntimeError, match="workspace"):
        _custom_loss(ya, tg).backward()
    _custom_loss(yb, tg).backward()                         # the latest forward is still fine
    # the separator's own get_output counts as a forward on that workspace too
    yc = net(mix)
    sep.get_output(mix, True)
    with pytest.raises(RuntimeError, match="workspace"):
        _custom_loss(yc, tg).backward()
    # an in-place edit of the arena between forward and backward: torch's version check
    yd = net(mix)
    with torch.no_grad():
        net.arena.mul_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        _custom_loss(yd, tg).backward()


# ------------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_backward_is_bitwise_deterministic(lib, mode):
    if mode == "f32":
        sep, ocfg, params, mix, tg = _setup("full_small")
    else:
        sep, ocfg, params, mix, tg = _setup_bf16("m5_shaped")
    outs = sep.get_output(mix, True)
    dout = _upstream(outs, ocfg["source_names"], tg)
    runs = []
    for _ in range(2):
        d_mix = sep.backward(dout, input_grad=True)
        torch.cuda.synchronize()
        runs.append((sep.grads.clone(), d_mix))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
