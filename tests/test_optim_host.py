"""CPU-only checks of the extended optimizer (include/wun.h: wun_optim_step, wun_ema_update, wun_optim_abi_size; DESIGN.md
5.26): the float64 oracle of tests/_optim_np.py against torch.optim.AdamW and a transcription of TF's assign_moving_average,
training.lr_factor at the edges of every kind, the config checks, the SpectrogramTrainer's refusals, the checkpoint entry
names with and without an EMA, and every argument refusal of the two entries on a plan built without a GPU."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _optim_np as onp

import wave_u_net_amd as wun
from wave_u_net_amd import _lib, checkpoint, tf_checkpoint
from wave_u_net_amd.separator import UnetAudioSeparator, check_ema_decay, check_weight_decay
from wave_u_net_amd.training import (SpectrogramTrainer, lr_factor, optimizer_settings, schedule_settings, scheduled_lr)

WUN_ERR_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _small_cfg(**kw):
    return wun.get_config("baseline", **dict(dict(num_layers=2, num_initial_filters=8, filter_size=5, context=True,
                                                  output_type="difference", task="multi_instrument"), **kw))


@pytest.fixture(scope="module")
def plan():
    s = UnetAudioSeparator(_small_cfg())
    i, _ = s.get_padding(np.array([2, 1, 0]))
    return s._plan(2, int(i[1]))


# ------------------------------------------------------------------------------------------------ ABI surface
def test_symbols_declared_exported_and_bound(lib):
    assert lib.wun_optim_abi_size() == C.sizeof(_lib.WunOptimConfig) == 28
    assert [n for n, _ in _lib.WunOptimConfig._fields_] == ["beta1", "beta2", "eps", "weight_decay", "ema_decay", "clip_norm",
                                                             "flags"]
    sizes = (C.c_int64 * 4)()
    assert lib.wun_abi_sizes(sizes, 4) == 3                     # wun_abi_sizes keeps its three entries
    assert len(lib.wun_optim_step.argtypes) == 17 and len(lib.wun_ema_update.argtypes) == 9
    assert lib.wun_optim_step.argtypes[-4:] == lib.wun_adam_step_select.argtypes[-2:] * 2


# ------------------------------------------------------------------------------------------------ the oracle
def test_float64_oracle_matches_torch_adamw():
    """5 steps of torch.optim.AdamW in float64 on two tensors, weight decay on the first only.  PyTorch puts eps outside the
    bias correction (sqrt(v) / sqrt(1 - b2^t) + eps); eps_t = eps / sqrt(1 - b2^t) per step turns that into TF's placement."""
    rng = np.random.default_rng(5)
    lr, b1, b2, eps, wd = 3e-3, 0.9, 0.999, 1e-8, 0.05
    n0, n1 = 37, 23
    p0 = rng.standard_normal(n0 + n1)
    decay = np.arange(n0 + n1) < n0
    tp = [torch.tensor(p0[:n0].copy(), dtype=torch.float64, requires_grad=True),
          torch.tensor(p0[n0:].copy(), dtype=torch.float64, requires_grad=True)]
    opt = torch.optim.AdamW([{"params": [tp[0]], "weight_decay": wd}, {"params": [tp[1]], "weight_decay": 0.0}], lr=lr,
                            betas=(b1, b2), eps=eps)
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for t in range(1, 6):
        g = rng.standard_normal(n0 + n1) * 10.0 ** rng.uniform(-3, 1)
        tp[0].grad = torch.tensor(g[:n0].copy())
        tp[1].grad = torch.tensor(g[n0:].copy())
        for group in opt.param_groups:
            group["eps"] = eps / math.sqrt(1.0 - b2 ** t)
        opt.step()
        p, m, v = onp.step64(p, g, m, v, t, lr, b1, b2, eps, weight_decay=wd, decay=decay)
        want = np.concatenate([tp[0].detach().numpy(), tp[1].detach().numpy()])
        assert np.max(np.abs(p - want) / np.abs(want)) <= 1e-12, t
    # the decay did reach the first tensor only: without it the second is unchanged, the first is not
    q, _, _ = onp.step64(p0, g, np.zeros_like(p0), np.zeros_like(p0), 1, lr, b1, b2, eps)
    r, _, _ = onp.step64(p0, g, np.zeros_like(p0), np.zeros_like(p0), 1, lr, b1, b2, eps, weight_decay=wd, decay=decay)
    assert np.array_equal(q[n0:], r[n0:]) and not np.array_equal(q[:n0], r[:n0])


@pytest.mark.parametrize("warmup", [False, True])
def test_ema_matches_assign_moving_average(warmup):
    rng = np.random.default_rng(9)
    ema, theta = rng.standard_normal(101), rng.standard_normal(101)
    for step in (1, 2, 9, 100, 8990, 8991, 10 ** 6):
        d = onp.tf_ema_decay(float(np.float32(0.999)), step if warmup else None)
        want = onp.assign_moving_average(ema, theta, d)
        got = onp.ema64(ema, theta, 0.999, step, warmup)
        assert np.max(np.abs(got - want)) <= 1e-15 * np.max(np.abs(want)), step
        # the float32 restatement stays within its three roundings of it
        e32, t32 = ema.astype(np.float32), theta.astype(np.float32)
        got32 = onp.ema32(e32, t32, 0.999, step, warmup)
        ref = onp.ema64(e32, t32, 0.999, step, warmup)
        ulp = np.spacing(np.maximum(np.abs(e32), np.abs(t32))).astype(np.float64)
        assert np.max(np.abs(got32 - ref) / ulp) <= 2.0
    assert onp.ema_weight(0.999, 1, True) == 1.0 - 2.0 / 11.0          # warm-up: min(0.999, 2 / 11)
    assert onp.ema_weight(0.5, 10 ** 6, True) == 0.5


# ------------------------------------------------------------------------------------------------ lr schedule
def test_lr_factor_edges():
    assert lr_factor(None, 0) == 1.0 == lr_factor(None, 10 ** 9)
    assert lr_factor({"kind": "constant"}, 0) == 1.0 == lr_factor({}, 7)
    warm = {"warmup_steps": 4}
    assert [lr_factor(warm, s) for s in range(6)] == [0.25, 0.5, 0.75, 1.0, 1.0, 1.0]
    cos = {"warmup_steps": 2, "kind": "cosine", "total_steps": 6, "min_factor": 0.1}
    assert lr_factor(cos, 0) == 0.5 and lr_factor(cos, 1) == 1.0                 # step 0, the last warm-up step
    assert lr_factor(cos, 2) == 1.0                                               # the cosine starts at 1
    assert lr_factor(cos, 4) == pytest.approx(0.1 + 0.9 * 0.5, abs=1e-15)
    assert lr_factor(cos, 6) == 0.1 == lr_factor(cos, 7) == lr_factor(cos, 10 ** 6)   # total_steps and beyond
    assert lr_factor(cos, 5) > 0.1
    cos0 = {"kind": "cosine", "total_steps": 4}
    assert lr_factor(cos0, 0) == 1.0 and lr_factor(cos0, 4) == 0.0 and lr_factor(cos0, 2) == pytest.approx(0.5, abs=1e-15)
    st = {"warmup_steps": 1, "kind": "step", "step_size": 3, "gamma": 0.5}
    assert [lr_factor(st, s) for s in (0, 1, 3, 4, 6, 7)] == [1.0, 1.0, 1.0, 0.5, 0.5, 0.25]
    ex = {"warmup_steps": 2, "kind": "exponential", "gamma": 0.9}
    assert [lr_factor(ex, s) for s in (0, 1, 2, 3, 5)] == [0.5, 1.0, 1.0, 0.9, 0.9 ** 3]
    for sched in (warm, cos, cos0, st, ex, None):
        for s in (0, 1, 2, 3, 4, 5, 6, 7, 50):
            assert lr_factor(sched, s) == onp.lr_factor(sched, s), (sched, s)
            assert isinstance(lr_factor(sched, s), float)
            # the Trainer keeps the checked copy and hands that one in at every step
            assert lr_factor(schedule_settings(sched), s) == lr_factor(sched, s)
        assert schedule_settings(schedule_settings(sched)) == schedule_settings(sched)
    # the step's lr: float32(init_sup_sep_lr * factor), the product in float64
    assert scheduled_lr(1e-4, cos, 4) == float(np.float32(1e-4 * lr_factor(cos, 4)))
    assert scheduled_lr(1e-4, None, 3) == float(np.float32(1e-4))
    with pytest.raises(ValueError):
        lr_factor(warm, -1)


@pytest.mark.parametrize("bad", [
    {"kind": "linear"}, {"warmup": 3}, {"warmup_steps": -1}, {"warmup_steps": 1.5}, {"warmup_steps": True},
    {"kind": "cosine"}, {"kind": "cosine", "total_steps": 0}, {"kind": "cosine", "total_steps": 5, "warmup_steps": 5},
    {"kind": "cosine", "total_steps": 5, "min_factor": 1.5}, {"kind": "cosine", "total_steps": 5, "min_factor": -0.1},
    {"kind": "cosine", "total_steps": 5, "gamma": 0.5}, {"kind": "step", "gamma": 0.5}, {"kind": "step", "step_size": 3},
    {"kind": "step", "step_size": 0, "gamma": 0.5}, {"kind": "step", "step_size": 2, "gamma": 0.0},
    {"kind": "step", "step_size": 2, "gamma": 1.5}, {"kind": "exponential"}, {"kind": "exponential", "gamma": math.nan},
    {"kind": "exponential", "gamma": 0.9, "step_size": 2}, {"kind": "constant", "total_steps": 5},
    {"kind": "constant", "min_factor": 0.5}, "cosine", [1, 2]])
def test_schedule_validation(bad):
    with pytest.raises(ValueError):
        schedule_settings(bad)
    with pytest.raises(ValueError):
        lr_factor(bad, 0)


def test_optimizer_validation():
    assert optimizer_settings(None) is None and schedule_settings(None) is None
    assert optimizer_settings({}) == {"weight_decay": 0.0, "decay_variables": None, "ema_decay": None, "ema_warmup": False,
                                      "eval_with_ema": False}
    full = optimizer_settings({"weight_decay": 0.01, "decay_variables": ["separator/conv1d/kernel"], "ema_decay": 0.999,
                               "ema_warmup": True, "eval_with_ema": True})
    assert full["weight_decay"] == 0.01 and full["ema_decay"] == 0.999 and full["ema_warmup"] and full["eval_with_ema"]
    for bad in ({"weight_decay": -1e-3}, {"weight_decay": math.nan}, {"weight_decay": "x"}, {"weight_decay": True},
                {"weight_decay": math.inf}, {"ema_decay": 1.0}, {"ema_decay": -0.1}, {"ema_decay": math.nan},
                {"ema_warmup": True}, {"eval_with_ema": True}, {"ema_decay": 0.9, "ema_warmup": 1},
                {"decay_variables": "separator/conv1d/kernel"}, {"decay_variables": [3]}, {"l2": 0.1}, "adamw"):
        with pytest.raises(ValueError):
            optimizer_settings(bad)
    for bad in (-1.0, math.nan, "x", True, math.inf):
        with pytest.raises(ValueError):
            check_weight_decay(bad)
    for bad in (1.0, 1.5, -0.01, math.nan, "x", True):
        with pytest.raises(ValueError):
            check_ema_decay(bad)
    assert check_ema_decay(0) == 0.0 and check_weight_decay(0) == 0.0
    cfg = wun.get_config("baseline")
    assert "optimizer" not in cfg and "lr_schedule" not in cfg                      # extension keys: absent = today's calls
    assert wun.config.EXTENSION_DEFAULTS["optimizer"] is None and wun.config.EXTENSION_DEFAULTS["lr_schedule"] is None


def test_trainer_refuses_bad_settings_at_construction():
    """Unknown keys and inconsistent values raise ValueError before the Trainer touches a device."""
    from wave_u_net_amd.training import Trainer
    cfg = _small_cfg()
    with pytest.raises(ValueError, match="optimizer"):
        Trainer(dict(cfg, optimizer={"decay": 0.1}))
    with pytest.raises(ValueError, match="lr_schedule"):
        Trainer(cfg, lr_schedule={"kind": "cosine"})
    with pytest.raises(ValueError, match="ema_decay"):
        Trainer(cfg, optimizer={"eval_with_ema": True})


@pytest.mark.parametrize("key,value", [("optimizer", {"weight_decay": 0.01}), ("lr_schedule", {"warmup_steps": 10})])
def test_spectrogram_trainer_refuses_the_new_keys(key, value):
    cfg = wun.get_config("unet_spectrogram_l1")
    with pytest.raises(NotImplementedError, match=key):
        SpectrogramTrainer(dict(cfg, **{key: value}))


def test_cli_override_reaches_the_settings():
    from wave_u_net_amd.__main__ import _parse, _weights
    _, name, over, opts = _parse(["train", "with", "cfg.full", 'model_config.optimizer={"weight_decay":0.01,"ema_decay":0.999}',
                                  'model_config.lr_schedule={"warmup_steps":100,"kind":"cosine","total_steps":1000}'])
    cfg = wun.get_config(name, **over)
    assert optimizer_settings(cfg["optimizer"])["ema_decay"] == 0.999
    assert schedule_settings(cfg["lr_schedule"])["total_steps"] == 1000
    _, _, _, opts = _parse(["predict", "with", "cfg.full", "weights=ema", "input_path=x.wav"])
    assert _weights(opts) == "ema" and _weights({}) is None
    with pytest.raises(SystemExit):
        _weights({"weights": "best"})


# ------------------------------------------------------------------------------------------------ checkpoints
def _cpu_separator():
    sep = UnetAudioSeparator(_small_cfg(), device="cpu")
    sep.variables()
    return sep


def test_checkpoint_entry_names(tmp_path):
    sep = _cpu_separator()
    names = [n for n, _, _ in sep.variable_table()]
    # without an EMA: exactly the entries save_checkpoint has always written
    p = checkpoint.save_checkpoint(sep, str(tmp_path / "a.npz"))
    assert sorted(np.load(p).files) == sorted(names + ["adam_m", "adam_v", "global_step"])
    t = checkpoint.save_checkpoint(sep, str(tmp_path / "a-tf"), "tf")
    want_tf = names + ["global_step", "separator_solver/beta1_power", "separator_solver/beta2_power"]
    want_tf += ["separator_solver/%s/Adam" % n for n in names] + ["separator_solver/%s/Adam_1" % n for n in names]
    assert sorted(n for n, _, _ in tf_checkpoint.list_variables(t)) == sorted(want_tf)
    # with one: ema/<variable>, and <variable>/ExponentialMovingAverage in the TF format
    sep._ensure_ema()
    sep.ema.mul_(0.5).add_(0.125)
    sep.global_step = 3
    p = checkpoint.save_checkpoint(sep, str(tmp_path / "b.npz"))
    assert sorted(np.load(p).files) == sorted(names + ["adam_m", "adam_v", "global_step"] + ["ema/" + n for n in names])
    t = checkpoint.save_checkpoint(sep, str(tmp_path / "b-tf"), "tf")
    assert sorted(n for n, _, _ in tf_checkpoint.list_variables(t)) == sorted(want_tf + [n + "/ExponentialMovingAverage"
                                                                                          for n in names])
    # round trip, both formats, bit for bit; with_optimizer=False still restores the EMA (it is weights)
    for path in (p, t):
        for with_opt in (True, False):
            other = _cpu_separator()
            assert other.ema is None
            assert checkpoint.load_checkpoint(other, path, with_optimizer=with_opt) == 3
            assert torch.equal(other.ema.view(torch.int32), sep.ema.view(torch.int32))
            assert torch.equal(other.params.view(torch.int32), sep.params.view(torch.int32))
    # a checkpoint without an EMA: a separator that keeps none gets none; one that keeps one starts it from the variables
    a = str(tmp_path / "a.npz")
    other = _cpu_separator()
    checkpoint.load_checkpoint(other, a)
    assert other.ema is None
    other._ensure_ema()
    other.ema.fill_(7.0)
    checkpoint.load_checkpoint(other, a)
    assert torch.equal(other.ema, other.params)
    with pytest.raises(RuntimeError, match="no EMA"):
        _cpu_separator().ema_variables()
    with pytest.raises(RuntimeError, match="no EMA"):
        with _cpu_separator().ema_weights():
            pass


def test_weights_context_errors():
    from wave_u_net_amd.evaluate import weights_context
    sep = _cpu_separator()
    with weights_context(sep, None):
        pass
    with weights_context(sep, "trained"):
        pass
    with pytest.raises(RuntimeError, match="no EMA"):
        weights_context(sep, "ema")
    with pytest.raises(ValueError):
        weights_context(sep, "best")
    sep._ensure_ema()
    sep.ema.add_(1.0)
    before = sep.params.clone()
    with pytest.raises(KeyError):
        with weights_context(sep, "ema"):
            assert torch.equal(sep.params, before + 1.0) and torch.equal(sep.ema, before)     # the arenas are exchanged
            raise KeyError("inside")
    assert torch.equal(sep.params, before)                      # restored after the exception


# ------------------------------------------------------------------------------------------------ argument refusals
# Non-null pointers that are never dereferenced: every call below must fail its argument check first.
_FAKE = C.c_void_p(0x1000)
_FAKE_MISALIGNED = C.c_void_p(0x1004)


def _mask(bits):
    m = np.asarray(bits, dtype=np.uint8)
    return m, m.ctypes.data_as(C.POINTER(C.c_uint8))


def _optim(lib, plan, handle=True, ptrs=(_FAKE,) * 4, ema=_FAKE, step=1, cfg="default", ws=_FAKE, skipped=_FAKE, sel=None,
           nsel=None, dec=None, ndec=None, **c):
    conf = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, ema_decay=0.999, clip_norm=1.0, flags=3)
    conf.update(c)
    sm, sp = _mask(sel) if sel is not None else (None, None)
    dm, dp = _mask(dec) if dec is not None else (None, None)
    nsel = (len(sm) if sm is not None else 0) if nsel is None else nsel
    ndec = (len(dm) if dm is not None else 0) if ndec is None else ndec
    wc = _lib.WunOptimConfig(*[conf[k] for k in ("beta1", "beta2", "eps", "weight_decay", "ema_decay", "clip_norm", "flags")])
    return lib.wun_optim_step(plan.handle if handle else None, *ptrs, ema, step, 1e-4, 1.0,
                              C.byref(wc) if cfg == "default" else None, ws, skipped, None, sp, nsel, dp, ndec)


def test_optim_step_argument_errors(lib, plan):
    nt = len(plan.tensors)
    assert _optim(lib, plan, handle=False) == WUN_ERR_INVALID
    for i in range(4):                                                    # params, grads, m, v
        ptrs = [_FAKE] * 4
        ptrs[i] = None
        assert _optim(lib, plan, ptrs=tuple(ptrs)) == WUN_ERR_INVALID, i
    assert _optim(lib, plan, cfg=None) == WUN_ERR_INVALID
    assert _optim(lib, plan, step=0) == WUN_ERR_INVALID
    for wd in (-1e-6, -math.inf, math.nan):
        assert _optim(lib, plan, weight_decay=wd) == WUN_ERR_INVALID, wd
        assert "weight_decay" in lib.wun_last_error().decode()
    for d in (1.0, 1.5, -0.1, math.nan):
        assert _optim(lib, plan, ema_decay=d) == WUN_ERR_INVALID, d
        assert "ema_decay" in lib.wun_last_error().decode()
    for clip in (0.0, -1.0, -math.inf, math.nan):
        assert _optim(lib, plan, clip_norm=clip) == WUN_ERR_INVALID, clip
        assert "clip_norm" in lib.wun_last_error().decode()
    assert _optim(lib, plan, flags=4) == WUN_ERR_INVALID
    assert _optim(lib, plan, flags=8 | 1) == WUN_ERR_INVALID
    assert "flags" in lib.wun_last_error().decode()
    assert _optim(lib, plan, skipped=None) == WUN_ERR_INVALID             # skipping asks for the counter
    assert "skipped" in lib.wun_last_error().decode()
    assert _optim(lib, plan, ws=None) == WUN_ERR_INVALID                  # clipping asks for the norm workspace
    assert _optim(lib, plan, ws=_FAKE_MISALIGNED) == WUN_ERR_INVALID
    assert _optim(lib, plan, ws=None, clip_norm=math.inf, flags=1) == WUN_ERR_INVALID       # ... and so does skipping
    assert _optim(lib, plan, nsel=3) == WUN_ERR_INVALID
    assert _optim(lib, plan, sel=[1] * nt, nsel=nt + 1) == WUN_ERR_INVALID
    assert _optim(lib, plan, sel=[0] * (nt - 1)) == WUN_ERR_INVALID
    assert _optim(lib, plan, ndec=3) == WUN_ERR_INVALID                   # a bad ndecay
    assert _optim(lib, plan, dec=[1] * nt, ndec=nt - 1) == WUN_ERR_INVALID
    assert _optim(lib, plan, dec=[1] * (nt + 1)) == WUN_ERR_INVALID
    assert "nselect" in lib.wun_last_error().decode()


def test_ema_update_argument_errors(lib, plan):
    nt = len(plan.tensors)

    def call(handle=True, ema=_FAKE, params=_FAKE, decay=0.999, step=1, flags=0, sel=None, nsel=None):
        sm, sp = _mask(sel) if sel is not None else (None, None)
        nsel = (len(sm) if sm is not None else 0) if nsel is None else nsel
        return lib.wun_ema_update(plan.handle if handle else None, ema, params, decay, step, flags, None, sp, nsel)
    assert call(handle=False) == WUN_ERR_INVALID
    assert call(ema=None) == WUN_ERR_INVALID
    assert call(params=None) == WUN_ERR_INVALID
    for d in (1.0, 2.0, -0.5, math.nan):
        assert call(decay=d) == WUN_ERR_INVALID, d
    assert call(step=-1) == WUN_ERR_INVALID
    assert call(flags=1) == WUN_ERR_INVALID                                # WUN_CLIP_SKIP_NONFINITE is not a flag of this entry
    assert call(flags=4) == WUN_ERR_INVALID
    assert call(nsel=2) == WUN_ERR_INVALID
    assert call(sel=[1] * (nt + 1)) == WUN_ERR_INVALID
    # nothing selected: no launch, no error, and the fake pointers are never dereferenced
    assert call(sel=[0] * nt) == 0
    assert _optim(lib, plan, sel=[0] * nt, clip_norm=math.inf, flags=0, ws=None, skipped=None) == 0
