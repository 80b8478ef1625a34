"""GPU tests of global gradient-norm clipping and non-finite step skipping (include/wun.h: wun_grad_norm, wun_adam_step_clip;
DESIGN.md 5.7), of UnetAudioSeparator.grad_norm / adam_step(clip_norm=, skip_nonfinite=) and of Trainer(clip_grad_norm=).

The float64 reference lives here: per-tensor sums of squares, tf.clip_by_global_norm (scale clip * min(1/N, 1/clip)) and the
TF-Adam rule (Training.py:77), all in torch float64.  Norms must lie within 2 fp32 ulp of it and be bitwise reproducible; an
inactive clip must leave params, m and v bit-equal to wun_adam_step / wun_adam_step_select; an active clip must match the
reference within the Adam bounds of test_gpu_parity.py (2e-6 / 4e-6)."""
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_backward import _setup, _setup_bf16
from test_gpu_backward_select import SENTINEL, _bits, _ranges

import wave_u_net_amd as wun
from wave_u_net_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
DP_TOL = 2e-5                          # x max(1, max|p|): the tolerance of test_data_parallel_gpu.py
ADAM_TOL = 2e-6                        # one TF-Adam update vs float64 (test_gpu_parity.py)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


# ------------------------------------------------------------------------------------------------ float64 reference
def _sizes(sep):
    return [(off, int(np.prod(shp))) for _, off, shp in sep._active.tensors]


def _sums64(sep, g):
    """Per-tensor float64 sums of squares of the arena g (tensor floats only)."""
    g64 = g.double()
    return torch.stack([(g64[o:o + n] ** 2).sum() for o, n in _sizes(sep)]).cpu()


def _ulp(x):
    return np.spacing(np.abs(np.float32(x)))


def _within_ulps(got, ref, ulps, tag):
    got = np.asarray(got, dtype=np.float32).reshape(-1)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    err = np.abs(got.astype(np.float64) - ref)
    lim = ulps * _ulp(ref).astype(np.float64)
    bad = np.nonzero(err > lim)[0]
    assert bad.size == 0, (tag, bad[:5], got[bad[:5]], ref[bad[:5]])


def _tf_adam64(p, g, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8):
    lr_t = lr * math.sqrt(1 - b2 ** step) / (1 - b1 ** step)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    return p - lr_t * m / (torch.sqrt(v) + eps), m, v


def _clip64(g64, sel, clip):
    """tf.clip_by_global_norm over the selected floats: (clipped gradient, global norm)."""
    n = torch.sqrt((g64[sel] ** 2).sum())
    return g64 * (clip * torch.minimum(1.0 / n, torch.tensor(1.0 / clip, dtype=torch.float64))), float(n)


def _random_arena(sep, seed=3):
    """Tensor k of the arena ~ N(0, 1) * 10^(-8 + 11 k / (nt - 1)): magnitudes 1e-8 ... 1e3; NaN sentinel in the padding."""
    n = int(sep._active.info.arena_floats)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.zeros(n, dtype=torch.float32)
    sz = _sizes(sep)
    for k, (o, c) in enumerate(sz):
        a[o:o + c] = torch.randn(c, generator=gen) * 10.0 ** (-8 + 11 * k / max(1, len(sz) - 1))
    a = a.cuda()
    pad = ~_ranges(sep, np.ones(len(sz), dtype=np.uint8))
    a.view(torch.int32)[pad] = SENTINEL
    return a, pad


def _every_other(sep):
    return [n for k, (n, _, _) in enumerate(sep._active.tensors) if k % 2 == 0]


# ------------------------------------------------------------------------------------------------ 1. norms
def _deep_sep():
    from wave_u_net_amd.separator import UnetAudioSeparator
    sep = UnetAudioSeparator(wun.get_config("deep_l16_f48"), device="cuda:0")
    sep._active = sep._any_plan()
    sep._ensure_variables(sep._active)
    return sep


def _norm_plan(kind):
    if kind == "fp32_small":
        return _setup("full_multi_small")[0]
    if kind == "bf16":
        sep = _setup_bf16("m5_shaped")[0]
        assert sep.effective_dtype == "bf16"
        return sep
    return _deep_sep()


@pytest.mark.parametrize("kind", ["fp32_small", "bf16", "deep_l16_f48"])
def test_grad_norm(lib, kind):
    sep = _norm_plan(kind)
    nt = len(sep._active.tensors)
    a, pad = _random_arena(sep)
    sep.grads.copy_(a)
    if kind == "deep_l16_f48":
        assert max(n for _, n in _sizes(sep)) > 1000 * 8192           # one tensor spans over a thousand chunks
    sums = _sums64(sep, sep.grads)
    glob, per = sep.grad_norm()
    torch.cuda.synchronize()
    _within_ulps(per.cpu().numpy(), torch.sqrt(sums).numpy(), 2, kind + "/per-tensor")
    _within_ulps(glob.cpu().numpy(), math.sqrt(float(sums.sum())), 2, kind + "/global")
    assert per.shape == (nt,) and glob.dim() == 0
    # bitwise reproducible
    for _ in range(2):
        g2, p2 = sep.grad_norm()
        assert torch.equal(_bits(g2), _bits(glob)) and torch.equal(_bits(p2), _bits(per))
    # a selection: selected entries bit-equal to the full call's, 0 elsewhere, global over the selection only
    names = _every_other(sep)
    mask = sep.select_mask(names).astype(bool)
    gs, ps = sep.grad_norm(variables=names)
    torch.cuda.synchronize()
    assert torch.equal(_bits(ps[mask]), _bits(per[mask]))
    assert (ps[~mask] == 0).all()
    _within_ulps(gs.cpu().numpy(), math.sqrt(float(sums[mask].sum())), 2, kind + "/selected global")
    # a NaN in an unselected tensor is never read
    off, n = _sizes(sep)[int(np.nonzero(~mask)[0][0])]
    sep.grads[off + n // 2] = float("nan")
    gs2, ps2 = sep.grad_norm(variables=names)
    assert torch.equal(_bits(gs2), _bits(gs)) and torch.equal(_bits(ps2), _bits(ps))
    gn, _ = sep.grad_norm()
    assert math.isnan(gn.item())
    sep.grads.copy_(a)
    # grad_scale: |s| * norm
    gsc, psc = sep.grad_norm(grad_scale=-0.25)
    torch.cuda.synchronize()
    _within_ulps(psc.cpu().numpy(), 0.25 * torch.sqrt(sums).numpy(), 2, kind + "/scaled per-tensor")
    _within_ulps(gsc.cpu().numpy(), 0.25 * math.sqrt(float(sums.sum())), 2, kind + "/scaled global")
    assert (_bits(sep.grads)[pad] == SENTINEL).all()                  # the norm writes nothing into the arena


# ------------------------------------------------------------------------------------------------ 2. - 4. clipped Adam
def _trained(name="full_small"):
    """A separator after 3 real steps (m, v non-zero) and a fresh gradient in sep.grads."""
    sep, ocfg, params, mix, tg = _setup(name)
    for _ in range(3):
        sep.get_output(mix, True)
        sep.loss_and_gradients(tg)
        sep.adam_step(1e-3)
    sep.get_output(mix, True)
    sep.loss_and_gradients(tg)
    torch.cuda.synchronize()
    return sep


def _state(sep):
    return [t.clone() for t in (sep.params, sep.adam_m, sep.adam_v)], sep.global_step


def _restore(sep, st):
    for t, s in zip((sep.params, sep.adam_m, sep.adam_v), st[0]):
        t.copy_(s)
    sep.global_step = st[1]


def _assert_bits_equal(xs, ys, tag):
    for x, y, what in zip(xs, ys, ("params", "m", "v")):
        assert torch.equal(_bits(x), _bits(y)), (tag, what)


@pytest.mark.parametrize("variables", [None, "every_other"])
def test_inactive_clip_is_bit_exact(lib, variables):
    sep = _trained()
    names = _every_other(sep) if variables else None
    st = _state(sep)
    sep.adam_step(1e-3, variables=names)                              # wun_adam_step / wun_adam_step_select
    ref = [t.clone() for t in (sep.params, sep.adam_m, sep.adam_v)]
    norm, _ = sep.grad_norm(variables=names)
    for clip in (float(norm.item()), 2.0 * float(norm.item()), math.inf):
        for skip in (False, True):
            _restore(sep, st)
            n = sep.adam_step(1e-3, variables=names, clip_norm=clip, skip_nonfinite=skip)
            torch.cuda.synchronize()
            assert torch.equal(_bits(n), _bits(norm)), clip
            _assert_bits_equal((sep.params, sep.adam_m, sep.adam_v), ref, (clip, skip))
            assert sep.global_step == st[1] + 1
    _restore(sep, st)
    sep.adam_step(1e-3, variables=names, skip_nonfinite=True)          # skip only: no clipping
    _assert_bits_equal((sep.params, sep.adam_m, sep.adam_v), ref, "skip only")
    if names is not None:
        sel = _ranges(sep, sep.select_mask(names))
        for t, s in zip((sep.params, sep.adam_m, sep.adam_v), st[0]):
            assert torch.equal(_bits(t[~sel]), _bits(s[~sel]))
    assert sep.skipped_steps == 0


@pytest.mark.parametrize("variables", [None, "every_other"])
def test_active_clip_matches_tf(lib, variables):
    sep = _trained("full_multi_small")
    names = _every_other(sep) if variables else None
    sel = _ranges(sep, sep.select_mask(names) if names else np.ones(len(sep._active.tensors), dtype=np.uint8))
    st = _state(sep)
    norm, _ = sep.grad_norm(variables=names)
    clip = 0.1 * float(norm.item())
    g64 = sep.grads.double().cpu()
    gc, n64 = _clip64(g64, torch.from_numpy(sel.cpu().numpy()), clip)
    p, m, v = (t.double().cpu() for t in st[0])
    pe, me, ve = _tf_adam64(p, gc, m, v, st[1] + 1, 1e-3)
    got_n = sep.adam_step(1e-3, variables=names, clip_norm=clip)
    torch.cuda.synchronize()
    _within_ulps(got_n.cpu().numpy(), n64, 2, "global norm")
    s = sel.cpu()
    pg, mg, vg = (t.double().cpu() for t in (sep.params, sep.adam_m, sep.adam_v))
    assert (pg[s] - pe[s]).abs().max().item() <= ADAM_TOL
    assert (mg[s] - me[s]).abs().max().item() <= 1e-6 * max(1e-30, me[s].abs().max().item())
    assert (vg[s] - ve[s]).abs().max().item() <= 1e-5 * max(1e-30, ve[s].abs().max().item())
    # the update did clip: it differs from the unclipped one
    assert not torch.equal(_bits(sep.params[sel]), _bits(st[0][0][sel]))
    for t, o in zip((sep.params, sep.adam_m, sep.adam_v), st[0]):
        assert torch.equal(_bits(t[~sel]), _bits(o[~sel]))


@pytest.mark.parametrize("variables", [None, "every_other"])
def test_skip_nonfinite(lib, variables):
    sep = _trained()
    names = _every_other(sep) if variables else None
    mask = sep.select_mask(names) if names else np.ones(len(sep._active.tensors), dtype=np.uint8)
    g0 = sep.grads.clone()
    st = _state(sep)
    k_sel = int(np.nonzero(mask)[0][-1])
    off, n = _sizes(sep)[k_sel]
    for count, bad in ((1, float("inf")), (2, float("nan"))):
        sep.grads.copy_(g0)
        sep.grads[off + n // 3] = bad
        r = sep.adam_step(1e-3, variables=names, clip_norm=1.0, skip_nonfinite=True)
        torch.cuda.synchronize()
        assert not math.isfinite(r.item())
        _assert_bits_equal((sep.params, sep.adam_m, sep.adam_v), st[0], bad)
        assert sep.skipped_steps == count
        assert sep.global_step == st[1] + count                       # TF's global_step still counts the sess.run
    if names is not None:
        # a non-finite float in an UNSELECTED tensor is not seen: the step applies
        k_un = int(np.nonzero(mask == 0)[0][0])
        o2, n2 = _sizes(sep)[k_un]
        sep.grads.copy_(g0)
        sep.grads[o2] = float("inf")
        sep.global_step = st[1]
        r = sep.adam_step(1e-3, variables=names, clip_norm=math.inf, skip_nonfinite=True)
        assert math.isfinite(r.item()) and sep.skipped_steps == 2
        ref_run = [t.clone() for t in (sep.params, sep.adam_m, sep.adam_v)]
        _restore(sep, st)
        sep.adam_step(1e-3, variables=names)
        _assert_bits_equal((sep.params, sep.adam_m, sep.adam_v), ref_run, "inf in an unselected tensor")
    # the next finite call applies normally, with lr_t of the caller's step
    sep.grads.copy_(g0)
    _restore(sep, st)
    sep.adam_step(1e-3, variables=names)
    ref = [t.clone() for t in (sep.params, sep.adam_m, sep.adam_v)]
    _restore(sep, st)
    sep.adam_step(1e-3, variables=names, clip_norm=math.inf, skip_nonfinite=True)
    torch.cuda.synchronize()
    _assert_bits_equal((sep.params, sep.adam_m, sep.adam_v), ref, "finite after skips")
    assert sep.skipped_steps == 2


def test_skip_counter_raw_abi(lib):
    """wun_adam_step_clip directly: the caller's int64 counter, no clipping flag = a NaN update is applied as TF would."""
    sep = _trained()
    st = _state(sep)
    ws = torch.empty(int(lib.wun_grad_norm_workspace_floats(sep._active.handle)), device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    sep.grads[0] = float("nan")

    def call(flags, skipped):
        _lib.check(lib.wun_adam_step_clip(sep._active.handle, sep.params.data_ptr(), sep.grads.data_ptr(),
                                          sep.adam_m.data_ptr(), sep.adam_v.data_ptr(), st[1] + 1, 1e-3, 0.9, 0.999, 1e-8,
                                          1.0, 1.0, flags, ws.data_ptr(), skipped, sep._stream(), None, 0))
    call(1, cnt.data_ptr())
    call(1, cnt.data_ptr())
    torch.cuda.synchronize()
    assert cnt.item() == 2
    _assert_bits_equal((sep.params, sep.adam_m, sep.adam_v), st[0], "skipped")
    call(0, None)
    torch.cuda.synchronize()
    assert torch.isnan(sep.params[0]).item() and cnt.item() == 2


# ------------------------------------------------------------------------------------------------ 5. Trainer
def _dp_cfg():
    import dp_worker
    return dp_worker.make_cfg()


def _batch(cfg, n):
    import dp_worker
    from wave_u_net_amd.training import Trainer
    probe = Trainer(dict(cfg, batch_size=n))
    mix, targets = dp_worker.global_batch(cfg, probe.t_in, probe.t_out, n)
    return mix.cuda(), targets.cuda()


def _run(cfg, steps, mix, targets, **kw):
    from wave_u_net_amd.training import Trainer
    tr = Trainer(cfg, **kw)
    for _ in range(steps):
        tr.step(mix, targets)
    torch.cuda.synchronize()
    return tr


def test_trainer_inactive_clip_bit_equal(lib):
    cfg = dict(_dp_cfg(), batch_size=12)
    mix, targets = _batch(cfg, 12)
    a = _run(cfg, 3, mix, targets)
    b = _run(cfg, 3, mix, targets, clip_grad_norm=1e30)
    c = _run(dict(cfg, clip_grad_norm=1e30, skip_nonfinite_steps=True), 3, mix, targets)
    assert a.grad_norm is None and a.clip_norm is None
    assert b.clip_norm == 1e30 and not b.skip_nonfinite and c.skip_nonfinite
    for t in (b, c):
        _assert_bits_equal((t.sep.params, t.sep.adam_m, t.sep.adam_v), (a.sep.params, a.sep.adam_m, a.sep.adam_v), "trainer")
        assert math.isfinite(t.grad_norm.item()) and t.sep.skipped_steps == 0


def test_trainer_active_clip_equals_hand_sequence(lib):
    """Trainer(clip_grad_norm) against get_output / loss_and_gradients and a float64 clip + TF-Adam, 3 steps."""
    from wave_u_net_amd.separator import UnetAudioSeparator
    cfg = dict(_dp_cfg(), batch_size=12)
    mix, targets = _batch(cfg, 12)
    probe = _run(cfg, 1, mix, targets, clip_grad_norm=1e30)
    clip = 0.05 * float(probe.grad_norm.item())
    tr = _run(cfg, 3, mix, targets, clip_grad_norm=clip)
    sep = UnetAudioSeparator(tr.cfg, device="cuda:0", seed=1337)
    p = m = v = None
    for step in range(1, 4):
        sep.get_output(mix, True)
        sep.loss_and_gradients(targets)
        torch.cuda.synchronize()
        if p is None:
            p = sep.params.double().cpu()
            m, v = torch.zeros_like(p), torch.zeros_like(p)
        g64 = sep.grads.double().cpu()
        gc, n = _clip64(g64, torch.ones_like(g64, dtype=torch.bool), clip)
        assert n > clip                                              # the clip is active at every step
        p, m, v = _tf_adam64(p, gc, m, v, step, cfg["init_sup_sep_lr"])
        sep.params.copy_(p.float())
    err = (tr.sep.params.double().cpu() - p).abs().max().item()
    assert err <= 2 * ADAM_TOL * max(1.0, p.abs().max().item()), err


def test_trainer_accumulation_norm_is_of_the_mean_gradient(lib):
    cfg = dict(_dp_cfg(), batch_size=12)
    mix, targets = _batch(cfg, 12)
    tr = _run(cfg, 1, mix, targets, grad_accum_steps=2, clip_grad_norm=1e-3)
    # sep.grads holds the SUM of the two micro-batch gradients (Adam does not touch it); the norm is of that sum / 2
    sums = _sums64(tr.sep, tr.sep.grads)
    _within_ulps(tr.grad_norm.cpu().numpy(), 0.5 * math.sqrt(float(sums.sum())), 2, "k = 2")
    g, _ = tr.sep.grad_norm(grad_scale=0.5)
    assert torch.equal(_bits(g), _bits(tr.grad_norm))


def test_trainer_clip_benchmarked_plan_pinned_table(lib):
    """configs[1], M1 with context, B = 16, the pinned tuning table imported (as bench.py does): inactive clip bit-equal to the
    default step, active clip vs float64, the norm over the 10.26M-float arena within 2 ulp."""
    from wave_u_net_amd.training import Trainer, synthetic_source
    cfg = wun.get_config("m1_context")
    tr = Trainer(cfg, batch_size=16, clip_grad_norm=1e30)
    mix, targets = synthetic_source(cfg, 16, tr.t_in, tr.t_out, tr.device, seed=1337)()
    tr.tune(mix, targets, pinned_table=open(os.path.join(ROOT, "profiles", "round6_tune_table.txt")).read())
    assert tr.tune_source == "pinned"
    tr.step(mix, targets)                                             # m, v non-zero
    st = _state(tr.sep)
    tr.step(mix, targets)
    torch.cuda.synchronize()
    clipped_inactive = [t.clone() for t in (tr.sep.params, tr.sep.adam_m, tr.sep.adam_v)]
    sums = _sums64(tr.sep, tr.sep.grads)
    _within_ulps(tr.grad_norm.cpu().numpy(), math.sqrt(float(sums.sum())), 2, "B16 global")
    norm = float(tr.grad_norm.item())
    _restore(tr.sep, st)
    tr.clip_norm = None
    tr.step(mix, targets)                                             # the default step: wun_adam_step
    torch.cuda.synchronize()
    _assert_bits_equal((tr.sep.params, tr.sep.adam_m, tr.sep.adam_v), clipped_inactive, "B16 inactive")
    # active: the same gradient (same params), clipped to 0.1 x its norm
    g64 = tr.sep.grads.double().cpu()
    gc, _ = _clip64(g64, torch.ones_like(g64, dtype=torch.bool), 0.1 * norm)
    pe, _, _ = _tf_adam64(*(t.double().cpu() for t in (st[0][0], gc, st[0][1], st[0][2])), st[1] + 1, cfg["init_sup_sep_lr"])
    _restore(tr.sep, st)
    tr.sep.adam_step(tr.lr, clip_norm=0.1 * norm)
    torch.cuda.synchronize()
    assert (tr.sep.params.double().cpu() - pe).abs().max().item() <= ADAM_TOL


def test_train_logs_grad_norm_only_when_enabled(lib, tmp_path, monkeypatch):
    from wave_u_net_amd import training
    monkeypatch.setenv("WUN_NO_TUNE", "1")
    tmp = str(tmp_path)
    cfg = wun.get_config("full", num_layers=3, num_initial_filters=8, num_frames=40, batch_size=4, epoch_it=2,
                         model_base_dir=os.path.join(tmp, "ckpt"), log_dir=os.path.join(tmp, "logs"), init_sup_sep_lr=1e-3)
    training.train(cfg, "plain")
    training.train(dict(cfg, clip_grad_norm=1e-2, skip_nonfinite_steps=True), "clipped")
    plain = [json.loads(l) for l in open(os.path.join(tmp, "logs", "plain", "train.jsonl"))]
    clipped = [json.loads(l) for l in open(os.path.join(tmp, "logs", "clipped", "train.jsonl"))]
    assert len(plain) == len(clipped) == 2
    assert all("grad_norm" not in r and "skipped_steps" not in r for r in plain)
    assert all(math.isfinite(r["grad_norm"]) and r["grad_norm"] > 0 and r["skipped_steps"] == 0 for r in clipped)


# ------------------------------------------------------------------------------------------------ 6. data parallel
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_two_ranks_clipping_equal_one_process(tmp_path):
    """Two ranks on the one GPU (gloo), per-rank batch 6, clip active: replicas bit-identical, and equal to one process on the
    global batch of 12 within DP_TOL."""
    import dp_worker
    from wave_u_net_amd import training
    steps, clip = 3, 1e-3
    out = os.path.join(str(tmp_path), "dp_clip")
    env = dict(os.environ, WUN_DIST_BACKEND="gloo", WUN_NO_TUNE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "dp_clip_worker.py"), out, str(steps), repr(clip)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r0, r1 = np.load(out + ".rank0.npz"), np.load(out + ".rank1.npz")
    assert int(r0["world"]) == 2
    for k in ("params", "m", "v", "norms"):
        assert np.array_equal(r0[k].view(np.int32), r1[k].view(np.int32)), k
    assert np.all(r0["norms"] > clip)                                # active at every step
    cfg = dict(dp_worker.make_cfg(), batch_size=12)
    tr = training.Trainer(cfg, clip_grad_norm=clip)
    mix, targets = dp_worker.global_batch(cfg, tr.t_in, tr.t_out, 12)
    mix, targets = mix.to(tr.device), targets.to(tr.device)
    for _ in range(steps):
        tr.step(mix, targets)
    torch.cuda.synchronize()
    ref = tr.sep.params.cpu().numpy()
    assert np.abs(r0["params"] - ref).max() <= DP_TOL * max(1.0, np.abs(ref).max())
