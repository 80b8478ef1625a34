"""GPU tests of gradient accumulation (include/wun.h: wun_backward_accumulate, wun_loss_backward_accumulate) and of
Trainer(grad_accum_steps = k).

The contract is bitwise: on one forward pass, G = what the overwriting _select call writes; with `grads` pre-filled with random
finite values A (and a NaN sentinel in the padding floats), the accumulating call must leave A + G (torch float32 add) in every
selected float, A in every other float, and write d_mix / loss bit-equal to the overwriting call's.  Plans: same padding and
context in fp32, the bf16 cases, the benchmarked configs[1] B = 16 plan with its pinned table, and small plans under the
kernel-selection switches so that every writer of final gradient floats runs in its accumulating form."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_backward import BF16_CASES, _setup, _setup_bf16
from test_gpu_backward_select import SENTINEL, _Ctx, _bits, _mask_arg, _pattern, _ranges

import wave_u_net_amd as wun
from wave_u_net_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
DP_TOL = 2e-5                          # x max(1, max|p|): the tolerance of test_data_parallel_gpu.py


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def _start(sep, seed=7):
    """A: random finite floats in every tensor float, the NaN sentinel in the padding floats."""
    n = int(sep._active.info.arena_floats)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    a = (torch.randn(n, generator=gen) * 0.01).cuda()
    pad = ~_ranges(sep, np.ones(len(sep._active.tensors), dtype=np.uint8))
    a.view(torch.int32)[pad] = SENTINEL
    return a, pad


def _acc_backward(ctx, grads, mask, want_mix, buckets=None):
    sep = ctx.sep
    dm = torch.full(ctx.mix_shape, float("nan"), device="cuda") if want_mix else None
    starts, events, nb = buckets if buckets else (None, None, 0)
    sel, nsel = _mask_arg(mask) if mask is not None else (None, 0)
    _lib.check(ctx.lib.wun_backward_accumulate(sep._active.handle, sep.params.data_ptr(), None, ctx.ws.data_ptr(),
                                               ctx.outs.data_ptr(), ctx.dout.data_ptr(),
                                               grads.data_ptr() if (mask is None or mask.any()) else None,
                                               dm.data_ptr() if dm is not None else None, sep._stream(),
                                               starts, events, nb, sel, nsel))
    return dm


def _acc_loss(ctx, grads, mask):
    sep = ctx.sep
    loss = torch.full((), float("nan"), device="cuda")
    sel, nsel = _mask_arg(mask) if mask is not None else (None, 0)
    _lib.check(ctx.lib.wun_loss_backward_accumulate(sep._active.handle, sep.params.data_ptr(), None, ctx.ws.data_ptr(),
                                                    ctx.outs.data_ptr(), ctx.tg.data_ptr(), grads.data_ptr(), loss.data_ptr(),
                                                    sep._stream(), None, None, 0, sel, nsel))
    return loss


def _expect(a, g, sel):
    """A + G at the selected floats (torch float32 add), A elsewhere."""
    e = a.clone()
    e[sel] = a[sel] + g[sel]
    return e


def _check(got, exp, tag):
    bad = int((_bits(got) != _bits(exp)).sum().item())
    assert bad == 0, (tag, "floats that differ from A + G / A", bad)


def _run_contract(ctx, tag, patterns=(None,)):
    """Both entry points, with and without d_mix, for each selection (None = every tensor); determinism of the accumulating
    call on the same inputs."""
    sep = ctx.sep
    a, pad = _start(sep)
    for name in patterns:
        mask = None if name is None else _pattern(sep, name)
        sel = ~pad if mask is None else _ranges(sep, mask)
        t = "%s/%s" % (tag, name or "all")
        if mask is not None and not mask.any():
            continue
        # G of the overwriting calls: the _Ctx references (full calls) restricted to the selection -- the _select calls write
        # the selected floats bit-equal to them (test_gpu_backward_select.py)
        g = a.clone()
        _acc_backward(ctx, g, mask, False)
        torch.cuda.synchronize()
        _check(g, _expect(a, ctx.g_full, sel), t + "/backward")
        g2 = a.clone()
        _acc_backward(ctx, g2, mask, False)
        torch.cuda.synchronize()
        assert torch.equal(_bits(g2), _bits(g)), (t, "not deterministic")
        g = a.clone()
        dm = _acc_backward(ctx, g, mask, True)
        torch.cuda.synchronize()
        _check(g, _expect(a, ctx.g_full_m, sel), t + "/backward+d_mix")
        assert torch.equal(_bits(dm), _bits(ctx.dmix_full)), (t, "d_mix")
        g = a.clone()
        loss = _acc_loss(ctx, g, mask)
        torch.cuda.synchronize()
        _check(g, _expect(a, ctx.g_loss, sel), t + "/loss_backward")
        assert _bits(loss).item() == _bits(ctx.loss).item(), (t, loss.item(), ctx.loss.item())
        assert (_bits(g)[pad] == SENTINEL).all(), (t, "padding written")


# ------------------------------------------------------------------------------------------------ 1. bitwise contract
@pytest.mark.parametrize("name", ["learned_same_small", "full_small", "full_multi_small"])
def test_accumulate_contract_fp32(lib, name):
    sep, ocfg, params, mix, tg = _setup(name)
    _run_contract(_Ctx(lib, sep, mix, tg), "f32_" + name)


@pytest.mark.parametrize("key", sorted(BF16_CASES))
def test_accumulate_contract_bf16(lib, key):
    sep, ocfg, params, mix, tg = _setup_bf16(key)
    assert sep.effective_dtype == "bf16"
    _run_contract(_Ctx(lib, sep, mix, tg), "bf16_" + key)


def test_accumulate_contract_benchmarked_plan_pinned_table(lib):
    """configs[1], M1 with context, B = 16, the pinned tuning table imported (as bench.py does)."""
    from wave_u_net_amd.training import Trainer, synthetic_source
    cfg = wun.get_config("m1_context")
    tr = Trainer(cfg, batch_size=16)
    mix, targets = synthetic_source(cfg, 16, tr.t_in, tr.t_out, tr.device, seed=1337)()
    tr.tune(mix, targets, pinned_table=open(os.path.join(ROOT, "profiles", "round6_tune_table.txt")).read())
    assert tr.tune_source == "pinned"
    ctx = _Ctx(lib, tr.sep, mix, targets.to(torch.float32))
    _run_contract(ctx, "bench_B16_pinned", patterns=(None, "decoder"))
    _record_kernels(lib, ctx, "bench_B16_pinned")


# --------------------------------------------------------------------------------------------- 2. every writer kernel
# Which accumulating kernels each call launches is read from the library's profile brackets (wun_profile_begin / _end); the
# union over the cases below must hold every family's forms (the coverage test names them when it fails).
_SEEN = {}


def _record_kernels(lib, ctx, tag):
    a, _ = _start(ctx.sep)
    _lib.check(lib.wun_profile_begin())
    _acc_backward(ctx, a, None, False)
    buf = C.create_string_buffer(1 << 22)
    _lib.check(lib.wun_profile_end(buf, len(buf)))
    names = sorted({k["name"] for k in json.loads(buf.value.decode())["kernels"]})
    _SEEN[tag] = [n for n in names if "acc_kernel" in n or "interp_grad" in n]


WRITER_CASES = [   # (id, golden case, environment switches read at plan creation, B)
    ("no_win_context", "full_small", {"WUN_NO_WIN": "1"}, 3),
    ("no_narrow_context", "full_multi_small", {"WUN_NO_NARROW": "1"}, 3),
    ("no_fuse_ups_learned_same", "learned_same_small", {"WUN_NO_FUSE_UPS": "1"}, 3),
    ("learned_same_b8", "learned_same_small", {}, 8),
    ("no_win_same_b8", "learned_same_small", {"WUN_NO_WIN": "1"}, 8),
    # one excerpt of <= 128 positions per layer: one work unit per weight gradient, so every launch is single-split (direct)
    ("learned_same_b1", "learned_same_small", {}, 1),
    ("no_win_same_b1", "learned_same_small", {"WUN_NO_WIN": "1"}, 1),
]


@pytest.mark.parametrize("case", WRITER_CASES, ids=[c[0] for c in WRITER_CASES])
def test_accumulate_every_writer_kernel(lib, case):
    tag, name, env, B = case
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        sep, ocfg, params, mix, tg = _setup(name, B=B)          # (the plan reads the switches here, once)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    ctx = _Ctx(lib, sep, mix, tg)
    _run_contract(ctx, tag, patterns=(None, "every_other"))
    _record_kernels(lib, ctx, tag)


def test_accumulate_writer_kernel_coverage():
    """Runs after the cases above (file order): the direct and the reduce form of both exact-fp32 weight-gradient families
    ran in their accumulating form somewhere."""
    seen = {n.split("<")[0] for names in _SEEN.values() for n in names}
    if not _SEEN:
        pytest.skip("run with the writer-kernel cases")
    for k in ("wgrad_mfma_acc_kernel", "wgrad_reduce_acc_kernel", "wgrad_win_acc_kernel", "wgrad_win_reduce_acc_kernel"):
        assert k in seen, (k, _SEEN)


# --------------------------------------------------------------------------------------------- 3. select x accumulate
@pytest.mark.parametrize("name", ["full_small", "learned_same_small"])
def test_accumulate_with_selection(lib, name):
    sep, ocfg, params, mix, tg = _setup(name)
    _run_contract(_Ctx(lib, sep, mix, tg), "select_" + name, patterns=("head", "decoder", "every_other", "down0"))


# ------------------------------------------------------------------------------------------------- 4. bucket events
@pytest.mark.parametrize("name", ["full_small", "learned_same_small"])
def test_accumulate_bucket_events(lib, name):
    sep, ocfg, params, mix, tg = _setup(name)
    ctx = _Ctx(lib, sep, mix, tg)
    n = int(sep._active.info.arena_floats)
    offs = sorted({off for _, off, _ in sep._active.tensors})
    starts = sorted(offs[::3], reverse=True)
    assert starts[-1] == 0
    ends = [n] + starts[:-1]
    comm = torch.cuda.Stream()
    a, pad = _start(sep)
    for pattern in (None, "decoder", "every_other", "down0"):
        mask = None if pattern is None else _pattern(sep, pattern)
        sel = ~pad if mask is None else _ranges(sep, mask)
        events = []
        for _ in starts:
            ev = torch.cuda.Event(enable_timing=False)
            ev.record(torch.cuda.current_stream())
            events.append(ev)
        st = (C.c_int64 * len(starts))(*starts)
        evs = (C.c_void_p * len(starts))(*[int(e.cuda_event) for e in events])
        copy = torch.zeros(n, device="cuda")
        g = a.clone()
        _acc_backward(ctx, g, mask, False, buckets=(st, evs, len(starts)))
        for s, e, ev in zip(starts, ends, events):
            comm.wait_event(ev)
            with torch.cuda.stream(comm):
                copy[s:e].copy_(g[s:e])
        torch.cuda.synchronize()
        assert torch.equal(_bits(copy), _bits(g)), (name, pattern)
        _check(g, _expect(a, ctx.g_full, sel), "%s/buckets/%s" % (name, pattern))


# ---------------------------------------------------------------------------------------------------------- 5. Trainer
def _trainer_run(cfg, k, batch, steps, mix, targets):
    from wave_u_net_amd.training import Trainer
    tr = Trainer(dict(cfg, batch_size=batch), grad_accum_steps=k)
    losses = [tr.step(mix, targets) for _ in range(steps)]
    torch.cuda.synchronize()
    return tr, [float(x.item()) for x in losses]


def test_trainer_accumulation_matches_one_batch_fp32():
    import dp_worker
    cfg = dp_worker.make_cfg()
    from wave_u_net_amd.training import Trainer
    probe = Trainer(dict(cfg, batch_size=12))
    mix, targets = dp_worker.global_batch(cfg, probe.t_in, probe.t_out, 12)
    mix, targets = mix.to(probe.device), targets.to(probe.device)
    ref, ref_losses = _trainer_run(cfg, 1, 12, 3, mix, targets)
    p1 = ref.sep.params.cpu().numpy()
    for k in (2, 4):
        tr, losses = _trainer_run(cfg, k, 12, 3, mix, targets)
        assert tr.micro == 12 // k and tr.sep._active.info.batch == 12 // k
        pk = tr.sep.params.cpu().numpy()
        err = np.abs(pk - p1).max()
        assert err <= DP_TOL * max(1.0, np.abs(p1).max()), (k, err)
        assert np.allclose(losses, ref_losses, rtol=1e-4, atol=0), (k, losses, ref_losses)
    with pytest.raises(ValueError):
        Trainer(dict(cfg, batch_size=12), grad_accum_steps=5)
    with pytest.raises(ValueError):
        Trainer(dict(cfg, batch_size=12, grad_accum_steps=0))


def _by_hand(cfg, k, batch, steps, mix, targets):
    """The calls Trainer(grad_accum_steps = k).step makes, through the separator (one process: no all-reduce)."""
    from wave_u_net_amd.separator import UnetAudioSeparator
    sep = UnetAudioSeparator(cfg, device="cuda:0", seed=1337)
    b = batch // k
    for _ in range(steps):
        for i in range(k):
            sep.get_output(mix[i * b:(i + 1) * b], True)
            sep.loss_and_gradients(targets[:, i * b:(i + 1) * b], accumulate=i > 0)
        sep.adam_step(cfg["init_sup_sep_lr"], grad_scale=1.0 / k)
    torch.cuda.synchronize()
    return sep


def _hand_equal(cfg, batch, mix, targets):
    tr, _ = _trainer_run(cfg, 2, batch, 3, mix, targets)
    sep = _by_hand(tr.cfg, 2, batch, 3, mix, targets)
    assert torch.equal(_bits(tr.sep.params), _bits(sep.params))
    assert torch.equal(_bits(tr.sep.adam_m), _bits(sep.adam_m)) and torch.equal(_bits(tr.sep.adam_v), _bits(sep.adam_v))


def test_trainer_accumulation_equals_hand_sequence_fp32():
    import dp_worker
    from wave_u_net_amd.training import Trainer
    cfg = dp_worker.make_cfg()
    probe = Trainer(dict(cfg, batch_size=12))
    mix, targets = dp_worker.global_batch(cfg, probe.t_in, probe.t_out, 12)
    _hand_equal(cfg, 12, mix.cuda(), targets.cuda())


def test_trainer_accumulation_equals_hand_sequence_bf16():
    from oracle.golden_params import GOLDEN_CASES
    from wave_u_net_amd.training import Trainer, synthetic_source
    case = GOLDEN_CASES["full_small"]
    cfg = wun.get_config("baseline", compute_dtype="bf16", **dict(case["cfg"], num_frames=case["frames"], batch_size=4,
                                                                  init_sup_sep_lr=1e-3))
    probe = Trainer(cfg)
    assert probe.sep.effective_dtype == "bf16"
    mix, targets = synthetic_source(cfg, 4, probe.t_in, probe.t_out, probe.device, seed=5)()
    _hand_equal(cfg, 4, mix, targets)


# --------------------------------------------------------------------------------------------------- 6. data parallel
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("overlap", [True, False])
def test_two_ranks_accumulating_equal_one_process(tmp_path, overlap):
    """Two ranks on the one GPU (gloo), per-rank batch 6 in 2 micro-batches each, against one process with k = 1 on the
    global batch of 12."""
    import dp_worker
    from wave_u_net_amd import training
    steps = 3
    out = os.path.join(str(tmp_path), "dp_accum.npz")
    env = dict(os.environ, WUN_DIST_BACKEND="gloo", WUN_NO_TUNE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    if not overlap:
        env["WUN_NO_OVERLAP"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "dp_accum_worker.py"), out, str(steps)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    dp = np.load(out)
    assert int(dp["world"]) == 2 and int(dp["overlap"]) == int(overlap)
    cfg = dict(dp_worker.make_cfg(), batch_size=12)
    tr = training.Trainer(cfg)
    mix, targets = dp_worker.global_batch(cfg, tr.t_in, tr.t_out, 12)
    mix, targets = mix.to(tr.device), targets.to(tr.device)
    for _ in range(steps):
        tr.step(mix, targets)
    torch.cuda.synchronize()
    ref = tr.sep.params.cpu().numpy()
    assert np.abs(dp["params"] - ref).max() <= DP_TOL * max(1.0, np.abs(ref).max())
    assert np.all(np.isfinite(dp["losses"])) and dp["losses"][-1] < dp["losses"][0]
