"""GPU tests of the backward pass for a subset of the variables (include/wun.h: wun_backward_select, wun_loss_backward_select,
wun_adam_step_select) and of the frozen-variable / input-only paths of the torch.autograd module (wave_u_net_amd/autograd.py).

Every selection pattern runs on a forward pass whose full backward (wun_backward_ex / wun_loss_backward_ex) is the reference:
the selected tensors' gradient floats must be bit-equal to it, every other float of `grads` must still hold a sentinel bit
pattern written before the call, and d_mix / loss must be bit-equal to the full call's.  Both compute modes, a same-padding
and a context plan each, and the benchmarked configs[1] B = 16 plan with its pinned tuning table (where a misaligned launch
position would hand later launches other tilings and change bits)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_gpu_backward import BF16_CASES, _custom_loss, _setup, _setup_bf16, _upstream

import wave_u_net_amd as wun
from wave_u_net_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x7FC0BEEF                # a NaN no kernel writes
PATTERNS = ["all", "head", "decoder", "bottleneck", "mid_down", "down0", "every_other", "nothing"]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def _layers(sep):
    """Tensor indices per layer, in the order the forward pass runs the layers: down 0 .. L-1, bottleneck, (interp_j, up j)
    for each j, the output layer (every source's conv)."""
    names = [n for n, _, _ in sep._active.tensors]
    L = sep.num_layers

    def conv(c):
        base = "separator/conv1d" if c == 0 else "separator/conv1d_%d" % c
        return [names.index(base + "/kernel"), names.index(base + "/bias")]
    nconv = sum(1 for n in names if n.endswith("/kernel"))
    layers = {"down": [conv(i) for i in range(L)], "bott": conv(L), "up": [conv(L + 1 + j) for j in range(L)],
              "interp": [[names.index("separator/interp_%d" % j)] if "separator/interp_%d" % j in names else []
                         for j in range(L)],
              "head": [k for c in range(2 * L + 1, nconv) for k in conv(c)]}
    order = [*layers["down"], layers["bott"]]
    for j in range(L):
        if layers["interp"][j]:
            order.append(layers["interp"][j])
        order.append(layers["up"][j])
    order.append(layers["head"])
    layers["order"] = order
    return layers


def _pattern(sep, name):
    """The tensor mask of selection pattern `name` (uint8 per tensor, wun_plan_tensor order)."""
    ly = _layers(sep)
    L = sep.num_layers
    sel = []
    if name == "all":
        sel = [k for layer in ly["order"] for k in layer]
    elif name == "head":
        sel = ly["head"]
    elif name == "decoder":
        sel = [k for j in range(L) for k in ly["interp"][j] + ly["up"][j]] + ly["head"]
    elif name == "bottleneck":
        sel = ly["bott"]
    elif name == "mid_down":
        sel = ly["down"][L // 2]
    elif name == "down0":
        sel = ly["down"][0]
    elif name == "every_other":
        sel = [k for layer in ly["order"][::2] for k in layer]
    mask = np.zeros(len(sep._active.tensors), dtype=np.uint8)
    mask[sel] = 1
    return mask


def _ranges(sep, mask):
    sel = torch.zeros(int(sep._active.info.arena_floats), dtype=torch.bool)
    for k, (_, off, shp) in enumerate(sep._active.tensors):
        if mask[k]:
            sel[off:off + int(np.prod(shp))] = True
    return sel.cuda()


def _mask_arg(mask):
    return mask.ctypes.data_as(C.POINTER(C.c_uint8)), int(mask.size)


def _sentinel_like(t):
    g = torch.empty_like(t)
    g.view(torch.int32).fill_(SENTINEL)
    return g


class _Ctx(object):
    """One forward pass and its full-backward references."""

    def __init__(self, lib, sep, mix, tg):
        self.lib, self.sep = lib, sep
        names = sep.source_names
        outs = sep.get_output(mix, True)
        self.dout = _upstream(outs, names, tg).contiguous()
        self.tg = tg.contiguous()
        self.ws = sep._ws[sep._last_key]
        self.outs = sep._outs[sep._last_key]
        self.mix_shape = tuple(mix.shape)
        n = int(sep._active.info.arena_floats)
        self.g_full = self._full_backward(False)[0]
        self.g_full_m, self.dmix_full = self._full_backward(True)
        self.g_loss = torch.zeros(n, device="cuda")
        self.loss = torch.zeros((), device="cuda")
        _lib.check(lib.wun_loss_backward_ex(sep._active.handle, sep.params.data_ptr(), None, self.ws.data_ptr(),
                                            self.outs.data_ptr(), self.tg.data_ptr(), self.g_loss.data_ptr(),
                                            self.loss.data_ptr(), sep._stream(), None, None, 0))
        torch.cuda.synchronize()

    def _full_backward(self, want_mix):
        sep = self.sep
        g = torch.zeros(int(sep._active.info.arena_floats), device="cuda")
        dm = torch.empty(self.mix_shape, device="cuda") if want_mix else None
        _lib.check(self.lib.wun_backward_ex(sep._active.handle, sep.params.data_ptr(), None, self.ws.data_ptr(),
                                            self.outs.data_ptr(), self.dout.data_ptr(), g.data_ptr(),
                                            dm.data_ptr() if dm is not None else None, sep._stream(), None, None, 0))
        torch.cuda.synchronize()
        return g, dm

    def select(self, mask, want_mix, buckets=None):
        sep = self.sep
        g = _sentinel_like(self.g_full)
        dm = None
        if want_mix:
            dm = torch.empty(self.mix_shape, device="cuda")
            dm.view(torch.int32).fill_(SENTINEL)
        starts, events, nb = buckets if buckets else (None, None, 0)
        sel, nsel = _mask_arg(mask) if mask is not None else (None, 0)
        _lib.check(self.lib.wun_backward_select(sep._active.handle, sep.params.data_ptr(), None, self.ws.data_ptr(),
                                                self.outs.data_ptr(), self.dout.data_ptr(),
                                                g.data_ptr() if mask is None or mask.any() else None,
                                                dm.data_ptr() if dm is not None else None,
                                                sep._stream(), starts, events, nb, sel, nsel))
        return g, dm

    def loss_select(self, mask):
        sep = self.sep
        g = _sentinel_like(self.g_full)
        loss = torch.full((), float("nan"), device="cuda")
        _lib.check(self.lib.wun_loss_backward_select(sep._active.handle, sep.params.data_ptr(), None, self.ws.data_ptr(),
                                                     self.outs.data_ptr(), self.tg.data_ptr(), g.data_ptr(), loss.data_ptr(),
                                                     sep._stream(), None, None, 0, *_mask_arg(mask)))
        return g, loss


def _bits(t):
    return t.view(torch.int32)


def _check_grads(got, ref, sel, tag):
    gb, rb = _bits(got), _bits(ref)
    bad_sel = int((gb[sel] != rb[sel]).sum().item())
    bad_rest = int((gb[~sel] != SENTINEL).sum().item())
    assert bad_sel == 0 and bad_rest == 0, (tag, "selected floats that differ", bad_sel, "unselected floats written", bad_rest)


def _run_patterns(ctx, tag):
    sep = ctx.sep
    g, dm = ctx.select(None, True)                               # select = NULL: the full call
    torch.cuda.synchronize()
    assert torch.equal(_bits(g), _bits(ctx.g_full_m)) and torch.equal(_bits(dm), _bits(ctx.dmix_full)), tag
    for name in PATTERNS:
        mask = _pattern(sep, name)
        sel = _ranges(sep, mask)
        t = "%s/%s" % (tag, name)
        if mask.any():
            g, _ = ctx.select(mask, False)
            torch.cuda.synchronize()
            _check_grads(g, ctx.g_full, sel, t + "/backward")
            g, loss = ctx.loss_select(mask)
            torch.cuda.synchronize()
            _check_grads(g, ctx.g_loss, sel, t + "/loss_backward")
            assert _bits(loss).item() == _bits(ctx.loss).item(), (t, loss.item(), ctx.loss.item())
        g, dm = ctx.select(mask, True)
        torch.cuda.synchronize()
        if mask.any():
            _check_grads(g, ctx.g_full_m, sel, t + "/backward+d_mix")
        else:
            assert (_bits(g) == SENTINEL).all()                  # (grads = NULL: nothing written, nothing read)
        assert torch.equal(_bits(dm), _bits(ctx.dmix_full)), (t, "d_mix")


FP32_CASES = ["learned_same_small", "full_small", "full_multi_small"]


@pytest.mark.parametrize("name", FP32_CASES)
def test_selection_patterns_fp32(lib, name):
    sep, ocfg, params, mix, tg = _setup(name)
    _run_patterns(_Ctx(lib, sep, mix, tg), "f32_" + name)


@pytest.mark.parametrize("key", ["deep_l16_f48_shaped", "m5_shaped"])
def test_selection_patterns_bf16(lib, key):
    assert key in BF16_CASES
    sep, ocfg, params, mix, tg = _setup_bf16(key)
    assert sep.effective_dtype == "bf16"
    _run_patterns(_Ctx(lib, sep, mix, tg), "bf16_" + key)


def test_selection_patterns_benchmarked_plan_pinned_table(lib):
    """configs[1], M1 with context, B = 16, 147443 -> 16389, the pinned tuning table imported (as bench.py does)."""
    from wave_u_net_amd.training import Trainer, synthetic_source
    cfg = wun.get_config("m1_context")
    table = os.path.join(ROOT, "profiles", "round6_tune_table.txt")
    tr = Trainer(cfg, batch_size=16)
    assert (tr.t_in, tr.t_out) == (147443, 16389)
    mix, targets = synthetic_source(cfg, 16, tr.t_in, tr.t_out, tr.device, seed=1337)()
    tr.tune(mix, targets, pinned_table=open(table).read())
    sep = tr.sep
    assert sep.tune_export().startswith("wun-tune 2 ")
    tg = targets.to(torch.float32)
    _run_patterns(_Ctx(lib, sep, mix, tg), "bench_B16_pinned")


# ------------------------------------------------------------------------------------------------------- bucket events
@pytest.mark.parametrize("name", ["full_small", "learned_same_small"])
def test_bucket_events_fire_for_every_bucket(lib, name):
    sep, ocfg, params, mix, tg = _setup(name)
    ctx = _Ctx(lib, sep, mix, tg)
    n = int(sep._active.info.arena_floats)
    offs = sorted({off for _, off, _ in sep._active.tensors})
    starts = sorted(offs[::3], reverse=True)                     # every third tensor starts a bucket; the last starts at 0
    assert starts[-1] == 0
    ends = [n] + starts[:-1]
    comm = torch.cuda.Stream()
    for pattern in ("decoder", "every_other", "head", "down0"):
        mask = _pattern(sep, pattern)
        events = []
        for _ in starts:
            ev = torch.cuda.Event(enable_timing=False)
            ev.record(torch.cuda.current_stream())
            events.append(ev)
        st = (C.c_int64 * len(starts))(*starts)
        evs = (C.c_void_p * len(starts))(*[int(e.cuda_event) for e in events])
        copy = torch.zeros(n, device="cuda")
        g, _ = ctx.select(mask, False, buckets=(st, evs, len(starts)))
        for s, e, ev in zip(starts, ends, events):
            comm.wait_event(ev)
            with torch.cuda.stream(comm):
                copy[s:e].copy_(g[s:e])
        torch.cuda.synchronize()
        assert torch.equal(_bits(copy), _bits(g)), (name, pattern)
        _check_grads(g, ctx.g_full, _ranges(sep, mask), name + "/buckets/" + pattern)


# ------------------------------------------------------------------------------------------------------------ autograd
def _encoder(net):
    L = net.sep.num_layers
    return ["separator/conv1d%s/%s" % ("" if c == 0 else "_%d" % c, kb) for c in range(L + 1) for kb in ("kernel", "bias")]


@pytest.mark.parametrize("name", ["full_small", "learned_same_small"])
def test_autograd_frozen_encoder(lib, name):
    sep, ocfg, params, mix, tg = _setup(name)
    net = sep.module()
    ga_full = torch.autograd.grad(_custom_loss(net(mix), tg), [net.arena])[0]
    frozen = _encoder(net)
    net.freeze(frozen)
    assert net.frozen() == [n for n in net.variable_names() if n in set(frozen)]
    _custom_loss(net(mix), tg).backward()
    g = net.arena.grad
    mask = np.array([0 if n in set(frozen) else 1 for n in net.variable_names()], dtype=np.uint8)
    sel = _ranges(sep, mask)
    torch.cuda.synchronize()
    assert torch.equal(_bits(g[sel]), _bits(ga_full[sel]))
    assert (g[~sel] == 0).all()
    assert (g[sel] != 0).any()
    net.unfreeze(frozen)
    assert net.frozen() == []
    with pytest.raises(KeyError):
        net.freeze(["separator/conv1d_99/kernel"])
    net.freeze(["separator/conv1d_1/kernel"])                  # kernel without its bias: refused at backward
    with pytest.raises(NotImplementedError):
        _custom_loss(net(mix), tg).backward()


@pytest.mark.parametrize("name", ["full_small", "learned_same_small"])
def test_autograd_input_only(lib, name):
    sep, ocfg, params, mix, tg = _setup(name)
    net = sep.module()
    m = mix.clone().requires_grad_(True)
    y = net(m)
    _, gm_full = torch.autograd.grad(_custom_loss(y, tg), [net.arena, m])
    net.arena.requires_grad_(False)
    net.arena.grad = None
    m2 = mix.clone().requires_grad_(True)
    _custom_loss(net(m2), tg).backward()
    torch.cuda.synchronize()
    assert net.arena.grad is None
    assert torch.equal(_bits(m2.grad), _bits(gm_full))
    # the separator's own input-only gradient: the same bits, self.grads untouched
    outs = sep.get_output(mix, True)
    before = sep.grads.clone()
    dm = sep.backward(_upstream(outs, sep.source_names, tg), input_grad=True, variables=[])
    torch.cuda.synchronize()
    assert torch.equal(_bits(dm), _bits(gm_full)) and torch.equal(_bits(sep.grads), _bits(before))


# ---------------------------------------------------------------------------------------------------------------- Adam
@pytest.mark.parametrize("name", ["full_small", "full_multi_small"])
def test_adam_step_select(lib, name):
    sep, ocfg, params, mix, tg = _setup(name)
    for _ in range(3):                                           # m, v non-zero
        sep.get_output(mix, True)
        sep.loss_and_gradients(tg)
        sep.adam_step(1e-3)
    sep.get_output(mix, True)
    sep.loss_and_gradients(tg)
    torch.cuda.synchronize()
    snap = [t.clone() for t in (sep.params, sep.adam_m, sep.adam_v)]
    step0 = sep.global_step
    names = [n for n, _, _ in sep._active.tensors]
    chosen = [n for k, n in enumerate(names) if k % 3 != 1]      # an irregular subset: runs of several tensors, single ones
    mask = sep.select_mask(chosen)
    sep.adam_step(1e-3, variables=chosen)
    torch.cuda.synchronize()
    assert sep.global_step == step0 + 1
    got = [t.clone() for t in (sep.params, sep.adam_m, sep.adam_v)]
    for t, s in zip((sep.params, sep.adam_m, sep.adam_v), snap):
        t.copy_(s)
    _lib.check(lib.wun_adam_step(sep._active.handle, sep.params.data_ptr(), sep.grads.data_ptr(), sep.adam_m.data_ptr(),
                                 sep.adam_v.data_ptr(), step0 + 1, 1e-3, 0.9, 0.999, 1e-8, 1.0, sep._stream()))
    torch.cuda.synchronize()
    sel = _ranges(sep, mask)
    for a, full, s, what in zip(got, (sep.params, sep.adam_m, sep.adam_v), snap, ("params", "m", "v")):
        assert torch.equal(_bits(a[sel]), _bits(full[sel])), what
        assert torch.equal(_bits(a[~sel]), _bits(s[~sel])), what
        assert not torch.equal(_bits(a[sel]), _bits(s[sel])), what
    # nothing selected: no launch, nothing moves
    before = [t.clone() for t in (sep.params, sep.adam_m, sep.adam_v)]
    sep.adam_step(1e-3, variables=[])
    torch.cuda.synchronize()
    for t, b in zip((sep.params, sep.adam_m, sep.adam_v), before):
        assert torch.equal(_bits(t), _bits(b))
