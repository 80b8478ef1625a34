"""GPU tests of the extended optimizer (include/wun.h: wun_optim_step, wun_ema_update) and of everything built
on it: adam_step's new arguments, the EMA arena and ema_weights(), the Trainer's optimizer / lr_schedule settings,
checkpoints, validation and the CLI.

Plans (the smallest that can still go wrong):
  small       2 layers, 8 filters, filter_size 5, the minimum frames -- in fp32 and in the bf16 mode (which it qualifies for)
  odd         the odd-filter geometry of the golden case odd_filters_small: tensor sizes and offsets are no multiples of 4
  many        7 layers, learned upsampling, four sources: 45 tensors, one above 8192 floats -- the norm has more than one
              chunk, and with the kernels decaying and the biases not, the walk has over 32 runs: more than one range batch
The float64 oracle and the bit-exact float32 restatements of the step and of the EMA line live in tests/_optim_np.py."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _optim_np as onp
from _unaligned import _offset_copy

from oracle.golden_params import GOLDEN_CASES

import wave_u_net_amd as wun
from wave_u_net_amd import _lib, checkpoint, training, validation
from wave_u_net_amd.separator import UnetAudioSeparator

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x7FC0BEEF                # a NaN no kernel writes
B1, B2, EPS = 0.9, 0.999, 1e-8


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def _small_cfg(**kw):
    # (input_filter_size follows filter_size: get_padding sizes the hops of separate_track by it)
    return wun.get_config("baseline", **dict(dict(num_layers=2, num_initial_filters=8, filter_size=5, input_filter_size=5,
                                                  num_frames=64, context=True, output_type="difference", mono_downmix=False),
                                             **kw))


PLANS = {
    "small": lambda: _small_cfg(),
    "small_bf16": lambda: _small_cfg(compute_dtype="bf16"),
    "odd": lambda: wun.get_config("baseline", **GOLDEN_CASES["odd_filters_small"]["cfg"]),
    "many": lambda: wun.get_config("baseline", num_layers=7, num_initial_filters=8, context=True, upsampling="learned",
                                   output_type="difference", task="multi_instrument"),
}


def _separator(kind, batch=2):
    sep = UnetAudioSeparator(PLANS[kind](), device="cuda:0")
    frames = int(sep.get_padding(np.array([batch, 1, 0]))[0][1])           # the minimum get_padding allows
    sep._active = sep._plan(batch, frames)
    sep._ensure_variables(sep._active)
    if kind == "small_bf16":
        assert sep.effective_dtype == "bf16"
    return sep, frames


def _sizes(sep):
    return [(off, int(np.prod(shp))) for _, off, shp in sep._active.tensors]


def _floats(sep, mask):
    """bool [arena]: the floats of the tensors whose byte of mask is set."""
    sel = torch.zeros(int(sep._active.info.arena_floats), dtype=torch.bool)
    for k, (off, n) in enumerate(_sizes(sep)):
        if mask[k]:
            sel[off:off + n] = True
    return sel.cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


class Arenas(object):
    """params, grads, m, v and ema of a plan, random: every tensor at its own magnitude, m with the gradient's sign (as a run
    of steps in one direction leaves it: m itself does not cancel), v >= 0."""

    def __init__(self, sep, seed=3):
        n = int(sep._active.info.arena_floats)
        gen = torch.Generator(device="cpu").manual_seed(seed)
        sz = _sizes(sep)
        scale = torch.ones(n)
        for k, (o, c) in enumerate(sz):
            scale[o:o + c] = 10.0 ** (-3 + 4 * k / max(1, len(sz) - 1))
        self.g = (torch.randn(n, generator=gen) * scale).cuda()
        self.p = torch.randn(n, generator=gen).cuda()
        self.m = (torch.sign(self.g.cpu()) * torch.rand(n, generator=gen) * scale).cuda()
        self.v = ((torch.rand(n, generator=gen) + 0.1) * scale * scale).cuda()
        self.ema = (self.p.cpu() + 0.05 * torch.randn(n, generator=gen)).cuda()

    def clone(self, shift=False):
        other = object.__new__(Arenas)
        for k in ("p", "g", "m", "v", "ema"):
            setattr(other, k, _offset_copy(getattr(self, k)) if shift else getattr(self, k).clone())
        return other

    def four(self):
        return self.p, self.m, self.v, self.ema


def _mask_arg(mask):
    if mask is None:
        return None, 0
    return mask.ctypes.data_as(C.POINTER(C.c_uint8)), int(mask.size)


def _ws(lib, sep):
    return (torch.empty(int(lib.wun_grad_norm_workspace_floats(sep._active.handle)), device="cuda"),
            torch.zeros(1, dtype=torch.int64, device="cuda"))


def _optim(lib, sep, a, step=4, lr=1e-3, gscale=1.0, wd=0.0, ema_decay=None, clip=math.inf, flags=0, sel=None, dec=None,
           ws=None, skipped=None, stream=None):
    cfg = _lib.WunOptimConfig(B1, B2, EPS, wd, ema_decay if ema_decay is not None else 0.0, clip, flags)
    _lib.check(lib.wun_optim_step(sep._active.handle, a.p.data_ptr(), a.g.data_ptr(), a.m.data_ptr(), a.v.data_ptr(),
                                  a.ema.data_ptr() if ema_decay is not None else None, step, lr, gscale, C.byref(cfg),
                                  ws.data_ptr() if ws is not None else None, skipped.data_ptr() if skipped is not None else None,
                                  stream if stream is not None else sep._stream(), *_mask_arg(sel), *_mask_arg(dec)))


def _every_other(sep):
    return np.array([1 if k % 2 == 0 else 0 for k in range(len(sep._active.tensors))], dtype=np.uint8)


def _kernels(sep):
    return np.array([1 if len(shp) > 1 else 0 for _, _, shp in sep._active.tensors], dtype=np.uint8)


def _equal(xs, ys, tag, names=("params", "m", "v", "ema")):
    for x, y, what in zip(xs, ys, names):
        assert torch.equal(_bits(x), _bits(y)), (tag, what)


def test_plans_are_what_the_cases_need():
    sep, _ = _separator("many")
    sz = [n for _, n in _sizes(sep)]
    assert len(sz) > 32 and max(sz) > 8192                  # more than one range batch (kernels decay, biases do not), > 1 chunk
    assert len(sz) // 2 <= 32                               # every other tensor: runs that never merge, one batch
    sep, _ = _separator("odd")
    assert any(o % 4 for o, _ in _sizes(sep)) and any(n % 4 for _, n in _sizes(sep))


# ------------------------------------------------------------------------------------------------ 1. bit equalities
@pytest.mark.parametrize("kind", ["small", "small_bf16", "odd", "many"])
@pytest.mark.parametrize("select", ["all", "every_other"])
def test_bit_equal_to_the_adam_entries(lib, kind, select):
    """Decay 0, no EMA: params, m and v bit-equal to wun_adam_step / _select / _clip (clipping active, inactive, skipping).
    With an EMA the three arenas keep those bits, the EMA is the float32 formula applied to them, and wun_ema_update after
    wun_adam_step gives the fused EMA's bits.  (Fails without the feature: the symbol does not exist.)"""
    sep, _ = _separator(kind)
    a0 = Arenas(sep)
    sel = None if select == "all" else _every_other(sep)
    ws, cnt = _ws(lib, sep)
    h, s = sep._active.handle, sep._stream()
    step, lr, gs = 4, 1e-3, 0.5

    ref = a0.clone()
    if sel is None:
        _lib.check(lib.wun_adam_step(h, ref.p.data_ptr(), ref.g.data_ptr(), ref.m.data_ptr(), ref.v.data_ptr(), step, lr, B1, B2,
                                     EPS, gs, s))
    else:
        _lib.check(lib.wun_adam_step_select(h, ref.p.data_ptr(), ref.g.data_ptr(), ref.m.data_ptr(), ref.v.data_ptr(), step, lr,
                                            B1, B2, EPS, gs, s, *_mask_arg(sel)))
    got = a0.clone()
    _optim(lib, sep, got, step, lr, gs, sel=sel)                                    # no norm launch: norm_ws NULL
    _equal(got.four(), ref.four()[:3] + (a0.ema,), "plain")
    for warm in (0, _lib.WUN_OPTIM_EMA_WARMUP):
        got = a0.clone()
        _optim(lib, sep, got, step, lr, gs, ema_decay=0.99, flags=warm, sel=sel)
        _equal(got.four()[:3], ref.four()[:3], "ema on")
        want = torch.from_numpy(onp.ema32(a0.ema.cpu().numpy(), ref.p.cpu().numpy(), 0.99, step, bool(warm))).cuda()
        if sel is not None:
            want = torch.where(_floats(sep, sel), want, a0.ema)
        assert torch.equal(_bits(got.ema), _bits(want)), ("ema formula", warm)
        assert not torch.equal(_bits(got.ema), _bits(a0.ema))
        alone = a0.ema.clone()
        _lib.check(lib.wun_ema_update(h, alone.data_ptr(), ref.p.data_ptr(), 0.99, step, warm, s, *_mask_arg(sel)))
        assert torch.equal(_bits(alone), _bits(got.ema)), ("wun_ema_update", warm)

    # the clipped entry: active, inactive, skipping
    _lib.check(lib.wun_grad_norm(h, a0.g.data_ptr(), gs, ws.data_ptr(), s, *_mask_arg(sel)))
    norm = float(ws[len(sep._active.tensors)].item())
    for clip, flag, bad in ((0.1 * norm, 0, False), (2.0 * norm, 1, False), (math.inf, 1, False), (1.0, 1, True)):
        ref, got = a0.clone(), a0.clone()
        if bad:
            k = int(np.nonzero(sel)[0][-1]) if sel is not None else len(sep._active.tensors) - 1
            o, n = _sizes(sep)[k]
            ref.g[o + n // 3] = float("inf")
            got.g[o + n // 3] = float("inf")
        bare = got.clone()                                                          # the same case with ema = NULL
        before = int(cnt.item())
        _lib.check(lib.wun_adam_step_clip(h, ref.p.data_ptr(), ref.g.data_ptr(), ref.m.data_ptr(), ref.v.data_ptr(), step, lr,
                                          B1, B2, EPS, gs, clip, flag, ws.data_ptr(), cnt.data_ptr(), s, *_mask_arg(sel)))
        _optim(lib, sep, got, step, lr, gs, ema_decay=0.99, clip=clip, flags=flag, sel=sel, ws=ws, skipped=cnt)
        _optim(lib, sep, bare, step, lr, gs, ema_decay=None, clip=clip, flags=flag, sel=sel, ws=ws, skipped=cnt)
        torch.cuda.synchronize()
        _equal(got.four()[:3], ref.four()[:3], ("clip", clip, flag, bad))
        # decay 0 and no EMA, with the norm / clip / skip prologue: wun_adam_step_clip's bits, the ema buffer never touched
        _equal(bare.four(), ref.four()[:3] + (a0.ema,), ("clip, no ema", clip, flag, bad))
        if bad:
            _equal(got.four(), a0.four(), "skipped")
            _equal(bare.four(), a0.four(), "skipped, no ema")
            assert int(cnt.item()) == before + 3                                    # one per entry
        else:
            assert int(cnt.item()) == before
            assert not torch.equal(_bits(got.ema), _bits(a0.ema))
            assert not torch.equal(_bits(bare.p), _bits(a0.p))


@pytest.mark.parametrize("kind", ["small", "small_bf16", "odd", "many"])
@pytest.mark.parametrize("select", ["all", "every_other"])
def test_bits_of_every_entry_against_the_float32_restatement(lib, kind, select):
    """params, m and v of wun_adam_step / _select, of wun_adam_step_clip (clip active at 0.1 N, inactive at 2 N, +inf with the
    skip flag) and of wun_optim_step with the rank > 1 tensors decaying and no EMA, bit for bit against _optim_np.step32 -- numpy
    with an exact fmaf, no library call -- on the selected floats; every other float keeps its bits.  N is the fp32 global norm
    the call leaves in norm_ws (tests/test_gpu_grad_clip.py checks its accuracy)."""
    sep, _ = _separator(kind)
    a0 = Arenas(sep)
    sel = None if select == "all" else _every_other(sep)
    nt = len(sep._active.tensors)
    chosen = _floats(sep, sel if sel is not None else np.ones(nt, dtype=np.uint8))
    dec = _kernels(sep)
    ws, cnt = _ws(lib, sep)
    h, s = sep._active.handle, sep._stream()
    step, lr, gs, wd = 4, 1e-3, 0.5, 0.1
    p0, g0, m0, v0 = (t.cpu().numpy() for t in (a0.p, a0.g, a0.m, a0.v))

    def check(got, tag, **kw):
        torch.cuda.synchronize()
        want = onp.step32(p0, g0, m0, v0, step, lr, B1, B2, EPS, gs, **kw)
        for x, w, o, what in zip((got.p, got.m, got.v), want, (a0.p, a0.m, a0.v), ("params", "m", "v")):
            w = torch.where(chosen, torch.from_numpy(w).cuda(), o)
            assert torch.equal(_bits(x), _bits(w)), (tag, what, int((_bits(x) != _bits(w)).sum().item()))
        assert not torch.equal(_bits(got.p), _bits(a0.p))
        assert torch.equal(_bits(got.g), _bits(a0.g)) and torch.equal(_bits(got.ema), _bits(a0.ema))

    got = a0.clone()
    if sel is None:
        _lib.check(lib.wun_adam_step(h, got.p.data_ptr(), got.g.data_ptr(), got.m.data_ptr(), got.v.data_ptr(), step, lr, B1, B2,
                                     EPS, gs, s))
    else:
        _lib.check(lib.wun_adam_step_select(h, got.p.data_ptr(), got.g.data_ptr(), got.m.data_ptr(), got.v.data_ptr(), step, lr,
                                            B1, B2, EPS, gs, s, *_mask_arg(sel)))
    check(got, "adam")

    def clipped(clip, flag):
        got = a0.clone()
        _lib.check(lib.wun_adam_step_clip(h, got.p.data_ptr(), got.g.data_ptr(), got.m.data_ptr(), got.v.data_ptr(), step, lr, B1,
                                          B2, EPS, gs, clip, flag, ws.data_ptr(), cnt.data_ptr(), s, *_mask_arg(sel)))
        return got, float(ws[nt].item())

    norm = clipped(math.inf, 0)[1]                     # the norm does not depend on the clip: every call below leaves this value
    assert math.isfinite(norm) and norm > 0
    for factor, flag in ((0.1, 0), (2.0, 0), (math.inf, _lib.WUN_CLIP_SKIP_NONFINITE)):
        got, n = clipped(factor * norm, flag)
        assert n == norm and int(cnt.item()) == 0
        check(got, ("clip", factor, flag), norm=norm, clip=factor * norm)
    got = a0.clone()
    _optim(lib, sep, got, step, lr, gs, wd=wd, sel=sel, dec=dec)
    check(got, "decay", weight_decay=wd, decay=_floats(sep, dec).cpu().numpy())


# ------------------------------------------------------------------------------------------------ 2. against float64
def _ulps(got, want64, *operands):
    """|got - want| in float32 ulps of the largest of |want| and the |operands| the value was formed from (the rule of
    test_gpu_specunet_train.py: a sum that cancels below its operands is not held to its own, smaller, ulp)."""
    scale = np.abs(np.asarray(want64, np.float64))
    for o in operands:
        scale = np.maximum(scale, np.abs(np.asarray(o, np.float64)))
    ulp = np.spacing(np.maximum(scale.astype(np.float32), np.float32(1e-37))).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - np.asarray(want64, np.float64)) / ulp


@pytest.mark.parametrize("kind", ["small", "small_bf16", "odd", "many"])
def test_three_steps_against_float64(lib, kind):
    """3 consecutive steps with decay (kernels only) and EMA warm-up on, each against the float64 formulas applied to the
    state the step started from: theta, m and v within 4 ulp, the ulp that of the largest operand of the sum that forms the
    value (theta: the decayed theta and the update; m: b1 m and (1 - b1) g; v: its own).  The EMA within 2 ulp of the float64
    formula on the new theta AS STORED (the line's input), the ulp that of the largest operand of its two sums (ema, theta,
    (1 - d)(ema - theta)): its roundings are the difference (1/2 ulp of it, times 1 - d <= 1), the product (1/2) and the final
    difference (1/2), which stays below 2 of that ulp also where ema and theta have opposite signs and the difference lies a
    binade above both.  The worst figures are printed before the assertion (DESIGN.md 5.26 records them)."""
    sep, _ = _separator(kind)
    a = Arenas(sep, seed=11)
    dec = _kernels(sep)
    decay = _floats(sep, dec).cpu().numpy()
    lr, wd, d, gs = 3e-3, 0.1, 0.999, 1.0
    worst = {"theta": 0.0, "m": 0.0, "v": 0.0, "ema": 0.0}
    gen = torch.Generator(device="cpu").manual_seed(5)
    for step in (1, 2, 3):
        p0, g, m0, v0, e0 = (t.cpu().numpy().astype(np.float64) for t in (a.p, a.g, a.m, a.v, a.ema))
        _optim(lib, sep, a, step, lr, gs, wd=wd, ema_decay=d, flags=_lib.WUN_OPTIM_EMA_WARMUP, dec=dec)
        torch.cuda.synchronize()
        p1, m1, v1, e1 = (t.cpu().numpy() for t in a.four())
        # the library's inputs are fp32: lr, weight_decay and the betas as it was handed them
        lr32, wd32 = float(np.float32(lr)), float(np.float32(wd))
        b1, b2, eps = float(np.float32(B1)), float(np.float32(B2)), float(np.float32(EPS))
        t, m, v = onp.step64(p0, g, m0, v0, step, lr32, b1, b2, eps, gs, weight_decay=wd32, decay=decay)
        pd = np.where(decay, p0 * (1.0 - lr32 * wd32), p0)
        worst["theta"] = max(worst["theta"], float(_ulps(p1, t, pd, t - pd).max()))
        worst["m"] = max(worst["m"], float(_ulps(m1, m, b1 * m0, (1 - b1) * g).max()))
        worst["v"] = max(worst["v"], float(_ulps(v1, v).max()))
        e = onp.ema64(e0, p1.astype(np.float64), d, step, True)
        worst["ema"] = max(worst["ema"], float(_ulps(e1, e, e0, p1, onp.ema_weight(d, step, True) * (e0 - p1)).max()))
        assert not np.array_equal(p1[decay], onp.step64(p0, g, m0, v0, step, lr32, b1, b2, eps, gs)[0][decay].astype(np.float32))
        # the next step's gradient: new values, the sign of m
        a.g.copy_((torch.sign(a.m.cpu()) * torch.rand(a.g.numel(), generator=gen) * a.g.abs().cpu().clamp_min(1e-6)).cuda())
    print("worst ulps [%s]: %s" % (kind, worst))
    assert worst["theta"] <= 4 and worst["m"] <= 4 and worst["v"] <= 4 and worst["ema"] <= 2, worst


# ------------------------------------------------------------------------------------------------ 3. footprint
@pytest.mark.parametrize("kind", ["odd", "many"])
def test_footprint(lib, kind):
    sep, _ = _separator(kind)
    a0 = Arenas(sep)
    sel = _every_other(sep)
    dec = np.zeros_like(sel)
    dec[np.nonzero(sel)[0][::2]] = 1                                 # half of the selected tensors decay ...
    dec[np.nonzero(sel == 0)[0][::2]] = 1                            # ... and unselected ones named in decay_select do not
    unsel = ~_floats(sep, sel)
    for t in (a0.p, a0.g, a0.m, a0.v, a0.ema):                       # a NaN pattern in every float no selected tensor owns
        _bits(t)[unsel] = SENTINEL
    ws, cnt = _ws(lib, sep)
    plain, decayed = a0.clone(), a0.clone()
    _optim(lib, sep, plain, ema_decay=0.9, sel=sel)
    _optim(lib, sep, decayed, wd=0.1, ema_decay=0.9, sel=sel, dec=dec)
    torch.cuda.synchronize()
    both = _floats(sep, sel & dec)
    only_sel = _floats(sep, sel & (1 - dec))
    assert both.any() and only_sel.any()
    for x, y, o in zip(decayed.four(), plain.four(), a0.four()):
        assert torch.equal(_bits(x)[only_sel], _bits(y)[only_sel])   # not in decay_select: the no-decay bits
        assert torch.equal(_bits(x)[unsel], _bits(o)[unsel]) and (_bits(x)[unsel] == SENTINEL).all()
        assert torch.equal(_bits(y)[unsel], _bits(o)[unsel])
    assert not torch.equal(_bits(decayed.p)[both], _bits(plain.p)[both])
    assert torch.equal(_bits(decayed.m)[both], _bits(plain.m)[both]) and torch.equal(_bits(decayed.v)[both], _bits(plain.v)[both])
    # decay_select NULL = every selected tensor decays; weight_decay 0 with a table = no decay at all
    every, none = a0.clone(), a0.clone()
    _optim(lib, sep, every, wd=0.1, ema_decay=0.9, sel=sel)
    _optim(lib, sep, none, wd=0.0, ema_decay=0.9, sel=sel, dec=dec)
    assert torch.equal(_bits(every.p)[both], _bits(decayed.p)[both])
    assert not torch.equal(_bits(every.p)[only_sel], _bits(plain.p)[only_sel])
    _equal(none.four(), plain.four(), "weight_decay 0")
    # a non-finite gradient: with the flag nothing is written and skipped grows by one; without it the NaN flows through
    bad = a0.clone()
    o, n = _sizes(sep)[int(np.nonzero(sel)[0][0])]
    bad.g[o + n // 2] = float("nan")
    g_bad = bad.g.clone()
    _optim(lib, sep, bad, wd=0.1, ema_decay=0.9, clip=1.0, flags=_lib.WUN_CLIP_SKIP_NONFINITE, sel=sel, dec=dec, ws=ws,
           skipped=cnt)
    torch.cuda.synchronize()
    _equal(bad.four(), a0.four(), "skipped")
    assert torch.equal(_bits(bad.g), _bits(g_bad)) and int(cnt.item()) == 1
    _optim(lib, sep, bad, wd=0.1, ema_decay=0.9, clip=1.0, flags=0, sel=sel, dec=dec, ws=ws, skipped=cnt)
    torch.cuda.synchronize()
    assert torch.isnan(bad.p[o + n // 2]).item() and torch.isnan(bad.ema[o + n // 2]).item() and int(cnt.item()) == 1
    for x, orig in zip(bad.four(), a0.four()):
        assert torch.equal(_bits(x)[unsel], _bits(orig)[unsel])


@pytest.mark.parametrize("with_ema", [False, True])
def test_skip_is_counted_once_over_several_launches(lib, with_ema):
    """'many' with the kernels decaying and the biases not: over 32 runs, so the walk takes more than one launch.  A skipped step
    still increments `skipped` once and writes nothing; the same gradient made finite again applies, with the bits of the
    step without the skip flag."""
    sep, _ = _separator("many")
    a0 = Arenas(sep)
    dec = _kernels(sep)
    assert len(sep._active.tensors) > 32 and int(np.abs(np.diff(dec.astype(np.int8))).sum()) + 1 > 32      # runs > one batch
    ws, cnt = _ws(lib, sep)
    d = 0.9 if with_ema else None
    bad = a0.clone()
    o, n = _sizes(sep)[len(sep._active.tensors) - 2]                  # a tensor of the LAST launch's runs
    bad.g[o + n // 2] = float("inf")
    g_bad = bad.g.clone()
    _optim(lib, sep, bad, wd=0.1, ema_decay=d, clip=1.0, flags=_lib.WUN_CLIP_SKIP_NONFINITE, dec=dec, ws=ws, skipped=cnt)
    torch.cuda.synchronize()
    assert int(cnt.item()) == 1
    _equal(bad.four(), a0.four(), "skipped")
    assert torch.equal(_bits(bad.g), _bits(g_bad))
    _optim(lib, sep, bad, wd=0.1, ema_decay=d, clip=1.0, flags=_lib.WUN_CLIP_SKIP_NONFINITE, dec=dec, ws=ws, skipped=cnt)
    torch.cuda.synchronize()
    assert int(cnt.item()) == 2
    _equal(bad.four(), a0.four(), "skipped twice")
    good, plain = a0.clone(), a0.clone()
    _optim(lib, sep, good, wd=0.1, ema_decay=d, clip=1.0, flags=_lib.WUN_CLIP_SKIP_NONFINITE, dec=dec, ws=ws, skipped=cnt)
    _optim(lib, sep, plain, wd=0.1, ema_decay=d, clip=1.0, flags=0, dec=dec, ws=ws)
    torch.cuda.synchronize()
    assert int(cnt.item()) == 2
    _equal(good.four(), plain.four(), "finite")
    assert not torch.equal(_bits(good.p), _bits(a0.p)) and torch.equal(_bits(good.ema), _bits(a0.ema)) != with_ema


# ------------------------------------------------------------------------------------------------ 4. independence
def _entry(lib, sep, entry, ws, cnt):
    """call(arenas, stream=None): one step through `entry`, with everything on that the entry has."""
    skip = _lib.WUN_CLIP_SKIP_NONFINITE
    if entry == "optim":
        kw = dict(wd=0.05, ema_decay=0.99, clip=1e-3, flags=_lib.WUN_OPTIM_EMA_WARMUP | skip, dec=_kernels(sep), ws=ws, skipped=cnt)
        return lambda a, stream=None: _optim(lib, sep, a, stream=stream, **kw)

    def call(a, stream=None):
        args = (sep._active.handle, a.p.data_ptr(), a.g.data_ptr(), a.m.data_ptr(), a.v.data_ptr(), 4, 1e-3, B1, B2, EPS, 1.0)
        s = stream if stream is not None else sep._stream()
        if entry == "adam":
            _lib.check(lib.wun_adam_step(*args, s))
        else:
            _lib.check(lib.wun_adam_step_clip(*args, 1e-3, skip, ws.data_ptr(), cnt.data_ptr(), s, None, 0))
    return call


@pytest.mark.parametrize("kind", ["odd", "many"])
@pytest.mark.parametrize("entry", ["optim", "adam", "adam_clip"])
def test_bits_do_not_depend_on_stream_repetition_or_alignment(lib, kind, entry):
    sep, _ = _separator(kind)
    a0 = Arenas(sep)
    ws, cnt = _ws(lib, sep)
    call = _entry(lib, sep, entry, ws, cnt)
    ref = a0.clone()
    call(ref)
    torch.cuda.synchronize()
    assert not torch.equal(_bits(ref.p), _bits(a0.p)) and int(cnt.item()) == 0
    again = a0.clone()
    call(again)
    _equal(again.four(), ref.four(), "repetition")
    side = torch.cuda.Stream()
    other = a0.clone()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        call(other, stream=C.c_void_p(side.cuda_stream))
    side.synchronize()
    _equal(other.four(), ref.four(), "stream")
    shifted = a0.clone(shift=True)                                   # every arena one float behind an allocation's start:
    call(shifted)                                                    # the 16-byte path with a scalar head
    _equal(shifted.four(), ref.four(), "one-float shift of every arena")
    mixed = a0.clone()                                               # arenas that do not share an alignment: the scalar path
    if entry == "optim":
        mixed.ema = _offset_copy(mixed.ema)
        mixed.v = _offset_copy(mixed.v)
    else:
        mixed.g = _offset_copy(mixed.g)
    call(mixed)
    torch.cuda.synchronize()
    _equal(mixed.four(), ref.four(), "mixed alignment")
    if entry == "optim":
        alone_a, alone_b = a0.ema.clone(), _offset_copy(a0.ema)
        for e in (alone_a, alone_b):
            _lib.check(lib.wun_ema_update(sep._active.handle, e.data_ptr(), a0.p.data_ptr(), 0.99, 3, 0, sep._stream(), None, 0))
        assert torch.equal(_bits(alone_a), _bits(alone_b))


def test_adam_step_footprint_without_a_selection(lib):
    """wun_adam_step with a NULL selection on 'odd', the four arenas embedded in larger buffers with sentinels before and
    behind: exactly the arena's floats are written -- the ends of the 16-byte loop, with the arena (a multiple of 4 floats) at a
    16-byte boundary (front of 4 floats: neither head nor tail), one float past it (5: a head of 3, a tail of 1) and three
    past it (7: a head of 1, a tail of 3) -- and the bits are those of the call on plain buffers."""
    sep, _ = _separator("odd")
    a0 = Arenas(sep)
    n = int(sep._active.info.arena_floats)
    assert n % 4 == 0 and n > 1024
    call = _entry(lib, sep, "adam", None, None)
    ref = a0.clone()
    call(ref)
    torch.cuda.synchronize()
    back = 7
    for front in (4, 5, 7):
        bufs, inner = {}, object.__new__(Arenas)
        for k in ("p", "g", "m", "v", "ema"):
            bufs[k] = torch.full((front + n + back,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
            setattr(inner, k, bufs[k][front:front + n])
            getattr(inner, k).copy_(getattr(a0, k))
            assert getattr(inner, k).data_ptr() % 16 == 4 * (front % 4)
        call(inner)
        torch.cuda.synchronize()
        _equal(inner.four(), ref.four(), ("embedded", front))
        assert torch.equal(_bits(inner.g), _bits(a0.g))
        for k, b in bufs.items():
            assert (_bits(b)[:front] == SENTINEL).all() and (_bits(b)[front + n:] == SENTINEL).all(), (front, k)


# ------------------------------------------------------------------------------------------------ 5. ema_weights()
def _trained_with_ema(kind, steps=3):
    sep, frames = _separator(kind, batch=2)
    gen = torch.Generator(device="cpu").manual_seed(21)
    mix = (torch.rand((2, frames, sep.num_channels), generator=gen) - 0.5).cuda()
    tout = int(sep._active.info.output_frames)
    tg = (0.3 * (torch.rand((len(sep.source_names), 2, tout, sep.num_channels), generator=gen) - 0.5)).cuda()
    for _ in range(steps):
        sep.get_output(mix, True)
        sep.loss_and_gradients(tg)
        sep.adam_step(2e-2, weight_decay=0.01, ema_decay=0.5)        # a large lr: the EMA clearly lags the weights
    torch.cuda.synchronize()
    return sep, mix, tg


def _track_estimates(sep, cfg):
    from wave_u_net_amd.evaluate import separate_track
    rng = np.random.default_rng(8)
    audio = rng.uniform(-0.5, 0.5, (700, sep.num_channels)).astype(np.float32)
    return separate_track(cfg, sep, audio, cfg["expected_sr"], batch_hops=3, return_device=True).clone()


@pytest.mark.parametrize("kind", ["small", "small_bf16"])
def test_ema_weights_runs_on_the_ema_values(lib, kind):
    """get_output(x, False) and separate_track under ema_weights() are bit-equal to a fresh separator loaded with
    ema_variables() -- in the bf16 mode this pins that the packed weight images follow the arena in use --, the trained
    outputs are back after the block, also after an exception, and the block is refused while gradients are pending."""
    sep, mix, tg = _trained_with_ema(kind)
    cfg = sep.model_config
    before = torch.stack(list(sep.get_output(mix, False).values())).clone()
    before_track = _track_estimates(sep, cfg)
    p_ptr, e_ptr = sep.params.data_ptr(), sep.ema.data_ptr()
    with sep.ema_weights() as inner:
        assert inner is sep and sep.params.data_ptr() == e_ptr and sep.ema.data_ptr() == p_ptr       # exchanged, not copied
        got = torch.stack(list(sep.get_output(mix, False).values())).clone()
        got_track = _track_estimates(sep, cfg)
        # the block infers only: nothing that makes, applies or mixes gradients, and not the module (it holds the trained arena)
        for refused in (lambda: sep.adam_step(1e-3), lambda: sep.get_output(mix, True), lambda: sep.loss_and_gradients(tg),
                        lambda: sep.backward(tg), lambda: sep.ema_update(0.5), lambda: sep.module()(mix),
                        lambda: sep.ema_weights().__enter__()):
            with pytest.raises(RuntimeError, match="inside ema_weights"):
                refused()
    assert sep.params.data_ptr() == p_ptr and sep.ema.data_ptr() == e_ptr
    fresh = UnetAudioSeparator(PLANS[kind](), device="cuda:0")
    fresh.load_variables(sep.ema_variables())
    want = torch.stack(list(fresh.get_output(mix, False).values()))
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(_bits(got_track), _bits(_track_estimates(fresh, cfg)))
    assert not torch.equal(_bits(got), _bits(before))                                            # the two weight sets differ
    after = torch.stack(list(sep.get_output(mix, False).values()))
    assert torch.equal(_bits(after), _bits(before))
    assert torch.equal(_bits(_track_estimates(sep, cfg)), _bits(before_track))
    with pytest.raises(KeyError):
        with sep.ema_weights():
            sep.get_output(mix, False)
            raise KeyError("inside")
    assert sep.params.data_ptr() == p_ptr
    assert torch.equal(_bits(torch.stack(list(sep.get_output(mix, False).values()))), _bits(before))
    # refused inside a training forward and with gradients pending; allowed again after the step
    sep.get_output(mix, True)
    with pytest.raises(RuntimeError, match="training forward"):
        with sep.ema_weights():
            pass
    sep.loss_and_gradients(tg)
    with pytest.raises(RuntimeError, match="pending"):
        with sep.ema_weights():
            pass
    with pytest.raises(ValueError):
        sep.adam_step(1e-3, weight_decay=-1.0)                        # a refused step leaves them pending
    with pytest.raises(RuntimeError, match="pending"):
        with sep.ema_weights():
            pass
    sep.adam_step(1e-3, ema_decay=0.5)
    with sep.ema_weights():
        pass
    # gradients that are only inspected: discard_gradients() lets the block in again, and asks for a new forward
    sep.get_output(mix, True)
    sep.loss_and_gradients(tg)
    sep.grad_norm()
    sep.discard_gradients()
    with sep.ema_weights():
        pass
    with pytest.raises(RuntimeError, match="get_output"):
        sep.loss_and_gradients(tg)


def test_separator_surface(lib):
    """adam_step's new arguments against the raw entry; decay_variables; ema_update; the autograd module's ema_update."""
    sep, mix, tg = _trained_with_ema("small", steps=1)
    names = [n for n, _, _ in sep._active.tensors]
    assert list(sep.decay_mask(None)) == [1 if n.endswith("kernel") else 0 for n in names]
    with pytest.raises(KeyError):
        sep.adam_step(1e-3, weight_decay=0.1, decay_variables=["separator/nope"])
    with pytest.raises(ValueError):
        sep.adam_step(1e-3, weight_decay=-0.1)
    with pytest.raises(ValueError):
        sep.adam_step(1e-3, ema_decay=1.0)
    sep.get_output(mix, True)
    sep.loss_and_gradients(tg)
    a = object.__new__(Arenas)
    a.p, a.g, a.m, a.v, a.ema = (t.clone() for t in (sep.params, sep.grads, sep.adam_m, sep.adam_v, sep.ema))
    step = sep.global_step + 1
    dec = sep.select_mask([names[0]])
    norm = sep.adam_step(1e-3, grad_scale=0.5, weight_decay=0.1, decay_variables=[names[0]], ema_decay=0.9, ema_warmup=True,
                         clip_norm=1e-2, skip_nonfinite=True)
    ws, cnt = _ws(lib, sep)
    _optim(lib, sep, a, step, 1e-3, 0.5, wd=0.1, ema_decay=0.9, clip=1e-2, flags=3, dec=dec, ws=ws, skipped=cnt)
    torch.cuda.synchronize()
    _equal((sep.params, sep.adam_m, sep.adam_v, sep.ema), a.four(), "adam_step")
    assert sep.global_step == step and torch.equal(_bits(norm), _bits(ws[len(names)]))
    want = onp.ema32(sep.ema.cpu().numpy(), sep.params.cpu().numpy(), 0.9, sep.global_step, False)
    sep.ema_update(0.9)
    assert np.array_equal(sep.ema.cpu().numpy().view(np.int32), want.view(np.int32))
    # the autograd module: torch's optimizer, then the EMA line
    fresh = UnetAudioSeparator(PLANS["small"](), device="cuda:0")
    net = fresh.module()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-2)
    e0 = fresh._ensure_ema().cpu().numpy().copy()                      # the EMA starts at the weights it is created from
    net(mix).square().mean().backward()
    opt.step()
    with pytest.raises(ValueError, match="step"):
        net.ema_update(0.9, warmup=True)                              # the module keeps no counter: warm-up needs the caller's
    net.ema_update(0.9, warmup=True, step=1)
    torch.cuda.synchronize()
    want = onp.ema32(e0, fresh.params.detach().cpu().numpy(), 0.9, 1, True)
    assert np.array_equal(fresh.ema.cpu().numpy().view(np.int32), want.view(np.int32))
    assert sorted(fresh.ema_variables()) == sorted(names)


# ------------------------------------------------------------------------------------------------ 6. Trainer
def _train_cfg(tmp, **kw):
    base = dict(num_layers=2, num_initial_filters=8, filter_size=5, input_filter_size=5, num_frames=24, batch_size=4, epoch_it=2,
                model_base_dir=os.path.join(tmp, "ckpt"), log_dir=os.path.join(tmp, "logs"), init_sup_sep_lr=1e-3)
    base.update(kw)
    return wun.get_config("full", **base)


OPT = {"weight_decay": 0.05, "ema_decay": 0.9, "ema_warmup": True}
SCHED = {"warmup_steps": 2, "kind": "cosine", "total_steps": 6, "min_factor": 0.1}


def _batch(cfg, tr):
    return training.synthetic_source(cfg, tr.batch, tr.t_in, tr.t_out, tr.device, seed=7)()


def _four(sep):
    return sep.params, sep.adam_m, sep.adam_v, sep.ema


@pytest.mark.parametrize("accum", [1, 2])
def test_trainer_equals_the_hand_sequence(lib, tmp_path, accum):
    """4 steps with optimizer + lr_schedule (warm-up 2, then cosine) equal the same 4 steps made by hand through
    sep.adam_step with lr_factor's values, bit for bit; with grad_accum_steps = 2 and clipping on as well."""
    cfg = _train_cfg(str(tmp_path))
    extra = dict(grad_accum_steps=2, clip_grad_norm=1e-3, skip_nonfinite=True) if accum == 2 else {}
    tr = training.Trainer(cfg, optimizer=OPT, lr_schedule=SCHED, **extra)
    mix, tg = _batch(cfg, tr)
    lrs = []
    for _ in range(4):
        tr.step(mix, tg)
        lrs.append(tr.last_lr)
    want = [float(np.float32(cfg["init_sup_sep_lr"] * onp.lr_factor(SCHED, s))) for s in range(4)]
    assert lrs == want and len(set(lrs)) >= 3
    sep = UnetAudioSeparator(tr.cfg, device="cuda:0", seed=1337)
    b = tr.batch // accum
    for s in range(4):
        for i in range(accum):
            sep.get_output(mix[i * b:(i + 1) * b], True)
            sep.loss_and_gradients(tg[:, i * b:(i + 1) * b], accumulate=i > 0)
        kw = dict(clip_norm=1e-3, skip_nonfinite=True) if accum == 2 else {}
        sep.adam_step(want[s], grad_scale=1.0 / accum, **OPT, **kw)
    torch.cuda.synchronize()
    _equal(_four(tr.sep), _four(sep), "trainer")
    assert tr.sep.global_step == 4 and not torch.equal(_bits(tr.sep.ema), _bits(tr.sep.params))


def test_train_logs_lr_and_checkpoints_the_ema_only_when_set(lib, tmp_path, monkeypatch):
    monkeypatch.setenv("WUN_NO_TUNE", "1")
    tmp = str(tmp_path)
    cfg = _train_cfg(tmp)
    plain_path = training.train(cfg, "plain")
    opt_path = training.train(dict(cfg, optimizer=OPT, lr_schedule=SCHED), "opt")
    only_sched = training.train(dict(cfg, lr_schedule={"warmup_steps": 4}), "sched")
    plain = [json.loads(l) for l in open(os.path.join(tmp, "logs", "plain", "train.jsonl"))]
    opt = [json.loads(l) for l in open(os.path.join(tmp, "logs", "opt", "train.jsonl"))]
    sched = [json.loads(l) for l in open(os.path.join(tmp, "logs", "sched", "train.jsonl"))]
    assert len(plain) == len(opt) == len(sched) == 2
    assert all(sorted(r) == ["elapsed_s", "global_step", "sep_loss"] for r in plain)             # today's log lines
    assert [r["lr"] for r in opt] == [training.scheduled_lr(1e-3, SCHED, s) for s in (0, 1)]
    assert [r["lr"] for r in sched] == [float(np.float32(1e-3 * 0.25)), float(np.float32(1e-3 * 0.5))]
    names = [n for n, _, _ in UnetAudioSeparator(cfg).variable_table()]
    assert sorted(np.load(plain_path).files) == sorted(names + ["adam_m", "adam_v", "global_step"])   # today's entries
    assert sorted(np.load(only_sched).files) == sorted(names + ["adam_m", "adam_v", "global_step"])
    assert sorted(np.load(opt_path).files) == sorted(names + ["adam_m", "adam_v", "global_step"] + ["ema/" + n for n in names])
    # resuming that checkpoint in a run that keeps no EMA: the EMA is dropped with a warning, not carried along stale
    with pytest.warns(RuntimeWarning, match="EMA"):
        resumed = training.train(cfg, "resumed", load_model=opt_path)
    assert sorted(np.load(resumed).files) == sorted(names + ["adam_m", "adam_v", "global_step"])
    assert int(np.load(resumed)["global_step"]) == 4


# ------------------------------------------------------------------------------------------------ 7. checkpoints
@pytest.mark.parametrize("fmt", ["npz", "tf"])
def test_checkpoint_round_trip_and_resume(lib, tmp_path, fmt):
    """Round trip with the EMA's bits; 2 steps, save, load, 2 more = 4 straight steps bit for bit, ema included (the schedule
    is keyed on the restored global_step); a checkpoint without an EMA starts the EMA from its variables."""
    cfg = _train_cfg(str(tmp_path))
    straight = training.Trainer(cfg, optimizer=OPT, lr_schedule=SCHED)
    mix, tg = _batch(cfg, straight)
    for _ in range(4):
        straight.step(mix, tg)
    first = training.Trainer(cfg, optimizer=OPT, lr_schedule=SCHED)
    for _ in range(2):
        first.step(mix, tg)
    path = os.path.join(str(tmp_path), "two.npz" if fmt == "npz" else "two-2")
    path = checkpoint.save_checkpoint(first.sep, path, fmt)
    second = training.Trainer(cfg, optimizer=OPT, lr_schedule=SCHED)
    second.sep.ema.fill_(3.0)
    assert checkpoint.load_checkpoint(second.sep, path) == 2
    _equal(_four(second.sep), _four(first.sep), "round trip")
    for _ in range(2):
        second.step(mix, tg)
    torch.cuda.synchronize()
    _equal(_four(second.sep), _four(straight.sep), "resumed")
    assert second.last_lr == straight.last_lr
    # no EMA in the file: the configured EMA starts from the restored variables
    plain = training.Trainer(cfg)
    plain.step(mix, tg)
    p2 = checkpoint.save_checkpoint(plain.sep, os.path.join(str(tmp_path), "plain.npz" if fmt == "npz" else "plain-1"), fmt)
    third = training.Trainer(cfg, optimizer=OPT)
    third.sep.ema.fill_(3.0)
    checkpoint.load_checkpoint(third.sep, p2)
    assert torch.equal(_bits(third.sep.ema), _bits(plain.sep.params)) and torch.equal(_bits(third.sep.params), _bits(plain.sep.params))


# ------------------------------------------------------------------------------------------------ 8. validation, CLI
def _tracks(cfg, lengths, seed):
    from wave_u_net_amd import datasets
    rng = np.random.default_rng(seed)
    return [datasets.make_track({k: (rng.uniform(-0.4, 0.4, (n, 2))).astype(np.float32) for k in cfg["source_names"]}, cfg)
            for n in lengths]


def test_validation_scores_the_ema_weights(lib, tmp_path):
    cfg = _train_cfg(str(tmp_path), num_snippets_per_track=4, cache_size=4)
    tr = training.Trainer(cfg, optimizer={"ema_decay": 0.5})
    mix, tg = _batch(cfg, tr)
    tr.lr = 2e-2                                                       # a few steps at a large lr: two clearly different weight sets
    for _ in range(3):
        tr.step(mix, tg)
    path = checkpoint.save_checkpoint(tr.sep, os.path.join(str(tmp_path), "v.npz"))
    tracks = _tracks(cfg, [500, 620], 3)
    ema_cfg = dict(cfg, optimizer={"ema_decay": 0.5, "eval_with_ema": True})
    trained = validation.test(cfg, "valid", "a", path, tracks=tracks)
    with_ema = validation.test(ema_cfg, "valid", "b", path, tracks=tracks)
    holder = UnetAudioSeparator(cfg, device="cuda:0")
    holder.load_variables(tr.sep.ema_variables())
    want = validation.test(cfg, "valid", "c", None, tracks=tracks, separator=holder)
    assert with_ema == want and with_ema != trained
    plain = checkpoint.save_checkpoint(training.Trainer(cfg).sep, os.path.join(str(tmp_path), "noema.npz"))
    with pytest.raises(RuntimeError, match="no EMA"):
        validation.test(ema_cfg, "valid", "d", plain, tracks=tracks)


def test_cli_predict_with_the_ema_weights(lib, tmp_path):
    """`predict ... weights=ema` as a child process: the estimates are those of a separator holding the EMA values."""
    from scipy.io import wavfile
    from wave_u_net_amd import evaluate
    tmp = str(tmp_path)
    over = dict(num_layers=2, num_initial_filters=8, filter_size=5, input_filter_size=5, num_frames=24, expected_sr=22050)
    cfg = wun.get_config("full", **over)
    tr = training.Trainer(dict(cfg, batch_size=4), optimizer={"ema_decay": 0.5})
    mix, tg = _batch(cfg, tr)
    tr.lr = 2e-2
    for _ in range(3):
        tr.step(mix, tg)
    path = checkpoint.save_checkpoint(tr.sep, os.path.join(tmp, "cli.npz"))
    rng = np.random.default_rng(4)
    inp = os.path.join(tmp, "song.wav")
    wavfile.write(inp, 22050, (rng.uniform(-0.5, 0.5, (1500, 2)) * 32767).astype(np.int16))
    args = ["model_config.%s=%r" % kv for kv in over.items()]
    for out, extra in (("out_ema", ["weights=ema"]), ("out_trained", [])):
        r = subprocess.run([sys.executable, "-m", "wave_u_net_amd", "predict", "with", "cfg.full", "model_path=" + path,
                            "input_path=" + inp, "output_path=" + os.path.join(tmp, out)] + args + extra,
                           capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
    holder = UnetAudioSeparator(cfg, device="cuda:0")
    holder.load_variables(tr.sep.ema_variables())
    want = evaluate.produce_source_estimates(cfg, None, inp, os.path.join(tmp, "want"), separator=holder)
    differs = False
    for name in cfg["source_names"]:
        a = wavfile.read(os.path.join(tmp, "out_ema", "song.wav_" + name + ".wav"))[1]
        b = wavfile.read(os.path.join(tmp, "out_trained", "song.wav_" + name + ".wav"))[1]
        assert np.array_equal(a, np.asarray(want[name], np.float32)), name
        differs = differs or not np.array_equal(a, b)
    assert differs
    with pytest.raises(RuntimeError, match="no EMA"):
        evaluate.produce_source_estimates(cfg, None, inp, os.path.join(tmp, "x"), separator=UnetAudioSeparator(cfg, device="cuda:0"),
                                          weights="ema")
