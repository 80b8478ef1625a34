"""The training step under every environment switch of the library (tests/_switches.py: one row per name
wun_switches_from_env reads) and under the serial schedule -- run with -m gpu on an MI355X.

Plan tier.  A RUN is get_output(mix, True), the upstream gradient of test_gpu_backward's loss AT THE DEFAULT RUN'S OUTPUTS,
backward(dout, input_grad=True) into an arena filled with NaN, synchronize; it keeps the stacked outputs, the whole gradient
arena and d_mix.  Every switched plan is a fresh separator built with the switch in the environment (switches are read once
per plan) and is compared with the default plan of the same case, which runs once per case:

  schedule          outputs, the gradient arena and d_mix bit for bit.  WUN_SINGLE_STREAM issues the same kernels with the same
                    arguments in issue order on one stream: it is the reference the three-stream schedule (ordered only by
                    stream_dep events) never had.  No kernel uses atomics and no tile choice depends on the stream, so a
                    difference is a missing edge.  Also: a step between wun_profile_begin / _end (one stream as well), and an
                    accumulating and a decoder-only backward under the serial schedule.
  wgrad-only        outputs and d_mix bit for bit; every gradient tensor within TOL (test_gpu_dedup.py: same operands, fp32
                    summation order) of the default's and, on fp32 plans, within GRAD_TOL_PINNED of the float64 oracle on the
                    device's LeakyReLU branches (the forward bits are equal: one oracle per case).  A bf16 plan's gradients
                    carry its operand rounding (1e-2 of the float64 oracle's): there the default plan is the reference, and the
                    float64 comparison of the switched kernel is the operator tier's, on bf16 dz planes.
  forward-touching  WUN_NO_DMA: bit for bit (the register-staged instantiation of the same tile).  The others: the float64
                    oracle on this run's own branches under GRAD_TOL_PINNED (fp32), the bounds of test_gpu_bf16.py's step
                    (bf16: its _step runs under the switch); whether the bits equalled the default's is recorded.

What shows that a switch took effect comes from a profiled step of the same plan (wun_profile_end's per-launch list,
WUN_PROFILE_DETAIL=1); the kinds are described in tests/_switches.py.  A case whose default step does not launch the switch's
target shows nothing either way; the last plan-tier test asserts that every row showed its effect on some case.

Operator tier: the kernel paths only a switch reaches, through the single-operator entries (they read the environment on
every call) against the float64 references the project has: wgrad_win_kernel at every unit length, narrow_wgrad_kernel's
LDS-staged form on the shapes the streaming form normally takes, the split cap of the narrow kernels, the bf16 conv tile
height under the LDS cap, and the refusal of in-workgroup split-K tiles."""
import ctypes as C
import json
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _switches as S
import _wgrad_np as W
from _observed import record
from oracle import shapes, waveunet_torch as wt
from oracle.golden_params import GOLDEN_CASES, golden_params
import test_gpu_wgrad_ops as WG
from test_gpu_backward import BF16_CASES, _mix_check, _oracle_custom, _setup, _setup_bf16, _upstream
from test_gpu_backward_select import SENTINEL, _pattern
from test_gpu_bf16 import OP_TOL as BF16_OP_TOL, _bf16_round, _step as bf16_step_within_its_bounds
from test_gpu_dedup import TOL
from test_gpu_parity import GRAD_TOL_PINNED, _gpu_pins, _grad_check
from test_gpu_variants import OP_TOL as CONV_OP_TOL, RETIRED_VARIANTS, _conv64
from test_gpu_wgrad_ops import OP_TOL, UNSUPPORTED, Job

import wave_u_net_amd as wun
from wave_u_net_amd import _lib
from wave_u_net_amd.separator import UnetAudioSeparator

pytestmark = pytest.mark.gpu

CASES = {c.key: c for c in S.CASES}
_DEFAULT = {}            # case key -> Default
_SHOWN = {}              # (switch, value) -> {case key: True / None}: evidence per case, for the coverage test
# the one (switch, value) whose effect no plan of the suite can show: see its evidence function
PLAN_SILENT = {("WUN_WIN_TK", "128")}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


@pytest.fixture(autouse=True)
def _leave_the_wgrad_ops_coverage_alone():
    """Job (test_gpu_wgrad_ops.py) notes every launch form in that module's coverage table: this file's launches must not
    count towards the coverage that file asserts for its own cases."""
    saved = {f: set(s) for f, s in WG._RAN.items()}
    yield
    for f, s in saved.items():
        WG._RAN[f] = s


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _environment(monkeypatch, env):
    for k in S.names():
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _setup_frames(case):
    """test_gpu_backward._setup at another length (fp32 golden cases)."""
    g = GOLDEN_CASES[case.golden]
    ocfg = shapes.finalize_config(dict(shapes.BASE_MODEL_CONFIG, **g["cfg"]))
    params = golden_params(ocfg, g["seed"])
    sep = UnetAudioSeparator(wun.get_config("baseline", **g["cfg"]), device="cuda:0")
    i, o = shapes.get_padding(ocfg, [case.batch, case.frames, 0])
    mix, targets = wt.synthetic_batch(ocfg, case.batch, i[1], o[1], seed=g["seed"] + 100)
    sep._plan(case.batch, i[1]); sep._active = sep._plans[(case.batch, i[1])]
    sep.load_variables(params)
    tg = torch.stack([torch.from_numpy(targets[n]) for n in ocfg["source_names"]]).cuda()
    return sep, ocfg, params, torch.from_numpy(mix).cuda(), tg


class Run(object):
    """One plan built under `env` and one run on it."""

    def __init__(self, case, env, monkeypatch, dout=None, want_pins=False):
        _environment(monkeypatch, env)
        if case.frames is not None:
            self.sep, self.ocfg, self.params, self.mix, self.tg = _setup_frames(case)
        else:
            setup = _setup if case.mode == "fp32" else _setup_bf16
            self.sep, self.ocfg, self.params, self.mix, self.tg = setup(case.golden, B=case.batch)
        self.case = case
        sep = self.sep
        outs = sep.get_output(self.mix, True)
        self.dout = dout if dout is not None else _upstream(outs, self.ocfg["source_names"], self.tg).contiguous()
        self.pins = _gpu_pins(sep, self.ocfg) if want_pins else None
        self.outs, self.grads, self.d_mix = self.step()

    def step(self):
        sep = self.sep
        sep.get_output(self.mix, True)
        outs = sep._outs[sep._last_key].clone()
        sep.grads.fill_(float("nan"))
        d_mix = sep.backward(self.dout, input_grad=True)
        torch.cuda.synchronize()
        return outs, sep.grads.clone(), d_mix.clone()

    def profiled_step(self, lib, monkeypatch):
        """-> ([(kernel name, tag)] in issue order, (outs, grads, d_mix)) of one step between the profile brackets."""
        monkeypatch.setenv("WUN_PROFILE_DETAIL", "1")
        buf = C.create_string_buffer(1 << 22)
        _lib.check(lib.wun_profile_begin())
        try:
            res = self.step()
        finally:
            rc = lib.wun_profile_end(buf, len(buf))
        _lib.check(rc)
        return [(k["name"], k["tag"]) for k in json.loads(buf.value.decode())["launches"]], res

    def tensors(self, arena):
        for name, off, shp in self.sep._active.tensors:
            yield name, arena[off:off + int(np.prod(shp))]


class Default(object):
    def __init__(self, lib, case, monkeypatch):
        self.run = Run(case, {}, monkeypatch, want_pins=case.mode == "fp32")
        self.launches, self.profiled = self.run.profiled_step(lib, monkeypatch)
        assert torch.isfinite(self.run.outs).all() and torch.isfinite(self.run.d_mix).all()
        for name, g in self.run.tensors(self.run.grads):
            assert torch.isfinite(g).all() and g.abs().max().item() > 0, name
        self._oracle = None

    def oracle(self, pins=None):
        """(tp, parameter gradients, d_mix) of the float64 oracle on `pins` (None: the default run's own, cached)."""
        r = self.run
        if pins is not None:
            return _oracle_custom(r.ocfg, r.params, r.mix, r.tg, pins)
        if self._oracle is None:
            self._oracle = _oracle_custom(r.ocfg, r.params, r.mix, r.tg, r.pins)
        return self._oracle


def _default(lib, case, monkeypatch):
    if case.key not in _DEFAULT:
        _DEFAULT[case.key] = Default(lib, case, monkeypatch)
    return _DEFAULT[case.key]


def _assert_equal_run(got, ref, tag):
    """(outs, grads, d_mix) bit for bit, naming the first tensor that differs."""
    assert _same_bits(got[0], ref[0]), (tag, "outputs differ", int((_bits(got[0]) != _bits(ref[0])).sum()))
    assert _same_bits(got[2], ref[2]), (tag, "d_mix differs", int((_bits(got[2]) != _bits(ref[2])).sum()))
    return _assert_equal_arena(got[1], ref[1], tag)


def _assert_equal_arena(got, ref, tag, run=None):
    if not _same_bits(got, ref):
        bad = int((_bits(got) != _bits(ref)).sum())
        names = []
        if run is not None:
            names = [n for (n, a), (_, b) in zip(run.tensors(got), run.tensors(ref)) if not _same_bits(a, b)]
        raise AssertionError((tag, "gradient arena differs", bad, names[:8]))


def _within_summation_order(run, ref, tag):
    """Every gradient tensor within TOL x max|default| of the default plan's.  -> (worst ratio, tensors that differ in bits)."""
    worst, differ = 0.0, 0
    for (name, g), (_, d) in zip(run.tensors(run.grads), run.tensors(ref.grads)):
        assert torch.isfinite(g).all(), (tag, name)
        scale = d.abs().max().item()
        err = (g.double() - d.double()).abs().max().item()
        assert err <= TOL * scale, (tag, name, err, scale)
        worst = max(worst, err / max(scale, 1e-30))
        differ += 0 if _same_bits(g, d) else 1
    return worst, differ


# ------------------------------------------------------------------------------------------------------------ evidence
def _narrow(launches):
    return [(n, t) for n, t in launches if n.startswith("narrow_wgrad_kernel")]


def _window(launches):
    return [(n, t) for n, t in launches if n.startswith("wgrad_win_kernel") or n.startswith("wgrad_win_acc_kernel")]


def _field(tag, key):
    return int(re.search(r"\b%s=(\d+)" % key, tag).group(1))


def _streaming(tag):
    return tag.endswith(" stream")


def ev_no_window(dflt, got, value, case):
    if not _window(dflt):
        return None
    assert not _window(got), _window(got)
    return True


def ev_no_narrow(dflt, got, value, case):
    if not _narrow(dflt):
        return None
    assert not _narrow(got), _narrow(got)
    return True


def ev_fewer_narrow(dflt, got, value, case):
    assert 0 < len(_narrow(got)) < len(_narrow(dflt)), (_narrow(got), _narrow(dflt))
    return True


def ev_lds_form(dflt, got, value, case):
    was = [t for _, t in _narrow(dflt) if _streaming(t)]
    if not was:
        return None
    now = [t for _, t in _narrow(got)]
    assert not [t for t in now if _streaming(t)], now
    # the same launches, in the same order, the streaming ones now without the mark (the LDS form's tag has no C1 of its own)
    assert len(now) == len(_narrow(dflt)), (now, _narrow(dflt))
    for (_, a), b in zip(_narrow(dflt), now):
        if _streaming(a):
            assert a[:-len(" stream")] == b, (a, b)
    return True


def ev_nsplit_tag(dflt, got, value, case):
    cap = int(value)
    now, was = [_field(t, "nsplit") for _, t in _narrow(got)], [_field(t, "nsplit") for _, t in _narrow(dflt)]
    assert now and len(now) == len(was) and all(1 <= n <= cap for n in now), (cap, now)
    assert all(n == min(w, cap) for n, w in zip(now, was)), (cap, now, was)      # (the default's count is its unit count here)
    return True if now != was else None


def ev_tk_tag(dflt, got, value, case):
    """16 is the floor: every launch.  32: every launch but rows of <= 16 positions (wgrad_win_geom halves TK while TK / 2 >= Tq).
    128: a unit of 128 positions needs S * 127 + K >= 132 floats per staged row, and the one-column-group workgroup every
    untuned launch uses stages 64 (K = 5) or 24 (K = 15) rows within 3 x 256 16-byte loads = 3072 floats: at most 128 per
    row.  So the request falls back to 64 in every launch of an untuned plan and the tags equal the default's; tk=128 runs
    with two column groups per workgroup only (a tuned choice): the operator tier forces that geometry."""
    now, was = _window(got), _window(dflt)
    if not was:
        return None
    assert len(now) == len(was)
    req = int(value)
    if req == 128:
        assert [t for _, t in now] == [t for _, t in was], (now, was)
        return None
    for _, t in now:
        assert _field(t, "tk") == (req if _field(t, "T") > req // 2 else 16), t
    return True if [t for _, t in now] != [t for _, t in was] else None


def ev_no_dma_name(dflt, got, value, case):
    if not [n for n, _ in dflt if ", dma" in n]:
        return None
    assert not [n for n, _ in got if ", dma" in n]
    return True


def ev_launch_list(dflt, got, value, case):
    return True if sorted(got) != sorted(dflt) else None


def ev_default_bits(dflt, got, value, case):
    assert got == dflt
    return True


EVIDENCE = {"no_window": ev_no_window, "no_narrow": ev_no_narrow, "fewer_narrow": ev_fewer_narrow, "lds_form": ev_lds_form,
            "nsplit_tag": ev_nsplit_tag, "tk_tag": ev_tk_tag, "no_dma_name": ev_no_dma_name, "launch_list": ev_launch_list,
            "default_bits": ev_default_bits, "spelling": None, "operator": None}


def _evidence(lib, row, value, case, run, dflt, monkeypatch):
    fn = EVIDENCE[row.evidence]
    if fn is None:
        return
    launches, res = run.profiled_step(lib, monkeypatch)
    # (the profiled step of the switched plan: one stream, same kernels -- the run's bits again)
    _assert_equal_run(res, (run.outs, run.grads, run.d_mix), "profiled step of the switched plan")
    shown = fn(dflt.launches, launches, value, case)
    _SHOWN.setdefault((row.name, value), {})[case.key] = shown


def _ids(matrix):
    return ["%s=%s-%s" % (r.name, v, c.key) for r, v, c in matrix]


# ------------------------------------------------------------------------------------------------- plan tier: schedule
SCHEDULE_MATRIX = S.plan_matrix(S.SCHEDULE)


@pytest.mark.parametrize("entry", SCHEDULE_MATRIX, ids=_ids(SCHEDULE_MATRIX))
def test_schedule_switch_leaves_every_bit(lib, entry, monkeypatch):
    row, value, case = entry
    dflt = _default(lib, case, monkeypatch)
    run = Run(case, {row.name: value}, monkeypatch, dout=dflt.run.dout)
    tag = "%s=%s %s" % (row.name, value, case.key)
    assert _same_bits(run.outs, dflt.run.outs), (tag, "outputs differ", int((_bits(run.outs) != _bits(dflt.run.outs)).sum()))
    assert _same_bits(run.d_mix, dflt.run.d_mix), (tag, "d_mix differs", int((_bits(run.d_mix) != _bits(dflt.run.d_mix)).sum()))
    _assert_equal_arena(run.grads, dflt.run.grads, tag, run)
    record("switches_schedule", tag + ": floats that differ", 0.0, 0.0)


@pytest.mark.parametrize("key", sorted(CASES))
def test_profiled_step_leaves_every_bit(lib, key, monkeypatch):
    """Between wun_profile_begin and wun_profile_end the step runs on one stream with an event pair around every launch."""
    dflt = _default(lib, CASES[key], monkeypatch)
    r = dflt.run
    assert dflt.launches, "the profile lists no launch"
    assert _same_bits(dflt.profiled[0], r.outs) and _same_bits(dflt.profiled[2], r.d_mix), key
    _assert_equal_arena(dflt.profiled[1], r.grads, S.PROFILED_STEP + " " + key, r)
    record("switches_schedule", "%s %s: floats that differ" % (S.PROFILED_STEP, key), 0.0, 0.0)


def _accumulate_and_frozen(run):
    """An accumulating backward onto a pre-filled arena, then a decoder-only backward into a sentinel-filled one (the pattern of
    test_gpu_backward_select.py), on the run's forward pass.  -> (arena, d_mix, arena, d_mix)."""
    sep = run.sep
    sep.get_output(run.mix, True)
    gen = torch.Generator(device="cpu").manual_seed(7)
    sep.grads.copy_((torch.randn(sep.grads.numel(), generator=gen) * 0.01).cuda())
    dm_acc = sep.backward(run.dout, input_grad=True, accumulate=True)
    torch.cuda.synchronize()
    acc = sep.grads.clone()
    names = [sep._active.tensors[k][0] for k in np.flatnonzero(_pattern(sep, "decoder"))]
    _bits(sep.grads).fill_(SENTINEL)
    dm_fro = sep.backward(run.dout, input_grad=True, variables=names)
    torch.cuda.synchronize()
    return acc, dm_acc.clone(), sep.grads.clone(), dm_fro.clone()


EXTRA = [(name, "1", key) for name, keys in sorted(S.SCHEDULE_EXTRA.items()) for key in keys]


@pytest.mark.parametrize("entry", EXTRA, ids=["%s=%s-%s" % e for e in EXTRA])
def test_serial_schedule_accumulating_and_frozen_backward(lib, entry, monkeypatch):
    """Both change what the side streams carry: accumulating launches take other instantiations, a frozen encoder skips its
    weight gradients while the input-gradient chain still runs."""
    name, value, key = entry
    case = CASES[key]
    dflt = _default(lib, case, monkeypatch)
    ref = _accumulate_and_frozen(dflt.run)
    run = Run(case, {name: value}, monkeypatch, dout=dflt.run.dout)
    got = _accumulate_and_frozen(run)
    tag = "%s=%s %s" % (name, value, key)
    _assert_equal_arena(got[0], ref[0], tag + " accumulate", run)
    assert _same_bits(got[1], ref[1]) and _same_bits(got[1], dflt.run.d_mix), (tag, "accumulate: d_mix")
    _assert_equal_arena(got[2], ref[2], tag + " decoder only", run)
    assert _same_bits(got[3], ref[3]) and _same_bits(got[3], dflt.run.d_mix), (tag, "decoder only: d_mix")
    kept = _bits(got[2]) == SENTINEL
    assert kept.any() and not kept.all(), "the decoder-only call must write some tensors and leave the others"
    record("switches_schedule", tag + " accumulate + decoder only: floats that differ", 0.0, 0.0)


# ----------------------------------------------------------------------------------------------- plan tier: wgrad-only
WGRAD_MATRIX = S.plan_matrix(S.WGRAD)


@pytest.mark.parametrize("entry", WGRAD_MATRIX, ids=_ids(WGRAD_MATRIX))
def test_wgrad_only_switch(lib, entry, monkeypatch):
    row, value, case = entry
    dflt = _default(lib, case, monkeypatch)
    run = Run(case, {row.name: value}, monkeypatch, dout=dflt.run.dout)
    tag = "%s=%s %s" % (row.name, value, case.key)
    assert _same_bits(run.outs, dflt.run.outs), (tag, "outputs differ")
    assert _same_bits(run.d_mix, dflt.run.d_mix), (tag, "d_mix differs")
    worst, differ = _within_summation_order(run, dflt.run, tag)
    record("switches_wgrad_only", tag + ": vs the default plan", worst, TOL)
    record("switches_wgrad_only", tag + ": gradient tensors whose bits differ from the default's", differ, len(run.sep._active.tensors))
    if case.mode == "fp32":
        tp, ograds, _ = dflt.oracle()
        w = _grad_check(run.sep, tp, ograds, tol=GRAD_TOL_PINNED, tag="switches " + tag)
        record("switches_wgrad_only", tag + ": vs the float64 oracle", w, GRAD_TOL_PINNED)
    _evidence(lib, row, value, case, run, dflt, monkeypatch)


# ----------------------------------------------------------------------------------------- plan tier: forward-touching
FORWARD_MATRIX = S.plan_matrix(S.FORWARD)


def _same_pins(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k][0], b[k][0]) and torch.equal(a[k][1], b[k][1]) for k in a)


@pytest.mark.parametrize("entry", FORWARD_MATRIX, ids=_ids(FORWARD_MATRIX))
def test_forward_touching_switch(lib, entry, monkeypatch):
    row, value, case = entry
    dflt = _default(lib, case, monkeypatch)
    fp32 = case.mode == "fp32"
    run = Run(case, {row.name: value}, monkeypatch, dout=dflt.run.dout, want_pins=fp32)
    tag = "%s=%s %s" % (row.name, value, case.key)
    equal = _same_bits(run.outs, dflt.run.outs) and _same_bits(run.d_mix, dflt.run.d_mix) and _same_bits(run.grads, dflt.run.grads)
    record("switches_forward_touching", tag + ": bits equal the default plan's (1 = yes)", float(equal), 1.0)
    if row.name in S.FORWARD_EQUAL:
        _assert_equal_run((run.outs, run.grads, run.d_mix), (dflt.run.outs, dflt.run.grads, dflt.run.d_mix), tag)
    elif fp32:
        # pins from this run's own forward pass; the oracle of the default run when they are the same branches
        tp, ograds, odmix = dflt.oracle() if _same_pins(run.pins, dflt.run.pins) else dflt.oracle(run.pins)
        w = _grad_check(run.sep, tp, ograds, tol=GRAD_TOL_PINNED, tag="switches " + tag)
        record("switches_forward_touching", tag + ": vs the float64 oracle", w, GRAD_TOL_PINNED)
        _mix_check(run.d_mix, odmix, "switches " + tag)
    else:
        assert torch.isfinite(run.outs).all() and torch.isfinite(run.d_mix).all()
        assert all(torch.isfinite(g).all() for _, g in run.tensors(run.grads))
    _evidence(lib, row, value, case, run, dflt, monkeypatch)
    if not fp32 and row.name not in S.FORWARD_EQUAL:
        # the bf16 bounds of this case, as test_gpu_bf16.py applies them: its step (outputs, loss, every gradient against the
        # float64 oracle and the layer-by-layer emulation) with its batch of 3 and its seeds, on a plan built under the switch
        _environment(monkeypatch, {row.name: value})
        name, over = BF16_CASES[case.golden]
        g = GOLDEN_CASES[name]
        cfg_over = dict(g["cfg"], **over)
        ocfg = shapes.finalize_config(dict(shapes.BASE_MODEL_CONFIG, **cfg_over))
        frames = 160 if not ocfg["context"] else g["frames"]
        bf16_step_within_its_bounds(cfg_over, ocfg, golden_params(ocfg, g["seed"]), 3, frames, g["seed"] + 100, "switches " + tag)


# ------------------------------------------------------------------------------------------------ plan tier: parse edges
EDGES = [(n, v, k) for n, v, _ in S.PARSE_EDGES for k in S.PARSE_EDGE_CASES]


@pytest.mark.parametrize("entry", EDGES, ids=["%s=%s-%s" % e for e in EDGES])
def test_value_read_as_unset_gives_the_default_plan(lib, entry, monkeypatch):
    name, value, key = entry
    case = CASES[key]
    dflt = _default(lib, case, monkeypatch)
    run = Run(case, {name: value}, monkeypatch, dout=dflt.run.dout)
    tag = "%s=%s %s" % (name, value, key)
    _assert_equal_run((run.outs, run.grads, run.d_mix), (dflt.run.outs, dflt.run.grads, dflt.run.d_mix), tag)
    launches, _ = run.profiled_step(lib, monkeypatch)
    ev_default_bits(dflt.launches, launches, value, case)
    record("switches_parse_edges", tag + ": floats that differ", 0.0, 0.0)


def test_every_row_showed_its_effect_on_some_case():
    """Runs after the plan tier (file order), over the (switch, value) pairs that ran."""
    silent = []
    for (name, value), per_case in sorted(_SHOWN.items()):
        if (name, value) in PLAN_SILENT:
            assert not any(per_case.values()), (name, value, per_case)
            continue
        applicable = {c.key for c in S.CASES if S.applies(S.row(name), c)}
        if set(per_case) >= applicable and not any(per_case.values()):
            silent.append((name, value, S.row(name).evidence))
    assert not silent, silent
    print("[switches] evidence shown per case:", {"%s=%s" % k: sorted(c for c, s in v.items() if s) for k, v in sorted(_SHOWN.items())})


# ==================================================================================================== operator tier
def _profiled_launches(lib, monkeypatch, fn):
    monkeypatch.setenv("WUN_PROFILE_DETAIL", "1")
    buf = C.create_string_buffer(1 << 20)
    _lib.check(lib.wun_profile_begin())
    try:
        res = fn()
        torch.cuda.synchronize()
    finally:
        rc = lib.wun_profile_end(buf, len(buf))
    _lib.check(rc)
    return res, [(k["name"], k["tag"]) for k in json.loads(buf.value.decode())["launches"]]


# ---- window weight gradients at every unit length ----
# form -> (K, loader, C0, C1, N, forced (column groups per workgroup, column tiles per wave))
WIN_FORMS = {
    "k15_stride1": (15, 0, 8, 0, 16, (0, 0)),
    "k15_deint": (15, 1, 8, 0, 16, (0, 0)),
    "k5": (5, 0, 8, 0, 16, (0, 0)),
    "k5_two_sources": (5, 0, 8, 8, 16, (0, 0)),
    # the only geometry a unit of 128 positions fits: 15 taps at stride 1, two column groups per workgroup (N = 32 has two)
    "k15_stride1_two_groups": (15, 0, 8, 0, 32, (2, 1)),
    "k15_two_sources_two_groups": (15, 0, 8, 8, 32, (2, 1)),
}
WIN_B = 2


def expect_tk(K, loader, groups, request, Tq):
    """The unit length wgrad_win_geom must settle on, from its stated rules: start at the request (64 when unset or not one of
    16 / 32 / 64 / 128); halve while half a unit still holds the row (TK / 2 >= Tq); halve while one staged row of a unit --
    S (TK - 1) + K floats -- exceeds what the workgroup's staging loads carry per row: 3 loads of 16 bytes x 256 threads per
    column group = 3072 floats per group, over 3 row tiles x 8 channels = 24 rows (K = 15) or 4 x 16 = 64 rows (K = 5), i.e.
    128 / 48 floats per row and group.  16 is the floor."""
    tk = request if request in (16, 32, 64, 128) else 64
    while tk > 16 and tk // 2 >= Tq:
        tk //= 2
    per_row = (128 if K == 15 else 48) * max(1, groups)
    while tk > 16 and (2 if loader else 1) * (tk - 1) + K > per_row:
        tk //= 2
    return tk


def _win_cases():
    out = []
    for request in (None, 16, 32, 128):
        t = request or 64
        for form, (K, loader, C0, C1, N, force) in WIN_FORMS.items():
            rows = tuple((Tq, expect_tk(K, loader, force[0], request, Tq)) for Tq in (t // 2, t - 1, t, t + 1, 2 * t + 3))
            out.append((request, form, rows))
    return out


WIN_CASES = _win_cases()


def _win_shape(form, Tq):
    K, loader, C0, C1, N, _ = WIN_FORMS[form]
    Tin = 2 * (Tq - 1) + K if loader else Tq + K - 1
    return W.make_shape(WIN_B, C0, C1, N, K, [dict(loader=loader, x0_off=3, x1_off=2 if C1 else 0, Tin=Tin, Tq=Tq)])


@pytest.mark.parametrize("case", WIN_CASES, ids=["tk%s-%s-Tq,tk=%s" % (c[0] or "unset", c[1], "/".join("%d,%d" % r for r in c[2])) for c in WIN_CASES])
def test_window_wgrad_at_every_unit_length(lib, case, monkeypatch):
    """wgrad_win_kernel through wun_op_wgrad_ex under WUN_WIN_TK, rows of TK / 2, TK - 1, TK, TK + 1 and 2 TK + 3 positions:
    the float64 reference at OP_TOL, the accumulate contract and the guard bands of test_gpu_wgrad_ops.py's Job; the unit
    length from the entry's work-unit count AND from the tk= field of the launches' tags."""
    request, form, rows = case
    _environment(monkeypatch, {} if request is None else {"WUN_WIN_TK": str(request)})
    force = WIN_FORMS[form][5]
    worst, fails = 0.0, []
    for i, (Tq, tk) in enumerate(rows):
        job = Job(lib, _win_shape(form, Tq), W.WIN, seed=2000 + 10 * WIN_CASES.index(case) + i, galign=i & 1)
        d = job.desc((0, 0), 0, force)
        units = lib.wun_op_wgrad_max_units(C.byref(d), 0)
        assert units == WIN_B * ((Tq + tk - 1) // tk), (Tq, tk, units)
        for ns in ((0, 0), (1, 0)):
            r, launches = _profiled_launches(lib, monkeypatch, lambda: job.store_and_accumulate(ns, force))
            assert r is not None, (form, force, "geometry refused")
            err, why, path, splits = r
            if ns[0] == 1:
                assert (path, splits) == (_lib.PATH_WGRAD_DIRECT, 1), (path, splits)
            tags = [t for _, t in _window(launches)]
            assert len(tags) == 2 and all(_field(t, "tk") == tk for t in tags), (Tq, tk, tags)
            worst, fails = max(worst, err), fails + ([(Tq, ns, why)] if why else [])
    WG.finish("switches_window_wgrad_unit_length", "WUN_WIN_TK=%s %s" % (request, form), worst, fails)


def test_window_unit_length_ignores_other_values(lib, monkeypatch):
    """WUN_WIN_TK=48 is none of 16 / 32 / 64 / 128: the default's units."""
    job = Job(lib, _win_shape("k15_stride1", 131), W.WIN, seed=2999)
    units = {}
    for v in (None, "48", "64", "32"):
        _environment(monkeypatch, {} if v is None else {"WUN_WIN_TK": v})
        d = job.desc()
        units[v] = lib.wun_op_wgrad_max_units(C.byref(d), 0)
    assert units[None] == units["48"] == units["64"] == WIN_B * 3 and units["32"] == WIN_B * 5, units


# ---- narrow weight gradients: the LDS-staged form on the streaming form's shapes, the split cap ----
NARROW_ENVS = [("WUN_NO_NARROW_STREAM", "1"), ("WUN_NARROW_SPLITS", "1"), ("WUN_NARROW_SPLITS", "3")]
NARROW_SHAPES = [(Cc, et, K) for Cc in (1, 2) for et in (0, 4) for K in (15, 5)]


def _audio_shape(Cc, K):
    """test_gpu_wgrad_ops.py's audio-input conv (W.audio_shape) with K taps: the stride-2 positions over rows of 5000, then
    300 stride-1 positions at an odd offset, consecutive splits of one partial list."""
    parts = [dict(loader=1, x0_off=0, Tin=5000, Tq=(5000 - K) // 2 + 1), dict(loader=0, x0_off=1001, Tin=300 + K - 1, Tq=300)]
    return W.make_shape(1, Cc, 0, 24, K, parts)


def test_audio_shape_is_the_wgrad_ops_shape():
    assert _audio_shape(2, 15) == W.audio_shape(2)


@pytest.mark.parametrize("shape", NARROW_SHAPES, ids=["C%d et%d K%d" % s for s in NARROW_SHAPES])
@pytest.mark.parametrize("env", NARROW_ENVS, ids=["%s=%s" % e for e in NARROW_ENVS])
def test_narrow_wgrad_under_its_switches(lib, env, shape, monkeypatch):
    Cc, et, K = shape
    job = Job(lib, _audio_shape(Cc, K), W.NARROW, seed=2400 + NARROW_SHAPES.index(shape), et=et)
    # the default: both parts stream, one split per unit (10 + 2 units)
    _environment(monkeypatch, {})
    d = job.desc()
    units = [lib.wun_op_wgrad_max_units(C.byref(d), i) for i in range(2)]
    assert units == [(job.shape["parts"][0]["Tq"] + 255) // 256, 2], units
    r, launches = _profiled_launches(lib, monkeypatch, lambda: job.store_and_accumulate((0, 0)))
    assert r[1] is None and r[3] == sum(units), r
    assert [_streaming(t) for _, t in _narrow(launches)] == [True] * 4, launches            # (2 parts x {store, accumulate})
    _environment(monkeypatch, dict([env]))
    r, launches = _profiled_launches(lib, monkeypatch, lambda: job.store_and_accumulate((0, 0)))
    err, why, path, splits = r
    tags = [t for _, t in _narrow(launches)]
    assert path == _lib.PATH_WGRAD_SPLIT and splits == lib.wun_op_wgrad_last_splits() and len(tags) == 4
    if env[0] == "WUN_NO_NARROW_STREAM":
        assert not any(_streaming(t) for t in tags), tags
        assert splits == sum(units), (splits, units)
    else:
        cap = int(env[1])
        assert all(_streaming(t) for t in tags), tags
        assert splits == sum(min(u, cap) for u in units) and splits < sum(units), (splits, units, cap)
        assert [_field(t, "nsplit") for t in tags] == [min(u, cap) for u in units] * 2, tags
    WG.finish("switches_narrow_wgrad", "%s=%s C%d et%d K%d" % (env + shape), err, [why] if why else [])


def test_narrow_forms_refuse_the_element_types_they_do_not_serve(lib, monkeypatch):
    """The streaming form reads fp32 audio and fp32 or bf16 dz (et in {0, 4}); the LDS-staged form also takes et = 2 (a bf16
    second source, which these one-source shapes do not have).  So et = 2 is refused while the streaming form owns the shape --
    by the host-only scratch query (narrow_wgrad_launch_ok) and by the launch, before any GPU work -- and served under
    WUN_NO_NARROW_STREAM; bf16 audio (et = 1) is refused either way."""
    job = Job(lib, _audio_shape(1, 15), W.NARROW, seed=2500, et=2)
    _environment(monkeypatch, {})
    d = job.desc()
    assert lib.wun_op_wgrad_ex_scratch(C.byref(d)) == UNSUPPORTED
    job.refused(d, UNSUPPORTED)
    _environment(monkeypatch, {"WUN_NO_NARROW_STREAM": "1"})
    assert lib.wun_op_wgrad_ex_scratch(C.byref(d)) > 0
    err, why, path, splits = job.store_and_accumulate((0, 0))
    WG.finish("switches_narrow_wgrad", "WUN_NO_NARROW_STREAM=1 C1 et2 K15", err, [why] if why else [])
    for env in ({}, {"WUN_NO_NARROW_STREAM": "1"}):
        _environment(monkeypatch, env)
        bad = Job(lib, _audio_shape(1, 15), W.NARROW, seed=2501, et=0)
        d = bad.desc()
        d.et = 1
        assert lib.wun_op_wgrad_ex_scratch(C.byref(d)) == UNSUPPORTED
        bad.refused(d, UNSUPPORTED)


# ---- in-workgroup split-K tiles ----
def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_split_k_tiles_are_refused_under_no_k3(lib, monkeypatch):
    """conv_choice_ok: `if (sw.no_k3 || ...) return false`.  (16, 72, 48, 5, 40) is a deep-level shape of test_gpu_variants.py's
    sweep on which forced in-workgroup split-K tiles run and match the float64 conv; under WUN_NO_K3=1 every one of them is
    refused before any GPU work (the output keeps its NaN), WUN_NO_K3=0 refuses nothing, and the dispatcher's own choice is
    not a split-K tile, so the unforced launch runs under the switch."""
    B, Cin, Cout, K, T = 16, 72, 48, 5, 40
    t_out = T - K + 1
    rng = np.random.default_rng(3100)
    x = rng.uniform(-1, 1, (B, Cin, T)).astype(np.float32)
    w = (rng.uniform(-1, 1, (K, Cin, Cout)) / np.sqrt(K * Cin)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, Cout).astype(np.float32)
    ref = _conv64(x, w, b, 1, 0, t_out)
    ref = torch.maximum(0.2 * ref, ref).numpy()
    dx, dw, db = (torch.from_numpy(a).cuda() for a in (x, w, b))
    y = torch.empty((B, Cout, t_out), device="cuda")
    k3 = range(max(RETIRED_VARIANTS) + 1, lib.wun_op_num_conv_variants())
    assert len(k3) == 11

    def launch(v):
        y.fill_(float("nan"))
        lib.wun_op_force_conv_variant(v, 1)
        try:
            rc = lib.wun_op_conv1d(dx.data_ptr(), dw.data_ptr(), db.data_ptr(), y.data_ptr(), B, Cin, Cout, K, T, t_out, 1, 0, 1, _stream())
        finally:
            lib.wun_op_force_conv_variant(-1, 0)
        torch.cuda.synchronize()
        return rc, y.cpu().numpy()

    worst, ran = 0.0, {}
    for value in (None, "0"):
        _environment(monkeypatch, {} if value is None else {"WUN_NO_K3": value})
        ran[value] = []
        for v in k3:
            rc, got = launch(v)
            if rc != 0:
                assert np.isnan(got).all(), v
                continue
            err = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
            assert err <= CONV_OP_TOL, (v, err)
            worst = max(worst, err)
            ran[value].append(v)
    assert len(ran[None]) >= 2 and ran["0"] == ran[None], ran
    _environment(monkeypatch, {"WUN_NO_K3": "1"})
    for v in k3:
        rc, got = launch(v)
        assert rc != 0 and np.isnan(got).all(), (v, rc)
    rc, got = launch(-1)
    assert rc == 0 and np.abs(got - ref).max() / max(1.0, np.abs(ref).max()) <= CONV_OP_TOL
    record("switches_split_k_refusal", "forced split-K tiles %s without the switch" % ran[None], worst, CONV_OP_TOL)


# ---- the bf16 conv's tile height under the LDS cap ----
# launch_conv_bf16: the tallest tile (MT x 64 positions) that leaves >= 512 tiles, then the tallest one at or below it whose
# LDS footprint bf16_lds() is within the cap (default 80 KiB: two workgroups per CU).  K = 5, stride 1, N = 64 (one column
# group of NW = 4), Tout = 4096; bf16_lds = stages x (rows x (64 nck + 32)) + stages x (K x 4 x nck x 64 x 16) bytes with
# rows = 64 MT + 4, stages = 2 when the channels need more than one stage of 32 nck:
#   B = 16, Cin = 32: 512 tiles at MT = 2 (256 at MT = 4).  nck = 1, one stage: MT = 2 takes 132 x 96 + 20480 = 33152 bytes,
#                     MT = 1 68 x 96 + 20480 = 27008.  Default: <2, 4>.  Cap 32 KiB = 32768: <1, 4>.
#   B = 32, Cin = 64: 512 tiles at MT = 4.  MT = 4 (nck = 1, two stages): 2 x 260 x 96 + 2 x 20480 = 90880 bytes > 80 KiB;
#                     MT = 2 (nck = 2, one stage): 132 x 160 + 40960 = 62080.  Default: <2, 4>.  Cap 160 KiB: <4, 4>.
LDS_CAP_CASES = [((16, 32, 64, 5, 4100), "32", "conv_bf16_kernel<2, 4>", "conv_bf16_kernel<1, 4>"),
                 ((32, 64, 64, 5, 4100), "160", "conv_bf16_kernel<2, 4>", "conv_bf16_kernel<4, 4>")]


@pytest.mark.parametrize("case", LDS_CAP_CASES, ids=["cap%s %s" % (c[1], c[0]) for c in LDS_CAP_CASES])
def test_bf16_conv_tile_height_follows_the_lds_cap(lib, case, monkeypatch):
    (B, Cin, Cout, K, T), cap, name_default, name_capped = case
    t_out = T - K + 1
    rng = np.random.default_rng(3200 + B)
    x = rng.uniform(-1, 1, (B, Cin, T)).astype(np.float32)
    w = (rng.uniform(-1, 1, (K, Cin, Cout)) / np.sqrt(K * Cin)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, Cout).astype(np.float32)
    ref = F.conv1d(torch.tensor(_bf16_round(x)), torch.tensor(_bf16_round(w)).permute(2, 1, 0), torch.tensor(b, dtype=torch.float64))
    ref = torch.maximum(0.2 * ref, ref).numpy()
    dx, dw, db = (torch.from_numpy(a).cuda() for a in (x, w, b))
    y = torch.empty((B, Cout, t_out), device="cuda")
    scr = torch.full((int(lib.wun_op_conv1d_bf16_scratch(Cin, Cout, K)) + 4096,), float("nan"), device="cuda")

    def launch():
        y.fill_(float("nan"))
        _lib.check(lib.wun_op_conv1d_bf16(dx.data_ptr(), dw.data_ptr(), db.data_ptr(), y.data_ptr(), scr.data_ptr(), B, Cin, Cout, K,
                                          T, t_out, 1, 0, 1, _stream()))

    outs = {}
    for value, want in ((None, name_default), (cap, name_capped)):
        _environment(monkeypatch, {} if value is None else {"WUN_BF16_LDS_CAP": value})
        _, launches = _profiled_launches(lib, monkeypatch, launch)
        names = [n for n, _ in launches if n.startswith("conv_bf16_kernel")]
        assert names == [want], (value, names)
        got = y.cpu().numpy()
        assert np.isfinite(got).all()
        err = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
        record("switches_bf16_lds_cap", "%s cap %s %s" % (case[0], value or "default", want), err, BF16_OP_TOL)
        assert err <= BF16_OP_TOL, (value, err)
        outs[value] = got
    record("switches_bf16_lds_cap", "%s cap %s: bits equal the default's (1 = yes)" % (case[0], cap), float(np.array_equal(outs[None], outs[cap])), 1.0)
