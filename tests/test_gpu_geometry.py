"""The training step over every crop and window geometry (tests/_geometry.py): the plans of SWEEP -- a cover of every level
and head signature its grid reaches: odd and even crop starts, asymmetric crops, windows with 0 / 1 / 2+ odd and even
positions, every parity of the level lengths, levels whose even half does not lie inside the next level's odd-window range,
one output frame -- each in two dressings (mono / linear upsampling / difference output; stereo / learned upsampling / four
direct outputs), against the oracles on the same weights and batch:

  * fp32: outputs, loss, every gradient and d loss / d mix of a loss that is not MSE against the float64 oracle evaluated on
    the kernels' own LeakyReLU branches (_gpu_pins -- on nets this small one flipped branch moves a bias by more than any
    free tolerance); inference against the training forward with AudioClip applied;
  * the plans whose window input gradient cannot start early (E outside W), under the three schedules of the odd window --
    each against the pinned oracle, and the gradients of the three against each other;
  * bf16 mode: every stored tensor, the loss and every gradient against oracle/bf16_emul.py layer by layer;
  * same padding down to a one-position bottleneck, even filter sizes (asymmetric padding) included.

One test per (filter triple, num_layers); its few plans run inside it.  Figures seen on an MI355X:
profiles/geometry_parity_observed.json."""
import numpy as np
import pytest
import torch

from oracle import shapes, waveunet_torch as wt
from oracle.golden_params import golden_params
from _observed import record
from test_gpu_parity import GRAD_TOL_PINNED, OUT_TOL, _gpu_pins, _grad_check, _loss_check, _out_check
from test_gpu_backward import _mix_check, _oracle_custom, _upstream
from test_gpu_bf16 import (BF16_GRAD_L2_TOL, BF16_LOSS_TOL, BF16_OUT_TOL, EMUL_FLIP_TOL, _compare_with_emulation)
from test_gpu_dedup import TOL as SCHEDULE_TOL

import wave_u_net_amd as wun
from wave_u_net_amd.separator import UnetAudioSeparator

import _geometry as geo

pytestmark = pytest.mark.gpu

B = 3
GRAD_FLOOR = 1e-3       # max|ref| of every conv kernel / bias gradient: _grad_check allows tol * max|ref| + 1e-7, so the absolute
                        # term adds at most 1e-4 relative -- four orders below the O(1) error of an indexing mistake
SCHEDULES = ({}, {"WUN_EARLY_WINDOW": "0"}, {"WUN_NO_ODD_ALIGN": "1"})
SAME_TRIPLES_LAYERS = [(t, L) for t in geo.TRIPLES for L in (1, 3)]


def _seeds(triple, L, t_in):
    return 400 + 10 * geo.TRIPLES.index(triple) + L, 7000 + t_in


_INPUTS = {}


def _inputs(ocfg, t_in, seeds):
    """(params, mix, targets) of one plan: golden_params and _geometry.batch.  The weights' seed is the first of
    seeds[0], seeds[0] + 50, ... at which every conv kernel's and bias's gradient of the FREE float64 oracle reaches 1.25 * GRAD_FLOOR
    in max-norm -- chosen on the reference alone, so that GRAD_FLOOR (asserted in _fp32_step on the pinned oracle) holds:
    the deep kernels of a 4-level net with 8 filters see 1e-4 .. 7e-3 depending on the draw."""
    key = (tuple(sorted((k, str(v)) for k, v in ocfg.items())), t_in, seeds)
    if key not in _INPUTS:
        t_out = shapes.layer_table(ocfg, t_in)["t_out"]
        mix, targets = geo.batch(ocfg, B, t_in, t_out, seeds[1])
        for seed in range(seeds[0], seeds[0] + 5000, 50):
            params = golden_params(ocfg, seed)
            _, grads, _ = wt.chunked_train_step(ocfg, params, mix, targets, dtype=torch.float64, chunk=B)
            if min(g.abs().max().item() for (n, _), g in zip(params, grads) if "/interp_" not in n) >= 1.25 * GRAD_FLOOR:
                break
        else:
            raise AssertionError("no weights with gradients above the floor: %r" % (key,))
        _INPUTS[key] = (params, mix, targets)
    return _INPUTS[key]


def _build(over, ocfg, t_in, dtype="f32"):
    """A fresh separator with one plan (B, t_in): a plan reads the environment switches when it is created."""
    sep = UnetAudioSeparator(wun.get_config("baseline", compute_dtype=dtype, **over), device="cuda:0")
    sep._plan(B, t_in); sep._active = sep._plans[(B, t_in)]
    t_out = int(sep._active.info.output_frames)
    assert t_out == shapes.layer_table(ocfg, t_in)["t_out"]
    return sep, t_out


def _fp32_step(over, ocfg, t_in, seeds, tag, inference=True):
    """One plan against the branch-pinned float64 oracle: outputs, loss, gradients, d_mix of _custom_loss, inference.
    Returns the MSE step's gradients (numpy, by name)."""
    params, mix, targets = _inputs(ocfg, t_in, seeds)
    sep, t_out = _build(over, ocfg, t_in)
    sep.load_variables(params)
    assert sep.effective_dtype == "f32"
    names = ocfg["source_names"]
    dmix = torch.from_numpy(mix).cuda()
    outs = {k: v.clone() for k, v in sep.get_output(dmix, True).items()}
    loss = sep.loss_and_gradients({k: torch.from_numpy(v) for k, v in targets.items()})
    torch.cuda.synchronize()
    pins = _gpu_pins(sep, ocfg)           # (asserts: the window's even positions hold the decimated stream's bits)
    ploss, pgrads, pouts = wt.chunked_train_step(ocfg, params, mix, targets, dtype=torch.float64, chunk=B, want_outputs=True,
                                                 pins=pins)
    tp = [(n, None) for n, _ in params]
    for n in names:
        assert tuple(outs[n].shape) == (B, t_out, ocfg["num_channels"]) and torch.isfinite(outs[n]).all(), (tag, n)
    _out_check(outs, pouts, names, tag)
    _loss_check(loss.item(), ploss, tag)
    for (n, _), og in zip(params, pgrads):
        if "/interp_" not in n:           # (exactly 0 where the bottleneck has one position: tests/test_gpu_elementwise.py is theirs)
            assert og.abs().max().item() >= GRAD_FLOOR, (tag, n, og.abs().max().item())
    _grad_check(sep, tp, pgrads, tol=GRAD_TOL_PINNED, tag=tag)
    grads = {k: v.detach().cpu().numpy().copy() for k, v in sep.gradients().items()}

    # a loss that is not MSE, and d loss / d mix: mix_grad_kernel's offsets at odd and asymmetric input crops
    tg = torch.stack([torch.from_numpy(targets[n]) for n in names]).cuda()
    d_mix = sep.backward(_upstream(outs, names, tg), input_grad=True)
    torch.cuda.synchronize()
    tpc, cgrads, odmix = _oracle_custom(ocfg, params, dmix, tg, pins)
    _grad_check(sep, tpc, cgrads, tol=GRAD_TOL_PINNED, tag="custom_loss_" + tag)
    assert tuple(d_mix.shape) == tuple(dmix.shape)
    _mix_check(d_mix, odmix, "custom_loss_" + tag)

    if inference:                         # other launches, the same geometry
        ev = sep.get_output(dmix, False)
        torch.cuda.synchronize()
        worst = max((ev[n] - outs[n].clamp(-1.0, 1.0)).abs().max().item() for n in names)
        record("inference_vs_clipped_training_forward", tag, worst, OUT_TOL)
        assert worst <= OUT_TOL, (tag, worst)
    return grads


def _bf16_step(over, ocfg, t_in, seeds, tag, pool):
    """One plan in the bf16 mode against the layer-by-layer emulation (asserted, the differing fraction pooled by the
    caller) and against the un-rounded float64 oracle (recorded: BF16_* were sized for longer sums than these nets have)."""
    params, mix, targets = _inputs(ocfg, t_in, seeds)
    sep, t_out = _build(over, ocfg, t_in, "bf16")
    sep.load_variables(params)
    assert sep.effective_dtype == "bf16", tag
    outs = sep.get_output(torch.from_numpy(mix).cuda(), True)
    loss = sep.loss_and_gradients({k: torch.from_numpy(v) for k, v in targets.items()})
    torch.cuda.synchronize()
    g = sep.gradients()
    assert all(torch.isfinite(v).all() for v in g.values()), tag
    oloss, ograds, oouts = wt.chunked_train_step(ocfg, params, mix, targets, dtype=torch.float64, chunk=B, want_outputs=True)
    eo = max((outs[n].cpu().double() - oouts[n]).abs().max().item() for n in ocfg["source_names"])
    record("bf16_outputs_vs_float64_oracle (not asserted)", tag, eo, BF16_OUT_TOL)
    record("bf16_loss_vs_float64_oracle (not asserted)", tag, abs(loss.item() - oloss) / max(abs(oloss), 1e-3), BF16_LOSS_TOL)
    l2 = max((g[n].cpu().double() - og).norm().item() / max(og.norm().item(), 1e-30)
             for (n, _), og in zip(params, ograds) if n.endswith("/kernel"))
    record("bf16_gradients_rel_l2_vs_float64_oracle (not asserted)", tag, l2, BF16_GRAD_L2_TOL)
    _compare_with_emulation(sep, ocfg, params, mix, targets, loss.item(), g, tag, flip_pool=pool)


def _pooled_flips(pool, tag):
    differ, total = sum(d for d, _ in pool), sum(n for _, n in pool)
    frac = differ / max(total, 1)
    record("bf16_stored_tensors_differing_fraction_pooled_vs_layerwise_emulation", "%s (%d of %d)" % (tag, differ, total), frac,
           EMUL_FLIP_TOL)
    assert frac <= EMUL_FLIP_TOL, (tag, differ, total)


@pytest.mark.parametrize("group", geo.GROUPS, ids=[geo.group_id(g) for g in geo.GROUPS])
def test_fp32_step_over_the_sweep(group, monkeypatch):
    monkeypatch.setenv("WUN_NO_TUNE", "1")
    for k in ("WUN_NO_DEDUP", "WUN_EARLY_WINDOW", "WUN_ODD_FUSE_MIN", "WUN_NO_ODD_ALIGN"):
        monkeypatch.delenv(k, raising=False)
    triple, L = group
    for t_in in geo.SWEEP.get(group, []):
        for dressing in sorted(geo.DRESSINGS):
            _fp32_step(geo.overrides(triple, L, dressing), geo.oracle_config(triple, L, dressing), t_in, _seeds(triple, L, t_in),
                       "%s_T%d_%s" % (geo.group_id(group), t_in, dressing))


NON_NESTED_GROUPS = sorted(geo.NON_NESTED_GROUPS)


@pytest.mark.parametrize("group", NON_NESTED_GROUPS, ids=[geo.group_id(g) for g in NON_NESTED_GROUPS])
def test_naturally_non_nested_plans_under_every_window_schedule(group, monkeypatch):
    """E outside W without a switch forcing it: level_early is false for that level, the window part of its input gradient
    runs after the row-wide conv.  Default / no early window / odd window start unaligned: each against the pinned oracle,
    and the three against each other to fp32 summation order."""
    monkeypatch.setenv("WUN_NO_TUNE", "1")
    triple, L = group
    for t_in in geo.NON_NESTED_GROUPS[group]:
        for dressing in sorted(geo.DRESSINGS):
            over, ocfg = geo.overrides(triple, L, dressing), geo.oracle_config(triple, L, dressing)
            assert 0 in geo.nested(ocfg, t_in)
            tag = "%s_T%d_%s" % (geo.group_id(group), t_in, dressing)
            runs = []
            for env in SCHEDULES:
                for k in ("WUN_NO_DEDUP", "WUN_EARLY_WINDOW", "WUN_ODD_FUSE_MIN", "WUN_NO_ODD_ALIGN"):
                    monkeypatch.delenv(k, raising=False)
                for k, v in env.items():
                    monkeypatch.setenv(k, v)
                runs.append(_fp32_step(over, ocfg, t_in, _seeds(triple, L, t_in), "%s %s" % (tag, sorted(env.items())),
                                       inference=False))
            worst = 0.0
            for other in runs[1:]:
                for k, ref in runs[0].items():
                    worst = max(worst, np.abs(other[k] - ref).max() / max(1e-12, np.abs(ref).max()))
            record("non_nested_window_schedules_gradients", tag, worst, SCHEDULE_TOL)
            assert worst <= SCHEDULE_TOL, (tag, worst)


SWEEP_GROUPS = sorted(geo.SWEEP)


@pytest.mark.parametrize("group", SWEEP_GROUPS, ids=[geo.group_id(g) for g in SWEEP_GROUPS])
def test_bf16_step_over_the_sweep(group, monkeypatch):
    monkeypatch.setenv("WUN_NO_TUNE", "1")
    triple, L = group
    pool = []
    for t_in in geo.SWEEP[group]:
        _bf16_step(geo.overrides(triple, L, "stereo"), geo.oracle_config(triple, L, "stereo"), t_in, _seeds(triple, L, t_in),
                   "bf16_%s_T%d_stereo" % (geo.group_id(group), t_in), pool)
    _pooled_flips(pool, "bf16_" + geo.group_id(group))


@pytest.mark.parametrize("group", SAME_TRIPLES_LAYERS, ids=[geo.group_id(g) for g in SAME_TRIPLES_LAYERS])
def test_same_padding_down_to_a_one_position_bottleneck(group, monkeypatch):
    """Tin = 2^L {1, 2, 3}: one, two and three bottleneck positions; an even filter_size pads asymmetrically."""
    monkeypatch.setenv("WUN_NO_TUNE", "1")
    triple, L = group
    over = dict(geo.overrides(triple, L, "mono"), context=False)
    ocfg = shapes.finalize_config(dict(shapes.BASE_MODEL_CONFIG, **over))
    pool = []
    for m in (1, 2, 3):
        t_in = m << L
        assert shapes.layer_table(ocfg, t_in)["bottleneck"]["t_conv"] == m
        tag = "same_%s_T%d_mono" % (geo.group_id(group), t_in)
        _fp32_step(over, ocfg, t_in, _seeds(triple, L, t_in), tag)
        _bf16_step(over, ocfg, t_in, _seeds(triple, L, t_in), "bf16_" + tag, pool)
    _pooled_flips(pool, "bf16_same_" + geo.group_id(group))
