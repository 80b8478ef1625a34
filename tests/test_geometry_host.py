"""The geometry sweep (tests/_geometry.py) on the host: what the grid reaches beside what the named cases reach, and every plan
of the grid -- both dressings, both compute dtypes -- created by the library and compared with oracle/shapes.py: output frames,
the variable table, where the activations live (wun_plan_activation), whether the bf16 mode is effective; and the lengths
below the shortest valid one, refused.  No GPU: a plan is host state."""
import ctypes as C

import pytest

from oracle import shapes
from oracle.golden_params import GOLDEN_CASES

import wave_u_net_amd as wun
from wave_u_net_amd import _lib
from wave_u_net_amd.separator import _Plan, _wun_config

import _geometry as geo

GRID_GROUPS = [(t, L) for t in geo.TRIPLES for L in geo.LAYERS]


def _named_cases():
    """(ocfg, t_in) of every context plan the named cases build: GOLDEN_CASES with context, test_gpu_dedup.CASES."""
    import test_gpu_dedup
    out = []
    for name in sorted(GOLDEN_CASES):
        case = GOLDEN_CASES[name]
        ocfg = shapes.finalize_config(dict(shapes.BASE_MODEL_CONFIG, **case["cfg"]))
        if ocfg["context"]:
            out.append((ocfg, shapes.get_padding(ocfg, [1, case["frames"], 0])[0][1]))
    for name, over, _ in test_gpu_dedup.CASES:
        cfg = wun.get_config(name, **over)
        ocfg = shapes.finalize_config({k: cfg[k] for k in shapes.BASE_MODEL_CONFIG})
        assert ocfg["context"]
        out.append((ocfg, shapes.get_padding(ocfg, [1, cfg["num_frames"], 0])[0][1]))
    return out


def test_sweep_covers_the_grid_and_the_named_cases_do_not():
    named_levels, named_heads = set(), set()
    for ocfg, t_in in _named_cases():
        lv, hd = geo.signature(ocfg, t_in)
        named_levels |= lv
        named_heads.add(hd)
    grid_levels, grid_heads = geo.reached(geo.CANDIDATES)
    sweep_levels, sweep_heads = geo.reached(geo.SWEEP_PLANS)
    print("named cases: %d level / %d head signatures; sweep: %d / %d" % (
        len(named_levels), len(named_heads), len(sweep_levels), len(sweep_heads)))
    assert (sweep_levels, sweep_heads) == (grid_levels, grid_heads)
    assert len(geo.SWEEP_PLANS) <= geo.MAX_SWEEP and set(geo.SWEEP_PLANS) <= set(geo.CANDIDATES)
    assert sorted(sum(([(g[0], g[1], t) for t in ts] for g, ts in geo.SWEEP.items()), [])) == sorted(geo.SWEEP_PLANS)
    # every field takes every value it can
    want = [{0, 1}, {0, 1}, {0, 1, 2}, {0, 1, 2}, {0, 1}, {0, 1}, {0, 1}, {-1, 0, 1}]
    for f, values in enumerate(want):
        assert {s[f] for s in sweep_levels} == values, (f, values)
    assert len(sweep_heads) == 12 and all({h[f] for h in sweep_heads} == {0, 1} for f in range(4))
    assert len(sweep_levels) >= 50
    # the gap: what the named cases reach is a strict subset, and it is small
    assert named_levels < sweep_levels and named_heads < sweep_heads
    assert (len(named_levels), len(named_heads)) == (6, 2)
    assert not any(s[2] < 2 or s[3] < 2 or s[7] == 0 for s in named_levels)       # n_odd, n_even in {0, 1}; E outside W
    # the plans whose window gradient cannot start early exist, and the sweep's groups hold all of them
    assert len(geo.NON_NESTED) == 12 and set(geo.NON_NESTED_GROUPS) <= set(geo.GROUPS)
    # deterministic: computed again, the same list
    assert geo._greedy_cover(geo._candidates()) == geo.SWEEP_PLANS


def test_batch_targets_are_the_reference_crop():
    ocfg = geo.oracle_config((8, 4, 2), 2, "stereo")
    mix, targets = geo.batch(ocfg, 3, 64, 7, seed=5)
    assert mix.shape == (3, 64, 2) and sorted(targets) == sorted(ocfg["source_names"])
    total = sum(targets.values())
    assert total.shape == (3, 7, 2)
    assert abs(total - mix[:, 28:35]).max() <= 1e-6             # (64 - 7) // 2 = 28, the odd frame dropped at the end
    assert abs(mix).max() <= 0.9 + 1e-6
    m2, t2 = geo.batch(ocfg, 3, 64, 7, seed=5)
    assert (m2 == mix).all() and all((t2[k] == targets[k]).all() for k in targets)


def _activation(lib, plan, kind, index):
    info = _lib.WunActivationInfo()
    _lib.check(lib.wun_plan_activation(plan.handle, kind, index, C.byref(info)))
    return int(info.channels), int(info.frames), int(info.t0), int(info.tstep)


@pytest.mark.parametrize("group", GRID_GROUPS, ids=[geo.group_id(g) for g in GRID_GROUPS])
def test_every_plan_of_the_grid_matches_the_oracle(group):
    lib = _lib.load()
    triple, L = group
    lengths = [t for tr, l_, t in geo.CANDIDATES if (tr, l_) == group]
    assert len(lengths) == 16
    for dressing in sorted(geo.DRESSINGS):
        ocfg = geo.oracle_config(triple, L, dressing)
        want_vars = [(n, list(s)) for n, s in shapes.variable_table(ocfg)]
        for dtype in ("f32", "bf16"):
            wcfg = _wun_config(wun.get_config("baseline", compute_dtype=dtype, **geo.overrides(triple, L, dressing)))
            for t_in in lengths:
                tag = (dressing, dtype, t_in)
                lt = shapes.layer_table(ocfg, t_in)
                plan = _Plan(lib, wcfg, 3, t_in)
                assert (plan.info.batch, plan.info.input_frames, plan.info.output_frames) == (3, t_in, lt["t_out"]), tag
                assert [(n, list(s)) for n, _, s in plan.tensors] == want_vars, tag
                # all four triples have filter_size >= 2 and 8 filters: the bf16 mode is effective on every plan of the grid
                assert int(plan.info.compute_dtype_effective) == (1 if dtype == "bf16" else 0), tag
                for i, d in enumerate(lt["down"]):
                    u = lt["up"][L - 1 - i]
                    for kind in (0, 8):                  # dec_i, dz_dec_i: the decimated stream
                        assert _activation(lib, plan, kind, i) == (d["cout"], d["t_dec"], 0, 2), (tag, kind, i)
                    for kind in (1, 7):                  # skip_i, dz_skip_i: the crop window
                        assert _activation(lib, plan, kind, i) == (d["cout"], u["t_up"], u["crop_start"], 1), (tag, kind, i)
                b = lt["bottleneck"]
                assert _activation(lib, plan, 2, 0) == (b["cout"], b["t_conv"], 0, 1), tag
                for j, u in enumerate(lt["up"]):
                    assert _activation(lib, plan, 3, j) == (u["cout"], u["t_conv"], 0, 1), (tag, j)


@pytest.mark.parametrize("group", GRID_GROUPS, ids=[geo.group_id(g) for g in GRID_GROUPS])
def test_lengths_below_the_shortest_valid_one_are_refused(group):
    lib = _lib.load()
    triple, L = group
    shortest = min(t for tr, l_, t in geo.CANDIDATES if (tr, l_) == group)
    assert shortest > 1
    for dressing in sorted(geo.DRESSINGS):
        ocfg = geo.oracle_config(triple, L, dressing)
        for dtype in ("f32", "bf16"):
            wcfg = _wun_config(wun.get_config("baseline", compute_dtype=dtype, **geo.overrides(triple, L, dressing)))
            for t_in in range(0, shortest):
                assert t_in == 0 or not geo.valid(ocfg, t_in)
                handle = C.c_void_p()
                rc = lib.wun_plan_create(C.byref(wcfg), 3, t_in, C.byref(handle))
                assert rc == -1 and not handle, (dressing, dtype, t_in, rc)          # WUN_ERR_INVALID, no plan
                assert lib.wun_last_error()
