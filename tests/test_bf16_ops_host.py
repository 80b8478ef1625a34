"""Host-side half of the bf16 conv operator tests (no GPU): the new C ABI entries exist and check their arguments before any
GPU work; the tile codes the launcher can ever accept, per mode and tap instantiation, are derived from the library itself
(wun_op_conv_bf16_choice_ok) and pinned; the GPU case list of tests/test_gpu_bf16_ops.py reaches every one of them; and the
float64 references of tests/_bf16_ops_np.py are SENSITIVE: every mutant misses the true reference by more than the bound the
GPU tests assert, on every case of theirs it applies to (as tests/test_elementwise_host.py does for the elementwise family)."""
import ctypes as C
import os

import numpy as np
import pytest

import _bf16_ops_np as R
import _elementwise_np as E
from wave_u_net_amd import _lib

NEW_SYMBOLS = ("wun_op_conv_bf16_abi_size", "wun_op_conv_bf16_ex_scratch", "wun_op_conv_bf16_ex", "wun_op_conv_bf16_choice_ok",
               "wun_op_first_conv")
C_FACTOR = 1.0            # tests/test_gpu_bf16_ops.py: the measured factor of the fp32 bound


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _desc(**kw):
    return _lib.WunOpConvBf16Desc(**kw)


def test_new_entries_are_exported_and_the_descriptor_has_the_librarys_size(lib):
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.wun_op_conv_bf16_abi_size() == C.sizeof(_lib.WunOpConvBf16Desc) == 23 * 4
    assert (_lib.OP_FIRST_CONV, _lib.PATH_FIRST_CONV, _lib.BF16_VARIANT_BASE) == (7, 10, 1000)
    assert lib.wun_op_last_path(_lib.OP_FIRST_CONV) == _lib.PATH_NONE
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    design = open(os.path.join(root, "DESIGN.md")).read()
    for name in NEW_SYMBOLS:
        assert "`%s`" % name in doc, name
    for name in ("wun_op_conv_bf16_ex", "wun_op_conv_bf16_choice_ok", "wun_op_first_conv", "WUN_BF16_VARIANT_BASE"):
        assert name in design, name


def test_argument_checks_run_before_any_gpu_work(lib):
    """Every refusal below happens on a machine without a GPU: the checks come first.  (Pointers are made-up addresses; a
    refused call never touches them.)"""
    p = 4096
    good = R.desc_fields(R.SWEEP_CASES[0])
    assert lib.wun_op_conv_bf16_choice_ok(None, 0) == -1
    assert lib.wun_op_conv_bf16_ex_scratch(None) == -1
    assert lib.wun_op_conv_bf16_ex_scratch(_desc(**good)) > 0
    bad = [dict(mode=3), dict(B=0), dict(C0=0), dict(K=0), dict(N0=0), dict(N0=good["N"] + 1), dict(x_off=-1),
           dict(x0_pitch=good["Tin"] - 1), dict(x_off=good["x0_pitch"]), dict(y0_pitch=good["Tout"] - 1), dict(acc_len=-1),
           dict(dec_pitch=1), dict(N0=8, y1_pitch=0)]
    for b in bad:
        d = _desc(**dict(good, **b))
        assert lib.wun_op_conv_bf16_choice_ok(d, 0) == -1, b
        assert lib.wun_op_conv_bf16_ex(d, p, None, p, None, p, p, None, None, None, p, None) == -1, b
    t2 = R.desc_fields(R.SWEEP_CASES[-1])
    for b in [dict(shift=1), dict(C1=8, x1_pitch=t2["x0_pitch"]), dict(N0=8, y1_pitch=t2["y0_pitch"]), dict(N=18, N0=18),
              dict(lrelu=1), dict(dec_pitch=64)]:
        assert lib.wun_op_conv_bf16_choice_ok(_desc(**dict(t2, **b)), 0) == -1, b
    d = _desc(**good)
    assert lib.wun_op_conv_bf16_ex(d, None, None, p, None, p, None, None, None, None, p, None) == -1          # null x0
    assert lib.wun_op_conv_bf16_ex(d, p, None, p, None, p, None, None, None, p, p, None) == -1                # dec without pitch
    assert lib.wun_op_conv_bf16_ex(d, p + 8, None, p, None, p, None, None, None, None, p, None) == -1         # misaligned rows
    assert lib.wun_op_conv_bf16_ex(d, p, None, p, None, p + 2, None, None, None, None, p, None) == -1         # fp32 y off 4 bytes
    # what the kernel does not serve: unsupported, not invalid
    for b in [dict(C0=4), dict(K=16, Tin=good["Tin"]), dict(x0_pitch=good["x0_pitch"] + 1)]:
        assert lib.wun_op_conv_bf16_ex(_desc(**dict(good, **b)), p, None, p, None, p, None, None, None, None, p, None) == -2, b
    two = dict(good, C0=12, C1=60, x1_pitch=good["x0_pitch"])
    assert lib.wun_op_conv_bf16_ex(_desc(**two), p, p, p, None, p, None, None, None, None, p, None) == -2     # C0 % 8 != 0
    # a forced code the launcher refuses: unsupported, before any GPU work; forced fp32 variants are not for this entry
    try:
        lib.wun_op_force_conv_variant(_lib.BF16_VARIANT_BASE + 26, 0)
        c = R.SWEEP_CASES[3]                                             # Tout = 20: no 256-row tile
        assert lib.wun_op_conv_bf16_choice_ok(_desc(**R.desc_fields(c)), 26) == 0
        assert lib.wun_op_conv_bf16_ex(_desc(**R.desc_fields(c)), p, None, p, None, p, None, None, None, None, p, None) == -2
    finally:
        lib.wun_op_force_conv_variant(-1, 0)
    # the audio-input conv
    f = lib.wun_op_first_conv
    assert f(None, p, None, p, None, 2, 1, 24, 15, 100, 86, 1, 0, 1, 1, 100, 88, 0, None) == -1
    assert f(p, p, None, p, None, 2, 1, 24, 15, 100, 86, 1, 0, 1, 1, 99, 88, 0, None) == -1                  # x_pitch < t_in
    assert f(p, p, None, p, None, 2, 1, 24, 15, 100, 86, 1, 0, 1, 1, 100, 85, 0, None) == -1                 # y_pitch < t_out
    assert f(p, p, None, p, p, 2, 1, 24, 15, 100, 86, 1, 0, 1, 1, 100, 88, 42, None) == -1                   # dec_pitch < 43
    assert f(p, p, None, p, None, 2, 1, 24, 15, 100, 86, 3, 0, 1, 1, 100, 88, 0, None) == -2                 # stride
    for cin, k, yp, yptr in [(3, 15, 88, p), (1, 16, 88, p), (1, 15, 86, p), (1, 15, 88, p + 8)]:            # first_conv_supported
        assert f(p, p, None, yptr, None, 2, cin, 24, k, 100, 86, 1, 0, 1, 1, 100, yp, 0, None) == -2, (cin, k, yp)


# ---------------------------------------------------------------------------------------------------------------------------
# which tile codes can ever run
# ---------------------------------------------------------------------------------------------------------------------------
def _legal_codes(lib, c, x_off=0):
    d = _desc(**R.desc_fields(c, x_off=x_off))
    out = set()
    for code in range(R.NCODES):
        rc = lib.wun_op_conv_bf16_choice_ok(d, code)
        assert rc in (0, 1), (c, code, rc)
        if rc:
            out.add(code)
    return out


def _grid_case(mode, C_, N, taps, Tout):
    if mode == R.T2:
        if N % 4:
            return None
        return R._t2(C_, N, 2 * taps - 1, Tout) if Tout >= 2 * taps - 1 else None
    return R._fwd(mode, C_, N, taps, Tout, short=0)


@pytest.fixture(scope="module")
def reachable(lib):
    got = {}
    for key, taps_list in R.GRID_TAPS.items():
        mode = key[0]
        s = set()
        for taps in taps_list:
            assert R.kt_of(mode, taps) == key[1]
            for C_ in R.GRID_C:
                for N in R.GRID_N:
                    for T in R.GRID_T:
                        c = _grid_case(mode, C_, N, taps, T)
                        if c is not None:
                            s |= _legal_codes(lib, c)
        got[key] = tuple(sorted(s))
    return got


def test_reachable_tile_codes_are_the_pinned_sets(lib, reachable):
    """The legal sets per (mode, tap instantiation), from the library's own conv_bf16_choice_ok over GRID_C x GRID_N x GRID_T:
    everything else -- every NCK >= 2 tile of the stride-2 loader, NCK = 3 of the 128- and 256-row tiles, odd NW of the
    two-phase conv -- is compiled but unreachable."""
    assert reachable == R.LEGAL
    assert all(R.code_tile(c)[2] == 1 for key, s in reachable.items() if key[0] == R.S2 for c in s)
    assert all(R.code_tile(c)[1] % 2 == 0 for key, s in reachable.items() if key[0] == R.T2 for c in s)
    assert all(R.code_tile(c)[2] <= 2 for s in reachable.values() for c in s if R.code_tile(c)[0] >= 2)


def test_gpu_sweep_cases_reach_every_legal_code(lib):
    seen = {key: set() for key in R.LEGAL}
    for c in R.SWEEP_CASES:
        key = (c.mode, R.kt_of(c.mode, R.taps_of(c)))
        for x_off in (R.EVEN_OFF, R.ODD_OFF):
            codes = _legal_codes(lib, c, x_off)
            assert codes <= set(R.LEGAL[key]), (c, sorted(codes - set(R.LEGAL[key])))
            seen[key] |= codes
    for key, want in R.LEGAL.items():
        assert seen[key] == set(want), (key, sorted(set(want) - seen[key]))
    for sc in R.STORE_CASES:
        key = (sc.case.mode, R.kt_of(sc.case.mode, R.taps_of(sc.case)))
        assert sc.code in _legal_codes(lib, sc.case, sc.x_off), sc.name


def test_store_cases_cover_every_store_path():
    """Per mode: vector stores without and with a scalar tail (Tout = 0 / != 0 mod 4) and an output offset that breaks the
    16-byte alignment; two sources (C0 = 24, C1 = 16) with mask and ranged accumulate; the column split N0 < N."""
    for mode in (R.S1, R.S2, R.T2):
        mine = [s for s in R.STORE_CASES if s.case.mode == mode]
        assert any(s.y_off == 0 and s.case.Tout % 4 == 0 for s in mine), mode
        assert any(s.y_off == 0 and s.case.Tout % 4 != 0 for s in mine), mode
        assert any(s.y_off % 4 != 0 for s in mine), mode
        assert any(s.mask and s.acc is not None for s in mine) or mode == R.S2 and any(s.acc for s in mine), mode
    assert any((s.case.C0, s.case.C1) == (24, 16) and s.mask and s.acc and s.acc[1] for s in R.STORE_CASES)
    assert any(s.case.N0 < s.case.N and s.y_off == 0 for s in R.STORE_CASES)
    assert any(s.case.N0 < s.case.N and s.y_off % 4 for s in R.STORE_CASES)
    assert any(s.x_off % 2 for s in R.STORE_CASES) and any(s.dec for s in R.STORE_CASES)


# ---------------------------------------------------------------------------------------------------------------------------
# sensitivity
# ---------------------------------------------------------------------------------------------------------------------------
CONV_MUTANTS = ("drop_tap", "shift_taps", "drop_last_group", "swap_stage_groups", "odd_pair_partner", "admit_pad",
                "zero_last_col_tile", "swap_planes", "swap_phases")


@pytest.mark.parametrize("ci", range(len(R.SWEEP_CASES)), ids=[str(tuple(c)) for c in R.SWEEP_CASES])
def test_conv_mutants_miss_the_sweep_bound(ci):
    c = R.SWEEP_CASES[ci]
    inp = R.case_inputs(c)
    lrelu = c.mode != R.T2
    applied = set()
    for x_off in (R.EVEN_OFF, R.ODD_OFF):
        ref, bound, _ = R.case_reference(c, inp, lrelu=lrelu, x_off=x_off, c_factor=C_FACTOR)
        assert R.fp32_verdict(ref.astype(np.float32).astype(np.float64), ref, bound) <= 1          # the bound admits fp32 itself
        for m in CONV_MUTANTS:
            if not R.MUTANTS[m](c, {"x_off": x_off}):
                continue
            bad, _, _ = R.case_reference(c, inp, lrelu=lrelu, x_off=x_off, mutant=m)
            assert R.fp32_verdict(bad, ref, bound) > 1, (m, x_off)
            applied.add(m)
    assert {"drop_tap", "shift_taps", "drop_last_group", "odd_pair_partner", "admit_pad", "zero_last_col_tile"} <= applied


def test_every_conv_mutant_applies_somewhere():
    for m in CONV_MUTANTS:
        assert any(R.MUTANTS[m](c, {"x_off": R.ODD_OFF}) for c in R.SWEEP_CASES), m


def _store_opts(sc, bf16):
    return {"x_off": sc.x_off, "mask": sc.mask, "acc": sc.acc, "dec": sc.dec, "bf16": bf16}


@pytest.mark.parametrize("si", range(len(R.STORE_CASES)), ids=[s.name for s in R.STORE_CASES])
def test_store_mutants_miss_what_the_store_tests_assert(si):
    """fp32 output: the bound; bf16 output: bit equality with the rounding of the fp32 output, bit equality of the compact copy
    with the even positions, and the bf16 verdict against float64."""
    sc = R.STORE_CASES[si]
    c = sc.case
    inp = R.case_inputs(c, grid=R.store_grid(sc))
    kw = dict(lrelu=sc.lrelu, mask=sc.mask, acc=sc.acc, y_off=sc.y_off, x_off=sc.x_off)
    ref, bound, big = R.case_reference(c, inp, c_factor=C_FACTOR, **kw)
    stored = R.stored_bf16(ref)
    assert R.bf16_verdict(stored, ref, big, bound) <= 1
    for m in CONV_MUTANTS + ("acc_outside", "mask_slope"):
        if not R.MUTANTS[m](c, _store_opts(sc, 0)):
            continue
        bad, _, _ = R.case_reference(c, inp, mutant=m, **kw)
        assert R.fp32_verdict(bad, ref, bound) > 1, m
        assert R.bf16_verdict(R.stored_bf16(bad), ref, big, bound) > 1, m
    # a truncating store: not the nearest-even rounding of the fp32 result, and over the cap on differing elements
    trunc = R.stored_bf16(ref, "truncate")
    d, t = E.differ_count(trunc, stored)
    assert d > E.BF16_DIFF_SHARE * t, (d, t)
    if R.store_grid(sc) == R.COARSE:
        # exact ties of the bf16 rounding are common here, and half of them part nearest-even from nearest-away
        tie =np.abs(ref - R.stored_bf16(ref)) * 2 == E.bf16_spacing(ref)
        assert np.count_nonzero(tie) > 0.02 * tie.size
        assert np.count_nonzero(tie & (ref > stored)) > 0.005 * tie.size and np.count_nonzero(tie & (ref < stored)) > 0.005 * tie.size
    if sc.dec:
        assert not np.array_equal(R.dec_ref(stored, c.N0, "dec_odd")[:, :, :c.Tout // 2], R.dec_ref(stored, c.N0)[:, :, :c.Tout // 2])


def test_the_cap_on_differing_bf16_elements_is_a_fair_condition():
    """At most 1e-3 of a GPU test function's bf16 outputs may differ from the once-rounded float64 reference.  That holds only
    for inputs on which any valid fp32 execution stays well under it: a float32 numpy stand-in that sums in another order stays
    under HALF the cap on the store cases (pooled, as the GPU test pools them) and on the audio-input conv's cases."""
    diff = total = 0
    for sc in R.STORE_CASES:
        c = sc.case
        inp = R.case_inputs(c, grid=R.store_grid(sc))
        kw = dict(lrelu=sc.lrelu, mask=sc.mask, acc=sc.acc, y_off=sc.y_off)
        ref, bound, big = R.case_reference(c, inp, x_off=sc.x_off, c_factor=C_FACTOR, **kw)
        got = R.stored_bf16(R.standin_fp32(c, inp, **kw).astype(np.float64))
        assert R.bf16_verdict(got, ref, big, bound) <= 1, sc.name
        d, t = E.differ_count(got, R.stored_bf16(ref))
        diff, total = diff + d, total + t
    assert diff <= 0.5 * E.BF16_DIFF_SHARE * total, (diff, total)
    diff = total = 0
    for fc in R.first_cases():
        if fc.Tout > 100 and (fc.N, fc.k) != (56, 15):
            continue                                                     # (the long rows once per stride and channel count)
        c = R.first_as_case(fc)
        x, w, bias = R.first_inputs(fc, grid=True)
        inp = {"x": x, "w": w, "bias": bias, "mask": None, "prior": None}
        ref, bound, big = R.case_reference(c, inp, lrelu=True)
        got = R.stored_bf16(R.standin_fp32(c, inp, lrelu=True, bias_first=True).astype(np.float64))
        d, t = E.differ_count(got, R.stored_bf16(ref))
        diff, total = diff + d, total + t
    assert diff <= 0.5 * E.BF16_DIFF_SHARE * total, (diff, total)


@pytest.mark.parametrize("stride, cin", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_first_conv_mutants_miss_the_bound(stride, cin):
    """The audio-input conv's reference against the mutants that apply to a direct conv: a dropped tap, shifted taps, an admitted
    pad element (the clamped edge loads), swapped even / odd samples (stride 2), the compact copy from the odd positions."""
    for fc in R.first_cases():
        if (fc.stride, fc.cin) != (stride, cin) or (fc.Tout > 100 and fc.N != 24):
            continue
        c = R.first_as_case(fc)
        x, w, bias = R.first_inputs(fc)
        inp = {"x": x, "w": w, "bias": bias, "mask": None, "prior": None}
        ref, bound, big = R.case_reference(c, inp, lrelu=True)
        for m in ("drop_tap", "shift_taps", "admit_pad", "zero_last_col_tile") + (("swap_planes",) if stride == 2 else ()):
            if m == "admit_pad" and not fc.same:
                continue                                                 # a valid conv reads no pad
            bad, _, _ = R.case_reference(c, inp, lrelu=True, mutant=m)
            assert R.fp32_verdict(bad, ref, bound) > 1, (fc, m)
        assert not np.array_equal(R.dec_ref(ref, fc.N, "dec_odd")[:, :, :fc.Tout // 2], R.dec_ref(ref, fc.N)[:, :, :fc.Tout // 2])
