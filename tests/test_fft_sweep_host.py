"""What tests/test_gpu_fft_sweep.py assumes, checked without a GPU (tests/_fft_sweep_np.py): the launch ledger's
entries, the references against the definitions written out as DFT matrices, the geometry each case is chosen for, the float32
stand-in inside the hard bounds on every chosen case -- and that the sweep's verdicts can fail: each is applied to mutant
references (a dropped bin, a missing conjugate, a neighbour's samples, ...) at every size and must refuse every one."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fft_np as fo  # noqa: E402
import _fft_sweep_np as sw  # noqa: E402
import _griffin_lim_np as gl  # noqa: E402
import _mrstft_fft_np as mf  # noqa: E402
import _spectral_np as sp  # noqa: E402

from wave_u_net_amd import _lib  # noqa: E402
from test_griffin_lim_host import cpu_step, one_step_check  # noqa: E402

SIZES = sw.SIZES
CELLS = _lib.FFT_FAMILY_COUNT * _lib.FFT_SIZE_COUNT


# ---------------------------------------------------------------------------------------------------- the ledger's entries
def test_ledger_entries_without_a_launch():
    lib = _lib.load()
    assert (_lib.FFT_FAMILY_FORWARD, _lib.FFT_FAMILY_MAGNITUDE, _lib.FFT_FAMILY_SPEC_HEAD, _lib.FFT_FAMILY_INVERSE,
            _lib.FFT_FAMILY_ADJOINT, _lib.FFT_FAMILY_GRIFFIN_LIM, _lib.FFT_FAMILY_GRIFFIN_LIM_GIVEN,
            _lib.FFT_FAMILY_VOC_ANALYSIS) == tuple(range(8)) and CELLS == 64 == 8 * len(SIZES)
    assert [64 << j for j in range(_lib.FFT_SIZE_COUNT)] == SIZES
    lib.wun_fft_launch_counts_reset()
    buf = (C.c_int64 * (CELLS + 1))(*([-7] * (CELLS + 1)))
    assert lib.wun_fft_launch_counts(None, CELLS) == -1 and b"null" in lib.wun_last_error()
    assert lib.wun_fft_launch_counts(buf, CELLS - 1) == -1 and b"cap" in lib.wun_last_error()
    assert list(buf) == [-7] * (CELLS + 1)                  # a refused call writes nothing
    assert lib.wun_fft_launch_counts(buf, CELLS) == 0
    assert list(buf) == [0] * CELLS + [-7]                  # every counter 0 after the reset; nothing written behind the table
    P = 0x10000                                             # (never dereferenced: the size is refused before any GPU work)
    for bad in (32, 16384):
        assert lib.wun_stft_complex_fft(P, 1, 1, 40000, 1, bad, bad // 4, 0, 1, P, P, P, None) == -2
        assert lib.wun_stft_magnitude_fft(P, 1, 1, 40000, 1, bad, bad // 4, P, P, None) == -2
        assert lib.wun_istft_fft(P, P, 1, 1, bad, 1, bad, bad // 4, 0, 1, P, P, P, None) == -2
    assert lib.wun_fft_launch_counts(buf, CELLS) == 0 and list(buf) == [0] * CELLS + [-7]      # a refused size counts nothing


# ---------------------------------------------------------------------------------------------------- geometry
def test_geometry_table_is_the_kernels_formulas():
    assert sorted(sw.GEOMETRY) == SIZES
    for n_fft in SIZES:
        logm, tpf, fpw, bpt, stages, tail, result = sw.GEOMETRY[n_fft]
        assert sw.GEOMETRY[n_fft] == sw.geometry(n_fft)
        assert 2 << logm == n_fft and tpf * fpw == sw.BLOCK and tpf * bpt * 4 == n_fft // 2
        assert stages == logm // 2 + (logm & 1) and tail == bool(logm & 1) and result == (stages - 1) % 2
        assert 2 * 2 * fpw * (n_fft // 2) * 4 <= 64 * 1024   # two images of two planes: at most the 64 KB of 8192


@pytest.mark.parametrize("n_fft", SIZES)
def test_case_a_has_the_properties_it_is_chosen_for(n_fft):
    c = sw.case(n_fft, "A")
    assert c["R"] == 3 and c["F"] == 5 and c["hop"] * 4 == n_fft and c["lead"] == 0
    assert c["T"] == n_fft + 4 * c["hop"] and sp.num_frames(c["T"], n_fft, c["hop"]) == 5 == sp.num_frames(c["T"] + c["hop"] - 1, n_fft, c["hop"])
    assert sp.num_frames(c["T"] - 1, n_fft, c["hop"]) == 4   # the smallest T with five whole frames
    wgs = sw.workgroups(n_fft, c["R"], c["F"])
    fpw = sw.fpw(n_fft)
    assert sum(len(w) for w in wgs) == 15
    part = len(wgs[-1]) < fpw
    crossing = any(len(set(r for r, _ in w)) > 1 for w in wgs)
    if n_fft <= 1024:
        assert part                                          # a part-filled last workgroup
    if 128 <= n_fft <= 1024:
        assert crossing                                      # a row boundary inside a workgroup
    if n_fft == 64:
        assert len(wgs) == 1 and crossing                    # all 15 rows in one workgroup
    if n_fft >= 2048:
        assert fpw == 1 and len(wgs) == 15 and not part and not crossing


@pytest.mark.parametrize("n_fft", SIZES)
def test_the_other_cases(n_fft):
    b, c, d = (sw.case(n_fft, n) for n in "BCD")
    assert b["shape"][2] == 2 and b["hop"] * 4 == 3 * n_fft and b["hop"] & (b["hop"] - 1) and b["F"] == 3
    assert sp.num_frames(b["T"], n_fft, b["hop"]) == 3
    assert c["T"] == n_fft and c["F"] == c["R"] == 1 and c["lead"] == 0 and len(sw.workgroups(n_fft, 1, 1)[0]) == 1
    assert d["T"] == 5 < n_fft and d["centered"] and d["lead"] == n_fft - d["hop"] and d["F"] == 4
    assert [x["name"] for x in sw.cases(n_fft, True)] == list("ABCD") and [x["name"] for x in sw.cases(n_fft, False)] == list("ABC")


# ---------------------------------------------------------------------------------------------------- reference consistency
@pytest.mark.parametrize("n_fft", [n for n in SIZES if n <= 256])
def test_references_are_the_definitions(n_fft):
    """numpy.fft against the O(n^2) DFT matrices of wun_fft.hip's header comment: forward, inverse, unscaled adjoint."""
    for c in sw.cases(n_fft, True):
        ref, spec = sw.signal(c), sw.spectra(c)
        fr = fo.frames_of(ref["xr"], n_fft, c["hop"], c["lead"], c["F"])
        dre, dim = sw.dft_forward(fr, n_fft)
        assert np.abs(dre - ref["re"]).max() <= 1e-12 and np.abs(dim - ref["im"]).max() <= 1e-12
        sre, sim = sw.split_step(fr * sp.window(n_fft))      # the kernel's own route to the same numbers
        assert np.abs(sre - ref["re"]).max() <= 1e-12 and np.abs(sim[..., 1:-1] - ref["im"][..., 1:-1]).max() <= 1e-12
        re64, im64 = spec["re"].astype(np.float64), spec["im"].astype(np.float64).copy()
        im64[..., 0] = im64[..., -1] = 0.0
        assert np.abs(sw.dft_inverse(re64, im64, n_fft) - fo.inverse_frames(spec["re"], spec["im"], n_fft)).max() <= 1e-12
        want = sw.dft_adjoint(re64, spec["im"].astype(np.float64), n_fft)      # (Sb is 0 at the edges: their Im does not count)
        assert np.abs(want - mf.adjoint(re64, spec["im"].astype(np.float64), n_fft)).max() <= 1e-12 * n_fft


@pytest.mark.parametrize("n_fft", SIZES)
def test_magnitude_reference_is_hypot_of_the_forward_one(n_fft):
    for c in sw.cases(n_fft, False):
        ref = sw.signal(c)
        m = mf.magnitude(ref["x"].astype(np.float64), n_fft, c["hop"])
        assert m.shape == ref["re"].shape and np.abs(m - np.hypot(ref["re"], ref["im"])).max() <= 1e-12 * n_fft


@pytest.mark.parametrize("n_fft", SIZES)
def test_adjoint_reference_passes_the_dot_product_test(n_fft):
    """<STFT x, Y> = <x, STFT^H Y> in float64, every bin of Y counted once."""
    for c in sw.cases(n_fft, False):
        ref, spec = sw.signal(c), sw.spectra(c)
        yre, yim = spec["re"].astype(np.float64), spec["im"].astype(np.float64)
        lhs = (ref["re"] * yre + ref["im"] * yim).sum()
        fr = fo.frames_of(ref["xr"], n_fft, c["hop"], c["lead"], c["F"])
        rhs = (fr * mf.adjoint(yre, yim, n_fft)).sum()
        scale = (np.abs(ref["re"] * yre) + np.abs(ref["im"] * yim)).sum()
        assert abs(lhs - rhs) <= 1e-12 * scale
        assert abs(lhs - (fr * sw.adjoint_edges_twice(yre, yim, n_fft)).sum()) > 1e-6 * scale      # (the test can fail)


# ---------------------------------------------------------------------------------------------------- the stand-in
@pytest.mark.parametrize("n_fft", SIZES)
def test_stand_in_lies_inside_the_hard_bounds(n_fft):
    for c in sw.cases(n_fft, True):
        ref, spec = sw.signal(c), sw.spectra(c)
        b = ref["beta"][:, :, None]
        assert ref["e32"] > 0 and (np.abs(ref["r32"] - ref["re"]) <= b).all() and (np.abs(ref["i32"] - ref["im"]) <= b).all()
        ok, figs = sw.inverse_verdict(spec["y32"], spec)
        assert ok and spec["e32"] > 0, figs


@pytest.mark.parametrize("n_fft", SIZES)
def test_griffin_lim_cases_meet_the_one_step_rules_condition(n_fft):
    """The Griffin-Lim framings of the cases (gl_case) keep rows, hop and F, and the CPU float32 path obeys the one-step rule on
    them -- its condition on the inputs included, which the lead-0 framings miss from n_fft 2048 up."""
    for c0 in sw.cases(n_fft, True):
        c = sw.gl_case(c0)
        assert (c["R"], c["hop"], c["F"], c["shape"]) == (c0["R"], c0["hop"], c0["F"], c0["shape"]) and 0 <= c["lead"] < n_fft
        R, T, hop, lead, F = c["R"], c["T"], c["hop"], c["lead"], c["F"]
        mag, y0 = gl.fixture(n_fft + hop + R, R, T, n_fft, hop, lead, F)
        s0 = cpu_step(y0, mag, n_fft, hop, lead, T)
        s1 = cpu_step(s0, mag, n_fft, hop, lead, T)
        one_step_check("fft_sweep_host[%d-%s]" % (n_fft, c["name"]), [y0, s0], [s0, s1], mag, n_fft, hop, lead)


# ---------------------------------------------------------------------------------------------------- sensitivity
@pytest.mark.parametrize("n_fft", SIZES)
def test_forward_verdict_passes_the_reference_and_refuses_every_mutant(n_fft):
    for c in sw.cases(n_fft, True):
        ref = sw.signal(c)
        im = ref["im"].copy()
        im[..., 0] = im[..., -1] = 0.0
        assert sw.forward_verdict(ref["re"], im, ref)[0]
        mutants = sw.forward_mutants(c)
        assert len(mutants) == (5 if c["R"] > 1 else 4)
        for name, (re, im) in mutants.items():
            ok, figs = sw.forward_verdict(re, im, ref)
            assert not ok, (n_fft, c["name"], name, figs)
        if not c["centered"]:                                # the magnitude's rule sees the dropped bin too
            m = np.hypot(*mutants["bin M dropped"])
            assert not sw.magnitude_verdict(m, ref["x"], n_fft, c["hop"])[0]
            assert sw.magnitude_verdict(np.hypot(ref["re"], ref["im"]), ref["x"], n_fft, c["hop"])[0]


@pytest.mark.parametrize("n_fft", SIZES)
def test_inverse_verdict_passes_the_reference_and_refuses_every_mutant(n_fft):
    for c in sw.cases(n_fft, True):
        spec = sw.spectra(c)
        assert sw.inverse_verdict(spec["want"], spec)[0]
        for name, y in sw.inverse_mutants(c).items():
            ok, figs = sw.inverse_verdict(y, spec)
            assert not ok, (n_fft, c["name"], name, figs)


@pytest.mark.parametrize("n_fft", SIZES)
def test_gradient_verdict_refuses_the_adjoint_with_its_edges_counted_twice(n_fft):
    for c in sw.cases(n_fft, False):
        ref = sw.loss_pair(c)
        o64, t64 = ref["out"].astype(np.float64), ref["tgt"].astype(np.float64)
        signs = [np.sign(mf.magnitude(o64, n_fft, c["hop"]) - mf.magnitude(t64, n_fft, c["hop"]))]
        g64, g32 = sw.gradient(ref, signs), sw.gradient(ref, signs, fp32=True)
        assert sw.gradient_verdict(g32, g64, g32)[0]
        ok, figs = sw.gradient_verdict(sw.gradient(ref, signs, adjoint=sw.adjoint_edges_twice), g64, g32)
        assert not ok, (n_fft, c["name"], figs)
        assert mf.adjoint is sw._ADJOINT                     # (the mutant was put in and taken out again)
