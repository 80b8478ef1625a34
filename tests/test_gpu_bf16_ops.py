"""The bf16 convs as single operators on an MI355X (wave-u-net_amd/csrc/wun_bf16.hip): conv_bf16_kernel tile by tile in its three
modes, the epilogue the bf16 mode really runs (bf16 stores, masks, ranged accumulate, the column split, the compact copy), input
rows the CALLER made (any first-element offset, NaN row padding) and first_conv_kernel in its 16 instantiations -- each against
the float64 references of tests/_bf16_ops_np.py, which tests/test_bf16_ops_host.py judges against mutants on these very cases.

Everywhere: inputs and outputs sit in NaN-filled allocations with guards, the row padding of inputs AND outputs is NaN;
afterwards every element inside an output row is finite and every other element is still NaN.

Bounds.  fp32 output against float64: |err| <= c (terms + 2) 2^-24 sum|terms| + 2^-24 |ref| (+ 2^-24 of the magnitudes per 0.2f
product / accumulate add of the epilogue), c = C_FACTOR = 1: what round-to-nearest fp32 accumulation gives.  Whether the matrix
core's internal accumulation meets c = 1 was MEASURED on the library before this test existed, heuristic tiles, on
BF16_CONV_CASES / BF16_DGRAD_CASES of tests/test_gpu_bf16.py: worst err / bound 0.016 (K = 4, 13 channels), so c stays 1.
bf16 output: bit-equal to the nearest-even rounding of the fp32 output of the same launch (no tolerance); against float64 one
bf16 spacing + the fp32 bound per element, and at most 1e-3 of a test function's elements differing from the once-rounded
reference at all (inputs chosen so that this is a fair condition: tests/test_bf16_ops_host.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _bf16_ops_np as R
import _elementwise_np as E
from _observed import record
from test_gpu_elementwise import Rows
from wave_u_net_amd import _lib

pytestmark = pytest.mark.gpu

C_FACTOR = 1.0
NAN = float("nan")
RAN = {key: set() for key in R.LEGAL}           # (mode, KT instantiation) -> tile codes that ran in the sweep
REFUSED_OK = {"n": 0}                           # forced codes the library refused


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sync():
    """Wait for the launch; a device fault ends the whole run here (nothing more is started on a faulted device)."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error, stopping: %s" % e, returncode=3)


def _same_bits(a, b):
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _rne_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).double().numpy()


def _in_rows(x, pitch, off, bf=True):
    """[B, C, T] -> rows of `pitch` elements whose first sample is `off` elements in; everything else in the row is NaN."""
    B, Cn, T = x.shape
    r = Rows(B * Cn, pitch, pitch, 0, bf)
    r.view[:, off:off + T] = torch.as_tensor(np.asarray(x, dtype=np.float32).reshape(B * Cn, T)).to(r.view.dtype).cuda()
    return r


def _out_rows(B, Cn, T, pitch, off, bf, prior=None):
    """Output rows whose first element is `off` elements behind a 16-byte aligned row start -> (Rows, pointer of the row start)."""
    r = Rows(B * Cn, T, pitch, off, bf, prior)
    return r, r.ptr - off * r.buf.element_size()


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _run(lib, c, inp, code, x_off=0, y_off=0, lrelu=0, mask=0, acc=None, dec=0, bf=0):
    """One wun_op_conv_bf16_ex launch under forced tile `code` (None: the heuristic).  -> None when the library refuses the code,
    else {"y": [B, N, Tout], "dec": [B, N0, (Tout + 1) // 2] or None} as float64, footprints checked."""
    f = R.desc_fields(c, x_off=x_off, y_off=y_off, lrelu=lrelu, acc=acc, dec=dec, out_bf16=bf)
    d = _lib.WunOpConvBf16Desc(**f)
    what = (tuple(c), code, x_off, y_off, bf)
    x0 = _in_rows(inp["x"][:, :c.C0], f["x0_pitch"], x_off)
    x1 = _in_rows(inp["x"][:, c.C0:], f["x1_pitch"], x_off) if c.C1 else None
    w, bias = _dev(inp["w"]), (None if inp["bias"] is None else _dev(inp["bias"]))
    split = c.N0 < c.N
    prior = inp["prior"] if acc is not None else None
    y0, p0 = _out_rows(c.B, c.N0, c.Tout, f["y0_pitch"], y_off, bf, None if prior is None else prior[:, :c.N0])
    y1, p1 = _out_rows(c.B, c.N - c.N0, c.Tout, f["y1_pitch"], y_off, bf, None if prior is None else prior[:, c.N0:]) if split else (None, None)
    m0 = m1 = pm0 = pm1 = None
    if mask:
        m0, pm0 = _out_rows(c.B, c.N0, c.Tout, f["y0_pitch"], y_off, bf, inp["mask"][:, :c.N0])
        if split:
            m1, pm1 = _out_rows(c.B, c.N - c.N0, c.Tout, f["y1_pitch"], y_off, bf, inp["mask"][:, c.N0:])
    dr = Rows(c.B * c.N0, (c.Tout + 1) // 2, f["dec_pitch"], 0, bf) if dec else None
    scr = torch.full((int(lib.wun_op_conv_bf16_ex_scratch(d)) + 4096,), NAN, device="cuda")
    if code is not None:
        lib.wun_op_force_conv_variant(_lib.BF16_VARIANT_BASE + code, 0)
    try:
        rc = lib.wun_op_conv_bf16_ex(d, x0.ptr, None if x1 is None else x1.ptr, w.data_ptr(), None if bias is None else bias.data_ptr(),
                                     p0, p1, pm0, pm1, None if dr is None else dr.ptr, scr.data_ptr(), _stream())
    finally:
        lib.wun_op_force_conv_variant(-1, 0)
    if rc == -2 and code is not None:
        _sync()
        assert np.isnan(y0.buf.float().cpu().numpy()).all() or prior is not None, ("a refused launch wrote", what)
        return None
    _lib.check(rc)
    _sync()
    y0.check_footprint(("y0",) + what)
    y = y0.get((c.B, c.N0, c.Tout))
    if split:
        y1.check_footprint(("y1",) + what)
        y = np.concatenate([y, y1.get((c.B, c.N - c.N0, c.Tout))], axis=1)
    out = {"y": y, "dec": None}
    if dr is not None:
        dr.check_footprint(("dec",) + what)
        out["dec"] = dr.get((c.B, c.N0, (c.Tout + 1) // 2))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# a. every tile code under every mode, inputs at an even and an odd first-element offset
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(R.SWEEP_CASES)), ids=[str(tuple(c)) for c in R.SWEEP_CASES])
def test_every_tile_code_against_float64(lib, ci):
    c = R.SWEEP_CASES[ci]
    key = (c.mode, R.kt_of(c.mode, R.taps_of(c)))
    inp = R.case_inputs(c)
    lrelu = int(c.mode != R.T2)
    ref, bound, _ = R.case_reference(c, inp, lrelu=lrelu, c_factor=C_FACTOR)
    worst, ran = 0.0, set()
    for x_off in (R.EVEN_OFF, R.ODD_OFF):
        d = _lib.WunOpConvBf16Desc(**R.desc_fields(c, x_off=x_off, lrelu=lrelu))
        for code in range(R.NCODES):
            legal = lib.wun_op_conv_bf16_choice_ok(d, code) == 1
            got = _run(lib, c, inp, code, x_off=x_off, lrelu=lrelu)
            assert (got is not None) == legal, ("forced code accepted / refused against conv_bf16_choice_ok", code, x_off)
            if got is None:
                REFUSED_OK["n"] += 1
                continue
            assert code in R.LEGAL[key], ("a code outside the reachable set ran", key, code)
            ratio = R.fp32_verdict(got["y"], ref, bound)
            print("[bf16 op] %s code %2d off %d err/bound %.4f" % (tuple(c), code, x_off, ratio))
            worst = max(worst, ratio)
            assert ratio <= 1, (code, x_off, ratio)
            # the bf16 store of the same launch: the nearest-even rounding of the fp32 output, bit for bit
            gb = _run(lib, c, inp, code, x_off=x_off, lrelu=lrelu, bf=1)
            assert gb is not None and _same_bits(gb["y"], _rne_bf16(got["y"])), ("bf16 store != RNE(fp32 output)", code, x_off)
            ran.add(code)
    RAN[key] |= ran
    record("op_conv_bf16_tile_sweep", "mode %d %s err/bound" % (c.mode, tuple(c)[2:]), worst, 1.0)
    assert ran, "no tile ran"


# ---------------------------------------------------------------------------------------------------------------------------
# b. the store paths: bf16 output exact against the fp32 output, both against float64
# ---------------------------------------------------------------------------------------------------------------------------
def test_store_paths_bf16_is_the_rounded_fp32_output(lib):
    pool = [0, 0]
    worst32 = {R.S1: 0.0, R.S2: 0.0, R.T2: 0.0}
    worst16 = dict(worst32)
    for sc in R.STORE_CASES:
        c = sc.case
        inp = R.case_inputs(c, grid=R.store_grid(sc))
        kw = dict(x_off=sc.x_off, y_off=sc.y_off, lrelu=sc.lrelu, mask=sc.mask, acc=sc.acc)
        ref, bound, big = R.case_reference(c, inp, c_factor=C_FACTOR, **kw)
        g32 = _run(lib, c, inp, sc.code, dec=sc.dec, bf=0, **kw)
        g16 = _run(lib, c, inp, sc.code, dec=sc.dec, bf=1, **kw)
        assert g32 is not None and g16 is not None, (sc.name, "forced code refused")
        r32 = R.fp32_verdict(g32["y"], ref, bound)
        print("[bf16 op] store %-22s fp32 err/bound %.4f" % (sc.name, r32))
        assert r32 <= 1, (sc.name, r32)
        # no tolerance: the bf16 launch stores RNE of what the fp32 launch stores (with accumulate: of fl32(prior + v), the same
        # bf16-representable prior given to both)
        assert _same_bits(g16["y"], _rne_bf16(g32["y"])), (sc.name, "bf16 store != RNE(fp32 output)")
        if sc.dec:
            n = (c.Tout + 1) // 2
            assert _same_bits(g16["dec"], g16["y"][:, :c.N0, 0::2][:, :, :n]), (sc.name, "bf16 compact copy != even positions")
            assert _same_bits(g32["dec"], g32["y"][:, :c.N0, 0::2][:, :, :n]), (sc.name, "fp32 compact copy != even positions")
        r16 = R.bf16_verdict(g16["y"], ref, big, bound, pool)
        print("[bf16 op] store %-22s bf16 err/bound %.4f" % (sc.name, r16))
        assert r16 <= 1, (sc.name, r16)
        worst32[c.mode], worst16[c.mode] = max(worst32[c.mode], r32), max(worst16[c.mode], r16)
    for mode in worst32:
        record("op_conv_bf16_store_paths", "mode %d fp32 err/bound" % mode, worst32[mode], 1.0)
        record("op_conv_bf16_store_paths", "mode %d bf16 err/bound" % mode, worst16[mode], 1.0)
    share = pool[0] / pool[1]
    record("op_conv_bf16_store_paths", "share of bf16 elements off the once-rounded reference", share, E.BF16_DIFF_SHARE)
    assert share <= E.BF16_DIFF_SHARE, pool


# ---------------------------------------------------------------------------------------------------------------------------
# c. first_conv_kernel: stride x channels x output type x tap instantiation
# ---------------------------------------------------------------------------------------------------------------------------
def _run_first(lib, fc, x, w, bias, bf, dec):
    Tin, shift = R.first_geometry(fc)
    B = R.FIRST_B
    xp, yp, dp = Tin + 3, (fc.Tout + 3) // 4 * 4 + 4, (fc.Tout + 1) // 2 + 3
    xr = Rows(B * fc.cin, Tin, xp, 0, False, x)
    yr = Rows(B * fc.N, fc.Tout, yp, 0, bf)
    dr = Rows(B * fc.N, (fc.Tout + 1) // 2, dp, 0, bf) if dec else None
    wd, bd = _dev(w), _dev(bias)
    _lib.check(lib.wun_op_first_conv(xr.ptr, wd.data_ptr(), bd.data_ptr(), yr.ptr, None if dr is None else dr.ptr, B, fc.cin, fc.N,
                                     fc.k, Tin, fc.Tout, fc.stride, shift, 1, int(bf), xp, yp, dp if dec else 0, _stream()))
    _sync()
    assert lib.wun_op_last_path(_lib.OP_FIRST_CONV) == _lib.PATH_FIRST_CONV
    yr.check_footprint(("first_conv y", fc, bf))
    y = yr.get((B, fc.N, fc.Tout))
    if dr is not None:
        # positions q >> 1 for even q < Tout only, and nothing past them
        dr.check_footprint(("first_conv dec", fc, bf))
        assert _same_bits(dr.get((B, fc.N, (fc.Tout + 1) // 2)), y[:, :, 0::2]), ("compact copy != even positions", fc, bf)
    return y


@pytest.mark.parametrize("stride, cin", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_first_conv_every_instantiation(lib, stride, cin):
    pool = [0, 0]
    worst32 = worst16 = 0.0
    seen = set()
    for fc in R.first_cases():
        if (fc.stride, fc.cin) != (stride, cin):
            continue
        c = R.first_as_case(fc)
        dec = (fc.N == 24)                                   # with and without the compact copy, at both lengths
        # ordinary fp32 operands: the (terms + 2) bound with c = 1 (plain fmaf), and the bf16 store against the fp32 one
        x, w, bias = R.first_inputs(fc)
        ref, bound, big = R.case_reference(c, {"x": x, "w": w, "bias": bias, "mask": None, "prior": None}, lrelu=True)
        y32 = _run_first(lib, fc, x, w, bias, 0, dec)
        r32 = R.fp32_verdict(y32, ref, bound)
        assert r32 <= 1, (fc, r32)
        y16 = _run_first(lib, fc, x, w, bias, 1, dec)
        assert _same_bits(y16, _rne_bf16(y32)), (fc, "bf16 store != RNE(fp32 output)")
        # operands on the fine grid: bf16 rows against float64
        x, w, bias = R.first_inputs(fc, grid=R.FINE)
        ref, bound, big = R.case_reference(c, {"x": x, "w": w, "bias": bias, "mask": None, "prior": None}, lrelu=True)
        g16 = _run_first(lib, fc, x, w, bias, 1, dec)
        r16 = R.bf16_verdict(g16, ref, big, bound, pool)
        assert r16 <= 1, (fc, r16)
        worst32, worst16 = max(worst32, r32), max(worst16, r16)
        seen |= {(fc.stride, fc.cin, ob, 15 if fc.k == 15 else 0) for ob in (0, 1)}
    assert len(seen) == 4                                    # bf16 / fp32 output x KT in {15, run-time} of this (SI, CIN)
    record("op_first_conv", "stride %d cin %d fp32 err/bound" % (stride, cin), worst32, 1.0)
    record("op_first_conv", "stride %d cin %d bf16 err/bound" % (stride, cin), worst16, 1.0)
    share = pool[0] / pool[1]
    record("op_first_conv", "stride %d cin %d share of bf16 elements off the reference" % (stride, cin), share, E.BF16_DIFF_SHARE)
    assert share <= E.BF16_DIFF_SHARE, pool


# ---------------------------------------------------------------------------------------------------------------------------
# d. the old entries under a forced code == the general entry, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
OLD_CONV_CASES = [(2, 24, 48, 15, 700, 1, 0, False), (2, 24, 48, 15, 701, 2, 0, False), (2, 40, 24, 5, 300, 1, 2, True)]
OLD_DGRAD_CASES = [(2, 96, 24, 7, 1000, 2)]                  # both from tests/test_gpu_bf16.py


def _old_conv(lib, x, w, b, B, Cin, Cout, K, T, t_out, stride, pad):
    y = torch.full((B, Cout, t_out), NAN, device="cuda")
    scr = torch.full((int(lib.wun_op_conv1d_bf16_scratch(Cin, Cout, K)) + 4096,), NAN, device="cuda")
    dx, dw, db = _dev(x), _dev(w), _dev(b)
    rc = lib.wun_op_conv1d_bf16(dx.data_ptr(), dw.data_ptr(), db.data_ptr(), y.data_ptr(), scr.data_ptr(), B, Cin, Cout, K, T, t_out,
                                stride, pad, 1, _stream())
    _sync()
    return rc, y.cpu().numpy().astype(np.float64)


def test_forced_codes_through_the_old_entries_equal_the_general_entry(lib):
    compared = 0
    for case in OLD_CONV_CASES:
        B, Cin, Cout, K, T, stride, pad, same = case
        rng = np.random.default_rng(R._seed(*[int(v) for v in case]))
        x = rng.uniform(-1, 1, (B, Cin, T)).astype(np.float32)
        w = (rng.uniform(-1, 1, (K, Cin, Cout)) / np.sqrt(K * Cin)).astype(np.float32)
        b = rng.uniform(-0.1, 0.1, Cout).astype(np.float32)
        t_out = T if same else (T - K) // stride + 1
        c = R.Case(R.S2 if stride == 2 else R.S1, B, Cin, 0, Cout, Cout, K, T, t_out, pad)
        inp = {"x": E.bf16_round(x), "w": w, "bias": b, "mask": None, "prior": None}
        rc, base = _old_conv(lib, x, w, b, B, Cin, Cout, K, T, t_out, stride, pad)
        _lib.check(rc)
        assert _same_bits(_run(lib, c, inp, None, lrelu=1)["y"], base), (case, "heuristic tile")
        for code in range(R.NCODES):
            lib.wun_op_force_conv_variant(_lib.BF16_VARIANT_BASE + code, 0)
            try:
                rc, old = _old_conv(lib, x, w, b, B, Cin, Cout, K, T, t_out, stride, pad)
            finally:
                lib.wun_op_force_conv_variant(-1, 0)
            new = _run(lib, c, inp, code, x_off=3, lrelu=1)
            assert (rc == -2) == (new is None), (case, code, rc)
            if new is None:
                assert np.isnan(old).all(), (case, code, "a refused launch wrote")
                continue
            _lib.check(rc)
            assert _same_bits(old, new["y"]), (case, code)
            compared += 1
        # a forced fp32 variant number is not for the bf16 entry ...
        lib.wun_op_force_conv_variant(3, 0)
        try:
            rc, old = _old_conv(lib, x, w, b, B, Cin, Cout, K, T, t_out, stride, pad)
        finally:
            lib.wun_op_force_conv_variant(-1, 0)
        _lib.check(rc)
        assert _same_bits(old, base), (case, "forced fp32 variant changed the bf16 entry")
    # ... and a forced bf16 code not for the fp32 entry
    B, Cin, Cout, K, T = 2, 24, 48, 15, 300
    rng = np.random.default_rng(5)
    x, w = _dev(rng.uniform(-1, 1, (B, Cin, T))), _dev(rng.uniform(-1, 1, (K, Cin, Cout)) / 19.0)
    outs = []
    for force in (-1, _lib.BF16_VARIANT_BASE + 9):
        y = torch.full((B, Cout, T - K + 1), NAN, device="cuda")
        lib.wun_op_force_conv_variant(force, 0)
        try:
            _lib.check(lib.wun_op_conv1d(x.data_ptr(), w.data_ptr(), None, y.data_ptr(), B, Cin, Cout, K, T, T - K + 1, 1, 0, 0, _stream()))
        finally:
            lib.wun_op_force_conv_variant(-1, 0)
        _sync()
        outs.append(y.cpu().numpy())
    assert np.isfinite(outs[0]).all() and np.array_equal(outs[0], outs[1])
    for case in OLD_DGRAD_CASES:
        B, Cin, Cout, K, T, stride = case
        t_out = (T - K) // stride + 1
        rng = np.random.default_rng(R._seed(*case))
        w = (rng.uniform(-1, 1, (K, Cin, Cout)) / np.sqrt(K * Cin)).astype(np.float32)
        dz = rng.uniform(-1, 1, (B, Cout, t_out)).astype(np.float32)
        c = R.Case(R.T2, B, Cout, 0, Cin, Cin, K, t_out, T, 0)
        inp = {"x": E.bf16_round(dz), "w": w, "bias": None, "mask": None, "prior": None}
        for code in [None] + list(range(R.NCODES)):
            gdx = torch.full((B, Cin, T), NAN, device="cuda")
            scr = torch.full((int(lib.wun_op_conv1d_dgrad_bf16_scratch(Cin, Cout, K)) + 4096,), NAN, device="cuda")
            dw, dzg = _dev(w), _dev(dz)
            if code is not None:
                lib.wun_op_force_conv_variant(_lib.BF16_VARIANT_BASE + code, 0)
            try:
                rc = lib.wun_op_conv1d_dgrad_bf16(dzg.data_ptr(), dw.data_ptr(), gdx.data_ptr(), scr.data_ptr(), B, Cin, Cout, K, T,
                                                  t_out, stride, 0, _stream())
            finally:
                lib.wun_op_force_conv_variant(-1, 0)
            _sync()
            new = _run(lib, c, inp, code, x_off=1)
            assert (rc == -2) == (new is None), (case, code, rc)
            if new is None:
                continue
            _lib.check(rc)
            assert _same_bits(gdx.cpu().numpy().astype(np.float64), new["y"]), (case, code)
            compared += 1
    assert compared >= 24


# ---------------------------------------------------------------------------------------------------------------------------
# last: the sweep reached every reachable (mode, tap instantiation, tile code) and nothing else was accepted
# ---------------------------------------------------------------------------------------------------------------------------
def test_every_reachable_code_ran_and_nothing_else_was_accepted():
    for key, want in R.LEGAL.items():
        print("[bf16 op] mode %d KT %2d ran codes %s" % (key[0], key[1], sorted(RAN[key])))
        assert RAN[key] == set(want), (key, "missing", sorted(set(want) - RAN[key]), "extra", sorted(RAN[key] - set(want)))
    record("op_conv_bf16_tile_sweep", "reachable (mode, KT, code) triples that ran / pinned", float(sum(len(v) for v in RAN.values())),
           float(sum(len(v) for v in R.LEGAL.values())))
    assert REFUSED_OK["n"] > 0
