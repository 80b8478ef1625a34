"""CPU-only checks of the BSS Eval scoring (include/wun.h: wun_bss_windows, wun_bss_scratch_doubles, wun_bss_correlations,
wun_bss_window_energies; wave_u_net_amd.bsseval): the window table, argument errors before any GPU work, the
museval-style JSON and the reference's statistics over it, and the analytic cases of the definition on the float64 oracle
(tests/_bsseval_np.py).  The same analytic cases run on the device path in tests/test_gpu_bsseval.py."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bsseval_np as ora  # noqa: E402
from wave_u_net_amd import _lib, bsseval, evaluate  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wun_bss_windows", "wun_bss_scratch_doubles", "wun_bss_correlations", "wun_bss_window_energies")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_declared_exported_and_documented(lib):
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in doc, name


# ---- window table --------------------------------------------------------------------------
@pytest.mark.parametrize("n, W, H, starts, lengths", [
    (3, 4, 4, [0], [3]),                               # n < W: one window over everything
    (12, 4, 4, [0, 4, 8], [4, 4, 4]),                  # exact multiple
    (14, 4, 4, [0, 4, 8], [4, 4, 6]),                  # remainder: the last window is extended
    (4, 4, 4, [0], [4]),
    (11, 4, 2, [0, 2, 4, 6], [4, 4, 4, 5]),            # overlapping hops
    (9, 0, 0, [0], [9]),                               # no windowing
])
def test_window_table(n, W, H, starts, lengths):
    assert bsseval.window_table(n, W, H) == (starts, lengths)
    assert ora.windows(n, W, H) == (starts, lengths)
    if W:
        nwin = (n - W + H) // H if n >= W else 1
        assert len(starts) == nwin


def test_window_table_rule_against_the_oracle():
    rng = np.random.RandomState(0)
    for _ in range(200):
        n, W, H = int(rng.randint(1, 500)), int(rng.randint(1, 60)), int(rng.randint(1, 60))
        s, l = bsseval.window_table(n, W, H)
        assert (s, l) == ora.windows(n, W, H)
        assert s[-1] + l[-1] == n


def test_window_table_errors(lib):
    st = (C.c_int64 * 4)()
    assert lib.wun_bss_windows(0, 4, 4, None, None, 0) == -1
    assert lib.wun_bss_windows(10, -1, 4, None, None, 0) == -1
    assert lib.wun_bss_windows(10, 4, 0, None, None, 0) == -1
    assert lib.wun_bss_windows(10, 4, 4, st, None, 4) == -1
    assert lib.wun_bss_windows(100, 4, 4, st, st, 4) == -1          # cap below the count
    with pytest.raises(ValueError):
        bsseval.window_table(0, 4, 4)


# ---- ABI argument errors: all before any GPU work (there is no GPU here) ------------------------
def test_scratch_query(lib):
    n, S, Cc, L = 100000, 2, 2, 512
    A = S * Cc
    corr = -(-n // 16384) * A * 2 * A * L
    assert lib.wun_bss_scratch_doubles(S, n, Cc, L, 0, 0) == corr
    en = 64 * S * -(-(44100 + L - 1) // 256) * 8
    assert lib.wun_bss_scratch_doubles(S, n, Cc, 1, 100, 44100) == max(-(-n // 16384) * A * 2 * A, 64 * S * -(-44100 // 256) * 8)
    assert lib.wun_bss_scratch_doubles(S, n, Cc, L, 100, 44100) == max(corr, en)
    for bad in ((0, n, Cc, L, 1, 1), (S, 0, Cc, L, 1, 1), (S, n, 3, L, 1, 1), (S, n, Cc, 0, 1, 1), (S, n, Cc, 513, 1, 1),
                (S, n, Cc, L, -1, 1), (S, n, Cc, L, 1, n + 1)):
        assert lib.wun_bss_scratch_doubles(*bad) == -1, bad


def test_entries_refuse_bad_arguments_before_gpu_work(lib):
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)                        # a non-null (host) pointer: never dereferenced by a refused call
    ok = dict(S=2, n=1000, Cc=2, L=32)

    def corr(refs=p, ests=p, R=p, D=p, scratch=p, **kw):
        a = dict(ok, **kw)
        return lib.wun_bss_correlations(refs, ests, a["S"], a["n"], a["Cc"], a["L"], R, D, scratch, None)

    for kw in (dict(refs=None), dict(ests=None), dict(R=None), dict(D=None), dict(scratch=None), dict(S=0), dict(Cc=0),
               dict(Cc=3), dict(L=0), dict(L=513), dict(n=0)):
        assert corr(**kw) == -1, kw
        assert lib.wun_last_error()

    st, ln = (C.c_int64 * 2)(0, 500), (C.c_int64 * 2)(500, 500)

    def en(refs=p, ests=p, c_all=p, c_own=p, starts=st, lengths=ln, nwin=2, out=p, scratch=p, **kw):
        a = dict(ok, **kw)
        return lib.wun_bss_window_energies(refs, ests, a["S"], a["n"], a["Cc"], a["L"], c_all, c_own, starts, lengths, nwin,
                                           out, scratch, None)

    for kw in (dict(refs=None), dict(ests=None), dict(starts=None), dict(lengths=None), dict(out=None), dict(scratch=None),
               dict(c_all=None), dict(c_own=None), dict(S=0), dict(Cc=4), dict(L=0), dict(L=600), dict(n=0), dict(nwin=0),
               dict(lengths=(C.c_int64 * 2)(500, 501)), dict(starts=(C.c_int64 * 2)(-1, 500)),
               dict(lengths=(C.c_int64 * 2)(0, 500))):
        assert en(**kw) == -1, kw
    # the staging limit of the projection: more than 8 reference signals, with filters only
    assert en(S=5, Cc=2) == -2
    assert en(S=9, Cc=1) == -2
    assert b"8 reference signals" in lib.wun_last_error()


def test_bss_eval_refuses_cpu_and_unknown_metrics():
    x = np.zeros((1, 100, 1), np.float32)
    with pytest.raises(ValueError):
        bsseval.bss_eval(x, x, 100, metrics=("SNR",))
    with pytest.raises(RuntimeError):
        bsseval.bss_eval(x, x, 100, device="cpu")


# ---- metrics from energies, JSON, statistics ------------------------------------------------------
def test_metrics_from_energies_nan_and_inf_rules():
    E = np.ones((3, 2, 8))
    E[:, :, 0] = 100.0
    E[1, 0, 1] = 0.0             # window 1: source 0's estimate is silent -> NaN for both sources
    E[2, 1, 5] = 0.0             # window 2: no interference in source 1 -> SIR = +inf
    got = bsseval.metrics_from_energies(E)
    want = ora.metrics_from_energies(E)
    for m in bsseval.METRICS:
        assert got[m].shape == (2, 3) and got[m].dtype == np.float64
        np.testing.assert_array_equal(got[m], want[m])
        assert np.isnan(got[m][:, 1]).all() and not np.isnan(got[m][:, [0, 2]]).any()
    assert got["SDR"][0, 0] == 20.0 and np.isposinf(got["SIR"][1, 2]) and got["SIR"][0, 2] == 0.0


def _write(folder, name, per_source):
    scores = {m: np.array(per_source, np.float64) + i for i, m in enumerate(bsseval.METRICS)}
    return bsseval.write_track_json(os.path.join(folder, name), ["accompaniment", "vocals"], scores)


def test_json_round_trip_and_mean_metrics(tmp_path):
    d = str(tmp_path)
    _write(d, "a.json", [[1.0, 2.0, np.nan], [5.0, np.inf, 7.0]])
    _write(d, "b.json", [[3.0, np.nan], [9.0, 11.0]])
    _write(d, "test.json", [[1000.0], [1000.0]])                      # skipped (Evaluate.py:213-215)
    js = json.load(open(os.path.join(d, "a.json")))
    assert [t["name"] for t in js["targets"]] == ["accompaniment", "vocals"]
    fr = js["targets"][0]["frames"]
    assert [f["time"] for f in fr] == [0.0, 1.0, 2.0] and all(f["duration"] == 1.0 for f in fr)
    assert set(fr[0]["metrics"]) == {"SDR", "SIR", "ISR", "SAR"}
    assert fr[0]["metrics"]["SDR"] == 1.0 and fr[0]["metrics"]["ISR"] == 2.0
    assert np.isnan(fr[2]["metrics"]["SDR"]) and np.isposinf(js["targets"][1]["frames"][1]["metrics"]["SDR"])

    segs = evaluate.compute_mean_metrics(d, compute_averages=False)
    assert len(segs) == 2
    np.testing.assert_array_equal(np.sort(segs[0][~np.isnan(segs[0])]), [1.0, 2.0, 3.0])
    assert np.isnan(segs[0]).sum() == 2 and 1000.0 not in segs[0]
    med, mad, mean, sd = evaluate.compute_mean_metrics(d)[0]
    assert (med, mad) == (2.0, 1.0) and mean == 2.0 and abs(sd - np.std([1.0, 2.0, 3.0])) < 1e-15
    med, mad, mean, sd = evaluate.compute_mean_metrics(d, metric="SAR")[0]
    assert med == 5.0                                                    # SAR was written as SDR + 3


# ---- the analytic cases of the definition, on the oracle (L = 32, n = 6000) -------------------------------------------
# Inputs are float32 by contract, and SAR >= 200 dB needs estimates that lie EXACTLY in the span of the filtered references: a
# float32 rounding of the estimate is itself an artifact at -144 dB.  So the white noise is drawn on a grid of 2^-8, the FIR
# taps are powers of two and the leak is 51/512 = 0.0996 (0.1 to 9 bits): every estimate sample is then exact in float32.
L0, N0 = 32, 6000
LEAK = 51.0 / 512.0


def _white(rng, *shape):
    return np.round(rng.randn(*shape) * 256.0) / 256.0


def analytic_case2(L=L0, n=N0, seed=2):
    rng = np.random.RandomState(seed)
    s = _white(rng, n)
    s[n - (L - 1):] = 0.0
    h = np.zeros(L - 1)
    h[[0, 3, (L - 1) // 2, L - 2]] = [1.0, -0.5, 0.25, 0.125]
    est = np.convolve(s, h)[:n]
    assert (est.astype(np.float32) == est).all()
    return s.astype(np.float32)[None, :, None], est.astype(np.float32)[None, :, None]


def analytic_case3(n=N0, seed=4):
    """The bounds on SIR - SDR are properties of a draw, not of every draw: over seeds 3..11 the float64 oracle gives a minimum
    over the six windows between -0.020 and +0.005 dB (the finite-sample correlation of the two sources moves P_own); seeds 4
    and 9 meet the (0, 0.1) dB interval on the oracle, and the case is pinned to seed 4."""
    rng = np.random.RandomState(seed)
    s = _white(rng, 2, n, 1)
    est = s.copy()
    est[0] = s[0] + LEAK * s[1]
    assert (est.astype(np.float32) == est).all()
    return s.astype(np.float32), est.astype(np.float32)


def check_case1(got, refs, ests, starts, lengths):
    for k, (t0, w) in enumerate(zip(starts, lengths)):
        for j in range(refs.shape[0]):
            s = refs[j, t0:t0 + w].astype(np.float64)
            e = ests[j, t0:t0 + w].astype(np.float64)
            want = 10 * np.log10(np.sum(s ** 2) / np.sum((e - s) ** 2))
            assert abs(got["SDR"][j, k] - want) < 1e-9, (j, k, got["SDR"][j, k], want)


def check_case2(m):
    assert m["SDR"].shape == (1, 1)
    assert abs(m["ISR"][0, 0] - m["SDR"][0, 0]) < 1e-9
    assert np.isposinf(m["SIR"][0, 0])
    assert m["SAR"][0, 0] >= 200.0, m["SAR"]


def check_case3(m):
    assert m["SDR"].shape == (2, 6)
    assert (m["SAR"] >= 200.0).all(), m["SAR"]
    d = m["SIR"][0] - m["SDR"][0]
    assert ((d > 0) & (d < 0.1)).all(), d
    assert (m["ISR"][0] > m["SDR"][0] + 10.0).all(), (m["ISR"][0], m["SDR"][0])


def test_oracle_case1_sdr_identity():
    refs, ests = analytic_case3()
    ests = ests + np.float32(0.01) * np.random.RandomState(5).randn(*ests.shape).astype(np.float32)
    m = ora.bss_eval(refs, ests, 1000, filters_len=L0)
    st, ln = ora.windows(N0, 1000, 1000)
    check_case1(m, refs, ests, st, ln)
    only = ora.bss_eval(refs, ests, 1000, filters_len=L0, metrics=("SDR",))
    assert np.abs(only["SDR"] - m["SDR"]).max() < 1e-9


def test_oracle_case2_filtered_copy():
    refs, ests = analytic_case2()
    check_case2(ora.bss_eval(refs, ests, 1000, window=None, filters_len=L0))


def test_oracle_case3_known_leak():
    refs, ests = analytic_case3()
    check_case3(ora.bss_eval(refs, ests, N0 // 6, filters_len=L0))


def silent_case(n=N0, seed=4):
    rng = np.random.RandomState(seed)
    refs = rng.randn(2, n, 2).astype(np.float32)
    ests = (refs + 0.1 * rng.randn(2, n, 2)).astype(np.float32)
    refs[1, 1000:2000] = 0.0          # window 1: one reference silent
    ests[0, 4000:5000] = 0.0          # window 4: one estimate silent
    return refs, ests


def check_case4(m):
    for name, v in m.items():
        assert np.isnan(v[:, [1, 4]]).all(), name
        assert np.isfinite(v[:, [0, 2, 3, 5]]).all(), name


def test_oracle_case4_silent_windows():
    refs, ests = silent_case()
    check_case4(ora.bss_eval(refs, ests, 1000, filters_len=L0))
