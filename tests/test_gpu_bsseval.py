"""GPU tests of the BSS Eval scoring (include/wun.h: wun_bss_correlations, wun_bss_window_energies;
wave_u_net_amd.bsseval, evaluate.evaluate_track) against the float64 numpy oracle tests/_bsseval_np.py."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bsseval_np as ora  # noqa: E402
import test_bsseval_host as host  # noqa: E402  (the analytic cases and their checks)
from wave_u_net_amd import bsseval, evaluate  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
U = 2.0 ** -53

# End-to-end bound on |metric - oracle| in dB: 10 x the largest difference observed on these inputs on an MI355X, never above
# 0.005 dB (half the second decimal the reference reports).  The device and the oracle sum in different orders and solve with
# different LAPACK builds.  Observed values are beside the constants and in DESIGN.md 5.9.
E2E_CAP = 0.005
E2E_TOL_WHITE = 7.2e-12       # observed 7.11e-13 dB (white, S=2 C=2 L=512, and coloured, S=2 C=1 L=32)
E2E_TOL_REALISTIC = 1.9e-11   # observed 1.88e-12 dB (low-passed noise + partials, S=2 C=2 L=512)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


def make_signals(S, n, C, seed, kind="white"):
    """References and estimates [S, n, C] float32: estimates = filtered references + leakage from the other sources + noise."""
    rng = np.random.RandomState(seed)
    refs = rng.randn(S, n, C)
    if kind == "realistic":                      # low-passed, music-like: a strongly coloured spectrum and a few decaying partials
        from scipy.signal import lfilter
        t = np.arange(n)
        for j in range(S):
            for c in range(C):
                x = lfilter([1.0], [1.0, -1.8, 0.82], refs[j, :, c])            # two real poles near z = 0.9: ~ -60 dB at Nyquist
                x = x / x.std()
                for f in (0.011 * (j + 1), 0.023 * (c + 1) + 0.004 * j):
                    x = x + 0.7 * np.sin(2 * np.pi * f * t + rng.rand()) * (0.5 + 0.5 * np.cos(2 * np.pi * t / (n / 3.0 + 17 * j)))
                refs[j, :, c] = 0.2 * x
    elif kind == "coloured":
        refs = refs + 0.5 * np.roll(refs, 1, axis=1)
    ests = np.zeros_like(refs)
    for j in range(S):
        e = refs[j] + 0.3 * np.roll(refs[j], 3, axis=0) * (np.arange(n)[:, None] >= 3)
        for k in range(S):
            if k != j:
                e = e + 0.1 * refs[k][:, ::-1]
        ests[j] = e + 0.05 * refs.std() * rng.randn(n, C)
    return refs.astype(np.float32), ests.astype(np.float32)


# ---- correlations ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsel", ["L-1", "4099", "1000003"])
@pytest.mark.parametrize("L", [1, 32, 512])
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("S", [1, 2, 4])
def test_correlations_against_oracle(S, C, L, nsel):
    n = L - 1 if nsel == "L-1" else int(nsel)
    if n < 1:                                    # L = 1: n = 0 is not a signal -- the entry refuses it before any GPU work
        z = torch.zeros((S, 1, C), device=DEV)
        with pytest.raises(ValueError):
            bsseval.correlations(z[:, :0], z[:, :0], L, scratch=torch.zeros(8, dtype=torch.float64, device=DEV))
        return
    refs, ests = make_signals(S, n, C, seed=S * 100 + C * 10 + L)
    R, D = bsseval.correlations(_dev(refs), _dev(ests), L)
    R, D = R.cpu().numpy(), D.cpu().numpy()
    Ro, Do = ora.correlations(refs, ests, L)
    es = np.sum(ora._signals(refs) ** 2, axis=1)
    ee = np.sum(ora._signals(ests) ** 2, axis=1)
    bound_r = n * U * np.sqrt(es[:, None] * es[None, :])[:, :, None]
    bound_d = n * U * np.sqrt(es[:, None] * ee[None, :])[:, :, None]
    print("corr S=%d C=%d L=%d n=%d: max err / bound  R %.3g  D %.3g" % (
        S, C, L, n, (np.abs(R - Ro) / bound_r).max(), (np.abs(D - Do) / bound_d).max()))
    assert (np.abs(R - Ro) <= bound_r).all()
    assert (np.abs(D - Do) <= bound_d).all()


# ---- energies with the oracle's filters fed in -------------------------------------------------------------------------
@pytest.mark.parametrize("S, C, L, n, W", [(1, 1, 1, 1000, 300), (2, 2, 32, 4099, 1000), (2, 2, 512, 9000, 2000),
                                           (4, 2, 32, 3000, 700), (3, 1, 512, 2500, 0)])
def test_energies_against_oracle_with_its_filters(S, C, L, n, W):
    refs, ests = make_signals(S, n, C, seed=7 + S + L)
    Ro, Do = ora.correlations(refs, ests, L)
    c_all, c_own = ora.filters(Ro, Do, S, C)
    starts, lengths = ora.windows(n, W, W)
    want = ora.window_energies(refs, ests, starts, lengths, c_all, c_own)
    got = bsseval.window_energies(_dev(refs), _dev(ests), starts, lengths,
                                  torch.from_numpy(c_all).to(DEV), torch.from_numpy(c_own).to(DEV)).cpu().numpy()
    # every energy is a sum of squares of combinations of s, est, P_own, P_all; the energies of the same chain on absolute
    # values bound what any rounding can move: (|s| + |est| + |P_own| + |P_all|)^2 <= 4 (sum of the four squares)
    ab = ora.window_energies(np.abs(refs), np.abs(ests), starts, lengths, np.abs(c_all), np.abs(c_own))
    scale = 4.0 * (ab[:, :, 0] + ab[:, :, 1] + ab[:, :, 4] + ab[:, :, 6])
    A = S * C
    terms = np.array([(w + L - 1) * C for w in lengths], np.float64)[:, None] + 2.0 * (A * L + 2)
    bound = (terms * U * scale)[:, :, None]
    print("energies S=%d C=%d L=%d: max err / bound %.3g" % (S, C, L, (np.abs(got - want) / bound).max()))
    assert (np.abs(got - want) <= bound).all()
    # the filter-free form: energies 0..2, the rest zero
    free = bsseval.window_energies(_dev(refs), _dev(ests), starts, lengths, filters_len=L).cpu().numpy()
    want3 = ora.window_energies(refs, ests, starts, lengths)
    b3 = (np.array(lengths, np.float64)[:, None] * C * U * scale)[:, :, None]
    assert (np.abs(free[:, :, :3] - want3[:, :, :3]) <= b3).all() and (free[:, :, 3:] == 0).all()


# ---- analytic cases on the device path ------------------------------------------------------------------------------
def test_case1_sdr_identity():
    refs, ests = host.analytic_case3()
    ests = ests + np.float32(0.01) * np.random.RandomState(5).randn(*ests.shape).astype(np.float32)
    m = bsseval.bss_eval(refs, ests, 1000, filters_len=host.L0, device=DEV)
    st, ln = ora.windows(host.N0, 1000, 1000)
    host.check_case1(m, refs, ests, st, ln)
    only = bsseval.bss_eval(refs, ests, 1000, filters_len=host.L0, metrics=("SDR",), device=DEV)
    assert np.abs(only["SDR"] - m["SDR"]).max() < 1e-9


@pytest.mark.parametrize("L", [32, 512])
def test_case2_filtered_copy(L):
    refs, ests = host.analytic_case2(L=L)
    check = ora.bss_eval(refs, ests, 1000, window=None, filters_len=L)
    print("case 2 L=%d oracle: SAR %.1f ISR-SDR %.3g" % (L, check["SAR"][0, 0], check["ISR"][0, 0] - check["SDR"][0, 0]))
    m = bsseval.bss_eval(refs, ests, 1000, window=None, filters_len=L, device=DEV)
    print("case 2 L=%d device: SAR %.1f ISR-SDR %.3g SIR %s" % (L, m["SAR"][0, 0], m["ISR"][0, 0] - m["SDR"][0, 0], m["SIR"][0, 0]))
    host.check_case2(m)


def test_case3_known_leak():
    refs, ests = host.analytic_case3()
    m = bsseval.bss_eval(refs, ests, host.N0 // 6, filters_len=host.L0, device=DEV)
    print("case 3 device: SAR min %.1f  SIR-SDR %s  ISR-SDR min %.1f" % (
        m["SAR"].min(), np.round(m["SIR"][0] - m["SDR"][0], 4), (m["ISR"][0] - m["SDR"][0]).min()))
    host.check_case3(m)


def test_case4_silent_windows():
    refs, ests = host.silent_case()
    host.check_case4(bsseval.bss_eval(refs, ests, 1000, filters_len=host.L0, device=DEV))
    host.check_case4(bsseval.bss_eval(refs, ests, 1000, metrics=("SDR",), device=DEV))


# ---- end to end ---------------------------------------------------------------------------------------------------
def _end_to_end(kind, S, C, n, sr, L, seed):
    refs, ests = make_signals(S, n, C, seed, kind)
    if kind != "realistic":
        ests[0, 2 * sr:3 * sr] = 0.0                          # one silent estimate window: the NaN pattern
    want = ora.bss_eval(refs, ests, sr, filters_len=L)
    got = bsseval.bss_eval(refs, ests, sr, filters_len=L, device=DEV)
    worst = 0.0
    for m in bsseval.METRICS:
        assert got[m].shape == want[m].shape
        np.testing.assert_array_equal(np.isnan(got[m]), np.isnan(want[m]))
        np.testing.assert_array_equal(np.isposinf(got[m]), np.isposinf(want[m]))
        fin = np.isfinite(want[m])
        assert np.isfinite(got[m][fin]).all()
        if fin.any():
            worst = max(worst, float(np.abs(got[m][fin] - want[m][fin]).max()))
    return worst


def test_end_to_end_well_conditioned():
    worst = max(_end_to_end("white", 2, 2, 6 * 8000 + 2400, 8000, 512, 11),
                _end_to_end("coloured", 2, 1, 5 * 4000 + 100, 4000, 32, 12))
    print("end to end, well conditioned: max |dB - oracle| = %.3g (bound %.3g)" % (worst, E2E_TOL_WHITE))
    assert E2E_TOL_WHITE <= E2E_CAP and worst <= E2E_TOL_WHITE


def test_end_to_end_realistic():
    worst = _end_to_end("realistic", 2, 2, 6 * 8000 + 2400, 8000, 512, 13)
    print("end to end, realistic: max |dB - oracle| = %.3g (bound %.3g)" % (worst, E2E_TOL_REALISTIC))
    assert E2E_TOL_REALISTIC <= E2E_CAP and worst <= E2E_TOL_REALISTIC


# ---- determinism --------------------------------------------------------------------------------------------------
def _repro_digest(offset):
    """sha256 over the correlation and energy bits of one fixed call, the track placed `offset` frames into a larger buffer."""
    S, n, C, L = 2, 40000, 2, 64
    refs, ests = make_signals(S, n, C, seed=21)
    big_r = torch.zeros((S * n * C + 4096,), device=DEV)
    big_e = torch.zeros((S * n * C + 4096,), device=DEV)
    r = big_r[offset:offset + S * n * C].view(S, n, C)
    e = big_e[offset:offset + S * n * C].view(S, n, C)
    r.copy_(_dev(refs)); e.copy_(_dev(ests))
    R, D = bsseval.correlations(r, e, L)
    c_all, c_own = bsseval.solve_filters(R, D, S, C)
    st, ln = bsseval.window_table(n, 9000, 9000)
    E = bsseval.window_energies(r, e, st, ln, c_all, c_own)
    E0 = bsseval.window_energies(r, e, st, ln)
    h = hashlib.sha256()
    for t in (R, D, E, E0):
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


def test_bit_reproducible_across_calls_offsets_and_processes():
    a = _repro_digest(0)
    assert _repro_digest(0) == a                              # the same call twice
    assert _repro_digest(1) == a and _repro_digest(1003) == a  # other buffer offsets (4-byte and odd alignments)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "digest"], capture_output=True, text=True, timeout=600,
                       cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == a             # a fresh process


def test_sdr_alone_computes_no_correlations(monkeypatch):
    refs, ests = make_signals(2, 9000, 2, seed=31)
    before = dict(bsseval.LAUNCHES)

    def boom(*a, **k):
        raise AssertionError("the filters were asked for")
    monkeypatch.setattr(bsseval, "solve_filters", boom)
    monkeypatch.setattr(bsseval, "correlations", boom)
    m = bsseval.bss_eval(refs, ests, 3000, metrics=("SDR",), device=DEV)
    assert bsseval.LAUNCHES["correlations"] == before["correlations"]
    assert bsseval.LAUNCHES["energies"] == before["energies"] + 1
    want = ora.bss_eval(refs, ests, 3000, metrics=("SDR",))
    assert np.abs(m["SDR"] - want["SDR"]).max() < 1e-9


# ---- the reference's callers ------------------------------------------------------------------------------------------
def test_evaluate_track_writes_museval_json(tmp_path):
    import wave_u_net_amd as wun
    from wave_u_net_amd.separator import UnetAudioSeparator
    cfg = wun.get_config("baseline_stereo", num_layers=3, num_initial_filters=4, num_frames=1024, expected_sr=8000)
    sep = UnetAudioSeparator(cfg, device=DEV)
    names = list(cfg["source_names"])
    sr, n = 8000, 3 * 8000 + 500
    rng = np.random.RandomState(41)
    stems = {k: (0.3 * rng.randn(n, 2)).astype(np.float32) for k in names}
    mix = sum(stems.values()).astype(np.float32)
    scores = evaluate.evaluate_track(cfg, sep, mix, stems, sr, results_dir=str(tmp_path), name="song", filters_len=64)
    path = os.path.join(str(tmp_path), "song.json")
    assert os.path.exists(path)
    js = json.load(open(path))
    assert [t["name"] for t in js["targets"]] == names
    for j, t in enumerate(js["targets"]):
        assert len(t["frames"]) == 3
        for k, fr in enumerate(t["frames"]):
            assert fr["time"] == float(k) and fr["duration"] == 1.0
            assert set(fr["metrics"]) == {"SDR", "SIR", "ISR", "SAR"}
            for m in bsseval.METRICS:
                assert fr["metrics"][m] == scores[m][j, k]
    est = evaluate.separate_track(cfg, sep, mix, sr)
    ref = np.stack([stems[k] for k in names])
    again = bsseval.bss_eval(ref, np.stack([est[k] for k in names]), sr, filters_len=64, device=DEV)
    for m in bsseval.METRICS:
        np.testing.assert_array_equal(again[m], scores[m])
    dev = evaluate.separate_track(cfg, sep, mix, sr, return_device=True)
    assert dev.is_cuda and tuple(dev.shape) == (len(names), n, 2)
    for j, k in enumerate(names):
        assert np.array_equal(dev[j].cpu().numpy(), est[k])
    stats = evaluate.compute_mean_metrics(str(tmp_path))
    assert len(stats) == len(names)
    for j, (med, mad, mean, sd) in enumerate(stats):
        assert med == np.nanmedian(scores["SDR"][j]) and np.isfinite([mad, mean, sd]).all()


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "digest":
    print(_repro_digest(0))
