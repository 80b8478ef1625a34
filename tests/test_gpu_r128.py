"""GPU tests of the rest of the EBU R 128 meter (include/wun.h: wun_true_peak, wun_loudness_r128; wave_u_net_amd.loudness:
true_peak, r128, the true_peak_limit key) against the resampler kernel (bit for bit) and the float64 numpy
oracle tests/_r128_np.py.

Tolerances.  True peak: the device value IS the maximum of the resampler's output (compared bit for bit); against the float64
oracle it may differ by what tests/test_gpu_resample.py allows the resampler itself, the largest elementwise bound
(K + 2) 2^-24 (|h| * |v|)[t] + 2^-24 |y64[t]|.  Short-term blocks: the bound tests/test_gpu_loudness.py forms for the 0.4 s blocks
with N3 for Nb -- e = 4 x the error the numpy emulation of the chunked schedule shows against the serial recurrence, a block's
mean square moves by at most sum_c 2 sqrt(ms_c) e_c + e_c^2, plus N3 2^-53 relative for another order of the N3 squares; in LU
-10 log10(1 - tol_z / z).  The loudness range is a difference of two block values: the sum of their two tolerances."""
import numpy as np
import pytest
import torch

import _loudness_np as ora
import _observed
import _r128_np as r128o
from _unaligned import _offset_copy
from test_gpu_loudness import SR, _separator
from test_gpu_resample import _abs_filter

from wave_u_net_amd import loudness
from wave_u_net_amd import resample as rs
from wave_u_net_amd.evaluate import separate_track

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LIMIT = 10.0 ** (-1.0 / 20.0)                     # -1 dBTP


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _i64(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _noise(n, C, seed=0, amp=0.25):
    return (amp * np.random.RandomState(seed).randn(n, C)).astype(np.float32)


def _sine45(n, C=1, amp=1.0):
    """A quarter-rate sine sampled at 45 degrees: every sample +-0.7071 amp, the waveform reaches amp between them."""
    return np.tile((amp * np.sin(2 * np.pi * 0.25 * np.arange(n) + np.pi / 4))[:, None], [1, C]).astype(np.float32)


def _peak_input(kind, n, C):
    if kind == "noise":
        return _noise(n, C, 100 + n + C, 0.5)
    if kind == "sine45":
        x = _sine45(n, C)
        if C == 2:
            x[:, 1] *= np.float32(0.5)
        return x
    x = np.zeros((n, C), np.float32)                # the halo on either side: an impulse at the first / the last frame
    x[0 if kind == "impulse_first" else n - 1] = [1.0, -0.75][:C]
    return x


def _resampled(x, L):
    """wun_resample of x [n, C] by L / 1, per channel, all n L frames: the signal whose maximum the true peak is."""
    y = torch.empty((x.shape[0] * L, x.shape[1]), dtype=torch.float32, device=x.device)
    return rs.resample_into(x, y, 0, y.shape[0], L, 1)


# ---- the true peak is the resampler's maximum ----------------------------------------------------
@pytest.mark.parametrize("sr", [48000, 96000, 8000, 192000])              # L = 4, 2, 32, 1
def test_true_peak_is_the_resamplers_maximum_bit_for_bit(sr):
    L = loudness.oversampling(sr)
    K = rs.design(L, 1).shape[1] if L > 1 else 1
    worst = 0.0
    for n in (1, 2, 255, 256, 257, 805, 2000):
        for C in (1, 2):
            for kind in ("noise", "impulse_first", "impulse_last", "sine45"):
                xh = _peak_input(kind, n, C)
                x = _dev(xh)
                tp = loudness.true_peak(x, sr)
                assert tp.shape == (1 + C,) and tp.dtype == torch.float64
                y = _resampled(x, L)
                want = y.abs().amax(dim=0).double()
                assert torch.equal(_i64(tp[1:]), _i64(want)), (sr, n, C, kind, tp, want)       # per channel
                assert torch.equal(_i64(tp[0:1]), _i64(y.abs().max().double().reshape(1))), (sr, n, C, kind)
                if L == 1:
                    assert tp[0].item() == float(np.max(np.abs(xh)))                             # the sample peak
                # against the float64 oracle: the resampler's own elementwise bound, at its largest
                ref, per = r128o.true_peak(xh, sr)
                tol = 0.0
                if L > 1:
                    from scipy.signal import resample_poly
                    v = xh.astype(np.float64)
                    mag = resample_poly(np.abs(v), L, 1, axis=0, window=_abs_filter(L, 1))
                    tol = float(np.max((K + 2) * 2.0 ** -24 * mag + 2.0 ** -24 * np.abs(resample_poly(v, L, 1, axis=0))))
                got = tp.cpu().numpy()
                err = max(abs(got[0] - ref), float(np.max(np.abs(got[1:] - per))))
                worst = max(worst, err / tol if tol else err)
                assert err <= tol, (sr, n, C, kind, err, tol)
    _observed.record("test_gpu_r128.true_peak_vs_float64", "sr=%d L=%d" % (sr, L), worst, 1.0)


def test_true_peak_of_the_45_degree_sine_reads_over_full_scale():
    x = _dev(_sine45(2000))
    for sr in (48000, 8000):                                                # L = 4 and L = 32
        tp = loudness.true_peak(x, sr).cpu().numpy()
        assert 1.00 <= tp[0] <= 1.03 and abs(tp[0] - 1.0134) < 1e-3 and tp[1] == tp[0]
    assert abs(loudness.true_peak(x, 192000)[0].item() - 0.70711) < 1e-5   # L = 1: the sample peak


# ---- true peak hygiene -----------------------------------------------------------------------------
def test_true_peak_nan_and_inf():
    for sr in (48000, 192000):
        x = _noise(1500, 2, 30)
        x[700, 1] = np.nan
        tp = loudness.true_peak(_dev(x), sr).cpu().numpy()
        assert np.isnan(tp[0]) and np.isnan(tp[2]) and np.isfinite(tp[1])
        x[700, 1] = np.inf
        tp = loudness.true_peak(_dev(x), sr).cpu().numpy()
        assert tp[0] == np.inf and tp[2] == np.inf and np.isfinite(tp[1])
        x[700, 1] = -np.inf
        x[1499, 0] = np.nan                                                  # a NaN outweighs an infinity
        tp = loudness.true_peak(_dev(x), sr).cpu().numpy()
        assert np.isnan(tp[0]) and np.isnan(tp[1]) and tp[2] == np.inf


def test_true_peak_bits_do_not_depend_on_scratch_alignment_or_stream():
    sr = 48000
    x = _dev(_noise(5 * 1024 + 77, 2, 31))                                   # six workgroups
    lib = loudness._lib.load()
    need = int(lib.wun_true_peak_scratch_doubles(x.shape[0], 2))
    a = loudness.true_peak(x, sr, scratch=torch.zeros(need, dtype=torch.float64, device=DEV))
    b = loudness.true_peak(x, sr, scratch=torch.full((need,), float("nan"), dtype=torch.float64, device=DEV))
    c = loudness.true_peak(x, sr, scratch=torch.full((need,), 1e300, dtype=torch.float64, device=DEV))
    d = loudness.true_peak(_offset_copy(x), sr)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        e = loudness.true_peak(x, sr)
        r1 = loudness.r128(x, sr)
    side.synchronize()
    r0 = loudness.r128(x, sr)
    r2 = loudness.r128(_offset_copy(x), sr, scratch=torch.full((loudness.r128_scratch_doubles(x.shape[0], 2, sr),), float("nan"),
                                                                  dtype=torch.float64, device=DEV))
    for other in (b, c, d, e):
        assert torch.equal(_i64(a), _i64(other))
    assert torch.equal(_i64(r0), _i64(r1)) and torch.equal(_i64(r0), _i64(r2)) and torch.equal(_i64(r0[4:5]), _i64(a[0:1]))
    assert torch.isfinite(a).all() and a[0].item() == max(a[1].item(), a[2].item())


def test_guards_around_every_buffer_stay_untouched():
    sr, G = 8000, 64
    n, C = 4 * sr + 123, 2                                                   # 4 s: 11 short-term blocks
    nb3 = loudness.short_term_blocks(n, sr)
    x = _dev(_noise(n, C, 32))
    lib = loudness._lib.load()
    L = loudness.oversampling(sr)

    def guarded(count, dtype):
        buf = torch.full((count + 2 * G,), 7.0, dtype=dtype, device=DEV)
        return buf, buf[G:G + count]

    xbuf, xg = guarded(n * C, torch.float32)
    xg.copy_(x.view(-1))
    tbuf, tab = guarded(L * 21, torch.float32)
    tab.copy_(torch.from_numpy(rs.design(L, 1)).view(-1))
    s1buf, s1 = guarded(int(lib.wun_true_peak_scratch_doubles(n, C)), torch.float64)
    s2buf, s2 = guarded(loudness.r128_scratch_doubles(n, C, sr), torch.float64)
    obuf, out = guarded(1 + C, torch.float64)
    rbuf, rep = guarded(8, torch.float64)
    stbuf, st = guarded(nb3, torch.float64)
    stream = loudness._stream(torch.device(DEV))
    loudness._lib.check(lib.wun_true_peak(xg.data_ptr(), n, C, L, tab.data_ptr(), out.data_ptr(), s1.data_ptr(), stream))
    loudness._lib.check(lib.wun_loudness_r128(xg.data_ptr(), n, C, sr, tab.data_ptr(), rep.data_ptr(), st.data_ptr(), s2.data_ptr(),
                                              stream))
    torch.cuda.synchronize()
    for buf, inner in ((xbuf, xg), (tbuf, tab), (s1buf, s1), (s2buf, s2), (obuf, out), (rbuf, rep), (stbuf, st)):
        assert (buf[:G] == 7.0).all() and (buf[G + inner.numel():] == 7.0).all()
    assert torch.equal(xg.view(n, C), x)                                     # the inputs are read only
    assert torch.equal(_i64(out), _i64(loudness.true_peak(x, sr)))
    want, want_st = loudness.r128(x, sr, return_short_term=True)
    assert torch.equal(_i64(rep), _i64(want)) and torch.equal(_i64(st), _i64(want_st)) and nb3 == 11


def _short_term_case(x, sr):
    """r128 of x on the device against the oracle, short-term block by block, under the bound of the module docstring.  Returns
    (report, short-term values) of the device as numpy, (z3, s) of the oracle and the per-block tolerance in LU."""
    n = x.shape[0]
    N3, step, nb3 = r128o.short_term_geometry(n, sr)
    z3, s = r128o.short_term(x, sr)
    rep, st = loudness.r128(_dev(x), sr, return_short_term=True)
    rep, st = rep.cpu().numpy(), st.cpu().numpy()
    assert st.shape == (nb3,)
    sos = ora.kweight_sos(sr)
    serial = ora.sosfilt_fast(sos, x)
    e = 4.0 * np.max(np.abs(ora.sosfilt_chunked(sos, x, loudness.chunk()) - serial), axis=0)          # per channel, absolute
    with np.errstate(over="ignore"):
        z_dev = 10.0 ** ((st + 0.691) / 10.0)
    tol_l = np.zeros(nb3)
    worst = 0.0
    for j in range(nb3):
        ms = np.mean(serial[j * step:j * step + N3] ** 2, axis=0)
        tol_z = float(np.sum(2.0 * np.sqrt(ms) * e + e * e)) + N3 * 2.0 ** -53 * z3[j]
        tol_z += 4e-15 * z3[j]                          # z_dev comes back through log10 and 10^x: a few float64 roundings
        assert abs(z_dev[j] - z3[j]) <= tol_z, (j, z_dev[j], z3[j], tol_z)
        if s[j] > -70.0:
            tol_l[j] = -10.0 * np.log10(1.0 - tol_z / z3[j]) + 1e-13                                  # + the roundings of log10 itself
            worst = max(worst, abs(st[j] - s[j]) / tol_l[j])
            assert abs(st[j] - s[j]) <= tol_l[j], (j, st[j], s[j], tol_l[j])
    if nb3:
        _observed.record("test_gpu_r128.short_term", "sr=%d n=%d C=%d (err / tol, worst block)" % (sr, n, x.shape[1]), worst, 1.0)
    return rep, st, z3, s, tol_l


# ---- the report slots shared with the old meter ----------------------------------------------------
@pytest.mark.parametrize("sr, n, C", [(8000, 136000 // 4, 2), (8000, 3000, 1), (48000, 2 * 48000 + 5, 2), (11025, 40000, 1)])
def test_report_slots_shared_with_integrated(sr, n, C):
    """11025 Hz: a step of 1102.5 frames rounds up, so the 3 s blocks' ends fall between the 0.4 s blocks' cuts."""
    xh = _noise(n, C, 33 + C, 0.1)
    x = _dev(xh)
    meter, blk = loudness.integrated(x, sr, return_blocks=True)
    rep, st = loudness.r128(x, sr, return_short_term=True)
    assert rep.shape == (8,) and rep.dtype == torch.float64 and st.shape == (loudness.short_term_blocks(n, sr),)
    assert torch.equal(_i64(rep[0:1]), _i64(meter[0:1]))                     # integrated loudness
    assert torch.equal(_i64(rep[5:6]), _i64(meter[3:4]))                     # sample peak
    assert torch.equal(_i64(rep[6:7]), _i64(meter[1:2]))                     # gating blocks kept
    if blk.numel():
        assert torch.equal(_i64(rep[2:3]), _i64(blk.max().reshape(1)))      # max momentary
    else:
        assert rep[2].item() == -np.inf
    assert torch.equal(_i64(rep[4:5]), _i64(loudness.true_peak(x, sr)[0:1]))
    if st.numel():
        assert torch.equal(_i64(rep[3:4]), _i64(st.max().reshape(1)))
    rep2, st2, _, _, _ = _short_term_case(xh, sr)                            # the short-term blocks against the oracle, at every rate
    assert np.array_equal(rep2, rep.cpu().numpy()) and np.array_equal(st2, st.cpu().numpy())


# ---- short-term blocks and the loudness range ------------------------------------------------------
def _range_input():
    sr = 8000
    a, b = int(4.5 * sr), int(3.5 * sr)
    x = np.concatenate([_noise(a, 2, 20, 0.25), _noise(a, 2, 21, 0.25 * 10.0 ** (-12.0 / 20.0)),
                        _noise(a, 2, 22, 0.25 * 10.0 ** (-30.0 / 20.0)), np.zeros((b, 2), np.float32)])
    return sr, x


def test_short_term_blocks_and_loudness_range_at_8k():
    """4.5 s of noise, 4.5 s 12 dB down, 4.5 s 30 dB down (under the relative gate), 3.5 s of digital silence (under the absolute
    gate once the filter's tail is gone): both gates drop blocks, and the two ranks fall into different level steps."""
    sr, x = _range_input()
    n = x.shape[0]
    assert n == 136000
    N3, step, nb3 = r128o.short_term_geometry(n, sr)
    z3, s = r128o.short_term(x, sr)
    lra, keep, gate, sel = r128o.loudness_range(z3, s)
    absg = s > -70.0
    # the margins, on the oracle: no block at a gate's edge, the selected values clear of their neighbours
    assert (nb3, int(absg.sum()), int(keep.sum())) == (141, 135, 90) and abs(lra - 16.63) < 0.05
    assert np.min(np.abs(s[np.isfinite(s)] + 70.0)) >= 0.01 and np.min(np.abs(s[absg] - gate)) >= 0.01
    order = np.nonzero(keep)[0][np.argsort(s[keep], kind="stable")]
    lo, hi = r128o.ranks(order.size)
    assert (int(order[lo]), int(order[hi])) == sel
    gaps = [abs(s[order[r + d]] - s[order[r]]) for r in (lo, hi) for d in (-1, 1) if 0 <= r + d < order.size]
    assert min(gaps) >= 1e-6

    rep, st, _, _, tol_l = _short_term_case(x, sr)                           # every z3_j and s_j within its bound
    assert st.shape == (nb3,) and rep[7] == keep.sum()                       # block count and kept count exact
    assert 2.0 * np.max(tol_l) < min(gaps)              # so the device selects the oracle's two blocks
    tol = tol_l[sel[0]] + tol_l[sel[1]]
    _observed.record("test_gpu_r128.loudness_range", "sr=8000 n=136000 C=2", abs(rep[1] - lra), tol)
    assert abs(rep[1] - lra) <= tol, (rep[1], lra, tol)
    assert rep[1] == st[sel[1]] - st[sel[0]]                                # the difference of the two selected device values
    top = int(np.argmax(s))
    _observed.record("test_gpu_r128.max_short_term", "sr=8000 n=136000 C=2", abs(rep[3] - s[top]), tol_l[top])
    assert abs(rep[3] - s[top]) <= tol_l[top] and rep[3] == st.max()
    # the other readings of the same report
    want = r128o.r128(x, sr)[0]
    assert rep[6] == want[6] and rep[5] == want[5] and abs(rep[0] - want[0]) < 1e-6 and abs(rep[2] - want[2]) < 1e-6


def test_range_of_nearly_equal_short_term_values():
    """A constant tone: every short-term value past the filter's onset is the same to a few ulps, some perhaps exactly: the counts
    by (value, index) are still a permutation, both ranks are written over the poisoned scratch, and the range is what sorting
    the device's own values gives."""
    sr = 8000
    x = np.tile((0.1 * np.sin(2 * np.pi * 1000.0 * np.arange(12 * sr) / sr))[:, None], [1, 2]).astype(np.float32)
    rep, st = loudness.r128(_dev(x), sr, return_short_term=True, scratch=torch.full(
        (loudness.r128_scratch_doubles(x.shape[0], 2, sr),), float("nan"), dtype=torch.float64, device=DEV))
    rep, st = rep.cpu().numpy(), st.cpu().numpy()
    v = np.sort(st)
    lo, hi = r128o.ranks(v.size)
    assert rep[7] == v.size == 91
    assert rep[1] == v[hi] - v[lo] and 0.0 <= rep[1] < 0.01


# ---- edges -------------------------------------------------------------------------------------
def test_edges_of_the_short_term_meter():
    sr = 8000
    N3 = r128o.short_term_geometry(1, sr)[0]
    rep, st = loudness.r128(_dev(_noise(N3 - 1, 2, 34)), sr, return_short_term=True)
    rep = rep.cpu().numpy()
    assert st.numel() == 0 and rep[1] == 0.0 and rep[3] == -np.inf and rep[7] == 0 and np.isfinite(rep[0]) and np.isfinite(rep[2])
    rep, st = loudness.r128(_dev(_noise(N3, 2, 35)), sr, return_short_term=True)
    rep = rep.cpu().numpy()
    assert st.numel() == 1 and rep[1] == 0.0 and rep[7] == 1 and rep[3] == st[0].item() and np.isfinite(rep[3])
    rep = loudness.r128(_dev(np.zeros((N3 + 4000, 1), np.float32)), sr).cpu().numpy()
    assert rep[0] == -np.inf and rep[1] == 0.0 and rep[2] == -np.inf and rep[3] == -np.inf
    assert rep[4] == 0.0 and rep[5] == 0.0 and rep[6] == 0 and rep[7] == 0


def test_a_nan_sample_gives_nan_readings():
    sr = 8000
    x = _noise(4 * sr, 2, 36)
    x[sr // 2, 1] = np.nan
    xd = _dev(x)
    rep = loudness.r128(xd, sr).cpu().numpy()
    meter = loudness.integrated(xd, sr).cpu().numpy()
    assert np.isnan(rep[:5]).all() and np.isnan(rep[5])
    assert rep[6] == meter[1] and rep[7] == 0                               # the counts as the meter defines them: NaN blocks pass no gate


# ---- the ceiling -----------------------------------------------------------------------------------
def test_true_peak_limit_holds_the_true_peak_where_the_sample_peak_limit_does_not():
    sr = 8000
    x = _dev(_sine45(2 * sr, 1, 0.1))
    L0 = loudness.integrated(x, sr)[0].item()
    target = L0 + 20.0                                                       # the target gain alone: 10, the waveform to 1.0134
    g_free = 10.0 ** ((target - L0) / 20.0)
    tp0 = loudness.true_peak(x, sr)[0].item()
    pk0 = x.abs().max().item()
    assert g_free * tp0 > LIMIT > g_free * pk0                               # the target gain alone: true peak over, sample peak under
    y, g = loudness.normalize(x, sr, target=target, max_gain_db=60.0, true_peak_limit=-1.0)
    tp = loudness.true_peak(y, sr)[0].item()
    print("true peak after the ceiling %.9g, limit %.9g, ulp %.3g" % (tp, LIMIT, float(np.spacing(np.float32(LIMIT)))))
    assert g[0].item() < g_free and tp <= LIMIT + float(np.spacing(np.float32(LIMIT)))
    assert tp > 0.999 * LIMIT                                                # the ceiling binds, and no more than needed
    y2, g2 = loudness.normalize(x, sr, target=target, max_gain_db=60.0, peak_limit=LIMIT)
    assert abs(g2[0].item() / g_free - 1.0) < 1e-6 and loudness.true_peak(y2, sr)[0].item() > 1.1 * LIMIT
    # the composition normalize() stands for
    rep = loudness.r128(x, sr)
    meter = loudness.meter_from_r128(rep, x.shape[0], sr)
    assert torch.equal(_i64(meter), _i64(torch.stack([rep[0], rep[6], torch.tensor(float(loudness.blocks(x.shape[0], sr)),
                                                                                    dtype=torch.float64, device=DEV), rep[4]])))
    assert torch.equal(_bits(g), _bits(loudness.gain(meter, target, 60.0, peak_limit=LIMIT)))
    with pytest.raises(ValueError):
        loudness.normalize(x, sr, peak_limit=0.9, true_peak_limit=-1.0)


def _count_calls(monkeypatch, name):
    calls = []
    real = getattr(loudness, name)

    def wrapper(*a, **kw):
        calls.append(name)
        return real(*a, **kw)
    monkeypatch.setattr(loudness, name, wrapper)
    return calls


def test_separate_track_with_a_true_peak_limit_is_the_composition_of_the_public_pieces(monkeypatch):
    cfg, sep = _separator("baseline_context_small")
    chan = 1 if cfg["mono_downmix"] else 2
    audio = _noise(4100, chan, 10, 0.01)
    spec = {"target": -5, "max_gain_db": 60, "true_peak_limit": -1}          # the target gain alone would clip: the ceiling binds
    probe = {}
    calls = _count_calls(monkeypatch, "r128")
    got = separate_track(cfg, sep, audio, SR, return_device=True, loudness=spec, loudness_probe=probe, batch_hops=16)
    assert calls == ["r128"]
    x = _dev(audio)
    rep = loudness.r128(x, SR)
    g = loudness.gain(loudness.meter_from_r128(rep, x.shape[0], SR), -5.0, 60.0, peak_limit=LIMIT)
    out = separate_track(cfg, sep, loudness.scale_(x.clone(), g[0:1]), SR, return_device=True, batch_hops=16)
    want = loudness.scale_(out, g[1:2])
    assert got.shape == want.shape and torch.equal(_bits(got), _bits(want)) and got.abs().max().item() > 0
    assert torch.equal(_bits(probe["gain"]), _bits(g))
    free = loudness.gain(loudness.integrated(x, SR), -5.0, 60.0)
    assert g[0].item() < free[0].item()                                       # the ceiling bound
    seen = probe["padded"][probe["offset"]:probe["offset"] + probe["frames"]].contiguous()
    # what the network read: the float32 gain, the float32 products and the 21-tap float32 chains, each 2^-24 relative on
    # sums whose absolute terms stay under 3 x the peak: below 25 x 3 x 2^-24 = 5e-6
    assert loudness.true_peak(seen, SR)[0].item() <= LIMIT * (1.0 + 1e-5)


def test_without_the_key_nothing_new_is_called(monkeypatch):
    cfg, sep = _separator("baseline_context_small")
    audio = _noise(4100, 1 if cfg["mono_downmix"] else 2, 11, 0.01)
    r_calls = _count_calls(monkeypatch, "r128")
    t_calls = _count_calls(monkeypatch, "true_peak")
    i_calls = _count_calls(monkeypatch, "integrated")
    a = separate_track(cfg, sep, audio, SR, return_device=True, loudness=-23, batch_hops=16)
    b = separate_track(cfg, sep, audio, SR, return_device=True, loudness={"target": -23, "peak_limit": 0.5}, batch_hops=16)
    assert r_calls == [] and t_calls == [] and i_calls == ["integrated", "integrated"]
    x = _dev(audio)
    g = loudness.gain(loudness.integrated(x, SR), -23.0, 30.0, None)
    want = loudness.scale_(separate_track(cfg, sep, loudness.scale_(x.clone(), g[0:1]), SR, return_device=True, batch_hops=16), g[1:2])
    assert torch.equal(_bits(a), _bits(want)) and a.shape == b.shape


def test_normalize_tracks_with_a_true_peak_limit():
    import wave_u_net_amd as wun
    from wave_u_net_amd import datasets
    cfg = wun.get_config("baseline_stereo", expected_sr=SR)
    stems = {k: _sine45(2 * SR, 2, 0.05) for k in cfg["source_names"]}
    track = datasets.make_track(stems, cfg)
    spec = {"target": 3.0, "max_gain_db": 60.0, "true_peak_limit": -1.0, "data": True}      # a target the ceiling must stop
    out, gains = datasets.normalize_tracks([track], cfg, DEV, spec)
    mix = _dev(track["mix"])
    want = loudness.gain(loudness.meter_from_r128(loudness.r128(mix, SR), mix.shape[0], SR), 3.0, 60.0, peak_limit=LIMIT)
    assert gains[0] == want.cpu().numpy()[0] and np.array_equal(out[0]["mix"], track["mix"] * gains[0])
    assert loudness.true_peak(_dev(out[0]["mix"]), SR)[0].item() <= LIMIT * (1.0 + 1e-5)     # as above
    free = loudness.gain(loudness.integrated(mix, SR), 3.0, 60.0).cpu().numpy()[0]
    assert gains[0] < free
