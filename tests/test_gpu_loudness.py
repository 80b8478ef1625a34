"""GPU tests of the recursive filter and the loudness meter (include/wun.h: wun_sosfilt, wun_loudness, wun_loudness_gain,
wun_scale_by; wave_u_net_amd.loudness; evaluate.separate_track(loudness=..); datasets.normalize_tracks) against the
float64 numpy oracle tests/_loudness_np.py.

Tolerances.  Filter: a device value (float64, rounded once to float32) against float32(serial oracle): one float32 ulp at
max |y| plus 4 times the error the numpy emulation of the chunked schedule shows against the serial recurrence on THAT input
(_loudness_np.filter_tolerance; tests/test_loudness_host.py shows that the emulation without its carries misses it by 1000 x).
Meter: with e = 4 x that emulation error (absolute), a block's mean square per channel moves by at most
2 sqrt(ms_c) e_c + e_c^2, and summing Nb squares in another order by Nb 2^-53 relative; in LU that is
-10 log10(1 - tol_z / z), i.e. 8.7 x the relative filter error + 4.3 Nb 2^-53 for a stationary signal."""
import numpy as np
import pytest
import torch

import _loudness_np as ora
import _observed
from _unaligned import _offset_copy, _offset_full

import wave_u_net_amd as wun
from wave_u_net_amd import datasets, loudness
from wave_u_net_amd.evaluate import separate_track

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ora.filter_cases()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _sizes():
    ch, tile = loudness.chunk(), loudness.tile()
    return [1, 2, ch - 1, ch, ch + 1, 3 * ch + 37, (tile + 1) * ch]       # the last: one chunk past the workgroup tile


# ---- wun_sosfilt against the serial oracle ---------------------------------------------------------
@pytest.mark.parametrize("kind", ora.INPUT_KINDS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_sosfilt_matches_the_serial_recurrence(case, kind):
    ch = loudness.chunk()
    sos = CASES[case]
    for n in _sizes():
        for C in (1, 2):
            x = ora.filter_input(kind, n, C, ch)
            serial = ora.sosfilt_serial(sos, x) if n <= 4 * ch else ora.sosfilt_fast(sos, x)
            tol = ora.filter_tolerance(serial, ora.sosfilt_chunked(sos, x, ch))
            got = loudness.sosfilt(_dev(x), sos).cpu().numpy()
            assert got.shape == x.shape and got.dtype == np.float32
            err = float(np.max(np.abs(got.astype(np.float64) - serial.astype(np.float32).astype(np.float64))))
            _observed.record("test_sosfilt_matches_the_serial_recurrence[%s-%s]" % (case, kind), "n=%d C=%d" % (n, C),
                             err / max(np.max(np.abs(serial)), 1e-300), tol / max(np.max(np.abs(serial)), 1e-300))
            assert err <= tol, (case, kind, n, C, err, tol)


def test_k_weight_is_sosfilt_of_the_design():
    x = _dev(ora.filter_input("noise", 1000, 2, loudness.chunk()))
    assert torch.equal(loudness.k_weight(x, 44100), loudness.sosfilt(x, loudness.kweight_sos(44100)))


# ---- contracts and bits ------------------------------------------------------------------------
def _noise(n, C, seed=0, amp=0.25):
    return (amp * np.random.RandomState(seed).randn(n, C)).astype(np.float32)


def _run_all(x, sr, scratch_fill):
    """(filtered, meter, blocks) with both entries' scratch pre-filled with `scratch_fill`."""
    n, C = x.shape
    lib_need = loudness._lib.load().wun_sosfilt_scratch_doubles(n, C, 2)
    s1 = torch.full((lib_need,), scratch_fill, dtype=torch.float64, device=DEV)
    s2 = torch.full((loudness.scratch_doubles(n, C, sr),), scratch_fill, dtype=torch.float64, device=DEV)
    y = loudness.sosfilt(x, loudness.kweight_sos(sr), scratch=s1)
    meter, blk = loudness.integrated(x, sr, return_blocks=True, scratch=s2)
    return y, meter, blk


def test_runs_are_bit_equal_and_scratch_contents_do_not_matter():
    sr = 8000
    x = _dev(_noise(70 * loudness.chunk() + 11, 2, 1))
    a = _run_all(x, sr, 0.0)
    b = _run_all(x, sr, 0.0)
    c = _run_all(x, sr, float("nan"))
    for u, v, w in zip(a, b, c):
        assert torch.equal(u.view(torch.int32 if u.dtype == torch.float32 else torch.int64),
                           v.view(torch.int32 if v.dtype == torch.float32 else torch.int64))
        assert torch.equal(u.view(torch.int32 if u.dtype == torch.float32 else torch.int64),
                           w.view(torch.int32 if w.dtype == torch.float32 else torch.int64))
    assert torch.isfinite(a[1]).all() and a[2].numel() == loudness.blocks(x.shape[0], sr) > 0


def test_guards_around_every_buffer_stay_untouched():
    sr, G = 8000, 64
    n, C = sr, 2                                                             # one second: 7 blocks
    nb = loudness.blocks(n, sr)
    x = _dev(_noise(n, C, 2))
    lib = loudness._lib.load()

    def guarded(count, dtype):
        buf = torch.full((count + 2 * G,), 7.0, dtype=dtype, device=DEV)
        return buf, buf[G:G + count]

    ybuf, y = guarded(n * C, torch.float32)
    s1buf, s1 = guarded(lib.wun_sosfilt_scratch_doubles(n, C, 2), torch.float64)
    s2buf, s2 = guarded(loudness.scratch_doubles(n, C, sr), torch.float64)
    mbuf, m = guarded(4, torch.float64)
    bbuf, b = guarded(nb, torch.float64)
    gbuf, g = guarded(2, torch.float32)
    stream = loudness._stream(torch.device(DEV))
    sos = np.ascontiguousarray(loudness.kweight_sos(sr))
    import ctypes as C_
    loudness._lib.check(lib.wun_sosfilt(x.data_ptr(), n, C, sos.ctypes.data_as(C_.POINTER(C_.c_double)), 2, y.data_ptr(),
                                        s1.data_ptr(), stream))
    loudness._lib.check(lib.wun_loudness(x.data_ptr(), n, C, sr, m.data_ptr(), b.data_ptr(), s2.data_ptr(), stream))
    loudness._lib.check(lib.wun_loudness_gain(m.data_ptr(), -23.0, 30.0, 0.0, g.data_ptr(), stream))
    zbuf, z = guarded(n * C, torch.float32)
    z.copy_(x.view(-1))
    loudness._lib.check(lib.wun_scale_by(z.data_ptr(), n * C, g.data_ptr(), stream))
    torch.cuda.synchronize()
    for buf, inner in ((ybuf, y), (s1buf, s1), (s2buf, s2), (mbuf, m), (bbuf, b), (gbuf, g), (zbuf, z)):
        assert (buf[:G] == 7.0).all() and (buf[G + inner.numel():] == 7.0).all()
    assert torch.equal(y.view(n, C), loudness.k_weight(x, sr))
    assert torch.equal(z.view(n, C), x * g[0])                             # one fp32 product per sample


def test_buffers_one_float_off_16_bytes():
    sr = 8000
    x = _dev(_noise(sr + 77, 2, 3))
    xo = _offset_copy(x)
    yo = _offset_full(x.shape, float("nan"), device=DEV)
    loudness.sosfilt(xo, loudness.kweight_sos(sr), out=yo)
    assert torch.equal(_bits(yo), _bits(loudness.k_weight(x, sr)))
    assert torch.equal(loudness.integrated(xo, sr).view(torch.int64), loudness.integrated(x, sr).view(torch.int64))
    g = loudness.gain(loudness.integrated(x, sr))
    assert torch.equal(_bits(loudness.scale_(xo.clone(), g[0:1])), _bits(x * g[0]))
    z = _offset_copy(x)
    loudness.scale_(z, g[0:1])
    assert torch.equal(_bits(z), _bits(x * g[0]))


def test_a_side_stream_gives_the_same_bits():
    sr = 8000
    x = _dev(_noise(sr + 5, 2, 4))
    y0, m0, b0 = _run_all(x, sr, 0.0)
    g0 = loudness.gain(m0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        y1, m1, b1 = _run_all(x, sr, 0.0)
        g1 = loudness.gain(m1)
        z1 = loudness.scale_(x.clone(), g1[0:1])
    side.synchronize()
    assert torch.equal(_bits(y0), _bits(y1)) and torch.equal(m0.view(torch.int64), m1.view(torch.int64))
    assert torch.equal(b0.view(torch.int64), b1.view(torch.int64)) and torch.equal(_bits(g0), _bits(g1))
    assert torch.equal(_bits(z1), _bits(x * g0[0]))


def test_a_nan_sample_gives_a_nan_reading_and_unit_gain():
    sr = 8000
    x = _noise(2 * sr, 2, 5)
    x[sr // 2, 1] = np.nan
    meter = loudness.integrated(_dev(x), sr)
    g = loudness.gain(meter, -23.0).cpu().numpy()
    m = meter.cpu().numpy()
    assert np.isnan(m[0]) and np.isnan(m[3]) and m[2] == loudness.blocks(2 * sr, sr)
    assert g[0] == 1.0 and g[1] == 1.0


# ---- the meter against the oracle ------------------------------------------------------------------
def _meter_case(x, sr):
    """Device reading of x against the oracle's, block by block; returns (device meter, oracle result)."""
    n, C = x.shape
    ch = loudness.chunk()
    sos = ora.kweight_sos(sr)
    serial = ora.sosfilt_fast(sos, x)
    e = 4.0 * np.max(np.abs(ora.sosfilt_chunked(sos, x, ch) - serial), axis=0)          # per channel, absolute
    L, kept, nb, peak, l = ora.loudness(x, sr)
    Nb, step, _ = ora.block_geometry(n, sr)
    meter, blk = loudness.integrated(_dev(x), sr, return_blocks=True)
    m, blk = meter.cpu().numpy(), blk.cpu().numpy()
    assert blk.shape == (nb,) and m[2] == nb and m[1] == kept
    assert m[3] == peak                                                                  # the maximum is unique: exact
    z_ref = 10.0 ** ((l + 0.691) / 10.0)
    with np.errstate(over="ignore"):
        z_dev = 10.0 ** ((blk + 0.691) / 10.0)
    worst = 0.0
    for j in range(nb):
        ms = np.mean(serial[j * step:j * step + Nb] ** 2, axis=0)
        tol_z = float(np.sum(2.0 * np.sqrt(ms) * e + e * e)) + Nb * 2.0 ** -53 * z_ref[j]
        tol_z += 4e-15 * z_ref[j]                       # z_dev comes back through log10 and 10^x: a few float64 roundings
        assert abs(z_dev[j] - z_ref[j]) <= tol_z, (j, z_dev[j], z_ref[j], tol_z)
        if l[j] > -70.0:
            tol_l = -10.0 * np.log10(1.0 - tol_z / z_ref[j]) + 1e-13                     # + the roundings of log10 itself at |l| < 100
            worst = max(worst, abs(blk[j] - l[j]) / tol_l)
            assert abs(blk[j] - l[j]) <= tol_l, (j, blk[j], l[j], tol_l)
    if np.isfinite(L):
        # the gated mean moves by no more than its blocks do: the largest relative block tolerance, + the kept blocks reordered
        keep = (l > -70.0) & (l > -0.691 + 10.0 * np.log10(np.mean(z_ref[l > -70.0])) - 10.0)
        rel = max((float(np.sum(2.0 * np.sqrt(np.mean(serial[j * step:j * step + Nb] ** 2, axis=0)) * e + e * e)) / z_ref[j]
                   for j in np.nonzero(keep)[0]))
        tol_L = -10.0 * np.log10(1.0 - rel - (Nb + kept) * 2.0 ** -53) + 1e-13
        _observed.record("test_gpu_loudness.meter", "sr=%d n=%d C=%d" % (sr, n, C), abs(m[0] - L), tol_L)
        assert abs(m[0] - L) <= tol_L, (m[0], L, tol_L)
    else:
        assert m[0] == -np.inf
    return m, (L, kept, nb, peak, l)


@pytest.mark.parametrize("C", [1, 2])
def test_meter_block_boundaries_at_8k(C):
    sr = 8000
    Nb, step, _ = ora.block_geometry(sr, sr)
    for n, nb in ((Nb - 1, 0), (Nb, 1), (Nb + step - 1, 1), (Nb + step, 2)):
        m, ref = _meter_case(_noise(n, C, n), sr)
        assert m[2] == nb == ref[2]
        if nb == 0:
            assert m[0] == -np.inf and m[1] == 0


def test_meter_stereo_noise_at_8k():
    m, ref = _meter_case(_noise(int(1.3 * 8000), 2, 6), 8000)
    assert ref[2] == 10 and np.isfinite(m[0])


def test_meter_both_gates_at_8k():
    """1.5 s loud, 1.5 s 25 dB quieter (above -70 LUFS, under the relative gate), 1.5 s of digital silence (under the absolute
    gate once the filter's tail is gone)."""
    sr = 8000
    k = int(1.5 * sr)
    x = np.concatenate([_noise(k, 2, 7, 0.25), _noise(k, 2, 8, 0.25 * 10.0 ** (-25.0 / 20.0)), np.zeros((k, 2), np.float32)])
    L, kept, nb, peak, l = ora.loudness(x, sr)
    absg = l > -70.0
    gate = -0.691 + 10.0 * np.log10(np.mean(10.0 ** ((l[absg] + 0.691) / 10.0))) - 10.0
    assert 0 < kept < absg.sum() < nb                                       # both gates drop blocks
    assert np.min(np.abs(l[np.isfinite(l)] + 70.0)) > 0.01 and np.min(np.abs(l[absg] - gate)) > 0.01     # none at a gate's edge
    m, _ = _meter_case(x, sr)
    assert m[1] == kept


def test_meter_tone_at_48k():
    sr = 48000
    t = np.arange(2 * sr) / float(sr)
    x = np.tile(np.sin(2 * np.pi * 997.0 * t)[:, None], [1, 2]).astype(np.float32)
    x[12345, 0] = 1.25                                                       # the unique maximum
    m, ref = _meter_case(x, sr)
    assert abs(m[0] - 0.0) < 0.01 and ref[2] == 17


# ---- gain and scaling --------------------------------------------------------------------------
def _meter_tensor(L, peak):
    return torch.tensor([L, 1.0, 1.0, peak], dtype=torch.float64, device=DEV)


def test_gain_rule():
    for L, peak, kw in ((-33.0, 0.1, {}), (-13.5, 0.9, {}), (-80.0, 0.001, {}), (-45.0, 0.2, {"max_gain_db": 12.0}),
                        (-33.0, 0.5, {"peak_limit": 0.9}), (-33.0, 0.05, {"peak_limit": 0.9}), (-23.0, 0.3, {"target": -16.0}),
                        (-np.inf, 0.0, {}), (np.inf, 1.0, {}), (np.nan, 0.3, {"peak_limit": 0.5})):
        got = loudness.gain(_meter_tensor(L, peak), **kw).cpu().numpy()
        want = ora.gain(L, peak, **kw)
        # pow() on the device and in numpy may differ in the last float64 place: one float32 ulp after the rounding
        assert abs(float(got[0]) - float(want[0])) <= 2.0 ** -23 * float(want[0]), (L, peak, kw, got, want)
        assert got[1] == np.float32(1.0 / np.float64(got[0]))               # gain[1] is as defined, from the stored gain[0]
        if not np.isfinite(L):
            assert got[0] == 1.0 and got[1] == 1.0
    # the cap and the peak limit bind where expected
    assert loudness.gain(_meter_tensor(-80.0, 0.001)).cpu()[0] == np.float32(10.0 ** 1.5)
    assert loudness.gain(_meter_tensor(-33.0, 0.5), peak_limit=0.9).cpu()[0] == np.float32(0.9 / 0.5)
    assert loudness.gain(_meter_tensor(-33.0, 0.05), peak_limit=0.9).cpu()[0] > 3.0      # the limit is not reached


def test_normalize_reaches_the_target():
    sr = 8000
    x = _dev(_noise(2 * sr, 2, 9, 0.01))
    y, g = loudness.normalize(x, sr, target=-20.0)
    assert torch.equal(y, x * g[0]) and y.data_ptr() != x.data_ptr()
    L0, L1 = loudness.integrated(x, sr)[0].item(), loudness.integrated(y, sr)[0].item()
    # the float32 gain (2^-24 relative: 5e-7 dB) and the float32 products (their errors average out over a block's squares)
    assert abs(L1 + 20.0) <= 1e-5 and abs((L1 - L0) - 20.0 * np.log10(g[0].item())) <= 1e-5
    z, g2 = loudness.normalize(x, sr, target=-20.0, inplace=True)
    assert z.data_ptr() == x.data_ptr() and torch.equal(z, y) and torch.equal(g, g2)


# ---- separate_track(loudness=..) ----------------------------------------------------------------------
SR = 8000                    # blocks of 3200 frames: a track of a few thousand frames has some


def _separator(name):
    from oracle import shapes
    from oracle.golden_params import GOLDEN_CASES, golden_params
    from wave_u_net_amd.separator import UnetAudioSeparator
    case = GOLDEN_CASES[name]
    ocfg = shapes.finalize_config(dict(shapes.BASE_MODEL_CONFIG, **case["cfg"]))
    cfg = wun.get_config("baseline", num_frames=case["frames"], expected_sr=SR, **case["cfg"])
    sep = UnetAudioSeparator(cfg, device=DEV)
    i, o = shapes.get_padding(ocfg, [1, case["frames"], 0])
    sep._plan(1, i[1]); sep._active = sep._plans[(1, i[1])]
    sep.load_variables(golden_params(ocfg, case["seed"]))
    return cfg, sep


def _spec_separator():
    import _specunet_np as so
    from wave_u_net_amd import UnetSpectrogramSeparator
    n_fft, hop, L, nif, F, B = 64, 48, 2, 3, 8, 2
    T = (F - 1) * hop + n_fft
    cfg = wun.get_config("unet_spectrogram", num_layers=L, num_initial_filters=nif, spec_frame_len=n_fft, spec_hop=hop,
                         num_frames=T, batch_size=B, expected_sr=SR)
    sep = UnetSpectrogramSeparator(cfg, device=DEV)
    sep.load_variables(so.random_variables(L, nif, seed=23 + L))
    return cfg, sep


def _composed(cfg, sep, audio, spec, **kw):
    """The composition from the public pieces: integrated -> gain -> scale -> separate_track -> scale by gain[1]."""
    spec = loudness.from_config(spec)
    x = _dev(audio)
    g = loudness.gain(loudness.integrated(x, SR), spec["target"], spec["max_gain_db"], spec["peak_limit"])
    out = separate_track(cfg, sep, loudness.scale_(x.clone(), g[0:1]), SR, return_device=True, **kw)
    return (loudness.scale_(out, g[1:2]) if spec["restore"] else out), g


@pytest.mark.parametrize("name, spec, kw", [
    ("baseline_context_small", {"target": -23}, {}),
    ("baseline_stereo_small", {"target": -23}, {}),
    ("baseline_stereo_small", {"target": -23, "restore": False}, {}),
    ("baseline_stereo_small", {"target": -23}, {"postfilter": {"n_fft": 64, "hop": 16}}),
    ("baseline_context_small", {"target": -23, "peak_limit": 0.5}, {"overlap": 0.25}),
    ("spectrogram", {"target": -23}, {}),
    ("spectrogram", -18.0, {"overlap": 0.25}),
])
def test_the_keyword_is_the_composition_of_the_public_pieces(name, spec, kw):
    cfg, sep = _spec_separator() if name == "spectrogram" else _separator(name)
    chan = 1 if cfg["mono_downmix"] else 2
    audio = _noise(4100, chan, 10, 0.01)                                      # -35 (stereo) / -38 LUFS (mono): far from the target
    kw = dict(kw, batch_hops=16 if name != "spectrogram" else 2)
    probe = {}
    got = separate_track(cfg, sep, audio, SR, return_device=True, loudness=spec, loudness_probe=probe, **kw)
    want, g = _composed(cfg, sep, audio, spec, **kw)
    assert got.shape == want.shape and torch.equal(_bits(got), _bits(want))
    assert torch.equal(_bits(probe["gain"]), _bits(g)) and g[0].item() > 1.5 and got.abs().max().item() > 0
    plain = separate_track(cfg, sep, audio, SR, return_device=True, **kw)
    assert not torch.equal(got, plain)
    host = separate_track(cfg, sep, audio, SR, loudness=spec, **kw)
    for si, k in enumerate(cfg["source_names"]):
        assert np.array_equal(host[k], got[si].cpu().numpy())


def test_the_default_is_the_path_without_the_keyword():
    for cfg, sep in (_separator("baseline_stereo_small"), _spec_separator()):
        chan = 1 if cfg["mono_downmix"] else 2
        audio = _noise(4100, chan, 11, 0.02)
        a = separate_track(cfg, sep, audio, SR, return_device=True, batch_hops=2)
        b = separate_track(cfg, sep, audio, SR, return_device=True, batch_hops=2, loudness=None)
        assert torch.equal(_bits(a), _bits(b))


def test_a_mix_40_db_down_is_fed_at_the_level_of_the_original():
    """On a file at another rate (the meter sees the resampled frames): the loudness of what the network reads."""
    cfg, sep = _separator("baseline_stereo_small")
    audio = _noise(6000, 2, 12, 0.1)
    levels = []
    for scale in (1.0, 0.01):
        probe = {}
        separate_track(cfg, sep, (audio * np.float32(scale)).astype(np.float32), 12000, return_device=True, loudness={"target": -23, "max_gain_db": 60},
                       loudness_probe=probe, batch_hops=16)
        seen = probe["padded"][probe["offset"]:probe["offset"] + probe["frames"]]
        before = probe["meter"][0].item()
        levels.append((before, loudness.integrated(seen.contiguous(), SR)[0].item()))
    assert abs((levels[0][0] - levels[1][0]) - 40.0) < 1e-3                  # as it arrives: 40 dB apart
    # after the normalisation both read the target: the float32 gain and products (see test_normalize_reaches_the_target)
    assert abs(levels[0][1] + 23.0) <= 1e-5 and abs(levels[1][1] + 23.0) <= 1e-5


# ---- training data ---------------------------------------------------------------------------
def test_normalize_tracks():
    cfg = wun.get_config("baseline_stereo", expected_sr=SR)
    rng = np.random.RandomState(13)
    tracks = []
    for amp in (0.3, 0.02, 0.002):
        stems = {k: (amp * rng.randn(2 * SR, 2)).astype(np.float32) for k in cfg["source_names"]}
        tracks.append(datasets.make_track(stems, cfg))
    spec = {"target": -23.0, "data": True}
    out, gains = datasets.normalize_tracks(tracks, cfg, DEV, spec)
    assert gains.dtype == np.float32 and gains.shape == (3,) and len(out) == 3
    for t_in, t_out, g in zip(tracks, out, gains):
        want = loudness.gain(loudness.integrated(_dev(t_in["mix"]), SR), -23.0).cpu().numpy()[0]
        assert g == want                                                     # the gains returned are the meter's
        assert set(t_out) == set(t_in)
        for k in t_in:                                                       # stems and mix carry that one fp32 factor
            assert t_out[k].dtype == np.float32 and np.array_equal(t_out[k], t_in[k] * g)
        assert abs(loudness.integrated(_dev(t_out["mix"]), SR)[0].item() + 23.0) <= 1e-5
    assert gains[0] < gains[1] < gains[2] and np.array_equal(tracks[0]["mix"], datasets.make_track(
        {k: tracks[0][k] for k in cfg["source_names"]}, cfg)["mix"])        # the given tracks are left as they are
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        datasets.normalize_tracks(tracks, cfg, "cpu", spec)
    assert datasets.loudness_data_spec(dict(cfg, loudness=spec))["data"] and datasets.loudness_data_spec(cfg) is None
    assert datasets.loudness_data_spec(dict(cfg, loudness=-23)) is None
