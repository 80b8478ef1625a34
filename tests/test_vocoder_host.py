"""CPU-only checks of the phase vocoder (include/wun.h: wun_time_stretch and its helpers; datasets.vocoder_descriptors): the
binding and the struct, the length rule against brute force, the scratch formula, every argument error of the entry before any
GPU work (no device here), the float64 oracle of tests/_vocoder_np.py on signals whose answer is known, the order and the
source of the draws, the placement rule, the bank's limit and every ValueError."""
import ctypes as C
import os

import numpy as np
import pytest

import wave_u_net_amd as wun
from wave_u_net_amd import _lib, datasets, validation, vocoder

import _vocoder_np as vnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WUN_ERR_INVALID, WUN_ERR_UNSUPPORTED = -1, -2
_FAKE = C.c_void_p(0x1000)          # non-null, aligned, never dereferenced: every call below fails a check first
T_IN, T_OUT = 90, 40
LENGTHS = [400, 257, 333]            # padded track lengths of a 3-track set
OFFSETS = [0, 400, 657]


def _cfg(name="full_multi_instrument", **kw):
    base = dict(batch_size=4, num_snippets_per_track=3, cache_size=5)
    base.update(kw)
    return wun.get_config(name, **base)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _ceil(a, b):
    return -((-a) // b)


# ---------------------------------------------------------------------------------------- the C ABI
def test_symbols_struct_and_binding(lib):
    assert 64 == _lib.STRETCH_JOBS
    assert lib.wun_stretch_abi_size() == C.sizeof(_lib.WunStretchJob) == 32 == vocoder.JOB_DTYPE.itemsize
    for f, off in {"x": 0, "y": 8, "n_in": 16, "n_out": 20, "num": 24, "den": 28}.items():
        assert getattr(_lib.WunStretchJob, f).offset == off == vocoder.JOB_DTYPE.fields[f][1], f
    assert len(lib.wun_time_stretch.argtypes) == 8
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "5.24" in design and "`wun_time_stretch`" in design


@pytest.mark.parametrize("num,den", [(1, 1), (10, 9), (9, 10), (2, 1), (1, 2), (20, 21), (64, 63), (4, 5)])
def test_frames_is_the_ceiling(lib, num, den):
    for n_in in (1, 2, 41, 700, 3000, 147443, 1 << 31):
        got = lib.wun_time_stretch_frames(n_in, num, den)
        n = max(0, (n_in * den) // num - 2)                         # brute force from below: the smallest n with n num >= n_in den
        while n * num < n_in * den:
            n += 1
        assert got == n == vnp.stretch_frames(n_in, num, den) == vocoder.frames(n_in, num, den)


def test_frames_refuses_bad_arguments(lib):
    for n_in in (0, -1, (1 << 40) + 1):
        assert lib.wun_time_stretch_frames(n_in, 10, 9) == WUN_ERR_INVALID and "n_in" in lib.wun_last_error().decode()
    for num, den, word in ((0, 1, "positive"), (3, -2, "positive"), (4, 6, "coprime"), (20, 18, "coprime")):
        assert lib.wun_time_stretch_frames(90, num, den) == WUN_ERR_INVALID and word in lib.wun_last_error().decode()
    for num, den, word in ((65, 64, "ceiling"), (64, 65, "ceiling"), (1, 3, "[1/2, 2]"), (3, 1, "[1/2, 2]")):
        assert lib.wun_time_stretch_frames(90, num, den) == WUN_ERR_UNSUPPORTED and word in lib.wun_last_error().decode()
    with pytest.raises(ValueError, match="coprime"):
        vocoder.frames(90, 4, 6)
    with pytest.raises(NotImplementedError, match="ceiling"):
        vocoder.frames(90, 65, 64)


def _jobs(n, n_in=700, n_out=630, num=10, den=9, x0=0x100000, y0=0x4000000, step=0x10000):
    return vocoder.job_table([(x0 + step * i, y0 + step * i, n_in, n_out, num, den) for i in range(n)])


def test_scratch_formula(lib):
    for n_fft, hop in ((64, 16), (256, 64), (2048, 512), (8192, 1)):
        K = n_fft // 2 + 1
        for c in (1, 2):
            outs = [1, 17, 630, 5000] + [300 + 7 * i for i in range(76)]           # 80 jobs: two launch sets
            t = _jobs(len(outs))
            t["n_out"] = outs
            rows = [c * sum(vnp.centered_frames(n, n_fft, hop) for n in outs[j0:j0 + 64]) for j0 in (0, 64)]
            assert vocoder.scratch_floats(t, c, n_fft, hop) == max(rows) * (2 * K + n_fft)
            assert vocoder.scratch_floats(t[:3], c, n_fft, hop) == c * sum(
                vnp.centered_frames(n, n_fft, hop) for n in outs[:3]) * (2 * K + n_fft)
    t = _jobs(2)
    assert lib.wun_time_stretch_scratch_floats(None, 2, 2, 256, 64) == WUN_ERR_INVALID
    for kw in ({"J": 0}, {"c": 0}, {"c": 3}, {"hop": 48}, {"hop": 128}, {"hop": 0}):
        a = dict(J=2, c=2, n_fft=256, hop=64)
        a.update(kw)
        assert lib.wun_time_stretch_scratch_floats(t.ctypes.data, a["J"], a["c"], a["n_fft"], a["hop"]) == WUN_ERR_INVALID, kw
    for n_fft in (32, 96, 16384):
        assert lib.wun_time_stretch_scratch_floats(t.ctypes.data, 2, 2, n_fft, 8) == WUN_ERR_UNSUPPORTED
    t["n_out"][1] = 0
    with pytest.raises(ValueError, match="job 1"):
        vocoder.scratch_floats(t, 2, 256, 64)


def test_every_argument_error_comes_before_any_gpu_work(lib):
    def call(t=None, J=None, c=2, n_fft=256, hop=64, table=_FAKE, scratch=_FAKE, null_jobs=False):
        t = _jobs(3) if t is None else t
        return lib.wun_time_stretch(None if null_jobs else t.ctypes.data, len(t) if J is None else J, c, n_fft, hop, table, scratch, None)

    def err():
        return lib.wun_last_error().decode()

    def with_(n=3, **kw):
        t = _jobs(n)
        for k, (i, v) in kw.items():
            t[k][i] = v
        return t
    for kw in ({"null_jobs": True}, {"table": None}, {"scratch": None}, {"t": with_(x=(1, 0))}, {"t": with_(y=(2, 0))}):
        assert call(**kw) == WUN_ERR_INVALID and "null" in err(), kw
    for kw in ({"J": 0}, {"J": -3}, {"c": 0}, {"c": 3}, {"hop": 0}, {"hop": 48}, {"hop": 128}, {"hop": -64},
               {"table": C.c_void_p(0x1002)}, {"scratch": C.c_void_p(0x1001)}, {"t": with_(x=(0, 0x100002))}, {"t": with_(y=(0, 0x4000001))},
               {"t": with_(n_in=(1, 0))}, {"t": with_(n_in=(1, -5))}, {"t": with_(n_out=(2, 0))}, {"t": with_(n_out=(2, 631))},
               {"t": with_(num=(0, 0))}, {"t": with_(den=(0, -9))}, {"t": with_(num=(1, 20), den=(1, 18))}):
        assert call(**kw) == WUN_ERR_INVALID, kw
    for n_fft in (32, 96, 16384, 0):
        assert call(n_fft=n_fft, hop=8) == WUN_ERR_UNSUPPORTED and "n_fft" in err()
    for num, den in ((65, 64), (3, 1), (1, 3)):
        assert call(t=with_(num=(1, num), den=(1, den), n_out=(1, 1))) == WUN_ERR_UNSUPPORTED, (num, den)
    # the longest legal output passes that check: 1/1 and n_out = n_in reaches the next one (here: the overlap)
    t = with_(num=(0, 1), den=(0, 1), n_out=(0, 700), y=(0, 0x100000 + 8))
    assert call(t=t) == WUN_ERR_INVALID and "overlaps x of job 0" in err()
    # a bad job in the second launch set (job 70 of 80) is found before the first set is launched
    t = _jobs(80)
    t["n_out"][70] = 631
    assert call(t=t) == WUN_ERR_INVALID and "job 70" in err()
    t = _jobs(80)
    t["den"][70] = 0
    assert call(t=t) == WUN_ERR_INVALID and "job 70" in err()
    # y over an x: its own, another job's, one in the other launch set; touching ranges are legal up to that check
    for j, i in ((1, 1), (2, 0), (3, 75), (75, 3)):
        t = _jobs(80)
        t["y"][j] = t["x"][i] + 4 * (700 * 2 - 1)                    # the last float of x
        assert call(t=t) == WUN_ERR_INVALID and "y of job %d overlaps x of job %d" % (j, i) in err(), (j, i)
    t = _jobs(80)
    t["y"][5] = t["x"][9] - 4 * 630 * 2 + 4                          # the last float of y on the first of x
    assert call(t=t) == WUN_ERR_INVALID and "y of job 5 overlaps x of job 9" in err()
    # the Python wrappers carry the library's words
    with pytest.raises(ValueError, match="GPU"):
        vocoder.time_stretch(np.zeros((10, 1), np.float32), 10, 9)
    with pytest.raises(ValueError, match="GPU"):
        vocoder.pitch_shift(np.zeros((10, 1), np.float32), 18, 17)


# ---------------------------------------------------------------------------------------- the oracle on known answers
def test_oracle_identity_length_and_tone():
    rng = np.random.default_rng(0)
    x = rng.normal(0, 0.5, (1500, 2)).astype(np.float32)
    for n_fft, hop in ((64, 16), (256, 64)):
        y = vnp.time_stretch(x, 1, 1, n_fft, hop)
        assert y.shape == x.shape and np.abs(y - x).max() < 1e-6          # the float32 rounding of the increment: ~1e-7
    f0 = 16.0 / 256.0
    tone = (0.5 * np.sin(2.0 * np.pi * f0 * np.arange(4000)))[:, None].astype(np.float32)
    for num, den in ((10, 9), (4, 5)):
        y = vnp.time_stretch(tone, num, den, 256, 64)
        assert y.shape == (_ceil(4000 * den, num), 1)
        assert abs(vnp.peak_frequency(y[:, 0], 512) - f0) < 1e-6 * f0     # a bin-centred tone keeps its frequency
        short = vnp.time_stretch(tone, num, den, 256, 64, n_out=1000)
        assert short.shape == (1000, 1) and np.abs(short[:700] - y[:700]).max() < 1e-12   # a cut output is a prefix away from its end


# ---------------------------------------------------------------------------------------- the descriptor stream
class _RecordingAug(object):
    """Generator that logs every draw the augmentations take, by kind and in order."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.log = []

    def random(self):
        r = self.rng.random()
        self.log.append(("u", float(r)))
        return r

    def integers(self, lo, hi, size=None, dtype=np.int64):
        assert size is None
        r = self.rng.integers(lo, hi, size=size, dtype=dtype)
        self.log.append(("i", int(lo), int(hi), int(r)))
        return r


def _span(key, ratio, t_in=T_IN):
    num, den = ratio
    n_out = datasets.speed_source_frames(t_in, num, den) if key == "pitch_shift" else t_in
    return _ceil(n_out * num, den), n_out


def test_draw_order_and_the_records_the_draws_give():
    cfg = _cfg()
    S = len(cfg["source_names"])
    augment = {"remix": 0.5, "speed": 0.3, "speed_rates": [[20, 19], [9, 8]], "pitch_shift": 0.4,
               "pitch_shift_rates": [[18, 17], [9, 8], [34, 36]], "time_stretch": 0.5, "time_stretch_rates": [[10, 9], [40, 42]]}
    active = datasets.check_augment(cfg, augment)
    assert active == {"remix": 0.5, "speed": 0.3, "pitch_shift": 0.4, "time_stretch": 0.5, "speed_rates": ((20, 19), (9, 8)),
                      "pitch_shift_rates": ((18, 17), (9, 8), (17, 18)), "time_stretch_rates": ((10, 9), (20, 21)),
                      "vocoder_fft": (2048, 512), "bank_rates": ((20, 19), (9, 8), (18, 17), (17, 18))}
    ratios = {"pitch_shift": active["pitch_shift_rates"], "time_stretch": active["time_stretch_rates"]}
    rec_rng = _RecordingAug(5)
    got = datasets.vocoder_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(21), augment, rec_rng)
    base = datasets.snippet_descriptors(cfg, LENGTHS, T_IN, T_OUT, "train", np.random.default_rng(21))
    seen = set()
    for _ in range(150):
        k0 = len(rec_rng.log)
        rec, mix_mode, rate, jobs = next(got)
        ti, pos, gains = next(base)                                 # the base stream is untouched by the draws
        log = rec_rng.log[k0:]
        assert mix_mode == 1 and rate.dtype == np.uint8 and rate.shape == (S,) and jobs.dtype == np.int64 and jobs.shape == (S, 4)
        where = [(ti, pos)] * S
        k = 1
        remixed = log[0][1] < 0.5                                   # 1. remix
        if remixed:
            for s in range(1, S):
                where[s] = (log[k][3], log[k + 1][3])
                k += 2
        took = None
        for key, p, R in (("speed", 0.3, 2), ("pitch_shift", 0.4, 3), ("time_stretch", 0.5, 2)):    # 2. speed, then the two new keys
            assert log[k][0] == "u"
            hit = log[k][1] < p
            k += 1
            if not hit:
                continue
            n = S if remixed else 1                                 #    one pick per source of a remixed snippet, else one for all
            assert all(e[:3] == ("i", 0, R) for e in log[k:k + n])
            picks = [e[3] for e in log[k:k + n]] * (1 if remixed else S)
            k += n
            took = key
            break                                                   #    a snippet that took one draws nothing for the later ones
        assert len(log) == k
        seen.add((remixed, took))
        for s in range(S):
            tj, p = where[s]
            if took in (None, "speed"):
                assert not jobs[s].any()
                continue
            num, den = ratios[took][picks[s]]
            n_span, n_out = _span(took, (num, den))
            assert LENGTHS[tj] >= n_span                            # (these tracks are long enough for every ratio)
            start = OFFSETS[tj] + min(max(p + (T_IN - n_span) // 2, 0), LENGTHS[tj] - n_span)
            assert tuple(jobs[s]) == (start, n_span, num, den) and rec["start"][s] == start
            assert rate[s] == (active["bank_rates"].index((num, den)) + 1 if took == "pitch_shift" else 0)
            assert n_out <= vnp.stretch_frames(n_span, num, den)    # the job is legal
    assert seen == {(r, t) for r in (False, True) for t in (None, "speed", "pitch_shift", "time_stretch")}


def test_without_the_new_keys_the_stream_is_speed_descriptors_own():
    cfg = _cfg()
    for augment in (None, {}, {"remix": 0.5, "polarity": 0.5, "speed": 0.5}, {"speed": 1, "pitch_shift": 0, "time_stretch": 0.0}):
        plain = None if augment is None else {k: v for k, v in augment.items() if k not in datasets.VOCODER_KEYS}
        a_rng, b_rng = _RecordingAug(9), _RecordingAug(9)
        a = datasets.speed_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(4), plain, a_rng)
        b = datasets.vocoder_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(4), augment, b_rng)
        for _ in range(30):
            (ra, ma, ta), (rb, mb, tb, jobs) = next(a), next(b)
            assert np.array_equal(ra, rb) and ma == mb and np.array_equal(ta, tb) and jobs.shape == (len(ra), 4) and not jobs.any()
        assert a_rng.log == b_rng.log
    # with an active new key the earlier generators point at the new one
    for gen in (datasets.augmented_descriptors, datasets.speed_descriptors):
        for key in datasets.VOCODER_KEYS:
            with pytest.raises(ValueError, match="vocoder_descriptors"):
                next(gen(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(4), {key: 0.5}))
    # speed_descriptors keeps its 3-tuples, augmented_descriptors its 2-tuples
    assert len(next(datasets.speed_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(4), {"speed": 1}))) == 3
    assert len(next(datasets.augmented_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(4), {"remix": 1}))) == 2


def test_placement_and_fallback():
    cfg = _cfg(augmentation=False)
    S = len(cfg["source_names"])
    # Tin = 90: time_stretch 10/9 reads 100 frames; pitch_shift (17, 18) stretches ceil(95 * 17 / 18) = 90 frames to 95, which
    # the gather resamples to 90 -- a pitch shift reads about Tin frames whatever its ratio
    assert _span("time_stretch", (10, 9)) == (100, 90) and _span("pitch_shift", (17, 18)) == (90, 95)
    assert _span("pitch_shift", (18, 17)) == (90, 85)
    lengths, offsets = [95, 400], [0, 95]
    for key, ratio in (("time_stretch", (10, 9)), ("pitch_shift", (17, 18))):
        n_span, _ = _span(key, ratio)
        for remix in (0, 1):
            augment = {key: 1, key + "_rates": [list(ratio)], "remix": remix}
            got = datasets.vocoder_descriptors(cfg, lengths, 90, 40, np.random.default_rng(8), augment)
            plain = datasets.vocoder_descriptors(cfg, lengths, 90, 40, np.random.default_rng(8), {"remix": remix})
            short = long_ = 0
            for _ in range(60):
                rec, mode, rate, jobs = next(got)
                prec = next(plain)[0]
                assert mode == 1
                for s in range(S):
                    tj = int(rec["start"][s] >= 95)
                    local = int(rec["start"][s]) - offsets[tj]
                    if tj == 0 and (n_span > 95):
                        assert not jobs[s].any() and rate[s] == 0 and 0 <= local <= 95 - 90       # the plain window ...
                        assert remix or rec["start"][s] == prec["start"][s]                       # ... where it was
                        short += 1
                    else:
                        assert jobs[s][1] == n_span and 0 <= local <= lengths[tj] - n_span and jobs[s][0] == rec["start"][s]
                        assert tuple(jobs[s][2:]) == ratio and rate[s] == (1 if key == "pitch_shift" else 0)
                        lo = (90 - n_span) // 2
                        if not remix and 0 < local < lengths[tj] - n_span:     # away from the edges: centred on the plain window
                            assert local - lo == int(prec["start"][s]) - offsets[tj]
                        long_ += 1
                if not remix:                                           # stems of one song: together, fallback included
                    assert len(set(rec["start"].tolist())) == 1 and len({tuple(j) for j in jobs}) == 1
            assert long_ > 10 and (short > 10 or n_span <= 95)
    # 90 frames fit a track of 95: no fallback for that ratio; 100 do not
    assert _span("pitch_shift", (17, 18))[0] <= 95 < _span("time_stretch", (10, 9))[0]


def test_value_errors_and_what_stays_as_it_was():
    cfg = _cfg()

    def first(augment):
        return next(datasets.vocoder_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(1), augment))
    first({"pitch_shift": 0.5})
    first({"time_stretch": 1, "time_stretch_rates": [[2, 1], [1, 2], [64, 63]], "vocoder_fft": [64, 16]})
    first({"speed": 1, "speed_rates": [[10, 9], [20, 19], [20, 21], [10, 11]], "pitch_shift": 1})          # 4 + 4: the bank is full
    first({"speed": 1, "speed_rates": [[18, 17], [9, 8], [3, 2], [2, 3], [5, 4], [4, 5]], "pitch_shift": 1})   # 6 + 2 new
    for bad in ({"pitch": 0.5}, {"pitch_shift": 1.5}, {"time_stretch": -0.1}, {"pitch_shift": float("nan")}, {"time_stretch": "slow"},
                {"pitch_shift": None}, {"pitch_shift": True},
                {"pitch_shift_rates": [[18, 17]]}, {"time_stretch_rates": [[10, 9]]},                       # without their key
                {"pitch_shift": 0, "pitch_shift_rates": [[18, 17]]}, {"time_stretch": 1, "pitch_shift_rates": [[18, 17]]},
                {"speed": 1, "time_stretch_rates": [[10, 9]]}, {"vocoder_fft": [256, 64]}, {"speed": 1, "vocoder_fft": [256, 64]},
                {"pitch_shift": 1, "pitch_shift_rates": [[1, 1]]}, {"time_stretch": 1, "time_stretch_rates": [[7, 7]]},
                {"pitch_shift": 1, "pitch_shift_rates": [[18, 17], [36, 34]]}, {"time_stretch": 1, "time_stretch_rates": []},
                {"pitch_shift": 1, "pitch_shift_rates": [[65, 64]]}, {"time_stretch": 1, "time_stretch_rates": [[3, 1]]},
                {"time_stretch": 1, "time_stretch_rates": [[10.0, 9.0]]}, {"pitch_shift": 1, "pitch_shift_rates": "18/17"},
                {"pitch_shift": 1, "pitch_shift_rates": [[k + 10, k + 9] for k in range(9)]},
                {"pitch_shift": 1, "vocoder_fft": [100, 25]}, {"pitch_shift": 1, "vocoder_fft": [256, 128]},
                {"pitch_shift": 1, "vocoder_fft": [256, 48]}, {"time_stretch": 1, "vocoder_fft": [16384, 512]},
                {"time_stretch": 1, "vocoder_fft": [32, 8]}, {"time_stretch": 1, "vocoder_fft": 2048},
                {"time_stretch": 1, "vocoder_fft": [2048, 512, 1]}, {"time_stretch": 1, "vocoder_fft": [2048.0, 512]},
                # the union of the two banks: 5 + 4 new, 8 + 1 new
                {"speed": 1, "speed_rates": [[10, 9], [20, 19], [20, 21], [10, 11], [3, 2]], "pitch_shift": 1},
                {"speed": 1, "speed_rates": [[k + 10, k + 9] for k in range(8)], "pitch_shift": 1, "pitch_shift_rates": [[18, 17]]}):
        with pytest.raises(ValueError):
            first(bad)
        with pytest.raises(ValueError):
            datasets.check_augment(cfg, bad)
    # a shared ratio takes one entry of the bank
    act = datasets.check_augment(cfg, {"speed": 1, "speed_rates": [[k + 10, k + 9] for k in range(8)], "pitch_shift": 1,
                                       "pitch_shift_rates": [[12, 11], [34, 32]]})
    assert act["bank_rates"] == act["speed_rates"] and act["pitch_shift_rates"] == ((12, 11), (17, 16))
    # a vocoder_fft the Python check passes is one the library passes, and the reverse
    lib = _lib.load()
    t = vocoder.job_table([(0x1000, 0x100000, 100, 50, 1, 1)])
    for n_fft in (32, 64, 96, 256, 8192, 16384):
        for hop in (1, 3, 16, 64, 2048, 4096):
            try:
                datasets.check_augment(cfg, {"time_stretch": 1, "vocoder_fft": [n_fft, hop]})
                ok = True
            except ValueError:
                ok = False
            assert ok == (lib.wun_time_stretch_scratch_floats(t.ctypes.data, 1, 2, n_fft, hop) > 0), (n_fft, hop)
    # what check_augment returns for the earlier keys has not changed, nor the tuple of keys
    assert datasets.check_augment(cfg, {"remix": 0.5, "channel_swap": 0, "polarity": 1}) == {"remix": 0.5, "polarity": 1.0}
    assert datasets.check_augment(cfg, {"speed": 0.25}) == {"speed": 0.25, "speed_rates": ((10, 9), (20, 19), (20, 21), (10, 11))}
    assert datasets.AUGMENT_KEYS == ("remix", "channel_swap", "polarity", "speed")
    assert datasets.VOCODER_KEYS == ("pitch_shift", "time_stretch")
    assert datasets.check_augment(cfg, {"pitch_shift": 0.5, "time_stretch": 0.25}) == {
        "pitch_shift": 0.5, "time_stretch": 0.25, "pitch_shift_rates": ((18, 17), (9, 8), (17, 18), (8, 9)),
        "time_stretch_rates": ((10, 9), (20, 19), (20, 21), (10, 11)), "vocoder_fft": (2048, 512),
        "bank_rates": ((18, 17), (9, 8), (17, 18), (8, 9))}
    # the producer selection: the new keys are the fused producer's, on the train partition only
    fcfg = dict(cfg, data_producer="fused", augment={"pitch_shift": 0.5, "time_stretch": 0.5})
    assert validation.data_producer(fcfg) == "fused"
    for bad in (dict(cfg, augment={"pitch_shift": 0.5}), dict(cfg, data_producer="torch", augment={"time_stretch": 0.5}),
                dict(cfg, data_producer="fused", augment={"vocoder_fft": [256, 64]})):
        with pytest.raises(ValueError):
            validation.data_producer(bad)
