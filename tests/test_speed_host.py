"""CPU-only checks of speed perturbation in the fused batch producer (include/wun.h: wun_gather_snippets_speed,
wun_speed_source_frames, wun_speed_bank; datasets.speed_descriptors): the binding and the struct, the source-span rule against
brute force, every argument error of the entry before any GPU work (no device here), the numpy oracle of tests/_speed_np.py
against scipy's float64 resampler, the order and the source of the draws, the placement rule and every ValueError."""
import ctypes as C
import functools

import numpy as np
import pytest
from scipy.signal import firwin, resample_poly

import wave_u_net_amd as wun
from wave_u_net_amd import _lib, datasets, resample, validation

import _speed_np

WUN_ERR_INVALID, WUN_ERR_UNSUPPORTED = -1, -2
_FAKE = C.c_void_p(0x1000)          # non-null, 16-byte aligned, never dereferenced: every call below fails a check first
T_IN, T_OUT = 90, 40
RATIOS = [(10, 9), (20, 21), (3, 2), (1, 2), (2, 1), (64, 63)]
LENGTHS = [400, 257, 333]            # padded track lengths of a 3-track set
OFFSETS = [0, 400, 657]


def _cfg(name="full_multi_instrument", **kw):
    base = dict(batch_size=4, num_snippets_per_track=3, cache_size=5)
    base.update(kw)
    return wun.get_config(name, **base)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---------------------------------------------------------------------------------------- the C ABI
def test_symbols_struct_and_binding(lib):
    assert 8 == _lib.SPEED_RATES == datasets.SPEED_MAX_RATES and 64 == _lib.SPEED_MAX_RATIO == datasets.SPEED_MAX_RATIO
    assert lib.wun_speed_abi_size() == C.sizeof(_lib.WunSpeedBank) == 4 + 32 + 32 + 4 + 64      # 4 bytes of padding before the pointers
    for f, (off, size) in {"n": (0, 4), "up": (4, 32), "down": (36, 32), "table": (72, 64)}.items():
        fld = getattr(_lib.WunSpeedBank, f)
        assert (fld.offset, fld.size) == (off, size), f
    assert len(lib.wun_gather_snippets_speed.argtypes) == 15
    # the plain entry is what it was
    assert lib.wun_snippet_abi_size() == 16 and len(lib.wun_gather_snippets.argtypes) == 13 and _lib.SNIPPET_ROWS == 24


@pytest.mark.parametrize("up,down", RATIOS)
def test_source_frames_is_the_smallest_span(lib, up, down):
    for t_in in (1, 2, 41, 93, 2500, 147443):
        got = lib.wun_speed_source_frames(t_in, up, down)
        n = max(0, (t_in * down) // up - 3)                      # brute force from safely below
        while resample.frames(n, up, down) < t_in:
            n += 1
        assert resample.frames(max(n - 1, 0), up, down) < t_in or n == 0
        assert got == n == ((t_in - 1) * down) // up + 1 == datasets.speed_source_frames(t_in, up, down) == _speed_np.source_frames(t_in, up, down)


def test_source_frames_refuses_bad_arguments(lib):
    for t_in in (0, -1, -(1 << 40)):
        assert lib.wun_speed_source_frames(t_in, 10, 9) == WUN_ERR_INVALID
        assert "Tin" in lib.wun_last_error().decode()
    for up, down, word in ((0, 1, "positive"), (3, -2, "positive"), (4, 6, "coprime"), (20, 18, "coprime"), (1, 1, "1/1")):
        assert lib.wun_speed_source_frames(90, up, down) == WUN_ERR_INVALID, (up, down)
        assert word in lib.wun_last_error().decode()
    for up, down, word in ((65, 64, "ceiling"), (64, 65, "ceiling"), (1, 3, "[1/2, 2]"), (3, 1, "[1/2, 2]"), (31, 64, "[1/2, 2]")):
        assert lib.wun_speed_source_frames(90, up, down) == WUN_ERR_UNSUPPORTED, (up, down)
        assert word in lib.wun_last_error().decode()


def _bank(pairs=((10, 9), (20, 21)), n=None, tables=None):
    b = _lib.WunSpeedBank()
    b.n = len(pairs) if n is None else n
    for i, (up, down) in enumerate(pairs):
        b.up[i], b.down[i] = up, down
        b.table[i] = 0x4000 + 0x1000 * i if tables is None else tables[i]
    return b


def test_gather_speed_argument_errors_without_a_device(lib):
    frames, S, B = 1000, 2, 3

    def table(rows=B, start=0, gain=1.0, flags=0):
        t = np.zeros((rows, S), dtype=datasets.SNIPPET_DTYPE)
        t["start"], t["gain"], t["flags"] = start, gain, flags
        return t

    def rates(rows=B, fill=1):
        return np.full((rows, S), fill, dtype=np.uint8)

    def call(planes=(0x1000, 0x2000), mix_plane=_FAKE, frames=frames, c=2, s=S, b=B, tin=T_IN, tout=T_OUT, desc=None, rate=None,
             bank=None, mode=1, mix=_FAKE, tgt=_FAKE, null_planes=False, null_desc=False, null_rate=False, null_bank=False):
        desc = table(rows=b if b > 0 else B) if desc is None else desc
        rate = rates(rows=b if b > 0 else B) if rate is None else rate
        bank = _bank() if bank is None else bank
        arr = (C.c_void_p * 8)(*planes)
        return lib.wun_gather_snippets_speed(None if null_planes else arr, mix_plane, frames, c, s, b, tin, tout,
                                             None if null_desc else desc.ctypes.data, None if null_rate else rate.ctypes.data,
                                             None if null_bank else C.addressof(bank), mode, mix, tgt, None)

    def err():
        return lib.wun_last_error().decode()
    # everything the plain entry refuses, with rates and without
    for extra in ({}, {"null_rate": True, "null_bank": True}, {"rate": rates(fill=0)}):
        for kw in ({"null_planes": True}, {"null_desc": True}, {"mix": None}, {"tgt": None}, {"planes": (0x1000, 0)},
                   {"mix_plane": None, "mode": 0}):
            assert call(**dict(kw, **extra)) == WUN_ERR_INVALID, kw
            assert "null" in err()
        for kw in ({"mode": 2}, {"mode": -1}, {"c": 0}, {"c": 3}, {"s": 0}, {"s": 9}, {"b": 0}, {"b": -2},
                   {"tout": T_IN + 2}, {"tout": T_OUT + 1}, {"tout": 0}, {"frames": T_IN - 1}, {"frames": -1},
                   {"mix": C.c_void_p(0x1002)}, {"tgt": C.c_void_p(0x1001)}, {"planes": (0x1000, 0x2002)},
                   {"mix_plane": C.c_void_p(0x1003)}, {"desc": table(flags=4)}, {"c": 1, "desc": table(flags=1)}):
            assert call(**dict(kw, **extra)) == WUN_ERR_INVALID, kw
    # unit windows keep the rule with Tin, beside rated ones and alone
    for rate in (rates(fill=0), None):
        r = rates() if rate is None else rate
        r[1, 0] = 0
        for start in (-1, frames - T_IN + 1, 1 << 50):
            t = table()
            t["start"][1, 0] = start
            assert call(desc=t, rate=r) == WUN_ERR_INVALID
            assert "outside" in err() and "rated" not in err()
    # a rate index above bank->n
    for n, idx in ((2, 3), (2, 255), (1, 2), (0, 1)):
        r = rates()
        r[2, 1] = idx
        assert call(rate=r, bank=_bank(n=n)) == WUN_ERR_INVALID, (n, idx)
        assert "rate index" in err()
    # a non-zero rate with a null bank or with mix_mode 0
    assert call(null_bank=True) == WUN_ERR_INVALID and "bank" in err()
    r = rates(fill=0)
    r[2, 0] = 1
    assert call(rate=r, null_bank=True) == WUN_ERR_INVALID and "bank" in err()
    assert call(rate=r, mode=0) == WUN_ERR_INVALID and "mix_mode" in err()
    # the bank itself (checked whether or not a rate selects the entry)
    for rate in (None, rates(fill=0)):
        for n in (-1, 9, 1 << 20):
            assert call(rate=rate, bank=_bank(n=n)) == WUN_ERR_INVALID and "bank->n" in err()
        for pair, word in (((0, 1), "positive"), ((5, -4), "positive"), ((4, 6), "coprime"), ((20, 18), "coprime"), ((1, 1), "1/1")):
            assert call(rate=rate, bank=_bank(((10, 9), pair))) == WUN_ERR_INVALID, pair
            assert word in err() and "entry 1" in err()
        for pair, word in (((65, 64), "ceiling"), ((64, 65), "ceiling"), ((1, 3), "[1/2, 2]"), ((5, 2), "[1/2, 2]")):
            assert call(rate=rate, bank=_bank((pair, (10, 9)))) == WUN_ERR_UNSUPPORTED, pair
            assert word in err() and "entry 0" in err()
        assert call(rate=rate, bank=_bank(tables=(0x4000, 0))) == WUN_ERR_INVALID and "null table" in err()
        for bad in (0x5001, 0x5002, 0x5003):
            assert call(rate=rate, bank=_bank(tables=(0x4000, bad))) == WUN_ERR_INVALID and "aligned" in err()
    # a rated window: start < 0 or start + n_src > plane_frames, n_src of ITS entry
    n_slow, n_fast = ((T_IN - 1) * 9) // 10 + 1, ((T_IN - 1) * 21) // 20 + 1
    assert (n_slow, n_fast) == (81, 94)
    r = rates()
    r[:, 1] = 2
    for row, src, start in ((0, 0, -1), (1, 0, frames - n_slow + 1), (2, 1, frames - n_fast + 1), (1, 1, frames - T_IN + 1), (0, 1, 1 << 50)):
        t = table()
        t["start"][row, src] = start
        assert call(desc=t, rate=r) == WUN_ERR_INVALID, (row, src, start)
        assert "rated window" in err() and "outside" in err()
    # ... and the last legal starts pass that check (the call still fails, at a later row)
    t = table()
    t["start"][:, 0], t["start"][:, 1] = frames - n_slow, frames - n_fast
    r[2, 1] = 3
    assert call(desc=t, rate=r) == WUN_ERR_INVALID and "rate index" in err() and "row 2" in err()
    # a bad rate in a row of the SECOND launch: still before any GPU work
    rows = _lib.SNIPPET_ROWS + 1
    r = rates(rows=rows)
    r[-1, 1] = 3
    assert call(b=rows, rate=r) == WUN_ERR_INVALID and "rate index" in err() and "row %d" % (rows - 1) in err()
    t = table(rows=rows)
    t["start"][-1, 0] = frames - n_slow + 1
    assert call(b=rows, desc=t) == WUN_ERR_INVALID and "rated window" in err()


# ---------------------------------------------------------------------------------------- the oracle
@functools.lru_cache(maxsize=None)
def _abs_filter(up, down):
    """|h| of the design WITHOUT the factor `up`: scipy multiplies an array window by up itself."""
    mx = max(up, down)
    return np.abs(firwin(20 * mx + 1, 1.0 / mx, window=("kaiser", 5.0)))


@pytest.mark.parametrize("c", [1, 2])
@pytest.mark.parametrize("up,down", RATIOS)
def test_oracle_against_float64_resample_poly(up, down, c):
    """|r - y64| <= (K + 2) 2^-24 (|h| * |v|)[t] + 2^-24 |y64[t]|: the bound of tests/test_gpu_resample.py -- a length-K fp32 dot
    product accumulated in any order plus the rounding of the fp32 taps."""
    t_in = 93
    K = _speed_np.table(up, down).shape[1]
    assert K == -(-(20 * max(up, down) + 1) // up)
    n_src = _speed_np.source_frames(t_in, up, down)
    span = np.random.default_rng(up * 100 + down + c).uniform(-1, 1, (n_src, c)).astype(np.float32)
    r = _speed_np.resample_span(span, t_in, up, down)
    assert r.dtype == np.float32 and r.shape == (t_in, c)
    y64 = resample_poly(span.astype(np.float64), up, down, axis=0)
    assert y64.shape[0] >= t_in                                  # n_src frames are enough for the window
    mag = resample_poly(np.abs(span.astype(np.float64)), up, down, axis=0, window=_abs_filter(up, down))[:t_in]
    y64 = y64[:t_in]
    bound = (K + 2) * 2.0 ** -24 * mag + 2.0 ** -24 * np.abs(y64)
    err = np.abs(r.astype(np.float64) - y64)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("%d / %d, C = %d: max err %.3g, worst err / bound %.3f" % (up, down, c, err.max(), worst))
    assert np.all(err <= bound), worst


def test_oracle_unit_rate_is_the_plain_oracle():
    import _snippets_np
    plane = np.random.default_rng(2).uniform(-1, 1, (300, 2)).astype(np.float32)
    t = np.zeros((2, 1), dtype=datasets.SNIPPET_DTYPE)
    t["start"][:, 0], t["gain"][:, 0], t["flags"][:, 0] = [3, 200], [1.0, 0.8], [1, 2]
    mix, tgt = _speed_np.gather([plane], t, np.zeros((2, 1), np.uint8), [(10, 9)], T_IN, T_OUT)
    want_mix, want_tgt, _ = _snippets_np.gather([plane], None, t, 1, T_IN, T_OUT)
    assert np.array_equal(mix.view(np.int32), want_mix.view(np.int32)) and np.array_equal(tgt.view(np.int32), want_tgt.view(np.int32))


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


def _track_of(start):
    ti = int(np.searchsorted(np.cumsum(LENGTHS), start, side="right"))
    return ti, int(start) - OFFSETS[ti]


def test_draw_order_and_the_records_the_draws_give():
    cfg = _cfg()
    S = len(cfg["source_names"])
    bank = ((20, 19), (20, 21), (3, 2))
    augment = {"remix": 0.5, "channel_swap": 0.25, "polarity": 0.75, "speed": 0.6, "speed_rates": [[40, 38], [20, 21], (3, 2)]}
    assert datasets.check_augment(cfg, augment) == {"remix": 0.5, "channel_swap": 0.25, "polarity": 0.75, "speed": 0.6, "speed_rates": bank}
    rec_rng = _RecordingAug(5)
    got = datasets.speed_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(21), augment, rec_rng)
    base = datasets.snippet_descriptors(cfg, LENGTHS, T_IN, T_OUT, "train", np.random.default_rng(21))
    seen = set()
    for _ in range(80):
        k0 = len(rec_rng.log)
        rec, mix_mode, rate = next(got)
        ti, pos, gains = next(base)                                 # the base stream is untouched by the draws
        log = rec_rng.log[k0:]
        assert mix_mode == 1 and np.array_equal(rec["gain"], gains) and rate.dtype == np.uint8 and rate.shape == (S,)
        where = [(ti, pos)] * S
        assert log[0][0] == "u"
        k = 1
        remixed = log[0][1] < 0.5                                   # 1. remix; (track, start) per source >= 1
        if remixed:
            for s in range(1, S):
                assert log[k][:3] == ("i", 0, 3)
                tj = log[k][3]
                assert log[k + 1][:3] == ("i", 0, LENGTHS[tj] - T_IN)
                where[s] = (tj, log[k + 1][3])
                k += 2
        swap = [e[1] < 0.25 for e in log[k:k + S]]                  # 2. one uniform per source: swap
        neg = [e[1] < 0.75 for e in log[k + S:k + 2 * S]]           # 3. one uniform per source: polarity
        assert all(e[0] == "u" for e in log[k:k + 2 * S + 1])
        k += 2 * S
        taken = log[k][1] < 0.6                                     # 4. one uniform: speed
        k += 1
        picks = [None] * S
        if taken and remixed:                                       #    one pick per source ...
            assert all(e[:3] == ("i", 0, 3) for e in log[k:k + S])
            picks = [e[3] for e in log[k:k + S]]
            k += S
        elif taken:                                                 #    ... or one for all
            assert log[k][:3] == ("i", 0, 3)
            picks = [log[k][3]] * S
            k += 1
        assert len(log) == k
        assert list(rec["flags"]) == [int(a) * 1 + int(b) * 2 for a, b in zip(swap, neg)]
        for s in range(S):
            tj, p = where[s]
            if picks[s] is None:
                assert rate[s] == 0 and rec["start"][s] == OFFSETS[tj] + p
                continue
            n_src = datasets.speed_source_frames(T_IN, *bank[picks[s]])
            assert LENGTHS[tj] >= n_src and rate[s] == picks[s] + 1
            assert rec["start"][s] == OFFSETS[tj] + min(max(p + (T_IN - n_src) // 2, 0), LENGTHS[tj] - n_src)
        seen.add((remixed, taken))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}


def test_without_speed_the_stream_is_augmented_descriptors_own():
    cfg = _cfg()
    for augment in (None, {}, {"remix": 0.5, "polarity": 0.5}, {"remix": 0.5, "speed": 0}, {"speed": 0.0}):
        plain_aug = None if augment is None else {k: v for k, v in augment.items() if k != "speed"}
        a_rng, b_rng = _RecordingAug(9), _RecordingAug(9)
        a = datasets.augmented_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(4), plain_aug, a_rng)
        b = datasets.speed_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(4), augment, b_rng)
        c = datasets.augmented_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(4), augment, _RecordingAug(9))
        for _ in range(30):
            (ra, ma), (rb, mb, rate), (rc, mc) = next(a), next(b), next(c)
            assert np.array_equal(ra, rb) and np.array_equal(ra, rc) and ma == mb == mc and rate.dtype == np.uint8 and not rate.any()
        assert a_rng.log == b_rng.log
    # with an active speed the 2-tuple generator points at the new one
    with pytest.raises(ValueError, match="speed_descriptors"):
        next(datasets.augmented_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(4), {"speed": 0.5}))


def test_aug_rng_never_advances_rng_and_speed_makes_mix_mode_1():
    cfg = _cfg(augmentation=False)
    plain = datasets.speed_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(3))
    aug = datasets.speed_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(3), {"speed": 1})
    again = datasets.speed_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(3), {"speed": 1}, np.random.default_rng([1337, 1]))
    used = set()
    for _ in range(40):
        p, pmode, prate = next(plain)
        a, mode, rate = next(aug)
        b, _, brate = next(again)
        assert np.array_equal(a, b) and np.array_equal(rate, brate)               # the default second Generator
        assert pmode == 0 and mode == 1 and not prate.any() and rate.all()
        assert len(set(rate.tolist())) == 1 and len(set(a["start"].tolist())) == 1   # not remixed: one start, one rate
        ti, pos = _track_of(p["start"][0])
        n_src = datasets.speed_source_frames(T_IN, *datasets.SPEED_RATES_DEFAULT[rate[0] - 1])
        assert a["start"][0] == OFFSETS[ti] + min(max(pos + (T_IN - n_src) // 2, 0), LENGTHS[ti] - n_src)   # same base position
        used.add(int(rate[0]))
    assert used == {1, 2, 3, 4}


def test_placement_spans_stay_inside_their_track_and_short_tracks_fall_back():
    cfg = _cfg(augmentation=False)
    S = len(cfg["source_names"])
    # Tin = 90 at (10, 11) reads 98 frames: a padded track of 95 cannot, one of 400 can
    assert datasets.speed_source_frames(90, 10, 11) == 98 and datasets.speed_source_frames(90, 10, 9) == 81
    lengths, offsets = [95, 400], [0, 95]
    for augment in ({"speed": 1, "speed_rates": [[10, 11]]}, {"speed": 1, "remix": 1, "speed_rates": [[10, 11]]}):
        got = datasets.speed_descriptors(cfg, lengths, 90, 40, np.random.default_rng(8), augment)
        short = long_ = 0
        for _ in range(60):
            rec, mode, rate = next(got)
            for s in range(S):
                tj = int(rec["start"][s] >= 95)
                local = int(rec["start"][s]) - offsets[tj]
                if tj == 0:
                    assert rate[s] == 0 and 0 <= local <= 95 - 90      # the unit window, where it was
                    short += 1
                else:
                    assert rate[s] == 1 and 0 <= local <= 400 - 98
                    long_ += 1
            if "remix" not in augment:                                 # stems of one song: together, fallback included
                assert len(set(rec["start"].tolist())) == 1 and len(set(rate.tolist())) == 1
        assert short > 10 and long_ > 10
    # every span inside its track, all default rates, remixed or not; the centre rule is met away from the edges
    for augment in ({"speed": 1}, {"speed": 1, "remix": 0.5, "polarity": 0.5}):
        got = datasets.speed_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(8), augment)
        clipped = centred = 0
        for _ in range(150):
            rec, mode, rate = next(got)
            for s in range(S):
                ti, local = _track_of(rec["start"][s])
                assert rate[s] >= 1
                n_src = datasets.speed_source_frames(T_IN, *datasets.SPEED_RATES_DEFAULT[rate[s] - 1])
                assert 0 <= local and local + n_src <= LENGTHS[ti]
                lo = (T_IN - n_src) // 2
                # local = clip(pos + lo, 0, len - n_src) for a pos in [0, len - Tin): away from both edges the centres agree
                if 0 < local < LENGTHS[ti] - n_src:
                    pos = local - lo
                    assert 0 <= pos < LENGTHS[ti] - T_IN
                    assert abs((2 * local + n_src) - (2 * pos + T_IN)) <= 1
                    centred += 1
                else:
                    clipped += 1
        assert centred > 100 and clipped >= 1


def test_value_errors():
    cfg = _cfg()

    def first(augment):
        return next(datasets.speed_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(1), augment))
    first({"speed": 0.5})
    first({"speed": 1, "speed_rates": [[2, 1], [1, 2], [64, 63], [63, 64], [3, 2], [2, 3], [5, 4], [4, 5]]})   # 8 pairs, the limits
    for bad in ({"pitch": 0.5}, {"speed": 1.5}, {"speed": -0.1}, {"speed": float("nan")}, {"speed": "fast"}, {"speed": None},
                {"speed_rates": [[10, 9]]},                                      # without speed
                {"speed": 0, "speed_rates": [[10, 9]]},                          # speed not active
                {"remix": 0.5, "speed_rates": [[10, 9]]},
                {"speed": 0.5, "speed_rates": [[1, 1]]}, {"speed": 0.5, "speed_rates": [[7, 7]]},          # 1/1, also after reduction
                {"speed": 0.5, "speed_rates": [[10, 9], [20, 18]]},              # duplicates after reduction
                {"speed": 0.5, "speed_rates": [[10, 9]] * 2},
                {"speed": 0.5, "speed_rates": [[k + 10, k + 9] for k in range(9)]},                        # more than 8
                {"speed": 0.5, "speed_rates": []},
                {"speed": 0.5, "speed_rates": [[65, 64]]}, {"speed": 0.5, "speed_rates": [[1, 3]]},        # what the library refuses
                {"speed": 0.5, "speed_rates": [[5, 2]]}, {"speed": 0.5, "speed_rates": [[0, 1]]},
                {"speed": 0.5, "speed_rates": [[10, -9]]}, {"speed": 0.5, "speed_rates": [[10.0, 9.0]]},
                {"speed": 0.5, "speed_rates": [[10, 9, 8]]}, {"speed": 0.5, "speed_rates": "10/9"},
                {"speed": 0.5, "speed_rates": [10, 9]}, {"speed": 0.5, "speed_rates": 0.9}):
        with pytest.raises(ValueError):
            first(bad)
        with pytest.raises(ValueError):
            datasets.check_augment(cfg, bad)
    # a pair the Python check passes is one the library passes, and the reverse, over the whole grid
    lib = _lib.load()
    for up in range(1, 70):
        for down in range(1, 70):
            try:
                datasets.check_augment(cfg, {"speed": 1, "speed_rates": [[up, down]]})
                ok = True
            except ValueError:
                ok = False
            g = int(np.gcd(up, down))
            assert ok == (lib.wun_speed_source_frames(T_IN, up // g, down // g) > 0), (up, down)
    # what check_augment returns for the three earlier keys has not changed
    assert datasets.check_augment(cfg, {"remix": 0.5, "channel_swap": 0, "polarity": 1}) == {"remix": 0.5, "polarity": 1.0}
    assert datasets.check_augment(cfg, {"speed": 0.25}) == {"speed": 0.25, "speed_rates": ((10, 9), (20, 19), (20, 21), (10, 11))}
    assert datasets.AUGMENT_KEYS == ("remix", "channel_swap", "polarity", "speed")
    # the producer selection and the source: speed is the fused producer's, on the train partition only
    fcfg = dict(cfg, data_producer="fused", augment={"speed": 0.5, "speed_rates": [[20, 19], [20, 21]]})
    assert validation.data_producer(fcfg) == "fused"
    for bad in (dict(cfg, augment={"speed": 0.5}), dict(cfg, data_producer="torch", augment={"speed": 0.5}),
                dict(cfg, data_producer="fused", augment={"speed_rates": [[10, 9]]})):
        with pytest.raises(ValueError):
            validation.data_producer(bad)
    rng = np.random.default_rng(0)
    tracks = [datasets.make_track({k: rng.uniform(-0.4, 0.4, (n, 2)).astype(np.float32) for k in cfg["source_names"]}, cfg)
              for n in (400, 300)]
    with pytest.raises(RuntimeError):                                        # no CPU fallback
        datasets.FusedSnippetSource(cfg, tracks, T_IN, T_OUT, 4, "cpu", augment={"speed": 0.5})
    with pytest.raises(ValueError):
        datasets.FusedSnippetSource(cfg, tracks, T_IN, T_OUT, 4, "cpu", augment={"speed": 0.5, "speed_rates": [[1, 1]]})
    with pytest.raises(ValueError):
        datasets.FusedSnippetSource(cfg, tracks, T_IN, T_OUT, 4, "cpu", augment={"speed": 1}, partition="valid")


def test_cli_overrides_carry_speed_and_its_rates():
    from wave_u_net_amd.__main__ import _parse
    _, name, overrides, _ = _parse(["train", "with", "cfg.baseline_stereo", "model_config.data_producer=fused",
                                    'model_config.augment={"speed":0.5,"speed_rates":[[20,19],[20,21]]}', "data_root=/x"])
    cfg = wun.get_config(name, **overrides)
    assert validation.data_producer(cfg) == "fused" and cfg["augment"] == {"speed": 0.5, "speed_rates": [[20, 19], [20, 21]]}
    assert datasets.check_augment(cfg, cfg["augment"]) == {"speed": 0.5, "speed_rates": ((20, 19), (20, 21))}
