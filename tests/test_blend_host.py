"""CPU-only checks of blended separation (include/wun.h: wun_blend_positions, wun_blend_windows, wun_blend_finish,
wun_separate_track_blend; wave_u_net_amd/blend.py): the window table against a Python loop, every refusal of
the device entries before any GPU work (no device here), properties of the numpy statement tests/_blend_np.py, blend.py's CPU
path against that statement bit for bit, and evaluate.separate_track(overlap=.., shifts=..) on a numpy stand-in."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _blend_np as bn

import wave_u_net_amd as wun
from wave_u_net_amd import _lib, blend, evaluate
from wave_u_net_amd.evaluate import separate_track
from wave_u_net_amd.separator import UnetAudioSeparator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WUN_ERR_INVALID = -1
_FAKE = C.c_void_p(0x1000)          # non-null, 16-byte aligned, never dereferenced: every call below fails a check first


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_declared_exported_and_bound(lib):
    assert lib.wun_blend_abi_size() == C.sizeof(_lib.WunBlendWindow) == 16
    assert [n for n, _ in _lib.WunBlendWindow._fields_] == ["pos", "row", "flags"]
    assert (_lib.BLEND_NO_RISE, _lib.BLEND_NO_FALL) == (1, 2) == (bn.NO_RISE, bn.NO_FALL)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("wun_blend_positions", "wun_blend_windows", "wun_blend_finish", "wun_separate_track_blend"):
        assert name in doc, name


def _table(lib, tout, n, v, s):
    k = lib.wun_blend_positions(tout, n, v, s, None, 0)
    assert k > 0, lib.wun_last_error().decode()
    buf = (_lib.WunBlendWindow * k)()
    assert lib.wun_blend_positions(tout, n, v, s, buf, k) == k
    return [(w.pos, w.row, w.flags) for w in buf]


def _python_pass(tout, n, v, s):
    """The rule of the header in a plain loop: windows at k H - s until one reaches the end of the track."""
    h, out, k = tout - v, [], 0
    while True:
        out.append(k * h - s)
        if k * h - s + tout >= n:
            break
        k += 1
    return out


@pytest.mark.parametrize("tout", [1, 5, 37, 1031])
def test_positions_are_the_python_rule(lib, tout):
    grid = []
    for v in sorted({0, 1, tout // 3, tout - 1}):
        if v > tout - 1:
            continue
        h = tout - v
        for n in sorted({1, tout, tout + 1, 3 * tout + 2, tout + 4 * h, tout + 4 * h - 1, tout + 4 * h + 1}):
            for s in (0, 1, tout - 1, tout, tout + 3, 2 * tout + 1):
                grid.append((v, n, s))
        grid.append((v, tout + 4 * h - 2, 2))                 # with s = 2 the last window ends exactly at n
    for v, n, s in grid:
        got = _table(lib, tout, n, v, s)
        want = _python_pass(tout, n, v, s)
        assert [p for p, _, _ in got] == want, (tout, n, v, s)
        assert [r for _, r, _ in got] == list(range(len(want)))
        flags = [(bn.NO_RISE if k == 0 else 0) | (bn.NO_FALL if k == len(want) - 1 else 0) for k in range(len(want))]
        assert [f for _, _, f in got] == flags
        assert got == bn.pass_windows(tout, n, v, s)          # ... and the statement's own table
        assert got[-1][0] + tout >= n and (len(got) == 1 or got[-2][0] + tout < n)
    # n == Tout, no shift: one window with both flags
    assert _table(lib, tout, tout, 0, 0) == [(0, 0, bn.NO_RISE | bn.NO_FALL)]
    tab = blend.window_table(tout, 3 * tout + 2, tout // 3, [0, 2])
    assert tab.dtype == np.int64 and [tuple(r) for r in tab.tolist()] == bn.window_list(tout, 3 * tout + 2, tout // 3, [0, 2])


def test_last_window_ending_exactly_at_n(lib):
    got = _table(lib, 10, 34, 2, 0)                           # H = 8: windows at 0, 8, 16, 24; 24 + 10 == 34
    assert [p for p, _, _ in got] == [0, 8, 16, 24]
    assert [p for p, _, _ in _table(lib, 10, 35, 2, 0)] == [0, 8, 16, 24, 32]
    assert [p for p, _, _ in _table(lib, 10, 31, 2, 3)] == [-3, 5, 13, 21]     # 21 + 10 == 31


def test_positions_argument_errors(lib):
    buf = (_lib.WunBlendWindow * 4)()
    assert lib.wun_blend_positions(0, 10, 0, 0, buf, 4) == WUN_ERR_INVALID
    assert lib.wun_blend_positions(10, 0, 0, 0, buf, 4) == WUN_ERR_INVALID
    assert lib.wun_blend_positions(10, 40, -1, 0, buf, 4) == WUN_ERR_INVALID
    assert lib.wun_blend_positions(10, 40, 10, 0, buf, 4) == WUN_ERR_INVALID       # V = Tout: no stride left
    assert "overlap" in lib.wun_last_error().decode()
    assert lib.wun_blend_positions(10, 40, 0, -1, buf, 4) == WUN_ERR_INVALID
    assert "shift" in lib.wun_last_error().decode()
    assert lib.wun_blend_positions(10, 41, 0, 0, buf, 4) == WUN_ERR_INVALID        # 5 windows, cap 4
    assert "cap" in lib.wun_last_error().decode()
    assert lib.wun_blend_positions(10, 40, 0, 0, buf, 4) == 4
    assert lib.wun_blend_positions(10, 41, 0, 0, None, 0) == 5                     # count only
    with pytest.raises(ValueError):
        blend.window_table(10, 40, 10, [0])
    with pytest.raises(ValueError):
        blend.window_table(10, 40, 0, [])
    assert blend.shift_offsets(4, 11025) == [0, 2756, 5512, 8268] == [j * 11025 // 4 for j in range(4)]
    assert blend.shift_offsets(1, 7) == [0] and blend.shift_offsets(3, 0) == [0, 0, 0]
    with pytest.raises(ValueError):
        blend.shift_offsets(0, 5)


def _wins(*rows):
    buf = (_lib.WunBlendWindow * len(rows))()
    for i, (pos, row, flags) in enumerate(rows):
        buf[i].pos, buf[i].row, buf[i].flags = pos, row, flags
    return buf


def test_blend_windows_argument_errors_without_a_device(lib):
    def call(outs=_FAKE, S=2, B=3, tout=10, ch=2, wins=_wins((0, 0, 1), (8, 1, 0), (16, 2, 2)), nwin=3, v=2, preds=_FAKE,
             den=_FAKE, frames=26):
        return lib.wun_blend_windows(outs, S, B, tout, ch, wins, nwin, v, preds, den, frames, None)
    for kw in ({"outs": None}, {"wins": None}, {"preds": None}, {"den": None}):
        assert call(**kw) == WUN_ERR_INVALID, kw
        assert "null" in lib.wun_last_error().decode()
    for kw in ({"S": 0}, {"B": 0}, {"tout": 0}, {"ch": 0}, {"ch": 3}, {"nwin": 0}, {"nwin": -1}, {"v": -1}, {"v": 10},
               {"frames": -1}, {"wins": _wins((0, 3, 0)), "nwin": 1}, {"wins": _wins((0, -1, 0)), "nwin": 1},
               {"wins": _wins((0, 0, 4)), "nwin": 1}, {"wins": _wins((1 << 50, 0, 0)), "nwin": 1}):
        assert call(**kw) == WUN_ERR_INVALID, kw
    assert call(wins=_wins((0, 0, 4)), nwin=1) == WUN_ERR_INVALID and "flag" in lib.wun_last_error().decode()
    for kw in ({"outs": C.c_void_p(0x1002)}, {"preds": C.c_void_p(0x1001)}, {"den": C.c_void_p(0x1003)}):
        assert call(**kw) == WUN_ERR_INVALID, kw
        assert "aligned" in lib.wun_last_error().decode()


def test_blend_finish_argument_errors_without_a_device(lib):
    def call(preds=_FAKE, den=_FAKE, S=2, frames=26, ch=2):
        return lib.wun_blend_finish(preds, den, S, frames, ch, None)
    for kw in ({"preds": None}, {"den": None}, {"S": 0}, {"frames": -1}, {"ch": 0}, {"ch": 3},
               {"preds": C.c_void_p(0x1002)}, {"den": C.c_void_p(0x1001)}):
        assert call(**kw) == WUN_ERR_INVALID, kw


@pytest.fixture(scope="module")
def plan():
    """A small context plan: batch 3, Tin / Tout of get_padding(40).  Plans are host objects; no device is needed."""
    cfg = wun.get_config("baseline", num_layers=3, num_initial_filters=8, context=True, num_frames=40)
    sep = UnetAudioSeparator(cfg)
    i, o = sep.get_padding(np.array([1, 40, 0]))
    p = sep._plan(3, int(i[1]))
    return sep, p, int(i[1]), int(o[1])


def test_separate_track_blend_argument_errors_without_a_device(lib, plan):
    _, p, tin, tout = plan
    n, v, lead = 5 * tout + 3, tout // 4, 7
    shifts = (C.c_int64 * 2)(0, 7)
    need = lead + max(p for p, _, _ in bn.window_list(tout, n, v, [0, 7])) + tin   # the end of the farthest window

    def call(h_=p.handle, params=_FAKE, track=_FAKE, frames=need, lead_=lead, n_=n, v_=v, sh=shifts, nsh=2, ws=_FAKE,
             outs=_FAKE, preds=_FAKE, den=_FAKE):
        return lib.wun_separate_track_blend(h_, params, track, frames, lead_, n_, v_, sh, nsh, ws, outs, preds, den, None)
    for kw in ({"h_": None}, {"params": None}, {"track": None}, {"sh": None}, {"ws": None}, {"outs": None}, {"preds": None},
               {"den": None}):
        assert call(**kw) == WUN_ERR_INVALID, kw
        assert "null" in lib.wun_last_error().decode()
    for kw in ({"nsh": 0}, {"n_": 0}, {"v_": -1}, {"v_": tout}, {"lead_": -1}, {"frames": -1},
               {"sh": (C.c_int64 * 2)(0, -1)}):
        assert call(**kw) == WUN_ERR_INVALID, kw
    assert call(lead_=6) == WUN_ERR_INVALID                                    # lead below the largest shift
    msg = lib.wun_last_error().decode()
    assert "window 0 of pass 1" in msg and "outside" in msg
    assert call(frames=need - 1) == WUN_ERR_INVALID                            # one frame short behind the last hop
    msg = lib.wun_last_error().decode()
    assert "outside" in msg and re.search(r"window \d+ of pass [01]", msg)
    for kw in ({"track": C.c_void_p(0x1002)}, {"ws": C.c_void_p(0x1008)}, {"outs": C.c_void_p(0x1001)},
               {"preds": C.c_void_p(0x1002)}, {"den": C.c_void_p(0x1003)}):
        assert call(**kw) == WUN_ERR_INVALID, kw
        assert "aligned" in lib.wun_last_error().decode()


# ---- the numpy statement itself ----
GEOMETRIES = [(5, 23, 0, [0]), (5, 23, 2, [0]), (5, 23, 4, [0]), (37, 150, 12, [0]), (37, 150, 12, [0, 3, 41]),
              (37, 37, 36, [0, 5]), (12, 100, 6, [0]), (12, 100, 7, [2])]


@pytest.mark.parametrize("tout, n, v, shifts", GEOMETRIES)
def test_every_frame_of_a_track_level_table_is_covered(tout, n, v, shifts):
    wins = bn.window_list(tout, n, v, shifts)
    rows = [(p, g, f) for g, (p, _, f) in enumerate(wins)]
    x = np.ones((1, len(rows), tout, 1), np.float32)
    out, den = bn.blend(x, rows, v, n)
    assert np.all(den > 0)
    if len(shifts) == 1 and 2 * v <= tout:
        # One pass whose windows overlap in pairs only (V <= H): a frame lies in one window's flat part (den = 1 exactly) or in
        # one cross-fade, where den = fl(fl(a / (V + 1)) + fl(b / (V + 1))) with a + b = V + 1: each quotient is off by at most
        # 2^-25 (it is below 1), the sum's rounding by at most 2^-24 -- together within 2^-23 of 1.  (With V > H three or more
        # windows cover a frame and the trapezoids no longer sum to 1: den is then simply the sum, which the division removes.)
        assert np.abs(den.astype(np.float64) - 1.0).max() <= 2.0 ** -23
    # a mean of ones is one wherever the weights are exact enough: within 2 ulp
    assert np.abs(out - 1.0).max() <= 2.0 ** -22


def test_single_weight_one_cover_reproduces_the_input_bits():
    tout, n, v = 37, 150, 12
    wins = bn.pass_windows(tout, n, v, 0)
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, len(wins), tout, 2)).astype(np.float32)
    x[0, 1, 20, 0] = np.float32(1e-41)                                         # a denormal keeps its bits too
    out, den = bn.blend(x, wins, v, n)
    covers = np.zeros(n, int)
    for p, _, _ in wins:
        covers[max(p, 0):min(p + tout, n)] += 1
    single = np.flatnonzero(covers == 1)
    assert single.size > 0 and np.all(den[single] == 1.0)
    for p, row, flags in wins:
        for f in single:
            if p <= f < p + tout:
                assert np.array_equal(out[:, f].view(np.uint32), x[:, row, f - p].view(np.uint32))
    assert 0 in single and n - 1 in single                                     # the pass's first and last ramp are flat
    # (-0 is the one exception: fmaf(1, -0, +0) is +0)
    z = np.full((1, 1, 3, 1), -0.0, np.float32)
    out, _ = bn.blend(z, [(0, 0, 3)], 0, 3)
    assert np.all(out == 0) and not np.any(np.signbit(out))


def test_uncovered_frames_are_plus_zero():
    x = np.ones((1, 2, 4, 1), np.float32)
    out, den = bn.blend(x, [(0, 0, 0), (7, 1, 0)], 1, 12)
    assert np.all(den[4:7] == 0) and np.all(out[:, 4:7] == 0) and not np.any(np.signbit(out[:, 4:7]))
    assert den[11] == 0 and den[10] > 0


# ---- blend.py's CPU path against the statement ----
def _planted(rng, shape):
    x = rng.standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1)
    idx = rng.choice(flat.size, size=min(12, flat.size), replace=False)
    flat[idx[0::3]] = np.float32(-0.0)
    flat[idx[1::3]] = np.float32(1e-40)
    flat[idx[2::3]] = np.float32(-3e-39)
    return x


@pytest.mark.parametrize("chan", [1, 2])
@pytest.mark.parametrize("tout, v", [(5, 0), (5, 1), (5, 4), (37, 12), (37, 36), (64, 21)])
def test_cpu_path_equals_the_statement(tout, v, chan):
    rng = np.random.default_rng(100 * tout + 10 * v + chan)
    n = 3 * tout + 7
    wins = bn.window_list(tout, n, v, [0, 3]) + [(-tout + 2, 0, 0), (n - 3, 0, 3), (n + 5, 0, 0)]
    rows = [(p, g % 7, f) for g, (p, _, f) in enumerate(wins)]
    x = _planted(rng, (2, 7, tout, chan))
    want, want_den = bn.blend(x, rows, v, n)
    preds, den = torch.zeros((2, n, chan)), torch.zeros(n)
    tab = np.array(rows, dtype=np.int64)
    for k in range(0, len(rows), 5):                                           # any cut of the table: the same chain
        blend.blend_windows(torch.from_numpy(x), tab[k:k + 5], v, preds, den)
    assert np.array_equal(den.numpy().view(np.uint32), want_den.view(np.uint32))
    blend.blend_finish(preds, den)
    assert np.array_equal(preds.numpy().view(np.uint32), want.view(np.uint32))


def test_cpu_fma_rounds_once():
    """The double-rounding trap: a * b + c whose float64 sum is an exact float32 tie while the exact sum is not."""
    from _fma_chain_np import fmaf_np
    a = np.array([1.0 + 2.0 ** -23, 3.0, 1.5], np.float32)
    b = np.array([1.0 + 2.0 ** -23, 2.0 ** -30, 2.0 ** -60], np.float32)
    c = np.array([2.0 ** -24 - 2.0 ** -46, 1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24], np.float32)
    rng = np.random.default_rng(5)
    a = np.concatenate([a, rng.standard_normal(4096).astype(np.float32)])
    b = np.concatenate([b, rng.standard_normal(4096).astype(np.float32)])
    c = np.concatenate([c, (rng.standard_normal(4096) * 2.0 ** rng.integers(-30, 2, 4096)).astype(np.float32)])
    assert np.array_equal(blend._fma32(a, b, c).view(np.uint32), fmaf_np(a, b, c).view(np.uint32))


# ---- separate_track on a stand-in ----
class CropSeparator(object):
    """A numpy stand-in without a device: estimate i = centre crop * (i + 1)."""
    PAD = 16

    def __init__(self, cfg):
        self.cfg = cfg
        self.batches = []

    def get_padding(self, shape):
        c = 1 if self.cfg["mono_downmix"] else 2
        return np.array([shape[0], int(shape[1]) + 2 * self.PAD, c]), np.array([shape[0], int(shape[1]), c])

    def get_output(self, batch, training):
        assert training is False
        b = np.asarray(batch)
        self.batches.append(b.shape[0])
        core = b[:, self.PAD:b.shape[1] - self.PAD, :]
        return {n: core * np.float32(i + 1) for i, n in enumerate(self.cfg["source_names"])}


@pytest.mark.parametrize("overlap, shifts", [(0.25, None), (0.0, [0, 3, 70]), (0.5, 2)])
def test_separate_track_blends_on_the_stand_in(overlap, shifts):
    cfg = wun.get_config("baseline", num_frames=60, mono_downmix=False, context=True)
    n = 437
    audio = np.random.default_rng(7).uniform(-1, 1, (n, 2)).astype(np.float32)
    sep = CropSeparator(cfg)
    got = separate_track(cfg, sep, audio, cfg["expected_sr"], batch_hops=4, overlap=overlap, shifts=shifts, max_shift=50)
    v = int(round(overlap * 60))
    offsets = [0] if shifts is None else ([0, 25] if shifts == 2 else shifts)
    wins = bn.window_list(60, n, v, offsets)
    assert sum(sep.batches) == len(wins) and max(sep.batches) <= 4
    # the oracle on the crops the windows see
    lead = max(offsets)
    padded = np.zeros((lead + max(p for p, _, _ in wins) + 60 + 32 + n, 2), np.float32)
    padded[lead + 16:lead + 16 + n] = audio
    for i, name in enumerate(cfg["source_names"]):
        x = np.stack([padded[lead + p + 16:lead + p + 16 + 60] for p, _, _ in wins])[None] * np.float32(i + 1)
        want, _ = bn.blend(x, [(p, g, f) for g, (p, _, f) in enumerate(wins)], v, n)
        assert got[name].shape == (n, 2) and np.array_equal(got[name].view(np.uint32), want[0].view(np.uint32))
        # a pure crop: every window agrees on every frame, so the mean is the input up to the weights' rounding
        assert np.abs(got[name] - audio * (i + 1)).max() <= 4 * 2.0 ** -23 * (i + 1)


def test_plain_options_take_the_plain_path():
    cfg = wun.get_config("baseline", num_frames=60, mono_downmix=True, context=True)
    audio = np.random.default_rng(8).uniform(-1, 1, (437, 1)).astype(np.float32)
    want = separate_track(cfg, CropSeparator(cfg), audio, cfg["expected_sr"], batch_hops=4)
    for kw in ({"overlap": 0.0}, {"shifts": 0}, {"shifts": 1}, {"shifts": [0]}, {"overlap": 0, "shifts": None, "max_shift": 9}):
        sep = CropSeparator(cfg)
        got = separate_track(cfg, sep, audio, cfg["expected_sr"], batch_hops=4, **kw)
        assert all(np.array_equal(got[k], want[k]) for k in want), kw
        assert sum(sep.batches) == -(-max(437, 60 + 32) // 60)                  # the re-aligned grid, not the overhanging one


def test_option_errors_and_plumbing():
    cfg = wun.get_config("baseline", num_frames=60, context=True)
    audio = np.zeros((100, 1), np.float32)
    for kw in ({"overlap": 1.0}, {"overlap": -0.1}, {"overlap": "x"}, {"shifts": -1}, {"shifts": [0, -3]}, {"shifts": []},
               {"shifts": 2, "max_shift": -1}, {"shifts": [1.5]}, {"shifts": True}):
        with pytest.raises(ValueError):
            separate_track(cfg, CropSeparator(cfg), audio, cfg["expected_sr"], **kw)
    assert evaluate.blend_options(0.25, 4, None, 22050) == (0.25, [0, 2756, 5512, 8268])
    assert evaluate.blend_options(0, None, None, 22050) == (0.0, [0])
    # model_config["separation"] feeds the file-level programs; explicit arguments win
    assert wun.config.EXTENSION_DEFAULTS["separation"] is None and "separation" not in wun.config.BASE_MODEL_CONFIG
    cfg2 = dict(cfg, separation={"overlap": 0.25, "shifts": 4})
    assert evaluate.separation_options(cfg2) == {"overlap": 0.25, "shifts": 4, "max_shift": None}
    assert evaluate.separation_options(cfg2, overlap=0.5, max_shift=9) == {"overlap": 0.5, "shifts": 4, "max_shift": 9}
    assert evaluate.separation_options(cfg) == {"overlap": 0.0, "shifts": None, "max_shift": None}
    with pytest.raises(ValueError):
        evaluate.separation_options(dict(cfg, separation={"overlapp": 0.25}))
    for fn in (evaluate.produce_source_estimates, evaluate.evaluate_track, evaluate.produce_dataset_estimates):
        names = fn.__code__.co_varnames[:fn.__code__.co_argcount]
        assert names[-3:] == ("overlap", "shifts", "max_shift"), fn.__name__
    from wave_u_net_amd.__main__ import _parse, _separation
    _, _, over, opts = _parse(["evaluate", "with", "cfg.baseline", "data_root=/d", "estimates_path=/e", "overlap=0.25", "shifts=4"])
    assert opts["overlap"] == 0.25 and opts["shifts"] == 4
    assert _separation(opts, cfg) == {"overlap": 0.25, "shifts": 4, "max_shift": None}
    _, _, over, opts = _parse(["predict", "with", "cfg.baseline", "input_path=/x.wav", "shifts=[0,3,700]",
                               'model_config.separation={"overlap":0.5}'])
    assert _separation(opts, wun.get_config("baseline", **over)) == {"overlap": 0.5, "shifts": [0, 3, 700], "max_shift": None}
    with pytest.raises(SystemExit):
        _separation({"overlap": 1.5}, cfg)
