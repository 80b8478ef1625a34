"""CPU-only checks of whole-track separation (include/wun.h: wun_separate_positions, wun_forward_windows,
wun_scatter_windows, wun_separate_track): the hop table against evaluate._hop_positions, every argument error of the three
device entries before any GPU work (no device here), and evaluate.separate_track(hop_frames=...) on a numpy stand-in."""
import ctypes as C

import numpy as np
import pytest

import wave_u_net_amd as wun
from wave_u_net_amd import _lib
from wave_u_net_amd import evaluate
from wave_u_net_amd.evaluate import _hop_positions, budget_batch_hops, hop_geometry, predict_track, separate_track
from wave_u_net_amd.separator import UnetAudioSeparator

WUN_ERR_INVALID = -1
_FAKE = C.c_void_p(0x1000)          # non-null, 16-byte aligned, never dereferenced: every call below fails a check first


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _positions(lib, t_out, n_frames):
    n = lib.wun_separate_positions(t_out, n_frames, None, 0)
    assert n > 0
    buf = (C.c_int64 * n)()
    assert lib.wun_separate_positions(t_out, n_frames, buf, n) == n
    return list(buf)


@pytest.mark.parametrize("t_out", [1, 7, 300, 16389])
def test_positions_are_the_python_rule(lib, t_out):
    lengths = {t_out, t_out + 1, 2 * t_out - 1, 2 * t_out, 2 * t_out + 1, 5 * t_out - 1, 5 * t_out, 5 * t_out + 1,
               5 * t_out + t_out // 2, 17 * t_out + 3}
    for n_frames in sorted(lengths):
        got = _positions(lib, t_out, n_frames)
        assert got == _hop_positions(n_frames, t_out), (t_out, n_frames)
        assert len(got) == -(-n_frames // t_out) and got[-1] == n_frames - t_out
    assert _positions(lib, t_out, t_out) == [0]


def test_positions_argument_errors(lib):
    buf = (C.c_int64 * 4)()
    assert lib.wun_separate_positions(0, 10, buf, 4) == WUN_ERR_INVALID
    assert lib.wun_separate_positions(10, 9, buf, 4) == WUN_ERR_INVALID          # shorter than one hop
    assert lib.wun_separate_positions(10, 41, buf, 4) == WUN_ERR_INVALID         # 5 hops, cap 4
    assert "cap" in lib.wun_last_error().decode()
    assert lib.wun_separate_positions(10, 40, buf, 4) == 4 and list(buf) == [0, 10, 20, 30]
    assert lib.wun_separate_positions(10, 41, None, 0) == 5                      # count only


@pytest.fixture(scope="module")
def plan():
    """A small context plan: batch 3, Tin / Tout of get_padding(40).  Plans are host objects; no device is needed."""
    cfg = wun.get_config("baseline", num_layers=3, num_initial_filters=8, context=True, num_frames=40)
    sep = UnetAudioSeparator(cfg)
    i, o = sep.get_padding(np.array([1, 40, 0]))
    p = sep._plan(3, int(i[1]))
    return sep, p, int(i[1]), int(o[1])


def _pos(*v):
    return (C.c_int64 * len(v))(*v)


def test_forward_windows_argument_errors_without_a_device(lib, plan):
    _, p, tin, tout = plan
    track_frames = 5 * tin

    def call(h=p.handle, params=_FAKE, track=_FAKE, frames=track_frames, pos=_pos(0, 1, 2), npos=3, ws=_FAKE, outs=_FAKE):
        return lib.wun_forward_windows(h, params, track, frames, pos, npos, ws, outs, 0, None)
    for kw in ({"h": None}, {"params": None}, {"track": None}, {"pos": None}, {"ws": None}, {"outs": None}):
        assert call(**kw) == WUN_ERR_INVALID, kw
        assert "null" in lib.wun_last_error().decode()
    assert call(npos=0) == WUN_ERR_INVALID
    assert call(npos=-1) == WUN_ERR_INVALID
    assert call(pos=_pos(0, 1, 2, 3), npos=4) == WUN_ERR_INVALID                 # npos > batch
    assert "npos" in lib.wun_last_error().decode()
    assert call(pos=_pos(0, -1, 2)) == WUN_ERR_INVALID
    assert call(pos=_pos(0, 1, track_frames - tin + 1)) == WUN_ERR_INVALID        # one frame past the end
    assert "outside" in lib.wun_last_error().decode()
    assert call(frames=tin - 1, pos=_pos(0), npos=1) == WUN_ERR_INVALID           # track shorter than a window
    assert call(frames=-1) == WUN_ERR_INVALID
    assert call(track=C.c_void_p(0x1002)) == WUN_ERR_INVALID                      # not a float address
    assert call(ws=C.c_void_p(0x1004)) == WUN_ERR_INVALID                         # the workspace rows are 16-byte aligned
    assert "aligned" in lib.wun_last_error().decode()


def test_scatter_windows_argument_errors_without_a_device(lib, plan):
    _, p, tin, tout = plan
    pred_frames = 4 * tout

    def call(h=p.handle, outs=_FAKE, pos=_pos(0, tout, 2 * tout), npos=3, preds=_FAKE, frames=pred_frames):
        return lib.wun_scatter_windows(h, outs, pos, npos, preds, frames, None)
    for kw in ({"h": None}, {"outs": None}, {"pos": None}, {"preds": None}):
        assert call(**kw) == WUN_ERR_INVALID, kw
    assert call(npos=0) == WUN_ERR_INVALID
    assert call(pos=_pos(0, 1, 2, 3), npos=4) == WUN_ERR_INVALID
    assert call(pos=_pos(0, tout, 3 * tout + 1)) == WUN_ERR_INVALID
    assert "outside" in lib.wun_last_error().decode()
    assert call(pos=_pos(-1, tout, 2 * tout)) == WUN_ERR_INVALID
    assert call(frames=tout - 1, pos=_pos(0), npos=1) == WUN_ERR_INVALID
    assert call(preds=C.c_void_p(0x1001)) == WUN_ERR_INVALID


def test_separate_track_argument_errors_without_a_device(lib, plan):
    _, p, tin, tout = plan

    def call(h=p.handle, params=_FAKE, track=_FAKE, n=5 * tout + 3, ws=_FAKE, outs=_FAKE, preds=_FAKE):
        return lib.wun_separate_track(h, params, track, n, ws, outs, preds, None)
    for kw in ({"h": None}, {"params": None}, {"track": None}, {"ws": None}, {"outs": None}, {"preds": None}):
        assert call(**kw) == WUN_ERR_INVALID, kw
    assert call(n=tout - 1) == WUN_ERR_INVALID                                    # the caller pads short tracks
    assert "n_frames" in lib.wun_last_error().decode()
    assert call(n=0) == WUN_ERR_INVALID
    assert call(ws=C.c_void_p(0x1008)) == WUN_ERR_INVALID
    assert call(track=C.c_void_p(0x1001)) == WUN_ERR_INVALID


class FakeSeparator(object):
    """Stand-in with the separator surface whose geometry depends on the desired length, as get_padding's does:
    output = desired rounded up to a multiple of 4, input = output + 2 * 128; estimate = centre crop * gain."""
    PAD = 128

    def __init__(self, cfg, floats_per_frame=10):
        self.cfg = cfg
        self.floats_per_frame = floats_per_frame
        self.batches = []
        self.queries = []

    def get_padding(self, shape):
        c = 1 if self.cfg["mono_downmix"] else 2
        t_out = -(-int(shape[1]) // 4) * 4
        return np.array([shape[0], t_out + 2 * self.PAD, c]), np.array([shape[0], t_out, c])

    def workspace_floats(self, batch, frames):
        self.queries.append((batch, frames))
        return batch * frames * self.floats_per_frame

    def get_output(self, batch, training):
        assert training is False
        self.batches.append(np.array(batch, copy=True))
        core = np.asarray(batch)[:, self.PAD:np.asarray(batch).shape[1] - self.PAD, :]
        return {n: core * (i + 1) + 0.01 * i for i, n in enumerate(self.cfg["source_names"])}


def test_hop_geometry_is_get_padding():
    cfg = wun.get_config("baseline", num_frames=300, context=True)
    sep = FakeSeparator(cfg)
    assert hop_geometry(cfg, sep, 4099) == (300 + 256, 300)
    assert hop_geometry(cfg, sep, 4099, 1201) == (1204 + 256, 1204)
    assert hop_geometry(cfg, sep, 4099, "track") == (4100 + 256, 4100)
    for bad in (0, -5, True):
        with pytest.raises(ValueError):
            hop_geometry(cfg, sep, 4099, bad)
    same = wun.get_config("baseline", num_frames=4096, num_layers=3)              # same padding: whole multiples of 2^L
    assert hop_geometry(same, sep, 4099, 1201) == (1208 + 256, 1208) and hop_geometry(same, sep, 4099) == (4096 + 256, 4096)
    # ... and of the real separator: the C entry the plans are created from
    real = UnetAudioSeparator(wun.get_config("m1_context"))
    i, o = real.get_padding(np.array([1, 10 * 16389, 0]))
    assert hop_geometry(real.model_config, real, 10 ** 6, 10 * 16389) == (int(i[1]), int(o[1]))
    assert int(i[1]) - int(o[1]) == 147443 - 16389                                # the context does not grow with the hop


@pytest.mark.parametrize("hop", [None, 300, 1201, "track"])
def test_separate_track_hop_frames_on_the_stand_in(hop):
    cfg = wun.get_config("baseline", num_frames=300, mono_downmix=False, context=True)
    n = 4099
    audio = np.random.default_rng(7).uniform(-1, 1, (n, 2)).astype(np.float32)
    sep = FakeSeparator(cfg)
    got = separate_track(cfg, sep, audio, cfg["expected_sr"], batch_hops=4, hop_frames=hop)
    t_in, t_out = hop_geometry(cfg, sep, n, hop)
    assert all(b.shape[1] == t_in for b in sep.batches)                           # the plan lengths are get_padding's
    n_frames = max(n, t_in if hop is None else t_out)
    hops = -(-n_frames // t_out)
    assert sum(b.shape[0] for b in sep.batches) == hops
    if hop == "track":
        assert hops == 1 and len(sep.batches) == 1 and sep.batches[0].shape == (1, 4100 + 256, 2)
    # the stand-in is a pure crop: every tiling gives the same estimates
    for i, name in enumerate(cfg["source_names"]):
        assert got[name].shape == (n, 2) and np.array_equal(got[name], audio * (i + 1) + np.float32(0.01 * i))
    if hop is None:
        want = predict_track(cfg, FakeSeparator(cfg), audio, cfg["expected_sr"], batch_hops=4)
        assert all(np.array_equal(got[k], want[k]) for k in want)


def test_short_track_and_long_hop_is_one_hop():
    cfg = wun.get_config("baseline", num_frames=300, context=True)
    audio = np.random.default_rng(8).uniform(-1, 1, (100, 1)).astype(np.float32)
    sep = FakeSeparator(cfg)
    got = separate_track(cfg, sep, audio, cfg["expected_sr"], hop_frames=1000)
    assert len(sep.batches) == 1 and sep.batches[0].shape == (1, 1000 + 256, 1)
    assert np.array_equal(got[cfg["source_names"][0]], audio)


def test_byte_budget_lowers_batch_hops():
    cfg = wun.get_config("baseline", num_frames=300, context=True)
    sep = FakeSeparator(cfg, floats_per_frame=10)
    t_def = 300 + 256
    t_long = 1200 + 256
    # default budget: the default tiling's workspace at batch_hops = 8 -> 8 * 556 * 40 bytes; a long hop takes 1456 * 40
    assert budget_batch_hops(sep, 8, 100, t_long, t_def) == (8 * t_def) // t_long == 3
    assert (8, t_def) in sep.queries and (1, t_long) in sep.queries               # both figures come from the plan query
    assert budget_batch_hops(sep, 8, 2, t_long, t_def) == 2                       # never more than the hops there are
    assert budget_batch_hops(sep, 8, 100, t_long, t_def, workspace_bytes=5 * t_long * 40) == 5
    assert budget_batch_hops(sep, 8, 100, t_long, t_def, workspace_bytes=10 ** 12) == 8
    assert budget_batch_hops(sep, 8, 100, t_long, t_def, workspace_bytes=1) == 1  # one hop cannot be split
    # through separate_track: 4099 frames in hops of 1200 = 4 hops; the budget of 2 long hops gives chunks of 2
    audio = np.random.default_rng(9).uniform(-1, 1, (4099, 1)).astype(np.float32)
    separate_track(cfg, sep, audio, cfg["expected_sr"], batch_hops=8, hop_frames=1200, workspace_bytes=2 * t_long * 40)
    assert [b.shape[0] for b in sep.batches] == [2, 2]
    sep.batches = []
    separate_track(cfg, sep, audio, cfg["expected_sr"], batch_hops=8, hop_frames=1200)
    assert [b.shape[0] for b in sep.batches] == [3, 1]
    sep.batches = []
    separate_track(cfg, sep, audio, cfg["expected_sr"], batch_hops=8)             # the default tiling is not budgeted
    assert [b.shape[0] for b in sep.batches] == [8, 6]


def test_cli_hop_frames_option_is_parsed():
    from wave_u_net_amd.__main__ import _parse
    _, _, _, opts = _parse(["predict", "with", "cfg.baseline", "input_path=/x.wav", "hop_frames=163890"])
    assert opts["hop_frames"] == 163890
    _, _, _, opts = _parse(["predict", "with", "cfg.baseline", "input_path=/x.wav", "hop_frames=track"])
    assert opts["hop_frames"] == "track"
    assert evaluate.produce_source_estimates.__code__.co_varnames[:6][-1] == "hop_frames"
