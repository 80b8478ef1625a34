"""CPU-only checks of the fused batch producer (datasets.augmented_descriptors, datasets.FusedSnippetSource, include/wun.h:
wun_gather_snippets): the descriptor stream against snippet_descriptors, the order and the source of the augmentation draws,
every ValueError, the struct's size, every argument error of the entry before any GPU work (no device here), and the numpy
oracle of tests/_snippets_np.py against the reference pipeline."""
import ctypes as C

import numpy as np
import pytest

import wave_u_net_amd as wun
from wave_u_net_amd import _lib, datasets, validation

import _snippets_np

WUN_ERR_INVALID = -1
_FAKE = C.c_void_p(0x1000)          # non-null, 16-byte aligned, never dereferenced: every call below fails a check first
T_IN, T_OUT = 90, 40


def _cfg(name="full_multi_instrument", **kw):
    base = dict(batch_size=4, num_snippets_per_track=3, cache_size=5)
    base.update(kw)
    return wun.get_config(name, **base)


def _tracks(cfg, lengths, seed=0):
    rng = np.random.default_rng(seed)
    c = 1 if cfg["mono_downmix"] else 2
    return [datasets.make_track({k: rng.uniform(-0.4, 0.4, (n, c)).astype(np.float32) for k in cfg["source_names"]}, cfg)
            for n in lengths]


LENGTHS = [400, 257, 333]            # padded track lengths of a 3-track set
OFFSETS = [0, 400, 657]


def test_without_augment_the_base_stream_is_replayed():
    for aug_flag in (True, False):
        cfg = _cfg(augmentation=aug_flag)
        S = len(cfg["source_names"])
        base = datasets.snippet_descriptors(cfg, LENGTHS, T_IN, T_OUT, "train", np.random.default_rng(21))
        for augment in (None, {}, {"remix": 0, "polarity": 0.0}):
            got = datasets.augmented_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(21), augment)
            base = datasets.snippet_descriptors(cfg, LENGTHS, T_IN, T_OUT, "train", np.random.default_rng(21))
            for _ in range(31):                                     # 9 snippets per pass: more than three passes
                ti, pos, gains = next(base)
                rec, mix_mode = next(got)
                assert rec.dtype == datasets.SNIPPET_DTYPE and rec.shape == (S,)
                assert (rec["start"] == OFFSETS[ti] + pos).all() and (rec["flags"] == 0).all()
                if aug_flag:
                    assert mix_mode == 1 and np.array_equal(rec["gain"], gains) and gains.dtype == np.float32
                else:
                    assert mix_mode == 0 and gains is None and (rec["gain"] == 1.0).all()


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


def test_draw_order_and_the_records_the_draws_give():
    cfg = _cfg()
    S = len(cfg["source_names"])
    augment = {"remix": 0.5, "channel_swap": 0.25, "polarity": 0.75}
    rec_rng = _RecordingAug(5)
    got = datasets.augmented_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(21), augment, rec_rng)
    base = datasets.snippet_descriptors(cfg, LENGTHS, T_IN, T_OUT, "train", np.random.default_rng(21))
    taken = 0
    for _ in range(40):
        k0 = len(rec_rng.log)
        rec, mix_mode = next(got)
        ti, pos, gains = next(base)                                 # the base stream is untouched by the draws
        log = rec_rng.log[k0:]
        assert mix_mode == 1 and np.array_equal(rec["gain"], gains)
        want_start = [OFFSETS[ti] + pos] * S
        assert log[0][0] == "u"
        k = 1
        if log[0][1] < 0.5:                                         # 1. remix; 2. (track, start) per source >= 1
            taken += 1
            for s in range(1, S):
                assert log[k][:3] == ("i", 0, 3)
                tj = log[k][3]
                assert log[k + 1][:3] == ("i", 0, LENGTHS[tj] - T_IN)
                want_start[s] = OFFSETS[tj] + log[k + 1][3]
                k += 2
        swap = [e[1] < 0.25 for e in log[k:k + S]]                  # 3. one uniform per source: swap
        neg = [e[1] < 0.75 for e in log[k + S:k + 2 * S]]           # 4. one uniform per source: polarity
        assert len(log) == k + 2 * S and all(e[0] == "u" for e in log[k:])
        assert list(rec["start"]) == want_start
        assert list(rec["flags"]) == [int(a) * 1 + int(b) * 2 for a, b in zip(swap, neg)]
    assert 5 < taken < 35
    # keys at probability 0 (or absent) draw nothing
    rec_rng = _RecordingAug(5)
    got = datasets.augmented_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(21), {"polarity": 1, "remix": 0}, rec_rng)
    rec, _ = next(got)
    assert len(rec_rng.log) == S and (rec["flags"] == 2).all()


def test_aug_rng_never_advances_rng_and_has_a_default():
    cfg = _cfg()
    plain = datasets.augmented_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(3))
    aug = datasets.augmented_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(3), {"remix": 1, "polarity": 0.5})
    again = datasets.augmented_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(3), {"remix": 1, "polarity": 0.5},
                                           np.random.default_rng([1337, 1]))
    changed = 0
    for _ in range(25):
        p, _ = next(plain)
        a, mode = next(aug)
        b, _ = next(again)
        assert np.array_equal(a, b)                                 # the default second Generator
        assert a["start"][0] == p["start"][0] and np.array_equal(a["gain"], p["gain"]) and mode == 1
        changed += int((a["start"][1:] != p["start"][1:]).any())
    assert changed > 20


def test_remix_gives_every_later_source_its_own_position_in_range():
    cfg = _cfg(augmentation=False)
    got = datasets.augmented_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(8), {"remix": 1})
    ends = np.cumsum(LENGTHS)
    tracks_seen, distinct = set(), 0
    for _ in range(60):
        rec, mode = next(got)
        assert mode == 1 and (rec["gain"] == 1.0).all() and (rec["flags"] == 0).all()
        for s in range(len(rec)):
            ti = int(np.searchsorted(ends, rec["start"][s], side="right"))
            assert 0 <= rec["start"][s] - OFFSETS[ti] < LENGTHS[ti] - T_IN      # the window stays inside ONE track
            if s:
                tracks_seen.add(ti)
        distinct += int(len(set(rec["start"].tolist())) > 1)
    assert tracks_seen == {0, 1, 2} and distinct >= 58


def test_value_errors():
    cfg = _cfg()
    mono = _cfg("baseline")
    assert mono["mono_downmix"] and not cfg["mono_downmix"]

    def first(c, augment):
        return next(datasets.augmented_descriptors(c, LENGTHS, T_IN, T_OUT, np.random.default_rng(1), augment))
    for bad in ({"pitch": 0.5}, {"remix": 1.5}, {"remix": -0.1}, {"polarity": float("nan")}, {"channel_swap": "often"},
                {"remix": None}, ["remix"]):
        with pytest.raises(ValueError):
            first(cfg, bad)
    with pytest.raises(ValueError):
        first(mono, {"channel_swap": 0.5})
    first(mono, {"channel_swap": 0, "polarity": 0.5})               # probability 0: not active, no complaint
    # the producer selection (validation.data_producer): both keys stay out of the default configs
    assert "data_producer" not in cfg and "augment" not in cfg
    assert validation.data_producer(cfg) == "torch" and validation.data_producer(dict(cfg, data_producer="fused")) == "fused"
    for bad in (dict(cfg, data_producer="tf"), dict(cfg, augment={"remix": 0.5}),
                dict(cfg, data_producer="torch", augment={"remix": 0.5}), dict(cfg, data_producer="fused", augment={"x": 1}),
                dict(mono, data_producer="fused", augment={"channel_swap": 1})):
        with pytest.raises(ValueError):
            validation.data_producer(bad)
        with pytest.raises(ValueError):
            validation._train_source(bad, [], seed=1)


def test_fused_source_refuses_a_device_without_kernels():
    cfg = _cfg()
    with pytest.raises(RuntimeError):
        datasets.FusedSnippetSource(cfg, _tracks(cfg, [400, 300]), T_IN, T_OUT, 4, "cpu")
    with pytest.raises(ValueError):
        datasets.FusedSnippetSource(cfg, _tracks(cfg, [400, 300]), T_IN, T_OUT, 4, "cpu", augment={"remix": 2})
    with pytest.raises(ValueError):
        datasets.FusedSnippetSource(cfg, _tracks(cfg, [400, 300]), T_IN, T_OUT, 4, "cpu", augment={"remix": 1}, partition="valid")


def test_cli_overrides_carry_both_keys():
    from wave_u_net_amd.__main__ import _parse
    _, name, overrides, _ = _parse(["train", "with", "cfg.baseline_stereo", "model_config.data_producer=fused",
                                    'model_config.augment={"remix":0.5,"polarity":0.5}', "data_root=/x"])
    cfg = wun.get_config(name, **overrides)
    assert validation.data_producer(cfg) == "fused" and cfg["augment"] == {"remix": 0.5, "polarity": 0.5}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_struct_size_and_binding(lib):
    assert lib.wun_snippet_abi_size() == 16 == C.sizeof(_lib.WunSnippetSource) == datasets.SNIPPET_DTYPE.itemsize
    for f, (off, size) in {"start": (0, 8), "gain": (8, 4), "flags": (12, 4)}.items():
        fld = getattr(_lib.WunSnippetSource, f)
        assert (fld.offset, fld.size) == (off, size) == (datasets.SNIPPET_DTYPE.fields[f][1], datasets.SNIPPET_DTYPE[f].itemsize)
    assert 128 + _lib.SNIPPET_ROWS * 8 * 16 <= 4096  # the argument block for S = 8 under HIP's 4 KB
    assert len(lib.wun_gather_snippets.argtypes) == 13


def test_gather_argument_errors_without_a_device(lib):
    frames, S, B = 1000, 2, 3

    def table(rows=B, srcs=S, start=0, gain=1.0, flags=0):
        t = np.zeros((rows, srcs), dtype=datasets.SNIPPET_DTYPE)
        t["start"], t["gain"], t["flags"] = start, gain, flags
        return t

    def call(planes=(0x1000, 0x2000), mix_plane=_FAKE, frames=frames, c=2, s=S, b=B, tin=T_IN, tout=T_OUT, desc=None,
             mode=1, mix=_FAKE, tgt=_FAKE, null_planes=False, null_desc=False):
        desc = table() if desc is None else desc
        arr = (C.c_void_p * 8)(*planes)
        return lib.wun_gather_snippets(None if null_planes else arr, mix_plane, frames, c, s, b, tin, tout,
                                       None if null_desc else desc.ctypes.data, mode, mix, tgt, None)
    for kw in ({"null_planes": True}, {"null_desc": True}, {"mix": None}, {"tgt": None}, {"planes": (0x1000, 0)},
               {"mix_plane": None, "mode": 0}):
        assert call(**kw) == WUN_ERR_INVALID, kw
        assert "null" in lib.wun_last_error().decode()
    for kw in ({"mode": 2}, {"mode": -1}, {"c": 0}, {"c": 3}, {"s": 0}, {"s": 9}, {"b": 0}, {"b": -2},
               {"tout": T_IN + 2}, {"tout": T_OUT + 1}, {"tout": 0}, {"tout": -2},
               {"frames": T_IN - 1}, {"frames": -1},
               {"mix": C.c_void_p(0x1002)}, {"tgt": C.c_void_p(0x1001)}, {"planes": (0x1000, 0x2002)},
               {"mix_plane": C.c_void_p(0x1003)}):
        assert call(**kw) == WUN_ERR_INVALID, kw
    assert call(c=1, desc=table(flags=1)) == WUN_ERR_INVALID                      # the swap needs two channels
    assert "swap" in lib.wun_last_error().decode()
    for flags in (4, 8, 0x80000000, 7):
        assert call(desc=table(flags=flags)) == WUN_ERR_INVALID
        assert "flag" in lib.wun_last_error().decode()
    for r, s, start in ((0, 0, -1), (2, 1, frames - T_IN + 1), (1, 0, 1 << 50)):
        t = table()
        t["start"][r, s] = start
        assert call(desc=t) == WUN_ERR_INVALID
        assert "outside" in lib.wun_last_error().decode()
    t = table(rows=_lib.SNIPPET_ROWS + 1)                                         # a row of the SECOND launch: still before any GPU work
    t["start"][-1, 1] = frames
    assert call(b=_lib.SNIPPET_ROWS + 1, desc=t) == WUN_ERR_INVALID


@pytest.mark.parametrize("name", ["baseline", "full_multi_instrument"])
@pytest.mark.parametrize("aug_flag", [True, False])
def test_oracle_on_the_base_stream_is_get_dataset(name, aug_flag):
    cfg = _cfg(name, augmentation=aug_flag)
    names = list(cfg["source_names"])
    c = 1 if cfg["mono_downmix"] else 2
    tracks = _tracks(cfg, [400 - 50, 257 - 50, 333 - 50], seed=6)                 # padded by (90 - 40) / 2 on both sides: LENGTHS
    padded = [datasets.pad_track(t, (T_IN - T_OUT) // 2) for t in tracks]
    assert [p["mix"].shape[0] for p in padded] == LENGTHS
    planes = [np.concatenate([p[k] for p in padded]) for k in names]
    mix_plane = np.concatenate([p["mix"] for p in padded])
    host = datasets.get_dataset(cfg, [4, T_IN, c], [4, T_OUT, c], "train", tracks, seed=21)
    stream = datasets.augmented_descriptors(cfg, LENGTHS, T_IN, T_OUT, np.random.default_rng(21))
    for _ in range(6):
        rows = [next(stream) for _ in range(4)]
        modes = {m for _, m in rows}
        assert modes == {int(aug_flag)}
        mix, targets, _ = _snippets_np.gather(planes, mix_plane, np.stack([r for r, _ in rows]), modes.pop(), T_IN, T_OUT)
        hb = next(host)
        assert mix.dtype == np.float32 and np.array_equal(mix, hb["mix"])
        for si, k in enumerate(names):
            assert np.array_equal(targets[si], hb[k]), k
