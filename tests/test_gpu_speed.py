"""GPU tests of speed perturbation in the fused batch producer (include/wun.h: wun_gather_snippets_speed;
datasets.FusedSnippetSource with augment["speed"]): unit rates against wun_gather_snippets bit for bit, rated sources against the
numpy oracle of tests/_speed_np.py and against wun_resample bit for bit, the footprint on both sides, the class on its own
descriptors and rates, and a tiny training run."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import wave_u_net_amd as wun                                              # noqa: E402
from wave_u_net_amd import _lib, datasets, resample, training, validation  # noqa: E402

import _snippets_np                                                       # noqa: E402
import _speed_np                                                          # noqa: E402
from _unaligned import _offset_full                                       # noqa: E402

DEV = "cuda:0"
ROWS = _lib.SNIPPET_ROWS
BANK = [(10, 9), (20, 21), (3, 2), (1, 2), (2, 1)]
_BANKS = {}


def _bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _bank(pairs=tuple(BANK)):
    """The wun_speed_bank of `pairs` with its tables on the device (kept alive here)."""
    if pairs not in _BANKS:
        tabs = [torch.from_numpy(resample.design(up, down)).to(DEV) for up, down in pairs]
        b = _lib.WunSpeedBank()
        b.n = len(pairs)
        for i, ((up, down), t) in enumerate(zip(pairs, tabs)):
            b.up[i], b.down[i], b.table[i] = up, down, t.data_ptr()
        _BANKS[pairs] = (b, tabs)
    return _BANKS[pairs][0]


def _planes(S, c, frames, seed):
    """S host planes [frames, c] and their device copies, plane s starting s floats into an allocation: every offset of a
    plane inside a 16-byte granule occurs."""
    rng = np.random.default_rng(seed)
    host = [rng.uniform(-1, 1, (frames, c)).astype(np.float32) for _ in range(S)]
    return host, [_to_dev(h, s % 4) for s, h in enumerate(host)]


def _to_dev(h, off):
    buf = torch.zeros(h.size + 4, dtype=torch.float32, device=DEV)
    v = buf[off:off + h.size].view(*h.shape)
    v.copy_(torch.from_numpy(h))
    return v


def _off(n, k, fill=float("nan")):
    """n floats at k floats past a 16-byte boundary, four guard floats before and behind: (the buffer, the view)."""
    if k == 1:
        g = _offset_full((n + 8,), fill)
        assert g.data_ptr() % 16 in (4, 12)
        return g, g[4:4 + n]
    buf = torch.full((n + 8 + 4,), fill, dtype=torch.float32, device=DEV)
    g = buf[k:k + n + 8]
    assert g.data_ptr() % 16 == 4 * k
    return g, g[4:4 + n]


def _span(t_in, rate, bank=BANK):
    return t_in if rate == 0 else _speed_np.source_frames(t_in, *bank[rate - 1])


def _table(B, S, c, t_in, frames, seed, n_rates=len(BANK), unit_gain=False):
    """A seeded table and its rates: every rate index (0 included), first and last legal starts, all residues mod 4, gains with
    some equal to 1, every flag combination."""
    rng = np.random.default_rng(seed)
    t = np.zeros((B, S), dtype=datasets.SNIPPET_DTYPE)
    rates = np.zeros((B, S), dtype=np.uint8)
    k = 0
    for b in range(B):
        for s in range(S):
            rates[b, s] = (k + seed) % (n_rates + 1)
            last = frames - _span(t_in, int(rates[b, s]))
            t["start"][b, s] = (0, last, 1, last - 1, 2, last - 2, 3, last - 3)[k] if k < 8 else rng.integers(0, last + 1)
            t["flags"][b, s] = (k % 4) if c == 2 else 2 * (k % 2)
            t["gain"][b, s] = 1.0 if (unit_gain or k % 3 == 0) else np.float32(rng.uniform(0.7, 1.0))
            k += 1
    return t, rates


def _plain(dev, dev_mix, frames, table, mode, t_in, t_out):
    B, S = table.shape
    c = int(dev[0].shape[1])
    mix = torch.full((B, t_in, c), float("nan"), device=DEV)
    tgt = torch.full((S, B, t_out, c), float("nan"), device=DEV)
    arr = (C.c_void_p * S)(*[p.data_ptr() for p in dev])
    table = np.ascontiguousarray(table)
    _lib.check(_lib.load().wun_gather_snippets(arr, dev_mix.data_ptr() if dev_mix is not None else None, frames, c, S, B, t_in,
                                               t_out, table.ctypes.data, mode, mix.data_ptr(), tgt.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream))
    return mix, tgt


def _speed(dev, dev_mix, frames, table, rates, bank, mode, t_in, t_out, mix=None, tgt=None):
    B, S = table.shape
    c = int(dev[0].shape[1])
    if mix is None:
        mix = torch.full((B, t_in, c), float("nan"), device=DEV)
    if tgt is None:
        tgt = torch.full((S, B, t_out, c), float("nan"), device=DEV)
    arr = (C.c_void_p * S)(*[p.data_ptr() for p in dev])
    table = np.ascontiguousarray(table)
    rates = None if rates is None else np.ascontiguousarray(rates, dtype=np.uint8)
    _lib.check(_lib.load().wun_gather_snippets_speed(
        arr, dev_mix.data_ptr() if dev_mix is not None else None, frames, c, S, B, t_in, t_out, table.ctypes.data,
        None if rates is None else rates.ctypes.data, None if bank is None else C.addressof(bank), mode, mix.data_ptr(),
        tgt.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return mix, tgt


# ---------------------------------------------------------------------------------------- unit rates
@pytest.mark.parametrize("t_in,t_out", [(90, 40), (93, 41), (64, 64)])
@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("c", [1, 2])
def test_unit_rates_are_the_plain_gather_bit_for_bit(c, S, t_in, t_out):
    frames = 301
    host, dev = _planes(S + 1, c, frames, seed=10 * S + c)
    dev, dev_mix = dev[:S], dev[S]
    for B in (1, ROWS + 1):
        table, _ = _table(B, S, c, t_in, frames, seed=B, n_rates=0)
        zeros = np.zeros((B, S), np.uint8)
        for mode in (0, 1):
            want_mix, want_tgt = _plain(dev, dev_mix, frames, table, mode, t_in, t_out)
            for rates, bank in ((None, None), (zeros, None), (zeros, _bank()), (None, _bank())):
                mix, tgt = _speed(dev, dev_mix, frames, table, rates, bank, mode, t_in, t_out)
                assert np.array_equal(_bits(mix), _bits(want_mix)) and np.array_equal(_bits(tgt), _bits(want_tgt)), (B, mode)


def test_unit_gain_unit_rate_passes_the_bits_through():
    special = np.array([0x80000000, 0x00000001, 0x80012345, 0x7FC12345, 0xFFC00001, 0x7F812345, 0x007FFFFF, 0x3F800000],
                       dtype=np.uint32).view(np.float32)       # -0, denormals, quiet / signalling NaNs with payloads
    frames = 301
    for c in (1, 2):
        host = np.resize(special, frames * c).reshape(frames, c).copy()
        host[::7] = np.float32(0.25)
        dev = torch.from_numpy(host).to(DEV)
        other = torch.from_numpy(np.random.default_rng(c).uniform(-1, 1, (frames, c)).astype(np.float32)).to(DEV)
        table = np.zeros((3, 2), dtype=datasets.SNIPPET_DTYPE)
        table["start"][:, 0], table["gain"] = [0, 3, frames - 90], 1.0
        # all unit (the plain kernel), then beside a rated source (the unit path of the resampling kernel)
        for rates in (np.zeros((3, 2), np.uint8), np.array([[0, 1], [0, 2], [0, 3]], np.uint8)):
            mix, tgt = _speed([dev, other], None, frames, table, rates, _bank(), 1, 90, 40)
            for b, start in enumerate(table["start"][:, 0]):
                assert np.array_equal(_bits(tgt[0, b]), _bits(host[start + 25:start + 65])), (c, b)
        mix, _ = _speed([dev], None, frames, table[:, :1], np.zeros((3, 1), np.uint8), _bank(), 1, 90, 40)
        for b, start in enumerate(table["start"][:, 0]):
            assert np.array_equal(_bits(mix[b]), _bits(host[start:start + 90])), (c, b)


# ---------------------------------------------------------------------------------------- rated sources
FRAMES = 6000


@pytest.mark.parametrize("t_in,t_out", [(93, 41), (2500, 1100)])          # 2500 x 2 floats: four workgroup tiles and their edges
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("c", [1, 2])
def test_rated_sources_are_the_oracle_bit_for_bit(c, S, t_in, t_out):
    B = 5
    host, dev = _planes(S, c, FRAMES, seed=100 * S + c)
    table, rates = _table(B, S, c, t_in, FRAMES, seed=S + c + t_in)
    assert (S == 1 or set(rates.ravel().tolist()) == set(range(len(BANK) + 1))) and (table["gain"] == 1.0).any()
    want_mix, want_tgt = _speed_np.gather(host, table, rates, BANK, t_in, t_out)
    assert np.isfinite(want_mix).all()
    for k in (1, 2, 3):                                                  # outputs 1 to 3 floats off a 16-byte boundary
        n_mix, n_tgt = B * t_in * c, S * B * t_out * c
        gm, vm = _off(n_mix, k)
        gt, vt = _off(n_tgt, 4 - k)
        mix, tgt = vm.view(B, t_in, c), vt.view(S, B, t_out, c)
        _speed(dev, None, FRAMES, table, rates, _bank(), 1, t_in, t_out, mix, tgt)
        bad = np.argwhere(_bits(mix) != _bits(want_mix))
        assert bad.size == 0, (k, len(bad), bad[:4].tolist())
        assert np.array_equal(_bits(tgt), _bits(want_tgt)), k
        for g, n in ((gm, n_mix), (gt, n_tgt)):
            assert torch.isnan(g[:4]).all() and torch.isnan(g[4 + n:]).all()      # the guards are intact


@pytest.mark.parametrize("c", [1, 2])
def test_one_rated_source_is_wun_resample_bit_for_bit(c):
    t_in = 2500
    host, dev = _planes(1, c, FRAMES, seed=5 + c)
    for i, (up, down) in enumerate(BANK):
        n_src = _speed_np.source_frames(t_in, up, down)
        table = np.zeros((2, 1), dtype=datasets.SNIPPET_DTYPE)
        table["start"][:, 0], table["gain"] = [7, FRAMES - n_src], 1.0
        mix, tgt = _speed(dev, None, FRAMES, table, np.full((2, 1), i + 1, np.uint8), _bank(), 1, t_in, t_in)
        for b, start in enumerate(table["start"][:, 0]):
            y = torch.full((t_in, c), float("nan"), device=DEV)
            resample.resample_into(dev[0][start:start + n_src].contiguous(), y, 0, t_in, up, down)
            assert np.array_equal(_bits(mix[b]), _bits(y)) and np.array_equal(_bits(tgt[0, b]), _bits(y)), (up, down, b)


@pytest.mark.parametrize("c", [1, 2])
def test_footprint_nothing_outside_the_spans_is_read(c):
    S, B, t_in, t_out = 3, 5, 93, 41
    host, dev = _planes(S, c, FRAMES, seed=31 + c)
    table, rates = _table(B, S, c, t_in, FRAMES, seed=9)
    clean_mix, clean_tgt = _speed(dev, None, FRAMES, table, rates, _bank(), 1, t_in, t_out)
    assert torch.isfinite(clean_mix).all() and torch.isfinite(clean_tgt).all()
    for b in range(B):                                                   # row b alone, NaN over every plane outside ITS spans
        poisoned = []
        for s in range(S):
            h = np.full_like(host[s], np.nan)
            lo = int(table["start"][b, s])
            hi = lo + _span(t_in, int(rates[b, s]))
            h[lo:hi] = host[s][lo:hi]
            poisoned.append(_to_dev(h, (s + 1) % 4))
        mix, tgt = _speed(poisoned, None, FRAMES, table[b:b + 1], rates[b:b + 1], _bank(), 1, t_in, t_out)
        assert torch.isfinite(mix).all() and torch.isfinite(tgt).all(), b
        assert np.array_equal(_bits(mix[0]), _bits(clean_mix[b])) and np.array_equal(_bits(tgt[:, 0]), _bits(clean_tgt[:, b])), b


@pytest.mark.parametrize("c", [1, 2])
def test_a_batch_of_more_rows_than_a_launch_carries(c):
    S, B, t_in, t_out = 2, ROWS + 1, 93, 41
    host, dev = _planes(S, c, 700, seed=77 + c)
    rng = np.random.default_rng(3)
    table = np.zeros((B, S), dtype=datasets.SNIPPET_DTYPE)
    rates = rng.integers(0, 4, (B, S)).astype(np.uint8)                  # (10, 9), (20, 21), (3, 2) and the unit rate
    rates[-1] = (2, 0)                                                   # the second launch: one rated, one unit source
    for b in range(B):
        for s in range(S):
            table["start"][b, s] = rng.integers(0, 700 - _span(t_in, int(rates[b, s])) + 1)
    table["gain"] = rng.uniform(0.7, 1.0, (B, S)).astype(np.float32)
    table["flags"] = rng.integers(0, 4, (B, S)) & (3 if c == 2 else 2)
    want_mix, want_tgt = _speed_np.gather(host, table, rates, BANK, t_in, t_out)
    gm, vm = _off(B * t_in * c, 1)
    gt, vt = _off(S * B * t_out * c, 1)
    mix, tgt = vm.view(B, t_in, c), vt.view(S, B, t_out, c)
    _speed(dev, None, 700, table, rates, _bank(), 1, t_in, t_out, mix, tgt)
    assert np.array_equal(_bits(mix), _bits(want_mix)) and np.array_equal(_bits(tgt), _bits(want_tgt))
    for g, n in ((gm, mix.numel()), (gt, tgt.numel())):
        assert torch.isnan(g[:4]).all() and torch.isnan(g[4 + n:]).all()


# ---------------------------------------------------------------------------------------- the class
T_IN, T_OUT = 90, 40


def _cfg(name, **kw):
    base = dict(batch_size=4, num_snippets_per_track=3, cache_size=5)
    base.update(kw)
    return wun.get_config(name, **base)


def _tracks(cfg, lengths, seed):
    rng = np.random.default_rng(seed)
    c = 1 if cfg["mono_downmix"] else 2
    return [datasets.make_track({k: rng.uniform(-0.4, 0.4, (n, c)).astype(np.float32) for k in cfg["source_names"]}, cfg)
            for n in lengths]


@pytest.mark.parametrize("name", ["baseline", "full_multi_instrument"])
def test_fused_source_with_speed_delivers_the_oracles_batch(name):
    cfg = _cfg(name)
    names = list(cfg["source_names"])
    tracks = _tracks(cfg, [400, 257, 333], seed=12)
    padded = [datasets.pad_track(t, (T_IN - T_OUT) // 2) for t in tracks]
    planes = [np.concatenate([p[k] for p in padded]) for k in names]
    mix_plane = np.concatenate([p["mix"] for p in padded])
    fused = datasets.FusedSnippetSource(cfg, tracks, T_IN, T_OUT, 4, DEV, seed=3, augment={"speed": 1.0, "remix": 0.5})
    assert fused.speed_rates == datasets.SPEED_RATES_DEFAULT and fused.mix_mode == 1
    used, mixed = set(), 0
    for _ in range(6):
        table, rates = fused.descriptors().copy(), fused.rates().copy()
        assert table.shape == rates.shape == (4, len(names)) and rates.dtype == np.uint8 and rates.all()
        assert fused.rates() is fused.rates() and fused.descriptors() is fused.descriptors()     # peeking does not advance
        mix, targets = fused()
        want_mix, want_tgt = _speed_np.gather(planes, table, rates, fused.speed_rates, T_IN, T_OUT)
        assert np.array_equal(_bits(mix), _bits(want_mix)) and np.array_equal(_bits(targets), _bits(want_tgt))
        used |= set(rates.ravel().tolist())
        mixed += int((rates != rates[:, :1]).any())
    assert used == {1, 2, 3, 4} and (len(names) == 1 or mixed >= 1)
    # without speed the batches are what they were: the plain oracle on the plain stream, rates all zero
    for augment in ({"remix": 0.5, "polarity": 0.5}, {"remix": 0.5, "polarity": 0.5, "speed": 0}, None):
        fused = datasets.FusedSnippetSource(cfg, tracks, T_IN, T_OUT, 4, DEV, seed=3, augment=augment)
        stream = datasets.augmented_descriptors(cfg, [p["mix"].shape[0] for p in padded], T_IN, T_OUT, np.random.default_rng(3),
                                                augment if augment is None else {k: v for k, v in augment.items() if k != "speed"},
                                                np.random.default_rng([3, 1]))
        for _ in range(3):
            rows = [next(stream) for _ in range(4)]
            table = fused.descriptors().copy()
            assert np.array_equal(table, np.stack([r for r, _ in rows])) and not fused.rates().any() and fused._bank is None
            mix, targets = fused()
            want_mix, want_tgt, _ = _snippets_np.gather(planes, mix_plane, table, fused.mix_mode, T_IN, T_OUT)
            assert np.array_equal(_bits(mix), _bits(want_mix)) and np.array_equal(_bits(targets), _bits(want_tgt))


def test_training_with_the_fused_producer_and_speed(tmp_path, monkeypatch):
    monkeypatch.setenv("WUN_NO_TUNE", "1")
    tmp = str(tmp_path)
    cfg = wun.get_config("baseline_stereo", num_layers=3, num_initial_filters=8, num_frames=40, batch_size=4, epoch_it=3,
                         worse_epochs=1, num_snippets_per_track=6, cache_size=8, model_base_dir=os.path.join(tmp, "ckpt"),
                         log_dir=os.path.join(tmp, "logs"), init_sup_sep_lr=1e-3, data_producer="fused",
                         augment={"speed": 1.0, "remix": 0.5})
    tracks = _tracks(cfg, [700, 800, 650], seed=1)
    make, made = validation._train_source(cfg, tracks, seed=5), []

    def source(trainer):                                                 # the deferred constructor, watched
        made.append(make(trainer))
        rated.append(int(made[0].rates().any()))
        return made[0]
    source.needs_trainer = True
    rated = []
    path = training.train(cfg, "speed", batch_source=source)
    assert isinstance(made[0], datasets.FusedSnippetSource) and made[0].speed_rates == datasets.SPEED_RATES_DEFAULT and rated == [1]
    losses = [json.loads(l)["sep_loss"] for l in open(os.path.join(cfg["log_dir"], "speed", "train.jsonl"))]
    assert len(losses) == 3 and np.isfinite(losses).all()
    arrays = dict(np.load(path))
    init = wun.UnetAudioSeparator(cfg)
    start = {n: v.detach().cpu().numpy() for n, v in init.variables().items()}
    changed = [n for n in start if n in arrays and not np.array_equal(start[n], arrays[n])]
    assert changed and all(np.isfinite(arrays[n]).all() for n in start if n in arrays)
