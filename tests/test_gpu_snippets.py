"""GPU tests of the fused batch producer (include/wun.h: wun_gather_snippets; datasets.FusedSnippetSource): the operator against
the numpy oracle of tests/_snippets_np.py bit for bit, bit pass-through, footprint and independence, the class against the
reference pipeline (get_dataset), DeviceSnippetSource and the oracle, and training / validation end to end on a tiny config."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import wave_u_net_amd as wun                                   # noqa: E402
from wave_u_net_amd import _lib, datasets, training, validation  # noqa: E402

import _snippets_np                                            # noqa: E402
from _unaligned import _offset_full                            # noqa: E402

DEV = "cuda:0"
ROWS = _lib.SNIPPET_ROWS
FRAMES = 301                                                   # frames of a test plane


def _bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _planes(S, c, seed):
    """S host planes [FRAMES, c] and their device copies, plane s starting s floats into an allocation: every offset of a plane
    inside a 16-byte granule occurs."""
    rng = np.random.default_rng(seed)
    host = [rng.uniform(-1, 1, (FRAMES, c)).astype(np.float32) for _ in range(S + 1)]
    dev = []
    for s, h in enumerate(host):
        buf = torch.zeros(FRAMES * c + 4, dtype=torch.float32, device=DEV)
        v = buf[s % 4:s % 4 + FRAMES * c].view(FRAMES, c)
        v.copy_(torch.from_numpy(h))
        dev.append(v)
    return host[:S], host[S], dev[:S], dev[S]


def _table(B, S, c, t_in, unit_gain, seed):
    """Starts at all four residues mod 4, 0 and the last legal frame included; every flag combination; the gains."""
    rng = np.random.default_rng(seed)
    last = FRAMES - t_in
    fixed = [0, last, 1, 2, 3, last - 1, last - 2, last - 3, 4, 5, 6, 7]
    t = np.zeros((B, S), dtype=datasets.SNIPPET_DTYPE)
    k = 0
    for b in range(B):
        for s in range(S):
            t["start"][b, s] = fixed[k] if k < len(fixed) else rng.integers(0, last + 1)
            t["flags"][b, s] = (k % 4) if c == 2 else 2 * (k % 2)
            k += 1
    t["gain"] = 1.0 if unit_gain else rng.uniform(0.7, 1.0, (B, S)).astype(np.float32)
    assert B == 1 or ({int(v) % 4 for v in t["start"].ravel()} == {0, 1, 2, 3} and {0, last} <= set(t["start"].ravel().tolist()))
    return t


def _gather(dev_planes, dev_mix, table, mode, t_in, t_out, mix=None, tgt=None, stream=None):
    lib = _lib.load()
    B, S = table.shape
    c = int(dev_planes[0].shape[1])
    if mix is None:
        mix = torch.full((B, t_in, c), float("nan"), device=DEV)
    if tgt is None:
        tgt = torch.full((S, B, t_out, c), float("nan"), device=DEV)
    arr = (C.c_void_p * S)(*[p.data_ptr() for p in dev_planes])
    table = np.ascontiguousarray(table)
    st = stream if stream is not None else torch.cuda.current_stream()
    _lib.check(lib.wun_gather_snippets(arr, dev_mix.data_ptr() if dev_mix is not None else None, FRAMES, c, S, B, t_in, t_out,
                                       table.ctypes.data, mode, mix.data_ptr(), tgt.data_ptr(), st.cuda_stream))
    return mix, tgt


@pytest.mark.parametrize("t_in,t_out", [(90, 40), (93, 41), (64, 64)])      # odd pad; no multiple of 4; no crop
@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("c", [1, 2])
def test_operator_is_the_oracle_bit_for_bit(c, S, t_in, t_out):
    host, host_mix, dev, dev_mix = _planes(S, c, seed=10 * S + c)
    for B in (1, ROWS + 1):                                    # one row; one row more than a launch carries
        for mode in (0, 1):
            for unit_gain in (True, False):
                table = _table(B, S, c, t_in, unit_gain, seed=B + mode)
                mix, tgt = _gather(dev, dev_mix, table, mode, t_in, t_out)
                want_mix, want_tgt, _ = _snippets_np.gather(host, host_mix, table, mode, t_in, t_out)
                what = (B, mode, unit_gain)
                assert np.array_equal(_bits(mix), _bits(want_mix)), what
                assert np.array_equal(_bits(tgt), _bits(want_tgt)), what


def test_unit_gain_passes_the_bits_through():
    special = np.array([0x80000000, 0x00000001, 0x80012345, 0x7FC12345, 0xFFC00001, 0x7F812345, 0x007FFFFF, 0x3F800000],
                       dtype=np.uint32).view(np.float32)       # -0, denormals, quiet / signalling NaNs with payloads
    for c in (1, 2):
        host = np.resize(special, FRAMES * c).reshape(FRAMES, c).copy()
        host[::7] = np.float32(0.25)
        dev = torch.from_numpy(host).to(DEV)
        table = np.zeros((3, 1), dtype=datasets.SNIPPET_DTYPE)
        table["start"][:, 0], table["gain"] = [0, 3, FRAMES - 90], 1.0
        for mode, mix_plane in ((1, None), (0, dev)):
            mix, tgt = _gather([dev], mix_plane, table, mode, 90, 40)
            for b, start in enumerate(table["start"][:, 0]):
                assert np.array_equal(_bits(mix[b]), _bits(host[start:start + 90])), (c, mode, b)
                assert np.array_equal(_bits(tgt[0, b]), _bits(host[start + 25:start + 65])), (c, mode, b)


@pytest.mark.parametrize("c", [1, 2])
def test_footprint_and_independence(c):
    S, t_in, t_out, B = 3, 93, 41, ROWS + 1
    host, host_mix, dev, dev_mix = _planes(S, c, seed=77)
    table = _table(B, S, c, t_in, False, seed=4)
    for mode in (0, 1):
        want_mix, want_tgt, _ = _snippets_np.gather(host, host_mix, table, mode, t_in, t_out)
        ref = None
        side = torch.cuda.Stream()
        for fill, stream in ((float("nan"), None), (7.0, None), (float("nan"), side), (float("nan"), None)):
            n_mix, n_tgt = B * t_in * c, S * B * t_out * c
            # one float off 16-byte alignment, four guard floats before and behind
            gm, gt = _offset_full((n_mix + 8,), float("nan")), _offset_full((n_tgt + 8,), float("nan"))
            mix, tgt = gm[4:4 + n_mix].view(B, t_in, c), gt[4:4 + n_tgt].view(S, B, t_out, c)
            assert mix.data_ptr() % 16 == 4 and tgt.data_ptr() % 16 == 4
            mix.fill_(fill)
            tgt.fill_(fill)
            if stream is not None:
                stream.wait_stream(torch.cuda.current_stream())
            _gather(dev, dev_mix, table, mode, t_in, t_out, mix, tgt, stream)
            if stream is not None:
                torch.cuda.current_stream().wait_stream(stream)
            for g, n in ((gm, n_mix), (gt, n_tgt)):
                assert torch.isnan(g[:4]).all() and torch.isnan(g[4 + n:]).all()          # the guards are intact
            assert np.array_equal(_bits(mix), _bits(want_mix)) and np.array_equal(_bits(tgt), _bits(want_tgt)), (mode, fill)
            got = (_bits(mix).copy(), _bits(tgt).copy())
            if ref is not None:
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
            ref = got


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


def _same_batch(mix, targets, hb, names):
    assert np.array_equal(_bits(mix), _bits(hb["mix"]))
    for si, k in enumerate(names):
        assert np.array_equal(_bits(targets[si]), _bits(hb[k])), k


@pytest.mark.parametrize("name", ["baseline", "full_multi_instrument"])
@pytest.mark.parametrize("aug_flag", [True, False])
def test_fused_source_delivers_the_reference_pipelines_train_batches(name, aug_flag):
    cfg = _cfg(name, augmentation=aug_flag)
    names = list(cfg["source_names"])
    c = 1 if cfg["mono_downmix"] else 2
    tracks = _tracks(cfg, [400, 257, 333], seed=6)
    host = datasets.get_dataset(cfg, [4, T_IN, c], [4, T_OUT, c], "train", tracks, seed=21)
    fused = datasets.FusedSnippetSource(cfg, tracks, T_IN, T_OUT, 4, DEV, seed=21)
    torch_src = datasets.DeviceSnippetSource(cfg, tracks, T_IN, T_OUT, 4, DEV, seed=21)
    for _ in range(6):
        mix, targets = fused()
        assert mix.shape == (4, T_IN, c) and targets.shape == (len(names), 4, T_OUT, c) and mix.is_contiguous()
        _same_batch(mix, targets, next(host), names)
        tmix, ttargets = torch_src()
        assert torch.equal(mix, tmix) and torch.equal(targets, ttargets)


def test_fused_source_delivers_the_whole_valid_pass():
    cfg = _cfg("full_multi_instrument")
    names = list(cfg["source_names"])
    tracks = _tracks(cfg, [400, 257, 333], seed=9)
    want = list(datasets.get_dataset(cfg, [4, T_IN, 2], [4, T_OUT, 2], "valid", tracks))
    fused = datasets.FusedSnippetSource(cfg, tracks, T_IN, T_OUT, 4, DEV, partition="valid")
    got = list(fused)
    assert len(got) == len(want) >= 4
    for (mix, targets), hb in zip(got, want):
        _same_batch(mix, targets, hb, names)
    with pytest.raises(StopIteration):
        fused()


@pytest.mark.parametrize("name", ["baseline", "full_multi_instrument"])
def test_augmented_batches_are_the_oracle_on_the_sources_own_descriptors(name):
    cfg = _cfg(name)
    names = list(cfg["source_names"])
    c = 1 if cfg["mono_downmix"] else 2
    augment = {"remix": 0.6, "polarity": 0.5}
    if c == 2:
        augment["channel_swap"] = 0.5
    tracks = _tracks(cfg, [400, 257, 333], seed=12)
    for t_in, t_out in ((T_IN, T_OUT), (64, 64)):
        pad = (t_in - t_out) // 2
        padded = [datasets.pad_track(t, pad) for t in tracks]
        planes = [np.concatenate([p[k] for p in padded]) for k in names]
        mix_plane = np.concatenate([p["mix"] for p in padded])
        fused = datasets.FusedSnippetSource(cfg, tracks, t_in, t_out, 4, DEV, seed=3, augment=augment)
        flags, moved = set(), 0
        for _ in range(6):
            table = fused.descriptors().copy()
            assert table.shape == (4, len(names)) and table.dtype == datasets.SNIPPET_DTYPE and fused.mix_mode == 1
            assert fused.descriptors() is fused.descriptors()                           # peeking does not advance the stream
            mix, targets = fused()
            want_mix, want_tgt, _ = _snippets_np.gather(planes, mix_plane, table, 1, t_in, t_out)
            assert np.array_equal(_bits(mix), _bits(want_mix)) and np.array_equal(_bits(targets), _bits(want_tgt))
            if pad == 0:                             # no crop: the delivered targets ARE the windows the mix sums, in order
                acc = targets[0].clone()
                for s in range(1, len(names)):
                    acc = acc + targets[s]
                assert torch.equal(acc, mix)
            flags |= set(table["flags"].ravel().tolist())
            moved += int((table["start"][:, 1:] != table["start"][:, :1]).any())
        assert flags == ({0, 1, 2, 3} if c == 2 else {0, 2}) and moved >= 4


# ---------------------------------------------------------------------------------------- end to end
def _tiny(tmp, **kw):
    base = dict(num_layers=3, num_initial_filters=8, num_frames=40, batch_size=4, epoch_it=3, worse_epochs=1,
                num_snippets_per_track=6, cache_size=8, model_base_dir=os.path.join(tmp, "ckpt"),
                log_dir=os.path.join(tmp, "logs"), init_sup_sep_lr=1e-3)
    base.update(kw)
    return wun.get_config("baseline_stereo", **base)


def _run(cfg, tracks, exp):
    path = training.train(cfg, exp, batch_source=validation._train_source(cfg, tracks, seed=5))
    losses = [json.loads(l)["sep_loss"] for l in open(os.path.join(cfg["log_dir"], exp, "train.jsonl"))]
    return path, losses, dict(np.load(path))


def test_training_and_validation_with_the_fused_producer(tmp_path, monkeypatch):
    monkeypatch.setenv("WUN_NO_TUNE", "1")
    cfg = _tiny(str(tmp_path))
    fcfg = dict(cfg, data_producer="fused")
    tracks = _tracks(cfg, [700, 800, 650], seed=1)
    path, losses, arrays = _run(cfg, tracks, "torch")
    fpath, flosses, farrays = _run(fcfg, tracks, "fused")
    assert len(losses) == 3 and losses == flosses
    assert sorted(arrays) == sorted(farrays)
    for k in arrays:
        assert np.array_equal(arrays[k], farrays[k]), k
    valid = _tracks(cfg, [600, 900], seed=2)
    a = validation.test(cfg, "valid", "torch", path, tracks=valid)
    b = validation.test(fcfg, "valid", "fused", fpath, tracks=valid)
    assert a == b and np.isfinite(a) and a > 0
    # the augmentations: the run ends with finite losses and weights that moved
    acfg = dict(fcfg, augment={"remix": 0.5, "polarity": 0.5})
    apath, alosses, aarrays = _run(acfg, tracks, "augmented")
    assert len(alosses) == 3 and np.isfinite(alosses).all()
    assert alosses != losses
    init = wun.UnetAudioSeparator(cfg)
    start = {n: v.detach().cpu().numpy() for n, v in init.variables().items()}
    changed = [n for n in start if n in aarrays and not np.array_equal(start[n], aarrays[n])]
    assert changed and all(np.isfinite(aarrays[n]).all() for n in start if n in aarrays)
