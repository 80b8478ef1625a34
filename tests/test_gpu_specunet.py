"""GPU tests of the whole spectrogram U-Net through UnetSpectrogramSeparator (wun_spec_forward) against the
float64 oracle tests/_specunet_np.py.

Geometries: frame 64 / hop 48, L = 2, nif = 3, F = 8, B = 2 (the smallest with a skip); 64 / 48, L = 1, F = 2 (no up path: the
mask layer reads the bottleneck alone); 1024 / 768, L = 6, nif = 4, F = 64, B = 1 (the real depth and bin count at the smallest
legal frame count).  Audio of amplitude 0.3, glorot-scaled kernels, moving_variance in [0.5, 2], moving_mean / beta / biases of
order 0.1, fixed seeds.

Tolerance: every stage of the network is Lipschitz, so there are no conditioning exclusions; no end-to-end bound can be derived,
so it is measured at run time on a stand-in that is not the code under test -- the same oracle evaluated in float32 on the CPU.
bound = 8 x max |float32 oracle - float64 oracle| on the same inputs, floored at 2^-20 x max |output| (the factor 8: the MFMA's
strictly ascending order and the CPU's blocked order differ, and a 12-layer chain compounds that).  Audio and magnitudes each."""
import os
import sys

import ctypes as C

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _specunet_np as ora  # noqa: E402
import _postfilter_np as pf  # noqa: E402
from _observed import record  # noqa: E402
from _unaligned import _offset_copy, _offset_full  # noqa: E402

import wave_u_net_amd as wun  # noqa: E402
from wave_u_net_amd import _lib, checkpoint, datasets, evaluate, spectral, validation  # noqa: E402
from wave_u_net_amd.spectrogram import UnetSpectrogramSeparator  # noqa: E402

pytestmark = pytest.mark.gpu

# name -> (n_fft, hop, L, nif, F, B)
GEOMETRIES = {"skip": (64, 48, 2, 3, 8, 2), "flat": (64, 48, 1, 3, 2, 2), "deep": (1024, 768, 6, 4, 64, 1)}
_CACHE = {}


def _cfg(geo, **kw):
    n_fft, hop, L, nif, F, B = GEOMETRIES[geo]
    base = dict(num_layers=L, num_initial_filters=nif, spec_frame_len=n_fft, spec_hop=hop, num_frames=(F - 1) * hop + n_fft,
                batch_size=B)
    base.update(kw)
    return wun.get_config("unet_spectrogram", **base)


def _fixture(geo):
    """Inputs, weights and both oracles of a geometry, computed once and left unchanged."""
    if geo not in _CACHE:
        n_fft, hop, L, nif, F, B = GEOMETRIES[geo]
        T = (F - 1) * hop + n_fft
        rng = np.random.RandomState(17 + L + F)
        mix = (0.3 * rng.randn(B, T)).astype(np.float32)
        v = ora.random_variables(L, nif, seed=23 + L)
        ref = {"mix": mix, "vars": v, "T": T}
        for spec in (False, True):
            o64, X, M = ora.forward(mix, v, L, nif, n_fft, hop, return_spectrogram=spec)
            o32, _, _ = ora.forward(mix, v, L, nif, n_fft, hop, dtype=torch.float32, return_spectrogram=spec)
            o64, o32 = np.stack(o64), np.stack(o32)
            stand_in = np.abs(o32 - o64).max()
            ref[spec] = {"want": o64, "stand_in": stand_in, "bound": max(8.0 * stand_in, 2.0 ** -20 * np.abs(o64).max())}
        ref["X"], ref["M"] = X, M
        _CACHE[geo] = ref
    return _CACHE[geo]


def _separator(geo, variables=None, **kw):
    sep = UnetSpectrogramSeparator(_cfg(geo, **kw), device="cuda:0")
    sep.load_variables(_fixture(geo)["vars"] if variables is None else variables)
    return sep


def _run(sep, mix, spec=False):
    outs = sep.get_output(torch.from_numpy(mix[:, :, None]), False, return_spectrogram=spec)
    return np.stack([outs[k].cpu().numpy() for k in sep.source_names])           # [S, B, T, 1] or [S, B, F, K]


@pytest.mark.parametrize("spec", [False, True], ids=["audio", "mags"])
@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_model_against_float64(geo, spec):
    ref = _fixture(geo)
    n_fft, hop, L, nif, F, B = GEOMETRIES[geo]
    got = _run(_separator(geo), ref["mix"], spec)
    if spec:
        assert got.shape == (2, B, F, n_fft // 2 + 1)
    else:
        assert got.shape == (2, B, ref["T"], 1)
        got = got[..., 0]
    want, bound = ref[spec]["want"], ref[spec]["bound"]
    err = np.abs(got - want).max()
    name = "test_model_against_float64[%s-%s]" % (geo, "mags" if spec else "audio")
    record(name, "stand-in (fp32 CPU) max err", ref[spec]["stand_in"], bound)
    record(name, "max err", err, bound)
    assert np.isfinite(got).all() and err <= bound
    assert np.abs(want[0] - want[1]).max() > 100 * bound        # the two sources' networks differ: a swap would show


@pytest.mark.parametrize("geo", ["skip", "deep"])
def test_zero_convs_give_the_half_mask(geo):
    """All conv kernels and biases zero: mask == sigmoid(0) == 0.5 exactly, whatever the batch norms hold; the magnitudes are
    0.5 M bit for bit and the audio is ISTFT_tf(0.5 X) bit for bit."""
    ref = _fixture(geo)
    n_fft, hop, L, nif, F, B = GEOMETRIES[geo]
    sep = _separator(geo, ora.random_variables(L, nif, seed=5, zero_convs=True))
    mix = torch.from_numpy(ref["mix"]).cuda()
    M = spectral.stft_magnitude(mix[None, :, :, None], n_fft, hop, transform="fft")[0, :, 0]      # [B, F, K]
    mags = sep.get_output(mix[:, :, None], False, return_spectrogram=True)
    for k in sep.source_names:
        assert torch.equal(mags[k], 0.5 * M)
    re, im = spectral.stft(mix[None, :, :, None], n_fft, hop, transform="fft")
    half = spectral.istft_tf(0.5 * re, 0.5 * im, n_fft, hop, transform="fft")[0]  # [B, T, 1]
    audio = sep.get_output(mix[:, :, None], False)
    for k in sep.source_names:
        assert torch.equal(audio[k], half)


@pytest.mark.parametrize("transform", ["gemm", "fft"])
@pytest.mark.parametrize("n_fft, hop, F", [(64, 48, 8), (64, 16, 9), (1024, 768, 4)])
def test_istft_tf_against_float64(n_fft, hop, F, transform):
    """wun_istft_tf on fp32 spectra against the oracle.  Bound, as tests/_postfilter_np.py derives it for wun_istft: a frame of the
    inverse carries at most g = 2 K u sum_k c_k (|Re| + |Im|) / n_fft; an output sample the sum of g over its covering frames over
    ITS denominator D[t mod hop], plus 4 u |y| for the overlap-add, the denominator and the division."""
    T = (F - 1) * hop + n_fft
    x = torch.tensor(0.3 * np.random.RandomState(n_fft + hop).randn(3, T), dtype=torch.float64)
    z = ora.stft(x, n_fft, hop).to(torch.complex64)                              # the inputs: fp32 numbers
    re, im = z.real.contiguous(), z.imag.contiguous()
    got = spectral.istft_tf(re.cuda()[None, :, None], im.cuda()[None, :, None], n_fft, hop, transform=transform)[0, :, :, 0].cpu().numpy()
    want = ora.istft_tf(z.to(torch.complex128), n_fft, hop).numpy()
    K = n_fft // 2 + 1
    g = 2 * K * pf.U * ((re.abs() + im.abs()).double().numpy() * pf.c_k(n_fft)).sum(-1) / n_fft        # [R, F]
    num = pf._overlap_add(np.broadcast_to(g[:, :, None], (3, F, n_fft)), T, hop, 0)
    bound = num / ora.steady_denominator(n_fft, hop).numpy()[np.arange(T) % hop] + 4 * pf.U * np.abs(want)
    ratio = (np.abs(got - want) / bound).max()
    record("test_istft_tf_against_float64[%d-%d-%s]" % (n_fft, hop, transform), "max err / bound", ratio, 1.0)
    assert np.isfinite(got).all() and (np.abs(got - want) <= bound).all()
    # the edges differ from wun_istft's (it divides by the covering frames' sum there), the steady state does not
    other = spectral.istft(re.cuda()[None, :, None], im.cuda()[None, :, None], T, n_fft, hop, transform=transform)[0, :, :, 0].cpu().numpy()
    assert np.abs(other[:, 1] - got[:, 1]).max() > 0
    if hop < n_fft // 2:
        mid = slice(n_fft, T - n_fft)
        assert np.abs(other[:, mid] - got[:, mid]).max() <= 2 * bound[:, mid].max()


@pytest.mark.parametrize("geo", ["skip", "deep"])
def test_last_bin_is_half_the_mixture(geo):
    ref = _fixture(geo)
    n_fft, hop = GEOMETRIES[geo][:2]
    sep = _separator(geo)
    mix = torch.from_numpy(ref["mix"]).cuda()
    M = spectral.stft_magnitude(mix[None, :, :, None], n_fft, hop, transform="fft")[0, :, 0]
    mags = sep.get_output(mix[:, :, None], False, return_spectrogram=True)
    for k in sep.source_names:
        assert torch.equal(mags[k][:, :, -1], 0.5 * M[:, :, -1])
        assert not torch.equal(mags[k][:, :, :-1], 0.5 * M[:, :, :-1])


def _swap_sources(variables, L):
    """The variable blocks of source 0 and source 1 exchanged (conv / conv_transpose indices +- L, batch norms +- (2L - 1))."""
    def index(name):
        stem = name.split("/")[1]
        base, _, num = stem.rpartition("_")
        if num.isdigit():
            return base, int(num)
        return stem, 0

    out = {}
    for name, val in variables.items():
        stem, i = index(name)
        per = 2 * L - 1 if stem == "BatchNorm" else L
        j = i + per if i < per else i - per
        out["separator/%s/%s" % (stem if j == 0 else "%s_%d" % (stem, j), name.split("/")[2])] = val
    assert set(out) == set(variables)
    return out


@pytest.mark.parametrize("geo", ["skip", "deep"])
def test_swapping_the_sources_swaps_the_outputs(geo):
    ref = _fixture(geo)
    L = GEOMETRIES[geo][2]
    a = _run(_separator(geo), ref["mix"])
    b = _run(_separator(geo, _swap_sources(ref["vars"], L)), ref["mix"])
    assert np.array_equal(a[0].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[0].view(np.uint32))
    assert not np.array_equal(a[0], a[1])


def test_batch_independence_and_repeatability():
    ref = _fixture("skip")
    sep = _separator("skip")
    for spec in (False, True):
        both = _run(sep, ref["mix"], spec)
        alone = _run(sep, ref["mix"][1:2], spec)
        assert np.array_equal(both[:, 1:2].view(np.uint32), alone.view(np.uint32))
        fresh = _run(_separator("skip"), ref["mix"], spec)                       # two fresh separators: equal bits
        assert np.array_equal(both.view(np.uint32), fresh.view(np.uint32))


def test_initial_weights_run_and_two_separators_agree():
    mix = _fixture("skip")["mix"]
    a = _run(UnetSpectrogramSeparator(_cfg("skip"), device="cuda:0"), mix)
    b = _run(UnetSpectrogramSeparator(_cfg("skip"), device="cuda:0"), mix)
    assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("fmt", ["npz", "tf"])
def test_checkpoint_round_trip(tmp_path, fmt):
    ref = _fixture("skip")
    sep = _separator("skip")
    sep.global_step = 321
    path = checkpoint.save_checkpoint(sep, str(tmp_path / ("ck.npz" if fmt == "npz" else "ck-321")), fmt=fmt)
    fresh = UnetSpectrogramSeparator(_cfg("skip"), device="cuda:0", seed=99)
    assert checkpoint.load_checkpoint(fresh, path, with_optimizer=False) == 321
    for spec in (False, True):
        assert np.array_equal(_run(sep, ref["mix"], spec).view(np.uint32), _run(fresh, ref["mix"], spec).view(np.uint32))


@pytest.mark.parametrize("raw", [True, False], ids=["mse", "mag_l1"])
def test_validation_loss_matches_the_oracle(tmp_path, raw):
    """validation.test on a two-track toy partition, both objectives of Test.py:63-70, against the float64 oracle on the same
    batches.  The bound is the end-to-end bound e of the geometry propagated through the loss: a mean of |d| moves by at most e,
    a mean of d^2 by at most 2 max|d| e + e^2; the running mean over batches and the mean over sources keep either figure."""
    n_fft, hop, L, nif, F, B = GEOMETRIES["skip"]
    cfg = _cfg("skip", raw_audio_loss=raw, log_dir=str(tmp_path / "logs"), num_snippets_per_track=3, cache_size=4)
    ref = _fixture("skip")
    sep = _separator("skip", raw_audio_loss=raw)
    rng = np.random.default_rng(3)
    tracks = [datasets.make_track({k: rng.uniform(-0.3, 0.3, (n, 1)).astype(np.float32) for k in cfg["source_names"]}, cfg)
              for n in (900, 1200)]
    got = validation.test(cfg, "valid", "exp", None, tracks=tracks, separator=sep)
    in_shape, out_shape = sep.get_padding(np.array([cfg["batch_size"], cfg["num_frames"], 0]))
    total, k, bound = 0.0, 1, 0.0
    e = ref[not raw]["bound"]
    for b in datasets.get_dataset(cfg, in_shape, out_shape, "valid", tracks):
        outs, _, _ = ora.forward(b["mix"][:, :, 0], ref["vars"], L, nif, n_fft, hop, return_spectrogram=not raw)
        cur = 0.0
        for s, name in enumerate(cfg["source_names"]):
            real = torch.from_numpy(b[name][:, :, 0]).double()
            if raw:
                d = real.numpy() - outs[s]
                cur += np.mean(d ** 2)
                bound = max(bound, 2 * np.abs(d).max() * e + e * e)
            else:
                d = ora.stft(real, n_fft, hop).abs().numpy() - outs[s]
                cur += np.mean(np.abs(d))
                # (+ the targets' own fp32 magnitudes: sqrt(2) beta per bin and the root's roundings, as test_gpu_postfilter.py)
                mt = ora.stft(real, n_fft, hop).abs().numpy()
                beta = pf.beta(real.numpy(), n_fft, hop, 0, F)[:, :, None]
                bound = max(bound, e + float(np.mean(np.sqrt(2.0) * beta + 2.0 ** -22 * mt)))
        cur /= cfg["num_sources"]
        total += (cur - total) / k
        k += 1
    assert k > 2
    record("test_validation_loss_matches_the_oracle[%s]" % ("mse" if raw else "mag_l1"), "loss err", abs(got - total), bound)
    assert abs(got - total) <= bound + 2.0 ** -22 * abs(total)
    assert os.path.exists(os.path.join(cfg["log_dir"], "exp", "test.jsonl"))


def test_predict_track_returns_the_tracks_length():
    cfg = _cfg("skip")
    sep = _separator("skip")
    n = int(2.5 * cfg["num_frames"])
    audio = (0.3 * np.random.RandomState(4).randn(n, 1)).astype(np.float32)
    preds = evaluate.predict_track(cfg, sep, audio, cfg["expected_sr"])
    assert set(preds) == set(cfg["source_names"])
    for k in preds:
        assert preds[k].shape == (n, 1) and np.isfinite(preds[k]).all() and np.abs(preds[k]).max() > 0
    # the first hop is the model on the first num_frames samples
    first = _run(sep, audio[None, :cfg["num_frames"], 0])
    assert np.array_equal(preds[cfg["source_names"][0]][:cfg["num_frames"]], first[0, 0])
    # and the device path of the file-level programs gives the same track
    dev = evaluate.separate_track(cfg, sep, audio, cfg["expected_sr"])
    for k in preds:
        assert dev[k].shape == (n, 1) and np.array_equal(dev[k], preds[k])


# ---------------------------------------------------------------------------------------------------- wun_spec_forward, directly
# The separator class asks the entry for two sources and one output at a time, into an uninitialised workspace.  The entry
# allows 1..8 sources and both outputs in one call and promises that its bits do not depend on what the workspace held, on
# pointer alignment beyond 4 bytes or on the stream: these tests call it through the C ABI with buffers of their own.
GUARD = 64                                                   # floats before and after a guarded buffer
GUARD_BITS = 0x7FC0BEEF                                      # a NaN no arithmetic produces


class _Direct(object):
    """wun_spec_forward on a geometry of GEOMETRIES for S sources: the flat params buffer filled from wun_spec_tensor's table."""

    def __init__(self, geo, S, seed=None):
        self.lib = _lib.load()
        self.n_fft, self.hop, self.L, self.nif, self.F, self.B = GEOMETRIES[geo]
        self.S, self.K, self.T = S, self.n_fft // 2 + 1, (self.F - 1) * self.hop + self.n_fft
        self.cfg = _lib.WunSpecConfig(self.L, self.nif, S, self.n_fft, self.hop)
        self.vars = ora.random_variables(self.L, self.nif, seed=(31 + self.L + S) if seed is None else seed, S=S)
        n, info = int(self.lib.wun_spec_num_tensors(C.byref(self.cfg))), _lib.WunTensorInfo()
        host = np.full(int(self.lib.wun_spec_param_floats(C.byref(self.cfg))), np.nan, np.float32)
        for i in range(n):
            _lib.check(self.lib.wun_spec_tensor(C.byref(self.cfg), i, C.byref(info)))
            v = self.vars[info.name.decode()]
            assert v.shape == tuple(int(info.shape[d]) for d in range(info.ndim))
            host[info.offset:info.offset + v.size] = v.reshape(-1)
        assert n == len(self.vars) and np.isfinite(host).all()             # packed: every float of the buffer belongs to a tensor
        self.params = torch.from_numpy(host).cuda()
        self.mix_host = _fixture(geo)["mix"]
        self.mix = torch.from_numpy(self.mix_host).cuda()
        self.table = spectral._fft_table(self.n_fft, self.mix.device)
        self.ws_floats = int(self.lib.wun_spec_workspace_floats(C.byref(self.cfg), self.B, self.T))
        assert self.ws_floats > 0

    def shapes(self):
        return (self.S, self.B, self.T, 1), (self.S, self.B, self.F, self.K)

    def buffers(self, audio=True, mags=True):
        """Fresh NaN-filled outputs (an unwritten float shows) and workspace."""
        sa, sm = self.shapes()
        nan = float("nan")
        return (torch.full(sa, nan, device="cuda") if audio else None, torch.full(sm, nan, device="cuda") if mags else None,
                torch.full((self.ws_floats,), nan, device="cuda"))

    def run(self, audio, mags, ws, mix=None, params=None):
        """One call on the current stream; the outputs as numpy (None for an output not asked for)."""
        mix = self.mix if mix is None else mix
        params = self.params if params is None else params
        stream = torch.cuda.current_stream()
        _lib.check(self.lib.wun_spec_forward(C.byref(self.cfg), params.data_ptr(), mix.data_ptr(), self.B, self.T, self.table.data_ptr(),
                                             None if audio is None else audio.data_ptr(), None if mags is None else mags.data_ptr(),
                                             ws.data_ptr(), C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        return tuple(None if t is None else t.cpu().numpy() for t in (audio, mags))

    def both(self):
        """(audio, mags) of the plain call: both outputs at once, aligned buffers, the default stream.  Computed once."""
        if not hasattr(self, "_both"):
            self._both = self.run(*self.buffers())
            assert all(np.isfinite(a).all() for a in self._both)
        return self._both


_DIRECT = {}


def _direct(geo, S):
    if (geo, S) not in _DIRECT:
        _DIRECT[(geo, S)] = _Direct(geo, S)
    return _DIRECT[(geo, S)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("S", [1, 3])
def test_other_source_counts_against_float64(S):
    """S = 1 and S = 3 (the table arithmetic s L + i, s (2L - 1) + j beyond S = 2), audio and magnitudes, under the bound rule of
    this file: 8 x the float32-CPU oracle's own error, floored at 2^-20 max |output|."""
    d = _direct("skip", S)
    got = dict(zip((False, True), d.both()))
    for spec in (False, True):
        o64, _, _ = ora.forward(d.mix_host, d.vars, d.L, d.nif, d.n_fft, d.hop, S=S, return_spectrogram=spec)
        o32, _, _ = ora.forward(d.mix_host, d.vars, d.L, d.nif, d.n_fft, d.hop, S=S, dtype=torch.float32, return_spectrogram=spec)
        want, o32 = np.stack(o64), np.stack(o32)
        stand_in = np.abs(o32 - want).max()
        bound = max(8.0 * stand_in, 2.0 ** -20 * np.abs(want).max())
        g = got[spec][..., 0] if not spec else got[spec]
        assert g.shape == want.shape == ((S, d.B, d.F, d.K) if spec else (S, d.B, d.T))
        err = np.abs(g - want).max()
        name = "test_other_source_counts_against_float64[%d-%s]" % (S, "mags" if spec else "audio")
        record(name, "stand-in (fp32 CPU) max err", stand_in, bound)
        record(name, "max err", err, bound)
        assert np.isfinite(g).all() and err <= bound
        for i in range(S):
            for j in range(i + 1, S):                        # every source has its own network: a mixed-up index would show
                assert np.abs(want[i] - want[j]).max() > 100 * bound


@pytest.mark.parametrize("geo, S", [("skip", 2), ("skip", 3), ("flat", 2)])
def test_both_outputs_in_one_call_are_the_two_single_calls(geo, S):
    d = _direct(geo, S)
    audio, mags = d.both()
    a, _, ws = d.buffers(mags=False)
    alone_audio, none = d.run(a, None, ws)
    assert none is None
    _, m, ws = d.buffers(audio=False)
    _, alone_mags = d.run(None, m, ws)
    assert np.array_equal(_bits(audio), _bits(alone_audio)) and np.array_equal(_bits(mags), _bits(alone_mags))


def _guarded(n):
    """-> (whole, interior): n floats with GUARD floats of GUARD_BITS on either side; the interior holds the pattern too."""
    whole = torch.full((n + 2 * GUARD,), GUARD_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    return whole, whole[GUARD:GUARD + n]


def _guards_intact(whole):
    w = whole.view(torch.int32)
    return bool((w[:GUARD] == GUARD_BITS).all()) and bool((w[-GUARD:] == GUARD_BITS).all())


@pytest.mark.parametrize("geo", ["skip", "flat"])
def test_workspace_contents_do_not_matter_and_nothing_is_written_outside(geo):
    d = _direct(geo, 2)
    sa, sm = d.shapes()
    outs = []
    for fill in (0.0, float("nan")):
        wa, a = _guarded(int(np.prod(sa)))
        wm, m = _guarded(int(np.prod(sm)))
        ww, ws = _guarded(d.ws_floats)
        ws.fill_(fill)
        outs.append(d.run(a.view(*sa), m.view(*sm), ws))
        assert _guards_intact(wa) and _guards_intact(wm) and _guards_intact(ww)
        assert all(np.isfinite(o).all() for o in outs[-1])                   # every output float was written
    for zeroed, poisoned, plain in zip(outs[0], outs[1], d.both()):
        assert np.array_equal(_bits(zeroed), _bits(poisoned)) and np.array_equal(_bits(zeroed), _bits(plain))


@pytest.mark.parametrize("which", ["mix", "params", "audio", "mags", "workspace", "all"])
def test_forward_bits_do_not_depend_on_alignment(which):
    """Every buffer one float behind an allocation's start, one at a time and all together.  The workspace too: its float64 tail
    (the window squares of the inverse STFT) is aligned by the library from the pointer it is given (f64_tail, csrc/wun_stft.h),
    and the scratch formula holds the room."""
    d = _direct("skip", 2)
    sa, sm = d.shapes()
    moved = lambda name: which in (name, "all")              # noqa: E731
    nan = float("nan")
    a = _offset_full(sa, nan) if moved("audio") else torch.full(sa, nan, device="cuda")
    m = _offset_full(sm, nan) if moved("mags") else torch.full(sm, nan, device="cuda")
    ws = _offset_full((d.ws_floats,), nan) if moved("workspace") else torch.full((d.ws_floats,), nan, device="cuda")
    got = d.run(a, m, ws, mix=_offset_copy(d.mix) if moved("mix") else None, params=_offset_copy(d.params) if moved("params") else None)
    for g, want in zip(got, d.both()):
        assert np.array_equal(_bits(g), _bits(want))


def test_forward_on_a_side_stream():
    d = _direct("skip", 2)
    want = d.both()
    a, m, ws = d.buffers()
    torch.cuda.synchronize()                                 # the buffers' fills ran on the default stream
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream().cuda_stream == side.cuda_stream != torch.cuda.default_stream().cuda_stream
        got = d.run(a, m, ws)
    for g, w in zip(got, want):
        assert np.array_equal(_bits(g), _bits(w))
