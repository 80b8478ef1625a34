"""GPU tests of the phase vocoder (include/wun.h: wun_time_stretch; vocoder.time_stretch / pitch_shift): batched
heterogeneous jobs against the float64 oracle of tests/_vocoder_np.py, the identity at 1/1, the frequency of a stretched and of
a pitch-shifted tone, and the independence of a job's bits from the other jobs, the launch set, the scratch and the floats around
its span; then the fused producer with the two augmentations against the two entries it calls, bit for bit, and a tiny training
run."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import wave_u_net_amd as wun                                              # noqa: E402
from wave_u_net_amd import _lib, datasets, resample, training, validation, vocoder   # noqa: E402

import _vocoder_np as vnp                                                 # noqa: E402
from _observed import record                                              # noqa: E402

DEV = "cuda:0"
RATIOS = [(10, 9), (9, 10), (2, 1), (1, 2), (20, 21)]
# max |y - y64| / max |y64| against the oracle: 8x the largest value observed over the cases below on an MI355X,
# and never above 1e-4 -- a misplaced frame or bin shows at 1e-2 and above
TOL_ORACLE = 9.0e-5                 # observed: 1.13e-5 (n_fft 64 and 128, C 1); 6.7e-7 .. 4.7e-6 at 2048 and 4096
# the same figure of the identity at 1/1 against x itself; never above 1e-5
TOL_IDENTITY = 2.9e-6               # observed: 3.6e-7 (n_fft 64), 1.8e-7 (256, 2048)


def _bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def _signal(n, c, seed, f0=0.0731):
    """White noise of sigma 0.5 plus one sinusoid: every bin stays far above the float32 FFT's error."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)[:, None]
    return (rng.normal(0.0, 0.5, (n, c)) + 0.8 * np.sin(2.0 * np.pi * f0 * t + np.arange(c))).astype(np.float32)


class _Arena:
    """One device buffer of NaN; take(n, k) gives n floats at k floats past a 16-byte boundary with at least four NaN floats
    before and behind."""

    def __init__(self, floats):
        self.buf = torch.full((floats,), float("nan"), dtype=torch.float32, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.at = 0
        self.views = []

    def take(self, n, k):
        lo = (self.at + 4 + 3) // 4 * 4 + k
        assert lo + n + 4 <= self.buf.numel()
        self.at = lo + n
        v = self.buf[lo:lo + n]
        assert v.data_ptr() % 16 == 4 * k
        self.views.append((lo, n))
        return v

    def guards_intact(self):
        """Every float outside the views handed out is still NaN."""
        mask = torch.ones(self.buf.numel(), dtype=torch.bool, device=DEV)
        for lo, n in self.views:
            mask[lo:lo + n] = False
        return bool(torch.isnan(self.buf[mask]).all())


def _run(jobs, c, n_fft, hop, scratch_fill=None):
    """jobs: (x view, y view, n_in, n_out, num, den); one wun_time_stretch call."""
    table = vocoder.job_table([(x.data_ptr(), y.data_ptr(), n_in, n_out, num, den) for x, y, n_in, n_out, num, den in jobs])
    scratch = torch.empty(vocoder.scratch_floats(table, c, n_fft, hop), dtype=torch.float32, device=DEV)
    if scratch_fill is not None:
        scratch.fill_(scratch_fill)
    vocoder.run(table, c, n_fft, hop, scratch, DEV)
    torch.cuda.synchronize()


def _cases(n_ins):
    """Every ratio x every n_in x (the full length, a length cut short)."""
    out = []
    for num, den in RATIOS:
        for n_in in n_ins:
            full = vnp.stretch_frames(n_in, num, den)
            out += [(n_in, full, num, den), (n_in, full - full // 3 - 1, num, den)]
    return out


# ---------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("c", [1, 2])
@pytest.mark.parametrize("n_fft,hop,n_ins,ratios", [
    (64, 16, (700, 3000), None),                 # the radix-2 tail, 32 frames per workgroup
    (128, 32, (700, 3000), None),                # radix 4 only
    (2048, 512, (700, 5000), None),              # one frame per workgroup
    (4096, 1024, (9000,), [(10, 9)]),            # two butterflies per lane
])
def test_jobs_of_one_call_match_the_oracle(n_fft, hop, n_ins, ratios, c):
    cases = _cases(n_ins) if ratios is None else [(n_ins[0], vnp.stretch_frames(n_ins[0], *ratios[0]) - 5) + ratios[0]]
    xin = _Arena(sum(n + 12 for n, _, _, _ in cases) * c + 64)
    yout = _Arena(sum(n + 12 for _, n, _, _ in cases) * c + 64)
    jobs, hosts = [], []
    for i, (n_in, n_out, num, den) in enumerate(cases):
        h = _signal(n_in, c, seed=1000 * n_fft + 10 * i + c)
        xv = xin.take(n_in * c, 1 + i % 3)
        xv.copy_(torch.from_numpy(h).reshape(-1))
        jobs.append((xv, yout.take(n_out * c, 3 - i % 3), n_in, n_out, num, den))
        hosts.append(h)
    _run(jobs, c, n_fft, hop)
    assert yout.guards_intact() and xin.guards_intact()
    worst = 0.0
    for (xv, yv, n_in, n_out, num, den), h in zip(jobs, hosts):
        want = vnp.time_stretch(h, num, den, n_fft, hop, n_out)
        got = yv.cpu().numpy().reshape(n_out, c).astype(np.float64)
        assert np.isfinite(got).all(), (n_in, n_out, num, den)
        err = np.abs(got - want).max() / np.abs(want).max()
        worst = max(worst, err)
        assert err < TOL_ORACLE, (n_in, n_out, num, den, err)
    record("test_gpu_vocoder::oracle", "n_fft %d hop %d C %d" % (n_fft, hop, c), worst, TOL_ORACLE)


# ---------------------------------------------------------------------------------------- identity
@pytest.mark.parametrize("n_fft,hop", [(64, 16), (256, 64), (2048, 512)])
def test_unit_ratio_reproduces_the_input(n_fft, hop):
    worst = 0.0
    for c in (1, 2):
        h = _signal(5000, c, seed=n_fft + c)
        x = torch.from_numpy(h).to(DEV)
        y = vocoder.time_stretch(x, 1, 1, n_fft, hop)
        assert tuple(y.shape) == (5000, c)
        worst = max(worst, float(np.abs(y.cpu().numpy().astype(np.float64) - h).max() / np.abs(h).max()))
    record("test_gpu_vocoder::identity", "n_fft %d hop %d" % (n_fft, hop), worst, TOL_IDENTITY)
    assert worst < TOL_IDENTITY


# ---------------------------------------------------------------------------------------- a tone keeps / moves its frequency
F0 = 16.0 / 256.0


def _tone(n):
    return (0.5 * np.sin(2.0 * np.pi * F0 * np.arange(n, dtype=np.float64)))[:, None].astype(np.float32)


@pytest.mark.parametrize("num,den", [(10, 9), (4, 5)])
def test_a_stretched_tone_keeps_its_frequency(num, den):
    x = torch.from_numpy(_tone(4000)).to(DEV)
    y = vocoder.time_stretch(x, num, den, 256, 64)
    assert y.shape[0] == vnp.stretch_frames(4000, num, den)                # a resampler would be 10 % / 25 % off in frequency
    f = vnp.peak_frequency(y[:, 0].cpu().numpy(), 512)
    record("test_gpu_vocoder::tone", "stretch %d/%d" % (num, den), abs(f / F0 - 1.0), 1e-4)
    assert abs(f - F0) < 1e-4 * F0


def test_a_pitch_shifted_tone_moves_by_the_ratio():
    x = torch.from_numpy(_tone(4000)).to(DEV)
    y = vocoder.pitch_shift(x, 18, 17, 256, 64)
    assert tuple(y.shape) == (4000, 1)
    f = vnp.peak_frequency(y[:, 0].cpu().numpy(), 512)
    want = F0 * 17.0 / 18.0
    record("test_gpu_vocoder::tone", "pitch_shift 18/17", abs(f / want - 1.0), 1e-3)
    assert abs(f - want) < 1e-3 * want


# ---------------------------------------------------------------------------------------- bit-level independence
@pytest.mark.parametrize("c", [1, 2])
def test_a_jobs_bits_do_not_depend_on_its_neighbours_the_scratch_or_its_surroundings(c):
    n_fft, hop, n_in, num, den = 256, 64, 1500, 10, 9
    n_out = vnp.stretch_frames(n_in, num, den) - 7
    h = _signal(n_in, c, seed=40 + c)
    others = [_signal(300 + 37 * i, c, seed=500 + i) for i in range(79)]

    def job(arena_x, arena_y, host, n_o, ratio, k):
        xv = arena_x.take(host.size, k)
        xv.copy_(torch.from_numpy(host).reshape(-1))
        return (xv, arena_y.take(n_o * c, (k + 1) % 4), host.shape[0], n_o) + ratio

    def other_jobs(ax, ay, idx):
        return [job(ax, ay, others[i], vnp.stretch_frames(others[i].shape[0], *RATIOS[i % 5]), RATIOS[i % 5], i % 4) for i in idx]

    floats = (n_in + sum(o.shape[0] for o in others) * 3 + 80 * 16) * c + 64
    # alone
    ax, ay = _Arena(floats), _Arena(floats)
    alone = job(ax, ay, h, n_out, (num, den), 1)
    _run([alone], c, n_fft, hop)
    want = _bits(alone[1])
    assert np.isfinite(alone[1].cpu().numpy()).all()
    # among 64 others (job 30 of 65: the first launch set is full), and as job 65 of 80 (the second launch set)
    for place, n_others in ((30, 64), (64, 79)):
        ax, ay = _Arena(floats), _Arena(floats)
        before = other_jobs(ax, ay, range(place))
        mine = job(ax, ay, h, n_out, (num, den), 3)
        jobs = before + [mine] + other_jobs(ax, ay, range(place, n_others))
        assert len(jobs) == n_others + 1
        _run(jobs, c, n_fft, hop, scratch_fill=float("nan"))               # NaN-filled scratch
        assert np.array_equal(_bits(mine[1]), want), place
        assert ay.guards_intact() and ax.guards_intact()
        assert all(np.isfinite(j[1].cpu().numpy()).all() for j in jobs)
    # a span inside a longer buffer: NaN planted around it (the arena's fill) or finite floats there change nothing
    ax, ay = _Arena(floats), _Arena(floats)
    wide = torch.from_numpy(_signal(n_in + 40, c, seed=7)).to(DEV).reshape(-1)
    wide[20 * c:(20 + n_in) * c] = torch.from_numpy(h).reshape(-1).to(DEV)
    inside = (wide[20 * c:(20 + n_in) * c], ay.take(n_out * c, 2), n_in, n_out, num, den)
    _run([inside], c, n_fft, hop, scratch_fill=float("nan"))
    assert np.array_equal(_bits(inside[1]), want)


# ---------------------------------------------------------------------------------------- the fused producer
P_TIN, P_TOUT, P_FFT = 2500, 1100, (256, 64)


def _producer(augment, B, seed=3):
    """Two stereo tracks whose padded lengths are 3300 and 2700 (planes of 6000 frames): a time stretch at 10/9 reads 2778
    frames, more than the second track holds."""
    cfg = wun.get_config("baseline_stereo", batch_size=B, num_snippets_per_track=3, cache_size=5)
    rng = np.random.default_rng(11)
    tracks = [datasets.make_track({k: rng.uniform(-0.4, 0.4, (n, 2)).astype(np.float32) for k in cfg["source_names"]}, cfg)
              for n in (1900, 1300)]
    if augment is not None:
        augment = dict(augment, vocoder_fft=list(P_FFT))
    fused = datasets.FusedSnippetSource(cfg, tracks, P_TIN, P_TOUT, B, DEV, seed=seed, augment=augment)
    assert fused.plane_frames == 6000 and fused.channels == 2 and len(fused.names) == 2
    return fused


def _by_the_two_entries(fused, table, rates, jobs):
    """The batch of (table, rates, jobs) from wun_time_stretch on the spans the jobs name, then wun_gather_snippets_speed, on
    planes of this test's own: the tracks, then slots of NaN."""
    B, S, c = table.shape[0], len(fused.names), fused.channels
    planes = [fused.data[k].clone() for k in fused.names]
    for pl in planes:
        pl[fused.plane_frames:] = float("nan")
    rows = []
    for b, s in np.argwhere(jobs[:, :, 1] > 0):
        start, n_span, num, den = (int(v) for v in jobs[b, s])
        n_out = datasets.speed_source_frames(P_TIN, *fused.bank_rates[rates[b, s] - 1]) if rates[b, s] else P_TIN
        base = planes[s].data_ptr()
        rows.append((base + 8 * start, base + 8 * (fused.plane_frames + b * fused.slot_frames), n_span, n_out, num, den))
        assert table["start"][b, s] == fused.plane_frames + b * fused.slot_frames
    if rows:
        jt = vocoder.job_table(rows)
        scratch = torch.full((vocoder.scratch_floats(jt, c, *P_FFT),), float("nan"), dtype=torch.float32, device=DEV)
        vocoder.run(jt, c, P_FFT[0], P_FFT[1], scratch, DEV)
    bank = None
    if fused.bank_rates:
        tabs = [torch.from_numpy(resample.design(up, down)).to(DEV) for up, down in fused.bank_rates]
        bank = _lib.WunSpeedBank()
        bank.n = len(tabs)
        for i, ((up, down), t) in enumerate(zip(fused.bank_rates, tabs)):
            bank.up[i], bank.down[i], bank.table[i] = up, down, t.data_ptr()
    mix = torch.full((B, P_TIN, c), float("nan"), device=DEV)
    tgt = torch.full((S, B, P_TOUT, c), float("nan"), device=DEV)
    arr = (C.c_void_p * S)(*[pl.data_ptr() for pl in planes])
    table, rates = np.ascontiguousarray(table), np.ascontiguousarray(rates, dtype=np.uint8)
    _lib.check(_lib.load().wun_gather_snippets_speed(
        arr, None, int(planes[0].shape[0]), c, S, B, P_TIN, P_TOUT, table.ctypes.data, rates.ctypes.data,
        None if bank is None else C.addressof(bank), 1, mix.data_ptr(), tgt.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return mix, tgt


@pytest.mark.parametrize("key", ["pitch_shift", "time_stretch"])
@pytest.mark.parametrize("B,batches", [(3, 4), (25, 1)])                 # 25 rows: two launches of the gather, 50 jobs
def test_fused_source_delivers_the_batch_of_the_two_entries(key, B, batches):
    fused = _producer({key: 1.0}, B)
    plain = _producer(None, B)
    assert fused.mix_mode == 1 and fused.vocoder_fft == P_FFT and fused._scratch is not None
    assert plain.slot_frames == 0 and plain._scratch is None and plain.gather_frames == plain.plane_frames and not plain.jobs().any()
    scratch_ptr, fell_back = fused._scratch.data_ptr(), 0
    for _ in range(batches):
        table, rates, jobs = fused.descriptors().copy(), fused.rates().copy(), fused.jobs().copy()
        assert jobs.shape == (B, 2, 4) and fused.jobs() is fused.jobs()                     # peeking does not advance
        ptable = plain.descriptors().copy()
        mix, tgt = fused()
        pmix, ptgt = plain()
        want_mix, want_tgt = _by_the_two_entries(fused, table, rates, jobs)
        assert torch.isfinite(mix).all() and torch.isfinite(tgt).all()
        assert np.array_equal(_bits(mix), _bits(want_mix)) and np.array_equal(_bits(tgt), _bits(want_tgt))
        has_job = jobs[:, :, 1] > 0
        if key == "pitch_shift":
            assert has_job.all() and rates.all() and set(rates.ravel().tolist()) <= {1, 2, 3, 4}
        else:
            assert not rates.any()
            for b, s in np.argwhere(~has_job):                           # fell back: the plain window, where it was
                assert table["start"][b, s] == ptable["start"][b, s] >= 3300      # (the short track)
                assert np.array_equal(_bits(tgt[s, b]), _bits(ptgt[s, b]))
                fell_back += 1
            for b in range(B):                                           # stems of one song: together
                assert has_job[b].all() or not has_job[b].any()
                assert (has_job[b].all() and (jobs[b, :, 1:] == jobs[b, 0, 1:]).all()) or np.array_equal(_bits(mix[b]), _bits(pmix[b]))
    assert fused._scratch.data_ptr() == scratch_ptr                      # allocated once
    assert key == "pitch_shift" or fell_back >= 1


def test_rows_that_do_not_take_pitch_shift_are_the_plain_rows():
    fused, plain = _producer({"pitch_shift": 0.5}, 3), _producer(None, 3)
    took = kept = 0
    for _ in range(6):
        jobs = fused.jobs().copy()
        mix, tgt = fused()
        pmix, ptgt = plain()
        for b in range(3):
            if jobs[b, :, 1].any():
                took += 1
                assert not np.array_equal(_bits(mix[b]), _bits(pmix[b]))
            else:
                kept += 1
                assert np.array_equal(_bits(mix[b]), _bits(pmix[b])) and np.array_equal(_bits(tgt[:, b]), _bits(ptgt[:, b]))
    assert took >= 3 and kept >= 3


def test_training_with_the_fused_producer_and_the_vocoder(tmp_path, monkeypatch):
    monkeypatch.setenv("WUN_NO_TUNE", "1")
    tmp = str(tmp_path)
    cfg = wun.get_config("baseline_stereo", num_layers=3, num_initial_filters=8, num_frames=40, batch_size=4, epoch_it=3,
                         worse_epochs=1, num_snippets_per_track=6, cache_size=8, model_base_dir=os.path.join(tmp, "ckpt"),
                         log_dir=os.path.join(tmp, "logs"), init_sup_sep_lr=1e-3, data_producer="fused",
                         augment={"pitch_shift": 0.5, "time_stretch": 0.5})
    rng = np.random.default_rng(1)
    tracks = [datasets.make_track({k: rng.uniform(-0.4, 0.4, (n, 2)).astype(np.float32) for k in cfg["source_names"]}, cfg)
              for n in (700, 800, 650)]
    make, made = validation._train_source(cfg, tracks, seed=5), []

    def source(trainer):                                                 # the deferred constructor, watched
        made.append(make(trainer))
        return made[0]
    source.needs_trainer = True
    training.train(cfg, "vocoder", batch_source=source)
    assert isinstance(made[0], datasets.FusedSnippetSource) and made[0].vocoder_fft == (2048, 512) and made[0].slot_frames > 0
    losses = [json.loads(l)["sep_loss"] for l in open(os.path.join(cfg["log_dir"], "vocoder", "train.jsonl"))]
    assert len(losses) == 3 and np.isfinite(losses).all()
