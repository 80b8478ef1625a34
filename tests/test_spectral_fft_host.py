"""CPU-only checks of the spectral loss's FFT path (include/wun.h: wun_stft_magnitude_fft, wun_spectral_fft_scratch_floats,
wun_spectral_loss_fft, wun_spectral_terms_fft_scratch_floats, wun_spectral_loss_terms_fft; SpectralLoss(transform="fft");
DESIGN.md 5.16): the numpy.fft oracle tests/_mrstft_fft_np.py against the dense-basis oracles it restates, what the GPU test
assumes of its cases, every refusal of the new entries before any GPU work, their scratch formula, and the Python keyword.
The device path is checked against that oracle in tests/test_gpu_spectral_fft.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mrstft_fft_np as fo  # noqa: E402
import _mrstft_np as mr  # noqa: E402
import _spectral_np as ora  # noqa: E402
from _observed import record  # noqa: E402
from wave_u_net_amd import _lib, spectral, training  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wun_stft_magnitude_fft", "wun_spectral_fft_scratch_floats", "wun_spectral_loss_fft",
         "wun_spectral_terms_fft_scratch_floats", "wun_spectral_loss_terms_fft")
INVALID, UNSUPPORTED = -1, -2
P = 0x1000                  # a non-null "device pointer": every call below must fail before any GPU work reads it
ALL = {"mag_l1": 0.7, "log_mag_l1": 0.4, "sc": 1.3, "complex_l1": 0.6}
TERM_SETS = {"mag_l1": {"mag_l1": 1.0}, "log_mag_l1": {"log_mag_l1": 1.0}, "sc": {"sc": 1.0}, "complex_l1": {"complex_l1": 1.0},
             "sc_log": {"sc": 1.0, "log_mag_l1": 1.0}, "all": ALL}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _terms(mag_l1=1.0, log_mag_l1=0.0, sc=0.0, complex_l1=0.0, log_eps=1e-3, sc_eps=1.0):
    return _lib.WunSpectralTerms(mag_l1, log_mag_l1, sc, complex_l1, log_eps, sc_eps)


def test_declared_exported_and_documented(lib):
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in NAMES:
        assert name in doc and name in design, name
    for op, gemm in (("magnitude", "wun_stft_magnitude"), ("loss", "wun_spectral_loss"), ("loss_terms", "wun_spectral_loss_terms")):
        assert spectral._ENTRIES["gemm"][op] == gemm and spectral._ENTRIES["fft"][op] == gemm + "_fft"
    assert spectral._ENTRIES["gemm"]["loss_scratch"] == "wun_spectral_scratch_floats"
    assert spectral._ENTRIES["fft"]["loss_scratch"] == "wun_spectral_fft_scratch_floats"
    assert spectral._ENTRIES["fft"]["loss_terms_scratch"] == "wun_spectral_terms_fft_scratch_floats"
    # a twin has its sibling's argument list
    for name in NAMES:
        sib = name.replace("_fft", "")
        assert _lib._SIGS[name] == _lib._SIGS[sib], name


# ---------------------------------------------------------------------------------------------------- the oracle itself
@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("name", sorted(TERM_SETS))
def test_oracle_is_the_dense_oracle(name, pinned):
    """The numpy.fft restatement against _mrstft_np's dense basis at n_fft <= 1024: losses and gradient to 1e-10 relative, with
    float64's own signs and with pinned ones (random: any sign pattern must give the same gradient through both)."""
    rng = np.random.RandomState(31)
    out, tgt = rng.randn(2, 2, 1300, 2), rng.randn(2, 2, 1300, 2)
    res, w, mw, le, se = [(64, 48), (256, 100), (1024, 256)], [1.0, 0.5, 0.25], 0.3, 1e-3, 1.0
    signs = None
    if pinned:
        signs = [np.sign(rng.randn(8, ora.num_frames(1300, n, h), n // 2 + 1)) for n, h in res]
    args = (out, tgt, res, w, mw, TERM_SETS[name], le, se)
    l0, g0 = mr.loss_and_grad(*args, signs=signs)
    l1, g1 = fo.loss_and_grad(*args, signs=signs)
    el, eg = np.abs(l1 - l0).max() / np.abs(l0).max(), np.abs(g1 - g0).max() / np.abs(g0).max()
    record("spectral_fft_host::test_oracle_is_the_dense_oracle[%s-%s]" % (name, pinned), "losses, gradient", max(el, eg), 1e-10)
    assert el <= 1e-10 and eg <= 1e-10
    if name == "mag_l1":                                     # ... and the one-term oracle of wun_spectral_loss
        l2, g2 = ora.loss_and_grad(out, tgt, res, w, mw, signs=signs)
        assert np.abs(l1[:2 + len(res)] - l2).max() <= 1e-10 * np.abs(l2).max()
        assert np.abs(g1 - g2).max() <= 1e-10 * np.abs(g2).max()


@pytest.mark.parametrize("name", sorted(TERM_SETS))
def test_fp32_yardstick_is_close_to_float64(name):
    """grad_fp32_fft is the same formula in fp32: its distance from float64 is fp32 rounding, far below the gradient's scale
    (the dense stand-in's figure is printed beside it)."""
    rng = np.random.RandomState(32)
    out, tgt = rng.randn(2, 2, 700, 1).astype(np.float32), rng.randn(2, 2, 700, 1).astype(np.float32)
    res, w = [(64, 16), (512, 128)], [1.0, 0.5]
    signs = [np.sign(fo.magnitude(out, n, h) - fo.magnitude(tgt, n, h)) for n, h in res]
    args = (out, tgt, res, w, 0.25, TERM_SETS[name], float(np.float32(0.0625)), 1.0)
    _, g64 = fo.loss_and_grad(*args, signs=signs)
    e_fft = np.abs(fo.grad_fp32_fft(*args, signs).astype(np.float64) - g64).max() / np.abs(g64).max()
    e_mm = np.abs(mr.grad_fp32(*args, signs).astype(np.float64) - g64).max() / np.abs(g64).max()
    record("spectral_fft_host::test_fp32_yardstick[%s]" % name, "dense e32", e_mm, 1e-4)
    record("spectral_fft_host::test_fp32_yardstick[%s]" % name, "fft e32", e_fft, 1e-4)
    assert 0 < e_fft < 1e-4


@pytest.mark.parametrize("name", sorted(fo.CASES))
def test_log_eps_of_the_cases(name):
    """What tests/test_gpu_spectral_fft.py assumes of a case, before any GPU call: log_eps is the smallest power of two (1e-3 at
    n_fft 64) with every magnitude bound delta <= log_eps / 4, so that the log term's bound is finite and not vacuous."""
    ref = fo.case(name)
    worst = 0.0
    for n_fft, hop in ref["res"]:
        for x in (ref["out"], ref["tgt"]):
            x64 = x.astype(np.float64)
            worst = max(worst, fo.magnitude_bound(x64, n_fft, hop, fo.magnitude(x64, n_fft, hop)).max())
    le = ref["log_eps"]
    record("spectral_fft_host::test_log_eps_of_the_cases[%s]" % name, "max delta / (log_eps / 4)", worst / (le / 4), 1.0)
    assert worst <= le / 4
    if max(n for n, _ in ref["res"]) == 64:
        assert le == 1e-3
    else:
        assert le == 2.0 ** round(np.log2(le)) and worst > le / 8           # the next smaller power of two would not do


@pytest.mark.parametrize("name", sorted(fo.CASES))
def test_yardstick_signs_stay_inside_the_tie_rule(name):
    """The GPU test pins the gradient's signs to sgn(Me - Mt) of the device's float32 magnitudes and asserts that such a sign
    differs from float64's only where the magnitudes tie within their bounds.  The float32 yardstick's own signs satisfy that
    condition on these inputs: the oracle alone stays inside it."""
    ref = fo.case(name)
    for n_fft, hop in ref["res"]:
        sg = np.sign(fo.magnitude_fp32(ref["out"], n_fft, hop) - fo.magnitude_fp32(ref["tgt"], n_fft, hop)).astype(np.float64)
        d64, tie = fo.tie(ref["out"].astype(np.float64), ref["tgt"].astype(np.float64), n_fft, hop)
        flipped = sg != np.sign(d64)
        record("spectral_fft_host::test_yardstick_signs[%s]" % name, "signs differing from float64 (count)", flipped.sum(), sg.size)
        assert not (flipped & ~tie).any()


# ---------------------------------------------------------------------------------------------------- the entries' refusals
def _loss(lib, entry="wun_spectral_loss_terms_fft", S=2, B=3, T=200, Cn=2, res=((64, 48),), weights=(1.0,), mse_weight=0.0, nres=None,
          terms=None, null_terms=False, outputs=P, targets=P, losses=P, scratch=P, tables=None, null_tables=False):
    n = max(len(res), 1)
    tabs = None if null_tables else (C.c_void_p * n)(*(tables if tables is not None else [P] * n))
    head = (outputs, targets, S, B, T, Cn, mse_weight, len(res) if nres is None else nres, (C.c_int32 * n)(*[r[0] for r in res]),
            (C.c_int32 * n)(*[r[1] for r in res]), (C.c_float * n)(*(list(weights) + [1.0] * n)[:n]))
    tail = (tabs, None, losses, scratch, None)
    if "terms" not in entry:
        return getattr(lib, entry)(*(head + tail))
    tw = None if null_terms else C.byref(terms if terms is not None else _terms())
    return getattr(lib, entry)(*(head + (tw,) + tail))


@pytest.mark.parametrize("entry", ["wun_spectral_loss_fft", "wun_spectral_loss_terms_fft"])
def test_loss_argument_errors(lib, entry):
    """The siblings' refusals, order and codes (tests/test_spectral_host.py, tests/test_mrstft_host.py), every one before any
    GPU work: the pointers are not device memory and there may be no device at all.  Only the n_fft list is longer."""
    for kw in ({"outputs": None}, {"targets": None}, {"losses": None}, {"scratch": None}, {"null_tables": True}, {"tables": [None]}):
        assert _loss(lib, entry, **kw) == INVALID, kw
    for kw in ({"S": 0}, {"B": 0}, {"Cn": 0}, {"Cn": 3}, {"S": -1}):
        assert _loss(lib, entry, **kw) == INVALID, kw
    assert _loss(lib, entry, T=63) == INVALID
    assert _loss(lib, entry, res=((4096, 1024),), T=4095) == INVALID and b"fewer frames than n_fft" in lib.wun_last_error()
    assert _loss(lib, entry, res=((64, 48), (8192, 2048)), weights=(1.0, 1.0), T=8191) == INVALID
    assert _loss(lib, entry, res=((64, 0),)) == INVALID and _loss(lib, entry, res=((64, 65),)) == INVALID
    assert _loss(lib, entry, res=((4096, 4097),), T=10000) == INVALID
    assert _loss(lib, entry, nres=-1) == INVALID
    assert _loss(lib, entry, res=((64, 48),) * 9, weights=(1.0,) * 9) == INVALID
    for bad in (-1.0, float("nan"), float("inf")):
        assert _loss(lib, entry, weights=(bad,)) == INVALID, bad
        assert _loss(lib, entry, mse_weight=bad) == INVALID, bad
    for bad in (32, 96, 16384, 0, 6000):
        assert _loss(lib, entry, res=((bad, 16),), T=40000) == UNSUPPORTED, bad
        assert b"n_fft" in lib.wun_last_error() and b"8192" in lib.wun_last_error() and entry.encode() in lib.wun_last_error()
    assert _loss(lib, entry, res=((16384, 96),), T=40000) == UNSUPPORTED           # n_fft before the hop
    assert _loss(lib, entry, outputs=None, res=((96, 16),)) == INVALID and b"null argument" in lib.wun_last_error()
    if "terms" in entry:
        assert _loss(lib, entry, null_terms=True) == INVALID and b"terms" in lib.wun_last_error()
        for kw in ({"sc": -1.0}, {"log_eps": 0.0}, {"sc_eps": float("nan")}, {"mag_l1": float("inf")}):
            assert _loss(lib, entry, terms=_terms(**kw)) == INVALID, kw
        assert _loss(lib, entry, res=((96, 16),), T=10000, terms=_terms(log_eps=0.0)) == UNSUPPORTED    # the existing checks first
    # the GEMM siblings keep their list: 4096 is still refused there
    assert _loss(lib, entry.replace("_fft", ""), res=((4096, 1024),), T=10000) == UNSUPPORTED
    assert b"2048" in lib.wun_last_error()


def test_magnitude_argument_errors(lib):
    def mag(name="wun_stft_magnitude_fft", x=P, S=2, B=1, T=10000, Cn=1, n_fft=4096, hop=1024, table=P, mags=P):
        return getattr(lib, name)(x, S, B, T, Cn, n_fft, hop, table, mags, None)
    assert mag(x=None) == INVALID and mag(table=None) == INVALID and mag(mags=None) == INVALID
    assert mag(S=0) == INVALID and mag(Cn=3) == INVALID and mag(T=0) == INVALID
    for bad in (16384, 96, 32, 100):
        assert mag(n_fft=bad, T=40000) == UNSUPPORTED, bad
    assert mag(hop=0) == INVALID and mag(hop=4097) == INVALID
    assert mag(T=4095) == INVALID and mag(n_fft=8192, hop=2048, T=8191) == INVALID
    assert mag(name="wun_stft_magnitude") == UNSUPPORTED                            # the GEMM entry still stops at 2048


def _scratch(lib, fft=True, S=2, B=3, T=200, Cn=2, res=((64, 48),), nres=None, terms=None, null_terms=False, with_terms=True):
    n = max(len(res), 1)
    args = (S, B, T, Cn, len(res) if nres is None else nres, (C.c_int32 * n)(*[r[0] for r in res]), (C.c_int32 * n)(*[r[1] for r in res]))
    if not with_terms:
        return (lib.wun_spectral_fft_scratch_floats if fft else lib.wun_spectral_scratch_floats)(*args)
    tw = None if null_terms else C.byref(terms if terms is not None else _terms())
    return (lib.wun_spectral_terms_fft_scratch_floats if fft else lib.wun_spectral_terms_scratch_floats)(*(args + (tw,)))


@pytest.mark.parametrize("with_terms", [False, True])
def test_scratch_argument_errors_and_size(lib, with_terms):
    s = lambda **kw: _scratch(lib, with_terms=with_terms, **kw)  # noqa: E731
    assert s(S=0) == INVALID and s(T=63) == INVALID and s(nres=9) == INVALID and s(Cn=3) == INVALID
    assert s(res=((64, 65),)) == INVALID and s(res=((64, 0),)) == INVALID and s(res=((4096, 0),), T=10000) == INVALID
    for bad in (16384, 96, 32):
        assert s(res=((bad, 16),), T=40000) == UNSUPPORTED, bad
    assert s(res=((4096, 1024),), T=4095) == INVALID
    if with_terms:
        assert s(null_terms=True) == INVALID
        assert s(res=((100, 10),), null_terms=True) == UNSUPPORTED                  # the existing checks first
        assert s(terms=_terms(log_eps=0.0)) == INVALID
    # the GEMM entries still refuse 4096; the new ones accept 4096 and 8192
    assert s(fft=False, res=((4096, 1024),), T=10000) == UNSUPPORTED
    # the documented size, identical to the siblings' formula: per resolution R F (4 K + n_fft) floats, then the float64 partials
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    for (n_fft, hop, T) in ((64, 48, 200), (2048, 512, 5000), (4096, 1024, 9000), (8192, 2048, 20001)):
        R, S = 12, 2
        F, K = 1 + (T - n_fft) // hop, n_fft // 2 + 1
        E = R * F * K
        mse_parts, parts, src_parts = cdiv(R * T, 1024), cdiv(E, 1024), cdiv(E // S, 1024)
        base = R * F * (4 * K + n_fft)
        kw = dict(res=((n_fft, hop),), T=T)
        assert s(**kw) == base + 2 * (mse_parts + parts) + 2, (n_fft, hop)
        if n_fft <= 2048:
            assert s(**kw) == s(fft=False, **kw)
        if with_terms:
            assert s(terms=_terms(1, 1, 1, 1), **kw) == base + 2 * E + 2 * (mse_parts + 3 * parts + 2 * S * src_parts + 3 * S) + 2
            assert s(terms=_terms(0, 0, 1, 0), **kw) == base + 2 * (mse_parts + 2 * S * src_parts + 3 * S) + 2
    assert s(res=()) == 2 * cdiv(12 * 200, 1024) + 2
    # the Python front end follows the entry in use
    shape = (2, 3, 9000, 2)
    terms = {"sc": 1, "complex_l1": 1} if with_terms else None
    want = s(res=((4096, 1024),), T=9000, **({"terms": _terms(0, 0, 1, 1)} if with_terms else {}))
    assert spectral.SpectralLoss([(4096, 1024)], terms=terms, transform="fft").scratch_floats(shape) == want > 0
    with pytest.raises(NotImplementedError):
        spectral.SpectralLoss([(4096, 1024)], terms=terms).scratch_floats(shape)    # "gemm" stays the default and keeps its list
    with pytest.raises(NotImplementedError):
        spectral.SpectralLoss([(16384, 1024)], terms=terms, transform="fft").scratch_floats((2, 3, 40000, 2))
    with pytest.raises(ValueError):
        spectral.SpectralLoss([(4096, 1024)], terms=terms, transform="fft").scratch_floats((2, 3, 4095, 2))


# ---------------------------------------------------------------------------------------------------- the Python front end
def test_python_front_end_transform():
    with pytest.raises(ValueError):
        spectral.SpectralLoss([(64, 48)], transform="dct")
    with pytest.raises(ValueError):
        spectral.SpectralLoss.from_config({"resolutions": [[64, 48]], "transform": "dct"})
    with pytest.raises(ValueError):
        spectral.SpectralLoss.multi_resolution(transform="FFT")
    with pytest.raises(ValueError):
        spectral.entry("dct", "loss")
    with pytest.raises(ValueError):
        spectral.SpectralLoss.from_config({"resolutions": [[64, 48]], "transform": "fft", "transfrom": "fft"})     # unknown keys still raise
    loss = spectral.SpectralLoss.from_config({"resolutions": [[4096, 1024]], "transform": "fft", "terms": {"sc": 1}, "log_eps": 4.0})
    assert loss.transform == "fft" and loss.resolutions == [(4096, 1024)] and loss.log_eps == 4.0
    assert spectral.SpectralLoss.from_config({"resolutions": [[64, 48]]}).transform == "gemm"
    assert spectral.SpectralLoss([(64, 48)]).transform == "gemm" and spectral.SpectralLoss.multi_resolution().transform == "gemm"
    m = spectral.SpectralLoss.multi_resolution(transform="fft")
    assert m.transform == "fft" and m.resolutions == [(512, 128), (1024, 256), (2048, 512)]
    assert m.terms == {"mag_l1": 0.0, "log_mag_l1": 1.0, "sc": 1.0, "complex_l1": 0.0}
    m = spectral.SpectralLoss.multi_resolution("fft", resolutions=[(4096, 1024), (8192, 2048)])
    assert m.resolutions == [(4096, 1024), (8192, 2048)] and m.weights == [1.0, 1.0]
    # the Trainer's spec and model_config["spectral_loss"] pass the key through
    assert training.SpectralLoss.from_config({"resolutions": [[4096, 1024]], "transform": "fft"}).transform == "fft"


class _Lib(object):
    """A stand-in library that records which entries are reached and answers every count with 7."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a):
            self.calls.append(name)
            return 7 if name.endswith("scratch_floats") else 0
        return fn


@pytest.mark.parametrize("transform, suffix", [("gemm", ""), ("fft", "_fft")])
def test_entries_are_routed_by_the_transform(monkeypatch, transform, suffix):
    """scratch_floats and run reach the transform's entries and no other (no GPU: the library is a recorder)."""
    fake = _Lib()
    monkeypatch.setattr(_lib, "load", lambda: fake)
    scr = {"": ("wun_spectral_scratch_floats", "wun_spectral_terms_scratch_floats"),
           "_fft": ("wun_spectral_fft_scratch_floats", "wun_spectral_terms_fft_scratch_floats")}[suffix]
    plain = spectral.SpectralLoss([(64, 48)], transform=transform)
    multi = spectral.SpectralLoss.multi_resolution(transform=transform)
    assert plain.scratch_floats((2, 3, 200, 2)) == 7 and multi.scratch_floats((2, 3, 5000, 2)) == 7
    assert fake.calls == [scr[0], scr[1]]
    for op, name in (("loss", "wun_spectral_loss" + suffix), ("loss_terms", "wun_spectral_loss_terms" + suffix),
                     ("magnitude", "wun_stft_magnitude" + suffix)):
        fn, table = spectral.entry(transform, op)
        del fake.calls[:]
        fn()
        assert fake.calls == [name]
        assert table is (spectral._fft_table if transform == "fft" else spectral._table)
