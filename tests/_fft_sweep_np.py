"""Shapes, references, verdicts and mutants of the FFT sweep (tests/test_fft_sweep_host.py, tests/test_gpu_fft_sweep.py;
DESIGN.md 5.13): every kernel body of wun_fft.hip at every transform size, n_fft = 64 .. 8192.

No oracle of its own: the float64 references are the family tests' (_fft_np, _mrstft_fft_np, _griffin_lim_np, _vocoder_np,
_specunet_backward_np), every one a numpy.fft call.  This module adds

    GEOMETRY    FftGeom<LOGM> of wun_fft.hip restated per size, and `workgroups`: which frame rows share a workgroup
    cases       per size the four shapes below, chosen for what the per-body code around the FFT core does with that geometry
    verdicts    the rules the GPU test applies, as functions of (result, reference), so that the host test can apply the very
                same rules to mutant references and see them fail
    mutants     the subtle defects a body's index arithmetic can have, evaluated in float64

    case  rows (S, B, C)  hop        framing          F   what it reaches
    A     3 (1, 3, 1)     n_fft / 4  lead 0, whole    5   15 frame rows: no multiple of FPW up to 1024 (a part-filled last
                                                          workgroup), a row boundary inside a workgroup at 128 .. 1024
    B     2 (1, 1, 2)     3 n_fft/4  lead 0, whole    3   stereo (channel stride 2), the reference's 1024 / 768 ratio: no power of two
    C     1 (1, 1, 1)     n_fft / 4  lead 0, T=n_fft  1   one valid frame slot, FPW - 1 idle ones
    D     2 (1, 1, 2)     n_fft / 4  centred, T = 5   4   a track shorter than a frame (the centred entries only)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fft_np as fo  # noqa: E402
import _mrstft_fft_np as mf  # noqa: E402
import _spectral_np as sp  # noqa: E402

SIZES = [64, 128, 256, 512, 1024, 2048, 4096, 8192]
BLOCK = 256
# n_fft -> (LOGM, lanes per frame, frames per workgroup, butterflies per lane, stages, radix-2 tail, RESULT image): DESIGN.md 5.13
GEOMETRY = {
    64: (5, 8, 32, 1, 3, True, 0),
    128: (6, 16, 16, 1, 3, False, 0),
    256: (7, 32, 8, 1, 4, True, 1),
    512: (8, 64, 4, 1, 4, False, 1),
    1024: (9, 128, 2, 1, 5, True, 0),
    2048: (10, 256, 1, 1, 5, False, 0),
    4096: (11, 256, 1, 2, 6, True, 1),
    8192: (12, 256, 1, 4, 6, False, 1),
}
CASE_NAMES = ["A", "B", "C", "D"]
_CACHE = {}
_ADJOINT = mf.adjoint


def geometry(n_fft):
    """FftGeom<log2(n_fft / 2)> by its formulas (wun_fft.hip)."""
    M = n_fft // 2
    logm = M.bit_length() - 1
    tpf = min(M // 4, BLOCK)
    stages = (logm + 1) // 2
    return (logm, tpf, BLOCK // tpf, M // 4 // tpf, stages, bool(logm & 1), (stages - 1) & 1)


def fpw(n_fft):
    return GEOMETRY[n_fft][2]


def workgroups(n_fft, rows, F):
    """Frame row m = r F + f of a whole transform is slot m mod FPW of workgroup m // FPW: [[(r, f), ..], ..]."""
    w = fpw(n_fft)
    slots = [(r, f) for r in range(rows) for f in range(F)]
    return [slots[i:i + w] for i in range(0, len(slots), w)]


def case(n_fft, name):
    """{"shape": (S, B, C), "R", "T", "hop", "lead", "F", "centered"}."""
    hop = n_fft // 4
    if name == "A":
        shape, F, lead, centered = (1, 3, 1), 5, 0, False
        T = n_fft + (F - 1) * hop
    elif name == "B":
        hop = 3 * n_fft // 4
        shape, F, lead, centered = (1, 1, 2), 3, 0, False
        T = n_fft + (F - 1) * hop
    elif name == "C":
        shape, F, lead, centered, T = (1, 1, 1), 1, 0, False, n_fft
    else:
        shape, T, centered = (1, 1, 2), 5, True
        lead, F = fo.framing(T, n_fft, hop, True)
    return {"n_fft": n_fft, "name": name, "shape": shape, "R": shape[0] * shape[1] * shape[2], "T": T, "hop": hop, "lead": lead,
            "F": F, "centered": centered}


def cases(n_fft, centred_entry):
    """A, B, C, and D where the entry takes the centred framing."""
    return [case(n_fft, n) for n in (CASE_NAMES if centred_entry else CASE_NAMES[:3])]


def gl_case(c):
    """The case for Griffin-Lim: the same rows, hop and F -- the geometry the case is chosen for -- with a lead and a length at
    which every sample divides by a window-square sum above 0.2.  The one-step rule asks that of its inputs
    (test_griffin_lim_host.one_step_check: a pointwise bound below 1e-2 max |y|); at lead 0 the first samples divide by w^2
    near 1e-8, and from n_fft 2048 up the rule's own condition refuses such inputs.
      A  the centred framing's longest track with 5 frames, T = n_fft / 2: every sample under four frames
      B  hop = 3 n_fft / 4 leaves a window-square sum of 2 sin^4(pi / 8) = 0.043 in the middle of each overlap, too little for the
         condition from 4096 up; lead = 63 n_fft / 64 and T = 17 n_fft / 32 keep both overlaps' middles outside the track: frame 1
         carries it, the frames 0 and 2 reach its first and last n_fft / 64 samples with window values up to 0.0024 -- a
         misplaced frame still shows at 1e-2 of the signal, a thousand times the bound
      C  the middle quarter of the one frame"""
    n_fft = c["n_fft"]
    g = dict(c)
    if c["name"] == "A":
        g.update(lead=n_fft - c["hop"], T=2 * c["hop"])
    elif c["name"] == "B":
        g.update(lead=63 * n_fft // 64, T=34 * n_fft // 64)
    elif c["name"] == "C":
        g.update(lead=3 * n_fft // 8, T=n_fft // 4)
    ws = fo.window_sums(g["T"], g["F"], n_fft, g["hop"], g["lead"])
    assert ws.min() > 0.2 and (g["F"] - 1) * g["hop"] - g["lead"] < g["T"]      # (and the last frame holds samples)
    return g


def _seed(c, salt):
    return 7919 * c["n_fft"] + 31 * CASE_NAMES.index(c["name"]) + salt


def signal(c):
    """Audio [S, B, T, C] of amplitude 0.3 with its float64 transform, beta and the float32 stand-in -- computed once, never changed."""
    key = ("sig", c["n_fft"], c["name"])
    if key not in _CACHE:
        n_fft, hop, lead, F = c["n_fft"], c["hop"], c["lead"], c["F"]
        x = (0.3 * np.random.RandomState(_seed(c, 1)).randn(*(c["shape"][:2] + (c["T"], c["shape"][2])))).astype(np.float32)
        xr = sp.rows(x)
        re, im = fo.stft(xr, n_fft, hop, lead, F)
        r32, i32 = fo.stft_fp32(xr, n_fft, hop, lead, F)
        _CACHE[key] = {"x": x, "xr": xr, "re": re, "im": im, "r32": r32, "i32": i32, "beta": fo.beta(xr, n_fft, hop, lead, F),
                       "e32": max(np.abs(r32 - re).max(), np.abs(i32 - im).max())}
    return _CACHE[key]


def spectra(c):
    """Random float32 spectra [R, F, K], their float64 inverse, its bound and the float32 stand-in (test_gpu_fft's recipe)."""
    key = ("spec", c["n_fft"], c["name"])
    if key not in _CACHE:
        n_fft, hop, lead, F, T = c["n_fft"], c["hop"], c["lead"], c["F"], c["T"]
        rng = np.random.RandomState(_seed(c, 2))
        re = rng.randn(c["R"], F, n_fft // 2 + 1).astype(np.float32)
        im = rng.randn(c["R"], F, n_fft // 2 + 1).astype(np.float32)
        want = fo.istft(re, im, T, n_fft, hop, lead)
        ref_im = im.astype(np.float64).copy()
        ref_im[..., 0] = ref_im[..., -1] = 0.0               # (the definition does not read them; the bound must not count them)
        y32 = fo.istft_fp32(re, im, T, n_fft, hop, lead).astype(np.float64)
        _CACHE[key] = {"re": re, "im": im, "want": want, "y32": y32,
                       "bound": fo.istft_bound(re.astype(np.float64), ref_im, want, T, n_fft, hop, lead),
                       "e32": np.abs(y32 - want).max()}
    return _CACHE[key]


def loss_pair(c):
    """Estimates and targets [S, B, T, C] (randn, as _mrstft_fft_np.case) in the layout test_gpu_spectral_fft's helpers take."""
    key = ("loss", c["n_fft"], c["name"])
    if key not in _CACHE:
        assert not c["centered"]
        rng = np.random.RandomState(_seed(c, 3))
        shape = c["shape"][:2] + (c["T"], c["shape"][2])
        _CACHE[key] = {"out": rng.randn(*shape).astype(np.float32), "tgt": rng.randn(*shape).astype(np.float32),
                       "res": [(c["n_fft"], c["hop"])], "w": [1.0], "log_eps": 1e-3, "S": c["shape"][0], "oracle": {},
                       "gpu_mags": None, "gemm_mags": None}
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------- the definitions, O(n^2)
def dft_forward(frames, n_fft):
    """(Re, Im) of X[k] = sum_n w[n] frame[n] exp(-2 pi i n k / n_fft), k = 0 .. n_fft / 2, by the matrix (wun_fft.hip's header)."""
    cb, sb = sp.basis(n_fft)
    return frames @ cb, frames @ sb


def dft_inverse(re, im, n_fft):
    """frame[n] = (w[n] / n_fft) sum_k c_k (Re[k] cos(2 pi n k / N) - Im[k] sin(2 pi n k / N)), c = 1 at the bins 0 and N / 2, else 2."""
    cb, sb = sp.basis(n_fft)
    c = fo.ora.c_k(n_fft) / n_fft
    return (re * c) @ cb.T + (im * c) @ sb.T


def dft_adjoint(cre, cim, n_fft):
    """dframe[n] = w[n] sum_{k = 0 .. N / 2} cre[k] cos(2 pi n k / N) - cim[k] sin(2 pi n k / N): every bin once, unscaled."""
    cb, sb = sp.basis(n_fft)
    return cre @ cb.T + cim @ sb.T


# ---------------------------------------------------------------------------------------------------- verdicts
def forward_verdict(gre, gim, ref):
    """Every element within beta, max error <= 8 x the stand-in's, Im of the bins 0 and n_fft / 2 exactly 0.
    -> (passes, {figure: (observed, tolerance)})."""
    gre, gim = np.asarray(gre, np.float64), np.asarray(gim, np.float64)
    b = np.maximum(ref["beta"][:, :, None], 1e-300)
    err = np.maximum(np.abs(gre - ref["re"]), np.abs(gim - ref["im"]))
    edges = bool((gim[..., 0] == 0).all() and (gim[..., -1] == 0).all())
    finite = bool(np.isfinite(gre).all() and np.isfinite(gim).all())
    figs = {"max err / beta": ((err / b).max(), 1.0), "max err / stand-in's": (err.max() / ref["e32"], 8.0)}
    return finite and edges and all(o <= t for o, t in figs.values()), figs


def inverse_verdict(got, ref):
    """Every sample within istft_bound (exactly 0 where it is 0) and max error <= 8 x the stand-in's."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref["want"])
    live = ref["bound"] > 0
    dead_ok = bool((err[~live] == 0).all())
    figs = {"max err / bound": ((err[live] / ref["bound"][live]).max() if live.any() else 0.0, 1.0),
            "max err / stand-in's": (err.max() / ref["e32"], 8.0)}
    return bool(np.isfinite(got).all()) and dead_ok and all(o <= t for o, t in figs.values()), figs


def magnitude_verdict(got, x, n_fft, hop):
    """test_gpu_spectral_fft's magnitude rule: |got - M| <= sqrt(2) beta + 2^-22 M."""
    x64 = np.asarray(x, np.float64)
    want = mf.magnitude(x64, n_fft, hop)
    got = np.asarray(got, np.float64)
    figs = {"err / bound": ((np.abs(got - want) / mf.magnitude_bound(x64, n_fft, hop, want)).max(), 1.0)}
    return got.shape == want.shape and bool(np.isfinite(got).all()) and figs["err / bound"][0] <= 1.0, figs


def gradient(ref, signs, adjoint=None, fp32=False):
    """The one-term loss's gradient at pinned signs: _mrstft_fft_np's float64 formula (or its float32 yardstick), optionally
    with another adjoint transform in place of the reference's."""
    args = (ref["out"], ref["tgt"], ref["res"], ref["w"], 0.0, {"mag_l1": 1.0}, np.float32(ref["log_eps"]), 1.0)
    if fp32:
        return mf.grad_fp32_fft(*(args + (signs,)))
    keep = mf.adjoint
    try:
        if adjoint is not None:
            mf.adjoint = adjoint
        return mf.loss_and_grad(*args, signs=signs)[1]
    finally:
        mf.adjoint = keep


def gradient_verdict(got, g64, g32):
    """test_gpu_spectral_fft._check_gradient's rule: max err / max |g64| <= 8 x the float32 yardstick's."""
    scale = np.abs(g64).max()
    e32 = np.abs(np.asarray(g32, np.float64) - g64).max() / scale
    e = np.abs(np.asarray(got, np.float64) - g64).max() / scale
    return bool(scale > 0 and e <= 8 * e32), {"err / max |g64|": (e, 8 * e32)}


# ---------------------------------------------------------------------------------------------------- mutants (float64)
def _windowed(c, xr=None, window=None):
    ref = signal(c)
    w = sp.window(c["n_fft"]) if window is None else window
    return fo.frames_of(ref["xr"] if xr is None else xr, c["n_fft"], c["hop"], c["lead"], c["F"]) * w


def _rfft(fr):
    z = np.fft.rfft(fr, axis=-1)
    re, im = np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)
    im[..., 0] = im[..., -1] = 0.0
    return re, im


def split_step(fr, conj=True):
    """wun_fft.hip's real transform: z[m] = y[2m] + i y[2m+1], Z = FFT_M(z), E = (Z[k] + conj Z[M-k]) / 2,
    O = (Z[k] - conj Z[M-k]) / 2i, X[k] = E + W_N^k O, k = 0 .. M.  conj=False leaves the conjugate out."""
    N = fr.shape[-1]
    M = N // 2
    Z = np.fft.fft(fr[..., 0::2] + 1j * fr[..., 1::2], axis=-1)
    k = np.arange(M + 1)
    Zk, Zm = Z[..., k % M], Z[..., (M - k) % M]
    if conj:
        Zm = np.conj(Zm)
    X = 0.5 * (Zk + Zm) + np.exp(-2j * np.pi * k / N) * (Zk - Zm) / 2j
    re, im = np.ascontiguousarray(X.real), np.ascontiguousarray(X.imag)
    im[..., 0] = im[..., -1] = 0.0
    return re, im


def forward_mutants(c):
    """name -> (re, im) float64 of a subtly wrong forward transform of signal(c); only the mutants that apply to the case."""
    ref = signal(c)
    out = {}
    re, im = ref["re"].copy(), ref["im"].copy()
    im[..., 0] = im[..., -1] = 0.0
    dropped = re.copy()
    dropped[..., -1] = 0.0
    out["bin M dropped"] = (dropped, im)
    im0 = im.copy()
    im0[..., 0] = 1e-30
    out["Im of bin 0 non-zero"] = (re, im0)
    out["conjugate missing in the split step"] = split_step(_windowed(c), conj=False)
    if c["R"] > 1:
        xr = ref["xr"]
        out["frames of row r + 1 from row r's samples"] = _rfft(_windowed(c, xr=np.concatenate([xr[:1], xr[:-1]])))
    out["window index shifted by one"] = _rfft(_windowed(c, window=np.roll(sp.window(c["n_fft"]), 1)))
    return out


def inverse_mutants(c):
    """name -> y [R, T] float64 of a subtly wrong inverse of spectra(c)."""
    ref = spectra(c)
    n_fft, hop, lead, T = c["n_fft"], c["hop"], c["lead"], c["T"]
    z = np.asarray(ref["re"], np.float64) + 1j * np.asarray(ref["im"], np.float64)
    z[..., 0] = z[..., 0].real
    z[..., -1] = z[..., -1].real
    raw = np.fft.irfft(z, n=n_fft, axis=-1)
    return {"inverse scaled by 2 / n_fft": fo._finish(2.0 * raw * sp.window(n_fft), T, hop, lead, np.float64),
            "window index shifted by one": fo._finish(raw * np.roll(sp.window(n_fft), 1), T, hop, lead, np.float64)}


def adjoint_edges_twice(cre, cim, n_fft):
    """The adjoint with the bins 0 and n_fft / 2 counted twice, as the bins between them are by irfft."""
    z = np.asarray(cre, np.float64) + 1j * np.asarray(cim, np.float64)
    z[..., 0] = 2.0 * z[..., 0].real
    z[..., -1] = 2.0 * z[..., -1].real
    return _ADJOINT(z.real, z.imag, n_fft)
