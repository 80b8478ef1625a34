"""The post-filters of libwun.so (include/wun.h: wun_mask_filter, wun_wiener_filter): the estimates of
a track are masked against the mixture's own STFT, so they share the mixture's phase and sum back to the mixture.

    f = SoftMaskFilter(n_fft=2048, hop=512, power=2, eps=1e-10)
    out = f.apply(mix, estimates)                      # mix [n, C], estimates [S, n, C] -> [S, n, C]
    evaluate.separate_track(cfg, sep, audio, sr, postfilter=f)      # or model_config["postfilter"] = {"n_fft": 2048, ...}
    w = WienerFilter(n_fft=2048, hop=512, iterations=1)             # or postfilter={"kind": "wiener", "iterations": 1}
    g = SoftMaskFilter(n_fft=4096, hop=1024, transform="fft")       # the transforms through an FFT: n_fft up to 8192 (5.13)

Per channel, in the centred framing (frame f starts at f hop - (n_fft - hop), zeros outside the track):
X = STFT(mix), E_s = STFT(est_s), A_s = |E_s|^power, mask_s = (A_s + eps / S) / (sum_j A_j + eps), out_s = ISTFT(mask_s X).
Tensors on the GPU go through wun_mask_filter (no host sync; scratch cached per shape, tables shared with spectral.py); CPU
tensors through a plain torch float32 implementation of the same definition (numpy stand-in separators, host tests).
transform="gemm" (the default) runs the transforms as GEMMs against the [2, n_fft, K] table and stops at n_fft = 2048;
transform="fft" runs them as FFTs (wun_mask_filter_fft / wun_wiener_filter_fft; on the CPU torch.fft in float32) up to 8192.

WienerFilter starts from those masked spectra y_s and runs `iterations` EM steps of a local Gaussian model over the C channels
together (the header's definition): v_s = mean_c |y_s|^2, R_s[k] = sum_f y_s y_s^H / (em_eps + sum_f v_s) over the whole track,
Cxx = sum_s v_s R_s + sqrt(em_eps) I, y_s <- v_s R_s Cxx^-1 X, in float64 with the spectra kept in float32.  There is no global
rescaling of the mix (norbert's max_abs): the float64 algebra does not need it.  iterations = 0 is the soft mask, bit for bit.
"""
import numpy as np
import torch

from . import _lib, spectral

MAX_SOURCES = 8
MAX_ITERATIONS = 4
_KEYS = ("n_fft", "hop", "power", "eps", "transform")
MAX_N_FFT = {"gemm": 2048, "fft": 8192}


class SoftMaskFilter(object):
    """ValueError / NotImplementedError at construction for what wun_mask_filter refuses: n_fft must be a power of two in
    64..2048 (64..8192 with transform="fft"), hop a power of two of at most n_fft / 2 (every sample's window-square sum is then at least 0.5), power 1
    (magnitude ratio mask) or 2 (power ratio mask, single-channel Wiener), eps finite and positive."""
    _KEYS = _KEYS            # what from_config accepts; a subclass adds its own

    def __init__(self, n_fft=2048, hop=512, power=2, eps=1e-10, transform="gemm"):
        if transform not in MAX_N_FFT:
            raise ValueError("transform must be \"gemm\" or \"fft\", got %r" % (transform,))
        self.transform = transform
        for what, v in (("n_fft", n_fft), ("hop", hop), ("power", power)):
            if isinstance(v, bool) or int(v) != v:
                raise ValueError("%s must be an integer, got %r" % (what, v))
        self.n_fft, self.hop, self.power, self.eps = int(n_fft), int(hop), int(power), float(eps)
        if self.n_fft < 64 or self.n_fft > MAX_N_FFT[transform] or self.n_fft & (self.n_fft - 1):
            raise NotImplementedError("n_fft must be a power of two in 64..%d%s, got %d" % (
                MAX_N_FFT[transform], "" if transform == "fft" else " (up to 8192 with transform=\"fft\")", self.n_fft))
        if self.hop < 1 or self.hop & (self.hop - 1) or self.hop > self.n_fft // 2:
            raise ValueError("hop must be a power of two, at most n_fft / 2, got %d" % self.hop)
        if self.power not in (1, 2):
            raise ValueError("power must be 1 or 2, got %d" % self.power)
        if not (self.eps > 0.0 and np.isfinite(self.eps) and np.float32(self.eps) > 0):
            raise ValueError("eps must be finite and positive in float32, got %r" % (eps,))
        self._scratch = {}       # (S, n, C, device) -> float32 scratch of wun_mask_filter_scratch_floats

    @classmethod
    def from_config(cls, spec):
        """model_config["postfilter"]: None, an instance of the class, True (the defaults) or a dict with any of the class's
        _KEYS: `n_fft`, `hop`, `power`, `eps`, `transform`, and for WienerFilter `iterations`, `em_eps`."""
        if spec is None or isinstance(spec, cls):
            return spec
        if spec is True:
            return cls()
        if not isinstance(spec, dict):
            raise ValueError("postfilter must be None, True or a dict with %s, got %r" % (", ".join(cls._KEYS), spec))
        unknown = set(spec) - set(cls._KEYS)
        if unknown:
            raise ValueError("postfilter: unknown keys %s" % sorted(unknown))
        return cls(**spec)

    def spec(self):
        d = {"n_fft": self.n_fft, "hop": self.hop, "power": self.power, "eps": self.eps}
        if self.transform == "fft":          # (the default stays out: the spec of a default filter is what it always was)
            d["transform"] = "fft"
        return d

    def scratch_floats(self, S, n, Cn):
        return spectral.count(self.transform, "mask_filter_scratch", int(S), int(n), int(Cn), self.n_fft, self.hop)

    def run(self, mix, estimates, out, scratch):
        """wun_mask_filter (transform="fft": wun_mask_filter_fft) on the caller's buffers (contiguous float32 device tensors)."""
        S, n, Cn = (int(v) for v in estimates.shape)
        dev = estimates.device
        entry, table = spectral.entry(self.transform, "mask_filter")
        with torch.cuda.device(dev):
            _lib.check(entry(
                mix.data_ptr(), estimates.data_ptr(), S, n, Cn, self.n_fft, self.hop, self.power, self.eps,
                table(self.n_fft, dev).data_ptr(), out.data_ptr(), scratch.data_ptr(), _lib.stream(dev)))

    def apply(self, mix, estimates):
        """mix [n, C], estimates [S, n, C] (tensors of one device, or arrays) -> the filtered estimates, float32 [S, n, C] on
        that device."""
        mix = mix if torch.is_tensor(mix) else torch.from_numpy(np.ascontiguousarray(np.asarray(mix, dtype=np.float32)))
        estimates = estimates if torch.is_tensor(estimates) else torch.from_numpy(
            np.ascontiguousarray(np.asarray(estimates, dtype=np.float32)))
        if mix.dim() != 2 or estimates.dim() != 3 or tuple(estimates.shape[1:]) != tuple(mix.shape):
            raise ValueError("mix must be [n, C] and estimates [S, n, C], got %s and %s" % (tuple(mix.shape), tuple(estimates.shape)))
        if mix.device != estimates.device:
            raise ValueError("mix on %s, estimates on %s" % (mix.device, estimates.device))
        mix, estimates = mix.to(torch.float32).contiguous(), estimates.to(torch.float32).contiguous()
        if not estimates.is_cuda:
            return self._apply_cpu(mix, estimates)
        S, n, Cn = (int(v) for v in estimates.shape)
        key = (S, n, Cn, str(estimates.device))
        if key not in self._scratch:
            self._scratch[key] = torch.empty(self.scratch_floats(S, n, Cn), dtype=torch.float32, device=estimates.device)
        out = torch.empty_like(estimates)
        self.run(mix, estimates, out, self._scratch[key])
        return out

    def _apply_cpu(self, mix, estimates):
        """The definition in torch float32 on the CPU: framed matmuls against the library's fp32 table (transform="fft":
        torch.fft.rfft / irfft of the frames times the float32 window), the window-square sums in float64."""
        S, n, Cn = (int(v) for v in estimates.shape)
        if S < 1 or n < 1 or Cn not in (1, 2):
            raise ValueError("S < 1, n < 1 or C not 1 or 2")
        if S > MAX_SOURCES:
            raise NotImplementedError("more than %d sources" % MAX_SOURCES)
        n_fft, hop = self.n_fft, self.hop
        lead = n_fft - hop
        F = -(-(n + lead) // hop)
        total = (F - 1) * hop + n_fft
        fft = self.transform == "fft"
        if fft:
            win = torch.from_numpy(spectral.fft_design(n_fft)[2])                # [n_fft], the table's float32 window
        else:
            tab = torch.from_numpy(spectral.design(n_fft))
            cb, sb = tab[0], tab[1]                                              # [n_fft, K]

        def transform(x):                                                        # [..., n, C] -> Re, Im [..., C, F, K]
            xp = torch.zeros(x.shape[:-2] + (Cn, total), dtype=torch.float32)
            xp[..., lead:lead + n] = x.transpose(-1, -2)
            fr = xp.unfold(-1, n_fft, hop)
            if fft:
                z = torch.fft.rfft(fr * win, dim=-1)
                return z.real.contiguous(), z.imag.contiguous()
            return fr @ cb, fr @ sb

        xre, xim = transform(mix)
        ere, eim = transform(estimates)
        a = ere * ere + eim * eim
        if self.power == 1:
            a = torch.sqrt(a)
        eps = torch.tensor(self.eps, dtype=torch.float32)
        den = a[0]
        for s in range(1, S):                                                    # j ascending
            den = den + a[s]
        den = den + eps
        mask = (a + eps / torch.tensor(float(S), dtype=torch.float32)) / den
        ck = torch.full((n_fft // 2 + 1,), 2.0 / n_fft, dtype=torch.float32)
        ck[0] = ck[-1] = 1.0 / n_fft
        yre, yim = self._refine_cpu(mask * xre, mask * xim, xre, xim)
        if fft:                                                                  # (irfft ignores Im of the bins 0 and n_fft / 2)
            frames = torch.fft.irfft(torch.complex(yre, yim), n=n_fft, dim=-1) * win
        else:
            frames = (yre * ck) @ cb.t() + (yim * ck) @ sb.t()                   # [S, C, F, n_fft]
        y = torch.zeros((S, Cn, total), dtype=torch.float32)
        w = 0.5 - 0.5 * torch.cos(2.0 * np.pi * torch.arange(n_fft, dtype=torch.float64) / n_fft)
        ws = torch.zeros(total, dtype=torch.float64)
        for f in range(F):                                                       # ascending f
            y[..., f * hop:f * hop + n_fft] += frames[..., f, :]
            ws[f * hop:f * hop + n_fft] += w * w
        live = ws >= 1e-8
        y = torch.where(live, y / torch.where(live, ws, torch.ones_like(ws)).to(torch.float32), torch.zeros_like(y))
        return y[..., lead:lead + n].transpose(-1, -2).contiguous()

    def _refine_cpu(self, yre, yim, xre, xim):
        """What lies between the mask and the inverse: nothing here."""
        return yre, yim


class WienerFilter(SoftMaskFilter):
    """The multichannel Wiener filter (wun_wiener_filter): SoftMaskFilter's settings, `iterations` in 0..4 EM steps and their
    regulariser `em_eps` (finite and positive in float32)."""
    _KEYS = _KEYS + ("iterations", "em_eps")

    def __init__(self, n_fft=2048, hop=512, power=2, eps=1e-10, iterations=1, em_eps=1e-10, transform="gemm"):
        SoftMaskFilter.__init__(self, n_fft, hop, power, eps, transform)
        if isinstance(iterations, bool) or int(iterations) != iterations:
            raise ValueError("iterations must be an integer, got %r" % (iterations,))
        self.iterations, self.em_eps = int(iterations), float(em_eps)
        if not 0 <= self.iterations <= MAX_ITERATIONS:
            raise ValueError("iterations must lie in 0..%d, got %d" % (MAX_ITERATIONS, self.iterations))
        if not (self.em_eps > 0.0 and np.isfinite(self.em_eps) and np.float32(self.em_eps) > 0 and np.isfinite(np.float32(self.em_eps))):
            raise ValueError("em_eps must be finite and positive in float32, got %r" % (em_eps,))

    def spec(self):
        return dict(SoftMaskFilter.spec(self), kind="wiener", iterations=self.iterations, em_eps=self.em_eps)

    def scratch_floats(self, S, n, Cn):
        return spectral.count(self.transform, "wiener_filter_scratch", int(S), int(n), int(Cn), self.n_fft, self.hop, self.iterations)

    def run(self, mix, estimates, out, scratch):
        """wun_wiener_filter (transform="fft": wun_wiener_filter_fft) on the caller's buffers (contiguous float32 device tensors)."""
        S, n, Cn = (int(v) for v in estimates.shape)
        dev = estimates.device
        entry, table = spectral.entry(self.transform, "wiener_filter")
        with torch.cuda.device(dev):
            _lib.check(entry(
                mix.data_ptr(), estimates.data_ptr(), S, n, Cn, self.n_fft, self.hop, self.power, self.eps, self.iterations,
                self.em_eps, table(self.n_fft, dev).data_ptr(), out.data_ptr(), scratch.data_ptr(), _lib.stream(dev)))

    def _refine_cpu(self, yre, yim, xre, xim):
        """The EM steps in float64 on float32 spectra: y [S, C, F, K], X [C, F, K]; closed forms for C = 1 and 2."""
        S, Cn = int(yre.shape[0]), int(yre.shape[1])
        eps = float(np.float32(self.em_eps))
        sq = float(np.sqrt(eps))
        x = torch.complex(xre.double(), xim.double())
        y = torch.complex(yre.double(), yim.double())
        for _ in range(self.iterations):
            p = y.real * y.real + y.imag * y.imag                                # [S, C, F, K]
            v = p[:, 0] if Cn == 1 else 0.5 * (p[:, 0] + p[:, 1])                # [S, F, K]
            den = (eps + v.sum(1))[:, None, :]                                   # [S, 1, K]
            r00 = p[:, 0].sum(1, keepdim=True) / den
            if Cn == 1:
                g = v * r00
                y = (g / (g.sum(0) + sq))[:, None] * x
            else:
                r11 = p[:, 1].sum(1, keepdim=True) / den
                r01 = (y[:, 0] * y[:, 1].conj()).sum(1, keepdim=True) / den
                a, d, b = (v * r00).sum(0) + sq, (v * r11).sum(0) + sq, (v * r01).sum(0)
                det = a * d - (b.real * b.real + b.imag * b.imag)
                z0, z1 = (d * x[0] - b * x[1]) / det, (a * x[1] - b.conj() * x[0]) / det
                y = torch.stack([v * (r00 * z0 + r01 * z1), v * (r01.conj() * z0 + r11 * z1)], 1)
            y = y.to(torch.complex64).to(torch.complex128)                       # spectra are stored as float32
        return y.real.to(torch.float32), y.imag.to(torch.float32)


KINDS = {"softmask": SoftMaskFilter, "wiener": WienerFilter}


def from_config(spec):
    """model_config["postfilter"] / the postfilter= option: None or an instance of either class passes through; True is the
    soft mask's defaults; a dict goes to the class its `kind` names ("softmask", the default, or "wiener") without that key."""
    if spec is None or isinstance(spec, SoftMaskFilter):
        return spec
    if not isinstance(spec, dict):
        return SoftMaskFilter.from_config(spec)
    spec = dict(spec)
    kind = spec.pop("kind", "softmask")
    if not isinstance(kind, str) or kind not in KINDS:
        raise ValueError("postfilter: kind must be one of %s, got %r" % (", ".join(sorted(KINDS)), kind))
    return KINDS[kind].from_config(spec)
