"""float64 oracle of the four-term spectral loss (include/wun.h: wun_spectral_loss_terms), for the tests only.

Per resolution j, with E = Re_e + i Im_e and T the STFTs of estimates and targets (tests/_spectral_np.py: the transform, the
rows r = (s * B + b) * C + c, so source s owns the rows [s B C, (s + 1) B C)), Me = |E|, Mt = |T|, d = Me - Mt, sg = sgn(d):
    mag_l1      mean |d|                                                coefficient of (Re_e, Im_e): sg / Me
    log_mag_l1  mean |log(Me + log_eps) - log(Mt + log_eps)|            sg / (Me + log_eps) / Me
    sc          mean_s sqrt(D_s / (N_s + sc_eps)), D_s = sum d^2, N_s = sum Mt^2 over the source's bins
                                                                        d / (sqrt(D_s) sqrt(N_s + sc_eps)) / S / Me
    complex_l1  mean |E - T|                                            (a, b) / |E - T|, a = Re_e - Re_t, b = Im_e - Im_t
every coefficient 0 where its denominator is.  L_j = sum_t terms[t] * term_t(j); total = mse_weight * MSE + sum_j weights[j] L_j.
losses = [total, MSE, L_0 .., then (mag_l1, log_mag_l1, sc, complex_l1) of resolution 0, of resolution 1, ..]; a term whose
weight is 0 is reported as 0.  The gradient takes the signs as an argument (as _spectral_np.loss_and_grad), so that a test
can pin them to the decisions the GPU made in fp32.
"""
import numpy as np
import torch

import _spectral_np as sp

TERMS = ("mag_l1", "log_mag_l1", "sc", "complex_l1")


def term_weights(terms):
    return [float(terms.get(t, 0.0)) for t in TERMS]


def source_sums(me, mt, S):
    """(D_s, N_s) float64 [S] of magnitudes [R, F, K] (any float type: the squares are formed in float64)."""
    me, mt = np.asarray(me), np.asarray(mt)
    d = (me - mt).astype(np.float64).reshape(S, -1)          # (fp32 inputs: the difference in fp32, as the device takes it)
    return (d * d).sum(1), (mt.astype(np.float64).reshape(S, -1) ** 2).sum(1)


def mag_terms(me, mt, S, log_eps, sc_eps):
    """(mag_l1, log_mag_l1, sc, SC_s [S]) in float64 from magnitudes [R, F, K]; fp32 magnitudes give d in fp32."""
    me, mt = np.asarray(me), np.asarray(mt)
    d = (me - mt).astype(np.float64)
    me64, mt64 = me.astype(np.float64), mt.astype(np.float64)
    D, N = source_sums(me, mt, S)
    scs = np.sqrt(D / (N + sc_eps))
    return np.abs(d).mean(), np.abs(np.log(me64 + log_eps) - np.log(mt64 + log_eps)).mean(), scs.mean(), scs


def _coefficients(xp, re, im, tre, tim, me, mt, sg, S, w, log_eps, sc_eps, D, N):
    """(cre, cim) of one resolution BEFORE the resolution's weight: mean terms over me.size, sc as it is.  xp: numpy-like
    namespace working in the arrays' own precision; D, N: [S] float64."""
    wm, wl, ws, wc = w
    E = me.size
    live = me > 0
    safe = xp.where(live, me, xp.ones_like(me))
    q = xp.zeros_like(me)
    if wm > 0:
        q = q + wm * sg
    if wl > 0:
        q = q + wl * sg / (me + log_eps)
    q = q / E
    if ws > 0:
        ok = D > 0
        fac = np.where(ok, 1.0 / (np.sqrt(np.where(ok, D, 1.0)) * np.sqrt(N + sc_eps)) / S, 0.0)
        fac = np.repeat(fac, E // S).reshape(me.shape).astype(me.dtype)
        q = q + ws * (me - mt) * fac
    cre = xp.where(live, q * re / safe, xp.zeros_like(me))
    cim = xp.where(live, q * im / safe, xp.zeros_like(me))
    if wc > 0:
        a, b = re - tre, im - tim
        m = xp.sqrt(a * a + b * b)
        on = m > 0
        ms = xp.where(on, m, xp.ones_like(m))
        cre = cre + xp.where(on, wc / E * a / ms, xp.zeros_like(m))
        cim = cim + xp.where(on, wc / E * b / ms, xp.zeros_like(m))
    return cre, cim


def loss_and_grad(out, tgt, resolutions, weights, mse_weight, terms, log_eps, sc_eps, signs=None):
    """(losses [2 + 5 nres], grad [S, B, T, C]) in float64.  signs: per resolution an [R, F, K] array used in place of
    sgn(Me - Mt) in the gradient (None: float64's own)."""
    out = np.asarray(out, dtype=np.float64)
    tgt = np.asarray(tgt, dtype=np.float64)
    w = term_weights(terms)
    S = out.shape[0]
    nres = len(resolutions)
    d = out - tgt
    mse = float(np.mean(d * d))
    g = mse_weight * 2.0 * d / d.size
    losses = np.zeros(2 + 5 * nres)
    losses[1] = mse
    total = mse_weight * mse
    xr, tr = sp.rows(out), sp.rows(tgt)
    T = xr.shape[1]
    for j, (n_fft, hop) in enumerate(resolutions):
        re, im = sp.stft(xr, n_fft, hop)
        tre, tim = sp.stft(tr, n_fft, hop)
        me, mt = np.sqrt(re * re + im * im), np.sqrt(tre * tre + tim * tim)
        mag, lg, sc, _ = mag_terms(me, mt, S, log_eps, sc_eps)
        cx = np.sqrt((re - tre) ** 2 + (im - tim) ** 2).mean()
        vals = [v if wt > 0 else 0.0 for v, wt in zip((mag, lg, sc, cx), w)]
        losses[2 + nres + 4 * j:2 + nres + 4 * j + 4] = vals
        losses[2 + j] = sum(wt * v for wt, v in zip(w, vals))
        total += weights[j] * losses[2 + j]
        sg = np.sign(me - mt) if signs is None else np.asarray(signs[j], dtype=np.float64)
        D, N = source_sums(me, mt, S)
        cre, cim = _coefficients(np, re, im, tre, tim, me, mt, sg, S, w, log_eps, sc_eps, D, N)
        cb, sb = sp.basis(n_fft)
        dframe = cre @ cb.T + cim @ sb.T
        g = g + sp.unrows(sp.overlap_add(dframe, T, hop) * weights[j], out.shape)
    losses[0] = total
    return losses, g


def grad_fp32(out, tgt, resolutions, weights, mse_weight, terms, log_eps, sc_eps, signs):
    """The pinned-sign gradient formula in float32 with CPU matmuls (D_s and N_s summed in float64 from the fp32 d and Mt, as
    the definition has them): a second, independent fp32 computation whose distance from float64 is the yardstick of the GPU's
    (returns float32 [S, B, T, C])."""
    out32 = np.asarray(out, dtype=np.float32)
    tgt32 = np.asarray(tgt, dtype=np.float32)
    w = term_weights(terms)
    g = (out32 - tgt32) * np.float32(np.float64(np.float32(mse_weight)) * 2.0 / out32.size)
    S, B, T, C = out32.shape
    rows32 = lambda x: np.ascontiguousarray(x.transpose(0, 1, 3, 2).reshape(S * B * C, T))  # noqa: E731
    xr, tr = rows32(out32), rows32(tgt32)
    for j, (n_fft, hop) in enumerate(resolutions):
        cb, sb = (b.astype(np.float32) for b in sp.basis(n_fft))
        fr, ft = (np.ascontiguousarray(sp.frame_view(x, n_fft, hop)) for x in (xr, tr))
        mm = lambda a, b: (torch.from_numpy(a) @ torch.from_numpy(b)).numpy()  # noqa: E731
        re, im, tre, tim = mm(fr, cb), mm(fr, sb), mm(ft, cb), mm(ft, sb)
        me, mt = np.sqrt(re * re + im * im), np.sqrt(tre * tre + tim * tim)
        sg = np.asarray(signs[j], dtype=np.float32)
        D, N = source_sums(me, mt, S)
        cre, cim = _coefficients(np, re, im, tre, tim, me, mt, sg, S, [np.float32(x) for x in w], np.float32(log_eps),
                                 np.float64(np.float32(sc_eps)), D, N)
        dframe = mm(cre.astype(np.float32), np.ascontiguousarray(cb.T)) + mm(cim.astype(np.float32), np.ascontiguousarray(sb.T))
        g = g + sp.unrows(sp.overlap_add(dframe, T, hop) * np.float32(weights[j]), out32.shape)
    return g.astype(np.float32)


def torch_total(out, tgt, resolutions, weights, mse_weight, terms, log_eps, sc_eps):
    """(losses, total tensor) of float64 torch tensors under torch.autograd: the definitions restated on torch.stft."""
    w = term_weights(terms)
    S, B, T, C = out.shape
    nres = len(resolutions)
    mse = ((out - tgt) ** 2).mean()
    total = mse_weight * mse
    losses = [None, mse] + [None] * (5 * nres)
    rows = lambda x: x.permute(0, 1, 3, 2).reshape(S * B * C, T)  # noqa: E731
    for j, (n_fft, hop) in enumerate(resolutions):
        win = torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
        ze, zt = (torch.stft(rows(x), n_fft, hop_length=hop, win_length=n_fft, window=win, center=False, onesided=True,
                             return_complex=True) for x in (out, tgt))
        me, mt = ze.abs(), zt.abs()
        mag = (me - mt).abs().mean()
        lg = (torch.log(me + log_eps) - torch.log(mt + log_eps)).abs().mean()
        D = ((me - mt) ** 2).reshape(S, -1).sum(1)
        N = (mt ** 2).reshape(S, -1).sum(1)
        sc = torch.sqrt(D / (N + sc_eps)).mean()
        cx = (ze - zt).abs().mean()
        vals = [v if wt > 0 else torch.zeros((), dtype=torch.float64) for v, wt in zip((mag, lg, sc, cx), w)]
        lj = sum(wt * v for wt, v in zip(w, vals))
        for t in range(4):
            losses[2 + nres + 4 * j + t] = vals[t]
        losses[2 + j] = lj
        total = total + weights[j] * lj
    losses[0] = total
    return torch.stack([torch.as_tensor(l, dtype=torch.float64) for l in losses]), total
