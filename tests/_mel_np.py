"""float64 oracle of the mel-scale terms of the spectral loss (include/wun.h: wun_mel_design, wun_op_mel_project,
wun_spectral_loss_mel), for the tests only.  Written from the definitions; it shares nothing with the kernels or
with the library's table builder.

Filterbank (HTK scale): mel(f) = 2595 log10(1 + f / 700); c[0 .. n_mels + 1] the frequencies of n_mels + 2 points equally spaced in
mel from mel(fmin) to mel(fmax), the two ends fmin and fmax themselves; f_k = k sample_rate / n_fft;
    W[b][k] = max(0, min((f_k - c[b]) / (c[b+1] - c[b]), (c[b+2] - f_k) / (c[b+2] - c[b+1])))       (times 2 / (c[b+2] - c[b]): area)
Terms on Pe = Me W^T and Pt = Mt W^T [R, F, n_mels], d = Pe - Pt, sg = sgn(d):
    mel_l1      mean |d|                                            dL / dPe = sg / (R F n_mels)
    log_mel_l1  mean |log(Pe + eps) - log(Pt + eps)|                sg / (Pe + eps) / (R F n_mels)
and dL / dMe = (dL / dPe) W, which joins the four linear-frequency terms' coefficient of (Re_e, Im_e) / Me (tests/_mrstft_np.py).
losses = the 2 + 5 nres slots of that oracle (L_j and the total with the mel terms in), then (mel_l1, log_mel_l1) per resolution.
The gradient takes the signs of both differences as arguments, so that a test can pin them to the device's fp32 decisions.
"""
import numpy as np
import torch

import _mrstft_np as mr
import _spectral_np as sp

MEL_TERMS = ("mel_l1", "log_mel_l1")


def hz_to_mel(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_to_hz(m):
    return 700.0 * (10.0 ** (np.asarray(m, dtype=np.float64) / 2595.0) - 1.0)


def corners(sample_rate, n_mels, fmin=0.0, fmax=None):
    fmax = sample_rate / 2.0 if not fmax else float(fmax)
    m0, m1 = hz_to_mel(fmin), hz_to_mel(fmax)
    c = mel_to_hz(m0 + (m1 - m0) * np.arange(n_mels + 2) / (n_mels + 1))
    c[0], c[-1] = fmin, fmax
    return c


def filterbank(n_fft, sample_rate, n_mels, fmin=0.0, fmax=None, norm=None):
    """W float64 [n_mels, K], not rounded."""
    c = corners(sample_rate, n_mels, fmin, fmax)
    f = np.arange(n_fft // 2 + 1, dtype=np.float64) * sample_rate / n_fft
    up = (f[None, :] - c[:-2, None]) / (c[1:-1] - c[:-2])[:, None]
    down = (c[2:, None] - f[None, :]) / (c[2:] - c[1:-1])[:, None]
    W = np.maximum(0.0, np.minimum(up, down))
    if norm in ("area", 1):
        W = W * (2.0 / (c[2:] - c[:-2]))[:, None]
    return W


def filterbank32(*a, **kw):
    """The definition's weights: float64, rounded once to float32."""
    return filterbank(*a, **kw).astype(np.float32)


def project(W, M):
    """P [.., n_mels] = M [.., K] W^T in float64."""
    return np.asarray(M, dtype=np.float64) @ np.asarray(W, dtype=np.float64).T


def adjoint(W, g):
    """q [.., K] = g [.., n_mels] W in float64."""
    return np.asarray(g, dtype=np.float64) @ np.asarray(W, dtype=np.float64)


def mel_terms(pe, pt, log_eps):
    pe, pt = np.asarray(pe), np.asarray(pt)
    d = (pe - pt).astype(np.float64)
    return np.abs(d).mean(), np.abs(np.log(pe.astype(np.float64) + log_eps) - np.log(pt.astype(np.float64) + log_eps)).mean()


def mel_weights(mel):
    return [float(mel["terms"].get(t, 0.0)) for t in MEL_TERMS]


def _mel_q(xp, W, pe, sg, wts, eps):
    """dL_j / dMe [R, F, K] of the mel terms, in the arrays' own precision."""
    g = xp.zeros_like(pe)
    if wts[0] > 0:
        g = g + wts[0] * sg
    if wts[1] > 0:
        g = g + wts[1] * sg / (pe + eps)
    return (g / pe.size) @ W


def loss_and_grad(out, tgt, resolutions, weights, mse_weight, terms, log_eps, sc_eps, mel, signs=None, mel_signs=None):
    """(losses [2 + 7 nres], grad [S, B, T, C]) in float64.  mel = {"W": [per resolution float32 [n_mels, K]], "terms": {..},
    "log_eps": e}.  signs / mel_signs: per resolution arrays used in place of sgn(Me - Mt) / sgn(Pe - Pt) in the gradient."""
    out, tgt = np.asarray(out, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    w, mw, me_eps = mr.term_weights(terms), mel_weights(mel), float(mel["log_eps"])
    S, nres = out.shape[0], len(resolutions)
    d = out - tgt
    mse = float(np.mean(d * d))
    g = mse_weight * 2.0 * d / d.size
    losses = np.zeros(2 + 7 * nres)
    losses[1] = mse
    total = mse_weight * mse
    xr, tr = sp.rows(out), sp.rows(tgt)
    T = xr.shape[1]
    for j, (n_fft, hop) in enumerate(resolutions):
        W = np.asarray(mel["W"][j], dtype=np.float64)
        re, im = sp.stft(xr, n_fft, hop)
        tre, tim = sp.stft(tr, n_fft, hop)
        me, mt = np.sqrt(re * re + im * im), np.sqrt(tre * tre + tim * tim)
        mag, lg, sc, _ = mr.mag_terms(me, mt, S, log_eps, sc_eps)
        cx = np.sqrt((re - tre) ** 2 + (im - tim) ** 2).mean()
        vals = [v if wt > 0 else 0.0 for v, wt in zip((mag, lg, sc, cx), w)]
        pe, pt = project(W, me), project(W, mt)
        mvals = [v if wt > 0 else 0.0 for v, wt in zip(mel_terms(pe, pt, me_eps), mw)]
        losses[2 + nres + 4 * j:2 + nres + 4 * j + 4] = vals
        losses[2 + 5 * nres + 2 * j:2 + 5 * nres + 2 * j + 2] = mvals
        losses[2 + j] = sum(wt * v for wt, v in zip(w, vals)) + sum(wt * v for wt, v in zip(mw, mvals))
        total += weights[j] * losses[2 + j]
        sg = np.sign(me - mt) if signs is None else np.asarray(signs[j], dtype=np.float64)
        msg = np.sign(pe - pt) if mel_signs is None else np.asarray(mel_signs[j], dtype=np.float64)
        D, N = mr.source_sums(me, mt, S)
        cre, cim = mr._coefficients(np, re, im, tre, tim, me, mt, sg, S, w, log_eps, sc_eps, D, N)
        q = _mel_q(np, W, pe, msg, mw, me_eps)
        live = me > 0
        safe = np.where(live, me, 1.0)
        cre = cre + np.where(live, q * re / safe, 0.0)
        cim = cim + np.where(live, q * im / safe, 0.0)
        cb, sb = sp.basis(n_fft)
        dframe = cre @ cb.T + cim @ sb.T
        g = g + sp.unrows(sp.overlap_add(dframe, T, hop) * weights[j], out.shape)
    losses[0] = total
    return losses, g


def loss_and_grad_fp32(out, tgt, resolutions, weights, mse_weight, terms, log_eps, sc_eps, mel, signs, mel_signs):
    """The same formulas in float32 with CPU matmuls and float32 means (D_s and N_s of sc in float64 from the fp32 d and Mt, as
    the definition has them): a second, independent fp32 computation whose distance from float64 is the yardstick of the
    GPU's.  (losses float32 [2 + 7 nres], grad float32 [S, B, T, C]); the gradient at the given signs."""
    f32 = np.float32
    out32, tgt32 = np.asarray(out, dtype=f32), np.asarray(tgt, dtype=f32)
    w, mw, me_eps = [f32(x) for x in mr.term_weights(terms)], [f32(x) for x in mel_weights(mel)], f32(mel["log_eps"])
    le = f32(log_eps)
    S, B, T, C = out32.shape
    nres = len(resolutions)
    d = out32 - tgt32
    mse = f32(np.mean(d * d, dtype=f32))
    g = d * f32(np.float64(f32(mse_weight)) * 2.0 / out32.size)
    losses = np.zeros(2 + 7 * nres, f32)
    losses[1] = mse
    total = f32(mse_weight) * mse
    rows32 = lambda x: np.ascontiguousarray(x.transpose(0, 1, 3, 2).reshape(S * B * C, T))  # noqa: E731
    mm = lambda a, b: (torch.from_numpy(np.ascontiguousarray(a)) @ torch.from_numpy(np.ascontiguousarray(b))).numpy()  # noqa: E731
    xr, tr = rows32(out32), rows32(tgt32)
    for j, (n_fft, hop) in enumerate(resolutions):
        W = np.asarray(mel["W"][j], dtype=f32)
        cb, sb = (b.astype(f32) for b in sp.basis(n_fft))
        fr, ft = (np.ascontiguousarray(sp.frame_view(x, n_fft, hop)) for x in (xr, tr))
        re, im, tre, tim = mm(fr, cb), mm(fr, sb), mm(ft, cb), mm(ft, sb)
        me, mt = np.sqrt(re * re + im * im), np.sqrt(tre * tre + tim * tim)
        D, N = mr.source_sums(me, mt, S)
        vals = [f32(np.mean(np.abs(me - mt), dtype=f32)), f32(np.mean(np.abs(np.log(me + le) - np.log(mt + le)), dtype=f32)),
                f32(np.sqrt(D / (N + np.float64(f32(sc_eps)))).mean()),
                f32(np.mean(np.sqrt((re - tre) ** 2 + (im - tim) ** 2), dtype=f32))]
        vals = [v if wt > 0 else f32(0) for v, wt in zip(vals, w)]
        pe, pt = mm(me, W.T), mm(mt, W.T)
        mvals = [f32(np.mean(np.abs(pe - pt), dtype=f32)), f32(np.mean(np.abs(np.log(pe + me_eps) - np.log(pt + me_eps)), dtype=f32))]
        mvals = [v if wt > 0 else f32(0) for v, wt in zip(mvals, mw)]
        losses[2 + nres + 4 * j:2 + nres + 4 * j + 4] = vals
        losses[2 + 5 * nres + 2 * j:2 + 5 * nres + 2 * j + 2] = mvals
        lj = f32(0)
        for wt, v in list(zip(w, vals)) + list(zip(mw, mvals)):
            lj = f32(lj + wt * v)
        losses[2 + j] = lj
        total = f32(total + f32(weights[j]) * lj)
        sg, msg = np.asarray(signs[j], dtype=f32), np.asarray(mel_signs[j], dtype=f32)
        cre, cim = mr._coefficients(np, re, im, tre, tim, me, mt, sg, S, w, le, np.float64(f32(sc_eps)), D, N)
        gm = np.zeros_like(pe)
        if mw[0] > 0:
            gm = gm + mw[0] * msg
        if mw[1] > 0:
            gm = gm + mw[1] * msg / (pe + me_eps)
        q = mm((gm / f32(pe.size)).astype(f32), W)
        live = me > 0
        safe = np.where(live, me, f32(1))
        cre = (cre + np.where(live, q * re / safe, f32(0))).astype(f32)
        cim = (cim + np.where(live, q * im / safe, f32(0))).astype(f32)
        dframe = mm(cre, cb.T) + mm(cim, sb.T)
        g = g + sp.unrows(sp.overlap_add(dframe, T, hop) * f32(weights[j]), out32.shape)
    losses[0] = total
    return losses, g.astype(f32)
