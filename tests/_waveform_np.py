"""Float64 numpy oracle of the waveform losses (include/wun.h: wun_waveform_loss), restating the definitions.

Audio is [S, B, Tout, C]; N = S B Tout C.  A row is one (s, b): R = S B rows, r = s B + b, the n = Tout C floats of that excerpt,
all channels together.  d = e - t.
    mse     mean over N of d^2                      gradient  w 2 d / N
    l1      mean over N of |d|                      gradient  w sgn(d) / N, sgn(0) = 0
    per row sum e, sum t, sum ee, sum tt, sum et, sum dd; with zero_mean mu_e = sum e / n, mu_t = sum t / n and
            See = max(sum ee - sum e mu_e, 0), Stt = max(sum tt - sum t mu_t, 0), Set = sum et - sum e mu_t,
            Dd = max(sum dd - (sum e - sum t)^2 / n, 0); without it mu = 0 and the raw sums.  e' = e - mu_e, t' = t - mu_t, d' = e' - t'
    si_sdr  P = Set^2 / (Stt + eps), Nn = max(See - P, 0), SI_r = 10 log10((P + eps) / (Nn + eps)); term -(1 / R) sum_r SI_r
            gradient A_r e' + B_r t', A_r = 2 k w / (R (Nn + eps)), B_r = -(w k / R) (2 Set / (Stt + eps)) (1 / (P + eps) + 1 / (Nn + eps))
    snr     SNR_r = 10 log10((Stt + eps) / (Dd + eps)); term -(1 / R) sum_r SNR_r;  gradient G_r d', G_r = 2 k w / (R (Dd + eps))
    k = 10 / ln 10; the clamps are constants of the gradient (the closed forms at the clamped values).
    total = sum_t w_t term_t; a term of weight 0 is reported as 0.
losses [5 + 2 S]: total, the unweighted mse, l1, si_sdr, snr, then the mean SI_r per source (dB) and the mean SNR_r per source."""
import numpy as np

TERMS = ("mse", "l1", "si_sdr", "snr")
K = 10.0 / np.log(10.0)


def row_stats(out, tgt, eps, zero_mean):
    """Per row [R]: a dict of mu_e, mu_t, See, Stt, Set, Dd, P, Nn, SI, SNR in float64."""
    S, B = out.shape[:2]
    e = np.asarray(out, np.float64).reshape(S * B, -1)
    t = np.asarray(tgt, np.float64).reshape(S * B, -1)
    n = e.shape[1]
    d = e - t
    se, st = e.sum(1), t.sum(1)
    see, stt, set_, sdd = (e * e).sum(1), (t * t).sum(1), (e * t).sum(1), (d * d).sum(1)
    if zero_mean:
        mue, mut = se / n, st / n
        See = np.maximum(see - se * mue, 0.0)
        Stt = np.maximum(stt - st * mut, 0.0)
        Set = set_ - se * mut
        Dd = np.maximum(sdd - (se - st) ** 2 / n, 0.0)
    else:
        mue, mut = np.zeros_like(se), np.zeros_like(st)
        See, Stt, Set, Dd = see, stt, set_, sdd
    P = Set * Set / (Stt + eps)
    Nn = np.maximum(See - P, 0.0)
    SI = 10.0 * np.log10((P + eps) / (Nn + eps))
    SNR = 10.0 * np.log10((Stt + eps) / (Dd + eps))
    return {"mu_e": mue, "mu_t": mut, "See": See, "Stt": Stt, "Set": Set, "Dd": Dd, "P": P, "Nn": Nn, "SI": SI, "SNR": SNR, "n": n}


def loss_and_grad(out, tgt, terms, eps=1e-8, zero_mean=True, parts=False):
    """(losses float64 [5 + 2 S], gradient float64 of out's shape).  parts=True: also a dict of the gradient's three parts
    ("mse", "l1", "v": the row terms' A e' + B t' + G d') and the row statistics."""
    out, tgt = np.asarray(out, np.float64), np.asarray(tgt, np.float64)
    S, B = out.shape[:2]
    R, N = S * B, out.size
    w = {t: float(terms.get(t, 0.0)) for t in TERMS}
    d = out - tgt
    losses = np.zeros(5 + 2 * S)
    g_mse, g_l1, g_v = np.zeros_like(out), np.zeros_like(out), np.zeros_like(out)
    if w["mse"] > 0:
        losses[1] = (d * d).sum() / N
        g_mse = w["mse"] * 2.0 * d / N
    if w["l1"] > 0:
        losses[2] = np.abs(d).sum() / N
        g_l1 = w["l1"] * np.sign(d) / N
    st = row_stats(out, tgt, eps, zero_mean)
    if w["si_sdr"] > 0 or w["snr"] > 0:
        e = out.reshape(R, -1) - st["mu_e"][:, None]
        t = tgt.reshape(R, -1) - st["mu_t"][:, None]
        v = np.zeros_like(e)
        if w["si_sdr"] > 0:
            A = 2.0 * K * w["si_sdr"] / (R * (st["Nn"] + eps))
            Bc = -(w["si_sdr"] * K / R) * (2.0 * st["Set"] / (st["Stt"] + eps)) * (1.0 / (st["P"] + eps) + 1.0 / (st["Nn"] + eps))
            v = v + A[:, None] * e + Bc[:, None] * t
            losses[3] = -st["SI"].sum() / R
            losses[5:5 + S] = st["SI"].reshape(S, B).mean(1)
        if w["snr"] > 0:
            G = 2.0 * K * w["snr"] / (R * (st["Dd"] + eps))
            v = v + G[:, None] * (e - t)
            losses[4] = -st["SNR"].sum() / R
            losses[5 + S:5 + 2 * S] = st["SNR"].reshape(S, B).mean(1)
        g_v = v.reshape(out.shape)
    losses[0] = sum(w[t] * losses[1 + i] for i, t in enumerate(TERMS))
    g = g_mse + g_l1 + g_v
    if parts:
        return losses, g, {"mse": g_mse, "l1": g_l1, "v": g_v, "rows": st}
    return losses, g
