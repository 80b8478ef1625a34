"""Float64 references of the elementwise family (wave-u-net_amd/csrc/wun_elementwise.hip: 2x upsampling and its adjoint, the
learned-interpolation weight gradient, the output head with its loss and gradients, the [B, T, C] -> NCW layout change) and of
the two fused forms in the split-K epilogue.

Two layers:
  * `*_ref`: the ORACLE's own functions (oracle/waveunet_torch.py: upsample_linear, upsample_learned, conv1d_tf, audio_clip,
    leaky_relu with the TF tie rule, separator_loss) in torch float64, autograd for every gradient.  Each also returns the sum
    of |terms| -- the same expression over absolute values -- that the error bounds of the GPU tests are made of.
  * `*_model`: the same operators written out element by element in numpy float64, the way the kernels compute them.  They
    exist to carry MUTANTS (a wrong clamp weight, a wrong tie, ...): tests/test_elementwise_host.py checks that the unmutated
    models equal the oracle references and that every mutant misses them by more than the GPU tests' bounds.
Also the bounds themselves, so that the host tests judge the mutants by exactly what the GPU tests assert."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import waveunet_torch as wt

EPS32 = 2.0 ** -24          # unit roundoff of fp32
# x max(1, max|ref|), for values through __expf / tanhf and for dw, which have no derivable bound: the project's single-operator
# tolerance (tests/test_gpu_parity.py: 2e-5) brought to within 10x of what these kernels were observed to deliver on an MI355X
# (sigmoid-weighted mid-points 1.6e-7, their adjoint 1.1e-7, dw 4.0e-7, tanh outputs 5.3e-7, the fused
# epilogue's upsampled conv outputs 4.1e-7)
OP_TOL = 5e-6
CONV_TOL = 2e-5             # x max(1, max|ref|): conv outputs themselves (tests/test_gpu_parity.py; observed <= 1.9e-6)
LOSS_TOL = 2e-6             # relative
BF16_DIFF_SHARE = 1e-3      # share of bf16 outputs that may differ from the once-rounded float64 reference at all


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, requires_grad=grad)


# ---------------------------------------------------------------------------------------------------------------------------
# bf16
# ---------------------------------------------------------------------------------------------------------------------------
def bf16_round(a, mode="nearest"):
    """float64 -> the bf16 grid (8 significant bits), ONE rounding: to nearest, ties to even ("nearest"), or towards zero
    ("truncate": the mutant).  Returned as float64 (every bf16 value is one).  Normal range only."""
    a = np.asarray(a, dtype=np.float64)
    m, e = np.frexp(a)                                   # a = m 2^e, 0.5 <= |m| < 1
    q = m * 256.0                                        # 128 <= |q| < 256: the integer part holds 8 significant bits
    q = np.rint(q) if mode == "nearest" else np.trunc(q)     # np.rint rounds halves to even
    return np.ldexp(q / 256.0, e)


def bf16_spacing(a):
    """Distance between neighbouring bf16 values at magnitude |a| (2^-7 of the binade's power of two)."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    _, e = np.frexp(np.maximum(a, 2.0 ** -126))
    return np.ldexp(1.0, e - 8)


def to_bf16_bits(a):
    """bf16-valued float array -> uint16 bit patterns."""
    f = np.ascontiguousarray(a, dtype=np.float32)
    assert np.array_equal(f.astype(np.float64), np.asarray(a, dtype=np.float64)), "not fp32-valued"
    u = f.view(np.uint32)
    assert not np.any(u & 0xFFFF), "not bf16-valued"
    return (u >> 16).astype(np.uint16)


def from_bf16_bits(u):
    return (np.ascontiguousarray(u, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------------
def fp32_bound(terms, mag, ref):
    """A length-`terms` fp32 dot product accumulated in any order, FMA or not, then a few more roundings:
    (terms + 2) 2^-24 sum|terms| + 2^-24 |ref| (tests/test_gpu_resample.py)."""
    return (terms + 2) * EPS32 * np.asarray(mag) + EPS32 * np.abs(ref)


def op_tol(ref):
    return OP_TOL * max(1.0, float(np.abs(ref).max()) if np.size(ref) else 0.0)


def bf16_bound(ref_rounded, largest_term, fp32_part):
    """|got - ref| for a bf16 store of an fp32 result: one bf16 spacing at max(|ref|, largest |term|) plus the fp32 bound."""
    return bf16_spacing(np.maximum(np.abs(ref_rounded), largest_term)) + fp32_part


# ---------------------------------------------------------------------------------------------------------------------------
# upsampling: oracle references
# ---------------------------------------------------------------------------------------------------------------------------
def _ups(x, w, context):
    return wt.upsample_linear(x, context) if w is None else wt.upsample_learned(x, w, context)


def upsample_ref(x, w, tup):
    """x [B, C, n] (w [C] or None, tup = 2n - 1 or 2n) -> y [B, C, tup], sum|terms|, largest |term| per element."""
    n = x.shape[2]
    assert tup in (2 * n - 1, 2 * n)
    ctx = tup == 2 * n - 1
    wv = None if w is None else _t(w)
    y = _ups(_t(x), wv, ctx).numpy()
    ax = np.abs(np.asarray(x, dtype=np.float64))
    mag = _ups(_t(ax), wv, ctx).numpy()
    # largest single term: the two neighbours' magnitudes (their weights are at most 1)
    nb = np.concatenate([ax[:, :, 1:], ax[:, :, -1:] if w is None else 0 * ax[:, :, -1:]], axis=2)
    big = np.empty((x.shape[0], x.shape[1], 2 * n))
    big[:, :, 0::2] = ax
    big[:, :, 1::2] = np.maximum(ax, nb)
    return y, mag, big[:, :, :tup]


def _pre_of(x):
    """A pre-activation whose LeakyReLU is x (x > 0: x, else 5 x): the oracle's leaky_relu then supplies the mask, with
    TensorFlow's 0.2 at the tie -- +0.0 and -0.0 alike."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(x > 0, x, 5.0 * x)


def upsample_backward_ref(dy, x, w, tup):
    """Adjoint of upsample_ref at the stored activation x, times LeakyReLU'(x); autograd through the oracle.
    -> dict(dz, dw (None when linear), dz_mag (the same sum over |dy|), dz_big (largest |term|))."""
    n = x.shape[2]
    ctx = tup == 2 * n - 1
    out = {}
    for key, g in (("dz", np.asarray(dy, dtype=np.float64)), ("dz_mag", np.abs(np.asarray(dy, dtype=np.float64)))):
        pre = _t(_pre_of(x), True)
        wv = None if w is None else _t(w, True)
        y = _ups(wt.leaky_relu(pre), wv, ctx)
        (y * _t(g)).sum().backward()
        out[key] = pre.grad.numpy()
        if key == "dz":
            out["dw"] = None if w is None else wv.grad.numpy()
    ad = np.abs(np.asarray(dy, dtype=np.float64))
    padded = np.zeros((ad.shape[0], ad.shape[1], 2 * n + 1))
    padded[:, :, 1:1 + tup] = ad                          # padded[2i + 1 + d] = |dy[2i + d]|, d = -1, 0, 1
    out["dz_big"] = np.maximum(np.maximum(padded[:, :, 0:2 * n:2], padded[:, :, 1:2 * n + 1:2]), padded[:, :, 2:2 * n + 2:2])
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# upsampling: element-wise models with mutants
# ---------------------------------------------------------------------------------------------------------------------------
def _sig(w, C, mutant):
    """sigmoid(w[c]) per channel [C]; "channel_xor": of channel c ^ 1 where that channel exists."""
    idx = np.arange(C)
    if mutant == "channel_xor":
        idx = np.where((idx ^ 1) < C, idx ^ 1, idx)
    return 1.0 / (1.0 + np.exp(-np.asarray(w, dtype=np.float64)[idx]))


def _next_sample(x, fill_last):
    """x[i + 1], with x[n] = x[n - 1] (fill_last) or 0."""
    last = x[:, :, -1:] if fill_last else np.zeros_like(x[:, :, -1:])
    return np.concatenate([x[:, :, 1:], last], axis=2)


def upsample_model(x, w, tup, mutant=None):
    """mutant: "x_n_repeats" (learned/same: x[n] = x[n-1] instead of 0), "channel_xor" (weight of channel c ^ 1),
    "tail_unwritten" (the last element of every row left NaN), "half_clamp" (linear/same: out[2n-1] = x[n-1] / 2)."""
    x = np.asarray(x, dtype=np.float64)
    B, C, n = x.shape
    y = np.full((B, C, 2 * n), np.nan)
    y[:, :, 0::2] = x
    if w is not None:
        s = _sig(w, C, mutant)[None, :, None]
        y[:, :, 1::2] = s * x + (1.0 - s) * _next_sample(x, mutant == "x_n_repeats")
    else:
        y[:, :, 1::2] = 0.5 * (x + _next_sample(x, True))
        if mutant == "half_clamp":
            y[:, :, 2 * n - 1] = 0.5 * x[:, :, n - 1]
    y = y[:, :, :tup].copy()
    if mutant == "tail_unwritten":
        y[:, :, tup - 1] = np.nan
    return y


def upsample_backward_model(dy, x, w, tup, mutant=None):
    """-> dz, dw.  mutant: "half_clamp" (weight 0.5 instead of 1 at i == n - 1, linear/same), "tie_one" (LeakyReLU' = 1
    at x == 0), "channel_xor", "x_n_repeats" (dw: x[n] = x[n-1]), "tail_unwritten" (dz[n-1] left NaN)."""
    dy = np.asarray(dy, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    B, C, n = x.shape
    p = np.zeros((B, C, 2 * n + 1))
    p[:, :, 1:1 + tup] = dy                               # p[2i + 1 + d] = dy[2i + d] (0 outside [0, tup)), d = -1, 0, 1
    dm1, d0, dp1 = p[:, :, 0:2 * n:2], p[:, :, 1:2 * n + 1:2], p[:, :, 2:2 * n + 2:2]
    wa = np.full((C, n), 0.5)
    wb = np.full((C, 1), 0.5)
    dw = None
    if w is not None:
        s = _sig(w, C, mutant)
        wa, wb = np.repeat(s[:, None], n, axis=1), (1.0 - s)[:, None]
        dw = s * (1.0 - s) * np.sum(dp1 * (x - _next_sample(x, mutant == "x_n_repeats")), axis=(0, 2))
    elif tup == 2 * n and mutant != "half_clamp":
        wa[:, n - 1] = 1.0                                 # same-mode clamp: out[2n-1] = x[n-1]
    pos = (x >= 0) if mutant == "tie_one" else (x > 0)
    dz = (d0 + wa[None] * dp1 + wb[None] * dm1) * np.where(pos, 1.0, 0.2)
    if mutant == "tail_unwritten":
        dz[:, :, n - 1] = np.nan
    return dz, dw


# ---------------------------------------------------------------------------------------------------------------------------
# head
# ---------------------------------------------------------------------------------------------------------------------------
class HeadCase:
    """Shapes and switches of one head problem (the fields of wun_op_head_desc)."""

    def __init__(self, C, F, Sh, difference, Ko, padl, Tfeat, Tout, B, tanh, training):
        self.C, self.F, self.Sh, self.difference, self.Ko, self.padl = C, F, Sh, int(difference), Ko, padl
        self.Tfeat, self.Tout, self.B, self.tanh, self.training = Tfeat, Tout, B, int(tanh), int(training)
        self.S = Sh + self.difference
        self.terms = Ko * (C + F) + 1

    def in_training(self):
        return HeadCase(self.C, self.F, self.Sh, self.difference, self.Ko, self.padl, self.Tfeat, self.Tout, self.B, self.tanh, 1)

    @property
    def cfg(self):
        return {"source_names": ["s%d" % i for i in range(self.S)], "mono_downmix": self.C == 1}

    def __repr__(self):
        return "C%d F%d Sh%d %s Ko%d padl%d Tf%d To%d B%d %s%s" % (
            self.C, self.F, self.Sh, "diff" if self.difference else "direct", self.Ko, self.padl, self.Tfeat, self.Tout, self.B,
            "tanh" if self.tanh else "linear", "/train" if self.training else "")


def _head_conv(hc, inp, W, b):
    """pre[b][c][t] = bias[c] + sum_{k, ci} W[k][ci][c] in[b][ci][t + k - padl], zero outside [0, Tfeat), 0 <= t < Tout:
    the oracle's conv1d_tf ('valid') on the explicitly padded input."""
    right = hc.Tout + hc.Ko - 1 - hc.padl - hc.Tfeat
    xp = F.pad(inp, (hc.padl, max(right, 0)))
    return wt.conv1d_tf(xp, W, b, False)[:, :, :hc.Tout]


def _head_forward_t(hc, mix_feat, mix_diff, feat, Ws, bs, act=True):
    """torch: mix_feat [B, C, Tfeat], mix_diff [B, C, Tout], feat [B, F, Tfeat] -> (list of S outputs [B, C, Tout], pres)."""
    inp = torch.cat([mix_feat, feat], dim=1)
    outs, pres, total = [], [], 0
    for s in range(hc.Sh):
        pre = _head_conv(hc, inp, Ws[s], bs[s])
        pres.append(pre)
        o = pre
        if act:
            o = torch.tanh(pre) if hc.tanh else wt.audio_clip(pre, bool(hc.training))
        outs.append(o)
        total = total + o
    if hc.difference:
        last = mix_diff - total
        outs.append(wt.audio_clip(last, bool(hc.training)) if act else last)
    return outs, pres


def head_forward_ref(hc, mix_feat, mix_diff, feat, Ws, bs):
    """-> out [S, B, Tout, C], mag (sum|terms| of the value each output was made from, before the activation; for the
    difference output |mix| + sum_s |out_s|), both float64."""
    outs, _ = _head_forward_t(hc, _t(mix_feat), _t(mix_diff), _t(feat), [_t(w) for w in Ws], [_t(b) for b in bs])
    mags, _ = _head_forward_t(hc, _t(np.abs(mix_feat)), _t(np.abs(mix_diff)), _t(np.abs(feat)), [_t(np.abs(w)) for w in Ws],
                              [_t(np.abs(b)) for b in bs], act=False)
    if hc.difference:
        mags[-1] = _t(np.abs(mix_diff)) + sum(o.abs() for o in outs[:-1])
    to = lambda l: torch.stack([o.permute(0, 2, 1) for o in l]).numpy()
    return to(outs), to(mags)


def head_backward_ref(hc, mix_feat, mix_diff, feat, Ws, bs, targets=None, d_outputs=None):
    """Autograd through the oracle's head at the stored activation `feat` (a LeakyReLU output; the mask follows the TF tie
    rule).  targets [S, B, Tout, C]: the MSE of separator_loss; d_outputs: that upstream gradient instead.
    The gradient is the TRAINING graph's (Utils.AudioClip clips at inference only; the backward kernels never read `training`).
    -> dict(loss (None with d_outputs), dpre [Sh, B, C, Tout], dzfeat [B, F, Tfeat], dfeat_abs(v): the transposed head conv
    with |W| applied to a non-negative [Sh, B, C, Tout] tensor)."""
    hc = hc.in_training()
    pre_f = _t(_pre_of(feat), True)
    Wt = [_t(w) for w in Ws]
    outs, pres = _head_forward_t(hc, _t(mix_feat), _t(mix_diff), wt.leaky_relu(pre_f), Wt, [_t(b) for b in bs])
    for p in pres:
        p.retain_grad()
    loss = None
    if targets is not None:
        names = hc.cfg["source_names"]
        loss = wt.separator_loss(hc.cfg, {n: outs[i].permute(0, 2, 1) for i, n in enumerate(names)},
                                 {n: _t(targets[i]) for i, n in enumerate(names)})
        loss.backward()
        loss = float(loss.detach())
    else:
        sum((outs[i] * _t(d_outputs[i]).permute(0, 2, 1)).sum() for i in range(hc.S)).backward()

    def dfeat_abs(v):
        f = _t(np.zeros_like(feat), True)
        z = torch.zeros(hc.B, hc.C, hc.Tfeat, dtype=torch.float64)
        tot = 0
        for s in range(hc.Sh):
            tot = tot + (_head_conv(hc, torch.cat([z, f], dim=1), Wt[s].abs(), None) * _t(v[s])).sum()
        tot.backward()
        return f.grad.numpy()

    return {"loss": loss, "dpre": torch.stack([p.grad for p in pres]).numpy(), "dzfeat": pre_f.grad.numpy(),
            "dfeat_abs": dfeat_abs}


def head_dpre_model(hc, out, targets=None, d_outputs=None, mutant=None):
    """head_bwd_kernel / head_grad_kernel written out: dpre [Sh, B, C, Tout] from out (and targets or d_outputs), all
    [S, B, Tout, C].  mutant: "no_tanh_derivative" (1 - y^2 dropped), "glast_sign" (+ glast instead of -).
    Also returns sum|terms| of dpre before the tanh factor."""
    out = np.asarray(out, dtype=np.float64)
    gscale = 2.0 / (hc.S * hc.B * hc.Tout * hc.C)
    if targets is not None:
        g = gscale * (out - np.asarray(targets, dtype=np.float64))
        gm = gscale * (np.abs(out) + np.abs(np.asarray(targets, dtype=np.float64)))
    else:
        g = np.asarray(d_outputs, dtype=np.float64)
        gm = np.abs(g)
    glast = g[hc.S - 1] if hc.difference else 0.0
    glm = gm[hc.S - 1] if hc.difference else 0.0
    dpre = g[:hc.Sh] + glast if mutant == "glast_sign" else g[:hc.Sh] - glast
    mag = gm[:hc.Sh] + glm
    if hc.tanh and mutant != "no_tanh_derivative":
        dpre = dpre * (1.0 - out[:hc.Sh] ** 2)
    return dpre.transpose(0, 1, 3, 2), mag.transpose(0, 1, 3, 2)


def dpre_bound(hc, mag, ref):
    """gscale (y - t) - glast, times 1 - y^2: at most 4 terms, each the product of up to three fp32 roundings, and a factor
    1 - y^2 (|y| <= 1) whose own error is below 5 2^-24 -> 12 2^-24 sum|terms| + 2^-24 |ref|."""
    return 12 * EPS32 * np.asarray(mag) + EPS32 * np.abs(ref)


def _tap_ranges(hc, k):
    """Output positions [t0, t1) whose tap k reads inside the feature map, and the first feature position they read."""
    t0 = max(0, hc.padl - k)
    t1 = min(hc.Tout, hc.Tfeat + hc.padl - k)
    return t0, t1, t0 + k - hc.padl


def head_dfeat_model(hc, dpre, feat, Ws, mutant=None):
    """head_dfeat_kernel written out: dzfeat[b][f][u] = LeakyReLU'(feat) sum_{k, s, c} W_s[k][C + f][c] dpre[s][b][c][u - k + padl].
    mutant: "tie_one", "channel_xor" (dpre of channel c ^ 1), "tail_unwritten"."""
    dpre = np.asarray(dpre, dtype=np.float64)
    feat = np.asarray(feat, dtype=np.float64)
    g = np.zeros((hc.B, hc.F, hc.Tfeat))
    for k in range(hc.Ko):
        t0, t1, u0 = _tap_ranges(hc, k)
        if t1 <= t0:
            continue
        for s in range(hc.Sh):
            for c in range(hc.C):
                cc = c ^ 1 if (mutant == "channel_xor" and (c ^ 1) < hc.C) else c
                wk = np.asarray(Ws[s], dtype=np.float64)[k, hc.C:, c]
                g[:, :, u0:u0 + t1 - t0] += wk[None, :, None] * dpre[s, :, cc, t0:t1][:, None, :]
    pos = (feat >= 0) if mutant == "tie_one" else (feat > 0)
    g = g * np.where(pos, 1.0, 0.2)
    if mutant == "tail_unwritten":
        g[:, :, hc.Tfeat - 1] = np.nan
    return g


def head_forward_model(hc, mix_feat, mix_diff, feat, Ws, bs, mutant=None):
    """head_fwd_kernel written out -> out [S, B, Tout, C].  mutant: "channel_xor" (output channel c ^ 1 of the weights),
    "tail_unwritten" (the last position left NaN)."""
    inp = np.concatenate([np.asarray(mix_feat, dtype=np.float64), np.asarray(feat, dtype=np.float64)], axis=1)
    out = np.full((hc.S, hc.B, hc.Tout, hc.C), np.nan)
    tot = np.zeros((hc.B, hc.Tout, hc.C))
    for s in range(hc.Sh):
        W, b = np.asarray(Ws[s], dtype=np.float64), np.asarray(bs[s], dtype=np.float64)
        for c in range(hc.C):
            cc = c ^ 1 if (mutant == "channel_xor" and (c ^ 1) < hc.C) else c
            acc = np.full((hc.B, hc.Tout), b[cc])
            for k in range(hc.Ko):
                t0, t1, u0 = _tap_ranges(hc, k)
                if t1 > t0:
                    acc[:, t0:t1] += np.einsum("bit,i->bt", inp[:, :, u0:u0 + t1 - t0], W[k, :, cc])
            v = np.tanh(acc) if hc.tanh else (acc if hc.training else np.clip(acc, -1, 1))
            out[s, :, :, c] = v
            tot[:, :, c] += v
    if hc.difference:
        v = np.asarray(mix_diff, dtype=np.float64).transpose(0, 2, 1) - tot
        out[hc.S - 1] = v if hc.training else np.clip(v, -1, 1)
    if mutant == "tail_unwritten":
        out[:, :, hc.Tout - 1, :] = np.nan
    return out


def head_out_bound(hc, out_ref, mag):
    """Per-element bound of the head's outputs [S, B, Tout, C].  Linear head sources: the fp32 dot-product bound with
    Ko (C + F) + 1 terms (clipping is 1-Lipschitz).  The difference output: mix - sum of Sh sources, each of which carries its
    own bound -> sum of the sources' bounds + (Sh + 3) 2^-24 (|mix| + sum|out_s|).  tanh sources: OP_TOL (tanhf has no
    derivable bound), and a difference output made of them Sh OP_TOL + its own fp32 part."""
    b = np.empty_like(out_ref)
    if hc.tanh:
        b[:hc.Sh] = op_tol(out_ref[:hc.Sh])
    else:
        b[:hc.Sh] = fp32_bound(hc.terms, mag[:hc.Sh], out_ref[:hc.Sh])
    if hc.difference:
        b[hc.S - 1] = b[:hc.Sh].sum(axis=0) + fp32_bound(hc.Sh + 1, mag[hc.S - 1], out_ref[hc.S - 1])
    return b


# ---------------------------------------------------------------------------------------------------------------------------
# layout change
# ---------------------------------------------------------------------------------------------------------------------------
def btc_to_ncw_ref(src):
    return np.ascontiguousarray(np.asarray(src).transpose(0, 2, 1))


# ---------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_elementwise.py (shared with the sensitivity tests of tests/test_elementwise_host.py, which judge
# the mutants on exactly these inputs)
# ---------------------------------------------------------------------------------------------------------------------------
UPS_N = (1, 2, 3, 4, 5, 7, 8, 9, 127, 128, 129, 257, 1029)      # 1029: interp_grad_rows_kernel's second trip (nmid > 1024)
UPS_BC = ((3, 5), (2, 1), (1, 8))                                # B * C mod 4 = 3, 2, 0


def _seed(*key):
    h = 2166136261
    for k in key:
        h = ((h ^ (int(k) & 0xFFFFFFFF)) * 16777619) & 0xFFFFFFFF
    return h


def _with_zeros(a):
    """Every fifth element (flat index 1, 6, 11, ..) an exact zero, alternately +0.0 and -0.0."""
    f = a.reshape(-1)
    idx = np.arange(1, f.size, 5)
    f[idx] = np.where((idx // 5) % 2 == 0, 0.0, -0.0).astype(f.dtype)
    return a


def ups_inputs(B, C, n, tup, learned, bf16):
    """x [B, C, n] (the mask operand of the adjoint: positive, negative, +0.0 and -0.0), dy [B, C, tup], w [C] in U(-4, 4) or
    None.  fp32-valued (bf16-valued with bf16) float64 arrays; w float32."""
    rng = np.random.default_rng(_seed(B, C, n, tup, learned, bf16))
    x = _with_zeros(rng.uniform(-1, 1, (B, C, n)).astype(np.float32)).astype(np.float64)
    dy = rng.uniform(-1, 1, (B, C, tup)).astype(np.float32).astype(np.float64)
    w = rng.uniform(-4, 4, C).astype(np.float32) if learned else None
    if bf16:
        x, dy = bf16_round(x), bf16_round(dy)
    return x, dy, w


HEAD_F = (1, 3, 4, 5, 8, 9, 24)
HEAD_TOUT = (1, 2, 3, 4, 5, 6, 7, 8, 257)          # 6: a two-position tail behind whole groups of four
HEAD_GEOM = ((1, 0, 0), (3, 1, 0), (3, 0, 2), (2, 0, 1))            # (Ko, padl, Tfeat - Tout)
HEAD_ACT = ((1, 0), (0, 0), (0, 1))                                 # (tanh, training)


def head_cases(F):
    """[(HeadCase, feat_bf16)] for one feature count: every C x Tout x geometry; the number of head sources (1..4), direct /
    difference, the activation, the feature map's type and the batch (1..3) drawn per case from a fixed seed."""
    out = []
    for C in (1, 2):
        for Tout in HEAD_TOUT:
            for gi, (Ko, padl, dT) in enumerate(HEAD_GEOM):
                rng = np.random.default_rng(_seed(F, C, Tout, gi, 7))
                Sh, diff, act, bf, B = (int(rng.integers(1, 5)), int(rng.integers(0, 2)), int(rng.integers(0, 3)),
                                        int(rng.integers(0, 2)), int(rng.integers(1, 4)))
                tanh, training = HEAD_ACT[act]
                out.append((HeadCase(C, F, Sh, diff, Ko, padl, Tout + dT, Tout, B, tanh, training), bf))
    return out


MIX_OFF_FEAT = 3                                                    # crop offsets into a mix row used by the tests


def head_inputs(hc, feat_bf16, seed=0):
    """dict: mix [B, C, mix_len] with off_feat / off_diff, feat [B, F, Tfeat] (+-0 included), Ws / bs per source (scaled so that
    |pre-activation| > 1 occurs), targets and d_outputs [S, B, Tout, C].  fp32-valued float64 arrays."""
    rng = np.random.default_rng(_seed(hc.C, hc.F, hc.Sh, hc.difference, hc.Ko, hc.padl, hc.Tfeat, hc.Tout, hc.B, hc.tanh, seed))
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    off_feat = MIX_OFF_FEAT
    off_diff = off_feat + (hc.Tfeat - hc.Tout + 1) // 2
    mix_len = off_feat + max(hc.Tfeat, hc.Tout + off_diff - off_feat) + 2
    d = {"off_feat": off_feat, "off_diff": off_diff, "mix_len": mix_len}
    d["mix"] = f32(rng.uniform(-1, 1, (hc.B, hc.C, mix_len)))
    feat = _with_zeros(rng.uniform(-1.5, 1.5, (hc.B, hc.F, hc.Tfeat)).astype(np.float32)).astype(np.float64)
    d["feat"] = bf16_round(feat) if feat_bf16 else feat
    scale = 3.0 / np.sqrt(hc.Ko * (hc.C + hc.F))
    d["Ws"] = [f32(rng.uniform(-1, 1, (hc.Ko, hc.C + hc.F, hc.C)) * scale) for _ in range(hc.Sh)]
    d["bs"] = [f32(rng.uniform(-0.5, 0.5, hc.C)) for _ in range(hc.Sh)]
    d["targets"] = f32(rng.uniform(-1, 1, (hc.S, hc.B, hc.Tout, hc.C)))
    d["d_outputs"] = f32(rng.uniform(-1, 1, (hc.S, hc.B, hc.Tout, hc.C)))
    d["mix_feat"] = d["mix"][:, :, off_feat:off_feat + hc.Tfeat]
    d["mix_diff"] = d["mix"][:, :, off_diff:off_diff + hc.Tout]
    return d


def head_param_layout(hc):
    """Parameter blocks in REVERSE order with gaps: (hoff per source, arena floats).  Block = W [Ko][C+F][C] then bias [C]."""
    blk = hc.Ko * (hc.C + hc.F) * hc.C + hc.C
    hoff = [3 + (hc.Sh - 1 - s) * (blk + 5) for s in range(hc.Sh)]
    return hoff, 3 + hc.Sh * (blk + 5)


def head_param_arena(hc, Ws, bs):
    hoff, n = head_param_layout(hc)
    arena = np.full(n, np.nan, dtype=np.float32)
    for s in range(hc.Sh):
        blk = np.concatenate([np.asarray(Ws[s], dtype=np.float32).reshape(-1), np.asarray(bs[s], dtype=np.float32)])
        arena[hoff[s]:hoff[s] + blk.size] = blk
    return hoff, arena


# ---------------------------------------------------------------------------------------------------------------------------
# verdicts: what the GPU tests assert, as functions the sensitivity tests can apply to a mutant
# ---------------------------------------------------------------------------------------------------------------------------
def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; inf where got is not finite (an element left unwritten).  0 / 0 counts as 0."""
    got, ref, bound = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    bound = np.broadcast_to(bound, ref.shape)
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


def differ_count(got, ref):
    return int(np.count_nonzero(np.asarray(got, dtype=np.float64) != np.asarray(ref, dtype=np.float64))), int(np.size(ref))


def ups_verdict(got, ref, w, bf, mag, big, pool=None):
    """The GPU test's verdict on an upsampled tensor: worst |err| / bound (> 1 fails)."""
    if bf:
        r = bf16_round(ref)
        part = op_tol(ref) if w is not None else fp32_bound(2, mag, ref)
        if pool is not None and np.isfinite(got).all():
            d, t = differ_count(got, r)
            pool[0] += d
            pool[1] += t
        return worst_ratio(got, r, bf16_bound(r, big, part))
    bound = np.zeros_like(ref)                                        # exact arithmetic: even outputs, linear mid-points
    if w is not None:
        bound[:, :, 1::2] = op_tol(ref)
    return worst_ratio(got, ref.astype(np.float32).astype(np.float64), bound)


def dz_verdict(got, r, w, bf, pool=None):
    part = op_tol(r["dz"]) if w is not None else fp32_bound(3, r["dz_mag"], r["dz"])
    if bf:
        rr = bf16_round(r["dz"])
        if pool is not None and np.isfinite(got).all():
            d, t = differ_count(got, rr)
            pool[0] += d
            pool[1] += t
        return worst_ratio(got, rr, bf16_bound(rr, r["dz_big"], part))
    return worst_ratio(got, r["dz"], part)


def dzfeat_verdict(hc, got, r, dp_mag, bf, pool=None):
    """dzfeat = mask * sum_{k, s, c} W dpre: Ko Sh C terms over the kernel's own dpre, which carries dpre_bound."""
    part = fp32_bound(hc.Ko * hc.Sh * hc.C, r["dfeat_abs"](np.abs(r["dpre"])), r["dzfeat"]) + \
        r["dfeat_abs"](dpre_bound(hc, dp_mag, r["dpre"]))
    if bf:
        rr = bf16_round(r["dzfeat"])
        if pool is not None and np.isfinite(got).all():
            d, t = differ_count(got, rr)
            pool[0] += d
            pool[1] += t
        return worst_ratio(got, rr, bf16_bound(rr, 0.0, part))
    return worst_ratio(got, r["dzfeat"], part)
