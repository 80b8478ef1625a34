"""The oracle of the spectrogram U-Net's backward pass from any upstream gradient (include/wun.h:
wun_spec_backward, wun_spec_train_audio, wun_op_spec_head_backward): the audio of a training forward, the head -- the adjoint of
ISTFT_tf and the mask gradient -- and the network backward of _specunet_train_np.loss_and_gradients restated with the head's dz as
an argument.  Written from the formulas in torch on the CPU WITHOUT autograd, in float64 (or, as the stand-in whose own error sets
the GPU tolerances, float32); tests/test_specunet_backward_host.py holds it to torch.autograd.

    u[t]  = d_audio[t] / D[t mod hop]                 (the header: the kernel divides by D rounded once to float32; the float32
                                                       stand-in does the same, the float64 oracle divides by the float64 D)
    G     = STFT(u), the forward's framing and window
    ga[k] = c_k (Re X[k] Re G[k] + Im X[k] Im G[k]),  c_0 = 1 / n_fft, c_k = 2 / n_fft for 0 < k < K - 1
    dmask = d_mags M + ga  (either term alone where the other gradient is absent),  dz = dmask * (mask (1 - mask)),  k < K - 1
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _specunet_np as ora  # noqa: E402
import _specunet_train_np as tro  # noqa: E402

GEOMETRIES = tro.GEOMETRIES
fixture, fixture_masks, train_forward = tro.fixture, tro.fixture_masks, tro.train_forward


def spectrum(mix, n_fft, hop, dtype=torch.float64):
    """X = STFT(mix) [B, F, K] complex, as train_forward takes it."""
    return ora.stft(torch.as_tensor(np.asarray(mix), dtype=dtype), n_fft, hop)


def audio_output(fw, mix, n_fft, hop):
    """[S][B, T]: ISTFT_tf(mask_s X) of a train_forward result (bin K - 1 takes the constant 0.5)."""
    B, F, K, L, S = fw["dims"]
    dtype = fw["M"].dtype
    X = spectrum(mix, n_fft, hop, dtype)
    half = torch.full((B, F, 1), 0.5, dtype=dtype)
    return [ora.istft_tf(torch.cat([fw["src"][s]["mask"], half], dim=2) * X, n_fft, hop) for s in range(S)]


def istft_tf_adjoint(d_audio, n_fft, hop):
    """d_audio [B, T] -> G = STFT(d_audio / D) [B, F, K] complex, and sum_n |w[n] u[f hop + n]| [B, F] (the floor's scale)."""
    dtype = d_audio.dtype
    T = d_audio.shape[-1]
    D = ora.steady_denominator(n_fft, hop, dtype)            # float32: the float64 sums rounded once
    u = d_audio / D[torch.arange(T) % hop]
    absw = (u.abs().unfold(-1, n_fft, hop) * ora.hann(n_fft, dtype)).sum(-1)
    return ora.stft(u, n_fft, hop), absw


def head(X, M, mask, d_mags, d_audio, n_fft, hop):
    """One source.  X [B, F, K] complex, M = |X|, mask [B, F, K - 1], d_mags [B, F, K] or None, d_audio [B, T] or None.
    -> (dz [B, F, K - 1], the floor's scale: max over bins of (|d_mags| M + c_k (|Re X| + |Im X|) sum_n |w u|) mask (1 - mask))."""
    assert d_mags is not None or d_audio is not None
    dtype = M.dtype
    K = M.shape[-1]
    dmask = torch.zeros_like(mask)
    scale = torch.zeros_like(mask)
    if d_mags is not None:
        dm = torch.as_tensor(np.asarray(d_mags), dtype=dtype)[..., :K - 1]
        dmask = dmask + dm * M[..., :K - 1]
        scale = scale + dm.abs() * M[..., :K - 1]
    if d_audio is not None:
        G, absw = istft_tf_adjoint(torch.as_tensor(np.asarray(d_audio), dtype=dtype), n_fft, hop)
        c = torch.full((K - 1,), 2.0 / n_fft, dtype=dtype)
        c[0] = 1.0 / n_fft
        Xs, Gs = X[..., :K - 1], G[..., :K - 1]
        dmask = dmask + c * (Xs.real * Gs.real + Xs.imag * Gs.imag)
        scale = scale + c * (Xs.real.abs() + Xs.imag.abs()) * absw[..., None]
    sg = mask * (1.0 - mask)
    return dmask * sg, float((scale * sg).max())


def network_backward(fw, dzs):
    """_specunet_train_np.loss_and_gradients from the head's dz on: dzs [S][B, F, K - 1] -> (grads {name: tensor}, floors {name:
    sum |terms| of the tensor at its largest output})."""
    B, F, K, L, S = fw["dims"]
    v = fw["v"]
    grads, floors = {}, {}
    for name, val in v.items():
        if name.endswith("moving_mean") or name.endswith("moving_variance"):
            grads[name] = torch.zeros_like(val)
    for s in range(S):
        c = fw["src"][s]
        down, up = tro.names(L, s)
        dz = dzs[s][..., None]
        g_skip = [None] * L
        g = None
        for i in range(L - 1, -1, -1):                       # the transposed layers, the mask layer first
            stem = up[i][0]
            grads[stem + "/kernel"] = tro.wgrad(dz, c["up_in"][i])
            floors[stem + "/kernel"] = float(tro.wgrad(dz.abs(), c["up_in"][i].abs()).max())
            grads[stem + "/bias"] = dz.reshape(-1, dz.shape[3]).sum(0)
            floors[stem + "/bias"] = float(dz.abs().reshape(-1, dz.shape[3]).sum(0).max())
            gin = ora.conv2d_s2(dz, v[stem + "/kernel"])
            if i == 0:
                g = gin
                break
            if c["mult"][i] is not None:
                gin = gin * c["mult"][i]
            c0 = c["act"][L - 1 - i].shape[3]
            g_skip[L - 1 - i] = gin[..., :c0]
            j = L + i - 1
            dz, dbeta, floors[up[i - 1][1] + "/beta"] = tro._bn_backward(gin[..., c0:], c["xh"][j], c["var"][j], c["zhat"][j], "relu")
            grads[up[i - 1][1] + "/beta"] = dbeta
        for i in range(L - 1, -1, -1):                       # the down path
            if g_skip[i] is not None:
                g = g + g_skip[i]
            dz, dbeta, floors[down[i][1] + "/beta"] = tro._bn_backward(g, c["xh"][i], c["var"][i], c["zhat"][i], "lrelu")
            grads[down[i][1] + "/beta"] = dbeta
            big = c["act"][i - 1] if i else fw["a0"]
            grads[down[i][0] + "/kernel"] = tro.wgrad(big, dz)
            floors[down[i][0] + "/kernel"] = float(tro.wgrad(big.abs(), dz.abs()).max())
            grads[down[i][0] + "/bias"] = dz.reshape(-1, dz.shape[3]).sum(0)
            floors[down[i][0] + "/bias"] = float(dz.abs().reshape(-1, dz.shape[3]).sum(0).max())
            if i:
                g = ora.conv2d_transpose_s2(dz, v[down[i][0] + "/kernel"])
    return grads, floors


def gradients(fw, mix, n_fft, hop, d_mags=None, d_audio=None):
    """fw: train_forward's result; d_mags [S, B, F, K] or None, d_audio [S, B, T] or None -> (grads, floors, dzs)."""
    B, F, K, L, S = fw["dims"]
    X = spectrum(mix, n_fft, hop, fw["M"].dtype)
    dzs = [head(X, fw["M"], fw["src"][s]["mask"], None if d_mags is None else d_mags[s], None if d_audio is None else d_audio[s],
                n_fft, hop)[0] for s in range(S)]
    grads, floors = network_backward(fw, dzs)
    return grads, floors, dzs


def l1_upstream(fw, targets, n_fft, hop):
    """d_mags [S, B, F, K] of Jansson's magnitude L1 (Training.py:55-63): -sign(R - M mask) / (S B F K)."""
    B, F, K, L, S = fw["dims"]
    dtype = fw["M"].dtype
    tg = torch.as_tensor(np.asarray(targets), dtype=dtype)
    return torch.stack([-torch.sign(ora.stft(tg[s], n_fft, hop).abs() - fw["mags"][s]) / float(S * B * F * K) for s in range(S)])


def mse_upstream(audio, targets):
    """(loss, d_audio [S, B, T]) of the raw-audio objective (Training.py:62-63): the mean over sources of the mean squared error."""
    a = torch.stack(list(audio))
    tg = torch.as_tensor(np.asarray(targets), dtype=a.dtype)
    d = a - tg
    return float((d * d).mean()), 2.0 * d / float(d.numel())


def mse_learning_curve(fx, steps, lr, dtype=torch.float32):
    """The float32 CPU restatement of the learning test: `steps` steps of Adam (tro.adam) on the MSE through the audio output,
    dropout 0, from the fixture's variables -> the losses."""
    variables = {k: np.asarray(a, dtype=np.float64) for k, a in fx["variables"].items()}
    m = {k: np.zeros_like(a) for k, a in variables.items()}
    vv = {k: np.zeros_like(a) for k, a in variables.items()}
    losses = []
    for step in range(1, steps + 1):
        cur = {k: a.astype(np.float32) for k, a in variables.items()}
        fw = train_forward(fx["mix"], cur, fx["L"], fx["nif"], fx["n_fft"], fx["hop"], None, dtype=dtype)
        loss, d_audio = mse_upstream(audio_output(fw, fx["mix"], fx["n_fft"], fx["hop"]), fx["targets"])
        losses.append(loss)
        grads, _, _ = gradients(fw, fx["mix"], fx["n_fft"], fx["hop"], d_audio=d_audio)
        for k in variables:
            if k.split("/")[-1].startswith("moving"):
                continue
            variables[k], m[k], vv[k] = tro.adam(variables[k], grads[k].numpy().astype(np.float64), m[k], vv[k], step, lr)
    return losses
