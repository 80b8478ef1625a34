"""The oracle of the spectrogram U-Net's training step: the forward at training=True with given dropout masks,
Jansson's magnitude L1, every gradient, TF-Adam and the moving averages -- written from the formulas in torch on the CPU WITHOUT
autograd, in float64 (or, as the stand-in whose own error sets the GPU tolerances, float32).  tests/test_specunet_train_host.py
holds it to torch.autograd.

Layout is TF's, as in _specunet_np.py.  Batch-norm layers are numbered j = 0..L-1 (down) and L..2L-2 (up); the transposed
layers i = 0..L-1, the last being the mask layer; dropout level lv is the concatenation that feeds transposed layer lv + 1.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _specunet_np as ora  # noqa: E402

BN_EPS = ora.BN_EPS
DROP_LEVELS = 3
_M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------ dropout keep bits (wun.h)
def _mix(z):
    """z: numpy uint64 array; arithmetic modulo 2^64."""
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def dropout_key(seed, step, source, level):
    u = lambda x: np.array([x & _M64], dtype=np.uint64)
    with np.errstate(over="ignore"):
        return _mix(_mix(_mix(u(int(seed))) + u(int(step))) + u((int(source) << 8) | int(level)))


def dropout_keep(seed, step, source, level, count, rate):
    """bool [count]: element e is kept iff (mix(key + e) >> 40) 2^-24 >= rate, compared in float32."""
    with np.errstate(over="ignore"):
        u = _mix(dropout_key(seed, step, source, level) + np.arange(count, dtype=np.uint64)) >> np.uint64(40)
    return (u.astype(np.float32) * np.float32(2.0 ** -24)) >= np.float32(rate)


def dropout_multipliers(seed, step, source, level, shape, rate):
    keep = dropout_keep(seed, step, source, level, int(np.prod(shape)), rate)
    return (keep.astype(np.float32) * (np.float32(1.0) / (np.float32(1.0) - np.float32(rate)))).reshape(shape)


# ------------------------------------------------------------------------------------------------ names
def names(L, s):
    """(down, up): lists of (conv stem, batch-norm stem or None) of source s."""
    down = [("separator/" + ora._suffix("conv2d", s * L + i), "separator/" + ora._suffix("BatchNorm", s * (2 * L - 1) + i))
            for i in range(L)]
    up = [("separator/" + ora._suffix("conv2d_transpose", s * L + i),
           "separator/" + ora._suffix("BatchNorm", s * (2 * L - 1) + L + i) if i < L - 1 else None) for i in range(L)]
    return down, up


# ------------------------------------------------------------------------------------------------ forward
def _bn_train(z, beta):
    n = z.shape[0] * z.shape[1] * z.shape[2]
    mu = z.reshape(n, -1).mean(0)
    var = ((z - mu) ** 2).reshape(n, -1).mean(0)             # biased, two passes
    xh = (z - mu) * torch.rsqrt(var + BN_EPS)
    return xh + beta, xh, mu, var


def train_forward(mix, variables, L, nif, n_fft, hop, masks=None, S=2, dtype=torch.float64):
    """mix [B, T]; masks {(source, level): multipliers [B, H, W, C]} or None.  -> dict with mags [S][B, F, K], M, and per source
    the cache of the backward: z, mean, var, xh, zhat, act per batch-norm layer, the (dropped) inputs of the transposed
    layers, the mask."""
    v = {k: torch.as_tensor(np.asarray(a), dtype=dtype) for k, a in variables.items()}
    x = torch.as_tensor(np.asarray(mix), dtype=dtype)
    B, T = x.shape
    X = ora.stft(x, n_fft, hop)
    F, K = X.shape[1], X.shape[2]
    M = X.abs()
    a0 = torch.log1p(M[:, :, :-1, None])
    out = {"M": M, "a0": a0, "mags": [], "src": [], "v": v, "dims": (B, F, K, L, S)}
    for s in range(S):
        down, up = names(L, s)
        c = {"z": [None] * (2 * L - 1), "mean": [None] * (2 * L - 1), "var": [None] * (2 * L - 1), "xh": [None] * (2 * L - 1),
             "zhat": [None] * (2 * L - 1), "act": [None] * (2 * L - 1), "up_in": [None] * L, "mult": [None] * L}
        cur = a0
        for i in range(L):
            z = ora.conv2d_s2(cur, v[down[i][0] + "/kernel"]) + v[down[i][0] + "/bias"]
            zhat, xh, mu, var = _bn_train(z, v[down[i][1] + "/beta"])
            cur = ora.leaky_relu(zhat)
            c["z"][i], c["mean"][i], c["var"][i], c["xh"][i], c["zhat"][i], c["act"][i] = z, mu, var, xh, zhat, cur
        for i in range(L):
            if i > 0:
                cur = torch.cat([c["act"][L - 1 - i], cur], dim=3)
                m = None if masks is None else masks.get((s, i - 1))
                if m is not None:
                    assert i - 1 < DROP_LEVELS
                    c["mult"][i] = torch.as_tensor(np.asarray(m), dtype=dtype)
                    cur = cur * c["mult"][i]
            c["up_in"][i] = cur
            z = ora.conv2d_transpose_s2(cur, v[up[i][0] + "/kernel"]) + v[up[i][0] + "/bias"]
            if i < L - 1:
                j = L + i
                zhat, xh, mu, var = _bn_train(z, v[up[i][1] + "/beta"])
                cur = torch.relu(zhat)
                c["z"][j], c["mean"][j], c["var"][j], c["xh"][j], c["zhat"][j], c["act"][j] = z, mu, var, xh, zhat, cur
            else:
                c["mask"] = torch.sigmoid(z)[..., 0]
        full = torch.cat([c["mask"], torch.full((B, F, 1), 0.5, dtype=dtype)], dim=2)
        out["mags"].append(M * full)
        out["src"].append(c)
    return out


# ------------------------------------------------------------------------------------------------ backward
def wgrad(big, small):
    """G[ky][kx][p][q] = sum_{b,y,x} Big[b][2y + ky - 1][2x + kx - 1][p] Small[b][y][x][q], zeros outside the big map."""
    B, H, W, _ = big.shape
    bp = torch.nn.functional.pad(big, (0, 0, 1, 2, 1, 2))
    g = torch.zeros((5, 5, big.shape[3], small.shape[3]), dtype=big.dtype)
    for ky in range(5):
        for kx in range(5):
            g[ky, kx] = torch.einsum("byxp,byxq->pq", bp[:, ky:ky + H:2, kx:kx + W:2, :], small)
    return g


def _bn_backward(g, xh, var, zhat, act):
    """g: the gradient behind the activation's output -> (dz, dbeta, the largest sum |g'| of a channel)."""
    if act == "lrelu":
        gp = torch.where(zhat > 0, g, 0.2 * g)
    else:
        gp = torch.where(zhat > 0, g, torch.zeros_like(g))
    n = g.shape[0] * g.shape[1] * g.shape[2]
    C = g.shape[3]
    mg = gp.reshape(n, C).mean(0)
    mgx = (gp * xh).reshape(n, C).mean(0)
    dz = torch.rsqrt(var + BN_EPS) * (gp - mg - xh * mgx)
    return dz, gp.reshape(n, C).sum(0), float(gp.abs().reshape(n, C).sum(0).max())


def loss_and_gradients(fw, targets, n_fft, hop):
    """fw: train_forward's result; targets [S, B, T] audio.  -> (loss, per-source losses, grads {name: tensor}, floors {name:
    sum |terms| of the tensor at its largest output}, diffs [S][B, F, K - 1] = R - M mask)."""
    B, F, K, L, S = fw["dims"]
    v, M = fw["v"], fw["M"]
    dtype = M.dtype
    tg = torch.as_tensor(np.asarray(targets), dtype=dtype)
    grads, floors, per, diffs = {}, {}, [], []
    for name, val in v.items():
        if name.endswith("moving_mean") or name.endswith("moving_variance"):
            grads[name] = torch.zeros_like(val)
    for s in range(S):
        c = fw["src"][s]
        down, up = names(L, s)
        R = ora.stft(tg[s], n_fft, hop).abs()
        d = R - fw["mags"][s]
        per.append(d.abs().mean())
        diffs.append(d[:, :, :-1])
        mask = c["mask"]
        dmask = -torch.sign(d[:, :, :-1]) * M[:, :, :-1] / float(S * B * F * K)
        dz = (dmask * mask * (1.0 - mask))[..., None]
        g_skip = [None] * L
        g = None
        for i in range(L - 1, -1, -1):                       # the transposed layers, the mask layer first
            stem = up[i][0]
            grads[stem + "/kernel"] = wgrad(dz, c["up_in"][i])
            floors[stem + "/kernel"] = float(wgrad(dz.abs(), c["up_in"][i].abs()).max())
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
            dz, dbeta, floors[up[i - 1][1] + "/beta"] = _bn_backward(gin[..., c0:], c["xh"][j], c["var"][j], c["zhat"][j], "relu")
            grads[up[i - 1][1] + "/beta"] = dbeta
        for i in range(L - 1, -1, -1):                       # the down path
            if g_skip[i] is not None:
                g = g + g_skip[i]
            dz, dbeta, floors[down[i][1] + "/beta"] = _bn_backward(g, c["xh"][i], c["var"][i], c["zhat"][i], "lrelu")
            grads[down[i][1] + "/beta"] = dbeta
            big = c["act"][i - 1] if i else fw["a0"]
            grads[down[i][0] + "/kernel"] = wgrad(big, dz)
            floors[down[i][0] + "/kernel"] = float(wgrad(big.abs(), dz.abs()).max())
            grads[down[i][0] + "/bias"] = dz.reshape(-1, dz.shape[3]).sum(0)
            floors[down[i][0] + "/bias"] = float(dz.abs().reshape(-1, dz.shape[3]).sum(0).max())
            if i:
                g = ora.conv2d_transpose_s2(dz, v[down[i][0] + "/kernel"])
    loss = sum(per) / float(S)
    return loss, per, grads, floors, diffs


# ------------------------------------------------------------------------------------------------ the update
def moving_average(moving, value, decay):
    """assign_moving_average without zero_debias: variable -= (1 - decay) (variable - value)."""
    return moving - (1.0 - decay) * (moving - value)


def unbiased(var, n):
    """What TF's fused batch norm hands to the moving average of the variance (read from TF's source; not verifiable here)."""
    return var * (float(n) / float(max(n - 1, 1)))


def adam(theta, g, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8):
    """TF's AdamOptimizer, 1-based step, float64 numpy."""
    lr_t = np.float64(np.float32(lr * np.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step)))
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    return theta - lr_t * m / (np.sqrt(v) + eps), m, v


# ------------------------------------------------------------------------------------------------ the fixtures of both test files
# (n_fft, hop, L, nif, F, B) as tests/test_gpu_specunet.py::GEOMETRIES, and the seed whose kinks lie far enough from every value
# (test_specunet_train_host.py::test_fixtures_stay_away_from_the_kinks chooses and checks them)
GEOMETRIES = {
    "skip": (64, 48, 2, 3, 8, 2),        # one up layer, one concatenation with dropout
    "flat": (64, 48, 1, 3, 2, 2),        # no up layer; the deepest map is 1 x 16
    "five": (64, 48, 5, 2, 32, 2),       # four up layers: the i < 3 dropout boundary; n = B = 2 at the deepest batch norm
    "flat_b1": (64, 48, 1, 3, 2, 1),     # small n through max(n - 1, 1)
}
SEEDS = {"skip": 0, "flat": 0, "five": 0, "flat_b1": 0}
DROPOUT_SEED = 1337


def fixture(name, seed=None):
    """-> dict: the geometry, mix [B, T], targets [S, B, T] (float32 values), variables."""
    n_fft, hop, L, nif, F, B = GEOMETRIES[name]
    seed = SEEDS[name] if seed is None else seed
    rng = np.random.RandomState(1000 + seed)
    T = (F - 1) * hop + n_fft
    targets = (0.5 * rng.randn(2, B, T)).astype(np.float32)
    mix = (targets[0] + targets[1]).astype(np.float32)
    return {"n_fft": n_fft, "hop": hop, "L": L, "nif": nif, "F": F, "B": B, "T": T, "mix": mix, "targets": targets,
            "variables": ora.random_variables(L, nif, 7 + seed)}


def dropout_shapes(fx):
    """{level: shape [B, H, W, C] of the concatenation} for the levels with dropout."""
    L, nif, F, B, W0 = fx["L"], fx["nif"], fx["F"], fx["B"], fx["n_fft"] // 2
    return {lv: (B, F >> (L - 1 - lv), W0 >> (L - 1 - lv), 2 * (nif << (L - 2 - lv))) for lv in range(min(L - 1, DROP_LEVELS))}


def fixture_masks(fx, rate, step=0, seed=DROPOUT_SEED, S=2):
    """{(source, level): multipliers}, or None where nothing is dropped (rate 0, or a geometry without an up level)."""
    if rate == 0 or not dropout_shapes(fx):
        return None
    return {(s, lv): dropout_multipliers(seed, step, s, lv, shp, rate) for s in range(S) for lv, shp in dropout_shapes(fx).items()}


def learn_fixture():
    """The fixed batch of the learning test on `skip`: a loud and a quiet noise source (0.5 and 0.05 rms), so that the masks
    have something to learn from the mixture's magnitude alone.  On the float32 CPU restatement (this module, dtype float32,
    `adam` above, lr 1e-3, dropout 0) the loss goes from 0.9679 at step 0 to 0.1985 at step 199: a fifth, against the half
    the test asks for."""
    fx = fixture("skip")
    rng = np.random.RandomState(5)
    tg = np.stack([0.5 * rng.randn(fx["B"], fx["T"]), 0.1 * 0.5 * rng.randn(fx["B"], fx["T"])]).astype(np.float32)
    fx["targets"], fx["mix"] = tg, (tg[0] + tg[1]).astype(np.float32)
    return fx
