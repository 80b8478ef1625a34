"""The extended optimizer step of include/wun.h (wun_optim_step, wun_ema_update) in numpy: the formulas in
float64, a bit-exact float32 restatement with the library's roundings, and the learning-rate factor of training.lr_factor
written out a second time.  Everything works on flat arrays; `decay` is a boolean array (which floats decay)."""
import math

import numpy as np

from _fma_chain_np import fmaf_np


def lr_t(step, lr, b1=0.9, b2=0.999):
    """TF-Adam's step size (Training.py:77), float64."""
    return lr * math.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step)


def clip_scale(norm, clip):
    """The factor on the scaled gradient: clip / N when N > clip, else none (1)."""
    return clip / norm if norm > clip else 1.0


def ema_weight(ema_decay, step, warmup):
    """1 - d_t in float64 from the fp32 ema_decay; d_t = decay, or min(decay, (1 + step) / (10 + step)) with warm-up
    (tf.train.ExponentialMovingAverage's num_updates rule)."""
    d = float(np.float32(ema_decay))
    if warmup:
        d = min(d, (1.0 + step) / (10.0 + step))
    return 1.0 - d


def step64(p, g, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0, scale=1.0, weight_decay=0.0, decay=None):
    """(theta, m, v) after one step, float64.  scale: clip_scale of the step; decay: bool array or None (nothing decays)."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    g = g * grad_scale * scale
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    if decay is not None and weight_decay:
        p = np.where(decay, p * (1.0 - lr * weight_decay), p)
    return p - lr_t(step, lr, b1, b2) * m / (np.sqrt(v) + eps), m, v


def ema64(ema, theta, ema_decay, step, warmup=False):
    """ema - (1 - d_t) (ema - theta), float64."""
    ema, theta = np.asarray(ema, np.float64), np.asarray(theta, np.float64)
    return ema - ema_weight(ema_decay, step, warmup) * (ema - theta)


def assign_moving_average(variable, value, decay):
    """A transcription of tensorflow.python.training.moving_averages.assign_moving_average without zero-debias:
    variable -= (variable - value) * (1 - decay)."""
    update_delta = (variable - value) * (1.0 - decay)
    return variable - update_delta


def tf_ema_decay(decay, num_updates=None):
    """tf.train.ExponentialMovingAverage.apply's decay: min(decay, (1 + num_updates) / (10 + num_updates)) when num_updates
    is given."""
    if num_updates is None:
        return decay
    return min(decay, (1.0 + num_updates) / (10.0 + num_updates))


def ema32(ema, theta, ema_decay, step, warmup=False):
    """The EMA line with the library's roundings: 1 - d_t rounded once to fp32; difference, product, difference each rounded
    (no fused multiply-add), so this is bit-exact."""
    f = np.float32
    ema, theta = np.asarray(ema, f), np.asarray(theta, f)
    w = f(ema_weight(ema_decay, step, warmup))
    return (ema - (w * (ema - theta)).astype(f)).astype(f)


def step32(p, g, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0, norm=None, clip=math.inf, weight_decay=0.0,
           decay=None):
    """(theta, m, v) with the library's roundings, bit-exact: g * grad_scale, times fp32(clip / N) when N > clip; m = fma(b1, m,
    (1 - b1) g); v = fma(b2, v, ((1 - b2) g) g), the fused multiply-adds exact (fmaf_np); theta * fp32(1 - lr wd) where it
    decays; theta - (lr_t m) / (sqrt(v) + eps), every other operation rounded once to fp32.  norm: the fp32 global norm N."""
    f = np.float32
    p, g, m, v = (np.asarray(a, f) for a in (p, g, m, v))
    gi = g * f(grad_scale)
    if norm is not None and f(norm) > f(clip):
        gi = gi * (f(clip) / f(norm))
    m = fmaf_np(f(b1), m, (f(1) - f(b1)) * gi)
    v = fmaf_np(f(b2), v, ((f(1) - f(b2)) * gi) * gi)
    if decay is not None and weight_decay:
        wdf = f(1.0 - float(f(lr)) * float(f(weight_decay)))
        p = np.where(decay, p * wdf, p)
    lt = f(lr_t(step, float(f(lr)), float(f(b1)), float(f(b2))))
    return (p - (lt * m) / (np.sqrt(v) + f(eps))).astype(f), m, v


def lr_factor(schedule, step):
    """training.lr_factor written out again (float64): linear warm-up over steps 0 .. warmup_steps - 1 from 1 / warmup_steps to
    1, then the kind on t = step - warmup_steps."""
    if schedule is None:
        return 1.0
    w = schedule.get("warmup_steps", 0)
    if step < w:
        return (step + 1) / w
    t = step - w
    kind = schedule.get("kind", "constant")
    if kind == "cosine":
        T = schedule["total_steps"] - w
        mf = schedule.get("min_factor", 0.0)
        return mf if t >= T else mf + (1 - mf) * (1 + math.cos(math.pi * t / T)) / 2
    if kind == "step":
        return schedule["gamma"] ** (t // schedule["step_size"])
    if kind == "exponential":
        return schedule["gamma"] ** t
    return 1.0
