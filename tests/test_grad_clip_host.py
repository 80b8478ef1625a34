"""CPU-only checks of gradient-norm clipping (include/wun.h: wun_grad_norm_workspace_floats, wun_grad_norm, wun_adam_step_clip):
declared, exported and bound; the norm workspace size; every argument error refused with WUN_ERR_INVALID before any GPU work
-- on a plan built without a GPU -- plus the clip_norm / clip_grad_norm checks of adam_step and the Trainer."""
import ctypes as C
import math

import numpy as np
import pytest

import wave_u_net_amd as wun
from wave_u_net_amd import _lib
from wave_u_net_amd.separator import UnetAudioSeparator, check_clip_norm
from wave_u_net_amd.training import clip_settings

WUN_ERR_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def plan():
    s = UnetAudioSeparator(wun.get_config("baseline", num_layers=3, num_initial_filters=8, context=True,
                                          upsampling="learned", output_type="difference", task="multi_instrument"))
    i, _ = s.get_padding(np.array([2, 300, 0]))
    return s._plan(2, int(i[1]))


def test_workspace_floats(lib, plan):
    nt = len(plan.tensors)
    n = lib.wun_grad_norm_workspace_floats(plan.handle)
    assert n >= nt + 1
    # at least one float64 partial (two floats) per tensor
    assert n >= nt + 1 + 2 * nt
    # chunks of at most 8192 floats that never cross a tensor boundary
    chunks = sum(-(-int(np.prod(shp)) // 8192) for _, _, shp in plan.tensors)
    assert n == ((nt + 2) & ~1) + 2 * chunks
    assert lib.wun_grad_norm_workspace_floats(None) == WUN_ERR_INVALID


# Non-null pointers that are never dereferenced: every call below must fail its argument check first.
_FAKE = C.c_void_p(0x1000)
_FAKE_MISALIGNED = C.c_void_p(0x1004)


def _mask(bits):
    m = np.asarray(bits, dtype=np.uint8)
    return m, m.ctypes.data_as(C.POINTER(C.c_uint8))


def _norm(lib, plan, mask=None, n=None, grads=_FAKE, ws=_FAKE, handle=True):
    m, ptr = _mask(mask) if mask is not None else (None, None)
    n = (len(m) if m is not None else 0) if n is None else n
    return lib.wun_grad_norm(plan.handle if handle else None, grads, 1.0, ws, None, ptr, n)


def _clip(lib, plan, mask=None, n=None, step=1, clip=1.0, flags=1, ws=_FAKE, skipped=_FAKE, handle=True,
          ptrs=(_FAKE, _FAKE, _FAKE, _FAKE)):
    m, ptr = _mask(mask) if mask is not None else (None, None)
    n = (len(m) if m is not None else 0) if n is None else n
    return lib.wun_adam_step_clip(plan.handle if handle else None, *ptrs, step, 1e-4, 0.9, 0.999, 1e-8, 1.0, clip, flags,
                                  ws, skipped, None, ptr, n)


def test_grad_norm_argument_errors(lib, plan):
    nt = len(plan.tensors)
    assert _norm(lib, plan, handle=False) == WUN_ERR_INVALID
    assert _norm(lib, plan, grads=None) == WUN_ERR_INVALID
    assert _norm(lib, plan, ws=None) == WUN_ERR_INVALID
    assert _norm(lib, plan, ws=_FAKE_MISALIGNED) == WUN_ERR_INVALID
    assert _norm(lib, plan, None, n=nt - 1) == WUN_ERR_INVALID            # NULL select: nselect 0 or num_tensors
    assert _norm(lib, plan, [1] * nt, n=nt - 1) == WUN_ERR_INVALID
    assert _norm(lib, plan, [1] * (nt + 1)) == WUN_ERR_INVALID
    assert "nselect" in lib.wun_last_error().decode()


def test_adam_step_clip_argument_errors(lib, plan):
    nt = len(plan.tensors)
    assert _clip(lib, plan, handle=False) == WUN_ERR_INVALID
    for i in range(4):                                                    # params, grads, m, v
        ptrs = [_FAKE] * 4
        ptrs[i] = None
        assert _clip(lib, plan, ptrs=tuple(ptrs)) == WUN_ERR_INVALID, i
    assert _clip(lib, plan, ws=None) == WUN_ERR_INVALID
    assert _clip(lib, plan, ws=_FAKE_MISALIGNED) == WUN_ERR_INVALID
    for clip in (0.0, -1.0, -math.inf, math.nan):
        assert _clip(lib, plan, clip=clip) == WUN_ERR_INVALID, clip
        assert "clip_norm" in lib.wun_last_error().decode()
    assert _clip(lib, plan, step=0) == WUN_ERR_INVALID
    assert _clip(lib, plan, step=-3) == WUN_ERR_INVALID
    assert _clip(lib, plan, flags=2) == WUN_ERR_INVALID
    assert _clip(lib, plan, skipped=None) == WUN_ERR_INVALID              # skipping asks for the counter
    assert "skipped" in lib.wun_last_error().decode()
    assert _clip(lib, plan, None, n=3) == WUN_ERR_INVALID
    assert _clip(lib, plan, [1] * nt, n=nt + 1) == WUN_ERR_INVALID
    assert _clip(lib, plan, [0] * (nt - 1)) == WUN_ERR_INVALID


def test_check_clip_norm():
    assert check_clip_norm(None) == math.inf
    assert check_clip_norm(1) == 1.0
    assert check_clip_norm(math.inf) == math.inf
    for bad in (0, 0.0, -1.0, math.nan, -math.inf, "x", True):
        with pytest.raises(ValueError):
            check_clip_norm(bad)


def test_trainer_clip_settings():
    cfg = wun.get_config("baseline")
    assert "clip_grad_norm" not in cfg and "skip_nonfinite_steps" not in cfg
    assert clip_settings(cfg) == (None, False)
    assert clip_settings(cfg, clip_grad_norm=5.0) == (5.0, False)
    assert clip_settings(cfg, skip_nonfinite=True) == (None, True)
    assert clip_settings(dict(cfg, clip_grad_norm=1.0, skip_nonfinite_steps=True)) == (1.0, True)
    assert clip_settings(dict(cfg, clip_grad_norm=1.0), clip_grad_norm=2.0) == (2.0, False)
    for bad in (0.0, -2.0, math.nan, "abc"):
        with pytest.raises(ValueError, match="clip_grad_norm"):
            clip_settings(cfg, clip_grad_norm=bad)
        with pytest.raises(ValueError, match="clip_grad_norm"):
            clip_settings(dict(cfg, clip_grad_norm=bad))


def test_cli_override_reaches_the_trainer():
    from wave_u_net_amd.__main__ import _parse
    from wave_u_net_amd.training import clip_settings
    cmd, name, over, _ = _parse(["train", "with", "cfg.full", "model_config.clip_grad_norm=1.0",
                                 "model_config.skip_nonfinite_steps=True"])
    assert clip_settings(wun.get_config(name, **over)) == (1.0, True)
