"""CPU-only checks of wun_backward / wun_backward_ex (include/wun.h): declared, exported, bound, and refusing bad arguments
with WUN_ERR_INVALID before any GPU work -- on a plan built without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import wave_u_net_amd as wun
from wave_u_net_amd import _lib
from wave_u_net_amd.separator import UnetAudioSeparator

WUN_ERR_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def plan(lib):
    sep = UnetAudioSeparator(wun.get_config("baseline", num_layers=3, num_initial_filters=8, context=True))
    i, _ = sep.get_padding(np.array([2, 300, 0]))
    return sep._plan(2, int(i[1]))


# A non-null pointer that is never dereferenced: every call below must fail its argument check first.
_FAKE = C.c_void_p(0x1000)


def _call(lib, plan, **null):
    args = dict(params=_FAKE, mix=_FAKE, ws=_FAKE, outs=_FAKE, dout=_FAKE, grads=_FAKE, dmix=None)
    args.update(null)
    return lib.wun_backward(plan.handle, args["params"], args["mix"], args["ws"], args["outs"], args["dout"],
                            args["grads"], args["dmix"], None)


@pytest.mark.parametrize("which", ["dout", "grads", "ws", "outs", "params"])
def test_null_required_pointer_is_invalid(lib, plan, which):
    assert _call(lib, plan, **{which: None}) == WUN_ERR_INVALID
    assert "null" in lib.wun_last_error().decode()
    # ... also when d_mix is asked for
    assert _call(lib, plan, **{which: None, "dmix": _FAKE}) == WUN_ERR_INVALID


def test_null_plan_is_invalid(lib):
    assert lib.wun_backward(None, _FAKE, _FAKE, _FAKE, _FAKE, _FAKE, _FAKE, None, None) == WUN_ERR_INVALID


def test_bad_buckets_are_invalid(lib, plan):
    def ex(starts, n, events=True):
        st = (C.c_int64 * max(len(starts), 1))(*(starts or [0]))
        ev = (C.c_void_p * max(len(starts), 1))(*([0x2000] * max(len(starts), 1))) if events else None
        return lib.wun_backward_ex(plan.handle, _FAKE, _FAKE, _FAKE, _FAKE, _FAKE, _FAKE, None, None, st, ev, n)
    assert ex([100, 100], 2) == WUN_ERR_INVALID                 # not strictly descending
    assert "descending" in lib.wun_last_error().decode()
    assert ex([10, 100], 2) == WUN_ERR_INVALID
    assert ex([100], -1) == WUN_ERR_INVALID
    assert ex([100], 1, events=False) == WUN_ERR_INVALID        # buckets without events


def test_separator_backward_needs_a_training_forward():
    sep = UnetAudioSeparator(wun.get_config("baseline", num_layers=3, num_initial_filters=8))
    with pytest.raises(RuntimeError):
        sep.backward(torch.zeros(2, 1, 4, 2))


def test_autograd_module_is_importable():
    from wave_u_net_amd.autograd import GetOutput, WaveUNet
    assert issubclass(WaveUNet, torch.nn.Module)
    assert issubclass(GetOutput, torch.autograd.Function)
    assert hasattr(UnetAudioSeparator, "module") and hasattr(UnetAudioSeparator, "backward")
