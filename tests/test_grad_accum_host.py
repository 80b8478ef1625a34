"""CPU-only checks of gradient accumulation (include/wun.h: wun_backward_accumulate, wun_loss_backward_accumulate): declared,
exported, bound with the _select calls' 14 arguments, and refusing bad arguments with WUN_ERR_INVALID / WUN_ERR_UNSUPPORTED
before any GPU work -- on a plan built without a GPU -- plus the Trainer's grad_accum_steps argument checks."""
import ctypes as C

import numpy as np
import pytest

import wave_u_net_amd as wun
from wave_u_net_amd import _lib
from wave_u_net_amd.separator import UnetAudioSeparator

WUN_ERR_INVALID, WUN_ERR_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def plan():
    s = UnetAudioSeparator(wun.get_config("baseline", num_layers=3, num_initial_filters=8, context=True,
                                          upsampling="learned", output_type="difference", task="multi_instrument"))
    i, _ = s.get_padding(np.array([2, 300, 0]))
    return s._plan(2, int(i[1]))


# A non-null pointer that is never dereferenced: every call below must fail its argument check first.
_FAKE = C.c_void_p(0x1000)


def _mask(bits):
    m = np.asarray(bits, dtype=np.uint8)
    return m, m.ctypes.data_as(C.POINTER(C.c_uint8))


def _bwd(lib, plan, mask, n=None, grads=_FAKE, dmix=None, handle=True, buckets=(None, None, 0)):
    m, ptr = _mask(mask) if mask is not None else (None, None)
    n = (len(m) if m is not None else 0) if n is None else n
    return lib.wun_backward_accumulate(plan.handle if handle else None, _FAKE, None, _FAKE, _FAKE, _FAKE, grads, dmix, None,
                                       *buckets, ptr, n)


def _loss(lib, plan, mask, n=None, grads=_FAKE, handle=True, buckets=(None, None, 0)):
    m, ptr = _mask(mask) if mask is not None else (None, None)
    n = (len(m) if m is not None else 0) if n is None else n
    return lib.wun_loss_backward_accumulate(plan.handle if handle else None, _FAKE, None, _FAKE, _FAKE, _FAKE, grads, _FAKE,
                                            None, *buckets, ptr, n)


def _names(plan):
    return [n for n, _, _ in plan.tensors]


def test_null_plan_is_invalid(lib, plan):
    nt = len(plan.tensors)
    for call in (_bwd, _loss):
        assert call(lib, plan, [1] * nt, handle=False) == WUN_ERR_INVALID, call
        assert call(lib, plan, None, handle=False) == WUN_ERR_INVALID, call


def test_bad_buckets_are_invalid(lib, plan):
    nt = len(plan.tensors)
    st = (C.c_int64 * 2)(100, 100)
    ev = (C.c_void_p * 2)(0x2000, 0x2000)
    for call in (_bwd, _loss):
        assert call(lib, plan, [1] * nt, buckets=(st, ev, 2)) == WUN_ERR_INVALID, call
        assert "descending" in lib.wun_last_error().decode()
        assert call(lib, plan, None, buckets=(None, None, 2)) == WUN_ERR_INVALID, call
        assert call(lib, plan, None, buckets=(st, ev, -1)) == WUN_ERR_INVALID, call


@pytest.mark.parametrize("delta", [-1, 1])
def test_wrong_nselect_is_invalid(lib, plan, delta):
    nt = len(plan.tensors)
    mask = [1] * (nt + 1)
    for call in (_bwd, _loss):
        assert call(lib, plan, mask, n=nt + delta) == WUN_ERR_INVALID, call
        assert "nselect" in lib.wun_last_error().decode()
        assert call(lib, plan, None, n=3) == WUN_ERR_INVALID, call        # NULL mask: 0 or num_tensors only


def test_null_grads_with_a_selection_is_invalid(lib, plan):
    nt = len(plan.tensors)
    one = [0] * nt
    one[_names(plan).index("separator/interp_0")] = 1
    for m in (one, [1] * nt, None):
        assert _bwd(lib, plan, m, grads=None) == WUN_ERR_INVALID
        assert _bwd(lib, plan, m, grads=None, dmix=_FAKE) == WUN_ERR_INVALID
        assert _loss(lib, plan, m, grads=None) == WUN_ERR_INVALID
    # nothing selected and no d_mix: nothing to compute
    assert _bwd(lib, plan, [0] * nt) == WUN_ERR_INVALID
    assert "nothing to compute" in lib.wun_last_error().decode()
    assert _loss(lib, plan, [0] * nt) == WUN_ERR_INVALID


def test_kernel_and_bias_selected_apart_is_unsupported(lib, plan):
    names = _names(plan)
    k = names.index("separator/conv1d_1/kernel")
    for off in (0, 1):                                           # kernel without its bias, bias without its kernel
        mask = [0] * len(names)
        mask[k + off] = 1
        assert _bwd(lib, plan, mask) == WUN_ERR_UNSUPPORTED
        assert "separator/conv1d_1/kernel" in lib.wun_last_error().decode()
        assert _loss(lib, plan, mask) == WUN_ERR_UNSUPPORTED
        assert _bwd(lib, plan, mask, dmix=_FAKE) == WUN_ERR_UNSUPPORTED
    heads = [i for i, n in enumerate(names) if n.endswith("/kernel")][-2:]   # two output convs: selected together only
    mask = [0] * len(names)
    mask[heads[0]] = mask[heads[0] + 1] = 1
    assert _bwd(lib, plan, mask) == WUN_ERR_UNSUPPORTED
    assert "output layer" in lib.wun_last_error().decode()


def test_separator_and_trainer_take_the_accumulate_arguments():
    import inspect
    from wave_u_net_amd.training import Trainer
    for meth in (UnetAudioSeparator.loss_and_gradients, UnetAudioSeparator.backward):
        p = inspect.signature(meth).parameters["accumulate"]
        assert p.default is False
    assert inspect.signature(Trainer.__init__).parameters["grad_accum_steps"].default is None
