"""CPU-only checks of wun_backward_select / wun_loss_backward_select / wun_adam_step_select (include/wun.h): declared, exported,
bound, and refusing bad selections with WUN_ERR_INVALID / WUN_ERR_UNSUPPORTED before any GPU work -- on a plan built without a
GPU -- and the separator's variable names."""
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
def sep():
    s = UnetAudioSeparator(wun.get_config("baseline", num_layers=3, num_initial_filters=8, context=True,
                                          upsampling="learned", output_type="difference", task="multi_instrument"))
    i, _ = s.get_padding(np.array([2, 300, 0]))
    s._active = s._plan(2, int(i[1]))
    return s


@pytest.fixture(scope="module")
def plan(sep):
    return sep._active


# A non-null pointer that is never dereferenced: every call below must fail its argument check first.
_FAKE = C.c_void_p(0x1000)


def _mask(bits):
    m = np.asarray(bits, dtype=np.uint8)
    return m, m.ctypes.data_as(C.POINTER(C.c_uint8))


def _bwd(lib, plan, mask, n=None, grads=_FAKE, dmix=None, handle=True):
    m, ptr = _mask(mask) if mask is not None else (None, None)
    n = (len(m) if m is not None else 0) if n is None else n
    return lib.wun_backward_select(plan.handle if handle else None, _FAKE, None, _FAKE, _FAKE, _FAKE, grads, dmix, None,
                                   None, None, 0, ptr, n)


def _loss(lib, plan, mask, n=None, handle=True):
    m, ptr = _mask(mask) if mask is not None else (None, None)
    n = (len(m) if m is not None else 0) if n is None else n
    return lib.wun_loss_backward_select(plan.handle if handle else None, _FAKE, None, _FAKE, _FAKE, _FAKE, _FAKE, _FAKE, None,
                                        None, None, 0, ptr, n)


def _adam(lib, plan, mask, n=None, step=1, handle=True):
    m, ptr = _mask(mask) if mask is not None else (None, None)
    n = (len(m) if m is not None else 0) if n is None else n
    return lib.wun_adam_step_select(plan.handle if handle else None, _FAKE, _FAKE, _FAKE, _FAKE, step, 1e-3, 0.9, 0.999, 1e-8,
                                    1.0, None, ptr, n)


def _names(plan):
    return [n for n, _, _ in plan.tensors]


def test_null_plan_is_invalid(lib, plan):
    nt = len(plan.tensors)
    assert _bwd(lib, plan, [1] * nt, handle=False) == WUN_ERR_INVALID
    assert _loss(lib, plan, [1] * nt, handle=False) == WUN_ERR_INVALID
    assert _adam(lib, plan, [1] * nt, handle=False) == WUN_ERR_INVALID


@pytest.mark.parametrize("delta", [-1, 1])
def test_wrong_nselect_is_invalid(lib, plan, delta):
    nt = len(plan.tensors)
    mask = [1] * (nt + 1)
    for call in (_bwd, _loss, _adam):
        assert call(lib, plan, mask, n=nt + delta) == WUN_ERR_INVALID, call
        assert "nselect" in lib.wun_last_error().decode()
    # a NULL mask with a count that is neither 0 nor num_tensors
    for call in (_bwd, _loss, _adam):
        assert call(lib, plan, None, n=3) == WUN_ERR_INVALID, call


def test_kernel_bias_mismatch_is_unsupported(lib, plan):
    names = _names(plan)
    k = names.index("separator/conv1d_1/kernel")
    mask = [0] * len(names)
    mask[k] = 1                                                  # kernel without its bias
    assert _bwd(lib, plan, mask) == WUN_ERR_UNSUPPORTED
    assert "separator/conv1d_1/kernel" in lib.wun_last_error().decode()
    assert _loss(lib, plan, mask) == WUN_ERR_UNSUPPORTED
    mask = [0] * len(names)
    mask[k + 1] = 1                                              # bias without its kernel
    assert _bwd(lib, plan, mask, dmix=_FAKE) == WUN_ERR_UNSUPPORTED
    # Adam takes any subset: the same mask gets past the selection check (and then refuses step 0, still before the GPU)
    assert _adam(lib, plan, mask, step=0) == WUN_ERR_INVALID
    assert "1-based" in lib.wun_last_error().decode()


def test_output_layer_convs_are_selected_together(lib, plan):
    names = _names(plan)
    heads = [k for k, n in enumerate(names) if n.endswith("/kernel")][-2:]   # difference output of 3 sources: 2 output convs
    mask = [0] * len(names)
    mask[heads[0]] = mask[heads[0] + 1] = 1
    assert _bwd(lib, plan, mask) == WUN_ERR_UNSUPPORTED
    assert "output layer" in lib.wun_last_error().decode()


def test_nothing_selected_needs_d_mix(lib, plan):
    nt = len(plan.tensors)
    assert _bwd(lib, plan, [0] * nt) == WUN_ERR_INVALID
    assert "nothing to compute" in lib.wun_last_error().decode()
    assert _bwd(lib, plan, [0] * nt, grads=None) == WUN_ERR_INVALID
    assert _loss(lib, plan, [0] * nt) == WUN_ERR_INVALID       # (the loss call has no d_mix)


def test_null_grads_needs_an_empty_selection(lib, plan):
    nt = len(plan.tensors)
    names = _names(plan)
    k = names.index("separator/interp_0")
    one = [0] * nt
    one[k] = 1
    for m in (one, [1] * nt):
        assert _bwd(lib, plan, m, grads=None) == WUN_ERR_INVALID
        assert "grads" in lib.wun_last_error().decode()
        assert _bwd(lib, plan, m, grads=None, dmix=_FAKE) == WUN_ERR_INVALID
    assert _bwd(lib, plan, None, grads=None, dmix=_FAKE) == WUN_ERR_INVALID      # NULL mask = every tensor


def test_null_required_pointers_are_invalid(lib, plan):
    nt = len(plan.tensors)
    m, ptr = _mask([1] * nt)
    assert lib.wun_backward_select(plan.handle, _FAKE, None, _FAKE, _FAKE, None, _FAKE, None, None, None, None, 0,
                                   ptr, nt) == WUN_ERR_INVALID
    assert lib.wun_loss_backward_select(plan.handle, _FAKE, None, _FAKE, _FAKE, _FAKE, _FAKE, None, None, None, None, 0,
                                        ptr, nt) == WUN_ERR_INVALID
    assert lib.wun_adam_step_select(plan.handle, _FAKE, None, _FAKE, _FAKE, 1, 1e-3, 0.9, 0.999, 1e-8, 1.0, None,
                                    ptr, nt) == WUN_ERR_INVALID


def test_bad_buckets_are_invalid(lib, plan):
    nt = len(plan.tensors)
    m, ptr = _mask([1] * nt)
    st = (C.c_int64 * 2)(100, 100)
    ev = (C.c_void_p * 2)(0x2000, 0x2000)
    assert lib.wun_backward_select(plan.handle, _FAKE, None, _FAKE, _FAKE, _FAKE, _FAKE, None, None, st, ev, 2,
                                   ptr, nt) == WUN_ERR_INVALID
    assert "descending" in lib.wun_last_error().decode()


def test_unknown_variable_names_raise_key_error(sep):
    names = _names(sep._active)
    assert sep.select_mask(None) is None
    m = sep.select_mask([names[3], names[0]])
    assert m.dtype == np.uint8 and list(np.flatnonzero(m)) == [0, 3]
    assert sep.select_mask(names[2]).sum() == 1
    assert sep.select_mask([]).sum() == 0
    with pytest.raises(KeyError):
        sep.select_mask(["separator/conv1d_99/kernel"])
    # every public entry point resolves the names first
    with pytest.raises(KeyError):
        sep.backward(None, input_grad=True, variables=["nope"])
    with pytest.raises(KeyError):
        sep.loss_and_gradients(None, variables=["nope"])
    with pytest.raises(KeyError):
        sep.adam_step(1e-3, variables=["nope"])


def test_autograd_freeze_api_exists():
    from wave_u_net_amd.autograd import WaveUNet
    for name in ("freeze", "unfreeze", "frozen", "variable_names"):
        assert callable(getattr(WaveUNet, name))
