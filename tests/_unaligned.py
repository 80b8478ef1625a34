"""A tensor at a base pointer that is 4-byte but not 8-byte aligned, for the GPU tests of the STFT family: the kernels gather
with scalar loads and must give the same bits from any float address."""
import torch


def _offset_copy(x):
    """A copy of x whose base pointer lies one float behind an allocation's start."""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    v = buf[1:].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 8 == 4 and v.is_contiguous()
    return v


def _offset_full(shape, value, dtype=torch.float32, device="cuda"):
    """An output view at such a pointer, every element `value` (NaN: an element the kernel leaves unwritten shows)."""
    n = 1
    for s in shape:
        n *= int(s)
    buf = torch.full((n + 1,), value, dtype=dtype, device=device)
    v = buf[1:].view(*shape)
    assert v.data_ptr() % 8 == 4 and v.is_contiguous()
    return v
