"""get_output under torch.autograd: the separator as a torch.nn.Module whose backward pass is wun_backward (include/wun.h).

    sep = UnetAudioSeparator(cfg)
    net = sep.module()                      # WaveUNet; net.arena is ONE nn.Parameter sharing storage with sep.params
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    y = net(mix)                            # [S, B, Tout, C], a fresh tensor per call
    loss = any_function_of(y)               # L1, weighted per source, spectral, ... (the reference: Training.py:50-63)
    loss.backward(); opt.step()             # d loss / d arena (padding floats 0) and, if mix requires grad, d loss / d mix

The separator keeps ONE workspace per (batch, frames): the activations the backward pass reads.  A second forward pass of
the same shape before the first one's backward overwrites them, so that backward raises RuntimeError instead of computing
wrong gradients (generation counter per workspace).  An in-place change of the arena between forward and backward trips
torch's own version check (the arena is saved for backward).  Second-order gradients are not supported (once_differentiable).
"""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib


def _forward(sep, arena, mix, training):
    """wun_forward into a newly allocated output tensor; returns (outputs, workspace key, generation)."""
    if mix.dim() != 3 or mix.shape[2] != sep.num_channels:
        raise ValueError("input must be [batch, samples, %d]" % sep.num_channels)
    plan = sep._plan(mix.shape[0], mix.shape[1])
    key = (int(mix.shape[0]), int(mix.shape[1]))
    shape = (len(sep.source_names), key[0], int(plan.info.output_frames), sep.num_channels)
    if key not in sep._ws:                   # (the separator's get_output allocates the same pair)
        sep._ws[key] = torch.empty(int(plan.info.workspace_floats), dtype=torch.float32, device=mix.device)
        sep._outs[key] = torch.empty(shape, dtype=torch.float32, device=mix.device)
    outs = torch.empty(shape, dtype=torch.float32, device=mix.device)
    _lib.check(sep._lib.wun_forward(plan.handle, arena.data_ptr(), mix.data_ptr(), sep._ws[key].data_ptr(),
                                    outs.data_ptr(), 1 if training else 0, sep._stream()))
    sep._ws_gen[key] = sep._ws_gen.get(key, 0) + 1
    # activation() now reads this workspace; the separator's own loss_and_gradients / backward refuse until its next
    # get_output(training=True) (they read the separator's output buffer, which this pass did not write)
    sep._active, sep._last_key, sep._last_training = plan, key, False
    return outs, key, sep._ws_gen[key]


class GetOutput(torch.autograd.Function):
    """outputs [S, B, Tout, C] = get_output(mix [B, Tin, C], training = True) with the parameters in `arena`."""

    @staticmethod
    def forward(ctx, mix, arena, sep):
        outs, key, gen = _forward(sep, arena, mix, True)
        ctx.sep, ctx.key, ctx.gen, ctx.mix_shape = sep, key, gen, tuple(mix.shape)
        ctx.save_for_backward(arena, outs)
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, d_outputs):
        arena, outs = ctx.saved_tensors          # (torch's version check: the arena must not change before backward)
        sep, key = ctx.sep, ctx.key
        if sep._ws_gen.get(key) != ctx.gen:
            raise RuntimeError("wave_u_net_amd: another forward pass of shape %s ran on the shared workspace after this "
                               "one; run backward before the next forward of the same shape" % (key,))
        grads = torch.zeros_like(arena)          # padding floats stay 0 for torch optimizers
        d_mix = torch.empty(ctx.mix_shape, dtype=torch.float32, device=arena.device) if ctx.needs_input_grad[0] else None
        dout = d_outputs.to(torch.float32).contiguous()
        plan = sep._plans[key]
        _lib.check(sep._lib.wun_backward(plan.handle, arena.data_ptr(), None, sep._ws[key].data_ptr(), outs.data_ptr(),
                                         dout.data_ptr(), grads.data_ptr(),
                                         d_mix.data_ptr() if d_mix is not None else None, sep._stream()))
        return d_mix, grads, None


class WaveUNet(torch.nn.Module):
    """A UnetAudioSeparator as a torch.nn.Module.  forward(mix [B, Tin, C]) -> [S, B, Tout, C] (source_names order).
    train(): differentiable w.r.t. `arena` and (if it requires grad) `mix`; eval(): training = 0 (AudioClip active,
    Utils.py:82-92), the output does not require grad."""

    def __init__(self, sep):
        super().__init__()
        self.sep = sep
        plan = sep._any_plan()
        sep._ensure_variables(plan)
        self.arena = torch.nn.Parameter(sep.params, requires_grad=True)    # shares storage with sep.params
        assert self.arena.data_ptr() == sep.params.data_ptr()
        self.tensors = list(plan.tensors)

    def forward(self, mix):
        dev = self.arena.device
        if not torch.is_tensor(mix):
            mix = torch.as_tensor(np.asarray(mix, dtype=np.float32))
        mix = mix.to(device=dev, dtype=torch.float32).contiguous()
        if not self.training:
            with torch.no_grad():
                return _forward(self.sep, self.arena, mix, False)[0]
        return GetOutput.apply(mix, self.arena, self.sep)

    def named_variables(self):
        """tf_name -> view of the arena (the TF variables, UnetAudioSeparator.py)."""
        return {name: self.arena[off:off + int(np.prod(shp))].view(*shp) for name, off, shp in self.tensors}

    def variable_grads(self):
        """tf_name -> view of arena.grad (after backward), or None."""
        g = self.arena.grad
        if g is None:
            return None
        return {name: g[off:off + int(np.prod(shp))].view(*shp) for name, off, shp in self.tensors}
