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

Frozen variables (fine-tuning part of the network) and input-only gradients (a frozen separator as a front end or a loss term):

    net.freeze([n for n in net.variable_names() if ...])   # e.g. the encoder; unfreeze(names), frozen()
    net.arena.requires_grad_(False)                         # and a mix that requires grad: only d loss / d mix is computed

The backward pass then runs wun_backward_select: launches no wanted gradient needs are skipped, and the frozen ranges of
arena.grad are 0, as the padding floats are.  A torch optimizer still steps every float of the one arena Parameter: with
weight decay (AdamW, Adam(weight_decay=...)) or momentum left over from earlier steps it moves frozen variables too.  The
separator's own adam_step(variables=...) leaves them bit-unchanged.
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
    def forward(ctx, mix, arena, sep, mask=None):
        outs, key, gen = _forward(sep, arena, mix, True)
        ctx.sep, ctx.key, ctx.gen, ctx.mix_shape, ctx.mask = sep, key, gen, tuple(mix.shape), mask
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
        want_arena = ctx.needs_input_grad[1]
        # padding floats (and frozen ranges) stay 0 for torch optimizers
        grads = torch.zeros_like(arena) if want_arena else None
        d_mix = torch.empty(ctx.mix_shape, dtype=torch.float32, device=arena.device) if ctx.needs_input_grad[0] else None
        dout = d_outputs.to(torch.float32).contiguous()
        plan = sep._plans[key]
        mask = ctx.mask
        if not want_arena:
            mask = np.zeros(len(plan.tensors), dtype=np.uint8)          # input-only gradient
        if mask is None:
            _lib.check(sep._lib.wun_backward(plan.handle, arena.data_ptr(), None, sep._ws[key].data_ptr(), outs.data_ptr(),
                                             dout.data_ptr(), grads.data_ptr(),
                                             d_mix.data_ptr() if d_mix is not None else None, sep._stream()))
        elif mask.any() or d_mix is not None:
            sel, n = sep._mask_arg(mask)
            _lib.check(sep._lib.wun_backward_select(
                plan.handle, arena.data_ptr(), None, sep._ws[key].data_ptr(), outs.data_ptr(), dout.data_ptr(),
                grads.data_ptr() if mask.any() else None, d_mix.data_ptr() if d_mix is not None else None, sep._stream(),
                None, None, 0, sel, n))
        return d_mix, grads, None, None


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
        self._frozen = set()

    def variable_names(self):
        """The TF variable names, in arena order."""
        return [name for name, _, _ in self.tensors]

    def _names(self, names):
        names = [names] if isinstance(names, str) else list(names)
        known = set(self.variable_names())
        for n in names:
            if n not in known:
                raise KeyError(n)
        return names

    def freeze(self, names):
        """Stop computing the gradients of these TF variables (their ranges of arena.grad are 0).  A conv's kernel and bias
        must be frozen together, and the output layer's convs together: else the backward pass raises NotImplementedError."""
        self._frozen.update(self._names(names))

    def unfreeze(self, names):
        for n in self._names(names):
            self._frozen.discard(n)

    def frozen(self):
        """The frozen TF variable names, in arena order."""
        return [n for n in self.variable_names() if n in self._frozen]

    def forward(self, mix):
        self.sep._refuse_in_ema("the autograd module's forward (it runs on its own arena, the trained weights)")
        dev = self.arena.device
        if not torch.is_tensor(mix):
            mix = torch.as_tensor(np.asarray(mix, dtype=np.float32))
        mix = mix.to(device=dev, dtype=torch.float32).contiguous()
        if not self.training:
            with torch.no_grad():
                return _forward(self.sep, self.arena, mix, False)[0]
        mask = None
        if self._frozen:
            mask = np.array([0 if n in self._frozen else 1 for n in self.variable_names()], dtype=np.uint8)
        return GetOutput.apply(mix, self.arena, self.sep, mask)

    def ema_update(self, decay, warmup=False, variables=None, step=None):
        """After the user's optimizer.step(): the separator's EMA of the weights moves towards the arena (sep.ema_update,
        wun_ema_update; the EMA arena starts as a copy of the weights at the first call).  step: TF's num_updates, needed for
        warmup=True -- the caller's own count of optimizer steps, which it keeps (and checkpoints) with its torch optimizer;
        the module keeps no counter.  sep.ema_variables() reads the EMA.  sep.ema_weights() serves the SEPARATOR's own calls
        (get_output, separate_track, validation): this module's forward takes `arena`, the trained Parameter, so it is
        refused inside that block rather than run quietly on the trained weights."""
        if warmup and step is None:
            raise ValueError("ema_update(warmup=True) needs step = the number of optimizer steps made so far")
        with torch.no_grad():
            self.sep.ema_update(decay, warmup=warmup, variables=variables, step=0 if step is None else step)

    def named_variables(self):
        """tf_name -> view of the arena (the TF variables, UnetAudioSeparator.py)."""
        return {name: self.arena[off:off + int(np.prod(shp))].view(*shp) for name, off, shp in self.tensors}

    def variable_grads(self):
        """tf_name -> view of arena.grad (after backward), or None."""
        g = self.arena.grad
        if g is None:
            return None
        return {name: g[off:off + int(np.prod(shp))].view(*shp) for name, off, shp in self.tensors}
