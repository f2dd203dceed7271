"""The parameter store of every hand-written trainer, and the optimizer bookkeeping that goes with it.

All trained parameters live in ONE flat float32 buffer (the masters).  The gradient, the optimizer moments and, where asked for, a bf16
mirror are flat buffers of the same layout, so an overflow check, a norm or an optimizer update is one launch over `size` elements
(padding included: it is zero and stays zero).  Every entry starts on a multiple of `pad` elements; an entry may reserve more than
its numel, and may be stored in another order than the one the model sees (a layout).  The model's parameters become views of the
masters, so nothing is copied between "the model's weights" and "the trainer's weights"."""
import math

import numpy as np
import torch

# nn.Adam's default betas as the float32 values the kernels work with: the host's bias correction must use the same ones (1 - 0.999f
# is 4.7e-5 above 0.001, which would be 2.3e-5 of every step)
ADAM_BETA1, ADAM_BETA2 = float(np.float32(0.9)), float(np.float32(0.999))


def adam_lr_t(lr, t, beta1, beta2):
    """The learning rate of Adam's step t (from 1) with both bias corrections folded in."""
    return lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)


class DynamicLossScale:
    """DynamicLossScaleUpdateCell(loss_scale_value, scale_factor, scale_window) (train.py:126-129): halve (min 1) on
    overflow, double after `scale_window` consecutive clean steps."""

    def __init__(self, init=1024.0, factor=2.0, window=1000):
        self.scale, self.factor, self.window, self.good = float(init), float(factor), int(window), 0

    def update(self, overflow):
        if overflow:
            self.scale = max(self.scale / self.factor, 1.0)
            self.good = 0
        else:
            self.good += 1
            if self.good >= self.window:
                self.scale *= self.factor
                self.good = 0


# ---- storage layouts: (the entry's 1-D slice, the shape the model sees) -> the view the model sees --------------------------------------
def stored_last_first(v, shape):
    """Stored (last, first), seen as (first, 1, last): a one-input-channel convolution kept tap-major, as its kernel reads it."""
    return v.view(shape[2], shape[0]).t().unsqueeze(1)


def stored_taps_inner(v, shape):
    """Stored (N, taps, C), the operand order of a convolution run as products, seen as (N, C, taps)."""
    return v.view(shape[0], shape[2], shape[1]).permute(0, 2, 1)


class FlatParams:
    """Name -> (offset, shape, numel) views into flat float32 / bf16 buffers.

    entries: (name, shape[, layout[, reserved]]) in flat order; `layout` one of the functions above (None: stored as seen), `reserved`
        an element count of at least numel that the entry occupies (rounded up to `pad` like numel).
    moments: names of further zero-filled float32 buffers of the same layout, reachable as attributes; a name is also the prefix of its
        checkpoint keys ("<moment>.<parameter>").
    mirror_bf16: `bf16` is a bf16 copy of the masters' layout (the matmul operands of the throughput mode), else the masters themselves."""

    def __init__(self, entries, device, mirror_bf16=True, pad=64, moments=("exp_avg", "exp_avg_sq")):
        self.index, self.pad, self.moments = {}, pad, tuple(moments)
        self._layout, self._reserved = {}, {}
        off = 0
        for name, shape, *more in entries:
            n = 1
            for s in shape:
                n *= s
            self.index[name] = (off, tuple(shape), n)
            if more and more[0] is not None:
                self._layout[name] = more[0]
            self._reserved[name] = (max([n] + more[1:]) + pad - 1) // pad * pad
            off += self._reserved[name]
        self.size = off
        self.master = torch.zeros(off, dtype=torch.float32, device=device)
        # (one allocation: the flat gradient and, behind it, the step's overflow flag - one fill zeroes both)
        self._grad_alloc = torch.zeros(off + 64, dtype=torch.float32, device=device)
        self.grad = self._grad_alloc[:off]
        self.flag = self._grad_alloc[off:off + 1].view(torch.int32)
        for m in self.moments:
            setattr(self, m, torch.zeros(off, dtype=torch.float32, device=device))
        self.bf16 = torch.zeros(off, dtype=torch.bfloat16, device=device) if mirror_bf16 else self.master
        self._pc, self._gc, self._wc = {}, {}, {}

    def _view(self, buf, name):
        off, shape, n = self.index[name]
        layout = self._layout.get(name)
        return buf[off:off + n].view(shape) if layout is None else layout(buf[off:off + n], shape)

    # (the views are cached: the flat buffers never move, and a step asks for ~600 of them)
    def p(self, name):
        v = self._pc.get(name)
        if v is None:
            v = self._pc[name] = self._view(self.master, name)
        return v

    def g(self, name):
        v = self._gc.get(name)
        if v is None:
            v = self._gc[name] = self._view(self.grad, name)
        return v

    def w(self, name):
        v = self._wc.get(name)
        if v is None:
            v = self._wc[name] = self._view(self.bf16, name)
        return v

    def span(self, names):
        lo = min(self.index[n][0] for n in names)
        hi = max(self.index[n][0] + self._reserved[n] for n in names)
        return lo, hi

    def ptr(self, name, buf=None):
        """The device address of an entry's first element in `buf` (default: the masters)."""
        buf = self.master if buf is None else buf
        return buf.data_ptr() + self.index[name][0] * buf.element_size()

    def bind(self, module):
        """Every entry takes the value of the module's parameter of that name, which then becomes a view of the masters."""
        params = dict(module.named_parameters())
        for name in self.index:
            view = self.p(name)
            view.copy_(params[name].detach().to(device=view.device, dtype=torch.float32))
            params[name].data = view

    def moment_state(self):
        """{"<moment>.<name>": a contiguous clone, in the shape the model sees} of every entry, for a checkpoint."""
        return {"%s.%s" % (m, name): self._view(getattr(self, m), name).detach().clone().contiguous()
                for name in self.index for m in self.moments}

    def load_moments(self, state):
        """The inverse of moment_state(); keys that `state` does not hold are left as they are."""
        for m in self.moments:
            buf = getattr(self, m)
            for name in self.index:
                if "%s.%s" % (m, name) in state:
                    self._view(buf, name).copy_(torch.as_tensor(state["%s.%s" % (m, name)]).to(buf.device, torch.float32))


class FlatTrainer:
    """What the model trainers share: `params`, the FlatParams of `self.model` (None until the first step binds it), the gradients and
    the checkpoint.  A trainer sets `model` and `steps`, calls _bind_params from its own bind, and may override the two hooks."""

    params = None
    _pending = None  # a state loaded before the first bind: its moments go in once the buffers exist

    def _bind_params(self, entries, device, **kw):
        self.params = FlatParams(entries, device, pad=8, **kw)
        self.params.bind(self.model)
        if self._pending is not None:
            self.params.load_moments(self._pending)
            self._pending = None

    def gradients(self):
        """{parameter name: float32 gradient, in the model's layout} of the last loss_and_grads / step (views of the flat gradient)."""
        return {name: self.params.g(name) for name in self.params.index}

    def state_dict(self):
        out = {k: v.detach().clone().contiguous() for k, v in self.model.state_dict().items()}
        if self.params is not None:
            out.update(self.params.moment_state())
        out["steps"] = torch.tensor(self.steps, dtype=torch.int64)
        out.update(self._extra_state())
        return out

    def load_state_dict(self, state):
        self.model.load_state_dict({k: torch.as_tensor(state[k]) for k in self.model.state_dict()})
        self.steps = int(state.get("steps", 0))
        if self.params is None:
            self._pending = dict(state)
        else:
            self.params.load_moments(state)
        self._loaded(state)

    def _extra_state(self):
        """Further checkpoint entries of this trainer."""
        return {}

    def _loaded(self, state):
        """After a load: read the trainer's own entries back, drop what was derived from the old values."""
