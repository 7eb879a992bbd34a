"""SGD for block-sparse layers on VBS handles: the optimizer step and the update of the handle in one pass (sparta_vbs_sgd_step).  torch is
imported when an optimizer is first used, as in autograd.py."""


class VbsSGD:
    """torch.optim.SGD (dampening 0, no Nesterov) for the stored values of block-sparse layers.

    pairs: a list of (handle, values) -- a DeviceVBS made with updatable=True and the float32 master copy of its stored values (the leaf tensor
    given to vbs_linear).  step() runs handle.sgd_step on every pair: values, the momentum buffer and the handle's images are updated by the same
    kernels, so the next vbs_linear forward does not call set_values (the handle records the tensor object it was stepped with: pass the leaf itself).
    A pair whose values have no gradient is left alone."""

    def __init__(self, pairs, lr, momentum=0.0, weight_decay=0.0):
        self.pairs = [(h, v) for h, v in pairs]
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("lr, momentum and weight_decay must be >= 0")
        self.lr, self.momentum, self.weight_decay = float(lr), float(momentum), float(weight_decay)
        self._bufs = [None] * len(self.pairs)

    def step(self, grad_scale=1.0):
        import torch
        for i, (handle, values) in enumerate(self.pairs):
            if values.grad is None:
                continue
            if self.momentum != 0.0 and self._bufs[i] is None:
                self._bufs[i] = torch.zeros_like(values, requires_grad=False)
            handle.sgd_step(values, values.grad, self._bufs[i], lr=self.lr, momentum=self.momentum, weight_decay=self.weight_decay,
                            grad_scale=grad_scale)

    def zero_grad(self, set_to_none=True):
        for _, values in self.pairs:
            if values.grad is None:
                continue
            if set_to_none:
                values.grad = None
            else:
                values.grad.detach_()
                values.grad.zero_()
