"""SGD and Adam / AdamW for block-sparse layers on VBS handles: the optimizer step and the update of the handle in one pass (sparta_vbs_sgd_step,
sparta_vbs_adam_step).  torch is imported when an optimizer is first used, as in autograd.py."""


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

    def step(self, grad_scale=1.0, ctl=None):
        """ctl: a GradCtl after collect() / finish(): its coefficient (clipping, 1 / loss scale) and its skip flag are read on the device (gradctl.py)"""
        import torch
        for i, (handle, values) in enumerate(self.pairs):
            if values.grad is None:
                continue
            if self.momentum != 0.0 and self._bufs[i] is None:
                self._bufs[i] = torch.zeros_like(values, requires_grad=False)
            handle.sgd_step(values, values.grad, self._bufs[i], lr=self.lr, momentum=self.momentum, weight_decay=self.weight_decay,
                            grad_scale=grad_scale, ctl=ctl)

    def zero_grad(self, set_to_none=True):
        for _, values in self.pairs:
            if values.grad is None:
                continue
            if set_to_none:
                values.grad = None
            else:
                values.grad.detach_()
                values.grad.zero_()


class VbsAdamW:
    """torch.optim.AdamW (decoupled=True, the default) / torch.optim.Adam with L2 weight decay (decoupled=False), without amsgrad and maximize, for the
    stored values of block-sparse layers.

    pairs: the (handle, values) list of VbsSGD.  step() runs handle.adam_step on every pair whose values have a gradient: values, exp_avg, exp_avg_sq and
    the handle's images are updated by the same kernels.  The state of a pair -- exp_avg, exp_avg_sq and the 8-word step state, which lives on the device and
    is advanced there (so a captured step replays correctly) -- is allocated at its first step; state_dict() / load_state_dict() carry it, and nothing else
    can checkpoint the step count."""

    def __init__(self, pairs, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=True):
        self.pairs = [(h, v) for h, v in pairs]
        if lr < 0 or weight_decay < 0:
            raise ValueError("lr and weight_decay must be >= 0")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("betas must lie in [0, 1)")
        if not eps > 0:
            raise ValueError("eps must be > 0")
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.weight_decay, self.decoupled = float(weight_decay), bool(decoupled)
        self._state = [None] * len(self.pairs)

    def _state_of(self, i):
        import torch
        if self._state[i] is None:
            values = self.pairs[i][1]
            self._state[i] = {"exp_avg": torch.zeros_like(values, requires_grad=False), "exp_avg_sq": torch.zeros_like(values, requires_grad=False),
                              "state": torch.zeros(8, dtype=torch.int32, device=values.device)}
        return self._state[i]

    def step(self, grad_scale=1.0, ctl=None):
        """ctl: as for VbsSGD.step; a skipped step leaves the step count where it is"""
        for i, (handle, values) in enumerate(self.pairs):
            if values.grad is None:
                continue
            s = self._state_of(i)
            handle.adam_step(values, values.grad, s["exp_avg"], s["exp_avg_sq"], s["state"], lr=self.lr, betas=self.betas, eps=self.eps,
                             weight_decay=self.weight_decay, decoupled=self.decoupled, grad_scale=grad_scale, ctl=ctl)

    def zero_grad(self, set_to_none=True):
        VbsSGD.zero_grad(self, set_to_none)

    def state_dict(self):
        """{"state": [per pair: None (no step yet) or {"exp_avg", "exp_avg_sq", "state"} as copies], "hyper": {...}}"""
        return {"state": [None if s is None else {k: t.detach().clone() for k, t in s.items()} for s in self._state],
                "hyper": {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay, "decoupled": self.decoupled}}

    def load_state_dict(self, sd):
        if len(sd["state"]) != len(self.pairs):
            raise ValueError("the state dict holds %d pairs, the optimizer %d" % (len(sd["state"]), len(self.pairs)))
        for i, src in enumerate(sd["state"]):
            if src is None:
                self._state[i] = None
                continue
            dst = self._state_of(i)
            for k, t in dst.items():
                if src[k].numel() != t.numel():
                    raise ValueError("pair %d: %s holds %d elements, expected %d" % (i, k, src[k].numel(), t.numel()))
                t.copy_(src[k].to(device=t.device).view(t.dtype) if src[k].dtype != t.dtype else src[k])
        h = sd.get("hyper", {})
        self.lr, self.betas, self.eps = float(h.get("lr", self.lr)), tuple(h.get("betas", self.betas)), float(h.get("eps", self.eps))
        self.weight_decay, self.decoupled = float(h.get("weight_decay", self.weight_decay)), bool(h.get("decoupled", self.decoupled))
