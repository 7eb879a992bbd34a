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

    def repattern(self, i, vbmat, keep=None, add=None, block_row_range=None):
        """Pair i moved onto a new block pattern (sparta_amd.repattern: the old pattern minus the blocks with keep[b] == 0 plus the blocks of `add`; vbmat is the
        VBR of the pair's handle, block_row_range the range the handle was created with).  The pair is replaced by the new handle and a new leaf `values`
        with the old one's requires_grad and grad = None; the momentum buffer, where it is allocated, travels in the same launch.  The old handle is left
        open and the old tensors are left as they are.  last_map holds the block map of the call.  Synchronises.  Returns (new_vbmat, new_handle, new_values).
        A refusal (sparta_amd.repattern: a new pattern that does not qualify for the fp8 weight image the old handle multiplies with, among others) raises
        before anything of the optimizer is replaced."""
        return self.repattern_commit(i, self.repattern_prepare(i, vbmat, keep=keep, add=add, block_row_range=block_row_range))

    def repattern_prepare(self, i, vbmat, keep=None, add=None, block_row_range=None):
        """the first half of repattern (sparta_amd.repattern_prepare on the pair's values and momentum buffer): everything that can refuse, nothing moved and
        nothing of the optimizer changed.  Returns the plan for repattern_commit(i, plan); a plan that is not committed must be closed (plan.close())"""
        from .device import repattern_prepare
        handle, values = self.pairs[i]
        buf = self._bufs[i]
        return repattern_prepare(vbmat, handle, [values.detach()] + ([buf] if buf is not None else []), keep=keep, add=add, block_row_range=block_row_range)

    def repattern_commit(self, i, plan):
        """the second half: the move, then the pair and the momentum buffer replaced.  Returns (new_vbmat, new_handle, new_values)"""
        from .device import repattern_commit
        values, buf = self.pairs[i][1], self._bufs[i]
        new_vbmat, new_handle, new_t, self.last_map = repattern_commit(plan)
        new_values = new_t[0].requires_grad_(values.requires_grad)
        self.pairs[i] = (new_handle, new_values)
        if buf is not None:
            self._bufs[i] = new_t[1]
        return new_vbmat, new_handle, new_values

    def zero_grad(self, set_to_none=True):
        for _, values in self.pairs:
            if values.grad is None:
                continue
            if set_to_none:
                values.grad = None
            else:
                values.grad.detach_()
                values.grad.zero_()

    def state_dict(self):
        """{"momentum_buffer": [per pair: None (no step with momentum yet) or a copy of the buffer], "hyper": {...}}"""
        return {"momentum_buffer": [None if b is None else b.detach().clone() for b in self._bufs],
                "hyper": {"lr": self.lr, "momentum": self.momentum, "weight_decay": self.weight_decay}}

    def load_state_dict(self, sd):
        import torch
        if len(sd["momentum_buffer"]) != len(self.pairs):
            raise ValueError("the state dict holds %d pairs, the optimizer %d" % (len(sd["momentum_buffer"]), len(self.pairs)))
        for i, src in enumerate(sd["momentum_buffer"]):
            values = self.pairs[i][1]
            if src is not None and src.numel() != values.numel():
                raise ValueError("pair %d: momentum_buffer holds %d elements, expected %d" % (i, src.numel(), values.numel()))
        for i, src in enumerate(sd["momentum_buffer"]):
            values = self.pairs[i][1]
            self._bufs[i] = None if src is None else src.detach().to(device=values.device, dtype=torch.float32).clone().reshape(-1)
        h = sd.get("hyper", {})
        self.lr, self.momentum = float(h.get("lr", self.lr)), float(h.get("momentum", self.momentum))
        self.weight_decay = float(h.get("weight_decay", self.weight_decay))


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

    def repattern(self, i, vbmat, keep=None, add=None, block_row_range=None):
        """VbsSGD.repattern for Adam: exp_avg and exp_avg_sq, where they are allocated, travel with the values in the same launch; the 8-word device state,
        which holds the step count, is kept as it is (the same tensor).  Returns (new_vbmat, new_handle, new_values)."""
        return self.repattern_commit(i, self.repattern_prepare(i, vbmat, keep=keep, add=add, block_row_range=block_row_range))

    def repattern_prepare(self, i, vbmat, keep=None, add=None, block_row_range=None):
        """VbsSGD.repattern_prepare on the pair's values, exp_avg and exp_avg_sq"""
        from .device import repattern_prepare
        handle, values = self.pairs[i]
        st = self._state[i]
        return repattern_prepare(vbmat, handle, [values.detach()] + ([st["exp_avg"], st["exp_avg_sq"]] if st is not None else []), keep=keep, add=add,
                                 block_row_range=block_row_range)

    def repattern_commit(self, i, plan):
        """VbsSGD.repattern_commit: the move, then the pair and its moments replaced (the step words stay the same tensor)"""
        from .device import repattern_commit
        values, st = self.pairs[i][1], self._state[i]
        new_vbmat, new_handle, new_t, self.last_map = repattern_commit(plan)
        new_values = new_t[0].requires_grad_(values.requires_grad)
        self.pairs[i] = (new_handle, new_values)
        if st is not None:
            self._state[i] = {"exp_avg": new_t[1], "exp_avg_sq": new_t[2], "state": st["state"]}
        return new_vbmat, new_handle, new_values

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
