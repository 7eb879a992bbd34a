"""Global-norm gradient clipping and loss scaling with skip-on-overflow for the VBS optimizers, decided on the device (sparta_grad_stats,
sparta_grad_ctl_finish; the steps read the result through sparta_vbs_*_step_ctl).  torch is imported when a GradCtl is made, as in optim.py."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib, check

_f32p = C.POINTER(C.c_float)


class GradCtl:
    """The control record R of include/sparta_amd.h on one device, and the calls that fill it.

        ctl = sa.GradCtl(loss_scale=1024.0, max_norm=1.0, growth_interval=2000)
        (loss * ctl.loss_scale).backward()        # .loss_scale is a 0-dim float32 view into R: no synchronisation
        ctl.collect([opt, dense_opt])             # every gradient present folded into the statistics, then finish()
        opt.step(ctl=ctl)                         # VbsSGD / VbsAdamW: g * coef, or the step skipped, read on the device

    max_norm = 0: no clipping.  growth_interval = 0: the loss scale stays where it is.  The hyper-parameters are call arguments of finish(): they are
    baked into a capture.  Everything is stream-ordered on torch's current stream and launches only; read() and state_dict() synchronise."""

    def __init__(self, device=0, loss_scale=1.0, max_norm=0.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=0):
        import torch
        if not (loss_scale > 0 and np.isfinite(np.float32(loss_scale))):
            raise ValueError("loss_scale must be a positive finite float32")
        self.device = int(device)
        self.max_norm, self.growth_factor, self.backoff_factor = float(max_norm), float(growth_factor), float(backoff_factor)
        self.growth_interval = int(growth_interval)
        self.R = torch.zeros(_lib.GRAD_CTL_BYTES // 4, dtype=torch.int32, device="cuda:%d" % self.device)
        assert self.R.data_ptr() % 8 == 0
        self._f32 = self.R[:16].view(torch.float32)
        self.loss_scale = self._f32[4]
        self.loss_scale.fill_(float(loss_scale))
        self._f32[7].fill_(float(np.float32(1.0) / np.float32(loss_scale)))        # the coef of a step taken before any finish(): the plain unscaling

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def add(self, tensor, first=False, timed=False):
        """sparta_grad_stats: the elements of `tensor` (a contiguous float32 tensor on this device; a gradient, not a parameter) folded into the statistics.
        first=True starts them over (accumulate = 0).  Returns kernel ms if timed else None."""
        import torch
        if not (tensor.is_cuda and tensor.dtype == torch.float32 and tensor.device.index == self.device and tensor.is_contiguous()):
            raise ValueError("GradCtl.add takes contiguous float32 tensors on device %d" % self.device)
        dt = C.c_float(0)
        with torch.cuda.device(self.device):
            check(lib.sparta_grad_stats(C.cast(C.c_void_p(tensor.data_ptr() if tensor.numel() else None), _f32p), tensor.numel(), C.c_void_p(self.R.data_ptr()),
                                        0 if first else 1, self._stream(), C.byref(dt) if timed else None))
        return dt.value if timed else None

    def collect(self, items):
        """The statistics over every gradient that is present, then finish().  items: VbsSGD / VbsAdamW (the .grad of their values), torch optimizers
        (the .grad of every parameter of their param_groups) and tensors (a tensor that requires grad stands for its .grad, any other is a gradient itself),
        or one of these."""
        import torch
        if isinstance(items, torch.Tensor) or hasattr(items, "pairs") or hasattr(items, "param_groups"):
            items = [items]
        grads = []
        for it in items:
            if hasattr(it, "pairs"):
                params = [v for _, v in it.pairs]
            elif hasattr(it, "param_groups"):
                params = [p for g in it.param_groups for p in g["params"]]
            elif it.requires_grad:
                params = [it]
            else:
                grads.append(it)
                continue
            grads.extend(p.grad for p in params if p.grad is not None)
        if not grads:
            grads = [torch.empty(0, dtype=torch.float32, device=self.R.device)]          # (the words are still zeroed)
        for i, g in enumerate(grads):
            self.add(g, first=i == 0)
        self.finish()

    def finish(self):
        """sparta_grad_ctl_finish: norm, coef and skip from the statistics; the loss scale and its growth tracker move"""
        import torch
        cfg = _lib.GradCtlCfg(self.max_norm, self.growth_factor, self.backoff_factor, self.growth_interval, (C.c_int32 * 4)())
        with torch.cuda.device(self.device):
            check(lib.sparta_grad_ctl_finish(C.c_void_p(self.R.data_ptr()), C.byref(cfg), self._stream()))

    def read(self):
        """the record as a dict (synchronises)"""
        w = self.R[:16].cpu().numpy().view(np.uint32)
        f = w.view(np.float32)
        i = w.view(np.int32)
        return {"ssq": float(w[0:2].view(np.float64)[0]), "nonfinite": int(i[2]), "loss_scale": float(f[4]) if w[4] else 1.0, "growth_tracker": int(i[5]),
                "norm": float(f[6]), "coef": float(f[7]), "skip": int(i[8]), "skipped_total": int(i[9]), "words": w.copy()}

    def state_dict(self):
        """{"loss_scale", "growth_tracker", "skipped_total"} (synchronises)"""
        r = self.read()
        return {k: r[k] for k in ("loss_scale", "growth_tracker", "skipped_total")}

    def load_state_dict(self, sd):
        """takes loss_scale, growth_tracker and skipped_total over; coef becomes 1 / loss_scale, as in a new GradCtl, until the next finish()"""
        import torch
        if not (sd["loss_scale"] > 0 and np.isfinite(np.float32(sd["loss_scale"]))):
            raise ValueError("loss_scale must be a positive finite float32")
        w = np.zeros(2, np.int32)
        w[0], w[1] = int(sd["growth_tracker"]), int(sd["skipped_total"])
        self.loss_scale.fill_(float(sd["loss_scale"]))
        self._f32[7].fill_(float(np.float32(1.0) / np.float32(sd["loss_scale"])))
        src = torch.from_numpy(w).to(self.R.device)
        self.R[5:6].copy_(src[0:1])
        self.R[9:10].copy_(src[1:2])
