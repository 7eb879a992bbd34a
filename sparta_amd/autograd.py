"""torch.autograd glue for a block-sparse linear layer on one VBS handle: forward (sparta_vbs_spmm), the gradient of the input
(sparta_vbs_spmm_t), the gradient of the stored values (sparta_vbs_sddmm) and the update (sparta_vbs_set_values) all run on the handle,
on the device, in stream order.  torch is imported when vbs_linear is first called, as in device.py."""
from . import _lib

_FN = None


def _function():
    global _FN
    if _FN is not None:
        return _FN
    import torch

    def load(handle, values):
        """writes `values` into the handle; returns the record of it left on the handle.  The record holds the tensor itself, so its address cannot go to
        another tensor while the record lives.  Once a call was recorded into a graph the record matches no tensor any more and every later forward
        writes the values again: a replay changes the handle's values without passing here."""
        handle.set_values(values.detach())
        if values.is_cuda and torch.cuda.is_current_stream_capturing():
            handle._autograd_captured = True
        rec = (None, None) if handle._autograd_captured else (values, values._version)
        handle._autograd_values = rec
        return rec

    class _VbsLinear(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, values, handle, refresh=False):
            n = x.shape[0]
            rec = handle._autograd_values                       # (tensor, version) the handle's values were last taken from; None after any other set_values
            if (rec is None or rec[0] is not values or rec[1] != values._version or refresh
                    or (values.is_cuda and torch.cuda.is_current_stream_capturing())):
                rec = load(handle, values)
            y = torch.empty((n, handle.rows), dtype=torch.float32, device=x.device)
            handle.spmm(x.detach(), y, n, accumulate=False)
            ctx.handle = handle
            ctx.rec = rec
            ctx.save_for_backward(x, values)
            return y

        @staticmethod
        def backward(ctx, grad_y):
            handle = ctx.handle
            x, values = ctx.saved_tensors                       # (raises if x or values was modified in place since forward)
            n = x.shape[0]
            gy = grad_y.contiguous().to(x.dtype)                # (16-bit handles take the operands in their own type)
            grad_x = grad_values = None
            if ctx.needs_input_grad[0]:
                if handle._autograd_values is not ctx.rec:      # the handle took other values since this forward: back to the ones it multiplied with
                    load(handle, values)
                gx = torch.empty((n, handle.cols), dtype=torch.float32, device=x.device)
                handle.spmm_t(gy, gx, n, accumulate=False)
                grad_x = gx.to(x.dtype)
            if ctx.needs_input_grad[1]:
                grad_values = torch.empty(handle._nztot(), dtype=torch.float32, device=x.device)
                handle.sddmm(gy, x.detach(), grad_values, n, accumulate=False)
            return grad_x, grad_values, None, None

    _FN = _VbsLinear
    return _FN


def vbs_linear(x, handle, values, refresh=False):
    """y = x @ A^T, i.e. torch.nn.functional.linear(x, A) with A the block-sparse matrix of `handle` (a DeviceVBS made with updatable=True and
    transposable=True; ValueError otherwise) holding `values`.

    x: contiguous (n, cols) tensor on the handle's device in the handle's operand type (float32 / float16 / bfloat16) -- it IS the
    column-major cols x n operand B of the product, and y, (n, rows) float32, IS the column-major C: no layout copies.  The rows of y are in
    the VBS's reordered order (sparta_amd.get_permutation gives the map).  values: the float32 master copy of the stored values, nztot
    elements in the layout of VBR.mab, on the device.

    The product is taken with what `values` holds at the call, and backward differentiates that product.  The handle keeps a record of the tensor
    object it last took its values from and of that tensor's version counter; set_values is skipped only when the same object comes again with
    the same version and nothing else wrote to the handle in between (DeviceVBS.set_values, set_values_host and close drop the record), so
    `values -= lr * values.grad` under no_grad, an optimizer step, another tensor or a set_values of the caller's own are all seen.  What the
    version counter does not see is not: after `values.data.copy_(...)`, `values.data -= ...` or a write through the raw pointer from outside
    torch, pass refresh=True, which always writes the values.  While the current stream is being captured set_values is always recorded, and from
    then on nothing is skipped on that handle (a replay changes its values without passing through Python).
    Backward: grad_x = A^T grad_y (spmm_t, returned in x.dtype), grad_values = grad_y x^T sampled on the stored blocks (sddmm); 16-bit
    handles round grad_y to their type first and need even rows and cols (their operands are read with an even leading dimension).  `values` is
    saved for backward: changing it in place between forward and backward raises torch's RuntimeError, as for any saved tensor; if the handle
    took other values in between (a second forward with another tensor, a set_values), backward first writes the saved ones back."""
    import torch
    if not (handle.updatable and handle.transposable):
        raise ValueError("vbs_linear needs a handle made with updatable=True and transposable=True")
    if handle.dtype != _lib.F32 and ((handle.rows | handle.cols) & 1):
        raise ValueError("vbs_linear on a 16-bit handle needs even rows and cols")
    want = {_lib.F32: torch.float32, _lib.F16: torch.float16, _lib.BF16: torch.bfloat16}[handle.dtype]
    if not (x.is_cuda and x.dim() == 2 and x.shape[1] == handle.cols and x.dtype == want and x.is_contiguous()):
        raise ValueError("x must be a contiguous (n, %d) %s tensor on the GPU" % (handle.cols, want))
    if not (values.is_cuda and values.dtype == torch.float32 and values.dim() == 1 and values.numel() == handle._nztot() and values.is_contiguous()):
        raise ValueError("values must be a contiguous float32 device tensor of nztot = %d elements" % handle._nztot())
    return _function().apply(x, values, handle, bool(refresh))
