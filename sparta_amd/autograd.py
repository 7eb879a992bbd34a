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

    class _VbsLinear(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, values, handle):
            n = x.shape[0]
            key = (values.data_ptr(), values._version)
            if getattr(handle, "_autograd_values", None) != key:
                handle.set_values(values.detach())
                handle._autograd_values = key
            y = torch.empty((n, handle.rows), dtype=torch.float32, device=x.device)
            handle.spmm(x.detach(), y, n, accumulate=False)
            ctx.handle = handle
            ctx.save_for_backward(x)
            return y

        @staticmethod
        def backward(ctx, grad_y):
            handle = ctx.handle
            (x,) = ctx.saved_tensors
            n = x.shape[0]
            gy = grad_y.contiguous().to(x.dtype)                # (16-bit handles take the operands in their own type)
            grad_x = grad_values = None
            if ctx.needs_input_grad[0]:
                gx = torch.empty((n, handle.cols), dtype=torch.float32, device=x.device)
                handle.spmm_t(gy, gx, n, accumulate=False)
                grad_x = gx.to(x.dtype)
            if ctx.needs_input_grad[1]:
                grad_values = torch.empty(handle._nztot(), dtype=torch.float32, device=x.device)
                handle.sddmm(gy, x.detach(), grad_values, n, accumulate=False)
            return grad_x, grad_values, None

    _FN = _VbsLinear
    return _FN


def vbs_linear(x, handle, values):
    """y = x @ A^T, i.e. torch.nn.functional.linear(x, A) with A the block-sparse matrix of `handle` (a DeviceVBS made with updatable=True and
    transposable=True; ValueError otherwise) holding `values`.

    x: contiguous (n, cols) tensor on the handle's device in the handle's operand type (float32 / float16 / bfloat16) -- it IS the
    column-major cols x n operand B of the product, and y, (n, rows) float32, IS the column-major C: no layout copies.  The rows of y are in
    the VBS's reordered order (sparta_amd.get_permutation gives the map).  values: the float32 master copy of the stored values, nztot
    elements in the layout of VBR.mab, on the device; it is written into the handle (set_values) whenever it changed since the last call
    (torch's version counter and data pointer), so `values -= lr * values.grad` between two calls is seen by the second without a host copy.
    Backward: grad_x = A^T grad_y (spmm_t, returned in x.dtype), grad_values = grad_y x^T sampled on the stored blocks (sddmm); 16-bit
    handles round grad_y to their type first and need even rows and cols (their operands are read with an even leading dimension)."""
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
    return _function().apply(x, values, handle)
