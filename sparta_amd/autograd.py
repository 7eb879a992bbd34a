"""torch.autograd glue for a block-sparse linear layer on one VBS handle: forward (sparta_vbs_spmm), the gradient of the input
(sparta_vbs_spmm_t), the gradient of the stored values (sparta_vbs_sddmm) and the update (sparta_vbs_set_values) all run on the handle,
on the device, in stream order; bias, activation and output type are one kernel behind the product and one in front of the backward
products (epilogue.py).  torch is imported when vbs_linear is first called, as in device.py."""
from . import _lib, epilogue

_FN = None
_FN_EPILOGUE = None


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
        def forward(ctx, x, values, handle, refresh=False, probe=None):
            n = x.shape[0]
            rec = handle._autograd_values                       # (tensor, version) the handle's values were last taken from; None after any other set_values
            if (rec is None or rec[0] is not values or rec[1] != values._version or refresh
                    or (values.is_cuda and torch.cuda.is_current_stream_capturing())):
                rec = load(handle, values)
            y = torch.empty((n, handle.rows), dtype=torch.float32, device=x.device)
            handle.spmm(x.detach(), y, n, accumulate=False)
            ctx.handle = handle
            ctx.rec = rec
            ctx.probe = probe
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
            if ctx.probe is not None:                           # the block scores of the same product, for the blocks the probe selects
                handle.sddmm_block_ssq(gy, x.detach(), n, sel=ctx.probe.sel, out=ctx.probe.out)
            return grad_x, grad_values, None, None, None

    class _VbsLinearEpilogue(torch.autograd.Function):
        """y = act(x @ A^T + bias) in out_dtype.  The values logic is _VbsLinear's; the elementwise work is epilogue_fwd / epilogue_bwd."""

        @staticmethod
        def forward(ctx, x, values, bias, handle, refresh, activation, out_dtype, probe=None):
            n = x.shape[0]
            rec = handle._autograd_values
            if (rec is None or rec[0] is not values or rec[1] != values._version or refresh
                    or (values.is_cuda and torch.cuda.is_current_stream_capturing())):
                rec = load(handle, values)
            z = torch.empty((n, handle.rows), dtype=torch.float32, device=x.device)
            handle.spmm(x.detach(), z, n, accumulate=False)
            b = None if bias is None else bias.detach()
            in_place = activation == "none" and out_dtype == torch.float32          # (z is not needed in backward: dz = grad_y)
            y = epilogue.epilogue_fwd(z, b, activation, out_dtype, out=z if in_place else None)
            ctx.handle = handle
            ctx.rec = rec
            ctx.probe = probe
            ctx.activation = activation
            ctx.has_bias = bias is not None
            ctx.save_for_backward(x, values, *(() if bias is None else (bias,)), *(() if activation == "none" else (z,)))
            return y

        @staticmethod
        def backward(ctx, grad_y):
            handle = ctx.handle
            saved = list(ctx.saved_tensors)                     # (raises if x, values or bias was modified in place since forward)
            x, values = saved[0], saved[1]
            bias = saved[2] if ctx.has_bias else None
            z = saved[-1] if ctx.activation != "none" else None
            n = x.shape[0]
            need_dbias = ctx.has_bias and ctx.needs_input_grad[2]
            grad_x = grad_values = grad_bias = None
            if not (need_dbias or ctx.needs_input_grad[0] or ctx.needs_input_grad[1] or ctx.probe is not None):
                return None, None, None, None, None, None, None, None
            # one pass: dz in the handle's operand type (what _VbsLinear's .to(x.dtype) did), and the bias gradient
            gy = grad_y.contiguous()
            if ctx.activation == "none" and not need_dbias and gy.dtype == x.dtype:
                dz = gy                                         # (dz = grad_y, already in the operand type: nothing to do)
            else:
                dz, grad_bias = epilogue.epilogue_bwd(gy, z, None if bias is None else bias.detach(), ctx.activation, x.dtype, need_dbias)
            if ctx.needs_input_grad[0]:
                if handle._autograd_values is not ctx.rec:      # the handle took other values since this forward: back to the ones it multiplied with
                    load(handle, values)
                gx = torch.empty((n, handle.cols), dtype=torch.float32, device=x.device)
                handle.spmm_t(dz, gx, n, accumulate=False)
                grad_x = gx.to(x.dtype)
            if ctx.needs_input_grad[1]:
                grad_values = torch.empty(handle._nztot(), dtype=torch.float32, device=x.device)
                handle.sddmm(dz, x.detach(), grad_values, n, accumulate=False)
            if ctx.probe is not None:                           # the block scores of the same product, for the blocks the probe selects
                handle.sddmm_block_ssq(dz, x.detach(), n, sel=ctx.probe.sel, out=ctx.probe.out)
            return grad_x, grad_values, grad_bias, None, None, None, None, None

    global _FN_EPILOGUE
    _FN = _VbsLinear
    _FN_EPILOGUE = _VbsLinearEpilogue
    return _FN


def _function_epilogue():
    _function()
    return _FN_EPILOGUE


def vbs_linear(x, handle, values, refresh=False, *, bias=None, activation="none", out_dtype=None, probe=None):
    """y = x @ A^T, i.e. torch.nn.functional.linear(x, A) with A the block-sparse matrix of `handle` (a DeviceVBS made with updatable=True and
    transposable=True; ValueError otherwise) holding `values`.  With bias, activation or out_dtype: y = act(x @ A^T + bias) in out_dtype (below).

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
    took other values in between (a second forward with another tensor, a set_values), backward first writes the saved ones back.
    On a handle with DeviceVBS.set_forward_a8 on, forward multiplies with the fp8 (e4m3) weights.  Backward uses the 16-bit image of the same values
    (straight-through).

    bias: a contiguous float32 (rows,) tensor on the handle's device, in the VBS's REORDERED row order like y (bias[i] belongs to column i of y), or None.
    activation: "none" | "relu" | "gelu" (the erf form, torch's default).  out_dtype: torch.float32 (the default) | float16 | bfloat16 -- what the next layer
    takes.  With all three at their defaults the call is the plain one above: the same Function, no extra launch.  Otherwise the product goes into an fp32
    z and ONE kernel (epilogue.epilogue_fwd, the pinned arithmetic of include/sparta_amd.h) makes y from it -- in place on z for activation "none" with a
    float32 y; z is saved for backward only with an activation.  Backward: ONE kernel (epilogue.epilogue_bwd) turns grad_y (any of the three types) into
    dz = grad_y * act'(z + bias) in the handle's operand type -- the operand of spmm_t and sddmm -- and, if bias requires grad, into grad_bias (float32
    (rows,), the row sums of the fp32 dz in a fixed fp64 order: bit-identical from run to run); with only bias requiring grad neither product runs.
    ValueError for anything else in the three arguments.

    probe: None, or an object with .sel (uint8 / bool, n_blocks) and .out (float64, n_blocks) on the handle's device, such as BlockPruner.probe(i) gives.
    Backward then also calls handle.sddmm_block_ssq(dz, x, n, sel=probe.sel, out=probe.out) with the operands of its sddmm call -- the squared gradient
    norm of every selected block, the pruned ones of a BlockPruner, which the live sddmm no longer computes -- whether or not values requires grad (as long
    as backward runs at all).  With probe=None the launches and the results are those of the call without the argument."""
    import torch
    if not (handle.updatable and handle.transposable):
        raise ValueError("vbs_linear needs a handle made with updatable=True and transposable=True")
    if handle.dtype != _lib.F32 and ((handle.rows | handle.cols) & 1):
        raise ValueError("vbs_linear on a 16-bit handle needs even rows and cols")
    epilogue.activation_code(activation)
    plain = bias is None and activation == "none" and out_dtype is None
    out_dtype, _ = epilogue.out_dtype_code(out_dtype)            # (None: float32)
    epilogue.check_bias(bias, handle.rows, handle.device)
    want = {_lib.F32: torch.float32, _lib.F16: torch.float16, _lib.BF16: torch.bfloat16}[handle.dtype]
    if not (x.is_cuda and x.dim() == 2 and x.shape[1] == handle.cols and x.dtype == want and x.is_contiguous()):
        raise ValueError("x must be a contiguous (n, %d) %s tensor on the GPU" % (handle.cols, want))
    if not (values.is_cuda and values.dtype == torch.float32 and values.dim() == 1 and values.numel() == handle._nztot() and values.is_contiguous()):
        raise ValueError("values must be a contiguous float32 device tensor of nztot = %d elements" % handle._nztot())
    if plain:
        return _function().apply(x, values, handle, bool(refresh), probe)
    return _function_epilogue().apply(x, values, bias, handle, bool(refresh), activation, out_dtype, probe)
