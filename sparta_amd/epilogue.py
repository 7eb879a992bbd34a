"""The epilogue of a block-sparse linear layer on torch tensors (sparta_epilogue_fwd / sparta_epilogue_bwd, k_epilogue.hip): bias, activation and the output
type in one kernel behind the forward product, and in one kernel in front of the two backward products, which also writes their operand in the handle's type
and the bias gradient.  A contiguous (n, rows) tensor IS the column-major rows x n matrix the entries take: no layout copies.  torch is imported when a
function is first called, as in gradctl.py."""
import ctypes as C

from . import _lib
from ._lib import lib, check

_f32p = C.POINTER(C.c_float)
ACTIVATIONS = {"none": _lib.ACT_NONE, "relu": _lib.ACT_RELU, "gelu": _lib.ACT_GELU}
_SCRATCH = {}          # device index -> the float64 tensor the run sums of the bias gradient pass through (grown on demand, never under capture)
_RETIRED = []          # every scratch tensor a larger one replaced: a graph captured earlier has its address in an epilogue_bwd node, so it is never freed
_SCRATCH_BYTES = {}    # (rows, n_cols) -> sparta_epilogue_scratch_bytes: a function of the shape alone, asked once per shape
_DTYPES = {}           # torch dtype -> SPARTA_* code, filled at the first call


def _dtypes():
    if not _DTYPES:
        import torch
        _DTYPES.update({torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16})
    return _DTYPES


def activation_code(activation):
    if activation not in ACTIVATIONS:
        raise ValueError("activation must be one of 'none', 'relu', 'gelu', not %r" % (activation,))
    return ACTIVATIONS[activation]


def out_dtype_code(out_dtype):
    """the SPARTA_* code of a torch dtype; None stands for float32"""
    import torch
    if out_dtype is None:
        out_dtype = torch.float32
    codes = _dtypes()
    if out_dtype not in codes:
        raise ValueError("out_dtype must be torch.float32, torch.float16 or torch.bfloat16, not %r" % (out_dtype,))
    return out_dtype, codes[out_dtype]


def check_bias(bias, rows, device):
    """bias: None, or a contiguous float32 (rows,) tensor on GPU `device` (an index)"""
    import torch
    if bias is None:
        return
    if not (isinstance(bias, torch.Tensor) and bias.dtype == torch.float32 and bias.dim() == 1 and bias.shape[0] == rows and bias.is_contiguous()
            and bias.is_cuda and bias.device.index == device):
        raise ValueError("bias must be a contiguous float32 (%d,) tensor on cuda:%d" % (rows, device))


def _matrix(t, name, dtypes):
    if not (t.is_cuda and t.dim() == 2 and t.is_contiguous() and t.dtype in dtypes):
        raise ValueError("%s must be a contiguous (n, rows) tensor on the GPU of type %s" % (name, " / ".join(str(d) for d in dtypes)))


def _ptr(t, typ=None):
    p = C.c_void_p(t.data_ptr() if t is not None and t.numel() else None)
    return C.cast(p, typ) if typ is not None else p


def _stream(device):
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class _On:
    """the entries run on the current device: switch to the tensors' device only where it is not the current one (the switch costs more host time than
    the launch)"""

    def __init__(self, device):
        import torch
        self.guard = None if torch.cuda.current_device() == device.index else torch.cuda.device(device)

    def __enter__(self):
        if self.guard is not None:
            self.guard.__enter__()

    def __exit__(self, *exc):
        if self.guard is not None:
            self.guard.__exit__(*exc)


def scratch_bytes(rows, n_cols):
    """sparta_epilogue_scratch_bytes: a function of (rows, n_cols) alone; 0 when one run of EPILOGUE_RUN columns covers n_cols"""
    key = (int(rows), int(n_cols))
    if key not in _SCRATCH_BYTES:
        out = C.c_int64(0)
        check(lib.sparta_epilogue_scratch_bytes(key[0], key[1], C.byref(out)))
        _SCRATCH_BYTES[key] = out.value
    return _SCRATCH_BYTES[key]


def _scratch(device, nbytes):
    import torch
    t = _SCRATCH.get(device.index)
    if t is None or t.numel() * 8 < nbytes:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("epilogue_bwd: the scratch of the bias gradient would have to grow while the stream is being captured -- run the call once "
                               "outside the capture first")
        if t is not None:
            _RETIRED.append(t)                                  # (a few KB to MB each, and each larger than the one before)
        t = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)
        _SCRATCH[device.index] = t
    return t


def epilogue_fwd(z, bias=None, activation="none", out_dtype=None, out=None, timed=False):
    """y = act(z + bias) rounded to out_dtype, in one kernel.  z: contiguous float32 (n, rows) on the GPU; bias: float32 (rows,) or None; activation "none" |
    "relu" | "gelu" (the erf form); out_dtype float32 (the default) | float16 | bfloat16.  out: the tensor to write, (n, rows) of out_dtype -- `out is z` runs in
    place (float32 only); None allocates.  Stream-ordered on torch's current stream.  Returns y, or (y, kernel ms) if timed."""
    import torch
    act = activation_code(activation)
    _matrix(z, "z", (torch.float32,))
    n, rows = z.shape
    check_bias(bias, rows, z.device.index)
    if out is None:
        out_dtype, code = out_dtype_code(out_dtype)
        out = torch.empty((n, rows), dtype=out_dtype, device=z.device)
    else:
        out_dtype, code = out_dtype_code(out.dtype if out_dtype is None else out_dtype)
        if not (out.is_cuda and out.shape == z.shape and out.dtype == out_dtype and out.is_contiguous() and out.device == z.device):
            raise ValueError("out must be a contiguous (%d, %d) %s tensor on %s" % (n, rows, out_dtype, z.device))
    dt = C.c_float(0)
    with _On(z.device):
        check(lib.sparta_epilogue_fwd(_ptr(z, _f32p), rows, _ptr(bias, _f32p), act, _ptr(out), rows, code, rows, n, _stream(z.device),
                                      C.byref(dt) if timed else None))
    return (out, dt.value) if timed else out


def epilogue_bwd(grad_y, z, bias, activation, dz_dtype, need_dbias, out=None, timed=False):
    """(dz, dbias) of y = act(z + bias): dz = grad_y * act'(z + bias) rounded to dz_dtype -- the operand of spmm_t and sddmm in the handle's type -- and, with
    need_dbias, dbias (float32 (rows,)) = the row sums of the fp32 dz before that rounding, in the fixed fp64 order of include/sparta_amd.h; else None.
    grad_y: contiguous (n, rows), float32 / float16 / bfloat16; z: the float32 (n, rows) input of the forward epilogue, None allowed with activation "none".
    out: the tensor to write dz to (`out is grad_y` runs in place, equal types only); None allocates.  One kernel (two when n > EPILOGUE_RUN and need_dbias),
    stream-ordered on torch's current stream.  Returns (dz, dbias), or (dz, dbias, kernel ms) if timed."""
    import torch
    act = activation_code(activation)
    codes = _dtypes()
    _matrix(grad_y, "grad_y", tuple(codes))
    n, rows = grad_y.shape
    dev = grad_y.device
    if z is None:
        if act != _lib.ACT_NONE:
            raise ValueError("epilogue_bwd needs z unless activation is 'none'")
    else:
        _matrix(z, "z", (torch.float32,))
        if z.shape != grad_y.shape or z.device != dev:
            raise ValueError("z must have the shape and the device of grad_y")
    check_bias(bias, rows, dev.index)
    dz_dtype, dz_code = out_dtype_code(dz_dtype)
    if out is None:
        out = torch.empty((n, rows), dtype=dz_dtype, device=dev)
    elif not (out.is_cuda and out.shape == grad_y.shape and out.dtype == dz_dtype and out.is_contiguous() and out.device == dev):
        raise ValueError("out must be a contiguous (%d, %d) %s tensor on %s" % (n, rows, dz_dtype, dev))
    dbias = scratch = None
    if need_dbias:
        dbias = torch.empty(rows, dtype=torch.float32, device=dev)
        nbytes = scratch_bytes(rows, n)
        if nbytes and rows:
            scratch = _scratch(dev, nbytes)
    dt = C.c_float(0)
    with _On(dev):
        check(lib.sparta_epilogue_bwd(_ptr(grad_y), rows, codes[grad_y.dtype], _ptr(z, _f32p), rows, _ptr(bias, _f32p), act, _ptr(out), rows, dz_code,
                                      _ptr(dbias, _f32p), _ptr(scratch), rows, n, _stream(dev), C.byref(dt) if timed else None))
    return (out, dbias, dt.value) if timed else (out, dbias)
