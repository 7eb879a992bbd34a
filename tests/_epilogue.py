"""References shared by the tests of the epilogue (sparta_epilogue_fwd / sparta_epilogue_bwd): fwd_ref and bwd_ref, the numpy float32 restatement of the
arithmetic include/sparta_amd.h pins -- every operation rounded once, in the order written, the bias gradient in runs of 32 columns in sequential fp64 -- and
the round-to-nearest-even conversions to fp16 / bf16.  Matrices are logical (rows, n_cols) arrays M[i, j]; `store` puts one into a column-major buffer with a
leading dimension.  Only erff has no numpy float32 form: it is math.erf rounded to float32, one of several legitimate erff, so GELU is compared with a
tolerance and everything else bit for bit."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
F32, F16, BF16 = 0, 1, 2
NONE, RELU, GELU = 0, 1, 2
ACT_NAME = {NONE: "none", RELU: "relu", GELU: "gelu"}
RUN = 32
ESIZE = {F32: 4, F16: 2, BF16: 2}
NP_STORE = {F32: np.float32, F16: np.uint16, BF16: np.uint16}


def _f(x):
    """an intermediate of the references: float32, or the restatement is not one"""
    assert isinstance(x, (np.ndarray, np.generic)) and x.dtype == f32, getattr(x, "dtype", type(x))
    return x


def rne_bits(x, dtype):
    """float32 -> the stored form: float32 itself, or the uint16 bits of fp16 / bf16 rounded to nearest even (a bf16 NaN keeps its sign and gets the quiet bit)"""
    x = _f(np.asarray(x, f32))
    if dtype == F32:
        return x.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        if dtype == F16:
            return x.astype(np.float16).view(np.uint16)
    u = x.view(np.uint32)
    nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    r = ((u.astype(np.uint64) + 0x7fff + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint64(16)).astype(np.uint32)
    r = np.where(nan, ((u >> np.uint32(16)) | np.uint32(0x40)) & np.uint32(0xffff), r & np.uint32(0xffff))
    return r.astype(np.uint16)


def widen(stored, dtype):
    """the stored form -> float32, exactly"""
    stored = np.asarray(stored)
    if dtype == F32:
        return _f(stored.astype(f32, copy=True))
    if dtype == F16:
        return _f(stored.astype(np.uint16).view(np.float16).astype(f32))
    return _f((stored.astype(np.uint32) << np.uint32(16)).view(f32))


def _erff(x):
    return _f(np.vectorize(math.erf, otypes=[f64])(_f(x).astype(f64)).astype(f32))


def _u(Z, bias):
    Z = _f(np.asarray(Z))
    if bias is None:
        return Z
    with np.errstate(invalid="ignore", over="ignore"):
        return _f(Z + _f(np.asarray(bias))[:, None])


def fwd_f32(Z, bias, act):
    """y before its rounding to the output type"""
    u = _u(Z, bias)
    with np.errstate(invalid="ignore", over="ignore"):
        if act == RELU:
            return _f(np.where(u <= f32(0), f32(0), u))
        if act == GELU:
            e = _erff(_f(u * f32(0.70710678)))
            return _f(_f(f32(0.5) * u) * _f(f32(1) + e))
    return _f(u.copy())


def fwd_ref(Z, bias, act, y_dtype=F32):
    """Y as stored: float32, or uint16 bits"""
    return rne_bits(fwd_f32(Z, bias, act), y_dtype)


def dbias_of(dz):
    """the pinned order: runs of RUN columns; inside a run sequential fp64, j ascending, from 0.0; the run sums added in run order; rounded once"""
    dz = _f(np.asarray(dz))
    rows, n = dz.shape
    total = np.zeros(rows, f64)
    with np.errstate(invalid="ignore", over="ignore"):
        for r0 in range(0, n, RUN):
            s = np.zeros(rows, f64)
            for j in range(r0, min(r0 + RUN, n)):
                s = s + dz[:, j].astype(f64)
            total = total + s
        return _f(total.astype(f32))


def bwd_f32(dY, Z, bias, act):
    """dz before its rounding to the output type; dY: float32 (already widened)"""
    dY = _f(np.asarray(dY))
    if act == NONE:
        return _f(dY.copy())
    u = _u(Z, bias)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if act == RELU:
            return _f(np.where(u <= f32(0), f32(0), dY))
        e = _erff(_f(u * f32(0.70710678)))
        cdf = _f(f32(0.5) * _f(f32(1) + e))
        t = _f(_f(f32(-0.5) * u) * u)
        pdf = _f(_f(u * _f(np.exp(t))) * f32(0.39894228))
        return _f(dY * _f(cdf + pdf))


def bwd_ref(dY, Z, bias, act, dz_dtype=F32):
    """(dZ as stored, dbias float32)"""
    dz = bwd_f32(dY, Z, bias, act)
    return rne_bits(dz, dz_dtype), dbias_of(dz)


def store(M, ld, dtype, offset=0, pad=None):
    """the column-major image of the stored form of M (rows x n_cols) with leading dimension ld behind `offset` elements; everything that is not an element of
    M holds `pad` (stored form; default: a NaN pattern)"""
    rows, n = M.shape
    if pad is None:
        pad = f32(np.nan) if dtype == F32 else np.uint16(0x7e01 if dtype == F16 else 0x7fc1)
    buf = np.full(offset + ld * max(n, 1), pad, NP_STORE[dtype])
    img = buf[offset:offset + ld * n].reshape(n, ld)
    img[:, :rows] = np.asarray(M).T
    return buf


def unstore(buf, rows, n, ld, offset=0):
    return np.asarray(buf)[offset:offset + ld * n].reshape(n, ld)[:, :rows].T.copy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == f32 else a


SPECIALS = np.array([np.inf, np.nan, -np.inf, -0.0, 0.0, 1e-30, -1e-30, 65520.0, -3.0e38, 1.0e-8], f32)


def special_values(rng, shape, scale=2.0):
    """(rows, n_cols) float32 data straddling 0 with +-Inf, one NaN, -0.0, +0.0, tiny and huge values put in -- at most ONE of them per row, so that a row sum
    never meets Inf - Inf (whose NaN has a sign that differs between processors) -- and a column of exact zeros of both signs where there is room"""
    rows, n = shape
    x = (rng.standard_normal(shape) * scale).astype(f32)
    for k, r in enumerate(rng.permutation(rows)[:len(SPECIALS)]):
        x[r, rng.integers(n)] = SPECIALS[k]
    return x
