"""The rule of the fp8 weight image (DeviceVBS.set_forward_a8; include/sparta_amd.h, "THE FP8 WEIGHT IMAGE") restated in numpy: the exponent of a group from
frexp, round-to-nearest-even to OCP e4m3fn in integer arithmetic on float64 (every product v * 2^-e is exact there), and the dequantised value in float64."""
import numpy as np

NAN_CODE = 0x7F
MAX_CODE = 0x7E          # 448


def exponent(amax):
    """e of a group whose largest finite |v| is amax (array or scalar): the smallest e with amax * 2^-e <= 448, clamped to [-126, 127]; 0 for amax == 0"""
    amax = np.asarray(amax, np.float64)
    m, x = np.frexp(amax)                                  # amax = m * 2^x, m in [0.5, 1)
    e = np.where(m <= 0.875, x - 9, x - 8)
    return np.where(amax == 0, 0, np.clip(e, -126, 127)).astype(np.int64)


def encode(x):
    """float64 x (|x| <= 448, or NaN / Inf) -> uint8 e4m3fn codes, round to nearest even; subnormals and the sign of zero kept; NaN, +-Inf -> 0x7F | sign"""
    x = np.asarray(x, np.float64)
    sign = np.where(np.signbit(x), 0x80, 0).astype(np.int64)
    a = np.abs(x)
    fin = np.isfinite(a)
    a = np.where(fin, a, 0.0)
    m, ex = np.frexp(a)                                    # a = m * 2^ex = (2 m) * 2^(ex - 1)
    normal = a >= 2.0 ** -6
    n = np.rint(np.ldexp(a, -(ex - 4))).astype(np.int64)   # a in units of 2^(ex - 1 - 3): 8 .. 16 (np.rint rounds halves to even)
    up = n == 16
    code_n = ((ex - 1 + up + 7) << 3) | np.where(up, 0, n - 8)
    code_n = np.minimum(code_n, MAX_CODE)
    code_s = np.rint(a * 512.0).astype(np.int64)           # multiples of 2^-9: 0 .. 8 (8 is the smallest normal code)
    code = np.where(normal, code_n, code_s)
    return (np.where(fin, code, NAN_CODE) | sign).astype(np.uint8)


def decode(codes):
    """uint8 e4m3fn codes -> float64"""
    c = np.asarray(codes, np.uint8).astype(np.int64)
    E, M = (c >> 3) & 15, c & 7
    v = np.where(E == 0, M * 2.0 ** -9, np.ldexp((8 + M).astype(np.float64), E - 10))
    v = np.where((c & 0x7F) == NAN_CODE, np.nan, v)
    return np.where(c & 0x80, -v, v)


def quantize(values, group):
    """the rule applied group by group: values float32 [n], group int [n] -> (codes uint8 [n], exps int64 [n], one entry per element)"""
    v = np.asarray(values, np.float32)
    group = np.asarray(group, np.int64)
    a = np.where(np.isfinite(v), np.abs(v), np.float32(0)).astype(np.float64)
    amax = np.zeros(int(group.max()) + 1 if group.size else 0, np.float64)
    np.maximum.at(amax, group, a)
    e = exponent(amax)[group]
    with np.errstate(all="ignore"):
        codes = encode(np.ldexp(v.astype(np.float64), -e))
    return codes, e


def dequantize(codes, exps):
    """code x 2^e in float64 (exact)"""
    with np.errstate(all="ignore"):
        return np.ldexp(decode(codes), np.asarray(exps, np.int64))


def quantize_group(v):
    """one group, v float32 of any shape -> (codes of the same shape, e)"""
    v = np.asarray(v, np.float32)
    codes, e = quantize(v.reshape(-1), np.zeros(v.size, np.int64))
    return codes.reshape(v.shape), (int(e[0]) if v.size else 0)
