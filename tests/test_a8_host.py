"""The rule of the fp8 weight image without a GPU: the numpy restatement (tests/_a8.py) against torch's CPU float32 -> float8_e4m3fn conversion on every code,
every midpoint between neighbouring codes and the floats next to each midpoint, and sparta_a8_quantize_group (the host code of the rule the quantise kernel
runs) against the restatement, bit for bit, on the cases where the rule can go wrong."""
import numpy as np
import pytest

import sparta_amd as sa

import _a8 as A8

f32 = np.float32


def _finite_codes():
    c = np.arange(256, dtype=np.uint8)
    return c[(c & 0x7F) != A8.NAN_CODE]


def _torch_codes(x):
    torch = pytest.importorskip("torch")
    if not hasattr(torch, "float8_e4m3fn"):
        pytest.skip("this torch has no float8_e4m3fn")
    return torch.from_numpy(np.ascontiguousarray(x, f32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def test_decode_encode_round_trip():
    c = _finite_codes()
    v = A8.decode(c)
    assert np.array_equal(A8.encode(v), c)
    assert v.max() == 448.0 and np.abs(v[v != 0]).min() == 2.0 ** -9
    assert A8.encode(np.array([np.nan, np.inf, -np.inf])).tolist() == [0x7F, 0x7F, 0xFF]
    assert A8.encode(np.array([0.0, -0.0])).tolist() == [0x00, 0x80]


def test_restatement_equals_torch_on_codes_midpoints_and_their_neighbours():
    pos = np.sort(A8.decode(np.arange(0, 0x7F, dtype=np.uint8)))              # 0 .. 448, ascending
    mid = (pos[:-1] + pos[1:]) / 2                                           # one more mantissa bit: exact in float32
    assert np.array_equal(mid.astype(f32).astype(np.float64), mid)
    m32 = mid.astype(f32)
    pts = np.concatenate([pos.astype(f32), m32, np.nextafter(m32, f32(0)), np.nextafter(m32, f32(1000)),
                          f32([2.0 ** -6, np.nextafter(f32(2.0 ** -6), f32(0)), 2.0 ** -9, 2.0 ** -10, np.nextafter(f32(2.0 ** -10), f32(1)), 448.0,
                               np.nextafter(f32(448.0), f32(0)), 1e-30, 1e-45])])
    pts = np.concatenate([pts, -pts])
    assert pts.dtype == f32 and np.abs(pts).max() == 448.0
    got = A8.encode(pts.astype(np.float64))
    assert np.array_equal(got, _torch_codes(pts)), np.flatnonzero(got != _torch_codes(pts))[:8]
    assert got[np.flatnonzero(pts == 0)].tolist().count(0x80) >= 1             # -0.0 keeps its sign


def _check(v, rows=None, kcols=None):
    """sparta_a8_quantize_group on v [kcols][ld] (rows <= ld) against the restatement on the rows x kcols values it covers; returns (codes, e)"""
    v = np.ascontiguousarray(v, f32)
    rows = v.shape[1] if rows is None else rows
    kcols = v.shape[0] if kcols is None else kcols
    codes, e = sa.a8_quantize_group((v, rows), kcols)
    want, we = A8.quantize_group(v[:kcols, :rows])
    assert codes.shape == (kcols, rows) and e == we, (e, we)
    assert np.array_equal(codes, want), np.argwhere(codes != want)[:8]
    return codes, e


def _rand(seed, kcols=32, ld=32):
    v = np.random.default_rng(seed).uniform(-1, 1, (kcols, ld)).astype(f32)
    v[v == 0] = 0.5
    return v


def test_amax_at_the_edge_of_an_exponent():
    """amax = 448 * 2^k still takes e = k; one ulp above it takes k + 1"""
    for k in (-130, -126, -100, -20, -9, -1, 0, 1, 7, 40, 100, 119):
        v = _rand(300 + k) * f32(2.0) ** f32(max(k, -126)) * f32(2.0) ** f32(min(k + 126, 0))
        v[3, 5] = f32(448.0) * f32(2.0) ** f32(max(k, -126)) * f32(2.0) ** f32(min(k + 126, 0))
        _, e = _check(v)
        assert e == max(k, -126), (k, e)
        v[3, 5] = -np.nextafter(v[3, 5], f32(np.inf))
        _, e = _check(v)
        assert e == max(k + 1, -126), (k, e)


def test_zeros_one_huge_element_and_minus_zero():
    codes, e = _check(np.zeros((32, 32), f32))
    assert e == 0 and not codes.any()
    v = _rand(7) * f32(1e-3)
    v[10, 3] = 3e4
    codes, e = _check(v)
    assert e == 7 and codes[10, 3] != 0
    v = _rand(8)
    v[0, 0] = -0.0
    codes, _ = _check(v)
    assert codes[0, 0] == 0x80
    v = np.zeros((32, 32), f32)
    v[1, 1] = -0.0
    codes, e = _check(v)
    assert e == 0 and codes[1, 1] == 0x80


def test_non_finite_elements_change_neither_the_exponent_nor_the_other_codes():
    v = _rand(9)
    base, e0 = _check(v)
    for bad, code in ((np.nan, None), (np.inf, 0x7F), (-np.inf, 0xFF)):
        w = v.copy()
        w[5, 6] = bad
        codes, e = _check(w)
        assert e == e0
        assert codes[5, 6] & 0x7F == 0x7F and (code is None or codes[5, 6] == code)
        codes[5, 6] = base[5, 6]
        assert np.array_equal(codes, base)
    w = np.full((32, 32), np.nan, f32)
    codes, e = _check(w)
    assert e == 0 and np.all(codes & 0x7F == 0x7F)


@pytest.mark.parametrize("kcols", [32, 64])
@pytest.mark.parametrize("rows,ld", [(32, 32), (17, 17), (17, 40), (1, 33), (0, 5)])
def test_rows_leading_dimension_and_width(kcols, rows, ld):
    v = _rand(20 + rows + ld, kcols, ld)
    v[:, rows:] = 1e6                                     # rows the group does not cover must not count
    _, e = _check(v, rows, kcols)
    assert e <= -8 or rows == 0


def test_exponent_at_the_clamps():
    """the lower clamp is reached by subnormal and tiny groups; no finite float reaches the upper one (FLT_MAX gives 120)"""
    v = _rand(30) * f32(1e-38) * f32(1e-5)
    assert np.abs(v).max() < np.finfo(f32).tiny
    codes, e = _check(v)
    assert e == -126
    v = _rand(31) * f32(2.0 ** -126) * f32(100.0)
    _, e = _check(v)
    assert e == -126
    v = _rand(32)
    v[2, 2] = np.finfo(f32).max
    codes, e = _check(v)
    assert e == 120 and codes[2, 2] == 0x78                 # 2^128 (rounded up) / 2^120 = 256
    assert A8.exponent(np.float64(2.0) ** 140) == 127


def test_bad_arguments():
    with pytest.raises(sa.SpartaError):
        sa.a8_quantize_group(np.zeros((16, 32), f32))
    with pytest.raises(sa.SpartaError):
        sa.a8_quantize_group((np.zeros((32, 40), f32), 33))
