"""sparta_vbs_spmm_t (A^T x dense on the stored blocks of a handle, k_spmm_t.hip) without a GPU: the entries are exported and refuse NULL
arguments, the kernels keep their state in registers, and the block-column index create builds (sparta_spmm_t_host_check walks it on the host)
gives y = A^T x, exactly on small-integer data."""
import ctypes as C

import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd import _lib
from sparta_amd._lib import lib

import _util as U
from test_code_object import _kernel_metadata
from test_sddmm_gpu import build_mats

_i64p, _f32p = C.POINTER(C.c_int64), C.POINTER(C.c_float)


def test_spmm_t_symbols_exported():
    for s in ("sparta_vbs_spmm_t", "sparta_spmm_t_host_check"):
        assert s in _lib.SYMBOLS and hasattr(lib, s)
    assert _lib.CREATE_TRANSPOSE == 2


def test_spmm_t_null_handle_is_invalid():
    Ct = (C.c_float * 4)()
    rc = lib.sparta_vbs_spmm_t(None, None, 1, 1, Ct, 1, 0, _lib.PTR_DEVICE, None, None)
    assert rc == _lib.ERR_INVALID
    msg = lib.sparta_last_error().decode()
    assert "sparta_vbs_spmm_t" in msg and "NULL" in msg, msg


def test_spmm_t_kernels_have_no_scratch_and_no_spills(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    ks = {n: m for n, m in kernels.items() if "vbs_spmm_t_" in n}
    # the product: fp32, fp16, bf16; the 16-bit image of set_values (k_update.hip): fp16, bf16
    assert len(ks) == 5 and sum("vbs_spmm_t_image_kernel" in n for n in ks) == 2, sorted(ks)
    for name, m in ks.items():
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == 0, (name, m)          # (operands go straight to registers: no LDS stage)


def host_check(v, x, br=None):
    b0, b1 = (0, v.block_rows) if br is None else br
    rp = np.ascontiguousarray(v.row_part, np.int64)
    nz = np.ascontiguousarray(v.nzcount, np.int64)
    jab = np.ascontiguousarray(v.jab, np.int64)
    mab = np.ascontiguousarray(v.mab, np.float32)
    x = np.ascontiguousarray(x, np.float32)
    y = np.full(v.cols, np.nan, np.float64)
    info = np.full(8, -1, np.int64)
    _lib.check(lib.sparta_spmm_t_host_check(v.rows, v.cols, v.block_rows, v.block_col_size, rp.ctypes.data_as(_i64p), nz.ctypes.data_as(_i64p),
                                            jab.ctypes.data_as(_i64p), mab.ctypes.data_as(_f32p), b0, b1, x.ctypes.data_as(_f32p),
                                            y.ctypes.data_as(C.POINTER(C.c_double)), info.ctypes.data_as(_i64p)))
    return y, info


def dense_of(v, br=None):
    """the dense (rows of the range) x cols matrix of the stored blocks, float64; positions past cols dropped"""
    b0, b1 = (0, v.block_rows) if br is None else br
    w = v.block_col_size
    r_lo = int(v.row_part[b0])
    D = np.zeros((int(v.row_part[b1]) - r_lo, v.cols))
    jo = mo = 0
    for ib in range(v.block_rows):
        r0, r1 = int(v.row_part[ib]), int(v.row_part[ib + 1])
        h, nb = r1 - r0, int(v.nzcount[ib])
        for b in range(nb):
            if b0 <= ib < b1:
                c0 = int(v.jab[jo + b]) * w
                c1 = min(c0 + w, v.cols)
                blk = v.mab[mo + b * w * h: mo + (b + 1) * w * h].astype(np.float64).reshape(w, h).T
                D[r0 - r_lo:r1 - r_lo, c0:c1] += blk[:, :c1 - c0]
        jo += nb
        mo += nb * h * w
    return D


def with_integer_values(v, seed):
    """the same pattern with small-integer values everywhere, the positions past cols of a ragged last block column included (they take no part)"""
    rng = np.random.default_rng(seed)
    u = sa.VBR()
    u.__dict__.update(v.__dict__)
    u.mab = rng.integers(-4, 5, int(v.nztot)).astype(np.float32)
    u._dev = u._dev_t = u._dev_tp = None
    return u


@pytest.fixture(scope="module")
def mats():
    return build_mats()


@pytest.mark.parametrize("key", ["grid1", "grid8", "grid32", "grid64", "jaccard", "padded"])
def test_index_walk_equals_numpy(mats, key):
    v = with_integer_values(mats[key], 5)
    x = np.random.default_rng(6).integers(-4, 5, v.rows).astype(np.float32)
    y, info = host_check(v, x)
    assert np.array_equal(y, dense_of(v).T @ x.astype(np.float64))
    assert info[0] == len(np.unique(v.jab))
    panels = -(-v.block_col_size // 32)
    assert info[1] == (-(-v.cols // v.block_col_size)) * panels and info[3] == 0 and info[2] >= 1


@pytest.mark.parametrize("key", sorted(set(U.TRAIN_F32 + U.TRAIN_H16)))
def test_index_walk_over_the_training_geometries(key):
    """the geometries of tests/test_train_geometry_gpu.py: w = 3 (29 of a panel's 32 columns masked), 13 with h = 1 and with block-rows of height 0, 48 and 96 (a panel
    of 16 / 32 behind full ones), 100 (32 + 32 + 32 + 4), 128 to 256 (four to eight panels per block column), heights up to 465, block-rows without a block"""
    v = with_integer_values(U.train_geometries()[key], 9)
    x = np.random.default_rng(10).integers(-4, 5, v.rows).astype(np.float32)
    y, info = host_check(v, x)
    assert np.array_equal(y, dense_of(v).T @ x.astype(np.float64))
    assert info[3] == 0                                               # no block column is split: one owner per element of y
    w = v.block_col_size
    assert info[0] == len(np.unique(v.jab)) and info[1] == (-(-v.cols // w)) * (-(-w // 32)) and info[2] >= 1


def test_index_walk_with_empty_block_columns_and_sub_range():
    m0 = sa.gen.uniform_random(200, 400, 700, seed=12)
    m = sa.CSR(200, 900, m0.rowptr, m0.colidx, m0.vals)             # columns 400 .. 899 hold nothing: block columns without a block
    g = np.arange(m.rows, dtype=np.int64) // 16
    v = with_integer_values(sa.VBR().fill_from_CSR_inplace(m, g, 8), 7)
    assert len(np.unique(v.jab)) < -(-v.cols // 8)
    x = np.random.default_rng(8).integers(-4, 5, v.rows).astype(np.float32)
    y, info = host_check(v, x)
    assert np.array_equal(y, dense_of(v).T @ x.astype(np.float64)) and info[0] == len(np.unique(v.jab))
    br = (3, 9)
    r_lo, r_hi = int(v.row_part[br[0]]), int(v.row_part[br[1]])
    jab_lo, jab_hi = int(np.sum(v.nzcount[:br[0]])), int(np.sum(v.nzcount[:br[1]]))
    y, info = host_check(v, x[r_lo:r_hi], br)
    assert np.array_equal(y, dense_of(v, br).T @ x[r_lo:r_hi].astype(np.float64))
    assert info[0] == len(np.unique(v.jab[jab_lo:jab_hi]))
