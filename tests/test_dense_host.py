"""The host side of the dense <-> blocks feature, without a GPU: the three C-ABI entries are exported and declared, and VBR.from_block_mask builds the
pattern the header's text describes -- held to the numpy restatement of tests/_dense.py on the block mask of every fp32 edge geometry (block-rows of
height 0, patterns without a block, ragged last block columns), through block_table() and a save / load round trip."""
import ctypes as C

import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd import _lib

import _dense as DN
import _util as U

NAMES = ("sparta_dense_block_ssq", "sparta_vbs_gather_dense", "sparta_vbs_scatter_dense")


def test_the_three_entries_are_exported():
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n in _lib.SYMBOLS and hasattr(raw, n) and getattr(_lib.lib, n).argtypes, n
    for n in ("dense_block_ssq", "sparsify"):
        assert callable(getattr(sa, n)), n
    for n in ("gather_dense", "scatter_dense", "to_dense"):
        assert callable(getattr(sa.DeviceVBS, n)), n
    assert callable(sa.VBR.from_block_mask)


def test_null_handles_come_back_as_status_codes():
    assert _lib.lib.sparta_vbs_gather_dense(None, None, 0, 0, 0, None, None, None) == _lib.ERR_INVALID
    assert _lib.lib.sparta_vbs_scatter_dense(None, None, None, 0, 0, 0, 0, None, None) == _lib.ERR_INVALID
    # the handle-free entry validates before it touches the GPU
    for args in ((None, 4, 7, _lib.F32, 4, 4, 1, 2, None, None),                   # a layout code that does not exist
                 (None, 4, _lib.ROW_MAJOR, 9, 4, 4, 1, 2, None, None),              # a dtype code that does not exist
                 (None, 3, _lib.ROW_MAJOR, _lib.F32, 4, 4, 1, 2, None, None),       # ldd < cols
                 (None, 3, _lib.COL_MAJOR, _lib.F32, 4, 2, 1, 2, None, None),       # ldd < rows
                 (None, 4, _lib.ROW_MAJOR, _lib.F32, 4, 4, 1, 0, None, None),       # block_col_size 0
                 (None, 4, _lib.ROW_MAJOR, _lib.F32, -1, 4, 1, 2, None, None),      # rows < 0
                 (None, 4, _lib.ROW_MAJOR, _lib.F32, 4, 4, 1, 2, None, None)):      # row_part NULL with block_rows > 0
        assert _lib.lib.sparta_dense_block_ssq(*args, None, None) == _lib.ERR_INVALID, args
    assert _lib.lib.sparta_dense_block_ssq(None, 4, _lib.ROW_MAJOR, _lib.F32, 4, 4, 0, 2, None, None, None, None) == _lib.OK          # no grid block: nothing to do


@pytest.mark.parametrize("key", U.EDGE_F32)
def test_from_block_mask_matches_the_restatement(key, tmp_path):
    v = U.edge_geometries("int")[key]
    w = int(v.block_col_size)
    mask = DN.geometry_block_mask(v)
    # the block mask agrees with the element mask of the geometry wherever a block has rows
    stored = U.stored_mask(v)
    for ib in range(v.block_rows):
        if v.row_part[ib + 1] > v.row_part[ib]:
            assert np.array_equal(stored[v.row_part[ib], ::w], mask[ib] != 0), (key, ib)
    nzcount, jab, nztot = DN.block_mask_arrays(v.rows, v.cols, v.row_part, w, mask)
    for m in (mask, mask.astype(np.float32) * -2.5, mask != 0):                       # non-zero is what counts, in any dtype
        p = sa.VBR.from_block_mask(v.rows, v.cols, v.row_part, w, m)
        assert (p.rows, p.cols, p.block_col_size, p.block_rows, p.block_cols) == (v.rows, v.cols, w, v.block_rows, mask.shape[1])
        assert np.array_equal(p.row_part, v.row_part) and np.array_equal(p.nzcount, nzcount) and np.array_equal(p.jab, jab)
        assert p.nztot == nztot == len(p.mab) and p.mab.dtype == np.float32 and not p.mab.any()
        # the edge geometries list their block columns in ascending order: the pattern is the geometry's own, block for block
        assert np.array_equal(p.nzcount, v.nzcount) and np.array_equal(p.jab, v.jab)
        assert np.array_equal(p.block_table(), v.block_table())
    path = tmp_path / "pattern.vbs"
    p.save(path)
    q = sa.VBR.load(path)
    assert np.array_equal(q.block_table(), v.block_table()) and np.array_equal(q.row_part, v.row_part) and np.array_equal(q.nzcount, nzcount)
    assert np.array_equal(q.jab, jab) and q.nztot == nztot and not q.mab.any()


def test_from_block_mask_of_an_all_zero_mask():
    v = U.edge_geometries("int")["heights"]
    w = int(v.block_col_size)
    p = sa.VBR.from_block_mask(v.rows, v.cols, v.row_part, w, np.zeros((v.block_rows, 7), np.uint8))
    assert p.nztot == 0 and len(p.jab) == 0 and not p.nzcount.any() and p.block_table().shape == (0, 4)
    full = sa.VBR.from_block_mask(v.rows, v.cols, v.row_part, w, np.ones((v.block_rows, 7)))
    assert full.nztot == v.rows * 7 * w and np.array_equal(full.jab, np.tile(np.arange(7), v.block_rows))
    assert np.array_equal(full.block_table()[:, 1].reshape(v.block_rows, 7), DN.grid_n_in(v.rows, v.cols, v.row_part, w))


def test_from_block_mask_refuses_a_mask_of_the_wrong_shape():
    rp = [0, 3, 3, 10]
    for bad in (np.ones((3, 2)), np.ones((2, 3)), np.ones(9), np.ones((3, 3, 1)), np.ones((4, 3))):
        with pytest.raises(ValueError):
            sa.VBR.from_block_mask(10, 9, rp, 4, bad)
    sa.VBR.from_block_mask(10, 9, rp, 4, np.ones((3, 3)))
    for rp_bad in ([0, 3, 2, 10], [1, 3, 10], [0, 3, 9]):
        with pytest.raises(ValueError):
            sa.VBR.from_block_mask(10, 9, rp_bad, 4, np.ones((len(rp_bad) - 1, 3)))
