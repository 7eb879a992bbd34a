"""tests/_util.py: edge_geometries() is the table its docstring gives, and edge_dense() / edge_sample() -- the float64 reference of tests/test_edge_geometry_gpu.py,
plain numpy on the expanded arrays -- agree with the two host-side walks the project already trusts: the oracle's VBR::multiply (bit for bit on the integer
values) and the walk of the block-column index behind sparta_vbs_spmm_t.  No GPU."""
import numpy as np
import pytest

import _util as U
from oracle import oracle as O

TABLE = {       # key: rows, cols, w, block-rows, stored blocks, nztot
    "one": (1, 1, 1, 1, 1, 1), "rowvec": (1, 300, 32, 1, 10, 320), "colvec": (300, 1, 3, 43, 29, 606), "narrow32": (100, 20, 32, 4, 4, 3200),
    "empty": (130, 200, 32, 9, 0, 0), "corner": (130, 200, 32, 9, 1, 64), "zeros": (96, 160, 32, 4, None, None), "tall": (322, 96, 32, 2, 6, 30912),
    "heights": (391, 112, 16, 16, None, None), "dense": (96, 128, 64, 2, 4, 12288), "w1": (70, 70, 1, 3, 21, 490),
    "heights32": (391, 112, 32, 16, None, None), "tall64": (322, 192, 64, 2, 6, 61824),
    "corner64": (130, 200, 64, 9, 1, 128), "heights64": (391, 112, 64, 16, None, None),
}
BOTH = [(k, vs) for vs in ("int", "real") for k in TABLE]


def test_the_key_lists():
    assert set(U.EDGE_F32) | set(U.EDGE_H16) == set(TABLE) == set(U.edge_geometries("int")) == set(U.edge_geometries("real"))
    assert set(U.EDGE_H16) == {"rowvec", "narrow32", "empty", "corner", "zeros", "tall", "dense", "heights32", "tall64"}
    assert set(U.EDGE_F32) == set(TABLE) - {"heights32", "tall64"}
    assert {k for k in U.EDGE_F32 if U.edge_geometries("int")[k].block_col_size % 64 == 0} == {"dense", "corner64", "heights64"}       # the per-class kernels' widths
    for k in U.EDGE_H16:
        assert U.edge_geometries("int")[k].block_col_size % 32 == 0


@pytest.mark.parametrize("key,vs", BOTH, ids=["%s-%s" % kv for kv in BOTH])
def test_the_table_is_what_it_says(key, vs):
    v = U.edge_geometries(vs)[key]
    rows, cols, w, n_brows, n_blocks, nztot = TABLE[key]
    hts = np.diff(v.row_part)
    assert (v.rows, v.cols, v.block_col_size, v.block_rows) == (rows, cols, w, n_brows)
    assert v.row_part[0] == 0 and v.row_part[-1] == rows and (hts >= 0).all() and rows < 400
    assert len(v.jab) == v.nzcount.sum() and len(v.mab) == v.nztot == (hts * v.nzcount).sum() * w
    if n_blocks is not None:
        assert (len(v.jab), int(v.nztot)) == (n_blocks, nztot)
    block_cols = (cols - 1) // w + 1
    jo = 0
    for nb in v.nzcount:                                             # ascending block columns inside the matrix
        j = v.jab[jo:jo + nb]
        assert (np.diff(j) > 0).all() and (j >= 0).all() and (j < block_cols).all()
        jo += nb
    blocks = U.edge_blocks(v)
    zero_block = [not v.mab[off:off + h * w].any() for off, _, h, _, _ in blocks]
    for (off, _, h, c0, valid), z in zip(blocks, zero_block):
        if not z:
            assert v.mab[off:off + w * h].all()                      # no zero inside a block that is not all zeros, the positions past cols included
    if vs == "int":
        assert np.array_equal(v.mab, np.round(v.mab)) and np.abs(v.mab).max(initial=0) <= 3
    else:
        assert np.abs(v.mab).max(initial=0) < 1 and (len(v.mab) == 0 or not np.array_equal(v.mab, np.round(v.mab)))
    if key != "zeros":
        assert not any(zero_block)
    # ---- per geometry ----
    if key == "one":
        assert hts.tolist() == [1] and v.jab.tolist() == [0]
    if key == "rowvec":
        assert hts.tolist() == [1] and v.jab.tolist() == list(range(10)) and blocks[-1][4] == 12
    if key == "colvec":
        assert cols < w and hts.tolist() == [7] * 42 + [6]
        assert [int(n) for n in v.nzcount] == [0 if ib % 3 == 2 else 1 for ib in range(43)] and all(b[4] == 1 for b in blocks)
    if key == "narrow32":
        assert cols < w and hts.tolist() == [25] * 4 and v.nzcount.tolist() == [1] * 4 and all(b[4] == 20 for b in blocks)
    if key in ("empty", "corner", "corner64"):
        assert hts.tolist() == [16] * 8 + [2]
    if key == "corner64":
        assert v.nzcount.tolist() == [0] * 8 + [1] and v.jab.tolist() == [3] and blocks[0][1:] == (128, 2, 192, 8)
    if key == "empty":
        assert not v.nzcount.any() and v.nztot == 0 and len(v.mab) == 0 and len(v.jab) == 0
    if key == "corner":
        assert v.nzcount.tolist() == [0] * 8 + [1] and v.jab.tolist() == [6] and blocks[0][1:] == (128, 2, 192, 8)
    if key == "zeros":
        assert hts.tolist() == [24] * 4 and (v.nzcount > 0).all() and 8 <= len(blocks) <= 12 + 4
        assert zero_block == [q % 2 == 0 for q in range(len(blocks))] and len(blocks) >= 4
    if key in ("tall", "tall64"):
        assert hts.tolist() == [257, 65] and v.nzcount.tolist() == [3, 3] and v.jab.tolist() == [0, 1, 2] * 2 and cols == 3 * w and hts[0] > 4 * 64
    if key in ("heights", "heights32", "heights64"):
        assert hts.tolist() == list(U.EDGE_HEIGHTS) and hts[0] == hts[-1] == hts[2] == hts[13] == 0
        for h, nb in zip(hts, v.nzcount):
            assert (nb == 0) == (h in (0, 1, 64))
        frac = len(blocks) / float(12 - 2) / block_cols
        assert 0.3 < frac < 0.75, frac
        assert (cols % w != 0) == (key != "heights")
        if key != "heights":
            assert any(b[4] == cols % w for b in blocks)             # the ragged block column is stored somewhere
    if key == "dense":
        assert hts.tolist() == [48, 48] and v.nzcount.tolist() == [2, 2] and cols == 2 * w and np.count_nonzero(U.edge_dense(v)) == rows * cols
    if key == "w1":
        assert hts.tolist() == [1, 5, 64] and v.nzcount.tolist() == [7, 7, 7]


def test_both_value_sets_share_the_pattern():
    a, b = U.edge_geometries("int"), U.edge_geometries("real")
    for k in TABLE:
        for f in ("row_part", "nzcount", "jab"):
            assert np.array_equal(getattr(a[k], f), getattr(b[k], f)), (k, f)


def test_edge_round_is_round_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -9, -0.3, 0.0, 3e38, 65504.0], np.float32)
    bf = U.edge_round(x, 2)
    assert bf[:4].tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0]      # ties to even; below the tie: down
    assert np.array_equal(U.edge_round(x[:6], 1), x[:6].astype(np.float16).astype(np.float64))
    assert np.array_equal(U.edge_round(x, 0), x.astype(np.float64))


def test_edge_round_rounds_as_torch_does():
    import torch
    r = np.random.default_rng(3).uniform(-4, 4, 4096).astype(np.float32)
    assert np.array_equal(U.edge_round(r, 2), torch.from_numpy(r).to(torch.bfloat16).double().numpy())
    assert np.array_equal(U.edge_round(r, 1), torch.from_numpy(r).to(torch.float16).double().numpy())


@pytest.mark.parametrize("key", list(TABLE))
def test_dense_reference_equals_the_oracle_multiply_bit_for_bit(key):
    v = U.edge_geometries("int")[key]
    n = 5
    B = np.random.default_rng(11).integers(-3, 4, (v.cols, n)).astype(np.float64)
    want = U.edge_dense(v) @ B
    got = O.vbr_multiply(v.rows, v.cols, v.block_col_size, v.row_part, v.nzcount, v.jab, v.mab, B.T.astype(np.float32).reshape(-1), n)
    assert np.array_equal(got.reshape(n, v.rows).T, want.astype(np.float32))
    if v.block_rows > 2:                                             # a range of block-rows: the slice of the reference
        br = (1, v.block_rows - 1)
        r0, r1 = int(v.row_part[br[0]]), int(v.row_part[br[1]])
        assert np.array_equal(U.edge_dense(v, br=br), U.edge_dense(v)[r0:r1])
        lo, hi = U.edge_mab_slice(v, br)
        assert np.array_equal(U.edge_sample(v, U.edge_dense(v), None)[lo:hi], U.edge_sample(v, U.edge_dense(v)[r0:r1], br))


@pytest.mark.parametrize("key,vs", BOTH, ids=["%s-%s" % kv for kv in BOTH])
def test_dense_reference_transposed_equals_the_index_walk(key, vs):
    v = U.edge_geometries(vs)[key]
    x = np.random.default_rng(12).integers(-3, 4, v.rows).astype(np.float32)
    y, info = U.spmm_t_host_check(v, x)
    want = U.edge_dense(v).T @ x.astype(np.float64)
    if vs == "int":
        assert np.array_equal(y, want)
    else:
        assert np.allclose(y, want, rtol=0, atol=1e-12 * max(1.0, np.abs(want).max()))
    assert info[0] == len(set(v.jab.tolist()))                       # block columns that hold a block


def test_columns_and_rows_without_a_stored_block():
    """what the spmm_t tests lean on: on empty and corner (almost) every column of A -- every row of Ct -- lies in no stored block; colvec's one column does,
    but a third of its block-rows hold none: those rows of A are empty"""
    stored = {k: U.edge_dense(U.edge_geometries("int")[k], mab=np.ones(len(U.edge_geometries("int")[k].mab), np.float32)) != 0 for k in ("empty", "corner", "corner64", "colvec")}
    assert (~stored["empty"].any(axis=0)).sum() == 200 and (~stored["corner"].any(axis=0)).sum() == (~stored["corner64"].any(axis=0)).sum() == 192
    assert stored["colvec"].any(axis=0).all() and (~stored["colvec"].any(axis=1)).sum() == 14 * 7


@pytest.mark.parametrize("key", list(TABLE))
def test_sample_is_the_inverse_of_dense_on_the_stored_positions(key):
    v = U.edge_geometries("real")[key]
    inside = U.edge_sample(v, np.ones((v.rows, v.cols))) != 0          # the stored positions inside the matrix
    assert np.array_equal(U.edge_sample(v, U.edge_dense(v)), np.where(inside, v.mab, 0).astype(np.float64))
    assert (~inside).sum() == sum((w_ - valid) * h for _, _, h, _, valid in U.edge_blocks(v) for w_ in [v.block_col_size])
    M = np.random.default_rng(13).uniform(-1, 1, (v.rows, v.cols))
    G = U.edge_sample(v, M)
    mask = U.edge_dense(v, mab=np.ones(len(v.mab), np.float32))
    assert np.array_equal(U.edge_dense(v, mab=G.astype(np.float32)), (M * mask).astype(np.float32).astype(np.float64))
