"""CPU checks of the poison helpers of tests/_util.py, which tests/test_poison_gpu.py relies on: for every geometry and poison placement the reference has
elements that must stay clean and elements that must turn non-finite, few or none that the contract leaves open, its clean elements are the unpoisoned
reference bit for bit, and the oracle's VBR::multiply agrees with it on which elements are finite."""
import numpy as np
import pytest

import _util as U
from oracle import oracle as O

N = 40
GEOS = [(k, dt) for k in U.POISON_F32 for dt in (0,)] + [(k, dt) for k in U.POISON_H16 for dt in (1, 2)]


def operand(shape, seed, dtype):
    return U.edge_round(np.random.default_rng(seed).uniform(-1, 1, shape), dtype)


def masks_ok(want, clean, dirty, open_, want0, open_cap):
    assert clean.any() and dirty.any()
    assert open_.sum() <= open_cap * open_.size, open_.mean()
    assert np.isfinite(want[clean]).all() and not np.isfinite(want[dirty]).any()
    assert np.array_equal(want[clean].view(np.uint64), want0[clean].view(np.uint64))
    assert not (clean & dirty).any() and (clean | dirty | open_).all()


@pytest.mark.parametrize("key,dtype", GEOS)
def test_forward_reference_on_the_written_out_geometries(key, dtype):
    v = U.poison_geometries()[key]
    hts = np.diff(v.row_part)
    assert list(hts) == U.POISON_HEIGHTS[key] and v.cols == U.POISON_COLS[key] and v.cols % v.block_col_size != 0
    sets = [tuple(U.poison_present(ib)) for ib in range(8)]
    assert len(set(sets)) == 8 and list(v.nzcount) == [6] * 8
    D, stored = U.edge_dense(v, dtype), U.stored_mask(v)
    assert (D[stored] != 0).all(), "a stored value inside cols is 0 (after rounding)"
    B = operand((v.cols, N), 1, dtype)
    want0 = U.poison_reference(D, stored, B)[0]
    assert np.allclose(want0, D @ B, rtol=0, atol=1e-12)
    for c, j in U.POISON_B_PLACEMENTS:
        for kind in U.POISON_VALUES:
            Bp = U.poisoned(B, U.block_col_rows(v, c), kind, j)
            want, clean, dirty, open_ = U.poison_reference(D, stored, Bp)
            masks_ok(want, clean, dirty, open_, want0, 0.0)
            rows_clean = np.concatenate([np.arange(v.rows)[U.block_row_rows(v, r)] for r in (c, (c - 3) % 8)])         # the block-rows that do not store c
            cols_clean = np.ones(N, bool)
            if j is not None:
                cols_clean[:] = False
                cols_clean[j] = True
            expect = np.zeros_like(clean)
            expect[np.ix_(rows_clean, cols_clean)] = True
            expect[:, ~cols_clean] = True
            assert np.array_equal(clean, expect)
            if dtype == 0:          # the oracle's VBR::multiply (column-major operands) never reads B outside a stored block column either
                with np.errstate(all="ignore"):
                    Co = O.vbr_multiply(v.rows, v.cols, v.block_col_size, v.row_part, v.nzcount, v.jab, v.mab, np.ascontiguousarray(Bp.T, np.float32).reshape(-1), N)
                assert np.array_equal(np.isfinite(Co.reshape(N, v.rows).T), np.isfinite(want)), (key, c, j, kind)


@pytest.mark.parametrize("key,dtype", GEOS)
def test_transposed_and_sddmm_references(key, dtype):
    v = U.poison_geometries()[key]
    for br in (None, (2, 6)):
        D, stored = U.edge_dense(v, dtype, br=br), U.stored_mask(v, br)
        X, Y = operand((D.shape[0], N), 2, dtype), operand((v.cols, N), 3, dtype)
        want0 = U.poison_reference_t(D, stored, X)[0]
        G0 = U.poison_reference_sddmm(v, X, Y, br)[0]
        assert np.array_equal(G0, U.edge_sample(v, X @ Y.T, br))
        for r in (3, 7) if br is None else (3, 5):
            for j in (None, 37):
                Xp = U.poisoned(X, U.block_row_rows(v, r, br), "mix", j)
                want, clean, dirty, open_ = U.poison_reference_t(D, stored, Xp)
                masks_ok(want, clean, dirty, open_, want0, 0.0)
                for c in (r, (r + 3) % 8):                                  # the block columns block-row r does not store
                    assert clean[U.block_col_rows(v, c)].all()
            G, gclean, gdirty = U.poison_reference_sddmm(v, U.poisoned(X, U.block_row_rows(v, r, br), "mix"), Y, br)
            assert gclean.any() and gdirty.any() and np.array_equal(G[gclean], G0[gclean]) and not np.isfinite(G[gdirty]).any()
            lo = [off for off, r0, h, _, _ in U.edge_blocks(v, br) if r0 == U.block_row_rows(v, r, br).start]
            assert gdirty.sum() == sum(h * valid for _, r0, h, _, valid in U.edge_blocks(v, br) if r0 == U.block_row_rows(v, r, br).start) and lo
        for c in (1, 7):
            G, gclean, gdirty = U.poison_reference_sddmm(v, X, U.poisoned(Y, U.block_col_rows(v, c), "mix"), br)
            assert gclean.any() and gdirty.any() and np.array_equal(G[gclean], G0[gclean]) and not np.isfinite(G[gdirty]).any()


@pytest.mark.parametrize("dtype", [0, 2])
def test_forward_reference_on_the_csr_matrix(dtype):
    m, g, w = U.poison_csr()
    assert (m.rows, m.cols) == (512, 512) and 5 <= m.nztot() / m.rows <= 7
    D, stored = U.csr_dense_and_stored(m, g, w)
    D = U.edge_round(D, dtype)
    assert (D != 0).sum() == m.nztot()
    B = operand((m.cols, N), 4, dtype)
    want0 = U.poison_reference(D, stored, B)[0]
    for c in U.PCSR_THIN:
        assert not stored[(np.arange(512) // 16) % 3 == 1][:, c * w:(c + 1) * w].any()
        for j in (None, 0, 37, -1):
            Bp = U.poisoned(B, slice(c * w, (c + 1) * w), "mix", j)
            want, clean, dirty, open_ = U.poison_reference(D, stored, Bp)
            if j is None:
                masks_ok(want, clean, dirty, open_, want0, 1.0 / 3.0)
                assert clean[(np.arange(512) // 16) % 3 == 1].all()
            else:
                col = np.arange(N)[j]
                masks_ok(want[:, [col]], clean[:, [col]], dirty[:, [col]], open_[:, [col]], want0[:, [col]], 1.0 / 3.0)
                assert np.delete(clean, col, axis=1).all()


@pytest.mark.parametrize("which,dtype", [("PUNI", 0), ("PUNI", 1), ("PSPLIT", 0), ("PSPLIT", 2)])
def test_forward_reference_on_the_clustered_and_the_split_matrix(which, dtype):
    """PUNI (the clustered generator of the union-tile tests) and PSPLIT (block-rows split into tiles and sparse rows), both thinned like PCSR: at most a
    third of the checked elements is open"""
    m, g, w = U.poison_union() if which == "PUNI" else U.poison_split()
    D, stored = U.csr_dense_and_stored(m, g, w)
    D = U.edge_round(D, dtype)
    assert (D != 0).sum() == m.nztot() and w == 32 and m.cols % w == 0
    perm = np.argsort(g, kind="stable")
    ids = np.unique(g)
    thinned = np.isin(g[perm], ids[1::3])                                    # rows, in the handle's order, of every third group
    assert thinned.any() and not thinned.all()
    B = operand((m.cols, N), 5, dtype)
    want0 = U.poison_reference(D, stored, B)[0]
    for c in U.PCSR_THIN:
        assert not stored[thinned][:, c * w:(c + 1) * w].any() and stored[~thinned][:, c * w:(c + 1) * w].all()
        for j in (None, 0, 37, -1):
            Bp = U.poisoned(B, slice(c * w, (c + 1) * w), "mix", j)
            want, clean, dirty, open_ = U.poison_reference(D, stored, Bp)
            if j is None:
                masks_ok(want, clean, dirty, open_, want0, 1.0 / 3.0)
                assert clean[thinned].all()
            else:
                col = np.arange(N)[j]
                masks_ok(want[:, [col]], clean[:, [col]], dirty[:, [col]], open_[:, [col]], want0[:, [col]], 1.0 / 3.0)
                assert np.delete(clean, col, axis=1).all()


@pytest.mark.parametrize("key", list(U.POISON_GATHERED))
def test_forward_reference_on_the_siblings_for_a_gathered_b(key):
    """P32G / P64G: the blocks of P32 / P64 on cols = 8 w, so that B splits into two slabs of 4 w rows"""
    v, of = U.poison_geometries()[key], U.poison_geometries()[U.POISON_GATHERED[key]]
    assert v.cols == 8 * v.block_col_size and np.array_equal(v.row_part, of.row_part) and np.array_equal(v.jab, of.jab)
    D, stored = U.edge_dense(v), U.stored_mask(v)
    assert (D[stored] != 0).all()
    B = operand((v.cols, N), 6, 0)
    want0 = U.poison_reference(D, stored, B)[0]
    for c, j in U.POISON_B_PLACEMENTS:
        want, clean, dirty, open_ = U.poison_reference(D, stored, U.poisoned(B, U.block_col_rows(v, c), "mix", j))
        masks_ok(want, clean, dirty, open_, want0, 0.0)
