"""numpy restatements for the dense <-> blocks feature, written from the text of include/sparta_amd.h ("DENSE <-> BLOCKS"), not from the library's code:
the grid score of sparta_dense_block_ssq and the pattern of VBR.from_block_mask."""
import numpy as np


def grid_n_in(rows, cols, row_part, w):
    """(block_rows, block_cols) int64: the elements of every grid block that lie inside the matrix"""
    row_part = np.asarray(row_part, np.int64)
    block_cols = (cols - 1) // w + 1
    widths = np.minimum(w, cols - np.arange(block_cols, dtype=np.int64) * w)
    return np.diff(row_part)[:, None] * widths[None, :]


def grid_ssq(D, row_part, w):
    """ssq[ib, jb] = the float64 sum of the float64 squares of the elements of D (rows x cols, any float type: widened exactly first) in rows
    row_part[ib] .. row_part[ib + 1] - 1 and columns jb * w .. min(cols, jb * w + w) - 1; a block without an element scores 0.0"""
    D = np.asarray(D)
    rows, cols = D.shape
    row_part = np.asarray(row_part, np.int64)
    block_rows, block_cols = len(row_part) - 1, (cols - 1) // w + 1
    out = np.zeros((block_rows, block_cols), np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        sq = D.astype(np.float64) ** 2
        for ib in range(block_rows):
            for jb in range(block_cols):
                out[ib, jb] = sq[row_part[ib]:row_part[ib + 1], jb * w:min(cols, jb * w + w)].sum()
    return out


def block_mask_arrays(rows, cols, row_part, w, mask):
    """(nzcount, jab, nztot) of the pattern whose block-row ib stores, in ascending order, the block columns jb with mask[ib, jb] != 0"""
    row_part = np.asarray(row_part, np.int64)
    block_rows, block_cols = len(row_part) - 1, (cols - 1) // w + 1
    assert np.shape(mask) == (block_rows, block_cols)
    nzcount, jab, nztot = [], [], 0
    for ib in range(block_rows):
        js = [jb for jb in range(block_cols) if mask[ib][jb] != 0]
        nzcount.append(len(js))
        jab += js
        nztot += len(js) * int(row_part[ib + 1] - row_part[ib]) * w
    return np.array(nzcount, np.int64), np.array(jab, np.int64), nztot


def geometry_block_mask(v):
    """(block_rows, block_cols) uint8: which grid blocks the VBR v stores"""
    mask = np.zeros((v.block_rows, (v.cols - 1) // int(v.block_col_size) + 1), np.uint8)
    q = 0
    for ib in range(v.block_rows):
        for _ in range(int(v.nzcount[ib])):
            mask[ib, int(v.jab[q])] = 1
            q += 1
    return mask


def select_mask(scores, sparsity):
    """the rule of prune.select on one layer without pruned blocks, by numpy: the floor(sparsity * n) lowest scores go (stable sort: ties to the lower index,
    a non-finite score counts as +Inf); returns the keep mask in the shape of scores"""
    s = np.asarray(scores, np.float64).reshape(-1)
    s = np.where(np.isfinite(s), s, np.inf)
    k = int(np.floor(sparsity * s.size))
    keep = np.ones(s.size, np.uint8)
    keep[np.argsort(s, kind="stable")[:k]] = 0
    return keep.reshape(np.shape(scores))
