"""The pattern rule and the block move of the repattern section of include/sparta_amd.h, restated in numpy / plain Python from the header's text (not from
the C++): the reference of tests/test_repattern_host.py, test_repattern_gpu.py and test_repattern_train_gpu.py."""
import numpy as np


class Invalid(Exception):
    """what the header answers with SPARTA_ERR_INVALID"""


def rule(cols, block_rows, w, row_part, nzcount, jab, b0, b1, keep=None, add=()):
    """-> (nzcount_out, jab_out, map, counts): the arrays of the whole matrix on the new pattern, per new block of the range the old block number in the
    range or -1, and {new nblocks, new nztot, new blocks in range, new nztot in range}"""
    row_part, nzcount, jab = (np.asarray(a, np.int64) for a in (row_part, nzcount, jab))
    block_cols = (cols - 1) // w + 1
    first = np.concatenate([[0], np.cumsum(nzcount)])                # first jab entry of every block-row
    n_old = int(first[b1] - first[b0])
    if keep is not None and len(keep) != n_old:
        raise Invalid("keep")
    added = {}
    for ib, jb in add:
        if not b0 <= ib < b1 or not 0 <= jb < block_cols:
            raise Invalid("an added block outside the range or the matrix")
        if jb in added.setdefault(ib, set()):
            raise Invalid("an added block given twice")
        added[ib].add(jb)
    nz_out, jab_out, bmap = nzcount.copy(), [int(j) for j in jab[:first[b0]]], []
    nz_range = 0
    for ib in range(b0, b1):
        cols_old = [int(j) for j in jab[first[ib]:first[ib + 1]]]
        if any(b <= a for a, b in zip(cols_old, cols_old[1:])) or any(not 0 <= j < block_cols for j in cols_old):
            raise Invalid("jab not strictly ascending inside a block-row of the range")
        number = {j: int(first[ib] - first[b0]) + k for k, j in enumerate(cols_old)}          # block column -> old block number in the range
        if added.get(ib, set()) & set(cols_old):
            raise Invalid("an added block is stored by the old pattern")
        kept = [j for j in cols_old if keep is None or keep[number[j]] != 0]
        new = sorted(kept + list(added.get(ib, ())))
        jab_out += new
        bmap += [number.get(j, -1) if j in kept else -1 for j in new]
        nz_out[ib] = len(new)
        nz_range += len(new) * int(row_part[ib + 1] - row_part[ib]) * w
    jab_out += [int(j) for j in jab[first[b1]:]]
    nztot = int((np.diff(row_part) * nz_out).sum()) * w
    counts = np.array([len(jab_out), nztot, len(bmap), nz_range], np.int64)
    return nz_out, np.array(jab_out, np.int64), np.array(bmap, np.int32), counts


def table(cols, w, row_part, nzcount, jab, b0, b1):
    """per stored block of the block-rows [b0, b1), mab order: (element offset into the range's slice of mab, n_all = h * w)"""
    first = np.concatenate([[0], np.cumsum(nzcount)])
    out, off = [], 0
    for ib in range(b0, b1):
        h = int(row_part[ib + 1] - row_part[ib])
        for _ in range(int(first[ib + 1] - first[ib])):
            out.append((off, h * w))
            off += h * w
    return out, off


def move(t_old, t_new, bmap, S, n_new):
    """S (the old range's slice of mab, any 4-byte type) moved: uint32 words of the new range's slice.  Every word belongs to one block."""
    S = np.ascontiguousarray(S).view(np.uint32)
    D = np.full(n_new, 0xDEADBEEF, np.uint32)
    for (off, n_all), m in zip(t_new, bmap):
        if m >= 0:
            assert t_old[m][1] == n_all
            D[off:off + n_all] = S[t_old[m][0]:t_old[m][0] + n_all]
        else:
            D[off:off + n_all] = 0                                  # +0.0f
    return D


def move_vbr(v, new_arrays, bmap, b0, b1, S):
    """the move between the ranges [b0, b1) of a VBR-like v (cols, block_col_size, row_part, nzcount, jab) and of (nzcount_out, jab_out)"""
    w = int(v.block_col_size)
    t_old, _ = table(v.cols, w, v.row_part, v.nzcount, v.jab, b0, b1)
    t_new, n_new = table(v.cols, w, v.row_part, new_arrays[0], new_arrays[1], b0, b1)
    return move(t_old, t_new, bmap, S, n_new)
