"""sparta_vbs_live_lists_host (VBR.live_lists): the rule of the live-block set as host code, against the numpy restatement of tests/_live.py.  No GPU.

The device kernels of k_live.hip are held to the same restatement in tests/test_live_gpu.py: one rule, two callers."""
import numpy as np
import pytest

import _live as L

cases = pytest.mark.parametrize("case", L.F32_CASES, ids=[L.case_id(c) for c in L.F32_CASES])


@cases
@pytest.mark.parametrize("name", L.MASKS)
def test_host_lists_follow_the_rule(case, name):
    key, br = case
    v, keep = L.geometry(key), L.mask(key, br, name)
    got = v.live_lists(keep, br)
    want = L.rule(v, keep, br)
    for k, w in zip(("sd_groups", "sd_count", "t_blocks", "t_count"), want):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], w), (k, got[k], w)
    # the counts of info are the sums over the lists
    info = got["info"]
    assert info[0] == 1 and info[1] == len(keep) and info[2] == int(np.count_nonzero(keep)) and info[7] == 0
    assert info[3] == len(got["sd_groups"]) and info[4] == int(got["sd_count"].sum()) == int((got["sd_groups"] >= 0).sum())
    assert info[5] == len(got["t_blocks"]) and info[6] == int(got["t_count"].sum()) == int((got["t_blocks"] >= 0).sum())


@cases
def test_all_live_reproduces_the_unmasked_lists(case):
    """every group of every block-row in order, every block column's whole list in block-row order: what the kernels walk without a live set"""
    key, br = case
    v = L.geometry(key)
    T = L.table(key, br)
    got = v.live_lists(np.ones(len(T), np.uint8), br)
    b0, b1 = (0, v.block_rows) if br is None else br
    w = int(v.block_col_size)
    groups = [(int(v.nzcount[ib]) * w + 31) // 32 if v.row_part[ib + 1] > v.row_part[ib] else 0 for ib in range(b0, b1)]
    assert np.array_equal(got["sd_count"], groups)
    assert np.array_equal(got["sd_groups"], np.concatenate([np.arange(g) for g in groups] + [np.zeros(0, int)]))
    # the list of a block column: its blocks of height > 0, ascending block number = block-row order (the order of build_spmm_t_index)
    n_all, bcol = T[:, 2], T[:, 3] & 0xffffffff
    block_cols = (int(v.cols) - 1) // w + 1
    lists = [np.flatnonzero((bcol == j) & (n_all > 0)) for j in range(block_cols)]
    assert np.array_equal(got["t_count"], [len(x) for x in lists])
    assert np.array_equal(got["t_blocks"], np.concatenate(lists + [np.zeros(0, int)]))


def test_a_straddling_group_lives_through_either_block():
    """w48: group 1 of a block-row (stored columns 32..63) overlaps blocks 0 and 1; it is dead only when both are"""
    v = L.geometry("w48")
    T = L.table("w48", None)
    brow = T[:, 3] >> 32
    ib = int(np.flatnonzero(np.bincount(brow) >= 2)[0])
    first = int(np.flatnonzero(brow == ib)[0])
    goff = int(sum((int(v.nzcount[r]) * 48 + 31) // 32 for r in range(ib)))
    for k0, k1, want in ((1, 0, True), (0, 1, True), (0, 0, False)):
        keep = np.ones(len(T), np.uint8)
        keep[first], keep[first + 1] = k0, k1
        got = v.live_lists(keep)
        assert (1 in got["sd_groups"][goff:goff + got["sd_count"][ib]]) == want


def test_bad_arguments_are_refused():
    v = L.geometry("small")
    with pytest.raises(ValueError):
        v.live_lists(np.ones(3, np.uint8))
    with pytest.raises(Exception):
        v.live_lists(np.ones(4, np.uint8), (2, 1))
