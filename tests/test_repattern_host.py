"""sparta_vbs_repattern_host (the pattern rule of a repattern, host code, no GPU) and VBR.repattern against the numpy restatement of tests/_repattern.py.

Geometries: `small` and `zrows` as tests/test_prune_gpu.py defines them (copied), `heights` whole and as the range (3, 9), `empty`, `corner`, `dense` of the
edge geometries and `w13z` of the training geometries.  Keep masks: all, none, every second block, two seeded random masks.  Add lists: none, and one block
of each kind a geometry offers -- in front of a block-row's first stored block, behind its last, in an empty block-row, in the ragged last block column, in
a block-row of height 0.  Every refusal the header lists leaves the outputs as they were."""
import ctypes as C
import functools

import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd import _lib
from sparta_amd._lib import lib

import _util as U  # noqa: E402
import _repattern as R  # noqa: E402

_i64p, _i32p, _u8p = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


def _small():
    """3 x 5, w 4: heights 1 and 2, both block columns stored, the second ragged (one column): blocks of 4, 1, 8 and 2 elements inside the matrix"""
    a = U._edge_arrays(3, 5, 4, [1, 2], [[0, 1], [0, 1]])
    return U.sa_vbr(a, U._edge_values(a, "real", 7290))


def _zrows():
    """10 x 40, w 16: heights 4, 0, 6, 0 with blocks IN the block-rows of height 0 (blocks without an element: block b is still entry b of jab)"""
    a = U._edge_arrays(10, 40, 16, [4, 0, 6, 0], [[0, 2], [1, 2], [2], [0]])
    return U.sa_vbr(a, U._edge_values(a, "real", 7291))


GEOS = (("small", None), ("zrows", None), ("heights", None), ("heights", (3, 9)), ("empty", None), ("corner", None), ("dense", None), ("w13z", None))
GEO_IDS = ["%s%s" % (k, "" if br is None else "-range") for k, br in GEOS]
KEEPS = ("all", "none", "second", "rand0", "rand1")
ADD_KINDS = ("front", "behind", "empty_row", "ragged", "height0")


@functools.lru_cache(maxsize=None)
def geometry(key):
    if key == "small":
        return _small()
    if key == "zrows":
        return _zrows()
    if key in U.TRAIN_F32:
        return U.train_geometries()[key]
    return U.edge_geometries("real")[key]


def rng_of(v, br):
    b0, b1 = br or (0, v.block_rows)
    first = np.concatenate([[0], np.cumsum(v.nzcount)])
    return b0, b1, int(first[b0]), int(first[b1])


def keep_mask(v, br, kind):
    b0, b1, q0, q1 = rng_of(v, br)
    n = q1 - q0
    if kind == "all":
        return None
    if kind == "none":
        return np.zeros(n, np.uint8)
    if kind == "second":
        return (np.arange(n) % 2 == 0).astype(np.uint8)
    return (np.random.default_rng(9300 + int(kind[-1]) + n).random(n) < 0.5).astype(np.uint8)


def add_candidates(v, br):
    """kind -> one (block-row, block column) of that kind in the range, where the geometry has one"""
    b0, b1, _, _ = rng_of(v, br)
    w = int(v.block_col_size)
    block_cols = (v.cols - 1) // w + 1
    ragged = v.cols % w != 0
    first = np.concatenate([[0], np.cumsum(v.nzcount)])
    out = {}
    for ib in range(b0, b1):
        stored = [int(j) for j in v.jab[first[ib]:first[ib + 1]]]
        h = int(v.row_part[ib + 1] - v.row_part[ib])
        free = [j for j in range(block_cols) if j not in stored]
        if stored and stored[0] > 0:
            out.setdefault("front", (ib, stored[0] - 1))
        if stored and stored[-1] < block_cols - 1:
            out.setdefault("behind", (ib, stored[-1] + 1))
        if not stored and h > 0:
            out.setdefault("empty_row", (ib, block_cols // 2))
        if ragged and block_cols - 1 in free and h > 0:
            out.setdefault("ragged", (ib, block_cols - 1))
        if h == 0 and free:
            out.setdefault("height0", (ib, free[0]))
    return out


def add_lists(v, br):
    c = add_candidates(v, br)
    lists = {"noadd": []}
    for k, pair in c.items():
        lists[k] = [pair]
    if len(c) > 1:
        lists["mixed"] = sorted(set(c.values()), reverse=True)       # several at once, given in descending order: the rule sorts
    return lists


CASES = [(g, k, a) for g in GEOS for k in KEEPS for a in add_lists(geometry(g[0]), g[1])]
CASE_IDS = ["%s-%s-%s" % (GEO_IDS[GEOS.index(g)], k, a) for g, k, a in CASES]


def raw(v, br, keep, add, nz_out, jab_out, map_out, counts, jab=None, n_add=None, add_null=False):
    """the C entry on the arrays of v; outputs are numpy arrays or None"""
    b0, b1, _, _ = rng_of(v, br)
    rp, nz = np.ascontiguousarray(v.row_part, np.int64), np.ascontiguousarray(v.nzcount, np.int64)
    jab = np.ascontiguousarray(v.jab if jab is None else jab, np.int64)
    addv = np.ascontiguousarray(np.asarray(add, np.int64).reshape(-1, 2))
    p = lambda a, t: None if a is None or a.size == 0 else a.ctypes.data_as(t)
    return lib.sparta_vbs_repattern_host(v.cols, v.block_rows, v.block_col_size, rp.ctypes.data_as(_i64p), nz.ctypes.data_as(_i64p), p(jab, _i64p), b0, b1,
                                         p(keep, _u8p), None if add_null else p(addv, _i64p), len(addv) if n_add is None else n_add, p(nz_out, _i64p),
                                         p(jab_out, _i64p), p(map_out, _i32p), None if counts is None else counts.ctypes.data_as(_i64p))


def test_every_kind_of_added_block_is_exercised():
    kinds = set()
    for key, br in GEOS:
        kinds |= set(add_candidates(geometry(key), br))
    assert kinds == set(ADD_KINDS), kinds
    # the builder's output and the written-out geometries have strictly ascending block columns inside every block-row: the rule's precondition
    for key, _ in GEOS:
        v = geometry(key)
        first = np.concatenate([[0], np.cumsum(v.nzcount)])
        for ib in range(v.block_rows):
            assert np.all(np.diff(v.jab[first[ib]:first[ib + 1]]) > 0), (key, ib)
    m = sa.gen.uniform_random(300, 260, 4000, seed=3)
    vb = sa.VBR().fill_from_CSR_inplace(m, sa.BlockingEngine(tau=0.5, col_block_size=16).GetGrouping(m), 16)
    first = np.concatenate([[0], np.cumsum(vb.nzcount)])
    assert all(np.all(np.diff(vb.jab[first[ib]:first[ib + 1]]) > 0) for ib in range(vb.block_rows))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_rule_and_host_move_equal_the_restatement(case, tmp_path):
    (key, br), kkind, akind = case
    v = geometry(key)
    b0, b1, q0, q1 = rng_of(v, br)
    keep, add = keep_mask(v, br, kkind), add_lists(v, br)[akind]
    nz_w, jab_w, map_w, counts_w = R.rule(v.cols, v.block_rows, int(v.block_col_size), v.row_part, v.nzcount, v.jab, b0, b1, keep, add)
    # counting call, then the full call
    counts = np.zeros(4, np.int64)
    assert raw(v, br, keep, add, None, None, None, counts) == _lib.OK
    assert np.array_equal(counts, counts_w)
    nz_o, jab_o, map_o = np.full(v.block_rows, -7, np.int64), np.full(counts[0], -7, np.int64), np.full(counts[2], -7, np.int32)
    assert raw(v, br, keep, add, nz_o, jab_o, map_o, counts) == _lib.OK
    assert np.array_equal(nz_o, nz_w) and np.array_equal(jab_o, jab_w) and np.array_equal(map_o, map_w) and np.array_equal(counts, counts_w)
    # properties, stated on their own
    first_n = np.concatenate([[0], np.cumsum(nz_o)])
    for ib in range(b0, b1):
        assert np.all(np.diff(jab_o[first_n[ib]:first_n[ib + 1]]) > 0)
    old = map_o[map_o >= 0]
    assert len(set(old.tolist())) == len(old) and np.all(old < q1 - q0)
    assert np.array_equal(np.sort(old), np.arange(q1 - q0) if keep is None else np.flatnonzero(keep))
    assert int((map_o < 0).sum()) == len(add)
    assert np.array_equal(nz_o[:b0], v.nzcount[:b0]) and np.array_equal(nz_o[b1:], v.nzcount[b1:])
    assert np.array_equal(jab_o[:q0], v.jab[:q0]) and np.array_equal(jab_o[first_n[b1]:], v.jab[q1:])
    # VBR.repattern: the same arrays, the restated move, and a round trip through the container (which checks the structural invariants)
    new, bmap = v.repattern(keep=keep, add=add, block_row_range=br)
    assert np.array_equal(bmap, map_w) and bmap.dtype == np.int32
    assert np.array_equal(new.nzcount, nz_w) and np.array_equal(new.jab, jab_w) and np.array_equal(new.row_part, v.row_part)
    assert (new.rows, new.cols, new.block_col_size, new.nztot) == (v.rows, v.cols, v.block_col_size, int(counts_w[1]))
    lo, hi = U.edge_mab_slice(v, (b0, b1))
    lo_n, hi_n = U.edge_mab_slice(new, (b0, b1))
    want = R.move_vbr(v, (nz_w, jab_w), map_w, b0, b1, v.mab[lo:hi])
    got = new.mab.view(np.uint32)
    assert lo_n == lo and np.array_equal(got[lo_n:hi_n], want)
    assert np.array_equal(got[:lo_n], v.mab.view(np.uint32)[:lo]) and np.array_equal(got[hi_n:], v.mab.view(np.uint32)[hi:])
    pattern_only, _ = v.repattern(keep=keep, add=add, block_row_range=br, values=False)
    assert np.array_equal(pattern_only.jab, new.jab) and not pattern_only.mab.any() and pattern_only.mab.size == new.mab.size
    if new.nztot > 0 or len(new.jab) > 0:
        path = tmp_path / "v.vbs"
        new.save(path)
        back = sa.VBR.load(path)
        assert np.array_equal(back.jab, new.jab) and np.array_equal(back.nzcount, new.nzcount) and np.array_equal(back.mab.view(np.uint32), got)


def test_move_carries_payloads_on_the_host():
    v = geometry("small")
    mab = v.mab.copy().view(np.uint32)
    mab[0], mab[5], mab[6] = 0x7FC12345, 0x80000000, 0xFF800001          # a NaN with a payload, -0.0, a signalling NaN
    w = sa.VBR.from_arrays(v.rows, v.cols, v.block_col_size, v.row_part, v.nzcount, v.jab, mab.view(np.float32))
    new, bmap = w.repattern(keep=np.array([1, 0, 1, 1], np.uint8))
    assert list(bmap) == [0, 2, 3]
    assert np.array_equal(new.mab.view(np.uint32), np.concatenate([mab[0:4], mab[8:24]]))


REFUSALS = ("unsorted", "jab_out_of_range", "add_outside_range", "add_row_negative", "add_col_too_large", "add_col_negative", "add_twice", "add_stored_kept",
            "add_stored_dead", "add_null", "jab_null", "one_output_null", "nzcount_out_null", "counts_null", "negative_n_add", "bad_range")


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals_write_nothing(what):
    v, br = geometry("heights"), (3, 9)
    b0, b1, q0, q1 = rng_of(v, br)
    first = np.concatenate([[0], np.cumsum(v.nzcount)])
    block_cols = (v.cols - 1) // int(v.block_col_size) + 1
    row = next(ib for ib in range(b0, b1) if v.nzcount[ib] >= 2 and v.nzcount[ib] < block_cols)          # a block-row with two blocks and a free column
    stored = [int(j) for j in v.jab[first[row]:first[row + 1]]]
    free = next(j for j in range(block_cols) if j not in stored)
    keep = np.ones(q1 - q0, np.uint8)
    keep[first[row] - q0] = 0                                                                            # the row's first block is dead
    kw, add, jab = {}, [(row, free)], None
    if what == "unsorted":
        jab = v.jab.copy()
        jab[first[row]], jab[first[row] + 1] = jab[first[row] + 1], jab[first[row]]
    elif what == "jab_out_of_range":
        jab = v.jab.copy()
        jab[first[row + 1] - 1] = block_cols
    elif what == "add_outside_range":
        add = [(b1, 0)]
    elif what == "add_row_negative":
        add = [(-1, 0)]
    elif what == "add_col_too_large":
        add = [(row, block_cols)]
    elif what == "add_col_negative":
        add = [(row, -1)]
    elif what == "add_twice":
        add = [(row, free), (b0, 0), (row, free)]
    elif what == "add_stored_kept":
        add = [(row, stored[1])]
    elif what == "add_stored_dead":
        add = [(row, stored[0])]
    elif what == "add_null":
        kw = {"add_null": True}
    elif what == "negative_n_add":
        kw = {"n_add": -1}
    counts = np.full(4, -7, np.int64)
    nz_o, jab_o, map_o = np.full(v.block_rows, -7, np.int64), np.full(len(v.jab) + 8, -7, np.int64), np.full(q1 - q0 + 8, -7, np.int32)
    outs = [nz_o, jab_o, map_o, counts]
    if what == "jab_null":
        rc = lib.sparta_vbs_repattern_host(v.cols, v.block_rows, v.block_col_size, np.ascontiguousarray(v.row_part).ctypes.data_as(_i64p),
                                           np.ascontiguousarray(v.nzcount).ctypes.data_as(_i64p), None, b0, b1, None, None, 0, nz_o.ctypes.data_as(_i64p),
                                           jab_o.ctypes.data_as(_i64p), map_o.ctypes.data_as(_i32p), counts.ctypes.data_as(_i64p))
    elif what == "one_output_null":
        rc = raw(v, br, keep, add, nz_o, jab_o, None, counts, **kw)
    elif what == "nzcount_out_null":
        rc = raw(v, br, keep, add, None, jab_o, map_o, counts, **kw)
    elif what == "counts_null":
        rc = raw(v, br, keep, add, nz_o, jab_o, map_o, None, **kw)
    elif what == "bad_range":
        rc = raw(v, (9, 3), None, [], nz_o, jab_o, map_o, counts)
    else:
        rc = raw(v, br, keep, add, nz_o, jab_o, map_o, counts, jab=jab, **kw)
    assert rc == _lib.ERR_INVALID, (what, rc)
    assert all(np.all(o == -7) for o in outs), what
    # the restatement refuses what it can express
    if what in ("unsorted", "add_outside_range", "add_row_negative", "add_col_too_large", "add_col_negative", "add_twice", "add_stored_kept", "add_stored_dead"):
        with pytest.raises(R.Invalid):
            R.rule(v.cols, v.block_rows, int(v.block_col_size), v.row_part, v.nzcount, v.jab if jab is None else jab, b0, b1, keep, add)
    # ... and the same call without the fault is taken
    assert raw(v, br, keep, [(row, free)], nz_o, jab_o, map_o, counts) == _lib.OK


def test_a_dead_stored_block_comes_back_through_keep():
    v = geometry("dense")
    new, bmap = v.repattern(keep=np.array([1, 0, 1, 1], np.uint8))
    assert list(bmap) == [0, 2, 3] and list(new.nzcount) == [1, 2]
    with pytest.raises(sa.SpartaError):
        v.repattern(keep=np.array([1, 0, 1, 1], np.uint8), add=[(0, 1)])
    again, bmap2 = new.repattern(add=[(0, 1)])
    assert list(bmap2) == [0, -1, 1, 2] and np.array_equal(again.jab, v.jab)
    assert not again.mab[48 * 64:2 * 48 * 64].any() and np.array_equal(again.mab[:48 * 64], v.mab[:48 * 64])
