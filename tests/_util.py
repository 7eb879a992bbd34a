"""shared helpers for the tests: golden fixtures, seeded matrices, tolerance bound"""
import ast
import hashlib
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def load(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


_mats = None


def matrices():
    """the seeded matrices of tests/golden/make_golden.py (regenerated, then checked against the stored checksums)"""
    global _mats
    if _mats is None:
        import sparta_amd as sa
        from golden.make_golden import unsorted_rows
        _mats = {
            "unsorted": unsorted_rows(),
            "u256": sa.gen.uniform_random(256, 256, 2000, seed=11),
            "band1k": sa.gen.banded(1000, 12, 0.6, seed=12),
            "rmat2k": sa.gen.rmat(11, 30000, seed=13, pattern_only=True),
            "rect": sa.gen.uniform_random(300, 517, 6000, seed=14),
            "fem": sa.gen.fem3d(4, 4, 9, 3, seed=15),
            "c1": sa.gen.config1(),
        }
        cases = load("cases.npz")
        for k, m in _mats.items():
            want = str(cases["%s/csr_sha" % k])
            got = sha(m.rowptr) + sha(m.colidx) + (sha(m.vals) if m.vals is not None else "")
            assert got == want, "seeded generator drifted for %s: golden fixtures no longer match their inputs" % k
    return _mats


TRAIN_ROWS, TRAIN_COLS = 500, 1102          # 1102 % w != 0 for every w below (a ragged last block column); both even (vbs_linear on 16-bit handles)
TRAIN_F32 = ("w3", "w13h1", "w48", "w100h200", "w128", "w128h20", "w128h80", "w200", "w13z")
TRAIN_H16 = ("w96", "w128", "w256")             # 16-bit handles need w % 32 == 0
_train = None


def train_geometries():
    """key -> VBR: one seeded 500 x 1102 matrix (~25 nonzeros per row; rows 32..63 and three scattered rows hold nothing) under the block widths and groupings
    of tests/test_train_geometry_gpu.py.  Shared by that file and the host-side walks of tests/test_spmm_t_host.py.
      w3        rows // 16       the reference's default -b; 32 % 3 != 0; block-rows 2 and 3 have no block
      w13h1     one row each     h = 1; the empty rows are block-rows without a block
      w48       rows // 16       panels of 32 + 16 stored columns
      w100h200  rows // 200      h = 200, 200, 100; panels 32 + 32 + 32 + 4
      w128      rows // 100      h = 100 (h % 8 = 4): tiles of 64 + 36 rows; four panels, four 32-deep steps per block (also a 16-bit geometry)
      w128h20   rows // 20       fp32: every tile <= 32 rows, so the handle has the fragment image (four slices per block), which then holds every element
      w128h80   rows // 80       fp32: tiles of 64 + 16 rows: the fragment image holds a part of the matrix only
      w200      Jaccard, tau 0.9 ragged heights (about 266, 133, 66) with a wide block, on the matrix thinned to three clusters of block columns (below)
      w13z      partition        16-row block-rows from a row partition with two repeated entries: two block-rows of height 0 in the middle
      w96       rows // 20       16-bit: h % 8 = 4, w = 64 + 32; block-row 2 (rows 40..59) has no block
      w256      rows // 40       16-bit: 33..64-row tiles, wide block"""
    global _train
    if _train is None:
        import sparta_amd as sa
        m0 = sa.gen.uniform_random(TRAIN_ROWS, TRAIN_COLS, 13000, seed=20261018)
        keep = np.ones(TRAIN_ROWS, bool)
        keep[32:64] = False
        keep[[100, 257, 499]] = False
        counts = np.diff(m0.rowptr) * keep
        sel = np.repeat(keep, np.diff(m0.rowptr))
        m = sa.CSR(TRAIN_ROWS, TRAIN_COLS, np.concatenate([[0], np.cumsum(counts)]), m0.colidx[sel], m0.vals[sel])
        rows = np.arange(TRAIN_ROWS, dtype=np.int64)

        def vbr(g, w):
            return sa.VBR().fill_from_CSR_inplace(m, g, w)

        # w200: at ~25 nonzeros per row every row meets all six 200-wide block columns and the Jaccard grouping would make ONE block-row.  Row i keeps the
        # nonzeros of the block columns of its cluster (i % 7 -> three disjoint clusters of 4 : 2 : 1 rows: rows of different clusters share no block column), so the grouping finds three block-rows of
        # different heights next to the one of the empty rows
        bcs = [(0, 1), (0, 1), (0, 1), (0, 1), (2, 3), (2, 3), (4, 5)]
        ri = np.repeat(rows, np.diff(m.rowptr))
        sel = np.array([c // 200 in bcs[r % 7] for r, c in zip(ri, m.colidx)], bool)
        mc = sa.CSR(TRAIN_ROWS, TRAIN_COLS, np.concatenate([[0], np.cumsum(np.bincount(ri[sel], minlength=TRAIN_ROWS))]), m.colidx[sel], m.vals[sel])
        part = np.concatenate([np.arange(0, 240, 16), [240, 240], np.arange(240, TRAIN_ROWS, 16), [TRAIN_ROWS]]).astype(np.int64)
        _train = {
            "w3": vbr(rows // 16, 3), "w13h1": vbr(rows, 13), "w48": vbr(rows // 16, 48), "w100h200": vbr(rows // 200, 100), "w128": vbr(rows // 100, 128),
            "w128h20": vbr(rows // 20, 128), "w128h80": vbr(rows // 80, 128),
            "w200": sa.VBR().fill_from_CSR_inplace(mc, sa.BlockingEngine(tau=0.9, col_block_size=200).GetGrouping(mc), 200),
            "w13z": sa.VBR().fill_from_CSR(m, part, 13),
            "w96": vbr(rows // 20, 96), "w256": vbr(rows // 40, 256),
        }
        for k, v in _train.items():
            assert v.rows == TRAIN_ROWS and v.cols == TRAIN_COLS and v.cols % v.block_col_size != 0, k
    return _train


def case_list():
    cases = load("cases.npz")
    out = []
    for key, name, cfg in cases["index"]:
        out.append((str(key), str(name), dict(ast.literal_eval(str(cfg)))))
    return out


def case_fields(key):
    cases = load("cases.npz")
    pre = key + "/"
    return {k[len(pre):]: cases[k] for k in cases.files if k.startswith(pre)}


def abs_bound(rows, cols, w, row_part, nzcount, jab, mab, B, n):
    """sum_k |a||b| per element of C (oracle arithmetic): the scale of the fp32 tolerance 1e-5 * sum|a||b|"""
    from oracle import oracle as O
    return O.vbr_multiply(rows, cols, w, row_part, nzcount, jab, np.abs(mab), np.abs(B), n)


# ---- edge geometries: tiny VBS matrices written out as arrays, shapes a builder-made test matrix never has ------------------------------------------------
EDGE_F32 = ("one", "rowvec", "colvec", "narrow32", "empty", "corner", "zeros", "tall", "heights", "dense", "w1", "corner64", "heights64")
EDGE_H16 = ("rowvec", "narrow32", "empty", "corner", "zeros", "tall", "dense", "heights32", "tall64")          # 16-bit handles need w % 32 == 0
EDGE_HEIGHTS = (0, 1, 0, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 0, 52, 0)
_edge = {}


def _edge_arrays(rows, cols, w, heights, present):
    """(rows, cols, w, row_part, nzcount, jab) from the heights of the block-rows and, per block-row, the ascending list of its block columns"""
    heights = [int(h) for h in heights]
    assert sum(heights) == rows and len(present) == len(heights)
    row_part = np.concatenate([[0], np.cumsum(heights)]).astype(np.int64)
    nzcount = np.array([len(p) for p in present], np.int64)
    jab = np.array([j for p in present for j in p], np.int64)
    return rows, cols, w, row_part, nzcount, jab


def edge_blocks(v, br=None):
    """(offset into mab, first row, h, first column, stored columns inside the matrix) of every stored block of the block-rows br = (b0, b1); offsets and rows
    count from the start of the range, as a range handle sees them"""
    b0, b1 = (0, v.block_rows) if br is None else br
    w = int(v.block_col_size)
    out, mo, jo = [], 0, int(np.sum(v.nzcount[:b0]))
    for ib in range(b0, b1):
        h = int(v.row_part[ib + 1] - v.row_part[ib])
        for b in range(int(v.nzcount[ib])):
            c0 = int(v.jab[jo + b]) * w
            out.append((mo, int(v.row_part[ib] - v.row_part[b0]), h, c0, min(w, v.cols - c0)))
            mo += h * w
        jo += int(v.nzcount[ib])
    return out


def edge_mab_slice(v, br):
    """(lo, hi): the elements of v.mab that belong to the block-rows br"""
    hts = np.diff(v.row_part) * v.nzcount * int(v.block_col_size)
    return int(hts[:br[0]].sum()), int(hts[:br[1]].sum())


def _edge_values(arr, kind, seed, zero_blocks=()):
    """seeded values in the mab layout: 'int' -3..3 without a zero, 'real' uniform(-1, 1).  The positions of a ragged last block column past cols hold seeded
    NON-ZERO values as well (a builder stores 0 there; a caller of the C-ABI need not): they lie outside the matrix and must take no part in any product, so a
    kernel that reads rows of B at or past cols meets a non-zero factor.  The stored blocks listed in zero_blocks hold 0.0 everywhere."""
    rows, cols, w, row_part, nzcount, jab = arr
    v = sa_vbr(arr, np.zeros(int((np.diff(row_part) * nzcount).sum()) * w, np.float32))
    rng = np.random.default_rng(seed)
    if kind == "int":
        x = rng.integers(-3, 4, v.nztot).astype(np.float32)
        x[x == 0] = 2.0
    else:
        x = rng.uniform(-1, 1, v.nztot).astype(np.float32)
        x[x == 0] = 0.5
    for q, (off, _, h, _, _) in enumerate(edge_blocks(v)):
        if q in zero_blocks:
            x[off:off + w * h] = 0.0
    return x


def sa_vbr(arr, mab):
    import sparta_amd as sa
    rows, cols, w, row_part, nzcount, jab = arr
    return sa.VBR.from_arrays(rows, cols, w, row_part, nzcount, jab, mab)


def edge_geometries(values="int"):
    """key -> VBR made with VBR.from_arrays from index arrays written out here (no builder involved), with seeded values (_edge_values: the stored positions past cols are non-zero too): values = 'int' (-3 .. 3, no zero
    inside a stored block unless the geometry says so: every order of additions gives the same bits) or 'real' (uniform(-1, 1)).  Shared by
    tests/test_edge_geometry_gpu.py and the CPU checks of tests/test_edge_geometry_host.py.  rows x cols, w, and what each one is for:
      one        1 x 1, w 1       one 1 x 1 block: every tile, panel and slab is almost all padding
      rowvec     1 x 300, w 32    one block-row of height 1 holding all 10 block columns, the last one ragged (12 real columns)
      colvec     300 x 1, w 3     cols < w; heights 7 with a ragged last block-row of 6; every third block-row without a block
      narrow32   100 x 20, w 32   cols < w at an MFMA panel width (the only block column is the ragged one); heights 25
      empty      130 x 200, w 32  16-row block-rows (last one 2), nzcount all 0, nztot 0, jab and mab empty: every work list of the handle is empty
      corner     130 x 200, w 32  as empty, with ONE block in the last (2-row) block-row, in the last (ragged, 8-column) block column
      zeros      96 x 160, w 32   heights 24; blocks at about half the positions; every value of every second stored block is 0.0
      tall       322 x 96, w 32   two block-rows, heights 257 and 65 (more than four 64-row tiles), each holding all three block columns
      heights    391 x 112, w 16  heights EDGE_HEIGHTS: zero heights first, in the middle and last; about half the blocks present; the block-rows of
                                  height 1 and 64 hold no block
      dense      96 x 128, w 64   heights 48; every block present, every value non-zero
      w1         70 x 70, w 1     heights 1, 5, 64; about 10 % of the 1-wide blocks present
      corner64   130 x 200, w 64  corner at the width of the per-class kernels (w % 64 == 0): eight block-rows without a block next to one block, which is ragged
      heights64  391 x 112, w 64  fp32: the height list of heights at the width of the per-class kernels; the second block column is ragged (48 real columns)
      heights32  391 x 112, w 32  16-bit: the height list of heights; the last block column is ragged (16 real columns)
      tall64     322 x 192, w 64  16-bit: tall at w 64: 64-row tiles of 64-wide blocks (pair / hub plan candidates)"""
    if values not in _edge:
        seed0 = {"int": 7100, "real": 7200}[values]
        rng = np.random.default_rng(20261018)                     # the patterns: the same for both value sets

        def half(n_brows, n_bcols, empty=()):
            out = []
            for ib in range(n_brows):
                p = [j for j in range(n_bcols) if rng.random() < 0.5] or [int(rng.integers(n_bcols))]
                out.append([] if ib in empty else p)
            return out

        hts = list(EDGE_HEIGHTS)
        no_block = [i for i, h in enumerate(hts) if h in (0, 1, 64)]
        h16_pat, h32_pat = half(16, 7, no_block), half(16, 4, no_block)
        zeros_pat = half(4, 5)
        w1_pat = [sorted(rng.choice(70, 7, replace=False).tolist()) for _ in range(3)]
        arrs = {
            "one": _edge_arrays(1, 1, 1, [1], [[0]]),
            "rowvec": _edge_arrays(1, 300, 32, [1], [list(range(10))]),
            "colvec": _edge_arrays(300, 1, 3, [7] * 42 + [6], [[] if ib % 3 == 2 else [0] for ib in range(43)]),
            "narrow32": _edge_arrays(100, 20, 32, [25] * 4, [[0]] * 4),
            "empty": _edge_arrays(130, 200, 32, [16] * 8 + [2], [[]] * 9),
            "corner": _edge_arrays(130, 200, 32, [16] * 8 + [2], [[]] * 8 + [[6]]),
            "zeros": _edge_arrays(96, 160, 32, [24] * 4, zeros_pat),
            "tall": _edge_arrays(322, 96, 32, [257, 65], [[0, 1, 2]] * 2),
            "heights": _edge_arrays(391, 112, 16, hts, h16_pat),
            "dense": _edge_arrays(96, 128, 64, [48, 48], [[0, 1]] * 2),
            "w1": _edge_arrays(70, 70, 1, [1, 5, 64], w1_pat),
            "heights32": _edge_arrays(391, 112, 32, hts, h32_pat),
            "tall64": _edge_arrays(322, 192, 64, [257, 65], [[0, 1, 2]] * 2),
            "corner64": _edge_arrays(130, 200, 64, [16] * 8 + [2], [[]] * 8 + [[3]]),
            "heights64": _edge_arrays(391, 112, 64, hts, half(16, 2, no_block)),
        }
        out = {}
        for i, (k, a) in enumerate(arrs.items()):
            n_blocks = int(a[4].sum())
            out[k] = sa_vbr(a, _edge_values(a, values, seed0 + i, zero_blocks=range(0, n_blocks, 2) if k == "zeros" else ()))
        _edge[values] = out
    return _edge[values]


def edge_round(x, dtype):
    """x as the storage type of a handle holds it, in float64: dtype 0 fp32, 1 fp16, 2 bf16 (round to nearest even), by numpy alone"""
    f = np.ascontiguousarray(x, np.float32)
    if dtype == 1:
        with np.errstate(over="ignore"):
            return f.astype(np.float16).astype(np.float64)
    if dtype == 2:
        u = f.view(np.uint32).astype(np.uint64)
        u = ((u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000).astype(np.uint32)
        with np.errstate(invalid="ignore"):
            out = u.view(np.float32).astype(np.float64).reshape(f.shape)
        out[np.isnan(f)] = np.nan          # (the carry of the rounding would take a NaN with only low mantissa bits set to Inf: a NaN stays a NaN)
        return out
    return f.astype(np.float64)


def edge_dense(v, dtype=0, mab=None, br=None):
    """the float64 (rows of the block-rows br) x cols matrix of the stored blocks, expanded from the arrays: element i of stored column q of a block is
    mab[off + q * h + i] (mab: the whole matrix's values or the range's); the positions of a ragged last block column past cols are dropped; values rounded to the handle's storage type first"""
    mab = edge_round(v.mab if mab is None else mab, dtype)
    b0, b1 = (0, v.block_rows) if br is None else br
    if len(mab) == len(v.mab):                                       # the whole matrix's values: take the range's
        mab = mab[slice(*edge_mab_slice(v, (b0, b1)))]
    D = np.zeros((int(v.row_part[b1] - v.row_part[b0]), v.cols))
    for off, r0, h, c0, valid in edge_blocks(v, br):
        D[r0:r0 + h, c0:c0 + valid] = mab[off:off + valid * h].reshape(valid, h).T
    return D


def edge_sample(v, M, br=None):
    """the rows x cols matrix M sampled back into the mab layout of the block-rows br (include/sparta_amd.h: G[off + q * h + i] = M[r0 + i, jb * w + q]);
    the positions past cols are 0"""
    w = int(v.block_col_size)
    blocks = edge_blocks(v, br)
    G = np.zeros(sum(h * w for _, _, h, _, _ in blocks))
    for off, r0, h, c0, valid in blocks:
        G[off:off + valid * h] = M[r0:r0 + h, c0:c0 + valid].T.reshape(-1)
    return G


def spmm_t_host_check(v, x, br=None):
    """y = A^T x by the host walk of the block-column index that sparta_vbs_create builds for sparta_vbs_spmm_t (sparta_spmm_t_host_check): (y, info)"""
    import ctypes as C
    from sparta_amd import _lib
    i64p, f32p = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    b0, b1 = (0, v.block_rows) if br is None else br
    rp, nz, jab = (np.ascontiguousarray(a, np.int64) for a in (v.row_part, v.nzcount, v.jab))
    mab, x = np.ascontiguousarray(v.mab, np.float32), np.ascontiguousarray(x, np.float32)
    y, info = np.full(v.cols, np.nan, np.float64), np.full(8, -1, np.int64)
    _lib.check(_lib.lib.sparta_spmm_t_host_check(v.rows, v.cols, v.block_rows, v.block_col_size, rp.ctypes.data_as(i64p), nz.ctypes.data_as(i64p), jab.ctypes.data_as(i64p),
                                                 mab.ctypes.data_as(f32p), b0, b1, x.ctypes.data_as(f32p), y.ctypes.data_as(C.POINTER(C.c_double)), info.ctypes.data_as(i64p)))
    return y, info


# ---- poison geometries: which operands does an output element depend on? ------------------------------------------------------------------------------------
POISON_F32 = ("P32", "P64", "P13")
POISON_H16 = ("P32", "P64")                         # 16-bit handles need w % 32 == 0
POISON_HEIGHTS = {"P32": [32, 32, 32, 20, 32, 32, 64, 7], "P64": [48, 48, 64, 33, 64, 64, 40, 64], "P13": [16, 5, 32, 1, 19, 64, 16, 33]}
POISON_COLS = {"P32": 8 * 32 - 11, "P64": 8 * 64 - 20, "P13": 8 * 13 - 4}
POISON_W = {"P32": 32, "P64": 64, "P13": 13}
PCSR_THIN = (3, 15)                                 # the block columns (w 32) that every third block-row of PCSR, PUNI and PSPLIT does not store
POISON_GATHERED = {"P32G": "P32", "P64G": "P64"}    # the siblings of P32 / P64 for a gathered B, which has cols = n_shards * shard_rows: the same blocks, cols = 8 w
_poison = None


def poison_present(ib):
    """the block columns block-row ib of P32 / P64 / P13 stores: all of 0..7 except ib and (ib + 3) % 8 -- no two block-rows store the same set"""
    return [j for j in range(8) if j not in (ib, (ib + 3) % 8)]


def poison_csr():
    """PCSR: (CSR 512 x 512, grouping rows // 16, w 32).  Per row: with probability 0.85 each one nonzero in block column 3 and one in block column 15 (the
    columns the poison goes to: a row that stores such a block column then usually has a nonzero in it, which keeps the `open` elements of the reference few),
    four more anywhere, every 37th row 40 more (rows long enough for the window plan); then every nonzero of block columns 3 and 15 is removed from every third
    block-row (ib % 3 == 1).  Values: seeded uniform(-1, 1), none 0."""
    import sparta_amd as sa
    rng = np.random.default_rng(20261019)
    rows = cols = 512
    rr, cc = [], []
    for i in range(rows):
        c = [rng.integers(0, cols, 4 + (40 if i % 37 == 5 else 0))]
        for bc in PCSR_THIN:
            if rng.random() < 0.85:
                c.append(bc * 32 + rng.integers(0, 32, 1))
        c = np.unique(np.concatenate(c))
        if (i // 16) % 3 == 1:
            c = c[~np.isin(c // 32, PCSR_THIN)]
        rr.append(np.full(len(c), i)); cc.append(c)
    r, c = np.concatenate(rr), np.concatenate(cc)
    vals = rng.uniform(-1, 1, len(c)).astype(np.float32)
    vals[vals == 0] = 0.5
    m = sa.CSR(rows, cols, np.concatenate([[0], np.cumsum(np.bincount(r, minlength=rows))]).astype(np.int64), c.astype(np.int32), vals)
    return m, np.arange(rows, dtype=np.int64) // 16, 32


def _thin(rows_of_groups, r, c, w):
    """drop every nonzero (r, c) of the block columns PCSR_THIN from every third group (index % 3 == 1); rows_of_groups: per group, its rows"""
    drop = np.zeros(len(r), bool)
    for gi, rows in enumerate(rows_of_groups):
        if gi % 3 == 1:
            drop |= np.isin(r, rows) & np.isin(c // w, PCSR_THIN)
    return r[~drop], c[~drop]


def _csr_of(rows, cols, r, c, seed):
    """the CSR of the positions (r, c) with seeded non-zero uniform(-1, 1) values"""
    import sparta_amd as sa
    o = np.lexsort((c, r))
    r, c = r[o], c[o]
    vals = np.random.default_rng(seed).uniform(-1, 1, len(c)).astype(np.float32)
    vals[vals == 0] = 0.5
    return sa.CSR(rows, cols, np.concatenate([[0], np.cumsum(np.bincount(r, minlength=rows))]).astype(np.int64), c.astype(np.int32), vals)


PUNI_SHAPE = (9, 48, 1024, 100, 3)                  # clustered(n_groups, rows_per, cols, shared, own): 432 x 1024, 32 block columns of width 32


def poison_union():
    """PUNI: (CSR, grouping, w 32) from the clustered generator of tests/test_union_host.py (the one tests/test_union_gpu.py uses) at a size that still gives one
    column-compacted tile per cluster: rows of a cluster (scattered over the matrix) share ~80 of 100 columns, about three per block column, so a row of a
    cluster that stores a block column nearly always has a nonzero in it; then every nonzero of the block columns PCSR_THIN is removed from every third cluster (every third block-row of the handle)."""
    from test_union_host import clustered, true_grouping
    ng, rp, cols, shared, own = PUNI_SHAPE
    m, order = clustered(ng, rp, cols, shared, own, seed=20261021)
    r = np.repeat(np.arange(m.rows), np.diff(m.rowptr))
    groups = sorted((order[gi * rp:(gi + 1) * rp] for gi in range(ng)), key=lambda rows: rows.min())          # in the order of the handle's block-rows (group id = smallest row)
    r, c = _thin(groups, r, np.asarray(m.colidx, np.int64), 32)
    return _csr_of(m.rows, cols, r, c, 20261022), true_grouping(order, rp), 32


def poison_split():
    """PSPLIT: (CSR 256 x 512, grouping rows // 32, w 32) whose block-rows sparta_vbs_create_from_csr splits into tiles and sparse rows: per row 20 of the 32
    columns of each of the block columns 3, 9 and 15 (well-filled blocks: tiles) and two nonzeros anywhere else (thin blocks: sparse rows that add); then
    every nonzero of the block columns PCSR_THIN is removed from every third block-row, which keeps its tile of block column 9 -- a 16-bit pair tile of such a
    block-row and its neighbour has an absent half in the block columns the poison goes to."""
    rng = np.random.default_rng(20261023)
    rows, cols, w = 256, 512, 32
    rr, cc = [], []
    for i in range(rows):
        c = np.unique(np.concatenate([bc * w + rng.choice(w, 20, replace=False) for bc in (3, 9, 15)] + [rng.integers(0, cols, 2)]))
        rr.append(np.full(len(c), i)); cc.append(c)
    r, c = _thin([np.arange(32 * gi, 32 * gi + 32) for gi in range(rows // 32)], np.concatenate(rr), np.concatenate(cc), w)
    return _csr_of(rows, cols, r, c, 20261024), np.arange(rows, dtype=np.int64) // 32, w


def poison_geometries():
    """key -> VBR made with VBR.from_arrays from index arrays written out here: 8 block-rows x 8 block columns, block-row ib stores poison_present(ib); every
    stored value is a seeded non-zero uniform(-1, 1) (the positions past cols too: they take no part in any product).  Shared by tests/test_poison_gpu.py and
    tests/test_poison_host.py.
      P32   w 32, heights 32 32 32 20 32 32 64 7 (16-bit: the pair plan takes (0, 1), (2, 3), (4, 5)), cols 8 * 32 - 11
      P64   w 64, heights 48 48 64 33 64 64 40 64 (16-bit: candidates of the hub plan), cols 8 * 64 - 20
      P13   w 13, heights 16 5 32 1 19 64 16 33, cols 8 * 13 - 4 (fp32 only)
      P32G, P64G   the blocks of P32 / P64 with cols = 8 w: a gathered B is n_shards slabs of cols / n_shards rows, which a ragged cols does not allow"""
    global _poison
    if _poison is None:
        _poison = {}
        for i, k in enumerate(POISON_F32):
            hts = POISON_HEIGHTS[k]
            a = _edge_arrays(sum(hts), POISON_COLS[k], POISON_W[k], hts, [poison_present(ib) for ib in range(8)])
            _poison[k] = sa_vbr(a, _edge_values(a, "real", 7300 + i))
        for i, (k, of) in enumerate(POISON_GATHERED.items()):
            hts = POISON_HEIGHTS[of]
            a = _edge_arrays(sum(hts), 8 * POISON_W[of], POISON_W[of], hts, [poison_present(ib) for ib in range(8)])
            _poison[k] = sa_vbr(a, _edge_values(a, "real", 7310 + i))
    return _poison


def stored_mask(v, br=None):
    """bool (rows of the block-rows br) x cols: the positions inside a stored block"""
    return edge_dense(v, mab=np.ones(len(v.mab), np.float32), br=br) != 0


def csr_dense_and_stored(m, g, w):
    """(D float64 rows x cols, stored bool) of a CSR under grouping g (groups ascending with the rows) on the w-grid, rows in the order of the handle that
    sparta_vbs_create_from_csr makes (the grouping's permutation): a block column is stored by a block-row (a group) when one of the group's rows has a nonzero in it"""
    D = np.zeros((m.rows, m.cols))
    r = np.repeat(np.arange(m.rows), np.diff(m.rowptr))
    D[r, m.colidx] = m.vals
    nbc = (m.cols + w - 1) // w
    has = np.zeros((int(g.max()) + 1, nbc), bool)
    has[g[r], m.colidx // w] = True
    stored = np.repeat(has[g], w, axis=1)[:, :m.cols]
    import sparta_amd as sa
    perm = np.asarray(sa.get_permutation(g), np.int64)          # row r of the handle (and of C) is row perm[r] of the CSR: the rows of a group together, groups by their id
    assert (np.diff(g[perm]) >= 0).all()
    return D[perm], stored[perm]


def poison_reference(D, stored, B):
    """float64 reference of D @ B under the dependency contract of include/sparta_amd.h, for a B that holds non-finite elements (the poison).  D: dense
    r x c (already rounded to the handle's storage type), stored: bool r x c, the positions inside stored blocks, B: c x n float64.  Row i of the product is
    D[i, stored[i]] @ B[stored[i]] (computed for all rows of one stored pattern at once): the rows of B outside the block columns that the row's block-row stores are not read (a dense D @ B would multiply them by
    0).  Returns (product, clean, dirty, open): clean -- no poisoned element of B lies in a stored block column of the row, in this column of B: the element
    must equal the unpoisoned product; dirty -- a non-zero of D meets a poisoned element: must be non-finite; open -- only stored zeros of A meet poison."""
    bad = ~np.isfinite(B)
    want = np.zeros((D.shape[0], B.shape[1]))
    with np.errstate(all="ignore"):
        pats, which = np.unique(stored, axis=0, return_inverse=True)            # rows of one block-row share their pattern: one product per pattern
        for q, s in enumerate(pats):
            rows = np.flatnonzero(which.reshape(-1) == q)
            want[rows] = D[np.ix_(rows, np.flatnonzero(s))] @ B[s]
    may = (stored.astype(np.float64) @ bad.astype(np.float64)) > 0
    dirty = ((D != 0).astype(np.float64) @ bad.astype(np.float64)) > 0
    assert not (dirty & ~may).any()
    return want, ~may, dirty, may & ~dirty


def poison_reference_t(D, stored, X):
    """the same for Ct = A^T X (sparta_vbs_spmm_t): row c of Ct reads the rows of X of the block-rows that store the block column of c"""
    return poison_reference(np.ascontiguousarray(D.T), np.ascontiguousarray(stored.T), X)


def poison_reference_sddmm(v, X, Y, br=None):
    """G = (X Y^T) sampled on the stored blocks, in the mab layout, float64: (G, clean, dirty).  G[i, c] reads row i of X and row c of Y and nothing else, so
    an element is dirty when one of the two rows holds poison (whatever the other row holds: a * Inf and 0 * Inf are both non-finite) and clean otherwise;
    the positions past cols are 0 and clean."""
    with np.errstate(all="ignore"):
        M = X @ Y.T
    bad = np.logical_or.outer(~np.isfinite(X).all(axis=1), ~np.isfinite(Y).all(axis=1))
    G = edge_sample(v, np.where(bad, 0.0, M), br)
    dirty = edge_sample(v, bad.astype(np.float64), br) != 0
    G[dirty] = edge_sample(v, np.where(bad, M, 0.0), br)[dirty]
    return G, ~dirty, dirty


POISON_VALUES = {"+inf": (np.inf,), "-inf": (-np.inf,), "nan": (np.nan,), "mix": (np.inf, np.nan, -np.inf), "1e5": (1.0e5,)}          # 1e5: finite in fp32 and bf16, Inf once rounded to fp16


def poisoned(M, rows, kind, col=None):
    """a copy of M (float64) with the poison `kind` in the rows `rows` (a slice or an index array): in every column, or in column `col` alone; 'mix' gives
    consecutive rows +Inf, NaN, -Inf in turn; '1e5' is stored as Inf (what the conversion to fp16 makes of it: the caller hands the device 1e5)"""
    M = M.copy()
    idx = np.arange(M.shape[0])[rows]
    vals = np.array([np.inf if x == 1.0e5 else x for x in POISON_VALUES[kind]])
    fill = vals[np.arange(len(idx)) % len(vals)]
    if col is None:
        M[idx, :] = fill[:, None]
    else:
        M[idx, col] = fill
    return M


def block_col_rows(v, c):
    """the rows of B (columns of A) of block column c, inside the matrix"""
    w = int(v.block_col_size)
    return slice(c * w, min((c + 1) * w, v.cols))


def block_row_rows(v, r, br=None):
    """the rows of block-row r, counted from the start of the range br"""
    b0 = 0 if br is None else br[0]
    return slice(int(v.row_part[r] - v.row_part[b0]), int(v.row_part[r + 1] - v.row_part[b0]))


POISON_B_PLACEMENTS = [(c, j) for c in (1, 7) for j in (None, 0, 37, -1)]          # (block column c*, column j* of B: None = all of them, -1 = the last)


# ---- accuracy inputs: is the arithmetic still fp32? -----------------------------------------------------------------------------------------------------------
ACC_Q = (1, 2, 3, 4, 8, None)                       # non-zeros row i of a block-row keeps (i % 6); None = all of its stored positions
ACC_EXP = {0: 12, 1: 8, 2: 12}                      # kind "wide": exponents -E .. E per storage type (f16: products up to 2^18 and sums of them stay far inside fp32, the operands inside fp16's normal range)
U32 = 2.0 ** -24                                    # the unit roundoff of fp32


def accuracy_draw(rng, size, kind, dtype):
    """float64 full-mantissa values m * 2^e, m uniform in [1, 2), random sign; kind 'wide': e uniform in -E..E (ACC_EXP), 'unit': e = 0; rounded to the storage
    type with edge_round (every value is then exactly what the device holds)"""
    m = rng.uniform(1.0, 2.0, size)
    e = rng.integers(-ACC_EXP[dtype], ACC_EXP[dtype] + 1, size) if kind == "wide" else np.zeros(size, np.int64)
    s = np.where(rng.random(size) < 0.5, -1.0, 1.0)
    assert kind in ("wide", "unit")
    return edge_round(s * m * 2.0 ** e, dtype).reshape(np.shape(m))


def accuracy_values(v, kind, dtype, seed, dense=False):
    """a mab (float32, already rounded to the storage type `dtype`) for the geometry v, index arrays unchanged: row i of each block-row keeps ACC_Q[i % 6]
    non-zeros among its stored positions inside cols (seeded choice), each an accuracy_draw value; everything else -- the other stored positions and the
    positions past cols -- is 0.0.  dense: every row keeps all of them (the A of spmm_ba: sparta_vbs_create_transposed drops exact zeros, and blocks that
    are nearly all zeros become sparse rows; the short sums then come from the other operand, accuracy_dense(few_rows_from=...))"""
    rng = np.random.default_rng(seed)
    w = int(v.block_col_size)
    mab = np.zeros(len(v.mab), np.float64)
    blocks = edge_blocks(v)
    for ib in range(v.block_rows):
        r0, h = int(v.row_part[ib]), int(v.row_part[ib + 1] - v.row_part[ib])
        mine = [(off, valid) for off, br0, bh, _, valid in blocks if br0 == r0 and bh == h and h > 0]
        if not mine or h == 0:
            continue
        pos = np.concatenate([off + np.arange(valid) * h for off, valid in mine])          # row 0's stored positions; row i: + i
        for i in range(h):
            q = None if dense else ACC_Q[i % len(ACC_Q)]
            sel = pos if q is None or q >= len(pos) else rng.choice(pos, q, replace=False)
            mab[sel + i] = accuracy_draw(rng, len(sel), kind, dtype)
    return mab.astype(np.float32)


def accuracy_csr(which, kind, dtype, seed):
    """(CSR, grouping, w) of PCSR / PCSR9 / PSPLIT / PUNI with the pattern unchanged and new values: row i keeps ACC_Q[i % 6] of its nonzeros as accuracy_draw values,
    the others are stored 0.0 (which the kernels skip or multiply: an exact zero adds no error either way)"""
    import sparta_amd as sa
    thin = which == "PCSR9"          # PCSR with ONE non-zero value in every ninth row and 0.0 everywhere else: 57 non-zeros on 512 columns, few enough (8 nnz < cols)
    #                                  for the sparse-row kernels to read a column-major B in place
    m, g, w = {"PCSR": poison_csr, "PCSR9": poison_csr, "PSPLIT": poison_split, "PUNI": poison_union}[which]()
    rng = np.random.default_rng(seed)
    vals = np.zeros(len(m.colidx), np.float64)
    for i in range(m.rows):
        lo, hi = int(m.rowptr[i]), int(m.rowptr[i + 1])
        q = ACC_Q[i % len(ACC_Q)]
        if thin:
            q = 1 if i % 9 == 0 else 0
        if hi > lo and q != 0:
            sel = np.arange(lo, hi) if q is None or q >= hi - lo else rng.choice(np.arange(lo, hi), q, replace=False)
            vals[sel] = accuracy_draw(rng, len(sel), kind, dtype)
    return sa.CSR(m.rows, m.cols, m.rowptr, m.colidx, vals.astype(np.float32)), g, w


def accuracy_dense(shape, kind, dtype, seed, k_sparse=False, few_rows_from=None):
    """a dense operand (float64, rounded to `dtype`) of accuracy_draw values.  k_sparse (the X / Y of sddmm, rows x k): row i is non-zero in only 1, 3 or all
    of the k columns (i % 3; the sets are nested and the same for every operand of one k, so a row of X meets a row of Y in min of the two counts).
    few_rows_from (the X of spmm_t / the B of spmm_ba, rows x n; an index array): column j keeps ACC_Q[j % 6] non-zero rows chosen among these rows."""
    rng = np.random.default_rng(seed)
    M = accuracy_draw(rng, shape, kind, dtype)
    if k_sparse:
        k = shape[1]
        order = np.random.default_rng(4242 + k).permutation(k)
        keep = np.zeros(shape, bool)
        for i in range(shape[0]):
            keep[i, order[:(1, 3, k)[i % 3]]] = True
        M = np.where(keep, M, 0.0)
    if few_rows_from is not None:
        keep = np.zeros(shape, bool)
        for j in range(shape[1]):
            q = ACC_Q[j % len(ACC_Q)]
            keep[few_rows_from if q is None or q >= len(few_rows_from) else rng.choice(few_rows_from, q, replace=False), j] = True
        M = np.where(keep, M, 0.0)
    return M


def gamma_terms(D, B, C0=None):
    """K of gamma_bound: per element of D @ B, the number of products of two non-zeros, plus 1 where C0 is given"""
    return (D != 0).astype(np.float64) @ (B != 0).astype(np.float64) + (0.0 if C0 is None else 1.0)


def gamma_bound(D, B, C0=None, factor=2.0):
    """per-element tolerance of an fp32 evaluation of D @ B (+ C0) against the exact product; D, B, C0 float64, already rounded for 16-bit handles.

        K   = (D != 0) @ (B != 0)  (+ 1 where C0 is given)          the number of fp32 terms the element really sums
        g_K = K u / (1 - K u),  u = 2^-24
        tol = min(1e-5, 2 g_K) * (|D| @ |B| + |C0|)

    Derivation (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1 and 4.2): each fp32 operation with round to nearest returns the exact result
    times (1 + d), |d| <= u.  In ANY summation tree of K products every product passes through at most K such factors: one for the rounding of the product (none
    when the multiply-add is fused, or when the product of two 16-bit values is exact) and at most K - 1 for the additions above it.  So the computed sum is
    sum a_k b_k (1 + t_k) with |t_k| <= (1 + u)^K - 1 <= g_K, whatever the order and whether fused or not: |computed - exact| <= g_K sum |a_k b_k|.  An exact zero
    operand gives the product 0 and x + 0 = x exactly, so it adds neither a term nor a rounding: K counts the non-zero products only (an accumulating call adds
    the previous C as one more term).  The factor 2 covers an adder that truncates instead of rounding to nearest (|d| <= 2 u).  The min keeps the bound at
    least as tight as the suite's 1e-5 * sum|a||b| for every K (2 g_K passes 1e-5 at K = 84).
    `factor` is 2 for every caller.  It may take another value only for the kernels of a matrix instruction whose own summation a stand-alone program has
    measured to be coarser than this model, and then that measured figure ("Parity bar"); nothing else may set it."""
    K = gamma_terms(D, B, C0)
    scale = np.abs(D) @ np.abs(B) + (0.0 if C0 is None else np.abs(C0))
    g = K * U32 / (1.0 - K * U32)
    return np.minimum(1e-5, factor * g) * scale


def fp32_eval(D, B, C0=None, order=None, product=None, store=np.float32, track=False):
    """sum over k in `order` (default ascending) of D[:, k] * B[k, :] with an unfused multiply and add in np.float32, starting from C0; the loop skips the k
    where a factor is all zero (x + 0 = x).  product(a, b): another arithmetic for the products (float64 in, float64 out: rounded to fp32 here); store: the
    type the partial sums are kept in.  Returns (sum as float64, smallest non-zero |partial sum or product|, largest) -- the last two only with track."""
    D32, B32 = D.astype(np.float32), B.astype(np.float32)
    acc = np.zeros((D.shape[0], B.shape[1]), store) if C0 is None else C0.astype(np.float32).astype(store)
    ks = np.flatnonzero((D != 0).any(axis=0) & (B != 0).any(axis=1))
    ks = ks if order is None else order(ks)
    lo, hi = np.inf, 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        for k in ks:
            p = D32[:, k, None] * B32[None, k, :] if product is None else product(D[:, k, None], B[None, k, :]).astype(np.float32)
            acc = (acc.astype(np.float32) + p).astype(store)
            for x in (p, acc) if track else ():
                a = np.abs(x[x != 0]).astype(np.float64)
                if a.size:
                    lo, hi = min(lo, float(a.min())), max(hi, float(a.max()))
    return acc.astype(np.float64), lo, hi


def _bf16_trunc(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32).astype(np.float64)


def weak_bf16_split(a, b):
    """the product of two fp32 values each split into three bf16 terms (hi + mid + lo = the value exactly: 3 x 8 bits), without the products of two low terms
    (mid x mid, mid x lo, lo x lo): a_hi * b + a_low * b_hi.  What is dropped is about 2^-16 of the product."""
    ah, bh = _bf16_trunc(a), _bf16_trunc(b)
    return ah * b + (a - ah) * bh


def weak_trunc10(a, b):
    """operands cut to 10 explicit mantissa bits (fp16's / TF32's) before an exact product"""
    cut = lambda x: (np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xffffe000)).view(np.float32).astype(np.float64)  # noqa: E731
    return cut(a) * cut(b)


# the input sets of tests/test_accuracy_gpu.py, by name; tests/test_accuracy_host.py proves the bound on each.  (op, source, dtype, kind, n or k)
ACC_SETS = (
    [("fwd", k, 0, "wide", n) for k in POISON_F32 for n in (128, 130)]
    + [("fwd", k, dt, "wide", n) for dt in (1, 2) for k, n in (("P32", 128), ("P64", 128), ("P64", 256))]
    + [("fwd", k, dt, "unit", 128) for k, dt in (("P32", 0), ("P64", 0), ("P13", 0), ("P32", 1), ("P64", 2), ("w128h20", 0), ("w128h80", 0), ("w256", 2))]
    + [("fwd", "P32G", 0, "wide", 128), ("fwd", "P64G", 2, "wide", 128)]
    + [("csr", "PCSR", 0, "wide", 40), ("csr", "PCSR", 0, "wide", 128), ("csr", "PCSR", 2, "wide", 128), ("csr", "PCSR", 0, "wide", 8),
       ("csr", "PSPLIT", 0, "wide", 128), ("csr", "PSPLIT", 2, "wide", 128), ("csr", "PUNI", 0, "wide", 128), ("csr", "PUNI", 2, "wide", 128)]
    + [("t", k, dt, kind, 128) for k, dt in (("P32", 0), ("P13", 0), ("P64", 1), ("P32", 2)) for kind in ("wide", "unit")]
    + [("ba", "P32", 0, "wide", 128)]
    + [("sddmm", k, dt, kind, kk) for k, dt in (("P32", 0), ("P13", 0), ("P64", 1), ("P32", 2)) for kk in (128, 37) for kind in (("wide", "unit") if kk == 128 else ("wide",))]
    + [("csr", "PCSR9", 0, "wide", 128), ("csr", "PCSR9", 2, "wide", 128)]          # (appended: the seed of a set follows its place in this list)
)
_acc = {}


def acc_id(s):
    return "%s-%s-%s-%s-%d" % (s[0], s[1], ("f32", "f16", "bf16")[s[2]], s[3], s[4])


def accuracy_set(s):
    """the operands of the input set s (one entry of ACC_SETS), cached and never changed: a dict with L, R (float64: the product under test is L @ R), C0 (the
    previous output of an accumulating call, fp32 values), check (bool: the elements of L @ R that the entry point writes) and what the op needs besides:
      fwd    v, mab: C = A B                      csr   m, g, w: the same on a handle made from a CSR (rows in the handle's order)
      t      v, mab: Ct = A^T X; L = A^T, R = X   ba    v, mab: C^T = A^T B^T on the transposed handle, the same operands
      sddmm  v, X, Y: L = X, R = Y^T, check = the stored positions inside cols"""
    if s in _acc:
        return _acc[s]
    op, key, dtype, kind, n = s
    seed = 20261100 + 7 * ACC_SETS.index(s)
    out = {}
    if op == "csr":
        m, g, w = accuracy_csr(key, kind, dtype, seed)
        D, _ = csr_dense_and_stored(m, g, w)
        out.update(m=m, g=g, w=w, L=D, R=accuracy_dense((m.cols, n), kind, dtype, seed + 1))
    else:
        v = (poison_geometries() if key.startswith("P") else train_geometries())[key]
        mab = accuracy_values(v, kind, dtype, seed, dense=op == "ba")
        D = edge_dense(v, dtype, mab=mab)
        out.update(v=v, mab=mab)
        if op == "fwd":
            out.update(L=D, R=accuracy_dense((v.cols, n), kind, dtype, seed + 1))
        elif op in ("t", "ba"):
            full = np.flatnonzero(((D != 0).sum(axis=1) == stored_mask(v).sum(axis=1)) & (D != 0).any(axis=1))          # the rows that kept all their positions
            out.update(L=np.ascontiguousarray(D.T), R=accuracy_dense((v.rows, n), kind, dtype, seed + 1, few_rows_from=full))
        else:
            X, Y = accuracy_dense((v.rows, n), kind, dtype, seed + 1, k_sparse=True), accuracy_dense((v.cols, n), kind, dtype, seed + 2, k_sparse=True)
            out.update(X=X, Y=Y, L=X, R=np.ascontiguousarray(Y.T), check=stored_mask(v))
    shape = (out["L"].shape[0], out["R"].shape[1])
    out.setdefault("check", np.ones(shape, bool))
    out["C0"] = accuracy_draw(np.random.default_rng(seed + 3), shape, kind, 0)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _acc[s] = out
    return out


def _bits(*u):
    return np.array(u, np.uint32).view(np.float32)


# fp32 inputs at the edges of the conversions to fp16 and bf16 (to_h16 at creation, the update and conversion kernels on the device); each also negated (ACC_SPECIALS)
_SPECIALS_POS = np.concatenate([
    np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8,          # ties to even in fp16 (down, up) and in bf16 (down, up)
              1 + 2.0 ** -11 + 2.0 ** -20, 1 + 2.0 ** -8 - 2.0 ** -20,                       # just above / just below a tie
              65504.0, 65519.99, 65520.0, 70000.0,                                           # fp16: the largest finite value; the last input that rounds to it; the first that rounds to Inf
              2.0 ** -14, 2.0 ** -14 - 2.0 ** -24, 2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), 2.0 ** -26, 1.5 * 2.0 ** -24,          # fp16: smallest normal, largest and smallest subnormal, ties and halves below them
              2.0 ** -126, 2.0 ** -133, 3 * 2.0 ** -133, 2.0 ** -134, 2.0 ** -134 * (1 + 2.0 ** -10), 2.0 ** -149, 2.0 ** -126 - 2.0 ** -133,          # bf16: smallest normal, subnormals (fp32 subnormals all), a tie to 0
              0.0, 1.0, np.inf], np.float64).astype(np.float32),
    _bits(0x7f7f0000, 0x7f7fffff, 0x7f7f8000, 0x7f7f7fff,          # bf16's largest finite value; fp32's (Inf in both 16-bit types); the tie that rounds to Inf in bf16; the last input that stays finite
          0x7f800001, 0x7f80ffff, 0x7fc00000, 0x7f801000),         # NaNs with only low mantissa bits set (a conversion that cuts the mantissa makes them Inf), the quiet NaN
])
ACC_SPECIALS = np.concatenate([_SPECIALS_POS, -_SPECIALS_POS])
