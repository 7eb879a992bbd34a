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
