"""Block pruning without a GPU: the block table (sparta_vbs_block_table_host, the function the device table of a handle is built by) against the walks of
tests/_util.py on every edge geometry and block-row range, the exported entries and their refusals, and the selection rule sparta_amd.prune.select on
the CPU."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd import _lib
from sparta_amd._lib import lib

from _util import edge_geometries, edge_blocks, edge_mab_slice, train_geometries, _edge_arrays, sa_vbr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_i64p = C.POINTER(C.c_int64)


def _check_table(v, br=None):
    """VBR.block_table(br) against edge_blocks(v, br): offset, n_in = h * stored columns inside, n_all = h * w, (local block-row) << 32 | block column"""
    b0, b1 = (0, v.block_rows) if br is None else br
    w = int(v.block_col_size)
    T = v.block_table(br)
    blocks = edge_blocks(v, br)
    assert T.shape == (len(blocks), 4) and T.dtype == np.int64
    ib = np.repeat(np.arange(b0, b1), np.asarray(v.nzcount[b0:b1], np.int64))
    jo = int(np.sum(v.nzcount[:b0]))
    for q, (off, r0, h, c0, valid) in enumerate(blocks):
        assert int(v.row_part[ib[q]] - v.row_part[b0]) == r0
        assert tuple(T[q]) == (off, h * valid, h * w, ((int(ib[q]) - b0) << 32) | (c0 // w)), (q, T[q])
        assert c0 // w == int(v.jab[jo + q])
    return T


@pytest.mark.parametrize("key", sorted(edge_geometries()))
def test_block_table_equals_edge_blocks(key):
    v = edge_geometries()[key]
    T = _check_table(v)
    assert len(T) == len(v.jab)
    if len(T):
        assert int(T[-1, 0] + T[-1, 2]) == len(v.mab)                      # the blocks tile mab
    ranges = [(0, 1)] + ([(1, v.block_rows)] if v.block_rows > 1 else []) + ([(3, 9), (2, 3), (12, 16)] if key == "heights" else [])
    for br in ranges:
        R = _check_table(v, br)
        lo, hi = edge_mab_slice(v, br)
        q0 = int(np.sum(v.nzcount[:br[0]]))
        assert (R[:, 0] + lo == T[q0:q0 + len(R), 0]).all() and (R[:, 1:3] == T[q0:q0 + len(R), 1:3]).all()
        assert all(lo <= lo + o and lo + o + n <= hi for o, n in zip(R[:, 0], R[:, 2]))


def test_block_table_named_cases():
    e = edge_geometries()
    assert e["empty"].block_table().shape == (0, 4)
    c = e["corner"].block_table()
    assert c.shape == (1, 4) and tuple(c[0]) == (0, 2 * 8, 2 * 32, (8 << 32) | 6)
    # zero heights: the block-rows of height 0 of `heights` hold no block; w13z's are in the middle of a builder-made matrix; the third geometry is written
    # out here with blocks IN its zero-height block-rows -- listed with no elements, so that block b stays entry b of jab
    z = sa_vbr(_edge_arrays(10, 40, 16, [4, 0, 6, 0], [[0, 2], [1, 2], [2], [0]]), np.arange(4 * 32 + 6 * 16, dtype=np.float32))
    for v in (e["heights"], train_geometries()["w13z"], z):
        T = _check_table(v)
        h = np.repeat(np.diff(v.row_part), np.asarray(v.nzcount, np.int64))
        assert len(T) == len(v.jab) and ((T[:, 3] & 0xffffffff) == v.jab).all()
        assert ((T[:, 2] == 0) == (h == 0)).all() and ((T[:, 1] == 0) == (h == 0)).all()
    assert (np.diff(e["heights"].row_part) == 0).any() and (np.diff(train_geometries()["w13z"].row_part) == 0).any()
    assert tuple(z.block_table()[:, 2]) == (64, 64, 0, 0, 96, 0) and tuple(z.block_table()[:, 1]) == (64, 32, 0, 0, 48, 0)
    assert tuple(z.block_table((1, 4))[:, 0]) == (0, 0, 0, 96)


def test_block_table_count_only_and_refusals():
    for key, v in edge_geometries().items():
        rp, nz, jab = (np.ascontiguousarray(a, np.int64) for a in (v.row_part, v.nzcount, v.jab))
        n = C.c_int64(-1)
        args = (v.cols, v.block_rows, v.block_col_size, rp.ctypes.data_as(_i64p), nz.ctypes.data_as(_i64p), jab.ctypes.data_as(_i64p))
        assert lib.sparta_vbs_block_table_host(*args, 0, v.block_rows, None, C.byref(n)) == _lib.OK
        assert n.value == len(v.jab) == len(v.block_table()), key
        if v.block_rows > 1:
            assert lib.sparta_vbs_block_table_host(*args, 1, v.block_rows, None, C.byref(n)) == _lib.OK
            assert n.value == len(v.jab) - int(v.nzcount[0])
        assert lib.sparta_vbs_block_table_host(*args, 0, v.block_rows + 1, None, C.byref(n)) == _lib.ERR_INVALID
        assert lib.sparta_vbs_block_table_host(*args, 0, v.block_rows, None, None) == _lib.ERR_INVALID
        assert "sparta_vbs_block_table_host" in lib.sparta_last_error().decode()
    v = edge_geometries()["dense"]
    rp, nz = (np.ascontiguousarray(a, np.int64) for a in (v.row_part, v.nzcount))
    bad = np.array([0, 1, 0, 7], np.int64)                                  # a block column past the last one
    T, n = np.zeros((4, 4), np.int64), C.c_int64(0)
    rc = lib.sparta_vbs_block_table_host(v.cols, v.block_rows, v.block_col_size, rp.ctypes.data_as(_i64p), nz.ctypes.data_as(_i64p), bad.ctypes.data_as(_i64p), 0, 2,
                                         T.ctypes.data_as(_i64p), C.byref(n))
    assert rc == _lib.ERR_INVALID and "jab" in lib.sparta_last_error().decode()


def test_prune_symbols_prototypes_and_null_handles():
    f32p, vp, u8p, f64p = C.POINTER(C.c_float), C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_double)
    for s in ("sparta_vbs_block_table_host", "sparta_vbs_block_count", "sparta_vbs_block_ssq", "sparta_vbs_mask_blocks"):
        assert s in _lib.SYMBOLS and hasattr(lib, s), s
    assert list(lib.sparta_vbs_block_ssq.argtypes) == [vp, f32p, f64p, vp, f32p]
    assert list(lib.sparta_vbs_mask_blocks.argtypes) == [vp, u8p, f32p, f32p, f32p, f32p, vp, f32p]
    hdr = open(os.path.join(ROOT, "include", "sparta_amd.h")).read()
    for decl in ("int sparta_vbs_block_ssq(sparta_vbs_t* A, const float* W, double* ssq_out, void* stream, float* dt_ms);",
                 "int sparta_vbs_mask_blocks(sparta_vbs_t* A, const uint8_t* keep, float* T0, float* T1, float* T2, float* T3, void* stream, float* dt_ms);",
                 "int sparta_vbs_block_count(const sparta_vbs_t* A, int64_t* n_blocks_out);", "n_in < 2^26"):
        assert decl in hdr, decl
    w, out, keep, n = (C.c_float * 4)(), (C.c_double * 4)(), (C.c_uint8 * 4)(), C.c_int64(5)
    for call, name in ((lambda: lib.sparta_vbs_block_ssq(None, w, out, None, None), "sparta_vbs_block_ssq"),
                       (lambda: lib.sparta_vbs_mask_blocks(None, keep, w, None, None, None, None, None), "sparta_vbs_mask_blocks"),
                       (lambda: lib.sparta_vbs_block_count(None, C.byref(n)), "sparta_vbs_block_count")):
        assert call() == _lib.ERR_INVALID
        msg = lib.sparta_last_error().decode()
        assert name in msg and "NULL" in msg, msg
    assert n.value == 5
    src = open(os.path.join(ROOT, "sparta_amd", "csrc", "k_prune.hip")).read()
    assert "atomic" not in src.lower() and "__shared__" not in src


# ---- the selection rule -------------------------------------------------------------------------------------------------------------------------------
torch = pytest.importorskip("torch")


def _sel(scores, keep, s, scope="global"):
    out = sa.prune.select([torch.tensor(x, dtype=torch.float64) for x in scores], [torch.tensor(k, dtype=torch.uint8) for k in keep], s, scope)
    assert all(o.dtype == torch.uint8 for o in out) and [o.numel() for o in out] == [len(k) for k in keep]
    return [o.tolist() for o in out]


def test_select_ties_go_to_the_lower_index():
    assert _sel([[1.0, 1.0, 1.0, 1.0]], [[1, 1, 1, 1]], 0.5) == [[0, 0, 1, 1]]
    assert _sel([[2.0, 1.0], [1.0, 1.0]], [[1, 1], [1, 1]], 0.5) == [[1, 0], [0, 1]]          # (layer, block): layer 0's 1.0, then layer 1's first
    assert _sel([[0.0, 3.0, 0.0, 0.0, 3.0]], [[1, 1, 1, 1, 1]], 0.4) == [[0, 1, 0, 1, 1]]


def test_select_is_monotone_and_hits_the_count():
    rng = np.random.default_rng(5)
    scores = [rng.integers(0, 6, n).astype(np.float64).tolist() for n in (7, 12, 1)]          # many ties
    keep = [[1] * 7, [1] * 12, [1]]
    for scope in ("global", "layer"):
        prev = keep
        for s in (0.0, 0.1, 0.25, 0.5, 0.5, 0.74, 0.75, 0.9, 1.0):
            new = _sel(scores, prev, s, scope)
            for p, q in zip(prev, new):
                assert all(b <= a for a, b in zip(p, q))                   # a pruned block stays pruned
            if scope == "global":
                assert sum(x == 0 for q in new for x in q) == math.floor(s * 20)
            else:
                assert [sum(x == 0 for x in q) for q in new] == [math.floor(s * n) for n in (7, 12, 1)]
            # the same masks in one step from nothing: the rule depends on the scores and the count alone
            assert new == _sel(scores, keep, s, scope)
            prev = new
    assert _sel(scores, keep, 0.0) == keep
    assert _sel(scores, keep, 1.0) == [[0] * 7, [0] * 12, [0]]


def test_select_never_takes_a_nonfinite_score_while_a_finite_one_is_left():
    inf, nan = float("inf"), float("nan")
    s = [[nan, 5.0, inf, 1.0, -inf, 2.0]]
    assert _sel(s, [[1] * 6], 0.5) == [[1, 0, 1, 0, 1, 0]]
    assert _sel(s, [[1] * 6], 0.84) == [[0, 0, 0, 0, 1, 0]]                # floor(5.04) = 5: three finite, then the non-finite in index order
    assert _sel(s, [[1] * 6], 1.0) == [[0] * 6]


def test_select_global_and_layer_differ():
    # layer 0 holds the four smallest scores: global pruning at 50 % empties it, per-layer pruning takes two of each
    scores, keep = [[1.0, 2.0, 3.0, 4.0], [10.0, 20.0, 30.0, 40.0]], [[1] * 4, [1] * 4]
    assert _sel(scores, keep, 0.5, "global") == [[0, 0, 0, 0], [1, 1, 1, 1]]
    assert _sel(scores, keep, 0.5, "layer") == [[0, 0, 1, 1], [0, 0, 1, 1]]


def test_select_below_the_pruned_count_changes_nothing():
    scores, keep = [[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]], [[1, 0, 1, 0, 0, 1]]
    for s in (0.0, 0.2, 0.5):                                              # k = 0, 1, 3 <= 3 already pruned
        assert _sel(scores, keep, s) == keep
    assert _sel(scores, keep, 0.67) == [[0, 0, 1, 0, 0, 1]]                # k = 4: one more, the lowest live score
    # the scores of pruned blocks do not matter (they are zeros after pruning, below every live score)
    assert _sel([[9.0, 0.0, 3.0, 0.0, 0.0, 1.0]], keep, 0.67) == [[1, 0, 1, 0, 0, 0]]
    with pytest.raises(ValueError):
        _sel(scores, keep, 1.5)
    with pytest.raises(ValueError):
        _sel(scores, keep, 0.5, "row")


def test_prune_imports_without_torch():
    code = ("import sys; sys.modules['torch'] = None\n"
            "import sparta_amd.prune as p, sparta_amd as sa\n"
            "assert p.BlockPruner is sa.BlockPruner and sys.modules.get('torch') is None\n"
            "print('ok')\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)
