"""The sparse-row device form (k_sparse.hip; sparta_amd/csrc/vbs_capi.cpp: order_sparse_rows) on the HOST: sparta_sparse_rows_host_check builds the form of a
CSR matrix -- the list of short rows, the long rows cut into segments, the column windows, the eight per-XCD streams -- and walks it as the kernels do for one
column of B, refusing a form in which a nonzero is not covered exactly once, a row's segments are out of order, or the window / stream order is broken.
Small-integer values: every order of additions gives the same bits, so the walked product must EQUAL the CSR product.  No GPU involved."""
import numpy as np
import pytest

import sparta_amd as sa

ROWS, COLS = 96, 512
_SWITCHES = ("SPARTA_SPARSE_SEG", "SPARTA_SP_WINDOW_COLS", "SPARTA_SP_LONG", "SPARTA_SP_MINSEG", "SPARTA_SP_XCD")
WINDOWS = [dict(SPARTA_SP_WINDOW_COLS="64", SPARTA_SP_LONG="8", SPARTA_SP_MINSEG=m, SPARTA_SP_XCD=x) for m in ("1", "4") for x in ("0", "1")]
# (switches, the base segment length and the long-row cut they put in force: below 2^20 nonzeros a segment is 32, a row is long above two segments;
#  with windows a row is long above SPARTA_SP_LONG)
SETTINGS = [({}, 32, 64), (dict(SPARTA_SPARSE_SEG="8"), 8, 16)] + [(w, 32, 8) for w in WINDOWS]
_ids = ["defaults", "seg8"] + ["win64-long8-minseg%s-xcd%s" % (w["SPARTA_SP_MINSEG"], w["SPARTA_SP_XCD"]) for w in WINDOWS]


def _csr(lengths, seed, window=None):
    """rows of the given lengths: ascending distinct columns (all inside one `window`-column window per row if given), values in +-1..3"""
    rng = np.random.default_rng(seed)
    rp, ci = [0], []
    for n in lengths:
        if window is None:
            c = rng.choice(COLS, n, replace=False)
        else:
            c = int(rng.integers(0, COLS // window)) * window + rng.choice(window, n, replace=False)
        ci.append(np.sort(c))
        rp.append(rp[-1] + n)
    ci = np.concatenate(ci).astype(np.int32)
    va = (rng.integers(1, 4, ci.size) * rng.choice([-1, 1], ci.size)).astype(np.float32)
    return np.array(rp, np.int64), ci, va


def _matrix(seg, long_cut, seed=5):
    """96 x 512: the row lengths at which the builder changes its mind -- 0, 1, the long-row cut and its neighbours, three segments and one more, a full row --
    in front of rows of 0..40 nonzeros"""
    rng = np.random.default_rng(seed)
    edge = [0, 1, long_cut - 1, long_cut, long_cut + 1, 3 * seg, 3 * seg + 1, COLS]
    lengths = edge + [int(n) for n in rng.integers(0, 41, ROWS - len(edge))]
    return _csr(lengths, seed + 1)


def _reference(rp, ci, va, x, crow, y0):
    y = y0.copy()
    for i in range(rp.size - 1):
        s = np.float32(np.dot(va[rp[i]:rp[i + 1]].astype(np.float64), x[ci[rp[i]:rp[i + 1]]].astype(np.float64)))
        r = int(crow[i]) & 0x7fffffff
        y[r] = y[r] + s if int(crow[i]) >> 31 else s
    return y


@pytest.fixture
def switches(monkeypatch):
    def put(env):
        for k in _SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    return put


@pytest.mark.parametrize("env,seg,long_cut", SETTINGS, ids=_ids)
@pytest.mark.parametrize("add_rows", [False, True], ids=["store", "add-bits"])
def test_walk_of_the_device_form_equals_the_product(switches, env, seg, long_cut, add_rows):
    switches(env)
    rp, ci, va = _matrix(seg, long_cut)
    rng = np.random.default_rng(11)
    x = rng.integers(-3, 4, COLS).astype(np.float32)
    crow = rng.permutation(ROWS).astype(np.int64)
    if add_rows:
        crow[::3] += 1 << 31                                     # bit 31: the row adds to what y holds (the sparse part of a mixed block-row)
    y0 = rng.integers(-5, 6, ROWS).astype(np.float32)
    y, info = sa.sparse_rows_host_check(rp, ci, va, COLS, x, crow=crow, y=y0)
    assert np.array_equal(y, _reference(rp, ci, va, x, crow, y0))
    lengths = np.diff(rp)
    assert (info["seg"], info["long"]) == (seg, long_cut), info
    assert info["rows"] == ROWS and info["short_rows"] == int((lengths <= long_cut).sum()) and info["long_rows"] == int((lengths > long_cut).sum()), info
    assert info["segments"] >= info["long_rows"] > 0
    if "SPARTA_SP_WINDOW_COLS" in env:
        # enough segments for the XCD order to be taken (64), and dealt to more than one stream: the branch cannot be skipped silently
        assert info["win_w"] == 64 and info["minseg"] == int(env["SPARTA_SP_MINSEG"]) and info["segments"] >= 64, info
        assert info["streams"] > 1 if env["SPARTA_SP_XCD"] == "1" else info["streams"] == 0, info
    else:
        assert info["win_w"] == 0 and info["streams"] == 0, info
        # without windows a long row of n nonzeros is cut every max(seg, min(512, sqrt(1.6 n) rounded up to 16)) nonzeros
        cut = lambda n: max(seg, min(512, (int(np.sqrt(1.6 * n)) + 15) // 16 * 16))      # noqa: E731
        assert info["segments"] == sum(-(-int(n) // cut(int(n))) for n in lengths if n > long_cut), info


@pytest.mark.parametrize("env", WINDOWS, ids=_ids[2:])
def test_a_row_inside_one_window_is_one_segment(switches, env):
    """Windows on: a segment ends early only where the row's columns cross into another window.  A row whose nonzeros all lie in ONE window has no such place, and
    at most 64 nonzeros (fewer than the 512 a segment may hold): no segment of it ends early -- every long row is exactly one segment."""
    switches(env)
    rng = np.random.default_rng(2)
    lengths = [0, 1, 8, 9, 64] + [int(n) for n in rng.integers(9, 65, ROWS - 5)]
    rp, ci, va = _csr(lengths, 3, window=64)
    x = rng.integers(-3, 4, COLS).astype(np.float32)
    y, info = sa.sparse_rows_host_check(rp, ci, va, COLS, x)
    assert np.array_equal(y, _reference(rp, ci, va, x, np.arange(ROWS), np.zeros(ROWS, np.float32)))
    assert info["long_rows"] == int((np.diff(rp) > 8).sum()) >= 64 and info["segments"] == info["long_rows"], info
    assert info["streams"] > 1 if env["SPARTA_SP_XCD"] == "1" else info["streams"] == 0, info


def test_rows_that_are_not_sparse_rows_are_left_alone(switches):
    switches({})
    rp, ci, va = _matrix(32, 64)
    x = np.ones(COLS, np.float32)
    crow = np.arange(ROWS, dtype=np.int64)
    crow[1::2] = -1                                              # rows of tiles: not part of the form, their y untouched
    y0 = np.full(ROWS, 7.0, np.float32)
    y, info = sa.sparse_rows_host_check(rp, ci, va, COLS, x, crow=crow, y=y0)
    full = _reference(rp, ci, va, x, np.arange(ROWS), y0)
    assert np.array_equal(y[0::2], full[0::2]) and np.all(y[1::2] == 7.0) and info["rows"] == ROWS // 2


def test_a_csr_that_is_not_one_is_refused(switches):
    """What the walk indexes with is checked first: a bad rowptr, column or crow is SPARTA_ERR_INVALID, not a read out of bounds.
    (The refusals of a broken FORM -- pad not a permutation, a window split across streams, ... -- cannot be provoked from here: the entry point builds the
    form itself from the CSR it is given, so a test sees them only if order_sparse_rows is wrong.  The tests above hold it to the product and the counts.)"""
    switches({})
    rp, ci, va = _matrix(32, 64)
    x = np.ones(COLS, np.float32)
    bad_rp = rp.copy(); bad_rp[5] = rp[6] + 1
    bad_ci = ci.copy(); bad_ci[7] = COLS
    crow = np.arange(ROWS, dtype=np.int64); crow[3] = ROWS
    for args, kw in (((bad_rp, ci, va), {}), ((rp, bad_ci, va), {}), ((rp, ci, va), dict(crow=crow))):
        with pytest.raises(sa.SpartaError):
            sa.sparse_rows_host_check(*args, COLS, x, **kw)
