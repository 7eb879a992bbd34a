"""The live forward product on the GPU: DeviceVBS.set_live_forward and what the 16-bit forward product does with a live-block set installed -- the contract of
include/sparta_amd.h, "WITH A LIVE-BLOCK SET INSTALLED AND LIVE FORWARD ON".

Handles: the 16-bit edge, training and poison geometries in f16 and bf16 plus three written out here -- `split` (one 32-row block-row of 300 32-wide blocks: a
split tile, asserted), `pairs` (eight 32-row block-rows of 32-wide blocks over a ragged last block column: pair tiles only, halves that disagree under
`one_per_row` and `row_dead`), `tiles64` (two 64-row block-rows of 64-wide blocks) and `short64` (block-rows of 24 and 17 rows of 64-wide blocks: the one-tile
kernels of 64-deep steps, through the C ring with a column-major C and without it with a row-major one) -- all made updatable and transposable; `split` and
`w96` once more on the plan with two sub-workers per workgroup (SPARTA_H16_WIDE=1: the 64-column waves).  LIVE_FORM lists the geometries
whose handle has ONE stream image and so takes the live form; the others (two stream images; P64 once its hub plan is forced) must say that they keep the
plain kernels.  References: a second handle of the same geometry that never gets the switch, and numpy."""
import functools

import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd import _lib
from sparta_amd.autograd import vbs_linear

torch = pytest.importorskip("torch")

import _util as U  # noqa: E402
import _live as L  # noqa: E402
import _live_forward as LF  # noqa: E402
from test_poison_gpu import TOL  # noqa: E402  (the suite's bound for 16-bit handles: TOL * sum|a||b|)

pytestmark = pytest.mark.gpu

f32 = np.float32
TDT = {sa.F16: torch.float16, sa.BF16: torch.bfloat16, sa.F32: torch.float32}
DT_ID = {sa.F16: "f16", sa.BF16: "bf16", sa.F32: "f32"}
H16 = (sa.F16, sa.BF16)
OWN = ("split", "pairs", "tiles64", "short64")
KEYS = U.EDGE_H16 + U.TRAIN_H16 + U.POISON_H16 + OWN
# the geometries whose 16-bit handle has one stream image (and no hub plan): the live form, and which image it is (1: <= 32-row tiles, 2: 64-row / pair tiles)
# (tall, heights32, tall64, w256 and P32 have both images; P64 is too small for a hub plan by default and takes the live form -- test_forms_taken forces the hub plan)
LIVE_FORM = {"rowvec": 1, "narrow32": 1, "corner": 1, "zeros": 1, "dense": 2, "w96": 1, "w128": 2, "P64": 2, "split": 1, "pairs": 2, "tiles64": 2, "short64": 1}
N_COLS = (8, 128, 256)
ENV = ("SPARTA_H16_PATH", "SPARTA_H16_AHEAD", "SPARTA_H16_PAIR", "SPARTA_H16_WIDE", "SPARTA_H16_SLAB256", "SPARTA_H16_QUAD", "SPARTA_CSTAGE", "SPARTA_HUB")


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


@functools.lru_cache(maxsize=None)
def geometry(key):
    if key == "split":
        a = U._edge_arrays(32, 300 * 32, 32, [32], [list(range(300))])
        return U.sa_vbr(a, U._edge_values(a, "real", 9100))
    if key == "pairs":
        a = U._edge_arrays(8 * 32, 8 * 32 - 11, 32, [32] * 8, [U.poison_present(ib) for ib in range(8)])
        return U.sa_vbr(a, U._edge_values(a, "real", 9101))
    if key == "tiles64":
        a = U._edge_arrays(128, 4 * 64, 64, [64, 64], [[0, 1, 3], [1, 2]])
        return U.sa_vbr(a, U._edge_values(a, "real", 9102))
    if key == "short64":
        a = U._edge_arrays(41, 3 * 64 - 5, 64, [24, 17], [[0, 2], [1, 2]])
        return U.sa_vbr(a, U._edge_values(a, "real", 9103))
    return L.geometry(key)


@functools.lru_cache(maxsize=None)
def table(key):
    T = geometry(key).block_table(None)
    T.setflags(write=False)
    return T


def mask(key, name):
    """tests/_live.py's masks on the geometries written out here as well"""
    if key not in OWN:
        return L.mask(key, None, name)
    T = table(key)
    n = len(T)
    brow, bcol = T[:, 3] >> 32, T[:, 3] & 0xffffffff
    keep = np.ones(n, np.uint8)
    if name == "none":
        keep[:] = 0
    elif name == "second":
        keep[1::2] = 0
    elif name == "one_per_row":
        keep[:] = 0
        keep[np.unique(brow, return_index=True)[1]] = 1
    elif name == "row_dead":
        keep[brow == np.bincount(brow).argmax()] = 0
    elif name == "col_dead":
        keep[bcol == np.bincount(bcol).argmax()] = 0
    elif name in ("rand50", "rand90"):
        keep[np.random.default_rng(9300 + n + int(name[4:])).random(n) < int(name[4:]) / 100.0] = 0
    return keep


CASES = [(k, dt) for dt in H16 for k in KEYS if int(geometry(k).nztot) > 0]           # (`empty` stores nothing: no values to set, no block to mask)
LIVE_CASES = [c for c in CASES if c[0] in LIVE_FORM]
case_id = lambda c: "%s-%s" % (c[0], DT_ID[c[1]])  # noqa: E731
cases = pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
live_cases = pytest.mark.parametrize("case", LIVE_CASES, ids=[case_id(c) for c in LIVE_CASES])

_HANDLES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for d in _HANDLES.values():
        d.close()
    _HANDLES.clear()


def handle(case, which):
    """two handles per case: "live" gets the switch, "plain" never does"""
    if (case, which) not in _HANDLES:
        key, dtype = case
        _HANDLES[(case, which)] = geometry(key).to_device(0, dtype=dtype, updatable=True, transposable=True)
    return _HANDLES[(case, which)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, f32)).cuda()


@functools.lru_cache(maxsize=None)
def values(key):
    """the stored values of the tests: seeded uniform(-1, 1), none zero"""
    x = np.random.default_rng(9200 + len(table(key))).uniform(-1, 1, int(geometry(key).nztot)).astype(f32)
    x[x == 0] = 0.5
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def rhs(key, dtype):
    """B of 256 columns as the device holds it (float64, cols x 256); the first n columns serve a product of n columns"""
    return U.edge_round(np.random.default_rng(9250).uniform(-1, 1, (geometry(key).cols, 256)), dtype)


def b_tensor(B, dtype):
    """column-major with an even leading dimension"""
    cols, n = B.shape
    ld = cols + (cols & 1)
    buf = np.zeros((n, ld), f32)
    with np.errstate(all="ignore"):
        buf[:, :cols] = B.T
    return torch.from_numpy(buf.reshape(-1)).to(TDT[dtype]).cuda(), ld


def product(d, key, Bt, ldb, n, row_major=False, C0=None):
    """C (rows x n, numpy) of one sparta_vbs_spmm; C0: accumulate onto it, else the output starts as NaN"""
    rows = int(geometry(key).rows)
    img = np.full((rows, n) if row_major else (n, rows), np.nan, f32)
    if C0 is not None:
        img[:] = C0 if row_major else C0.T
    Cd = torch.from_numpy(img.reshape(-1).copy()).cuda()
    d.spmm(Bt, Cd, n, accumulate=C0 is not None, c_layout=sa.ROW_MAJOR if row_major else sa.COL_MAJOR, ldb=ldb, ldc=n if row_major else rows)
    torch.cuda.synchronize()
    got = Cd.cpu().numpy()
    return got.reshape(rows, n) if row_major else got.reshape(n, rows).T


def install(d, key, name, W=None, live=True):
    """what BlockPruner does: the dead blocks +0.0 in the values, the handle given the values and (live) the mask"""
    keep = mask(key, name)
    kt = torch.from_numpy(np.array(keep)).cuda()
    Wt = dev(np.array(values(key)) if W is None else W)
    if W is None:
        d.mask_blocks(kt, Wt)
    d.set_values(Wt)
    if live:
        d.set_live_blocks(kt)
    return keep


def form_of(d):
    fi = d.live_forward_info()
    return max(fi["form_one_tile"], fi["form_pair"]), fi


def test_geometries_cover_what_they_are_for():
    """the split tile, the pair tiles and the handles that must keep the plain kernels are really there"""
    for dt in H16:
        fi = handle(("split", dt), "live").live_forward_info()
        assert fi["split_tiles"] > 0 and fi["capable"] == 1, fi
        assert handle(("split", dt), "live").info()["split_tiles"] == fi["split_tiles"]
        d = handle(("pairs", dt), "live")
        assert d.live_forward_info()["capable"] == 2 and d.info()["stream_steps"] < int(geometry("pairs").nzcount.sum()), d.info()
    for case in CASES:
        assert handle(case, "live").live_forward_info()["capable"] == LIVE_FORM.get(case[0], 0), case
    assert handle(("w96", sa.F16), "live").info()["split_tiles"] > 0 and handle(("w128", sa.F16), "live").info()["split_tiles"] > 0


@live_cases
def test_lists(case):
    """the device lists equal the host rule, the host rule equals the Python restatement, and both satisfy the invariants"""
    key, dtype = case
    d = handle(case, "live")
    d.set_live_forward(True)
    for name in L.MASKS:
        install(d, key, name)
        got = d.live_forward_lists()
        assert got["pair"] == (LIVE_FORM[key] == 2) and len(got["steps"]) == d.info()["stream_steps"]
        out, r_out, info = sa.live_forward_compact(got["steps"], got["ranges"], got["pair"], got["live"])
        assert np.array_equal(got["ranges_live"], r_out), (name, np.flatnonzero((got["ranges_live"] != r_out).any(axis=1))[:4])
        assert np.array_equal(got["steps_live"], out), (name, np.flatnonzero(got["steps_live"] != out)[:8])
        want, r_want = LF.rule(got["steps"], got["ranges"], got["pair"], got["live"])
        assert np.array_equal(out, want) and np.array_equal(r_out, r_want), name
        LF.check_invariants(got["steps"], got["ranges"], got["pair"], got["live"], got["steps_live"], got["ranges_live"])
        fi = d.live_forward_info()
        assert fi["kept_steps"] == info["kept"] and fi["steps"] == info["steps"] == len(out) and fi["switch"] == 1, (name, fi, info)
        if name == "all":
            assert info["kept"] == info["steps"] and info["dead_segments"] == 0
        if name == "none":
            assert info["kept"] == info["segments"] == info["dead_segments"]


@cases
def test_equivalence_on_dead_zero_values(case):
    """dead blocks +0.0 in the values: the product under the switch equals the plain product of a second handle element for element, the sign of a zero
    aside -- every mask, 8 / 128 / 256 columns (the slab and four-accumulator launches), both layouts of C, overwriting and accumulating"""
    key, dtype = case
    check_equivalence(handle(case, "live"), handle(case, "plain"), key, dtype)


def check_equivalence(a, b, key, dtype):
    a.set_live_forward(True)
    rows = int(geometry(key).rows)
    C0 = np.random.default_rng(9400).uniform(-1, 1, (rows, 256)).astype(f32)
    Bt, ldb = b_tensor(rhs(key, dtype), dtype)
    for name in L.MASKS:
        install(a, key, name)
        install(b, key, name, live=False)
        for n in N_COLS:
            for row_major in (False, True):
                for acc in (False, True):
                    c0 = C0[:, :n] if acc else None
                    x, y = product(a, key, Bt, ldb, n, row_major, c0), product(b, key, Bt, ldb, n, row_major, c0)
                    assert np.array_equal(x + f32(0), y + f32(0)), (name, n, row_major, acc, np.argwhere(~((x + f32(0)) == (y + f32(0))))[:4].tolist())
        form, fi = form_of(a)
        assert form == (2 if key in LIVE_FORM else 1) or fi["steps"] == 0 and form <= 1, (name, fi)
        assert form_of(b)[0] <= 1


@live_cases
def test_dead_blocks_depend_on_nothing(case):
    """NaN in every value of every dead block, NaN in every row of B of every block column that holds a dead block: a row of C whose live blocks avoid those
    block columns equals the product of the live blocks alone (the suite's bound for 16-bit handles), rows reached only through dead blocks are +0.0 or keep
    what they held.  With the switch off the same call shows the NaN in every row that has a dead block: the inputs bite."""
    key, dtype = case
    check_dead_blocks(handle(case, "live"), key, dtype)


def check_dead_blocks(d, key, dtype):
    v, T = geometry(key), table(key)
    d.set_live_forward(True)
    w, rows, cols = int(v.block_col_size), int(v.rows), int(v.cols)
    brow, bcol = T[:, 3] >> 32, T[:, 3] & 0xffffffff
    r0 = np.asarray(v.row_part, np.int64)
    B = rhs(key, dtype)
    checked = 0
    for name in L.MASKS:
        keep = mask(key, name)
        dead = keep == 0
        W = values(key).copy()
        W[~L.element_keep(T, keep)] = np.nan
        install(d, key, name, W=W)
        Wl = np.where(L.element_keep(T, keep), values(key), f32(0))
        D = U.edge_dense(v, dtype, mab=Wl)
        bad_cols = np.unique(bcol[dead])
        Bp = B.copy()
        for jb in bad_cols:
            Bp[jb * w:min((jb + 1) * w, cols)] = np.nan
        # block-rows none of whose live blocks lie in a poisoned block column
        ok_row = np.zeros(rows, bool)
        has_dead = np.zeros(rows, bool)
        for ib in range(v.block_rows):
            mine = brow == ib
            ok_row[r0[ib]:r0[ib + 1]] = not np.isin(bcol[mine & ~dead], bad_cols).any()
            has_dead[r0[ib]:r0[ib + 1]] = bool((mine & dead).any())
        Bt, ldb = b_tensor(Bp, dtype)
        for n in N_COLS:
            want, bound = D[ok_row] @ B[:, :n], np.abs(D[ok_row]) @ np.abs(B[:, :n])
            for row_major in (False, True):
                got = product(d, key, Bt, ldb, n, row_major)[ok_row].astype(np.float64)
                assert np.isfinite(got).all(), (name, n, row_major, "NaN reached %d elements that only live blocks define" % int((~np.isfinite(got)).sum()))
                assert (np.abs(got - want) <= TOL * bound + 1e-30).all(), (name, n, row_major, float(np.abs(got - want).max()))
                only_dead = (has_dead & ~np.abs(D).any(axis=1))[ok_row]
                assert not got[only_dead].any() and not np.signbit(got[only_dead]).any(), (name, n, "rows reached only through dead blocks are +0.0")
            C0 = np.random.default_rng(9500).uniform(-1, 1, (rows, n)).astype(f32)
            got = product(d, key, Bt, ldb, n, False, C0)[ok_row].astype(np.float64)
            assert (np.abs(got - (want + C0[ok_row])) <= TOL * (bound + np.abs(C0[ok_row])) + 1e-30).all(), (name, n, "accumulate")
            assert np.array_equal(got[only_dead], C0[ok_row][only_dead].astype(np.float64)), (name, n, "accumulate leaves rows of dead blocks alone")
        assert form_of(d)[0] == 2
        checked += int((ok_row & has_dead).sum())
        if dead.any():                                     # the switch off: every row with a dead block shows the NaN
            d.set_live_forward(False)
            got = product(d, key, Bt, ldb, 128)
            assert form_of(d)[0] == 1 and np.isnan(got[has_dead]).all(), (name, "the inputs do not bite")
            d.set_live_forward(True)
    assert checked > 0, "no row with a dead block could be checked"
    install(d, key, "all")


@pytest.mark.parametrize("key", ["split", "w96"])
def test_two_sub_workers_per_workgroup(key, monkeypatch):
    """the one-tile plan of 32-wide blocks with two sub-worker ranges per workgroup (SPARTA_H16_WIDE=1 at creation): the live 64-column-wave kernel on the
    compacted sub-ranges; with 256 columns it keeps the non-slab kernel"""
    monkeypatch.setenv("SPARTA_H16_WIDE", "1")
    dtype = sa.F16
    a, b = (geometry(key).to_device(0, dtype=dtype, updatable=True, transposable=True) for _ in range(2))
    try:
        a.set_live_forward(True)
        fi = a.live_forward_info()
        assert fi["capable"] == 1 and fi["ranges"] == 2 * a.info()["stream_workers"], (fi, a.info())
        check_equivalence(a, b, key, dtype)
        check_dead_blocks(a, key, dtype)
        install(a, key, "rand50")
        got = a.live_forward_lists()
        out, r_out, _ = sa.live_forward_compact(got["steps"], got["ranges"], got["pair"], got["live"])
        assert np.array_equal(got["steps_live"], out) and np.array_equal(got["ranges_live"], r_out)
    finally:
        a.close()
        b.close()


def test_forms_taken(monkeypatch):
    """live_forward_info says which kernels ran: the live form on a qualifying handle; the plain form on an fp32 handle, on P64 (hub plan), on a handle with
    two stream images, under SPARTA_H16_PATH=lds and SPARTA_H16_AHEAD=7, with the switch off and after set_live_blocks(None)"""
    key, dtype = "zeros", sa.F16
    case = (key, dtype)
    d, p = handle(case, "live"), handle(case, "plain")
    Bt, ldb = b_tensor(rhs(key, dtype), dtype)
    d.set_live_forward(True)
    install(d, key, "second")
    install(p, key, "second", live=False)
    want = product(p, key, Bt, ldb, 128)
    assert form_of(p)[0] == 1 and p.live_forward_info()["switch"] == 0
    assert np.array_equal(product(d, key, Bt, ldb, 128) + f32(0), want + f32(0)) and form_of(d)[0] == 2
    # (seven steps ahead is a choice of the launches outside the C ring: a row-major C here, the tiles of `zeros` are 24 rows tall)
    for env, rm in ((("SPARTA_H16_PATH", "lds"), False), (("SPARTA_H16_AHEAD", "7"), True)):
        monkeypatch.setenv(*env)
        assert np.array_equal(product(d, key, Bt, ldb, 128, rm) + f32(0), product(p, key, Bt, ldb, 128, rm) + f32(0)) and form_of(d)[0] == 1, env
        monkeypatch.delenv(env[0])
        assert np.array_equal(product(d, key, Bt, ldb, 128, rm) + f32(0), want + f32(0)) and form_of(d)[0] == 2, env
    d.set_live_forward(False)
    product(d, key, Bt, ldb, 128)
    assert form_of(d) [0] == 1 and d.live_forward_info()["switch"] == 0
    d.set_live_forward(True)
    product(d, key, Bt, ldb, 128)
    assert form_of(d)[0] == 2
    d.set_live_blocks(None)
    assert np.array_equal(product(d, key, Bt, ldb, 128) + f32(0), want + f32(0)) and form_of(d)[0] == 1 and d.live_forward_info()["switch"] == 1
    install(d, key, "second")
    product(d, key, Bt, ldb, 128)
    assert form_of(d)[0] == 2
    for k in ("P64", "P32"):                           # the hub plan (forced onto this small matrix as tests/test_poison_gpu.py forces it); two stream images
        if k == "P64":
            for name, val in (("SPARTA_HUB_MIN_TOTAL", "1"), ("SPARTA_HUB_MIN_STEPS", "1"), ("SPARTA_HUB_G", "2"), ("SPARTA_HUB_TAU", "0.25")):
                monkeypatch.setenv(name, val)
        h = geometry(k).to_device(0, dtype=dtype, updatable=True, transposable=True)
        try:
            assert (h.hub_info()["steps"] > 0) == (k == "P64")
            h.set_live_forward(True)
            install(h, k, "second")
            b, l = b_tensor(rhs(k, dtype), dtype)
            got = product(h, k, b, l, 128)
            fi = h.live_forward_info()
            assert fi["switch"] == 1 and fi["capable"] == 0 and fi["form_one_tile"] != 2 and fi["form_pair"] != 2 and fi["steps"] == 0, (k, fi)
            D = U.edge_dense(geometry(k), dtype, mab=np.where(L.element_keep(table(k), mask(k, "second")), values(k), f32(0)))
            assert (np.abs(got - D @ rhs(k, dtype)[:, :128]) <= TOL * (np.abs(D) @ np.abs(rhs(k, dtype)[:, :128])) + 1e-30).all(), k
        finally:
            h.close()
    v = geometry(key)
    h = v.to_device(0, dtype=sa.F32, updatable=True, transposable=True)
    try:
        h.set_live_forward(True)
        h.set_live_blocks(torch.from_numpy(np.array(mask(key, "second"))).cuda())
        b = torch.from_numpy(np.ascontiguousarray(rhs(key, sa.F32)[:, :128].T, f32).reshape(-1)).cuda()
        C = torch.zeros(128 * v.rows, device="cuda")
        h.spmm(b, C, 128)
        torch.cuda.synchronize()
        fi = h.live_forward_info()
        assert fi["switch"] == 1 and fi["capable"] == 0 and fi["form_one_tile"] == 0 and fi["form_pair"] == 0, fi
    finally:
        h.close()


def test_switches_and_refusals():
    v = geometry("zeros")
    d = v.to_device(0, dtype=sa.F16, transposable=True)
    try:
        with pytest.raises(sa.SpartaError) as e:
            d.set_live_forward(True)
        assert e.value.code == _lib.ERR_UNSUPPORTED and "SPARTA_CREATE_UPDATABLE" in str(e.value)
    finally:
        d.close()
    d = v.to_device(0, dtype=sa.F16, updatable=True, transposable=True)
    try:
        fi = d.live_forward_info()
        assert fi["switch"] == 0 and fi["capable"] == 1 and fi["kept_steps"] == 0
        with pytest.raises(sa.SpartaError):
            d.live_forward_lists()                       # no live set
        scratch = torch.zeros(4, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        caught = []
        with torch.cuda.stream(s):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                scratch.add_(1.0)
                try:
                    d.set_live_forward(True)
                except sa.SpartaError as err:
                    caught.append(err)
                scratch.add_(1.0)
            torch.cuda.synchronize()
            assert len(caught) == 1 and caught[0].code == _lib.ERR_UNSUPPORTED and "captured" in str(caught[0]) and "sparta_vbs_set_live_forward" in str(caught[0])
            g.replay()
            torch.cuda.synchronize()
        assert float(scratch[0]) == 2.0 and d.live_forward_info()["switch"] == 0
        d.set_live_forward(True)
        d.set_live_forward(False)
        assert d.live_forward_info()["switch"] == 0
    finally:
        d.close()


@pytest.mark.parametrize("key", ["zeros", "pairs"])
def test_capture(key):
    """set_live_blocks + spmm in one graph: a replay follows keep rewritten in place and equals the eager product of a second handle under the new mask.  The
    values are non-zero everywhere: what the replay computes depends on the mask alone"""
    dtype = sa.F16
    v = geometry(key)
    d, e = (v.to_device(0, dtype=dtype, updatable=True, transposable=True) for _ in range(2))
    try:
        rows, n = int(v.rows), 128
        Bt, ldb = b_tensor(rhs(key, dtype), dtype)
        masks = [mask(key, m) for m in ("second", "rand90", "one_per_row", "none", "all")]
        keep = torch.from_numpy(np.array(masks[0])).cuda()
        Wt = dev(np.array(values(key)))
        C = torch.zeros(n * rows, device="cuda")
        s = torch.cuda.Stream()
        for h in (d, e):
            h.set_values(Wt)
            h.set_live_forward(True)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            d.set_live_blocks(keep)                              # the eager warm-up: helper arrays
            d.spmm(Bt, C, n, ldb=ldb, ldc=rows)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                d.set_live_blocks(keep)
                d.spmm(Bt, C, n, ldb=ldb, ldc=rows)
            torch.cuda.synchronize()
            for m in masks[1:] + masks[:1]:
                keep.copy_(torch.from_numpy(np.array(m)).cuda())
                C.fill_(7.0)
                torch.cuda.synchronize()
                g.replay()
                torch.cuda.synchronize()
                got = C.cpu().numpy().reshape(n, rows).T
                e.set_live_blocks(torch.from_numpy(np.array(m)).cuda())
                want = product(e, key, Bt, ldb, n)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int(np.count_nonzero(m))
                assert d.live_info()["live_blocks"] == int(np.count_nonzero(m))
                D = U.edge_dense(v, dtype, mab=np.where(L.element_keep(table(key), m), values(key), f32(0)))
                ref, bound = D @ rhs(key, dtype)[:, :n], np.abs(D) @ np.abs(rhs(key, dtype)[:, :n])
                assert (np.abs(got - ref) <= TOL * bound + 1e-30).all()
        assert form_of(d)[0] == 2
    finally:
        d.close()
        e.close()


@pytest.mark.parametrize("key", ["w128", "w96"])          # (pair / 64-row tiles; one-tile records with split tiles; vbs_linear wants even rows and cols)
def test_training_with_live_forward(key):
    """vbs_linear + VbsAdamW + BlockPruner for four steps, prune(0.5) after the first and prune(0.75) after the third: BlockPruner(skip_pruned=True,
    live_steps=True, live_forward=True) against the same without live_forward -- W, both moments and the step state bit-identical"""
    dtype = sa.F16
    v = geometry(key)
    W0 = np.random.default_rng(5800).uniform(-1, 1, int(v.nztot)).astype(f32)
    n = 8
    rnd = lambda shape, seed, dt: U.edge_round(np.random.default_rng(seed).uniform(-1, 1, shape), dt)  # noqa: E731
    xs = [torch.from_numpy(rnd((n, v.cols), 5810 + s, dtype)).to(TDT[dtype]).cuda() for s in range(4)]
    gys = [torch.from_numpy(rnd((n, v.rows), 5820 + s, sa.F32)).float().cuda() for s in range(4)]

    def train(live_forward):
        H = v.to_device(0, dtype=dtype, updatable=True, transposable=True)
        try:
            W = torch.from_numpy(W0.copy()).cuda().requires_grad_(True)
            opt = sa.VbsAdamW([(H, W)], lr=1e-2, weight_decay=0.01)
            pruner = sa.BlockPruner(opt, skip_pruned=True, live_steps=True, live_forward=live_forward)
            trace, forms, ys = [], [], []
            for step in range(4):
                x = xs[step].clone().requires_grad_(True)
                opt.zero_grad()
                y = vbs_linear(x, H, W)
                forms.append(form_of(H)[0])
                ys.append(y.detach().float().cpu().numpy() + f32(0))
                y.backward(gys[step].to(y.dtype))
                opt.step()
                st = opt._state[0]
                trace.append([t.detach().cpu().numpy().copy() for t in (W, st["exp_avg"], st["exp_avg_sq"], st["state"])])
                if step in (0, 2):
                    pruner.prune(0.5 if step == 0 else 0.75)
            return trace, forms, ys, H.live_forward_info()
        finally:
            H.close()

    (a, fa, ya, ia), (b, fb, yb, ib) = train(True), train(False)
    live = 2 if LIVE_FORM.get(key, 0) else 1
    assert fa == [1, live, live, live] and fb == [1, 1, 1, 1] and ia["switch"] == 1 and ib["switch"] == 0, (fa, fb)
    for step, (ta, tb) in enumerate(zip(a, b)):
        assert np.array_equal(ya[step], yb[step]), step
        for name, x, y in zip(("W", "exp_avg", "exp_avg_sq", "state"), ta, tb):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (step, name)


def test_pruner_needs_skip_pruned():
    with pytest.raises(ValueError):
        sa.BlockPruner([], live_forward=True)
