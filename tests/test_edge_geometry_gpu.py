"""Degenerate block geometries through every device entry point: sparta_vbs_spmm (every forward path), sparta_vbs_create_from_csr, sparta_vbs_sddmm,
sparta_vbs_spmm_t, sparta_vbs_set_values and range handles, on the tiny matrices of tests/_util.py: edge_geometries() -- one row, one column, cols < w,
no block at all, one block in the last corner, all-zero blocks, block-rows of height 0 / 1 / 257, a fully dense VBS, w = 1.  They are made from arrays
(VBR.from_arrays), not by the builder: the shapes a caller of the C-ABI can hand over and a seeded random CSR never produces, where a launch has a grid of
zero workgroups, a plan zero workers, a panel is wider than the matrix.

Reference: tests/_util.py: edge_dense() expands the arrays into a float64 matrix (values rounded to the storage type first for 16-bit handles); A @ B, A.T @ X
and (X @ Y.T) sampled into the mab layout are plain numpy on it (tests/test_edge_geometry_host.py proves the expansion against the oracle's multiply and the
block-column index walk).  'int' values (-3 .. 3, operands -3 .. 3): every partial sum is an integer far below 2^24, so every kernel must give the float64
result cast to float32 bit for bit.  'real' values: |got - want| <= 1e-5 * sum|a||b| + 1e-30 per element (TOL of test_spmm_gpu.py); an accumulating call
adds 1e-5 * |C0| (one more fp32 addition, onto C0).

Conventions: device pointers throughout; an output is prefilled with NaN before an overwrite call and with a seeded finite C0 before an accumulate call; every
leading dimension is padded (rows + 5, cols + 3, n + 5; rounded up to even for 16-bit operands), the padding of an output must come back bit for bit, the
padding of an input holds a large finite value (3e38; 6e4 in fp16) that would wreck the result if it were multiplied."""
import ctypes as C

import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd import _lib
from sparta_amd._lib import lib

torch = pytest.importorskip("torch")

import _util as U  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-5
DT_ID = {sa.F32: "f32", sa.F16: "f16", sa.BF16: "bf16"}
TDT = {sa.F32: torch.float32, sa.F16: torch.float16, sa.BF16: torch.bfloat16}
BIG = {sa.F32: 3e38, sa.F16: 6e4, sa.BF16: 3e38}
PATH_NAME = {0: "none", 1: "stream", 2: "per-class", 3: "generic"}
VALUE_SETS = ("int", "real")
F32_CASES = [(k, sa.F32) for k in U.EDGE_F32]
H16_CASES = [(k, dt) for dt in (sa.F16, sa.BF16) for k in U.EDGE_H16]
ALL_CASES = F32_CASES + H16_CASES
ids_of = lambda cases: ["%s-%s" % (k, DT_ID[dt]) for k, dt in cases]  # noqa: E731
every = pytest.mark.parametrize("key,dtype", ALL_CASES, ids=ids_of(ALL_CASES))

MODE_ENV = ("SPARTA_SPARSE_K", "SPARTA_SPARSE_MIN_STEPS", "SPARTA_LAUNCH_NNZ", "SPARTA_COLRES", "SPARTA_UNION", "SPARTA_NO_VEC", "SPARTA_FORCE_GENERIC")
_HANDLES = {}
EVERY_F32 = {}        # fp32 geometry -> the paths that carried a product of 128 columns in test_forward_f32_every_path, checked by the last test
CARRIED = {}          # (geometry, dtype) -> what carried the default-mode product, printed by the last test


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for d in _HANDLES.values():
        d.close()
    _HANDLES.clear()


@pytest.fixture(params=["mfma-only", "with-sparse-rows", "library-defaults"])
def mode(request, monkeypatch):
    """the sparse-row modes of tests/test_spmm_gpu.py: every block-row on the MFMA kernels; the sparse-row path on with the rules that keep a small matrix on
    one kind of launch off; nothing overridden"""
    for k in MODE_ENV + ("SPARTA_PATH", "SPARTA_H16_PATH"):
        monkeypatch.delenv(k, raising=False)
    if request.param == "mfma-only":
        monkeypatch.setenv("SPARTA_SPARSE_K", "0")
    if request.param == "with-sparse-rows":
        monkeypatch.setenv("SPARTA_SPARSE_MIN_STEPS", "0")
    if request.param != "library-defaults":
        monkeypatch.setenv("SPARTA_LAUNCH_NNZ", "0")
        monkeypatch.setenv("SPARTA_COLRES", "0")
    return request.param


@pytest.fixture
def plain_env(monkeypatch):
    for k in MODE_ENV + ("SPARTA_PATH", "SPARTA_H16_PATH"):
        monkeypatch.delenv(k, raising=False)


def geometry(key, vs="int"):
    return U.edge_geometries(vs)[key]


def with_values(v, mab):
    return sa.VBR.from_arrays(v.rows, v.cols, v.block_col_size, v.row_part, v.nzcount, v.jab, np.ascontiguousarray(mab, np.float32))


def handle(tag, v, dtype, **kw):
    """one handle per tag for the module (the tag names geometry, values, dtype, flags and whatever of the environment the creation reads)"""
    if tag not in _HANDLES:
        _HANDLES[tag] = v.to_device(0, dtype=dtype, **kw)
    return _HANDLES[tag]


def ld_of(n, pad, dtype):
    x = n + pad
    return x + (x & 1) if dtype != sa.F32 else x


def operand(shape, seed, vs, dtype):
    """a seeded dense operand as the device will hold it, float64: integers -3 .. 3, or uniform(-1, 1) rounded to the handle's B type"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, shape).astype(np.float64) if vs == "int" else rng.uniform(-1, 1, shape)
    return U.edge_round(x, dtype)


def dev_in(M, ld, dtype):
    """M (r x n, exact in dtype) as a column-major device operand with leading dimension ld; the padding rows hold BIG"""
    r, n = M.shape
    buf = np.full((n, ld), BIG[dtype], np.float32)
    buf[:, :r] = M.T
    return torch.from_numpy(buf.reshape(-1)).to(TDT[dtype]).cuda()


def out_buffer(r, n, ld, row_major, C0):
    """(host image, lines, line length): an output of r x n with leading dimension ld -- NaN everywhere (overwrite) or C0 inside and 77 in the padding"""
    lines, used = (r, n) if row_major else (n, r)
    img = np.full((lines, ld), np.nan if C0 is None else 77.0, np.float32)
    if C0 is not None:
        img[:, :used] = C0 if row_major else C0.T
    return img, used


def read_out(Cd, img, used, row_major, what):
    got = Cd.cpu().numpy().reshape(img.shape)
    assert np.array_equal(got[:, used:].view(np.uint32), img[:, used:].view(np.uint32)), (what, "the padding of the output was written")
    return got[:, :used] if row_major else got[:, :used].T


def spmm(d, rows, Bd, ldb, n, row_major=False, C0=None, algo=sa.SPMM_MFMA, what=""):
    ldc = n + 5 if row_major else rows + 5
    img, used = out_buffer(rows, n, ldc, row_major, C0)
    Cd = torch.from_numpy(img.reshape(-1).copy()).cuda()
    d.spmm(Bd, Cd, n, accumulate=C0 is not None, algo=algo, c_layout=sa.ROW_MAJOR if row_major else sa.COL_MAJOR, ldb=ldb, ldc=ldc)
    torch.cuda.synchronize()
    return read_out(Cd, img, used, row_major, what)


def check(got, want, bound, vs, what, C0=None):
    """int: bit for bit; real: TOL * (sum|a||b| (+ |C0|)) + 1e-30.  No NaN may be left either way."""
    assert not np.isnan(got).any(), (what, "NaN left in the output")
    ref = want if C0 is None else want + C0
    if vs == "int":
        assert np.array_equal(got, ref.astype(np.float32)), (what, float(np.abs(got - ref).max(initial=0)))
    else:
        lim = TOL * (bound + (0 if C0 is None else np.abs(C0))) + 1e-30
        err = np.abs(got.astype(np.float64) - ref)
        assert (err <= lim).all(), (what, float(err.max(initial=0)), float((err / lim).max(initial=0)))


def expected_paths(d, v, dtype, n, forced):
    """the forward paths a product of n columns may end on under SPARTA_PATH = forced (None: unset), by the rule of sparta_vbs_spmm: the stream plan needs
    w % 32 == 0 and workers, the per-class kernels w % 64 == 0, both whole 128-column slabs; everything else is the generic kernels' (16-bit handles have the
    stream kernels only).  A forced path that quietly falls back fails the caller's assertion."""
    if dtype != sa.F32:
        return {"stream"}
    w, full = v.block_col_size, n % 128 == 0
    can_stream, can_class = w % 32 == 0 and full and d.info()["stream_workers"] > 0, w % 64 == 0 and full
    if forced == "stream":
        return {"stream"} if can_stream else {"generic"}
    if forced == "class":
        return {"per-class"} if can_class else {"generic"}
    if forced == "generic":
        return {"generic"}
    if can_stream and can_class:
        return {"stream", "per-class"}                 # the handle times both once and keeps the faster
    return {"stream"} if can_stream else {"per-class"} if can_class else {"generic"}


def forward_sweep(d, v, dtype, vs, ns, seed, what, br=None, record=None, D=None, forced=None):
    """overwrite and accumulate, C column- and row-major, every n of ns: the product of handle d against the reference (D: the dense form, if not v's own)"""
    D = U.edge_dense(v, dtype, br=br) if D is None else D
    rows = D.shape[0]
    for n in ns:
        B = operand((v.cols, n), seed + n, vs, dtype)
        ldb = ld_of(v.cols, 3, dtype)
        Bd = dev_in(B, ldb, dtype)
        want, bound = D @ B, np.abs(D) @ np.abs(B)
        C0 = operand((rows, n), seed + 500 + n, vs, sa.F32) * 5.0
        for row_major in (False, True):
            for acc in (None, C0):
                w_ = (what, "n=%d" % n, "C row-major" if row_major else "C column-major", "accumulate" if acc is not None else "overwrite")
                got = spmm(d, rows, Bd, ldb, n, row_major, acc, what=w_)
                check(got, want, bound, vs, w_, acc)
                carried = PATH_NAME[d.info()["last_path"]]
                assert carried in expected_paths(d, v, dtype, n, forced), (w_, "carried by", carried)
                if record is not None:
                    record.add((n, carried))
                if acc is not None and not D.any():
                    assert np.array_equal(got.view(np.uint32), acc.astype(np.float32).view(np.uint32)), (w_, "C += 0 changed C")


def report(key, dtype, d, paths):
    info, sp, cr, ui = d.info(), d.sparse_info(), d.colres_info(), d.union_info()
    CARRIED[(key, DT_ID[dtype])] = {"tiles": info["tiles16"] + info["tiles32"] + info["tiles64"], "stream_steps": info["stream_steps"], "paths": sorted(paths),
                                    "sparse_rows": sp["rows"], "sparse_nnz": sp["nnz"], "resident_columns": cr["nc"], "union_tiles": ui["tiles32"] + ui["tiles64"]}


# ---- 1. forward product, fp32 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", U.EDGE_F32)
def test_forward_f32_every_path(key, mode, monkeypatch):
    """SPARTA_PATH stream / class / generic / unset (read per call; a path the geometry cannot take falls to the generic kernels), n = 1, 128 (a whole slab:
    the stream and per-class kernels), 130; then the exact-order kernel on the same handle, bit-identical to the oracle's VBR::multiply"""
    for vs in VALUE_SETS:
        v = geometry(key, vs)
        d = handle((key, vs, "f32", mode), v, sa.F32)
        if mode != "with-sparse-rows":                                   # no block-row has left the tiles: a geometry of 32-wide panels has a stream plan, `empty` included
            assert (d.info()["stream_workers"] > 0) == (v.block_col_size % 32 == 0), d.info()
        for forced in ("stream", "class", "generic", None):
            if forced is None:
                monkeypatch.delenv("SPARTA_PATH", raising=False)
            else:
                monkeypatch.setenv("SPARTA_PATH", forced)
            seen = set()
            forward_sweep(d, v, sa.F32, vs, (1, 128, 130), 100, (key, vs, mode, forced or "unset"), record=seen, forced=forced)
            EVERY_F32.setdefault(key, set()).update(c for n, c in seen if n == 128)
            if forced is None and mode == "library-defaults" and vs == "real":
                report(key, sa.F32, d, {c for _, c in seen})
        n = 130
        B = operand((v.cols, n), 900, vs, sa.F32)
        ldb = v.cols + 3
        got = spmm(d, v.rows, dev_in(B, ldb, sa.F32), ldb, n, algo=sa.SPMM_EXACT, what=(key, vs, mode, "exact"))
        ref = O.vbr_multiply(v.rows, v.cols, v.block_col_size, v.row_part, v.nzcount, v.jab, v.mab, B.T.astype(np.float32).reshape(-1), n)
        assert np.array_equal(got.view(np.uint32), ref.reshape(n, v.rows).T.view(np.uint32)), (key, vs, mode, "exact-order kernel")


# ---- 2. forward product, 16-bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h16_path", [None, "lds", "direct"], ids=["unset", "lds", "direct"])
@pytest.mark.parametrize("key,dtype", H16_CASES, ids=ids_of(H16_CASES))
def test_forward_h16_every_kernel(key, dtype, h16_path, mode, monkeypatch):
    """SPARTA_H16_PATH is read when the plan is made and at every launch: one handle per setting.  n = 256 reaches the 256-column slab and the
    four-accumulator launches, n = 1 and 130 the padded tail slab"""
    if h16_path is not None:
        monkeypatch.setenv("SPARTA_H16_PATH", h16_path)
    for vs in VALUE_SETS:
        v = geometry(key, vs)
        d = handle((key, vs, DT_ID[dtype], mode, h16_path), v, dtype)
        seen = set()
        forward_sweep(d, v, dtype, vs, (1, 128, 256, 130), 200, (key, vs, DT_ID[dtype], mode, h16_path or "unset"), record=seen)
        if h16_path is None and mode == "library-defaults" and vs == "real":
            report(key, dtype, d, {c for _, c in seen})


# ---- 3. the same matrix through DeviceVBS.from_csr ---------------------------------------------------------------------------------------------
CSR_CASES = [(k, sa.F32) for k in U.EDGE_F32 if k != "heights"] + [(k, sa.F16) for k in U.EDGE_H16 if k != "heights32"]


@pytest.mark.parametrize("key,dtype", CSR_CASES, ids=ids_of(CSR_CASES))
def test_from_csr_gives_the_same_product(key, dtype, mode):
    """the CSR holds the non-zeros of the dense form, the grouping is the block-row of every row (row_part): the builder then makes its own VBS -- `zeros`
    loses its all-zero blocks, `empty` is a CSR without an entry -- and the product must still be the reference's, its rows in the order of the grouping's
    permutation (row r of C is row get_permutation(grouping)[r] of the CSR, as for VBR.fill_from_CSR_inplace)"""
    for vs in VALUE_SETS:
        v = geometry(key, vs)
        D = U.edge_dense(v)
        r, c = np.nonzero(D)
        m = sa.CSR(v.rows, v.cols, np.concatenate([[0], np.cumsum(np.bincount(r, minlength=v.rows))]), c.astype(np.int32), D[r, c].astype(np.float32))
        g = np.repeat(np.arange(v.block_rows, dtype=np.int64), np.diff(v.row_part))
        perm = sa.get_permutation(g)
        assert np.array_equal(np.sort(perm), np.arange(v.rows)) and np.array_equal(g[perm], g)          # rows move inside their block-row only
        d = sa.DeviceVBS.from_csr(m, g, v.block_col_size, device=0, dtype=dtype)
        try:
            assert (d.rows, d.cols) == (v.rows, v.cols)
            forward_sweep(d, v, dtype, vs, (1, 130), 300, (key, vs, DT_ID[dtype], mode, "from_csr"), D=U.edge_dense(v, dtype)[perm])
        finally:
            d.close()


# ---- 4. sddmm ----------------------------------------------------------------------------------------------------------------------------------
def sddmm(d, v, X, Y, dtype, G0=None, br=None, what=""):
    """G (+)= (X Y^T) on the stored blocks; G sits in a buffer with 8 guard elements behind it"""
    k = X.shape[1]
    ldx, ldy = ld_of(X.shape[0], 5, dtype), ld_of(v.cols, 3, dtype)
    lo, hi = U.edge_mab_slice(v, br or (0, v.block_rows))
    img = np.full(hi - lo + 8, np.nan if G0 is None else 77.0, np.float32)
    if G0 is not None:
        img[:hi - lo] = G0
    Gd = torch.from_numpy(img.copy()).cuda()
    d.sddmm(dev_in(X, ldx, dtype), dev_in(Y, ldy, dtype), Gd, k, accumulate=G0 is not None, ldx=ldx, ldy=ldy)
    torch.cuda.synchronize()
    got = Gd.cpu().numpy()
    assert np.array_equal(got[hi - lo:].view(np.uint32), img[hi - lo:].view(np.uint32)), (what, "sddmm wrote behind G")
    return got[:hi - lo]


def sddmm_sweep(d, v, dtype, vs, ks, seed, what, br=None):
    b0, b1 = br or (0, v.block_rows)
    rows = int(v.row_part[b1] - v.row_part[b0])
    for k in ks:
        X, Y = operand((rows, k), seed + k, vs, dtype), operand((v.cols, k), seed + 50 + k, vs, dtype)
        want, bound = U.edge_sample(v, X @ Y.T, br), U.edge_sample(v, np.abs(X) @ np.abs(Y).T, br)
        G0 = operand(want.shape, seed + 90 + k, vs, sa.F32) * 5.0
        for acc in (None, G0):
            w_ = (what, "k=%d" % k, "accumulate" if acc is not None else "overwrite")
            check(sddmm(d, v, X, Y, dtype, acc, br, w_), want, bound, vs, w_, acc)


@every
def test_sddmm(key, dtype, plain_env):
    for vs in VALUE_SETS:
        v = geometry(key, vs)
        sddmm_sweep(handle((key, vs, DT_ID[dtype], "plain"), v, dtype), v, dtype, vs, (1, 33, 128), 400, (key, vs, DT_ID[dtype], "sddmm"))


@pytest.mark.parametrize("dtype", [sa.F32, sa.F16, sa.BF16], ids=["f32", "f16", "bf16"])
def test_sddmm_on_the_empty_handle_touches_nothing(dtype, plain_env):
    v = geometry("empty")
    d = handle(("empty", "int", DT_ID[dtype], "plain"), v, dtype)
    assert d.info()["nztot"] == 0 and d.info()["nblocks"] == 0
    k = 33
    ldx, ldy = ld_of(v.rows, 5, dtype), ld_of(v.cols, 3, dtype)
    Xd, Yd = dev_in(operand((v.rows, k), 1, "int", dtype), ldx, dtype), dev_in(operand((v.cols, k), 2, "int", dtype), ldy, dtype)
    for acc in (0, 1):
        guard = torch.full((1,), 123.5, dtype=torch.float32, device="cuda")
        rc = lib.sparta_vbs_sddmm(d.h, C.c_void_p(Xd.data_ptr()), ldx, C.c_void_p(Yd.data_ptr()), ldy, k, C.cast(C.c_void_p(guard.data_ptr()), C.POINTER(C.c_float)),
                                  acc, _lib.PTR_DEVICE, C.c_void_p(torch.cuda.current_stream(0).cuda_stream), None)
        torch.cuda.synchronize()
        assert rc == 0, lib.sparta_last_error().decode()
        assert guard.item() == 123.5


# ---- 5. spmm_t ---------------------------------------------------------------------------------------------------------------------------------
def spmm_t(d, v, X, dtype, C0=None, what=""):
    """Ct (+)= A^T X: Ct is cols x n with ldo = cols + 3; nothing at or past row cols may be written"""
    n = X.shape[1]
    ldx, ldo = ld_of(X.shape[0], 5, dtype), v.cols + 3
    img, used = out_buffer(v.cols, n, ldo, False, C0)
    Cd = torch.from_numpy(img.reshape(-1).copy()).cuda()
    d.spmm_t(dev_in(X, ldx, dtype), Cd, n, accumulate=C0 is not None, ldx=ldx, ldo=ldo)
    torch.cuda.synchronize()
    return read_out(Cd, img, used, False, what)


def spmm_t_sweep(d, v, dtype, vs, ns, seed, what, br=None, mab=None):
    D = U.edge_dense(v, dtype, mab=mab, br=br)
    stored = U.edge_dense(v, mab=np.ones(len(v.mab), np.float32), br=br).any(axis=0)          # columns of A that lie in a stored block
    for n in ns:
        X = operand((D.shape[0], n), seed + n, vs, dtype)
        want, bound = D.T @ X, np.abs(D).T @ np.abs(X)
        C0 = operand((v.cols, n), seed + 70 + n, vs, sa.F32) * 5.0
        for acc in (None, C0):
            w_ = (what, "n=%d" % n, "accumulate" if acc is not None else "overwrite")
            got = spmm_t(d, v, X, dtype, acc, w_)
            check(got, want, bound, vs, w_, acc)
            if acc is None:
                assert not got[~stored].any(), (w_, "a row of Ct without a stored block is not 0")


@every
def test_spmm_t(key, dtype, plain_env):
    for vs in VALUE_SETS:
        v = geometry(key, vs)
        d = handle((key, vs, DT_ID[dtype], "t"), v, dtype, transposable=True)
        spmm_t_sweep(d, v, dtype, vs, (1, 33, 128), 500, (key, vs, DT_ID[dtype], "spmm_t"))


# ---- 6. set_values -----------------------------------------------------------------------------------------------------------------------------
def seeded_past_cols(v, vs, seed):
    """the geometry's values with a seeded non-zero at every stored position past cols: they must take no part in any product"""
    V = v.mab.copy()
    w = v.block_col_size
    rng = np.random.default_rng(seed)
    for off, _, h, _, valid in U.edge_blocks(v):
        n = (w - valid) * h
        V[off + valid * h:off + w * h] = rng.integers(1, 4, n) if vs == "int" else rng.uniform(0.25, 1, n)
    return V


def every_entry_point(d, v, dtype, vs, monkeypatch, forward_paths):
    """forward product per forced path at n = 128 (a whole slab: the stream and per-class kernels where the geometry has them) and n = 130 (the generic kernels;
    16-bit: a slab and the padded tail slab), sddmm and spmm_t of handle d, as raw results; the path that carried each forward product is asserted"""
    out, ops = [], {}
    ldb = ld_of(v.cols, 3, dtype)
    for n in (128, 130):
        ops[n] = operand((v.cols, n), 600 + n, vs, dtype)
        Bd = dev_in(ops[n], ldb, dtype)
        for name, forced in forward_paths:
            if forced is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, forced)
            for row_major in (False, True):
                what = "forward n=%d %s C %s" % (n, forced or "unset", "row-major" if row_major else "column-major")
                out.append((what, n, spmm(d, v.rows, Bd, ldb, n, row_major)))
                carried = PATH_NAME[d.info()["last_path"]]
                assert carried in expected_paths(d, v, dtype, n, forced if name == "SPARTA_PATH" else None), (what, "carried by", carried)
    X, Y = operand((v.rows, 33), 610, vs, dtype), operand((v.cols, 33), 611, vs, dtype)
    out.append(("sddmm", 0, sddmm(d, v, X, Y, dtype)))
    out.append(("spmm_t", 0, spmm_t(d, v, X, dtype)))
    return out, (ops, X, Y)


@every
def test_set_values_on_a_handle_created_from_zeros(key, dtype, plain_env, monkeypatch):
    """the order in which vbs_linear initialises a layer: the handle is created from an all-zero mab, then given the values.  Every entry point must then
    equal, bit for bit, a fresh handle created from the same values (and the reference); set back to zeros, an overwrite product is exactly 0.  fp32: the
    stream path reads the fragment image wherever the geometry has tiles of <= 32 rows of 32-wide panels, the per-class and generic kernels the
    reference-layout image: set_values must have refreshed both."""
    if dtype == sa.F32:
        settings = [(None, [("SPARTA_PATH", p) for p in ("stream", "class", "generic", None)])]
    else:                                    # SPARTA_H16_PATH is read when the plan is made as well: a pair of handles per setting
        settings = [(p, [("SPARTA_H16_PATH", p)]) for p in (None, "lds")]
    for vs in VALUE_SETS:
        v = geometry(key, vs)
        V = seeded_past_cols(v, vs, 620)
        zeros = np.zeros(len(v.mab), np.float32)
        D = U.edge_dense(v, dtype, mab=V)                                            # (drops the positions past cols)
        for create_env, paths in settings:
            monkeypatch.delenv("SPARTA_H16_PATH", raising=False)
            if create_env is not None:
                monkeypatch.setenv("SPARTA_H16_PATH", create_env)
            H = with_values(v, zeros).to_device(0, dtype=dtype, updatable=True, transposable=True)
            F = with_values(v, V).to_device(0, dtype=dtype, updatable=True, transposable=True)
            try:
                H.set_values(torch.from_numpy(V).cuda())
                got, (Bs, X, Y) = every_entry_point(H, v, dtype, vs, monkeypatch, paths)
                fresh, _ = every_entry_point(F, v, dtype, vs, monkeypatch, paths)
                for (what, n, a), (_, _, b) in zip(got, fresh):
                    assert not np.isnan(a).any(), (key, vs, what)
                    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (key, vs, what, "differs from a fresh handle")
                    if what.startswith("forward"):
                        check(a, D @ Bs[n], np.abs(D) @ np.abs(Bs[n]), vs, (key, vs, what))
                    elif what == "sddmm":
                        check(a, U.edge_sample(v, X @ Y.T), U.edge_sample(v, np.abs(X) @ np.abs(Y).T), vs, (key, vs, what))
                    else:
                        check(a, D.T @ X, np.abs(D).T @ np.abs(X), vs, (key, vs, what))
                H.set_values(torch.from_numpy(zeros).cuda())
                back, _ = every_entry_point(H, v, dtype, vs, monkeypatch, paths)
                for what, _, a in back:
                    if what != "sddmm":
                        assert not a.any(), (key, vs, what, "not 0 after set_values(zeros)")
            finally:
                H.close()
                F.close()


@pytest.mark.parametrize("dtype", [sa.F32, sa.F16, sa.BF16], ids=["f32", "f16", "bf16"])
def test_set_values_on_the_empty_handle(dtype, plain_env):
    v = geometry("empty")
    H = v.to_device(0, dtype=dtype, updatable=True, transposable=True)
    try:
        st = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
        assert lib.sparta_vbs_set_values(H.h, None, _lib.PTR_DEVICE, st, None) == 0, lib.sparta_last_error().decode()
        assert lib.sparta_vbs_set_values(H.h, None, _lib.PTR_HOST, None, None) == 0, lib.sparta_last_error().decode()
        H.set_values(torch.empty(0, dtype=torch.float32, device="cuda"))
        H.set_values_host(np.zeros(0, np.float32))
        forward_sweep(H, v, dtype, "int", (130,), 630, ("empty", DT_ID[dtype], "after set_values"))
    finally:
        H.close()


# ---- 7. range handles --------------------------------------------------------------------------------------------------------------------------
RANGES = {      # block-row ranges: heights* -- from a zero-height block-row; up to one; block-rows without any block (1 row: heights 0, 1, 0)
    "heights": [(2, 6), (12, 14), (0, 3)], "heights32": [(2, 6), (12, 14), (0, 3)],
    "corner": [(8, 9), (3, 9), (0, 8)],          # the block-row with the block alone; with empty block-rows in front; the block-rows without any block
    "tall": [(0, 1), (1, 2)], "tall64": [(0, 1), (1, 2)],        # one block-row each: the range starts in the middle of jab and mab
}
RANGE_CASES = [(k, sa.F32) for k in ("heights", "corner", "tall")] + [(k, sa.F16) for k in ("heights32", "corner", "tall64")]


@pytest.mark.parametrize("key,dtype", RANGE_CASES, ids=ids_of(RANGE_CASES))
def test_range_handles(key, dtype, plain_env):
    for vs in VALUE_SETS:
        v = geometry(key, vs)
        hts = np.diff(v.row_part)
        for br in RANGES[key]:
            rows = int(hts[br[0]:br[1]].sum())
            assert rows >= 1
            d = v.to_device(0, dtype=dtype, block_row_range=br, updatable=True, transposable=True)
            try:
                lo, hi = U.edge_mab_slice(v, br)
                assert (d.rows, d.cols, d.info()["nztot"]) == (rows, v.cols, hi - lo)
                what = (key, vs, DT_ID[dtype], "range %d:%d" % br)
                forward_sweep(d, v, dtype, vs, (1, 130), 700, what, br=br)
                sddmm_sweep(d, v, dtype, vs, (33,), 710, what, br=br)
                spmm_t_sweep(d, v, dtype, vs, (33,), 720, what, br=br)
                whole = -seeded_past_cols(v, vs, 730)
                d.set_values(torch.from_numpy(np.ascontiguousarray(whole[lo:hi])).cuda())          # the slice of the range, negated
                spmm_t_sweep(d, v, dtype, vs, (33,), 740, what + ("after set_values",), br=br, mab=whole)
            finally:
                d.close()
    kinds = RANGES["heights"]
    h = np.diff(geometry("heights").row_part)
    nz = geometry("heights").nzcount
    assert h[kinds[0][0]] == 0 and h[kinds[1][1] - 1] == 0 and not nz[kinds[2][0]:kinds[2][1]].any()


# ---- last in the file --------------------------------------------------------------------------------------------------------------------------
def test_zz_report_which_kernels_carried_the_default_products():
    """per geometry and dtype: what the handle's own records say carried the products of the library-defaults mode (printed: pytest -s, or the captured
    output of a failure)"""
    for k in sorted(CARRIED):
        print("edge geometry | %-10s %-4s | %s" % (k + (" ".join("%s=%s" % (a, "+".join(b) if isinstance(b, list) else b) for a, b in CARRIED[k].items()),)))
    if EVERY_F32:
        for key, paths in EVERY_F32.items():
            w = geometry(key).block_col_size
            want = {"generic"} | ({"stream"} if w % 32 == 0 else set()) | ({"per-class"} if w % 64 == 0 else set())
            assert paths == want, (key, paths, want)
        per_class = {k for k, p in EVERY_F32.items() if "per-class" in p}
        if set(U.EDGE_F32) <= set(EVERY_F32):
            assert per_class == {"dense", "corner64", "heights64"}, per_class          # corner64, heights64: block-rows without a block / of height 0 on the per-class kernels
    for (key, dt), rec in CARRIED.items():
        if key == "empty":
            assert rec["sparse_nnz"] == 0 and rec["stream_steps"] == 0, rec
        assert set(rec["paths"]) <= {"stream", "per-class", "generic"} and rec["paths"], rec
