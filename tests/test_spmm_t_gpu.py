"""sparta_vbs_spmm_t on the GPU (k_spmm_t.hip): Ct (+)= A^T * X on the stored blocks of a handle made with SPARTA_CREATE_TRANSPOSE.

Oracle: a float64 numpy restatement, block by block from the VBS arrays (Ct[jb*w : min(jb*w + w, cols)] += blk[:, :valid].T @ X[r0:r0+h]).
Small-integer A and X are exact in every dtype and must match bit for bit; random data within 1e-5 * (|A|^T |X|) (16-bit handles: against the
oracle on the rounded A and the rounded X)."""
import numpy as np
import pytest

import sparta_amd as sa

torch = pytest.importorskip("torch")

from test_set_values_gpu import (TDT, DT_ID, build_mats, tall_groups, values, oracle as fwd_oracle, dense_b, product, rounded, put)  # noqa: E402
from test_sddmm_gpu import oracle as sddmm_oracle  # noqa: E402

pytestmark = pytest.mark.gpu


def oracle(v, mab, X, b0=0, b1=None, absolute=False):
    """float64 Ct = A^T X for the values `mab` (the range's slice) on the pattern of block-rows [b0, b1) of v; X: the range's rows x n.  cols x n."""
    w = v.block_col_size
    b1 = v.block_rows if b1 is None else b1
    r_lo = int(v.row_part[b0])
    a = np.asarray(mab, np.float64)
    Xd = np.asarray(X, np.float64)
    if absolute:
        a, Xd = np.abs(a), np.abs(Xd)
    Ct = np.zeros((v.cols, Xd.shape[1]))
    jo = sum(int(v.nzcount[i]) for i in range(b0))
    mo = 0
    for ib in range(b0, b1):
        r0, h, nb = int(v.row_part[ib]) - r_lo, int(v.row_part[ib + 1] - v.row_part[ib]), int(v.nzcount[ib])
        for b in range(nb):
            c0 = int(v.jab[jo + b]) * w
            c1 = min(c0 + w, v.cols)
            blk = a[mo + b * w * h: mo + (b + 1) * w * h].reshape(w, h).T
            Ct[c0:c1] += blk[:, :c1 - c0].T @ Xd[r0:r0 + h]
        jo += nb
        mo += nb * h * w
    return Ct


@pytest.fixture(scope="module")
def mats():
    return build_mats()


def with_values(v, mab):
    u = sa.VBR()
    u.__dict__.update(v.__dict__)
    u.mab = np.ascontiguousarray(mab, np.float32)
    u._dev = u._dev_t = u._dev_tp = None
    return u


def dense_x(rows, n, seed, integer):
    rng = np.random.default_rng(seed)
    return rng.integers(-4, 5, (rows, n)).astype(np.float64) if integer else rng.uniform(-1, 1, (rows, n))


SENT = 12345.5


def run_t(d, X, dtype, cols, Ct0=None, accumulate=False, pad=True):
    """X float64 rows x n -> column-major device tensor of the handle's type, ldx padded (padding NaN: never read); Ct column-major with ldo padded,
    the padding rows hold SENT.  Returns (Ct cols x n float32 on the host, X as rounded float64); asserts the padding of Ct is untouched."""
    rows, n = X.shape
    ldx = -(-rows // 8) * 8 + (8 if pad else 0)
    ldo = cols + (5 if pad else 0)
    t = torch.full((n, ldx), float("nan"), dtype=torch.float64)
    t[:, :rows] = torch.from_numpy(np.ascontiguousarray(X.T))
    Xt = t.cuda().to(TDT[dtype]).reshape(-1)
    c = torch.full((n, ldo), float("nan"), dtype=torch.float32)
    if Ct0 is not None:
        c[:, :cols] = torch.from_numpy(np.ascontiguousarray(Ct0.T.astype(np.float32)))
    c[:, cols:] = SENT
    Ctt = c.cuda().reshape(-1)
    d.spmm_t(Xt, Ctt, n, accumulate=accumulate, ldx=ldx, ldo=ldo)
    torch.cuda.synchronize()
    out = Ctt.cpu().numpy().reshape(n, ldo)
    assert np.all(out[:, cols:] == SENT), "rows of Ct at or beyond cols were written"
    Xr = Xt.float().cpu().numpy().astype(np.float64).reshape(n, ldx)[:, :rows].T
    return out[:, :cols].T.copy(), Xr


def check_close(Ct, v, mab, Xr, what=""):
    ref, bound = oracle(v, mab, Xr), oracle(v, mab, Xr, absolute=True)
    assert not np.isnan(Ct).any(), what
    err = np.abs(Ct - ref)
    assert np.all(err <= 1e-5 * bound + 1e-30), (what, float((err - 1e-5 * bound).max()))


def hub_env(monkeypatch, key):
    if key == "hub":
        monkeypatch.setenv("SPARTA_HUB_MIN_TOTAL", "1")
        monkeypatch.setenv("SPARTA_HUB_MIN_STEPS", "1")


F32_KEYS = ["grid1", "grid8", "grid32", "grid64", "jaccard", "padded"]
H16_KEYS = ["grid32", "grid64", "jaccard", "padded", "pairs", "hub"]
CASES = [(k, sa.F32) for k in F32_KEYS] + [(k, dt) for dt in (sa.F16, sa.BF16) for k in H16_KEYS]
CASE_IDS = ["%s-%s" % (k, DT_ID[dt]) for k, dt in CASES]


@pytest.mark.parametrize("key,dtype", CASES, ids=CASE_IDS)
def test_spmm_t_integer_bit_exact(mats, key, dtype, monkeypatch):
    """integer values everywhere -- the positions past cols of the ragged last block column of the 517-column matrices included, NON-zero -- and integer X"""
    hub_env(monkeypatch, key)
    v0 = mats[key]
    V = np.random.default_rng(3).integers(-4, 5, int(v0.nztot)).astype(np.float32)
    V[V == 0] = 2.0
    v = with_values(v0, V)
    d = v.to_device(0, dtype=dtype, transposable=True)
    assert d.transposable and not d.updatable
    if key == "hub":
        assert d.hub_info()["steps"] > 0
    for n in (1, 5, 128, 200):
        X = dense_x(v.rows, n, 100 + n, integer=True)
        Ct, _ = run_t(d, X, dtype, v.cols)
        assert np.array_equal(Ct, oracle(v, V, X).astype(np.float32)), n
    d.close()


@pytest.mark.parametrize("key,dtype", CASES, ids=CASE_IDS)
def test_spmm_t_random_within_bound(mats, key, dtype, monkeypatch):
    hub_env(monkeypatch, key)
    v0 = mats[key]
    V = values(v0, 4, integer=False)
    d = with_values(v0, V).to_device(0, dtype=dtype, transposable=True)
    for n in (5, 128):
        Ct, Xr = run_t(d, dense_x(v0.rows, n, 200 + n, integer=False), dtype, v0.cols)
        check_close(Ct, v0, rounded(V, dtype), Xr, n)
    d.close()


def test_spmm_t_columns_without_a_block_are_zero():
    m0 = sa.gen.uniform_random(200, 400, 700, seed=12)
    m = sa.CSR(200, 900, m0.rowptr, m0.colidx, m0.vals)             # columns 400 .. 899 hold nothing
    v = sa.VBR().fill_from_CSR_inplace(m, np.arange(m.rows, dtype=np.int64) // 16, 8)
    V = np.random.default_rng(5).integers(1, 5, int(v.nztot)).astype(np.float32)
    d = with_values(v, V).to_device(0, transposable=True)
    X = dense_x(v.rows, 37, 7, integer=True)
    Ct, _ = run_t(d, X, sa.F32, v.cols)                              # (Ct starts as NaN)
    assert not np.isnan(Ct).any() and np.all(Ct[400:] == 0)
    assert np.array_equal(Ct, oracle(v, V, X).astype(np.float32))
    d.close()


@pytest.mark.parametrize("dtype", [sa.F32, sa.F16, sa.BF16], ids=["f32", "f16", "bf16"])
def test_spmm_t_ragged_column_values_set_through_set_values(mats, dtype):
    """the 517-column matrix: non-zero values stored past `cols` through set_values take no part, the rows of Ct past cols keep their sentinel"""
    v = mats["grid32"]
    d = v.to_device(0, dtype=dtype, updatable=True, transposable=True)
    V = np.random.default_rng(8).integers(1, 5, int(v.nztot)).astype(np.float32)      # no zero anywhere
    put(d, V)
    for n in (5, 128):
        X = dense_x(v.rows, n, 300 + n, integer=True)
        Ct, _ = run_t(d, X, dtype, v.cols)
        assert np.array_equal(Ct, oracle(v, V, X).astype(np.float32)), n
    d.close()


@pytest.mark.parametrize("dtype", [sa.F32, sa.F16], ids=["f32", "f16"])
def test_spmm_t_accumulate_adds(mats, dtype):
    v0 = mats["jaccard"]
    V = values(v0, 5, integer=True)
    d = with_values(v0, V).to_device(0, dtype=dtype, transposable=True)
    n = 40
    X = dense_x(v0.rows, n, 9, integer=True)
    C0 = np.random.default_rng(10).integers(-9, 10, (v0.cols, n)).astype(np.float64)
    Ct, _ = run_t(d, X, dtype, v0.cols, Ct0=C0, accumulate=True)
    assert np.array_equal(Ct, (C0 + oracle(v0, V, X)).astype(np.float32))
    d.close()


def test_spmm_t_is_the_adjoint_of_spmm(mats):
    v0 = mats["grid8"]
    V = values(v0, 6, integer=True)
    d = with_values(v0, V).to_device(0, transposable=True)
    n = 16
    B = dense_b(v0, n, 11, integer=True)
    X = dense_x(v0.rows, n, 12, integer=True)
    C, _ = product(d, v0, B, sa.F32)
    Ct, _ = run_t(d, X, sa.F32, v0.cols)
    assert float(np.sum(C.astype(np.float64) * X)) == float(np.sum(B * Ct.astype(np.float64)))
    d.close()


UPD_CASES = [("grid8", sa.F32), ("jaccard", sa.F32), ("padded", sa.F32), ("padded", sa.F16), ("pairs", sa.F16), ("pairs", sa.BF16), ("hub", sa.F16), ("hub", sa.BF16),
             ("jaccard", sa.BF16)]


@pytest.mark.parametrize("key,dtype", UPD_CASES, ids=["%s-%s" % (k, DT_ID[dt]) for k, dt in UPD_CASES])
def test_spmm_t_after_set_values(mats, key, dtype, monkeypatch):
    hub_env(monkeypatch, key)
    v = mats[key]
    H = v.to_device(0, dtype=dtype, updatable=True, transposable=True)
    assert H.updatable and H.transposable
    n = 128
    V1 = values(v, 1, integer=True)
    put(H, V1)
    X = dense_x(v.rows, n, 21, integer=True)
    Ct, _ = run_t(H, X, dtype, v.cols)
    assert np.array_equal(Ct, oracle(v, V1, X).astype(np.float32))
    C, _ = product(H, v, dense_b(v, n, 22, integer=True), dtype)       # the forward still follows the new values
    assert np.array_equal(C, fwd_oracle(v, V1, dense_b(v, n, 22, integer=True)).astype(np.float32))
    V2 = values(v, 2, integer=False)
    put(H, V2)
    F = with_values(v, V2).to_device(0, dtype=dtype, transposable=True)
    Xr = dense_x(v.rows, n, 23, integer=False)
    a, _ = run_t(H, Xr, dtype, v.cols)
    b, Xs = run_t(F, Xr, dtype, v.cols)
    assert np.array_equal(a, b)                                       # the same bits as a fresh transposable handle of the new values
    check_close(a, v, rounded(V2, dtype), Xs)
    H.close(); F.close()


def test_spmm_t_after_forward_products_on_the_stream_path(monkeypatch):
    """fp32: the case in which a plain handle drops its reference-layout image after the first products; a transposable one keeps it"""
    monkeypatch.delenv("SPARTA_F32_KEEP_LEGACY", raising=False)
    monkeypatch.setenv("SPARTA_PATH", "stream")
    m = sa.gen.uniform_random(512, 517, 20000, seed=51)
    v = sa.VBR().fill_from_CSR_inplace(m, np.arange(m.rows, dtype=np.int64) // 32, 32)
    n = 128
    P = v.to_device(0, updatable=True)
    H = v.to_device(0, updatable=True, transposable=True)
    B = dense_b(v, n, 30, integer=True)
    held = H.info()["a_bytes"]
    assert held == P.info()["a_bytes"]
    for _ in range(3):
        product(P, v, B, sa.F32); product(H, v, B, sa.F32)
    assert H.info()["a_bytes"] == held                                # nothing dropped
    assert P.info()["a_bytes"] in (held, held - 4 * (int(v.nztot) + 128))
    V1 = values(v, 3, integer=True)
    put(H, V1)
    X = dense_x(v.rows, n, 31, integer=True)
    Ct, _ = run_t(H, X, sa.F32, v.cols)
    assert np.array_equal(Ct, oracle(v, V1, X).astype(np.float32))
    C, _ = product(H, v, B, sa.F32)
    assert np.array_equal(C, fwd_oracle(v, V1, B).astype(np.float32))
    P.close(); H.close()


@pytest.mark.parametrize("dtype", [sa.F32, sa.F16], ids=["f32", "f16"])
def test_spmm_t_range_handles_add_up(mats, dtype):
    v0 = mats["grid32"]
    V = values(v0, 7, integer=True)
    v = with_values(v0, V)
    n = 24
    X = dense_x(v.rows, n, 40, integer=True)
    total = np.zeros((v.cols, n))
    cuts = [0, 5, 6, v.block_rows]
    mo = np.concatenate([[0], np.cumsum(v.nzcount * np.diff(v.row_part) * v.block_col_size)])
    for b0, b1 in zip(cuts, cuts[1:]):
        d = v.to_device(0, dtype=dtype, block_row_range=(b0, b1), transposable=True)
        r0, r1 = int(v.row_part[b0]), int(v.row_part[b1])
        assert d.rows == r1 - r0 and d.cols == v.cols
        part, _ = run_t(d, X[r0:r1], dtype, v.cols, Ct0=total, accumulate=True)
        assert np.array_equal(part, (total + oracle(v, V[mo[b0]:mo[b1]], X[r0:r1], b0, b1)).astype(np.float32))
        total = part.astype(np.float64)
        d.close()
    assert np.array_equal(total, oracle(v, V, X))


@pytest.mark.parametrize("dtype", [sa.F32, sa.BF16], ids=["f32", "bf16"])
def test_spmm_t_host_pointers_match_device_and_calls_repeat(mats, dtype):
    v0 = mats["jaccard"]
    V = values(v0, 8, integer=False)
    d = with_values(v0, V).to_device(0, dtype=dtype, transposable=True)
    n = 50
    X = dense_x(v0.rows, n, 50, integer=False)
    a, Xr = run_t(d, X, dtype, v0.cols, pad=False)
    b, _ = run_t(d, X, dtype, v0.cols, pad=False)
    assert np.array_equal(a, b)                                       # two identical calls, identical bits
    Ch = np.full(v0.cols * n, np.nan, np.float32)
    d.spmm_t_host(np.ascontiguousarray(X.T, np.float32).ravel(), n, Ch, accumulate=False)
    # (16-bit: the host path rounds the fp32 X on the device, the device path got X rounded by torch -- both to nearest even: the same bits)
    assert np.array_equal(Ch.reshape(n, v0.cols).T, a)
    C0 = np.ones(v0.cols * n, np.float32)
    d.spmm_t_host(np.ascontiguousarray(X.T, np.float32).ravel(), n, C0, accumulate=True)
    assert np.array_equal(C0.reshape(n, v0.cols).T, a + np.float32(1.0))
    d.close()


def test_multiply_T_on_the_cached_image(mats):
    v0 = mats["grid8"]
    v = with_values(v0, values(v0, 9, integer=True))
    n = 7
    X = dense_x(v.rows, n, 60, integer=True)
    Ct = v.multiply_T(np.ascontiguousarray(X.T, np.float32).ravel(), n)
    assert np.array_equal(Ct.reshape(n, v.cols).T, oracle(v, v.mab, X).astype(np.float32))
    dev = v._dev_tp
    V2 = values(v0, 10, integer=True)
    v.set_values(V2)
    assert v._dev_tp is dev                                           # updated in place, not re-created
    Ct = v.multiply_T(np.ascontiguousarray(X.T, np.float32).ravel(), n)
    assert np.array_equal(Ct.reshape(n, v.cols).T, oracle(v, V2, X).astype(np.float32))
    v._drop_device_images()


@pytest.mark.parametrize("dtype", [sa.F32, sa.F16], ids=["f32", "f16"])
def test_training_step_graph_capture(mats, dtype):
    """set_values -> spmm -> sddmm -> spmm_t captured as ONE single-branch graph after one eager pass; each replay uses what the captured tensors hold"""
    v = mats["padded"]
    n = 128
    H = v.to_device(0, dtype=dtype, updatable=True, transposable=True)
    tdt = TDT[dtype]
    Bt = torch.zeros((n, v.cols), dtype=tdt, device="cuda")
    Xt = torch.zeros((n, v.rows), dtype=tdt, device="cuda")
    W = torch.from_numpy(values(v, 11, integer=True)).cuda()
    Ct = torch.zeros(v.rows * n, dtype=torch.float32, device="cuda")
    G = torch.zeros(int(v.nztot), dtype=torch.float32, device="cuda")
    dB = torch.zeros(v.cols * n, dtype=torch.float32, device="cuda")

    def step():
        H.set_values(W)
        H.spmm(Bt.reshape(-1), Ct, n)
        H.sddmm(Xt.reshape(-1), Bt.reshape(-1), G, n)
        H.spmm_t(Xt.reshape(-1), dB, n)

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        step()                                                        # once outside a capture (tuning, work lists, scratch)
        torch.cuda.synchronize()
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph, stream=s):
            step()
        for seed in (12, 13):
            Vn = values(v, seed, integer=True)
            B = dense_b(v, n, seed, integer=True)
            X = dense_x(v.rows, n, seed + 50, integer=True)
            W.copy_(torch.from_numpy(Vn).cuda())
            Bt.copy_(torch.from_numpy(np.ascontiguousarray(B.T)).cuda().to(tdt))
            Xt.copy_(torch.from_numpy(np.ascontiguousarray(X.T)).cuda().to(tdt))
            gph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(Ct.cpu().numpy().reshape(n, v.rows).T, fwd_oracle(v, Vn, B).astype(np.float32)), seed
            assert np.array_equal(G.cpu().numpy(), sddmm_oracle(v, X, B).astype(np.float32)), seed
            assert np.array_equal(dB.cpu().numpy().reshape(n, v.cols).T, oracle(v, Vn, X).astype(np.float32)), seed
    H.close()


def test_spmm_t_refusals(mats):
    v = mats["jaccard"]
    n = 16
    t = tall_groups()
    handles = {
        "plain": v.to_device(0),
        "updatable": v.to_device(0, updatable=True),
        "from_csr": sa.DeviceVBS.from_csr(t, sa.BlockingEngine(tau=0.6, col_block_size=32).GetGrouping(t), 32, device=0),
        "transposed": sa.DeviceVBS.transposed_of(v, device=0),
    }
    for name, d in handles.items():
        assert not d.transposable, name
        X = torch.zeros(d.rows * n, dtype=torch.float32, device="cuda")
        Ct = torch.zeros(d.cols * n, dtype=torch.float32, device="cuda")
        with pytest.raises(sa.SpartaError) as e:
            d.spmm_t(X, Ct, n)
        assert e.value.code == sa._lib.ERR_UNSUPPORTED, name
        assert "SPARTA_CREATE_TRANSPOSE" in str(e.value), name
        with pytest.raises(sa.SpartaError) as e:
            d.spmm_t_host(np.zeros(d.rows * n, np.float32), n, np.zeros(d.cols * n, np.float32))
        assert e.value.code == sa._lib.ERR_UNSUPPORTED, name
    # ... and every one of them still multiplies
    B = dense_b(v, n, 90, integer=True)
    Bf = np.ascontiguousarray(B.T, np.float32).ravel()
    ref = fwd_oracle(v, v.mab, B)
    bound = fwd_oracle(v, np.abs(v.mab), np.abs(B))
    for name in ("plain", "updatable", "from_csr"):
        C = np.zeros(v.rows * n, np.float32)
        handles[name].spmm_host(Bf, n, C, accumulate=False)
        assert np.all(np.abs(C.reshape(n, v.rows).T - ref) <= 1e-5 * bound + 1e-30), name
    M = 8
    Bl = np.random.default_rng(91).integers(-4, 5, (M, v.rows)).astype(np.float64)
    Cba = np.zeros(M * v.cols, np.float32)
    handles["transposed"].spmm_BA_host(np.ascontiguousarray(Bl.T, np.float32).ravel(), M, Cba, accumulate=False)
    At = fwd_oracle(v, v.mab, np.eye(v.cols))
    assert np.all(np.abs(Cba.reshape(v.cols, M).T - Bl @ At) <= 1e-5 * (np.abs(Bl) @ np.abs(At)) + 1e-30)
    for h in handles.values():
        h.close()
    with pytest.raises(sa.SpartaError) as e:
        _create_with_flags(v, 4)                                       # (an unknown bit, through the C entry)
    assert e.value.code == sa._lib.ERR_INVALID
    d = v.to_device(0, transposable=True)
    X = torch.zeros((v.rows + 8) * n, dtype=torch.float32, device="cuda")
    Ct = torch.zeros((v.cols + 8) * n, dtype=torch.float32, device="cuda")
    for kw in (dict(ldo=v.cols - 1), dict(ldx=v.rows - 1)):
        with pytest.raises(sa.SpartaError) as e:
            _raw_spmm_t(d, X, Ct, n, **kw)
        assert e.value.code == sa._lib.ERR_INVALID, kw
    for bad_n in (0, -3):
        with pytest.raises(sa.SpartaError) as e:
            _raw_spmm_t(d, X, Ct, bad_n)
        assert e.value.code == sa._lib.ERR_INVALID, bad_n
    d.close()
    d16 = v.to_device(0, dtype=sa.F16, transposable=True)
    with pytest.raises(sa.SpartaError) as e:
        _raw_spmm_t(d16, X.half(), Ct, n, ldx=v.rows + 1)
    assert e.value.code == sa._lib.ERR_INVALID and "even" in str(e.value)
    d16.close()


def _raw_spmm_t(d, X, Ct, n, ldx=None, ldo=None):
    """the C entry without the Python wrapper's own argument checks"""
    import ctypes as C
    from sparta_amd._lib import lib, check
    st = torch.cuda.current_stream(0).cuda_stream
    check(lib.sparta_vbs_spmm_t(d.h, C.c_void_p(X.data_ptr()), d.rows if ldx is None else ldx, n, C.cast(C.c_void_p(Ct.data_ptr()), C.POINTER(C.c_float)),
                                d.cols if ldo is None else ldo, 0, sa._lib.PTR_DEVICE, C.c_void_p(st), None))


def _create_with_flags(v, flags):
    import ctypes as C
    from sparta_amd._lib import lib, check
    i64p, f32p = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    rp, nz, jab = (np.ascontiguousarray(a, np.int64) for a in (v.row_part, v.nzcount, v.jab))
    mab = np.ascontiguousarray(v.mab, np.float32)
    h = C.c_void_p(None)
    check(lib.sparta_vbs_create_range_ex(C.byref(h), v.rows, v.cols, v.block_rows, v.block_col_size, rp.ctypes.data_as(i64p), nz.ctypes.data_as(i64p),
                                         jab.ctypes.data_as(i64p), mab.ctypes.data_as(f32p), 0, v.block_rows, sa.F32, 0, flags))
    lib.sparta_vbs_destroy(h)


# info() and sparse_info() of DeviceVBS(v, updatable=True) -- flags = 1 -- as the commit BEFORE this feature reported them on an MI355X (read from a run of that
# commit's library on these matrices, the method tests/test_set_values_gpu.py describes; last_path is 0 before any product)
PARENT_INFO_UPDATABLE = {
    ('grid1', 0): ({'a_bytes': 377808, 'block_col_size': 1, 'block_rows': 19, 'cols': 517, 'exec_area': 95376, 'last_path': 0, 'nblocks': 5961, 'nztot': 94324, 'rows': 300, 'sparse_rows': 0, 'split_tiles': 0, 'stream_steps': 0, 'stream_workers': 0, 'tiles16': 19, 'tiles32': 0, 'tiles64': 0},
        {'hub_rows': 0, 'nnz': 0, 'rows': 0, 'short_rows': 0}),
    ('grid8', 0): ({'a_bytes': 624000, 'block_col_size': 8, 'block_rows': 19, 'cols': 517, 'exec_area': 157952, 'last_path': 0, 'nblocks': 1234, 'nztot': 155872, 'rows': 300, 'sparse_rows': 0, 'split_tiles': 0, 'stream_steps': 0, 'stream_workers': 0, 'tiles16': 19, 'tiles32': 0, 'tiles64': 0},
        {'hub_rows': 0, 'nnz': 0, 'rows': 0, 'short_rows': 0}),
    ('grid32', 0): ({'a_bytes': 2013632, 'block_col_size': 32, 'block_rows': 19, 'cols': 517, 'exec_area': 165376, 'last_path': 0, 'nblocks': 323, 'nztot': 163200, 'rows': 300, 'sparse_rows': 0, 'split_tiles': 19, 'stream_steps': 323, 'stream_workers': 512, 'tiles16': 19, 'tiles32': 0, 'tiles64': 0},
        {'hub_rows': 0, 'nnz': 0, 'rows': 0, 'short_rows': 0}),
    ('grid32', 1): ({'a_bytes': 727040, 'block_col_size': 32, 'block_rows': 19, 'cols': 517, 'exec_area': 165376, 'last_path': 0, 'nblocks': 323, 'nztot': 163200, 'rows': 300, 'sparse_rows': 0, 'split_tiles': 19, 'stream_steps': 323, 'stream_workers': 256, 'tiles16': 19, 'tiles32': 0, 'tiles64': 0},
        {'hub_rows': 0, 'nnz': 0, 'rows': 0, 'short_rows': 0}),
    ('grid64', 0): ({'a_bytes': 2131072, 'block_col_size': 64, 'block_rows': 19, 'cols': 517, 'exec_area': 175104, 'last_path': 0, 'nblocks': 171, 'nztot': 172800, 'rows': 300, 'sparse_rows': 0, 'split_tiles': 19, 'stream_steps': 342, 'stream_workers': 512, 'tiles16': 19, 'tiles32': 0, 'tiles64': 0},
        {'hub_rows': 0, 'nnz': 0, 'rows': 0, 'short_rows': 0}),
    ('hub', 1): ({'a_bytes': 1114112, 'block_col_size': 64, 'block_rows': 8, 'cols': 1000, 'exec_area': 524288, 'last_path': 0, 'nblocks': 128, 'nztot': 393216, 'rows': 384, 'sparse_rows': 0, 'split_tiles': 8, 'stream_steps': 128, 'stream_workers': 256, 'tiles16': 0, 'tiles32': 0, 'tiles64': 8},
        {'hub_rows': 0, 'nnz': 0, 'rows': 0, 'short_rows': 0}),
    ('jaccard', 0): ({'a_bytes': 307712, 'block_col_size': 32, 'block_rows': 3, 'cols': 700, 'exec_area': 98304, 'last_path': 0, 'nblocks': 24, 'nztot': 76800, 'rows': 300, 'sparse_rows': 0, 'split_tiles': 6, 'stream_steps': 48, 'stream_workers': 512, 'tiles16': 0, 'tiles32': 0, 'tiles64': 6},
        {'hub_rows': 0, 'nnz': 0, 'rows': 0, 'short_rows': 0}),
    ('jaccard', 1): ({'a_bytes': 262144, 'block_col_size': 32, 'block_rows': 3, 'cols': 700, 'exec_area': 98304, 'last_path': 0, 'nblocks': 24, 'nztot': 76800, 'rows': 300, 'sparse_rows': 0, 'split_tiles': 0, 'stream_steps': 48, 'stream_workers': 256, 'tiles16': 0, 'tiles32': 0, 'tiles64': 6},
        {'hub_rows': 0, 'nnz': 0, 'rows': 0, 'short_rows': 0}),
    ('padded', 0): ({'a_bytes': 215296, 'block_col_size': 32, 'block_rows': 6, 'cols': 192, 'exec_area': 24576, 'last_path': 0, 'nblocks': 24, 'nztot': 24576, 'rows': 192, 'sparse_rows': 0, 'split_tiles': 0, 'stream_steps': 24, 'stream_workers': 512, 'tiles16': 0, 'tiles32': 6, 'tiles64': 0},
        {'hub_rows': 0, 'nnz': 0, 'rows': 0, 'short_rows': 0}),
    ('padded', 1): ({'a_bytes': 122880, 'block_col_size': 32, 'block_rows': 6, 'cols': 192, 'exec_area': 24576, 'last_path': 0, 'nblocks': 24, 'nztot': 24576, 'rows': 192, 'sparse_rows': 0, 'split_tiles': 0, 'stream_steps': 14, 'stream_workers': 256, 'tiles16': 0, 'tiles32': 6, 'tiles64': 0},
        {'hub_rows': 0, 'nnz': 0, 'rows': 0, 'short_rows': 0}),
    ('pairs', 0): ({'a_bytes': 606016, 'block_col_size': 32, 'block_rows': 6, 'cols': 517, 'exec_area': 74752, 'last_path': 0, 'nblocks': 73, 'nztot': 71296, 'rows': 180, 'sparse_rows': 0, 'split_tiles': 6, 'stream_steps': 73, 'stream_workers': 512, 'tiles16': 0, 'tiles32': 6, 'tiles64': 0},
        {'hub_rows': 0, 'nnz': 0, 'rows': 0, 'short_rows': 0}),
    ('pairs', 1): ({'a_bytes': 253952, 'block_col_size': 32, 'block_rows': 6, 'cols': 517, 'exec_area': 74752, 'last_path': 0, 'nblocks': 73, 'nztot': 71296, 'rows': 180, 'sparse_rows': 0, 'split_tiles': 3, 'stream_steps': 46, 'stream_workers': 256, 'tiles16': 0, 'tiles32': 6, 'tiles64': 0},
        {'hub_rows': 0, 'nnz': 0, 'rows': 0, 'short_rows': 0}),
}


@pytest.mark.parametrize("key,dtype", sorted(PARENT_INFO_UPDATABLE), ids=["%s-%d" % kd for kd in sorted(PARENT_INFO_UPDATABLE)])
def test_updatable_creation_is_unchanged(mats, key, dtype):
    d = mats[key].to_device(0, dtype=dtype, updatable=True)
    info, sparse = PARENT_INFO_UPDATABLE[(key, dtype)]
    assert d.info() == info
    assert d.sparse_info() == sparse
    assert d.updatable and not d.transposable
    d.close()


@pytest.mark.parametrize("dtype", [sa.F32, sa.F16], ids=["f32", "f16"])
def test_forward_of_a_transposable_handle_has_the_bits_of_a_plain_one(mats, dtype):
    for key in ("grid32", "jaccard"):
        v = mats[key]
        P = v.to_device(0, dtype=dtype)
        T = v.to_device(0, dtype=dtype, transposable=True)
        assert P.sparse_info() == T.sparse_info()
        ip, it = P.info(), T.info()
        assert {k: x for k, x in ip.items() if k != "a_bytes"} == {k: x for k, x in it.items() if k != "a_bytes"}
        if dtype != sa.F32:
            assert it["a_bytes"] - ip["a_bytes"] == 2 * sum(-(-int(h) // 8) * 8 * v.block_col_size * int(nb) for h, nb in zip(np.diff(v.row_part), v.nzcount))
        B = dense_b(v, 128, 70, integer=False)
        a, _ = product(P, v, B, dtype)
        b, _ = product(T, v, B, dtype)
        assert np.array_equal(a, b), key
        P.close(); T.close()


def dense_and_mask(v, mab):
    """A (rows x cols, float64) and, per stored position of mab, its (row, column) or column -1 past cols"""
    w = v.block_col_size
    A = fwd_oracle(v, mab, np.eye(v.cols))
    rr, cc = np.zeros(int(v.nztot), np.int64), np.zeros(int(v.nztot), np.int64)
    jo = mo = 0
    for ib in range(v.block_rows):
        r0, h, nb = int(v.row_part[ib]), int(v.row_part[ib + 1] - v.row_part[ib]), int(v.nzcount[ib])
        for b in range(nb):
            c = int(v.jab[jo + b]) * w + np.repeat(np.arange(w), h)
            rr[mo + b * w * h: mo + (b + 1) * w * h] = r0 + np.tile(np.arange(h), w)
            cc[mo + b * w * h: mo + (b + 1) * w * h] = np.where(c < v.cols, c, -1)
        jo += nb
        mo += nb * h * w
    return A, rr, cc


@pytest.mark.parametrize("key,dtype", [("grid32", sa.F32), ("jaccard", sa.F16)], ids=["grid32-f32", "jaccard-f16"])
def test_vbs_linear_against_torch(mats, key, dtype):
    """the 300 x 517 matrix (fp32; a 16-bit handle takes its operands with an even leading dimension, so the f16 case runs on the 300 x 700 one): y, grad_x,
    grad_values against torch.nn.functional.linear with the dense A (reordered rows) in float64; two SGD steps in a row"""
    from sparta_amd.autograd import vbs_linear
    v = mats[key]
    tdt = TDT[dtype]
    H = v.to_device(0, dtype=dtype, updatable=True, transposable=True)
    n = 24

    for integer in (True, False):
        V = values(v, 30 + integer, integer=integer)
        W = torch.from_numpy(V).cuda().requires_grad_(True)
        x64 = dense_b(v, n, 31, integer=integer).T.copy()              # (n, cols)
        x = torch.from_numpy(x64).cuda().to(tdt).requires_grad_(True)
        gy64 = dense_x(v.rows, n, 32, integer=integer).T.copy()        # (n, rows)
        gy = torch.from_numpy(gy64).cuda().float()
        y = vbs_linear(x, H, W)
        y.backward(gy)
        torch.cuda.synchronize()
        A, rr, cc = dense_and_mask(v, rounded(V, dtype))
        xr = x.detach().double().cpu()
        gyr = gy.to(tdt).double().cpu()
        At = torch.from_numpy(A).requires_grad_(True)
        xt = xr.clone().requires_grad_(True)
        yt = torch.nn.functional.linear(xt, At)
        yt.backward(gyr)
        absA, absx, absg = np.abs(A), np.abs(xr.numpy()), np.abs(gyr.numpy())
        gv_ref = np.where(cc >= 0, At.grad.numpy()[rr, np.maximum(cc, 0)], 0.0)
        gv_bound = np.where(cc >= 0, (absg.T @ absx)[rr, np.maximum(cc, 0)], 0.0)
        got_y, got_gx, got_gv = y.detach().cpu().numpy(), x.grad.float().cpu().numpy(), W.grad.cpu().numpy()
        if integer:
            assert np.array_equal(got_y, yt.detach().numpy().astype(np.float32))
            assert np.array_equal(got_gx, xt.grad.numpy().astype(np.float32))
            assert np.array_equal(got_gv, gv_ref.astype(np.float32))
        else:
            assert np.all(np.abs(got_y - yt.detach().numpy()) <= 1e-5 * (absx @ absA.T) + 1e-30)
            if dtype == sa.F32:                                        # (a 16-bit grad_x is rounded to x.dtype on return: compared through that rounding)
                assert np.all(np.abs(got_gx - xt.grad.numpy()) <= 1e-5 * (absg @ absA) + 1e-30)
            else:
                lo = torch.from_numpy(xt.grad.numpy() - 1e-5 * (absg @ absA)).to(tdt).float().numpy()
                hi = torch.from_numpy(xt.grad.numpy() + 1e-5 * (absg @ absA)).to(tdt).float().numpy()
                assert np.all((got_gx >= lo) & (got_gx <= hi))
            assert np.all(np.abs(got_gv - gv_ref) <= 1e-5 * gv_bound + 1e-30)

    # two SGD steps in a row on integers: the second forward sees the updated values without any host copy
    V = values(v, 40, integer=True)
    W = torch.from_numpy(V).cuda().requires_grad_(True)
    x64 = dense_b(v, 8, 41, integer=True).T.copy()
    x = torch.from_numpy(x64).cuda().to(tdt)
    cur = V.astype(np.float64)
    for step in range(2):
        y = vbs_linear(x, H, W)
        A, rr, cc = dense_and_mask(v, cur)
        assert np.array_equal(y.detach().cpu().numpy(), (x64 @ A.T).astype(np.float32)), step
        gy64 = np.sign(dense_x(v.rows, 8, 42 + step, integer=True).T)            # entries -1, 0, 1: the updated values stay small integers
        y.backward(torch.from_numpy(gy64).cuda().float())
        with torch.no_grad():
            W -= W.grad
            W.grad = None
        g = np.where(cc >= 0, (gy64.T @ x64)[rr, np.maximum(cc, 0)], 0.0)
        cur = cur - g
        assert np.array_equal(W.detach().cpu().numpy(), cur.astype(np.float32)), step
    H.close()


def test_vbs_linear_needs_both_flags(mats):
    from sparta_amd.autograd import vbs_linear
    v = mats["padded"]
    x = torch.zeros((4, v.cols), dtype=torch.float32, device="cuda")
    W = torch.zeros(int(v.nztot), dtype=torch.float32, device="cuda")
    for kw in (dict(), dict(updatable=True), dict(transposable=True)):
        d = v.to_device(0, **kw)
        with pytest.raises(ValueError):
            vbs_linear(x, d, W)
        d.close()
