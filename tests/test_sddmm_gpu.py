"""sparta_vbs_sddmm on the GPU (k_sddmm.hip): G (+)= (X * Y^T) sampled on the stored blocks of a VBS handle, in the mab layout.

Oracle: a float64 numpy restatement -- per block-row and block, X[r0:r0+h] @ Y[jb*w : jb*w+w].T, ragged columns 0, flattened column-major at a_off.
Small-integer X, Y are exact in every dtype and must match bit for bit; random data within 1e-5 * sum|x||y| (16-bit handles: against the oracle on
the rounded inputs)."""
import numpy as np
import pytest

import sparta_amd as sa

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

TDT = {sa.F32: torch.float32, sa.F16: torch.float16, sa.BF16: torch.bfloat16}


def oracle(v, X, Y, absolute=False):
    """X: rows x k, Y: cols x k (float64, 2-D); G in the layout of v.mab"""
    if absolute:
        X, Y = np.abs(X), np.abs(Y)
    w = v.block_col_size
    G = np.zeros(int(v.nztot), np.float64)
    jo = mo = 0
    for ib in range(v.block_rows):
        r0, r1 = int(v.row_part[ib]), int(v.row_part[ib + 1])
        h, nb = r1 - r0, int(v.nzcount[ib])
        for b in range(nb):
            c0 = int(v.jab[jo + b]) * w
            c1 = min(c0 + w, v.cols)
            blk = np.zeros((h, w))
            blk[:, :c1 - c0] = X[r0:r1] @ Y[c0:c1].T
            G[mo + b * w * h: mo + (b + 1) * w * h] = blk.ravel(order="F")
        jo += nb
        mo += nb * h * w
    return G


def vbr_of(m, g, w, rbs=0, ff=False):
    return sa.VBR().fill_from_CSR_inplace(m, g, w, rbs, ff)


def tall_groups():
    """3 clusters of 100 rows with one column pattern each, rows scattered: the Jaccard grouping makes block-rows of height 100"""
    rng = np.random.default_rng(3)
    n, cols = 300, 700
    order = rng.permutation(n)
    rr, cc = [], []
    for gi in range(3):
        pat = np.sort(gi * 230 + rng.choice(230, 60, replace=False))       # (each cluster in its own column blocks)
        for r in order[gi * 100:(gi + 1) * 100]:
            rr.append(np.full(len(pat), r)); cc.append(pat)
    r, c = np.concatenate(rr), np.concatenate(cc)
    o = np.lexsort((c, r))
    r, c = r[o], c[o]
    rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int64)
    return sa.CSR(n, cols, rp, c.astype(np.int32), rng.uniform(-1, 1, len(c)).astype(np.float32))


def build_mats():
    out = {}
    m = sa.gen.uniform_random(300, 517, 9000, seed=41)             # 517 columns: a ragged last block column for every w below
    g = np.arange(m.rows, dtype=np.int64) // 16
    for w in (1, 8, 32, 64):
        out["grid%d" % w] = vbr_of(m, g, w)
    t = tall_groups()
    v = vbr_of(t, sa.BlockingEngine(tau=0.6, col_block_size=32).GetGrouping(t), 32)
    assert np.diff(v.row_part).max() > 64
    out["jaccard"] = v
    f = sa.gen.fem3d(3, 3, 7, 3, seed=9)
    eng = sa.BlockingEngine(blocking_algo=5, tau=0.6, col_block_size=32, row_block_size=32, force_fixed_size=True)
    v = vbr_of(f, eng.GetGrouping(f), 32, 32, True)
    assert v.rows > f.rows                                          # padding rows
    out["padded"] = v
    return out


@pytest.fixture(scope="module")
def mats():
    return build_mats()


_handles = {}


def handle(v, key, dtype):
    if (key, dtype) not in _handles:
        _handles[(key, dtype)] = v.to_device(0, dtype=dtype)
    return _handles[(key, dtype)]


def operands(v, k, seed, integer):
    rng = np.random.default_rng(seed)
    if integer:
        return rng.integers(-4, 5, (v.rows, k)).astype(np.float64), rng.integers(-4, 5, (v.cols, k)).astype(np.float64)
    return rng.uniform(-1, 1, (v.rows, k)), rng.uniform(-1, 1, (v.cols, k))


def colmajor(A, dtype, ld):
    """2-D float64 -> column-major device tensor of the handle's type with leading dimension ld (padding NaN: never read)"""
    t = torch.full((A.shape[1], ld), float("nan"), dtype=torch.float64)
    t[:, :A.shape[0]] = torch.from_numpy(np.ascontiguousarray(A.T))
    return t.cuda().to(TDT[dtype]).reshape(-1)


def run(d, X, Y, dtype, G=None, accumulate=False, ld_mult=8):
    """X, Y float64 2-D -> column-major device tensors of the handle's type (leading dimensions padded to a multiple of ld_mult); returns
    (G on the host, X and Y as rounded, float64)"""
    k = X.shape[1]
    ldx, ldy = -(-X.shape[0] // ld_mult) * ld_mult, -(-Y.shape[0] // ld_mult) * ld_mult
    Xt, Yt = colmajor(X, dtype, ldx), colmajor(Y, dtype, ldy)
    nz = d.info()["nztot"]
    Gt = torch.full((nz,), float("nan"), dtype=torch.float32, device="cuda") if G is None else torch.from_numpy(G.astype(np.float32)).cuda()
    d.sddmm(Xt, Yt, Gt, k, accumulate=accumulate, ldx=ldx, ldy=ldy)
    torch.cuda.synchronize()
    Xr = Xt.float().cpu().numpy().astype(np.float64).reshape(k, ldx)[:, :X.shape[0]].T
    Yr = Yt.float().cpu().numpy().astype(np.float64).reshape(k, ldy)[:, :Y.shape[0]].T
    return Gt.cpu().numpy(), Xr, Yr


def check_close(v, G, Xr, Yr):
    ref, bound = oracle(v, Xr, Yr), oracle(v, Xr, Yr, absolute=True)
    assert not np.isnan(G).any()
    err = np.abs(G - ref)
    assert np.all(err <= 1e-5 * bound + 1e-30), float((err - 1e-5 * bound).max())


@pytest.mark.parametrize("key", ["grid1", "grid8", "grid32", "grid64", "jaccard", "padded"])
@pytest.mark.parametrize("k", [1, 5, 128, 200])
def test_sddmm_f32_integer_bit_exact(mats, key, k):
    v = mats[key]
    X, Y = operands(v, k, seed=k, integer=True)
    G, _, _ = run(handle(v, key, sa.F32), X, Y, sa.F32)
    assert np.array_equal(G, oracle(v, X, Y).astype(np.float32))


@pytest.mark.parametrize("key", ["grid8", "grid32", "jaccard", "padded"])
def test_sddmm_f32_random_tolerance(mats, key):
    v = mats[key]
    X, Y = operands(v, 130, seed=1, integer=False)
    G, Xr, Yr = run(handle(v, key, sa.F32), X, Y, sa.F32)
    check_close(v, G, Xr, Yr)


@pytest.mark.parametrize("dtype", [sa.F16, sa.BF16])
@pytest.mark.parametrize("key", ["grid32", "grid64", "jaccard"])           # (16-bit handles need w % 32 == 0)
@pytest.mark.parametrize("k", [8, 128, 130])
def test_sddmm_h16(mats, dtype, key, k):
    v = mats[key]
    d = handle(v, key, dtype)
    ld_mult = 2 if k == 130 else 8                   # (k = 130: ldy = cols rounded up to even, not a multiple of 8 -> Y gathered column by column, not 8 columns per load)
    X, Y = operands(v, k, seed=k + 7, integer=True)
    G, _, _ = run(d, X, Y, dtype, ld_mult=ld_mult)
    assert np.array_equal(G, oracle(v, X, Y).astype(np.float32))
    X, Y = operands(v, k, seed=k + 8, integer=False)
    G, Xr, Yr = run(d, X, Y, dtype, ld_mult=ld_mult)
    check_close(v, G, Xr, Yr)


@pytest.mark.parametrize("dtype", [sa.F32, sa.BF16])
def test_sddmm_accumulate_adds(mats, dtype):
    v = mats["grid32"]
    d = handle(v, "grid32", dtype)
    X, Y = operands(v, 40, seed=2, integer=True)
    G0 = np.random.default_rng(5).integers(-50, 50, int(v.nztot)).astype(np.float32)
    G, _, _ = run(d, X, Y, dtype, G=G0, accumulate=True)
    assert np.array_equal(G, (G0 + oracle(v, X, Y)).astype(np.float32))


def test_sddmm_range_handle_is_slice(mats):
    v = mats["jaccard"]
    full = handle(v, "jaccard", sa.F32)
    X, Y = operands(v, 64, seed=3, integer=False)
    Gf, _, _ = run(full, X, Y, sa.F32)
    b0, b1 = 1, v.block_rows
    part = v.to_device(0, block_row_range=(b0, b1))
    r0 = int(v.row_part[b0])
    a0 = int(sum(int(v.nzcount[i]) * (int(v.row_part[i + 1]) - int(v.row_part[i])) for i in range(b0))) * v.block_col_size
    Gp, _, _ = run(part, X[r0:], Y, sa.F32)
    assert Gp.size == v.nztot - a0
    assert np.array_equal(Gp, Gf[a0:])


@pytest.mark.parametrize("dtype", [sa.F32, sa.F16])
def test_sddmm_host_pointers_match_device(mats, dtype):
    v = mats["grid32"]
    d = handle(v, "grid32", dtype)
    X, Y = operands(v, 33, seed=4, integer=False)
    Gd, _, _ = run(d, X, Y, dtype)
    Gh = np.full(int(v.nztot), 7.0, np.float32)
    ms = d.sddmm_host(X.T.astype(np.float32).ravel(), Y.T.astype(np.float32).ravel(), 33, Gh, accumulate=False)
    assert ms > 0
    assert np.array_equal(Gh, Gd)
    if dtype == sa.F32:                                 # the VBR entry: accumulates into G in the layout of mab
        G2 = v.sddmm(X.T.astype(np.float32).ravel(), Y.T.astype(np.float32).ravel(), 33)
        assert np.array_equal(G2, Gd)


def test_sddmm_is_the_gradient_of_the_product(mats):
    """sum(G * mab) = <dC, A B> for X = dC, Y = B, with the library's own spmm"""
    v = mats["jaccard"]
    d = handle(v, "jaccard", sa.F32)
    n = 48
    rng = np.random.default_rng(6)
    B = rng.uniform(-1, 1, (v.cols, n))
    dC = rng.uniform(-1, 1, (v.rows, n))
    Bt = torch.from_numpy(np.ascontiguousarray(B.T, np.float32)).cuda().reshape(-1)
    Ct = torch.zeros(v.rows * n, dtype=torch.float32, device="cuda")
    d.spmm(Bt, Ct, n)
    G, _, _ = run(d, dC, B, sa.F32)
    C = Ct.cpu().numpy().astype(np.float64).reshape(n, v.rows).T
    lhs = float(np.dot(G.astype(np.float64), v.mab.astype(np.float64)))
    rhs = float(np.sum(dC * C))
    scale = float(np.dot(oracle(v, np.abs(dC), np.abs(B)), np.abs(v.mab.astype(np.float64))))
    assert abs(lhs - rhs) <= 1e-5 * scale


def test_sddmm_leaves_spmm_alone(mats):
    v = mats["grid64"]
    d = handle(v, "grid64", sa.F32)
    n = 128
    Bt = torch.from_numpy(sa.gen.dense_rhs(v.cols, n, seed=8)).cuda()
    C1 = torch.zeros(v.rows * n, dtype=torch.float32, device="cuda")
    C2 = torch.zeros_like(C1)
    d.spmm(Bt, C1, n)
    X, Y = operands(v, 16, seed=9, integer=False)
    run(d, X, Y, sa.F32)
    run(d, X, Y, sa.F32, G=np.ones(int(v.nztot)), accumulate=True)
    d.spmm(Bt, C2, n)
    torch.cuda.synchronize()
    assert torch.equal(C1, C2)


def test_sddmm_graph_capture(mats):
    v = mats["padded"]
    d = v.to_device(0)                                   # fresh handle: the first call builds the work list
    k = 24
    X, Y = operands(v, k, seed=10, integer=False)
    Xt = torch.from_numpy(np.ascontiguousarray(X.T, np.float32)).cuda().reshape(-1)
    Yt = torch.from_numpy(np.ascontiguousarray(Y.T, np.float32)).cuda().reshape(-1)
    nz = d.info()["nztot"]
    G_eager = torch.zeros(nz, dtype=torch.float32, device="cuda")
    G_graph = torch.full((nz,), float("nan"), dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d.sddmm(Xt, Yt, G_eager, k)                      # once outside a capture
        torch.cuda.synchronize()
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph, stream=s):
            d.sddmm(Xt, Yt, G_graph, k)
        gph.replay()
    torch.cuda.synchronize()
    assert torch.equal(G_eager, G_graph)


def test_sddmm_refusals(mats):
    v = mats["grid32"]
    t = tall_groups()
    dc = sa.DeviceVBS.from_csr(t, sa.BlockingEngine(tau=0.6, col_block_size=32).GetGrouping(t), 32, device=0)
    X = torch.zeros(t.rows * 4, dtype=torch.float32, device="cuda")
    Y = torch.zeros(t.cols * 4, dtype=torch.float32, device="cuda")
    G = torch.zeros(max(dc.info()["nztot"], 1), dtype=torch.float32, device="cuda")
    with pytest.raises(sa.SpartaError) as e:
        dc.sddmm(X, Y, G, 4)
    assert e.value.code == sa._lib.ERR_UNSUPPORTED
    d = handle(v, "grid32", sa.F32)
    Xg = torch.zeros(v.rows * 4, dtype=torch.float32, device="cuda")
    Yg = torch.zeros(v.cols * 4, dtype=torch.float32, device="cuda")
    Gg = torch.zeros(int(v.nztot), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        d.sddmm(Xg.half(), Yg.half(), Gg, 4)                         # wrong dtype
    with pytest.raises(ValueError):
        d.sddmm(Xg[:-1], Yg, Gg, 4)                                  # X too small
    with pytest.raises(ValueError):
        d.sddmm(Xg, Yg, Gg[:-1], 4)                                  # G too small
