"""sparta_vbs_set_values on the GPU (k_update.hip): new values for the stored blocks of an updatable handle, same block pattern.

After set_values(V) every product of the handle must be what a handle created from V computes:
  * fp32, SPARTA_SPMM_EXACT (fixed summation order): bit for bit the product of a fresh handle;
  * SPARTA_SPMM_MFMA on small integers (|v| <= 4: every partial sum is exact in fp32, every value exact in f16 / bf16): bit for bit the float64 oracle;
  * SPARTA_SPMM_MFMA on random real data: |C - oracle| <= 1e-5 * sum|a||b| (16-bit handles: the oracle on inputs rounded with torch .to(dtype).float()).
The value sets differ in their ZERO PATTERN inside the blocks (whole columns of blocks empty in one set and filled in the next, whole blocks zero and
back): the fp32 fragment image compacts the non-empty columns of every step, so a plain overwrite of the values would give wrong products."""
import numpy as np
import pytest

import sparta_amd as sa

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

TDT = {sa.F32: torch.float32, sa.F16: torch.float16, sa.BF16: torch.bfloat16}
DT_ID = {sa.F32: "f32", sa.F16: "f16", sa.BF16: "bf16"}


# ---- matrices (the shapes of tests/test_sddmm_gpu.py, copied) + a hub matrix + a pair-tile matrix -----------------------------------------
def vbr_of(m, g, w, rbs=0, ff=False):
    return sa.VBR().fill_from_CSR_inplace(m, g, w, rbs, ff)


def tall_groups():
    """3 clusters of 100 rows with one column pattern each, rows scattered: the Jaccard grouping makes block-rows of height 100"""
    rng = np.random.default_rng(3)
    n, cols = 300, 700
    order = rng.permutation(n)
    rr, cc = [], []
    for gi in range(3):
        pat = np.sort(gi * 230 + rng.choice(230, 60, replace=False))
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
    assert v.rows > f.rows                                          # padding rows; 32-row block-rows: 16-bit handles walk them as pair tiles
    out["padded"] = v
    # pair tiles with a short last block-row (32, 32, 32, 32, 32, 20 rows) and few blocks per block-row: block columns present in one half of a pair only
    p = sa.gen.uniform_random(180, 517, 150, seed=43)
    v = vbr_of(p, np.arange(p.rows, dtype=np.int64) // 32, 32)
    hts = np.diff(v.row_part)
    assert hts[-1] == 20 and np.all(v.nzcount > 0)
    jo = np.concatenate([[0], np.cumsum(v.nzcount)])
    assert set(v.jab[jo[4]:jo[5]]) != set(v.jab[jo[5]:jo[6]])
    out["pairs"] = v
    # 16-bit hub plan: block-rows of 48 rows (33..64), w = 64, every block-row owns (nearly) every block column
    hm = sa.gen.uniform_random(384, 1000, 30000, seed=44)
    out["hub"] = vbr_of(hm, np.arange(hm.rows, dtype=np.int64) // 48, 64)
    return out


@pytest.fixture(scope="module")
def mats():
    return build_mats()


# ---- value sets ---------------------------------------------------------------------------------------------------------------------------
def blocks_of(v, b0=0, b1=None):
    """(offset into mab, h, block-column id) of every stored block of block-rows [b0, b1), offsets from the range's first element"""
    w = v.block_col_size
    out = []
    jo = mo = 0
    for ib in range(v.block_rows if b1 is None else b1):
        h, nb = int(v.row_part[ib + 1] - v.row_part[ib]), int(v.nzcount[ib])
        if ib >= b0:
            for b in range(nb):
                out.append((mo + b * w * h, h, int(v.jab[jo + b])))
        else:
            mo -= nb * h * w
        jo += nb
        mo += nb * h * w
    return out


def values(v, seed, integer):
    """nztot new values with their own zero pattern: ~half the elements zero, ~30 % of the columns of every block entirely zero, every fifth block (which
    ones depends on the seed) entirely zero; the positions past `cols` of a ragged last block column get values too (stored as given, never multiplied)"""
    rng = np.random.default_rng(seed)
    w = v.block_col_size
    n = int(v.nztot)
    x = rng.integers(-4, 5, n).astype(np.float32) if integer else rng.uniform(-1, 1, n).astype(np.float32)
    x[rng.random(n) < 0.5] = 0.0
    for q, (off, h, _) in enumerate(blocks_of(v)):
        blk = x[off:off + h * w].reshape(w, h)                       # column-major h x w: row c of this view = column c of the block
        blk[rng.random(w) < 0.3, :] = 0.0
        if (q + seed) % 5 == 0:
            blk[:, :] = 0.0
    return x


def column_masks(v, x):
    """per block and 32-deep column: has the column a non-zero (any row)"""
    w = v.block_col_size
    return np.concatenate([(x[off:off + h * w].reshape(w, h) != 0).any(axis=1) for off, h, _ in blocks_of(v)])


def oracle(v, mab, B, b0=0, b1=None):
    """float64 C = A * B for the values `mab` on the pattern of v (block-rows [b0, b1)); B: cols x n (2-D).  Returns rows x n."""
    w = v.block_col_size
    r_lo = int(v.row_part[b0])
    r_hi = int(v.row_part[v.block_rows if b1 is None else b1])
    C = np.zeros((r_hi - r_lo, B.shape[1]))
    a = np.asarray(mab, np.float64)
    Bd = np.asarray(B, np.float64)
    jo = sum(int(v.nzcount[i]) for i in range(b0))
    mo = 0
    for ib in range(b0, v.block_rows if b1 is None else b1):
        r0, h, nb = int(v.row_part[ib]) - r_lo, int(v.row_part[ib + 1] - v.row_part[ib]), int(v.nzcount[ib])
        for b in range(nb):
            c0 = int(v.jab[jo + b]) * w
            c1 = min(c0 + w, v.cols)
            blk = a[mo + b * w * h: mo + (b + 1) * w * h].reshape(w, h).T
            C[r0:r0 + h] += blk[:, :c1 - c0] @ Bd[c0:c1]
        jo += nb
        mo += nb * h * w
    return C


def dense_b(v, n, seed, integer):
    rng = np.random.default_rng(seed)
    return rng.integers(-4, 5, (v.cols, n)).astype(np.float64) if integer else rng.uniform(-1, 1, (v.cols, n))


def product(d, v, B, dtype, row_major=False, algo=sa.SPMM_MFMA, rows=None):
    """C = A * B through the handle: B float64 cols x n -> device tensor in the handle's type (column-major, ld even; or row-major, fp32 handles).
    Returns (C as rows x n float32 on the host, B as the handle saw it, float64)"""
    n = B.shape[1]
    rows = d.rows if rows is None else rows
    if row_major:
        Bt = torch.from_numpy(np.ascontiguousarray(B, np.float32)).cuda().reshape(-1)
        ldb, Br = n, Bt.cpu().numpy().astype(np.float64).reshape(v.cols, n)
    else:
        ldb = v.cols + (v.cols & 1)
        t = torch.zeros((n, ldb), dtype=torch.float64)
        t[:, :v.cols] = torch.from_numpy(np.ascontiguousarray(B.T))
        Bt = t.cuda().to(TDT[dtype]).reshape(-1)
        Br = Bt.float().cpu().numpy().astype(np.float64).reshape(n, ldb)[:, :v.cols].T
    Ct = torch.full((rows * n,), float("nan"), dtype=torch.float32, device="cuda")
    d.spmm(Bt, Ct, n, algo=algo, b_layout=sa.ROW_MAJOR if row_major else sa.COL_MAJOR, ldb=ldb)
    torch.cuda.synchronize()
    return Ct.cpu().numpy().reshape(n, rows).T, Br


def rounded(x, dtype):
    """the values a handle of `dtype` stores for x (the rounding tests/test_spmm_gpu.py checks 16-bit handles against)"""
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(TDT[dtype]).float().numpy()


def put(d, x):
    d.set_values(torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda())


def check_close(C, v, mab, Br, what=""):
    ref, bound = oracle(v, mab, Br), oracle(v, np.abs(mab), np.abs(Br))
    assert not np.isnan(C).any(), what
    err = np.abs(C - ref)
    assert np.all(err <= 1e-5 * bound + 1e-30), (what, float((err - 1e-5 * bound).max()))


CASES = [(k, sa.F32) for k in ("grid1", "grid8", "grid32", "grid64", "jaccard", "padded", "pairs")] + \
        [(k, dt) for dt in (sa.F16, sa.BF16) for k in ("grid32", "grid64", "jaccard", "padded", "pairs")]


@pytest.mark.parametrize("key,dtype", CASES, ids=["%s-%s" % (k, DT_ID[dt]) for k, dt in CASES])
def test_set_values_same_as_a_fresh_handle(mats, key, dtype):
    v = mats[key]
    H = v.to_device(0, dtype=dtype, updatable=True)                 # created from V0 = v.mab
    assert H.updatable and H.sparse_info()["rows"] == 0
    # (1) small integers: bit for bit the oracle, column-major B at three widths (+ row-major B on fp32 handles)
    V1 = values(v, 1, integer=True)
    m0, m1 = column_masks(v, v.mab), column_masks(v, V1)
    if v.block_col_size >= 8:                                       # (w = 1: a stored block is one column, never empty at creation)
        assert (m0 & ~m1).any() and (~m0 & m1).any()                # columns that become empty, columns that become non-empty
    put(H, V1)
    for n in (32, 128, 200):
        B = dense_b(v, n, 10 + n, integer=True)
        C, _ = product(H, v, B, dtype)
        assert np.array_equal(C, oracle(v, V1, B).astype(np.float32)), (key, n)
    if dtype == sa.F32:
        B = dense_b(v, 128, 11, integer=True)
        C, _ = product(H, v, B, dtype, row_major=True)
        assert np.array_equal(C, oracle(v, V1, B).astype(np.float32)), (key, "row-major B")
    # (2) other blocks zero, the zero blocks of V1 back: random real values within the MFMA tolerance ...
    V2 = values(v, 2, integer=False)
    put(H, V2)
    B = dense_b(v, 128, 12, integer=False)
    C, Br = product(H, v, B, dtype)
    check_close(C, v, rounded(V2, dtype), Br, key)
    if dtype == sa.F32:
        # ... and the exact-order kernel bit for bit what a fresh handle of V2 computes
        v2 = sa.VBR()
        v2.__dict__.update(v.__dict__)
        v2.mab, v2._dev, v2._dev_t = V2, None, None
        F = v2.to_device(0)
        Ch, _ = product(H, v, B, dtype, algo=sa.SPMM_EXACT)
        Cf, _ = product(F, v, B, dtype, algo=sa.SPMM_EXACT)
        assert np.array_equal(Ch.view(np.uint32), Cf.view(np.uint32)), key
        F.close()
    # (3) and integers once more
    V3 = values(v, 3, integer=True)
    put(H, V3)
    B = dense_b(v, 128, 13, integer=True)
    C, _ = product(H, v, B, dtype)
    assert np.array_equal(C, oracle(v, V3, B).astype(np.float32)), key
    H.close()


@pytest.mark.parametrize("dtype", [sa.F16, sa.BF16], ids=["f16", "bf16"])
def test_set_values_hub_slices(mats, dtype, monkeypatch):
    """the hub plan of a 16-bit handle of 64-wide blocks; the matrix is far too small for the default thresholds (8 steps per worker in all, 64 per tile), so
    the existing knobs lower them for this test"""
    monkeypatch.setenv("SPARTA_HUB_MIN_TOTAL", "1")
    monkeypatch.setenv("SPARTA_HUB_MIN_STEPS", "1")
    v = mats["hub"]
    H = v.to_device(0, dtype=dtype, updatable=True)
    assert H.hub_info()["steps"] > 0
    V1 = values(v, 1, integer=True)
    put(H, V1)
    for n in (128, 200):
        B = dense_b(v, n, 20 + n, integer=True)
        C, _ = product(H, v, B, dtype)
        assert np.array_equal(C, oracle(v, V1, B).astype(np.float32)), n
    V2 = values(v, 2, integer=False)
    put(H, V2)
    C, Br = product(H, v, dense_b(v, 128, 21, integer=False), dtype)
    check_close(C, v, rounded(V2, dtype), Br)
    H.close()


def test_set_values_16bit_rounding_of_special_values(mats):
    """NaN, Inf and values that round up to Inf go through the rounding creation applies: the products of an updated and of a fresh handle have the same bits"""
    v = mats["grid32"]
    V = values(v, 4, integer=False)
    nz = np.flatnonzero(V)
    V[nz[0]], V[nz[1]], V[nz[2]], V[nz[3]], V[nz[4]] = np.inf, -np.inf, np.nan, 65520.0, 1e-7
    v2 = sa.VBR()
    v2.__dict__.update(v.__dict__)
    v2.mab, v2._dev, v2._dev_t = V, None, None
    B = dense_b(v, 128, 30, integer=False)
    for dtype in (sa.F16, sa.BF16):
        H = v.to_device(0, dtype=dtype, updatable=True)
        F = v2.to_device(0, dtype=dtype, updatable=True)            # (updatable too: the same plan, whatever the sparse-row qualification would say)
        put(H, V)
        Ch, _ = product(H, v, B, dtype)
        Cf, _ = product(F, v, B, dtype)
        assert np.array_equal(Ch.view(np.uint32), Cf.view(np.uint32)), DT_ID[dtype]
        H.close(); F.close()


def test_set_values_on_a_handle_that_dropped_its_reference_layout_image(monkeypatch):
    """an fp32 handle whose products run on the no-barrier kernel keeps the fragment image only; set_values then writes that image alone and the exact-order
    kernel's image is rebuilt from it"""
    monkeypatch.delenv("SPARTA_F32_KEEP_LEGACY", raising=False)
    monkeypatch.setenv("SPARTA_PATH", "stream")                      # (as tests/test_spmm_gpu.py does for the same purpose: the stream kernels carry the products)
    m = sa.gen.uniform_random(512, 512, 40000, seed=45)
    v = vbr_of(m, np.arange(m.rows, dtype=np.int64) // 16, 32)
    H = v.to_device(0, updatable=True)
    a0 = H.info()["a_bytes"]
    B = dense_b(v, 128, 40, integer=False)
    product(H, v, B, sa.F32)
    if H.info()["a_bytes"] >= a0:
        pytest.skip("the no-barrier kernel did not carry the product on this run: the handle kept both images")
    V1 = values(v, 5, integer=False)
    put(H, V1)
    assert H.info()["a_bytes"] < a0                                  # still one image
    v2 = sa.VBR()
    v2.__dict__.update(v.__dict__)
    v2.mab, v2._dev, v2._dev_t = V1, None, None
    F = v2.to_device(0)
    Ch, _ = product(H, v, B, sa.F32, algo=sa.SPMM_EXACT)            # rebuilds the reference-layout image from the fragment image
    Cf, _ = product(F, v, B, sa.F32, algo=sa.SPMM_EXACT)
    assert np.array_equal(Ch.view(np.uint32), Cf.view(np.uint32))
    V2 = values(v, 6, integer=True)                                  # both images are there now
    put(H, V2)
    Bi = dense_b(v, 128, 41, integer=True)
    for algo in (sa.SPMM_MFMA, sa.SPMM_EXACT):
        C, _ = product(H, v, Bi, sa.F32, algo=algo)
        assert np.array_equal(C, oracle(v, V2, Bi).astype(np.float32)), algo
    H.close(); F.close()


@pytest.mark.parametrize("dtype", [sa.F32, sa.F16], ids=["f32", "f16"])
def test_sgd_step_with_sddmm(mats, dtype):
    """G = sddmm(dC, B); W = V0 - G; set_values(W): the next product is the oracle's on W, exactly (integers throughout)"""
    v = mats["padded"]
    k = 128 if dtype == sa.F32 else 8                                # (16-bit handles: |W| <= 4 + 8 * 16 stays exact in f16)
    rng = np.random.default_rng(50)
    V0 = values(v, 7, integer=True)
    H = v.to_device(0, dtype=dtype, updatable=True)
    put(H, V0)
    dC = rng.integers(-4, 5, (v.rows, k)).astype(np.float64)
    Bk = rng.integers(-4, 5, (v.cols, k)).astype(np.float64)
    lx, ly = v.rows + (v.rows & 1), v.cols + (v.cols & 1)
    X = torch.zeros((k, lx), dtype=torch.float64); X[:, :v.rows] = torch.from_numpy(np.ascontiguousarray(dC.T))
    Y = torch.zeros((k, ly), dtype=torch.float64); Y[:, :v.cols] = torch.from_numpy(np.ascontiguousarray(Bk.T))
    G = torch.zeros(int(v.nztot), dtype=torch.float32, device="cuda")
    H.sddmm(X.cuda().to(TDT[dtype]).reshape(-1), Y.cuda().to(TDT[dtype]).reshape(-1), G, k, ldx=lx, ldy=ly)
    W = torch.from_numpy(V0).cuda() - G
    H.set_values(W)
    Wh = W.cpu().numpy()
    assert np.abs(Wh).max() > 4                                      # the step did change the values
    B = dense_b(v, 128, 51, integer=True)
    C, _ = product(H, v, B, dtype)
    assert np.array_equal(C, oracle(v, Wh, B).astype(np.float32))
    H.close()


@pytest.mark.parametrize("dtype", [sa.F32, sa.BF16], ids=["f32", "bf16"])
def test_set_values_host_pointers_match_device(mats, dtype):
    v = mats["jaccard"]
    V1 = values(v, 8, integer=False)
    B = dense_b(v, 128, 60, integer=False)
    Hd = v.to_device(0, dtype=dtype, updatable=True)
    Hh = v.to_device(0, dtype=dtype, updatable=True)
    put(Hd, V1)
    assert Hh.set_values_host(V1) >= 0.0
    Cd, _ = product(Hd, v, B, dtype)
    Ch, _ = product(Hh, v, B, dtype)
    assert np.array_equal(Cd.view(np.uint32), Ch.view(np.uint32))
    Hd.close(); Hh.close()
    if dtype == sa.F32:                                              # the VBR entry: an updatable cached image is updated in place, any other is dropped
        v2 = sa.VBR()
        v2.__dict__.update(v.__dict__)
        v2._dev, v2._dev_t = v.to_device(0, updatable=True), None
        keep = v2._dev
        v2.set_values(V1)
        assert v2._dev is keep and np.array_equal(v2.mab, V1)
        Bf = np.ascontiguousarray(B.T, np.float32).ravel()
        C2 = np.zeros(v.rows * 128, np.float32)
        v2.multiply(Bf, 128, C2)
        check_close(C2.reshape(128, v.rows).T, v, V1, B.astype(np.float32).astype(np.float64))
        v2._dev.close()
        v2._dev = v.to_device(0)                                     # not updatable: dropped, the next multiply re-creates it from the new values
        v2.set_values(values(v, 9, integer=False))
        assert v2._dev is None
        C3 = np.zeros(v.rows * 128, np.float32)
        v2.multiply(Bf, 128, C3)
        check_close(C3.reshape(128, v.rows).T, v, v2.mab, B.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("dtype", [sa.F32, sa.F16], ids=["f32", "f16"])
def test_set_values_range_handle_takes_the_slice(mats, dtype):
    v = mats["jaccard"]
    b0, b1 = 1, v.block_rows
    a0 = int(sum(int(v.nzcount[i]) * (int(v.row_part[i + 1]) - int(v.row_part[i])) for i in range(b0))) * v.block_col_size
    H = v.to_device(0, dtype=dtype, block_row_range=(b0, b1), updatable=True)
    assert H.info()["nztot"] == v.nztot - a0
    V1 = values(v, 10, integer=True)
    put(H, V1[a0:])
    B = dense_b(v, 128, 70, integer=True)
    C, _ = product(H, v, B, dtype)
    assert np.array_equal(C, oracle(v, V1[a0:], B, b0, b1).astype(np.float32))
    with pytest.raises(ValueError):
        put(H, V1)                                                   # nztot of the whole matrix: wrong size for the range handle
    H.close()


@pytest.mark.parametrize("dtype", [sa.F32, sa.F16], ids=["f32", "f16"])
def test_set_values_graph_capture(mats, dtype):
    """set_values + spmm captured as one single-branch graph after one warm call; each replay uses what the mab tensor holds at that time"""
    v = mats["padded"]
    n = 128
    H = v.to_device(0, dtype=dtype, updatable=True)
    B = dense_b(v, n, 80, integer=True)
    ldb = v.cols + (v.cols & 1)
    t = torch.zeros((n, ldb), dtype=torch.float64)
    t[:, :v.cols] = torch.from_numpy(np.ascontiguousarray(B.T))
    Bt = t.cuda().to(TDT[dtype]).reshape(-1)
    W = torch.from_numpy(values(v, 11, integer=True)).cuda()
    Ct = torch.zeros(v.rows * n, dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        H.set_values(W)                                              # once outside a capture (the product's first call tunes and allocates)
        H.spmm(Bt, Ct, n, ldb=ldb)
        torch.cuda.synchronize()
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph, stream=s):
            H.set_values(W)
            H.spmm(Bt, Ct, n, ldb=ldb)
        for seed in (12, 13):
            Vn = values(v, seed, integer=True)
            W.copy_(torch.from_numpy(Vn).cuda())
            gph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(Ct.cpu().numpy().reshape(n, v.rows).T, oracle(v, Vn, B).astype(np.float32)), seed
    H.close()


def test_set_values_refusals(mats):
    v = mats["jaccard"]
    n = 128
    B = dense_b(v, n, 90, integer=False)
    Bf = np.ascontiguousarray(B.T, np.float32).ravel()
    B32 = B.astype(np.float32).astype(np.float64)
    t = tall_groups()
    handles = {
        "plain": v.to_device(0),
        "from_csr": sa.DeviceVBS.from_csr(t, sa.BlockingEngine(tau=0.6, col_block_size=32).GetGrouping(t), 32, device=0),
        "transposed": sa.DeviceVBS.transposed_of(v, device=0),
    }
    for name, d in handles.items():
        assert not d.updatable, name
        W = torch.zeros(max(d.info()["nztot"], 1), dtype=torch.float32, device="cuda")
        with pytest.raises(sa.SpartaError) as e:
            d.set_values(W[:d.info()["nztot"]] if d.info()["nztot"] else W[:0])
        assert e.value.code == sa._lib.ERR_UNSUPPORTED, name
        assert "SPARTA_CREATE_UPDATABLE" in str(e.value), name
        with pytest.raises(sa.SpartaError) as e:
            d.set_values_host(np.zeros(d.info()["nztot"], np.float32))
        assert e.value.code == sa._lib.ERR_UNSUPPORTED, name
    # ... and every one of them still multiplies
    C = np.zeros(v.rows * n, np.float32)
    handles["plain"].spmm_host(Bf, n, C, accumulate=False)
    check_close(C.reshape(n, v.rows).T, v, v.mab, B32, "plain")
    C = np.zeros(v.rows * n, np.float32)
    handles["from_csr"].spmm_host(Bf, n, C, accumulate=False)       # (the same matrix: v is the VBS of t under the same grouping)
    check_close(C.reshape(n, v.rows).T, v, v.mab, B32, "from_csr")
    M = 16
    rng = np.random.default_rng(91)
    Bl = rng.uniform(-1, 1, (M, v.rows))
    Cba = np.zeros(M * v.cols, np.float32)
    handles["transposed"].spmm_BA_host(np.ascontiguousarray(Bl.T, np.float32).ravel(), M, Cba, accumulate=False)
    Bl32 = Bl.astype(np.float32).astype(np.float64)
    At = oracle(v, v.mab, np.eye(v.cols))                            # A itself, dense
    ref, bound = Bl32 @ At, np.abs(Bl32) @ np.abs(At)
    assert np.all(np.abs(Cba.reshape(v.cols, M).T - ref) <= 1e-5 * bound + 1e-30)
    d = v.to_device(0, updatable=True)
    with pytest.raises(ValueError):
        d.set_values(torch.zeros(int(v.nztot), dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError):
        d.set_values(torch.zeros(int(v.nztot) - 1, dtype=torch.float32, device="cuda"))
    for h in list(handles.values()) + [d]:
        h.close()


# info() and sparse_info() of DeviceVBS(v) -- the old entry, flags = 0 -- as the commit BEFORE this feature reported them on an MI355X
# (read from a run of that commit's library on these matrices; last_path is 0 before any product)
PARENT_INFO = {
    ("grid1", 0): ({'a_bytes': 440784, 'block_col_size': 1, 'block_rows': 19, 'cols': 517, 'exec_area': 0, 'last_path': 0, 'nblocks': 5961, 'nztot': 94324, 'rows': 300, 'sparse_rows': 300, 'split_tiles': 0, 'stream_steps': 0, 'stream_workers': 0, 'tiles16': 0, 'tiles32': 0, 'tiles64': 0},
        {'hub_rows': 0, 'nnz': 9000, 'rows': 300, 'short_rows': 300}),
    ("grid32", 0): ({'a_bytes': 2013632, 'block_col_size': 32, 'block_rows': 19, 'cols': 517, 'exec_area': 165376, 'last_path': 0, 'nblocks': 323, 'nztot': 163200, 'rows': 300, 'sparse_rows': 0, 'split_tiles': 19, 'stream_steps': 323, 'stream_workers': 512, 'tiles16': 19, 'tiles32': 0, 'tiles64': 0},
        {'hub_rows': 0, 'nnz': 0, 'rows': 0, 'short_rows': 0}),
    ("grid32", 1): ({'a_bytes': 727040, 'block_col_size': 32, 'block_rows': 19, 'cols': 517, 'exec_area': 165376, 'last_path': 0, 'nblocks': 323, 'nztot': 163200, 'rows': 300, 'sparse_rows': 0, 'split_tiles': 19, 'stream_steps': 323, 'stream_workers': 256, 'tiles16': 19, 'tiles32': 0, 'tiles64': 0},
        {'hub_rows': 0, 'nnz': 0, 'rows': 0, 'short_rows': 0}),
    ("grid64", 0): ({'a_bytes': 2131072, 'block_col_size': 64, 'block_rows': 19, 'cols': 517, 'exec_area': 175104, 'last_path': 0, 'nblocks': 171, 'nztot': 172800, 'rows': 300, 'sparse_rows': 0, 'split_tiles': 19, 'stream_steps': 342, 'stream_workers': 512, 'tiles16': 19, 'tiles32': 0, 'tiles64': 0},
        {'hub_rows': 0, 'nnz': 0, 'rows': 0, 'short_rows': 0}),
    ("grid8", 0): ({'a_bytes': 624000, 'block_col_size': 8, 'block_rows': 19, 'cols': 517, 'exec_area': 157952, 'last_path': 0, 'nblocks': 1234, 'nztot': 155872, 'rows': 300, 'sparse_rows': 0, 'split_tiles': 0, 'stream_steps': 0, 'stream_workers': 0, 'tiles16': 19, 'tiles32': 0, 'tiles64': 0},
        {'hub_rows': 0, 'nnz': 0, 'rows': 0, 'short_rows': 0}),
    ("hub", 1): ({'a_bytes': 1114112, 'block_col_size': 64, 'block_rows': 8, 'cols': 1000, 'exec_area': 524288, 'last_path': 0, 'nblocks': 128, 'nztot': 393216, 'rows': 384, 'sparse_rows': 0, 'split_tiles': 8, 'stream_steps': 128, 'stream_workers': 256, 'tiles16': 0, 'tiles32': 0, 'tiles64': 8},
        {'hub_rows': 0, 'nnz': 0, 'rows': 0, 'short_rows': 0}),
    ("jaccard", 0): ({'a_bytes': 307712, 'block_col_size': 32, 'block_rows': 3, 'cols': 700, 'exec_area': 98304, 'last_path': 0, 'nblocks': 24, 'nztot': 76800, 'rows': 300, 'sparse_rows': 0, 'split_tiles': 6, 'stream_steps': 48, 'stream_workers': 512, 'tiles16': 0, 'tiles32': 0, 'tiles64': 6},
        {'hub_rows': 0, 'nnz': 0, 'rows': 0, 'short_rows': 0}),
    ("jaccard", 1): ({'a_bytes': 262144, 'block_col_size': 32, 'block_rows': 3, 'cols': 700, 'exec_area': 98304, 'last_path': 0, 'nblocks': 24, 'nztot': 76800, 'rows': 300, 'sparse_rows': 0, 'split_tiles': 0, 'stream_steps': 48, 'stream_workers': 256, 'tiles16': 0, 'tiles32': 0, 'tiles64': 6},
        {'hub_rows': 0, 'nnz': 0, 'rows': 0, 'short_rows': 0}),
    ("padded", 0): ({'a_bytes': 215296, 'block_col_size': 32, 'block_rows': 6, 'cols': 192, 'exec_area': 24576, 'last_path': 0, 'nblocks': 24, 'nztot': 24576, 'rows': 192, 'sparse_rows': 0, 'split_tiles': 0, 'stream_steps': 24, 'stream_workers': 512, 'tiles16': 0, 'tiles32': 6, 'tiles64': 0},
        {'hub_rows': 0, 'nnz': 0, 'rows': 0, 'short_rows': 0}),
    ("padded", 1): ({'a_bytes': 122880, 'block_col_size': 32, 'block_rows': 6, 'cols': 192, 'exec_area': 24576, 'last_path': 0, 'nblocks': 24, 'nztot': 24576, 'rows': 192, 'sparse_rows': 0, 'split_tiles': 0, 'stream_steps': 14, 'stream_workers': 256, 'tiles16': 0, 'tiles32': 6, 'tiles64': 0},
        {'hub_rows': 0, 'nnz': 0, 'rows': 0, 'short_rows': 0}),
    ("pairs", 0): ({'a_bytes': 606016, 'block_col_size': 32, 'block_rows': 6, 'cols': 517, 'exec_area': 74752, 'last_path': 0, 'nblocks': 73, 'nztot': 71296, 'rows': 180, 'sparse_rows': 0, 'split_tiles': 6, 'stream_steps': 73, 'stream_workers': 512, 'tiles16': 0, 'tiles32': 6, 'tiles64': 0},
        {'hub_rows': 0, 'nnz': 0, 'rows': 0, 'short_rows': 0}),
    ("pairs", 1): ({'a_bytes': 253952, 'block_col_size': 32, 'block_rows': 6, 'cols': 517, 'exec_area': 74752, 'last_path': 0, 'nblocks': 73, 'nztot': 71296, 'rows': 180, 'sparse_rows': 0, 'split_tiles': 3, 'stream_steps': 46, 'stream_workers': 256, 'tiles16': 0, 'tiles32': 6, 'tiles64': 0},
        {'hub_rows': 0, 'nnz': 0, 'rows': 0, 'short_rows': 0}),
}


@pytest.mark.parametrize("key,dtype", sorted(PARENT_INFO), ids=["%s-%d" % kd for kd in sorted(PARENT_INFO)])
def test_plain_creation_is_unchanged(mats, key, dtype):
    d = mats[key].to_device(0, dtype=dtype)
    info, sparse = PARENT_INFO[(key, dtype)]
    assert d.info() == info
    assert d.sparse_info() == sparse
    assert not d.updatable
    d.close()


def test_updatable_handle_keeps_sparse_row_candidates_in_the_tiles(monkeypatch):
    monkeypatch.setenv("SPARTA_SPARSE_MIN_STEPS", "1")
    monkeypatch.delenv("SPARTA_SPARSE_K", raising=False)
    m = sa.gen.uniform_random(256, 512, 2000, seed=46)               # ~8 nonzeros per step: below SPARTA_SPARSE_K = 24
    v = vbr_of(m, np.arange(m.rows, dtype=np.int64) // 32, 32)
    plain, upd = v.to_device(0), v.to_device(0, updatable=True)
    assert plain.info()["sparse_rows"] > 0 and plain.sparse_info()["rows"] > 0
    assert upd.info()["sparse_rows"] == 0 and upd.sparse_info()["rows"] == 0
    B = dense_b(v, 128, 95, integer=False)
    for d in (plain, upd):
        C, Br = product(d, v, B, sa.F32)
        check_close(C, v, v.mab, Br)
    V1 = values(v, 14, integer=True)
    put(upd, V1)
    Bi = dense_b(v, 128, 96, integer=True)
    C, _ = product(upd, v, Bi, sa.F32)
    assert np.array_equal(C, oracle(v, V1, Bi).astype(np.float32))
    plain.close(); upd.close()
