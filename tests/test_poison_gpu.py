"""Poison tests: an output element depends only on the operands that define it (the dependency contract of include/sparta_amd.h, next to sparta_vbs_spmm).

Every other GPU test feeds the kernels finite operands, and a kernel that multiplies a part of B, X or Y it has no business touching by a zero passes them:
0 * b = 0.  Here that part of the operand holds +Inf, -Inf or NaN (a finite 1e5 for an f16 handle given fp32 host data: the conversion makes it Inf): 0 * Inf
is NaN, and an output element that the contract says cannot see the poison turns non-finite.  The matrices are the poison geometries of tests/_util.py (8 x 8
blocks, block-row ib stores every block column but ib and (ib + 3) % 8: whatever two or four block-rows a planner puts into one tile own different block
columns) and a CSR matrix thinned the same way.

Reference: tests/_util.py: poison_reference() and relatives, plain numpy float64 on the dense form (values rounded to the storage type first for 16-bit
handles), which reads B only where the contract lets the element read it, and three masks: clean elements must be finite and within the suite's bound
1e-5 * sum|a||b| (computed on the unpoisoned operands; an accumulating call adds 1e-5 * |C0|) of the reference, dirty elements (a non-zero of A meets poison)
must be non-finite, open elements (only stored zeros of A meet poison) are not checked.  tests/test_poison_host.py checks the reference and the masks on the
CPU.  Outputs are prefilled with NaN before an overwrite call and with a seeded finite C0 before an accumulating one.  Every test asserts from the handle's
own records which kernel carried the product.  Non-finite floats are ordinary data: every read stays inside the caller's buffers."""
import numpy as np
import pytest

import sparta_amd as sa

torch = pytest.importorskip("torch")

import _util as U  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-5
DT_ID = {sa.F32: "f32", sa.F16: "f16", sa.BF16: "bf16"}
TDT = {sa.F32: torch.float32, sa.F16: torch.float16, sa.BF16: torch.bfloat16}
BIG = {sa.F32: 3e38, sa.F16: 6e4, sa.BF16: 3e38}           # the padding of an input's leading dimension: finite, and never read
PATH_NAME = {0: "none", 1: "stream", 2: "per-class", 3: "generic"}
ENV = ("SPARTA_PATH", "SPARTA_H16_PATH", "SPARTA_H16_PAIR", "SPARTA_HUB", "SPARTA_HUB_G", "SPARTA_HUB_MIN_TOTAL", "SPARTA_HUB_MIN_STEPS", "SPARTA_HUB_TAU", "SPARTA_SPARSE_K",
       "SPARTA_SPARSE_MIN_STEPS", "SPARTA_LAUNCH_NNZ", "SPARTA_COLRES", "SPARTA_UNION", "SPARTA_SP_WINDOW_COLS", "SPARTA_SP_LONG", "SPARTA_SP_MINSEG", "SPARTA_SPARSE_K_BLOCK", "SPARTA_COLRES_NC")
H16 = [sa.F16, sa.BF16]
ALL_TRAIN = [(k, sa.F32) for k in U.POISON_F32] + [(k, dt) for dt in H16 for k in U.POISON_H16]
ids_of = lambda cases: ["%s-%s" % (k, DT_ID[dt]) for k, dt in cases]  # noqa: E731


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def geometry(key):
    return U.poison_geometries()[key]


def ld_of(n, pad, dtype):
    x = n + pad
    return x + (x & 1) if dtype != sa.F32 else x


def operand(shape, seed, dtype):
    """seeded uniform(-1, 1) as the device will hold it (rounded to the handle's B type), float64"""
    return U.edge_round(np.random.default_rng(seed).uniform(-1, 1, shape), dtype)


def dev_in(M, ld, dtype):
    """M (r x n float64, may hold Inf / NaN) as a column-major device operand with leading dimension ld; the padding rows hold BIG"""
    r, n = M.shape
    buf = np.full((n, ld), BIG[dtype], np.float32)
    with np.errstate(all="ignore"):
        buf[:, :r] = M.T
    return torch.from_numpy(buf.reshape(-1)).to(TDT[dtype]).cuda()


def out_tensor(r, n, row_major, C0):
    """a dense r x n output: NaN everywhere (overwrite) or C0 (accumulate)"""
    img = np.full((r, n) if row_major else (n, r), np.nan, np.float32)
    if C0 is not None:
        img[:] = C0 if row_major else C0.T
    return torch.from_numpy(img.reshape(-1).copy()).cuda()


def read_out(Cd, r, n, row_major):
    got = Cd.cpu().numpy()
    return got.reshape(r, n) if row_major else got.reshape(n, r).T


def check(got, ref, what, C0=None):
    """ref = (want, clean, dirty, open, bound): see the head of the file"""
    want, clean, dirty, _, bound = ref
    got = got.astype(np.float64)
    assert np.isfinite(got[clean]).all(), (what, "poison reached %d elements that cannot see it, e.g. (row, column) %s"
                                           % (int((~np.isfinite(got) & clean).sum()), np.argwhere(~np.isfinite(got) & clean)[:4].tolist()))
    base = 0.0 if C0 is None else C0
    lim = TOL * (bound + np.abs(base)) + 1e-30
    err = np.abs(got - (np.where(clean, want, 0.0) + base))
    assert (err[clean] <= lim[clean]).all(), (what, float(err[clean].max(initial=0)), float((err[clean] / lim[clean]).max(initial=0)))
    assert not np.isfinite(got[dirty]).any(), (what, "%d elements that multiply the poison by a non-zero are finite" % int(np.isfinite(got[dirty]).sum()))


def forward_ref(D, stored, B, Bp):
    """the reference of D @ Bp (Bp: B with poison) with the bound taken from the unpoisoned B"""
    return U.poison_reference(D, stored, Bp) + (np.abs(D) @ np.abs(B),)


def b_combos(v, n, kinds=("+inf", "-inf", "nan", "mix")):
    """(rows of B to poison, column or None, kind, name): placement (a) -- every column, each poison value -- and (b) -- one column j* in {0, 37, n - 1}, the
    mixed values -- for block columns 1 and 7 (the ragged one)"""
    out = []
    for c in (1, 7):
        rows = U.block_col_rows(v, c)
        out += [(rows, None, kind, "c*=%d all columns %s" % (c, kind)) for kind in kinds]
        out += [(rows, j, "mix", "c*=%d column %d" % (c, j)) for j in (0, 37, n - 1)]
    return out


def spmm(d, rows, Bd, ldb, n, row_major=False, C0=None, algo=sa.SPMM_MFMA):
    Cd = out_tensor(rows, n, row_major, C0)
    d.spmm(Bd, Cd, n, accumulate=C0 is not None, algo=algo, c_layout=sa.ROW_MAJOR if row_major else sa.COL_MAJOR, ldb=ldb)
    torch.cuda.synchronize()
    return read_out(Cd, rows, n, row_major)


def forward_sweep(d, D, stored, cols, dtype, n, combos, seed, what, expect=None, every_layout=True):
    """every combo: overwrite into a column-major C; the first combo of each block column also row-major and accumulating.  expect(d): asserts the carrier."""
    B = operand((cols, n), seed, dtype)
    C0 = operand((D.shape[0], n), seed + 1, sa.F32) * 5.0
    ldb = ld_of(cols, 3, dtype)
    for q, (rows, j, kind, name) in enumerate(combos):
        Bp = U.poisoned(B, rows, kind, j)
        ref = forward_ref(D, stored, B, Bp)
        Bd = dev_in(Bp, ldb, dtype)
        variants = [(False, None)] + ([(True, None), (False, C0), (True, C0)] if every_layout and (j is None and kind in ("+inf", "mix")) else [])
        for row_major, acc in variants:
            w_ = (what, "n=%d" % n, name, "C row-major" if row_major else "C column-major", "accumulate" if acc is not None else "overwrite")
            check(spmm(d, D.shape[0], Bd, ldb, n, row_major, acc), ref, w_, acc)
            if expect is not None:
                expect(d, w_)


# ---- 1. forward product, fp32 ------------------------------------------------------------------------------------------------------------------
def f32_paths(d, v, n, forced):
    """the paths a product of n columns may end on (the rule of sparta_vbs_spmm, as in tests/test_edge_geometry_gpu.py)"""
    w, full = v.block_col_size, n % 128 == 0
    can_stream, can_class = w % 32 == 0 and full and d.info()["stream_workers"] > 0, w % 64 == 0 and full
    if forced == "stream":
        return {"stream"} if can_stream else {"generic"}
    if forced == "class":
        return {"per-class"} if can_class else {"generic"}
    if can_stream and can_class:
        return {"stream", "per-class"}
    return {"stream"} if can_stream else {"per-class"} if can_class else {"generic"}


@pytest.mark.parametrize("forced", ["stream", "class", None], ids=["stream", "class", "own-choice"])
@pytest.mark.parametrize("key", U.POISON_F32)
def test_forward_f32(key, forced, monkeypatch):
    """fp32 handles: SPARTA_PATH stream / class / the library's choice at n = 128 (a whole slab: the stream kernel for P32 and P64, the per-class kernels for
    P64), the generic (direct) kernels at n = 40 and for P13; SPARTA_SPMM_EXACT on P32"""
    monkeypatch.setenv("SPARTA_SPARSE_K", "0")                     # every block-row on the tiles
    if forced is not None:
        monkeypatch.setenv("SPARTA_PATH", forced)
    v = geometry(key)
    d = v.to_device(0)
    try:
        assert d.sparse_info()["rows"] == 0 and (d.info()["stream_workers"] > 0) == (v.block_col_size % 32 == 0), d.info()
        D, stored = U.edge_dense(v), U.stored_mask(v)
        seen = set()
        for n in (40, 128):
            def expect(d, w_, n=n):
                carried = PATH_NAME[d.info()["last_path"]]
                assert carried in f32_paths(d, v, n, forced), (w_, "carried by", carried)
                seen.add((n, carried))
            forward_sweep(d, D, stored, v.cols, sa.F32, n, b_combos(v, n), 100 + n, (key, forced or "own-choice"), expect)
        if key != "P13" and forced == "stream":
            assert (128, "stream") in seen, seen
        if key == "P64" and forced == "class":
            assert (128, "per-class") in seen, seen
        assert (40, "generic") in seen, seen
        if key == "P32" and forced is None:
            n = 40
            B = operand((v.cols, n), 300, sa.F32)
            for rows, j, kind, name in b_combos(v, n, kinds=("mix",)):
                Bp = U.poisoned(B, rows, kind, j)
                ldb = v.cols + 3
                got = spmm(d, v.rows, dev_in(Bp, ldb, sa.F32), ldb, n, algo=sa.SPMM_EXACT)
                check(got, forward_ref(D, stored, B, Bp), (key, "exact-order kernel", name))
    finally:
        d.close()


# ---- 2. forward product, 16-bit ----------------------------------------------------------------------------------------------------------------
def h16_host_product(d, v, D, stored, dtype, n, seed, what):
    """host pointers, fp32 B: the library rounds B on the device.  f16: a finite 1e5 becomes Inf there"""
    B = operand((v.cols, n), seed, dtype)
    for kind in ("mix",) + (("1e5",) if dtype == sa.F16 else ()):
        for c in (1, 7):
            rows = U.block_col_rows(v, c)
            Bp = U.poisoned(B, rows, kind)
            Bh = np.ascontiguousarray(B.T, np.float32)
            with np.errstate(all="ignore"):
                Bh[:, rows] = 1.0e5 if kind == "1e5" else Bp.T[:, rows]
            Ch = np.full(v.rows * n, np.nan, np.float32)
            d.spmm_host(Bh.reshape(-1), n, Ch, accumulate=False)
            check(Ch.reshape(n, v.rows).T, forward_ref(D, stored, B, Bp), (what, "host fp32 B", kind, "c*=%d" % c))


@pytest.mark.parametrize("h16_path", ["lds", "direct"])
@pytest.mark.parametrize("pair", ["pair-tiles", "no-pairs"])
@pytest.mark.parametrize("dtype", H16, ids=["f16", "bf16"])
def test_forward_h16_p32(dtype, pair, h16_path, monkeypatch):
    """P32 on a 16-bit handle: with the pair plan (the default: block-rows (0, 1), (2, 3), (4, 5) walked as 64-row tiles over the union of their block columns
    -- every step of such a tile has a half whose block-row lacks the column, or both halves present) and without, on the LDS and the direct kernels"""
    monkeypatch.setenv("SPARTA_SPARSE_K", "0")
    monkeypatch.setenv("SPARTA_H16_PATH", h16_path)
    if pair == "no-pairs":
        monkeypatch.setenv("SPARTA_H16_PAIR", "0")
    v = geometry("P32")
    d = v.to_device(0, dtype=dtype)
    try:
        info = d.info()
        # one step per tile and block column (32-wide blocks): 8 * 6 = 48 without pairs; a pair tile walks the union of its two block-rows' columns once
        assert (info["stream_steps"] < int(v.nzcount.sum())) == (pair == "pair-tiles") and info["stream_steps"] > 0 and d.sparse_info()["rows"] == 0, info
        D, stored = U.edge_dense(v, dtype), U.stored_mask(v)

        def expect(d, w_):
            assert PATH_NAME[d.info()["last_path"]] == "stream", (w_, d.info())
        for n in (128, 200):
            forward_sweep(d, D, stored, v.cols, dtype, n, b_combos(v, n), 400 + n, ("P32", DT_ID[dtype], pair, h16_path), expect)
        h16_host_product(d, v, D, stored, dtype, 128, 450, ("P32", DT_ID[dtype], pair, h16_path))
    finally:
        d.close()


@pytest.mark.parametrize("plan", ["stream", "hub-2", "hub-4"])
@pytest.mark.parametrize("dtype", H16, ids=["f16", "bf16"])
def test_forward_h16_p64(dtype, plan, monkeypatch):
    """P64 on a 16-bit handle: the stream kernels alone, and the hub plan (group tiles of 2 and 4 block-rows of 33..64 rows over the union of their block columns,
    k_hub16.hip) forced onto this small matrix"""
    monkeypatch.setenv("SPARTA_SPARSE_K", "0")
    if plan != "stream":
        monkeypatch.setenv("SPARTA_HUB_MIN_TOTAL", "1")
        monkeypatch.setenv("SPARTA_HUB_MIN_STEPS", "1")
        monkeypatch.setenv("SPARTA_HUB_G", plan[-1])
        monkeypatch.setenv("SPARTA_HUB_TAU", "0.25")               # two block-rows here share 4 or 5 of the 7 or 8 block columns of their union (0.5 .. 0.71), four
                                                                   # share 2 of 8: a group of four needs a threshold below that (the assertion on hub_info() below holds the plan to it)
    v = geometry("P64")
    d = v.to_device(0, dtype=dtype)
    try:
        hi = d.hub_info()
        if plan == "stream":
            assert hi["steps"] == 0, hi
        else:
            assert hi["steps"] > 0 and hi["groups"] >= 1 and hi["tiles_per_group"] == int(plan[-1]) and hi["union_area"] > hi["stored_area"] > 0, hi
        D, stored = U.edge_dense(v, dtype), U.stored_mask(v)

        def expect(d, w_):
            assert PATH_NAME[d.info()["last_path"]] == "stream", (w_, d.info())
        for n in (128, 200, 256):
            forward_sweep(d, D, stored, v.cols, dtype, n, b_combos(v, n), 500 + n, ("P64", DT_ID[dtype], plan), expect, every_layout=n != 200)
        h16_host_product(d, v, D, stored, dtype, 128, 550, ("P64", DT_ID[dtype], plan))
    finally:
        d.close()


# ---- 3. prepared B ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,dtype", [("P32", sa.F32), ("P64", sa.F32), ("P32", sa.F16), ("P64", sa.BF16)], ids=["P32-f32", "P64-f32", "P32-f16", "P64-bf16"])
def test_prepared_b(key, dtype, monkeypatch):
    """sparta_vbs_prepare_b + sparta_vbs_spmm_prepared on a poisoned B"""
    monkeypatch.setenv("SPARTA_SPARSE_K", "0")
    v = geometry(key)
    d = v.to_device(0, dtype=dtype)
    try:
        D, stored = U.edge_dense(v, dtype), U.stored_mask(v)
        n = 128
        B = operand((v.cols, n), 600, dtype)
        ldb = ld_of(v.cols, 3, dtype)
        for rows, j, kind, name in b_combos(v, n, kinds=("mix",)):
            Bp = U.poisoned(B, rows, kind, j)
            Bd = dev_in(Bp, ldb, dtype)
            P = d.prepare_b(Bd, n, ldb=ldb)
            try:
                Cd = out_tensor(v.rows, n, False, None)
                d.spmm_prepared(P, Cd)
                torch.cuda.synchronize()
                check(read_out(Cd, v.rows, n, False), forward_ref(D, stored, B, Bp), (key, DT_ID[dtype], "prepared B", name))
                assert PATH_NAME[d.info()["last_path"]] in (f32_paths(d, v, n, None) if dtype == sa.F32 else {"stream"}), d.info()
            finally:
                P.close()
    finally:
        d.close()


def gathered_image(Bp, shard_rows, shard_ld, shard_stride, dtype):
    """Bp (cols x n float64) as n_shards column-major slabs of shard_rows x n, shard_ld elements between the columns of a slab and shard_stride between the
    slabs; every element of the buffer outside the slabs -- the padding of shard_ld and the gap between the slabs -- holds poison (NaN, +Inf, -Inf in turn)"""
    cols, n = Bp.shape
    shards = cols // shard_rows
    buf = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange((shards - 1) * shard_stride + shard_ld * n) % 3]
    for s_ in range(shards):
        view = buf[s_ * shard_stride:s_ * shard_stride + shard_ld * n].reshape(n, shard_ld)
        with np.errstate(all="ignore"):
            view[:, :shard_rows] = Bp[s_ * shard_rows:(s_ + 1) * shard_rows].T
    return torch.from_numpy(buf).to(TDT[dtype]).cuda()


@pytest.mark.parametrize("key,dtype", [("P32G", sa.F32), ("P64G", sa.F32), ("P32G", sa.F16), ("P64G", sa.BF16)], ids=["P32G-f32", "P64G-f32", "P32G-f16", "P64G-bf16"])
def test_gathered_b(key, dtype, monkeypatch):
    """sparta_vbs_spmm_gathered, sparta_vbs_spmm_gathered_ld and sparta_vbs_prepare_b (shard_rows > 0) + sparta_vbs_spmm_prepared on P32G / P64G (cols = 8 w: a
    gathered B has cols = n_shards * shard_rows, which the ragged P32 / P64 do not allow): two slabs of 4 w rows with shard_stride > shard_ld * n, the gap
    between them and the padding of shard_ld poisoned entirely, in addition to placement (a) and one column of (b)"""
    monkeypatch.setenv("SPARTA_SPARSE_K", "0")
    v = geometry(key)
    d = v.to_device(0, dtype=dtype)
    try:
        D, stored = U.edge_dense(v, dtype), U.stored_mask(v)
        shard_rows = v.cols // 2
        for n in (40, 128):
            B = operand((v.cols, n), 650 + n, dtype)
            want_path = f32_paths(d, v, n, None) if dtype == sa.F32 else {"stream"}
            for c in (1, 7):
                for j in (None, 37):
                    Bp = U.poisoned(B, U.block_col_rows(v, c), "mix", j)
                    ref = forward_ref(D, stored, B, Bp)
                    for shard_ld, gap in ((shard_rows, 64), (shard_rows + 8, 0), (shard_rows + 8, 72)):          # _gathered; _gathered_ld, slabs back to back; both
                        stride = shard_ld * n + gap
                        Bd = gathered_image(Bp, shard_rows, shard_ld, stride, dtype)
                        what = (key, DT_ID[dtype], "n=%d c*=%d column %s" % (n, c, j), "shard_ld %d stride %d" % (shard_ld, stride))
                        Cd = out_tensor(v.rows, n, False, None)
                        d.spmm_gathered(Bd, shard_rows, Cd, n, shard_stride=stride, shard_ld=shard_ld)
                        torch.cuda.synchronize()
                        check(read_out(Cd, v.rows, n, False), ref, what + ("gathered",))
                        assert PATH_NAME[d.info()["last_path"]] in want_path, (what, d.info())
                        P = d.prepare_b(Bd, n, ldb=shard_ld, shard_rows=shard_rows, shard_stride=stride)
                        try:
                            Cd = out_tensor(v.rows, n, False, None)
                            d.spmm_prepared(P, Cd)
                            torch.cuda.synchronize()
                            check(read_out(Cd, v.rows, n, False), ref, what + ("prepared",))
                            assert PATH_NAME[d.info()["last_path"]] in want_path, (what, d.info())
                        finally:
                            P.close()
    finally:
        d.close()


# ---- 4. sparse rows and relatives: a handle made from a CSR ----------------------------------------------------------------------------------------
CSR_MODES = {          # mode -> (matrix, environment, types)
    "row-gather": ("PCSR", {"SPARTA_COLRES": "0"}, (sa.F32, sa.BF16)),
    "windows": ("PCSR", {"SPARTA_COLRES": "0", "SPARTA_SP_WINDOW_COLS": "64", "SPARTA_SP_LONG": "8", "SPARTA_SP_MINSEG": "1"}, (sa.F32, sa.BF16)),
    "resident-columns": ("PCSR", {}, (sa.F32,)),                                                   # (the resident-column kernel is fp32 only)
    "tiles-and-sparse-rows": ("PSPLIT", {"SPARTA_COLRES": "0", "SPARTA_UNION": "0", "SPARTA_SPARSE_K_BLOCK": "8"}, (sa.F32, sa.BF16)),
    "union-tiles": ("PUNI", {"SPARTA_COLRES": "0"}, (sa.F32, sa.F16)),
}
CSR_MATRIX = {"PCSR": U.poison_csr, "PSPLIT": U.poison_split, "PUNI": U.poison_union}
CSR_CASES = [(dt, mode) for mode, (_, _, dts) in CSR_MODES.items() for dt in dts]


@pytest.mark.parametrize("dtype,mode", CSR_CASES, ids=["%s-%s" % (DT_ID[dt], mode) for dt, mode in CSR_CASES])
def test_forward_from_csr_sparse_rows(dtype, mode, monkeypatch):
    """handles from sparta_vbs_create_from_csr.  PCSR: the row gather, the window plan (the smallest windows of
    test_sparse_rows_cut_at_column_windows_...), and the resident-column kernel (fp32, the reference's layouts, n = 8 and 1024 by the library's choice of the
    columns per workgroup, then 2, 3 and 4 of them at n = 8).  PSPLIT: block-rows split into tiles and sparse rows that add (SPARTA_SPARSE_K_BLOCK as in
    test_create_from_csr_splits_a_block_row_into_tiles_and_sparse_rows).  PUNI: the column-compacted (union) tiles.  The poison sits in block columns 3 and
    15, which every third block-row does not store; a row of a block-row that does store them but has no nonzero there is open."""
    monkeypatch.setenv("SPARTA_SPARSE_MIN_STEPS", "0")
    monkeypatch.setenv("SPARTA_LAUNCH_NNZ", "0")
    which, env, _ = CSR_MODES[mode]
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    m, g, w = CSR_MATRIX[which]()
    d = sa.DeviceVBS.from_csr(m, g, w, device=0, dtype=dtype)
    try:
        sp, ui, info = d.sparse_info(), d.union_info(), d.info()
        tiles = info["tiles16"] + info["tiles32"] + info["tiles64"]
        if which == "PCSR":
            assert sp["rows"] > 0 and sp["nnz"] == m.nztot() and tiles == 0 and ui["nnz"] == 0, (sp, ui, info)
        if mode == "windows":
            assert sp["hub_rows"] > 0, sp
        if mode == "tiles-and-sparse-rows":                        # tiles AND sparse rows, and every block-row has both: more rows add than any one kind of block-row has
            assert tiles >= m.rows // 32 and 0 < sp["nnz"] < m.nztot() and sp["rows"] > m.rows * 2 // 3 and ui["nnz"] == 0, (sp, ui, info)
        if mode == "union-tiles":
            assert ui["tiles32"] + ui["tiles64"] >= len(np.unique(g)) and ui["nnz"] > 0.7 * m.nztot() and ui["nnz"] + sp["nnz"] == m.nztot() and tiles == 0, (sp, ui, info)
        if mode == "resident-columns":
            assert d.colres_info()["slices"] > 0, d.colres_info()
        else:
            assert d.colres_info()["slices"] == 0, d.colres_info()
        D, stored = U.csr_dense_and_stored(m, g, w)
        D = U.edge_round(D, dtype)
        ncs = []

        def combos_of(n):
            out = []
            for c in U.PCSR_THIN:
                rows = slice(c * w, (c + 1) * w)
                out += [(rows, None, "mix", "c*=%d all columns" % c)] + [(rows, j, "mix", "c*=%d column %d" % (c, j)) for j in ((0, n - 1) if n < 38 else (0, 37, n - 1))]
            return out

        def expect(d, w_):
            nc = d.colres_info()["nc"]
            assert (nc > 0) == (mode == "resident-columns"), (w_, d.colres_info())
            ncs.append(nc)
        for n in (8, 1024) if mode == "resident-columns" else (40, 128):
            forward_sweep(d, D, stored, m.cols, dtype, n, combos_of(n), 700 + n, (which, DT_ID[dtype], mode), expect, every_layout=mode != "resident-columns")
        if mode == "resident-columns":
            for nc in (2, 3, 4):                                      # (columns of B per workgroup: each is a form of the kernel; 512 columns of B fit LDS four times)
                monkeypatch.setenv("SPARTA_COLRES_NC", str(nc))
                del ncs[:]
                forward_sweep(d, D, stored, m.cols, dtype, 8, combos_of(8), 708, (which, DT_ID[dtype], mode, "NC=%d" % nc), expect, every_layout=False)
                assert set(ncs) == {nc}, (nc, ncs)
    finally:
        d.close()


# ---- 5. B x A on a transposed handle ---------------------------------------------------------------------------------------------------------------
def test_spmm_ba_on_a_transposed_handle():
    """sparta_vbs_spmm_ba: C = B A with B M x rows(A) on the handle of A^T, which sparta_vbs_create_transposed makes from the CSR of A^T with the block columns
    of A as block-rows and a 32-wide grid over the rows of A as block columns.  C^T = A^T B^T is a forward product of that handle: column k of B meets row k
    of A, and the poison goes to the columns of B of one block column of A^T (c* = 1: rows 32..63 of A, exactly block-row 1, so the block columns 1 and 4 of A
    stay clean; c* = 7, the ragged one: rows of block-rows 6 and 7, which between them store every block column -- nothing stays clean but the other columns)"""
    v = geometry("P32")
    d = sa.DeviceVBS.transposed_of(v, device=0)
    try:
        info = d.info()          # every block of A^T is full: tiles, no sparse rows, no union tiles
        assert info["tiles16"] + info["tiles32"] + info["tiles64"] > 0 and d.sparse_info()["rows"] == 0 and d.union_info()["nnz"] == 0, (info, d.sparse_info(), d.union_info())
        Dt = np.ascontiguousarray(U.edge_dense(v).T)
        r, c = np.nonzero(Dt)
        has = np.zeros((8, (v.rows + 31) // 32), bool)
        has[r // v.block_col_size, c // 32] = True
        stored = np.repeat(np.repeat(has, v.block_col_size, axis=0)[:v.cols], 32, axis=1)[:, :v.rows]
        for M in (40, 128):
            Bt = operand((v.rows, M), 800 + M, sa.F32)                         # B^T: rows(A) x M
            for cell in (1, 7):
                for j in (None, 37):
                    Xp = U.poisoned(Bt, slice(32 * cell, min(32 * cell + 32, v.rows)), "mix", j)
                    ref = U.poison_reference(Dt, stored, Xp) + (np.abs(Dt) @ np.abs(Bt),)            # C^T: cols(A) x M
                    if cell == 1 and j is None:
                        assert ref[1][U.block_col_rows(v, 1)].all() and ref[1][U.block_col_rows(v, 4)].all() and ref[1].sum() == 64 * M
                    Ch = np.full(M * v.cols, np.nan, np.float32)
                    with np.errstate(all="ignore"):
                        Bh = np.ascontiguousarray(Xp, np.float32).reshape(-1)                        # B column-major M x rows(A) = B^T row-major
                    d.spmm_BA_host(Bh, M, Ch, accumulate=False)
                    check(Ch.reshape(v.cols, M), ref, ("spmm_ba", M, cell, j))
                    assert PATH_NAME[d.info()["last_path"]] == ("stream" if M % 128 == 0 and info["stream_workers"] > 0 else "generic"), (M, d.info())
    finally:
        d.close()


# ---- 6. the training entry points ------------------------------------------------------------------------------------------------------------------
RANGE = (2, 6)
_TRAIN = {}


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for d in _TRAIN.values():
        d.close()
    _TRAIN.clear()


def train_handle(key, dtype, br):
    if (key, dtype, br) not in _TRAIN:
        _TRAIN[(key, dtype, br)] = geometry(key).to_device(0, dtype=dtype, block_row_range=br, updatable=True, transposable=True)
    return _TRAIN[(key, dtype, br)]


@pytest.mark.parametrize("br", [None, RANGE], ids=["whole", "range"])
@pytest.mark.parametrize("key,dtype", ALL_TRAIN, ids=ids_of(ALL_TRAIN))
def test_spmm_t(key, dtype, br):
    """Ct = A^T X with every row of X of one block-row poisoned (r* = 3 and 7, the short block-rows -- 3 and 5 for the range 2..6 -- whose tile padding would
    reach the next block-row's rows): the rows of Ct of the block columns r* and (r* + 3) % 8 stay clean, every other row turns non-finite; then one column"""
    v = geometry(key)
    d = train_handle(key, dtype, br)
    D, stored = U.edge_dense(v, dtype, br=br), U.stored_mask(v, br)
    for n in (40, 128):
        X = operand((D.shape[0], n), 900 + n, dtype)
        C0 = operand((v.cols, n), 910 + n, sa.F32) * 5.0
        ldx = ld_of(D.shape[0], 5, dtype)
        for r in (3, 7) if br is None else (3, 5):
            for j, kind in ((None, "+inf"), (None, "nan"), (None, "mix"), (37, "mix")):
                Xp = U.poisoned(X, U.block_row_rows(v, r, br), kind, j)
                ref = U.poison_reference_t(D, stored, Xp) + (np.abs(D).T @ np.abs(X),)
                if j is None:
                    for c in (r, (r + 3) % 8):
                        assert ref[1][U.block_col_rows(v, c)].all()
                Xd = dev_in(Xp, ldx, dtype)
                for acc in (None, C0) if kind == "mix" else (None,):
                    Cd = out_tensor(v.cols, n, False, acc)
                    d.spmm_t(Xd, Cd, n, accumulate=acc is not None, ldx=ldx)
                    torch.cuda.synchronize()
                    check(read_out(Cd, v.cols, n, False), ref, (key, DT_ID[dtype], br, "spmm_t n=%d r*=%d" % (n, r), j, kind, "accumulate" if acc is not None else "overwrite"), acc)


@pytest.mark.parametrize("br", [None, RANGE], ids=["whole", "range"])
@pytest.mark.parametrize("key,dtype", ALL_TRAIN, ids=ids_of(ALL_TRAIN))
def test_sddmm(key, dtype, br):
    """G = (X Y^T) on the stored blocks: poison in X's rows of block-row r* makes exactly the blocks of r* non-finite, poison in Y's rows of block column c*
    exactly the blocks with jb = c*; overwrite (G prefilled with NaN) and accumulate (finite previous G)"""
    v = geometry(key)
    d = train_handle(key, dtype, br)
    b0, b1 = br or (0, 8)
    rows = int(v.row_part[b1] - v.row_part[b0])
    lo, hi = U.edge_mab_slice(v, (b0, b1))
    for k in (40, 128):
        X, Y = operand((rows, k), 1000 + k, dtype), operand((v.cols, k), 1010 + k, dtype)
        bound = U.edge_sample(v, np.abs(X) @ np.abs(Y).T, br)
        G0 = operand((hi - lo,), 1020 + k, sa.F32) * 5.0
        ldx, ldy = ld_of(rows, 5, dtype), ld_of(v.cols, 3, dtype)
        cases = [(U.poisoned(X, U.block_row_rows(v, r, br), kind), Y, "X r*=%d %s" % (r, kind)) for r in ((3, 7) if br is None else (3, 5)) for kind in ("mix", "nan")]
        cases += [(X, U.poisoned(Y, U.block_col_rows(v, c), kind), "Y c*=%d %s" % (c, kind)) for c in (1, 7) for kind in ("mix", "-inf")]
        for Xp, Yp, name in cases:
            G, clean, dirty = U.poison_reference_sddmm(v, Xp, Yp, br)
            assert clean.any() and dirty.any()
            Xd, Yd = dev_in(Xp, ldx, dtype), dev_in(Yp, ldy, dtype)
            for acc in (None, G0):
                Gd = torch.from_numpy(np.full(hi - lo, np.nan, np.float32) if acc is None else acc.astype(np.float32)).cuda()
                d.sddmm(Xd, Yd, Gd, k, accumulate=acc is not None, ldx=ldx, ldy=ldy)
                torch.cuda.synchronize()
                check(Gd.cpu().numpy(), (G, clean, dirty, None, bound), (key, DT_ID[dtype], br, "sddmm k=%d" % k, name, "accumulate" if acc is not None else "overwrite"),
                      None if acc is None else acc.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("br", [None, RANGE], ids=["whole", "range"])
@pytest.mark.parametrize("key,dtype", ALL_TRAIN, ids=ids_of(ALL_TRAIN))
def test_set_values(key, dtype, br, monkeypatch):
    """non-finite values in every stored block of block-row r*, then a forward product with a clean B: exactly the rows of r* are non-finite; clean values
    again: every element is clean again.  fp32: on the stream, per-class and generic kernels (the fragment image and the reference-layout image), each asserted from info()["last_path"]: P13
    runs the generic kernels whatever SPARTA_PATH says, P32 has no per-class kernel"""
    v = geometry(key)
    d = train_handle(key, dtype, br)
    b0, b1 = br or (0, 8)
    lo, hi = U.edge_mab_slice(v, (b0, b1))
    D, stored = U.edge_dense(v, dtype, br=br), U.stored_mask(v, br)
    rows = D.shape[0]
    V = v.mab[lo:hi].astype(np.float32)
    seen = set()
    try:
        for n, forced in ((128, "stream"), (128, "class"), (40, None)) if dtype == sa.F32 else ((128, None), (200, None)):
            monkeypatch.delenv("SPARTA_PATH", raising=False)
            if forced:
                monkeypatch.setenv("SPARTA_PATH", forced)
            B = operand((v.cols, n), 1100 + n, dtype)
            ldb = ld_of(v.cols, 3, dtype)
            Bd = dev_in(B, ldb, dtype)
            want, bound = D @ B, np.abs(D) @ np.abs(B)
            for r in (3, 7) if br is None else (3, 5):
                for bad in (np.inf, np.nan):
                    Vp = V.copy()
                    rr = U.block_row_rows(v, r, br)
                    for off, r0, h, _, _ in U.edge_blocks(v, br):
                        if r0 == rr.start:
                            Vp[off:off + h * v.block_col_size] = bad
                    d.set_values(torch.from_numpy(Vp).cuda())
                    dirty = np.zeros((rows, n), bool)
                    dirty[rr] = True
                    what = (key, DT_ID[dtype], br, "set_values r*=%d" % r, bad, "n=%d" % n, forced)
                    want_path = f32_paths(d, v, n, forced) if dtype == sa.F32 else {"stream"}
                    check(spmm(d, rows, Bd, ldb, n), (want, ~dirty, dirty, None, bound), what)
                    assert PATH_NAME[d.info()["last_path"]] in want_path, (what, d.info())
                    seen.add((n, forced, PATH_NAME[d.info()["last_path"]]))
                    d.set_values(torch.from_numpy(V).cuda())
                    check(spmm(d, rows, Bd, ldb, n), (want, np.ones((rows, n), bool), np.zeros((rows, n), bool), None, bound), what + ("clean values again",))
                    assert PATH_NAME[d.info()["last_path"]] in want_path, (what, d.info())
        if dtype == sa.F32:          # the three images of the values were all read: the stream kernel's (32-wide blocks and wider), the per-class kernels' (64-wide), the generic kernels'
            assert (40, None, "generic") in seen and ((128, "stream", "stream") in seen) == (key != "P13") and ((128, "class", "per-class") in seen) == (key == "P64"), seen
    finally:
        d.set_values(torch.from_numpy(V).cuda())
