"""Accuracy tests: every product kernel is held to the fp32 arithmetic DESIGN.md claims for it (section "Parity bar").

Bound tests: |got - ref64| <= gamma_bound per element (tests/_util.py: min(1e-5, 2 g_K) * sum|a||b| with K the number of non-zero products of the element), on
full-mantissa operands over a wide exponent range in which most elements sum fewer than five products (U.ACC_SETS; tests/test_accuracy_host.py proves the bound
for fp32 in any order and shows that a bf16-split product, 10-bit operands and fp16 partial sums miss it).  Exact tests: a single product on a 16-bit handle is
exact; scaling by powers of two and negation commute with every product, bit for bit; the 16-bit images (creation, set_values, the device conversion of host
operands) hold round-to-nearest-even values at every edge of the formats; fp32 subnormals underflow gradually.

Reference: numpy float64 on operands that are exactly what the device holds.  The carriers are forced and asserted from the handle's records as in
tests/test_poison_gpu.py, whose helpers this file imports.  Every check prints `ACC <carrier> <largest err / bound> <K there>` (pytest -s shows them;
profiles/accuracy/README.md is written from that output)."""
import numpy as np
import pytest

import sparta_amd as sa

torch = pytest.importorskip("torch")

import _util as U  # noqa: E402
from test_poison_gpu import PATH_NAME, DT_ID, f32_paths, ld_of, dev_in, out_tensor, read_out, gathered_image  # noqa: E402
from test_poison_gpu import ENV as POISON_ENV  # noqa: E402

pytestmark = pytest.mark.gpu

ENV = POISON_ENV + ("SPARTA_H16_DEPTH", "SPARTA_SPARSE_SEG")
H16 = [sa.F16, sa.BF16]
HUB_ENV = {"SPARTA_HUB_MIN_TOTAL": "1", "SPARTA_HUB_MIN_STEPS": "1", "SPARTA_HUB_TAU": "0.25"}          # (tests/test_poison_gpu.py: test_forward_h16_p64)
RECORD = {}


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module", autouse=True)
def _print_record():
    yield
    for carrier, (ratio, k) in sorted(RECORD.items()):
        print("ACCMAX %-60s %.4f K=%d" % (carrier, ratio, k))


def setenv(monkeypatch, env):
    for k, val in env.items():
        monkeypatch.setenv(k, val)


def vbr_of(v, mab):
    return U.sa_vbr((v.rows, v.cols, int(v.block_col_size), v.row_part, v.nzcount, v.jab), np.ascontiguousarray(mab, np.float32))


def fl32(x):
    """float64 / longdouble -> the nearest fp32, as float64"""
    with np.errstate(over="ignore"):
        return np.asarray(x).astype(np.float32).astype(np.float64)


def check_bound(got, L, R, C0, carrier, mask=None, exact_single=False, special=None):
    """got against L @ R (+ C0) under gamma_bound on the elements of mask; exact_single (16-bit handles): an element with ONE non-zero product equals it -- or
    fl32(C0 + a b) -- bit for bit.  special: (bool mask, expected fp32 values) of elements checked exactly elsewhere (left out here).  Records err / bound."""
    got = got.astype(np.float64)
    ref = L @ R + (0.0 if C0 is None else C0)
    tol, K = U.gamma_bound(L, R, C0), U.gamma_terms(L, R, C0)
    mask = np.ones(ref.shape, bool) if mask is None else mask
    if special is not None:
        mask = mask & ~special
    assert np.isfinite(got[mask]).all(), (carrier, "non-finite output")
    err = np.abs(got - ref)
    assert (err[mask & (tol == 0)] == 0).all(), (carrier, "an element without a non-zero product is not exact")
    ratio = np.where(mask & (tol > 0), err / np.where(tol > 0, tol, 1.0), 0.0)
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    print("ACC %s %.4f K=%d" % (carrier, ratio[at], K[at]))
    if ratio[at] >= RECORD.get(carrier, (-1.0, 0))[0]:
        RECORD[carrier] = (float(ratio[at]), int(K[at]))
    assert ratio[at] <= 1.0, (carrier, "err / bound %.3f at %s, K = %d, err %.3e" % (ratio[at], at, K[at], err[at]), "elements over the bound: %d" % int((ratio > 1).sum()))
    if exact_single:
        one = mask & (K - (0 if C0 is None else 1) == 1)
        assert one.any()
        want = fl32((L @ R).astype(np.longdouble) + (0 if C0 is None else C0.astype(np.longdouble)))          # (one product: L @ R is exact in float64)
        assert np.array_equal(got[one], want[one]), (carrier, "%d single products are not exact" % int((got[one] != want[one]).sum()))


def spmm(d, rows, cols, B, n, dtype, b_row=False, c_row=False, C0=None):
    """one product with device operands; B float64 cols x n in the layout asked for"""
    if b_row:
        Bd, ldb = torch.from_numpy(np.ascontiguousarray(B, np.float32)).cuda().reshape(-1), n
    else:
        ldb = ld_of(cols, 3, dtype)
        Bd = dev_in(B, ldb, dtype)
    Cd = out_tensor(rows, n, c_row, C0)
    d.spmm(Bd, Cd, n, accumulate=C0 is not None, b_layout=sa.ROW_MAJOR if b_row else sa.COL_MAJOR, c_layout=sa.ROW_MAJOR if c_row else sa.COL_MAJOR, ldb=ldb)
    torch.cuda.synchronize()
    return read_out(Cd, rows, n, c_row)


LAYOUTS = [(False, False, False), (True, True, False), (False, True, True), (True, False, True)]          # (B row-major, C row-major, accumulate)


# ---- 1. bound: forward product, fp32 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", ["stream", "class", None], ids=["stream", "class", "own-choice"])
@pytest.mark.parametrize("key", U.POISON_F32)
def test_forward_f32(key, forced, monkeypatch):
    """stream, per-class and generic kernels at n = 128 and n = 130 (no whole slab: generic), B and C column- and row-major, overwrite and accumulate"""
    monkeypatch.setenv("SPARTA_SPARSE_K", "0")
    if forced is not None:
        monkeypatch.setenv("SPARTA_PATH", forced)
    seen = set()
    for n in (128, 130):
        a = U.accuracy_set(("fwd", key, 0, "wide", n))
        v = a["v"]
        d = vbr_of(v, a["mab"]).to_device(0)
        try:
            assert d.sparse_info()["rows"] == 0, d.sparse_info()
            for b_row, c_row, acc in LAYOUTS:
                C0 = a["C0"] if acc else None
                got = spmm(d, v.rows, v.cols, a["R"], n, sa.F32, b_row, c_row, C0)
                carried = PATH_NAME[d.info()["last_path"]]
                assert carried in f32_paths(d, v, n, forced), (key, forced, n, carried)
                seen.add((n, carried))
                check_bound(got, a["L"], a["R"], C0, "forward f32 %s" % carried)
        finally:
            d.close()
    if key != "P13" and forced == "stream":
        assert (128, "stream") in seen, seen
    if key == "P64" and forced == "class":
        assert (128, "per-class") in seen, seen
    assert (130, "generic") in seen, seen


# ---- 2. bound + exact single products: forward product, 16-bit ------------------------------------------------------------------------------------------
H16_CONFIGS = {          # name -> (geometry, n, environment, carrier)
    "P32-lds-pairs": ("P32", 128, {"SPARTA_H16_PATH": "lds"}, "h16 lds kernel, pair tiles"),
    "P32-lds-depth4": ("P32", 128, {"SPARTA_H16_PATH": "lds", "SPARTA_H16_DEPTH": "4"}, "h16 lds kernel, depth 4"),
    "P32-direct-no-pairs": ("P32", 128, {"SPARTA_H16_PATH": "direct", "SPARTA_H16_PAIR": "0"}, "h16 direct kernel, no pairs"),
    "P32-auto": ("P32", 128, {}, "h16 own choice, pair tiles"),
    "P64-auto": ("P64", 128, {}, "h16 own choice, 64 x 64 slices"),
    "P64-hub-2": ("P64", 128, dict(HUB_ENV, SPARTA_HUB_G="2"), "h16 hub G=2"),
    "P64-hub-4": ("P64", 128, dict(HUB_ENV, SPARTA_HUB_G="4"), "h16 hub G=4"),
    "P64-slab-256": ("P64", 256, {}, "h16 own choice, 256-column slab"),
    "P64-lds-256": ("P64", 256, {"SPARTA_H16_PATH": "lds"}, "h16 lds kernel, n = 256"),
}


@pytest.mark.parametrize("config", list(H16_CONFIGS))
@pytest.mark.parametrize("dtype", H16, ids=["f16", "bf16"])
def test_forward_h16(dtype, config, monkeypatch):
    key, n, env, carrier = H16_CONFIGS[config]
    monkeypatch.setenv("SPARTA_SPARSE_K", "0")
    setenv(monkeypatch, env)
    a = U.accuracy_set(("fwd", key, dtype, "wide", n))
    v = a["v"]
    d = vbr_of(v, a["mab"]).to_device(0, dtype=dtype)
    try:
        info, hi = d.info(), d.hub_info()
        assert d.sparse_info()["rows"] == 0 and info["stream_steps"] + hi["steps"] > 0, info
        if key == "P32":
            assert (info["stream_steps"] < int(v.nzcount.sum())) == ("no-pairs" not in config), info
        if "hub" in config:
            assert hi["steps"] > 0 and hi["tiles_per_group"] == int(config[-1]), hi
        else:
            assert hi["steps"] == 0, hi
        carrier = "%s %s" % (DT_ID[dtype], carrier)
        for c_row, acc in ((False, False), (True, True)):
            C0 = a["C0"] if acc else None
            got = spmm(d, v.rows, v.cols, a["R"], n, dtype, False, c_row, C0)
            assert PATH_NAME[d.info()["last_path"]] == "stream", d.info()
            check_bound(got, a["L"], a["R"], C0, carrier, exact_single=True)
        # host pointers: the library converts the fp32 B on the device (the values are representable: the conversion must not change them)
        Bh = np.ascontiguousarray(a["R"].T, np.float32).reshape(-1)
        for acc in (False, True):
            Ch = np.ascontiguousarray(a["C0"].T, np.float32).reshape(-1).copy() if acc else np.full(v.rows * n, np.nan, np.float32)
            d.spmm_host(Bh, n, Ch, accumulate=acc)
            check_bound(Ch.reshape(n, v.rows).T, a["L"], a["R"], a["C0"] if acc else None, carrier + ", host B", exact_single=True)
    finally:
        d.close()


# ---- 3. bound: the sparse path and relatives (handles made from a CSR) ------------------------------------------------------------------------------------------
CSR_MODES = {          # mode -> (matrix, environment, (dtype, n) list)
    "short-rows-and-segments": ("PCSR", {"SPARTA_COLRES": "0", "SPARTA_SPARSE_SEG": "8"}, ((sa.F32, 40), (sa.F32, 128), (sa.BF16, 128))),
    "in-place-column-major-b": ("PCSR9", {"SPARTA_COLRES": "0"}, ((sa.F32, 128), (sa.BF16, 128))),
    "windows": ("PCSR", {"SPARTA_COLRES": "0", "SPARTA_SP_WINDOW_COLS": "64", "SPARTA_SP_LONG": "8", "SPARTA_SP_MINSEG": "1"}, ((sa.F32, 128), (sa.BF16, 128))),
    "resident-columns": ("PCSR", {}, ((sa.F32, 8),)),
    "tiles-and-sparse-rows": ("PSPLIT", {"SPARTA_COLRES": "0", "SPARTA_UNION": "0", "SPARTA_SPARSE_K_BLOCK": "8"}, ((sa.F32, 128), (sa.BF16, 128))),
    "union-tiles": ("PUNI", {"SPARTA_COLRES": "0"}, ((sa.F32, 128), (sa.BF16, 128))),
}
CSR_CASES = [(mode, dt, n) for mode, (_, _, dn) in CSR_MODES.items() for dt, n in dn]


def csr_handle(a, dtype, mode):
    """the handle of the input set a, with the plan of `mode` asserted from its records"""
    m = a["m"]
    d = sa.DeviceVBS.from_csr(m, a["g"], a["w"], device=0, dtype=dtype)
    sp, ui, info = d.sparse_info(), d.union_info(), d.info()
    tiles, nnz = info["tiles16"] + info["tiles32"] + info["tiles64"], int((m.vals != 0).sum())
    try:
        if mode in ("short-rows-and-segments", "windows", "resident-columns", "in-place-column-major-b"):
            assert sp["rows"] > 0 and sp["nnz"] == nnz and tiles == 0 and ui["nnz"] == 0 and sp["short_rows"] > 0, (sp, ui, info)
        if mode in ("short-rows-and-segments", "windows"):
            assert sp["hub_rows"] > 0, sp
        if mode == "in-place-column-major-b":          # the rule of sparta_vbs_spmm for reading a column-major B where it lies (as in tests/test_spmm_gpu.py): few sparse nonzeros
            assert 0 < sp["nnz"] * 8 < m.cols, sp
        else:
            assert sp["nnz"] * 8 >= m.cols or sp["nnz"] == 0, sp
        if mode == "tiles-and-sparse-rows":
            assert tiles > 0 and 0 < sp["nnz"] < nnz and ui["nnz"] == 0, (sp, ui, info)
        if mode == "union-tiles":
            assert ui["tiles32"] + ui["tiles64"] > 0 and ui["nnz"] > 0 and tiles == 0, (sp, ui, info)
        assert (d.colres_info()["slices"] > 0) == (mode == "resident-columns"), d.colres_info()
    except AssertionError:
        d.close()
        raise
    return d


@pytest.mark.parametrize("mode,dtype,n", CSR_CASES, ids=["%s-%s-n%d" % (mode, DT_ID[dt], n) for mode, dt, n in CSR_CASES])
def test_forward_from_csr(mode, dtype, n, monkeypatch):
    """short rows with long rows cut into segments, a column-major B read in place (PCSR9: so few sparse nonzeros that transposing B would cost more), the
    window plan, the resident-column kernel, tiles + sparse rows that add, union tiles"""
    monkeypatch.setenv("SPARTA_SPARSE_MIN_STEPS", "0")
    monkeypatch.setenv("SPARTA_LAUNCH_NNZ", "0")
    which, env, _ = CSR_MODES[mode]
    setenv(monkeypatch, env)
    a = U.accuracy_set(("csr", which, dtype, "wide", n))
    d = csr_handle(a, dtype, mode)
    try:
        rows, cols = a["L"].shape
        for b_row, c_row, acc in [(False, False, False), (False, True, True)] if dtype != sa.F32 or mode == "in-place-column-major-b" else LAYOUTS:
            C0 = a["C0"] if acc else None
            got = spmm(d, rows, cols, a["R"], n, dtype, b_row, c_row, C0)
            nc = d.colres_info()["nc"]
            if mode == "resident-columns" and not (b_row or c_row):          # (the resident-column kernel takes the reference's layouts)
                assert nc > 0, d.colres_info()
            if mode != "resident-columns":
                assert nc == 0, d.colres_info()
            check_bound(got, a["L"], a["R"], C0, "%s %s%s" % (DT_ID[dtype], mode, " (row gather)" if mode == "resident-columns" and nc == 0 else ""), exact_single=dtype != sa.F32)
    finally:
        d.close()


# ---- 4. bound: gathered and prepared B, B x A ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,dtype", [("P32G", sa.F32), ("P64G", sa.BF16)], ids=["P32G-f32", "P64G-bf16"])
def test_gathered_and_prepared_b(key, dtype, monkeypatch):
    monkeypatch.setenv("SPARTA_SPARSE_K", "0")
    n = 128
    a = U.accuracy_set(("fwd", key, dtype, "wide", n))
    v = a["v"]
    d = vbr_of(v, a["mab"]).to_device(0, dtype=dtype)
    try:
        want_path = f32_paths(d, v, n, None) if dtype == sa.F32 else {"stream"}
        shard_rows = v.cols // 2
        shard_ld = shard_rows + 8
        stride = shard_ld * n + 72
        Bd = gathered_image(a["R"], shard_rows, shard_ld, stride, dtype)
        Cd = out_tensor(v.rows, n, False, None)
        d.spmm_gathered(Bd, shard_rows, Cd, n, shard_stride=stride, shard_ld=shard_ld)
        torch.cuda.synchronize()
        assert PATH_NAME[d.info()["last_path"]] in want_path, d.info()
        check_bound(read_out(Cd, v.rows, n, False), a["L"], a["R"], None, "%s gathered B, %s" % (DT_ID[dtype], PATH_NAME[d.info()["last_path"]]), exact_single=dtype != sa.F32)
        ldb = ld_of(v.cols, 3, dtype)
        Bd = dev_in(a["R"], ldb, dtype)
        P = d.prepare_b(Bd, n, ldb=ldb)
        try:
            Cd = out_tensor(v.rows, n, False, a["C0"])
            d.spmm_prepared(P, Cd, accumulate=True)
            torch.cuda.synchronize()
            assert PATH_NAME[d.info()["last_path"]] in want_path, d.info()
            check_bound(read_out(Cd, v.rows, n, False), a["L"], a["R"], a["C0"], "%s prepared B, %s" % (DT_ID[dtype], PATH_NAME[d.info()["last_path"]]), exact_single=dtype != sa.F32)
        finally:
            P.close()
    finally:
        d.close()


def test_spmm_ba():
    """C = B A on the handle of A^T.  sparta_vbs_create_transposed drops the exact zeros of the blocks, so A is dense inside its blocks here (the transposed
    handle keeps tiles, as in tests/test_poison_gpu.py) and the short sums come from B: column j of B^T holds 1, 2, 3, 4, 8 or all of its rows"""
    a = U.accuracy_set(("ba", "P32", 0, "wide", 128))
    v, M = a["v"], 128
    d = sa.DeviceVBS.transposed_of(vbr_of(v, a["mab"]), device=0)
    try:
        info, sp, ui = d.info(), d.sparse_info(), d.union_info()
        assert info["tiles16"] + info["tiles32"] + info["tiles64"] > 0 and sp["rows"] == 0 and ui["nnz"] == 0, (info, sp, ui)
        want_path = "stream" if info["stream_workers"] > 0 else "generic"
        for acc in (False, True):
            Ch = np.ascontiguousarray(a["C0"], np.float32).reshape(-1).copy() if acc else np.full(M * v.cols, np.nan, np.float32)
            d.spmm_BA_host(np.ascontiguousarray(a["R"], np.float32).reshape(-1), M, Ch, accumulate=acc)
            assert PATH_NAME[d.info()["last_path"]] == want_path, d.info()
            check_bound(Ch.reshape(v.cols, M), a["L"], a["R"], a["C0"] if acc else None, "spmm_ba f32, tiles of the transposed handle, %s" % want_path)
    finally:
        d.close()


# ---- 5. bound: the training entry points ---------------------------------------------------------------------------------------------------------------
TRAIN = [("P32", sa.F32), ("P13", sa.F32), ("P64", sa.F16), ("P32", sa.BF16)]
TRAIN_IDS = ["%s-%s" % (k, DT_ID[dt]) for k, dt in TRAIN]


def run_spmm_t(d, v, X, n, dtype, C0=None):
    ldx = ld_of(v.rows, 5, dtype)
    Cd = out_tensor(v.cols, n, False, C0)
    d.spmm_t(dev_in(X, ldx, dtype), Cd, n, accumulate=C0 is not None, ldx=ldx)
    torch.cuda.synchronize()
    return read_out(Cd, v.cols, n, False)


def run_sddmm(d, v, X, Y, k, dtype, G0=None):
    ldx, ldy = ld_of(v.rows, 5, dtype), ld_of(v.cols, 3, dtype)
    Gd = torch.from_numpy(np.full(len(v.mab), np.nan, np.float32) if G0 is None else np.ascontiguousarray(G0, np.float32)).cuda()
    d.sddmm(dev_in(X, ldx, dtype), dev_in(Y, ldy, dtype), Gd, k, accumulate=G0 is not None, ldx=ldx, ldy=ldy)
    torch.cuda.synchronize()
    return Gd.cpu().numpy()


def dense_of_g(v, G):
    """the mab-layout G as a dense rows x cols matrix (0 outside the stored blocks) and the values of its positions past cols"""
    inside = U.edge_sample(v, np.ones((v.rows, v.cols))) != 0
    return U.edge_dense(v, mab=G.astype(np.float32)), G[~inside]


@pytest.mark.parametrize("key,dtype", TRAIN, ids=TRAIN_IDS)
def test_spmm_t(key, dtype):
    a = U.accuracy_set(("t", key, dtype, "wide", 128))
    v = a["v"]
    d = vbr_of(v, a["mab"]).to_device(0, dtype=dtype, transposable=True)
    try:
        for acc in (False, True):
            C0 = a["C0"] if acc else None
            check_bound(run_spmm_t(d, v, a["R"], 128, dtype, C0), a["L"], a["R"], C0, "spmm_t %s" % DT_ID[dtype], exact_single=dtype != sa.F32)
    finally:
        d.close()


@pytest.mark.parametrize("k", [128, 37])
@pytest.mark.parametrize("key,dtype", TRAIN, ids=TRAIN_IDS)
def test_sddmm(key, dtype, k):
    """X and Y sparse in k: a row holds 1, 3 or all of the k columns"""
    a = U.accuracy_set(("sddmm", key, dtype, "wide", k))
    v = a["v"]
    d = vbr_of(v, a["mab"]).to_device(0, dtype=dtype)
    try:
        for acc in (False, True):
            C0 = a["C0"] * a["check"] if acc else None          # (the previous G, dense; 0 outside the stored blocks)
            G0 = None if C0 is None else U.edge_sample(v, C0)
            got, past = dense_of_g(v, run_sddmm(d, v, a["X"], a["Y"], k, dtype, G0))
            assert (past == 0).all(), "positions past cols are not 0"
            check_bound(got, a["L"], a["R"], C0, "sddmm %s k=%d" % (DT_ID[dtype], k), mask=a["check"], exact_single=dtype != sa.F32)
    finally:
        d.close()


SET_VALUES = [("P32", sa.F32, "stream", 128), ("P64", sa.F32, "class", 128), ("P13", sa.F32, None, 130), ("P32", sa.F16, None, 128), ("P64", sa.BF16, None, 128)]


@pytest.mark.parametrize("key,dtype,forced,n", SET_VALUES, ids=["%s-%s-%s" % (k, DT_ID[dt], f or "own-choice") for k, dt, f, _ in SET_VALUES])
def test_forward_after_set_values(key, dtype, forced, n, monkeypatch):
    """an updatable handle created from the poison geometry's own values, given the accuracy values through sparta_vbs_set_values"""
    if forced:
        monkeypatch.setenv("SPARTA_PATH", forced)
    a = U.accuracy_set(("fwd", key, dtype, "wide", n))
    v = a["v"]
    d = v.to_device(0, dtype=dtype, updatable=True)
    try:
        d.set_values(torch.from_numpy(np.array(a["mab"])).cuda())
        got = spmm(d, v.rows, v.cols, a["R"], n, dtype)
        carried = PATH_NAME[d.info()["last_path"]]
        assert carried in (f32_paths(d, v, n, forced) if dtype == sa.F32 else {"stream"}) and (forced is None or carried == {"stream": "stream", "class": "per-class"}[forced]), d.info()
        check_bound(got, a["L"], a["R"], None, "forward after set_values, %s %s" % (DT_ID[dtype], carried), exact_single=dtype != sa.F32)
    finally:
        d.close()


# ---- 6. exact: powers of two and negation commute with every product ------------------------------------------------------------------------------------------
SCALES = ((5, -3), (-6, 0), (0, 7))
SCALING = [("P32", sa.F32, "stream"), ("P64", sa.F32, "class"), ("P13", sa.F32, "generic"), ("w128h20", sa.F32, "stream"), ("w128h80", sa.F32, "stream"),
           ("P32", sa.F16, None), ("P64", sa.BF16, None), ("P64", sa.BF16, "hub"), ("w256", sa.BF16, None)]


def negated(x):
    """-x as a kernel that starts its sums from +0 gives it: an element without a non-zero product, or whose products cancel, is +0 for -A as for A ((+0) + (-0) = +0)"""
    return np.where(x == 0, np.float32(0.0), -x)


def same_bits(x, y):
    return np.array_equal(np.ascontiguousarray(x, np.float32).view(np.uint32), np.ascontiguousarray(y, np.float32).view(np.uint32))


@pytest.mark.parametrize("key,dtype,forced", SCALING, ids=["%s-%s-%s" % (k, DT_ID[dt], f or "own-choice") for k, dt, f in SCALING])
def test_scaling_and_negation_are_exact(key, dtype, forced, monkeypatch):
    """C(2^s A, 2^t B) == 2^(s + t) C(A, B) and C(-A, B) == -C(A, B), bit for bit, on ONE updatable handle (A through set_values, B scaled on the device):
    unit-range operands, so nothing leaves the normal range.  fp32 handles force SPARTA_PATH: no autotune choice comes between two calls."""
    monkeypatch.setenv("SPARTA_SPARSE_K", "0")
    if forced == "hub":                               # (16-bit: the hub plan, forced onto this small matrix at creation)
        setenv(monkeypatch, dict(HUB_ENV, SPARTA_HUB_G="2"))
    elif forced:
        monkeypatch.setenv("SPARTA_PATH", forced)
    n = 128
    a = U.accuracy_set(("fwd", key, dtype, "unit", n))
    v, mab = a["v"], np.array(a["mab"])
    d = vbr_of(v, mab).to_device(0, dtype=dtype, updatable=True)
    try:
        assert dtype == sa.F32 or (d.hub_info()["steps"] > 0) == (forced == "hub"), d.hub_info()
        ldb = ld_of(v.cols, 3, dtype)
        Bd = dev_in(a["R"], ldb, dtype)

        def product(Bd_):
            Cd = out_tensor(v.rows, n, False, None)
            d.spmm(Bd_, Cd, n, ldb=ldb)
            torch.cuda.synchronize()
            carried = PATH_NAME[d.info()["last_path"]]
            assert carried == {"stream": "stream", "class": "per-class", "generic": "generic"}.get(forced, "stream"), (carried, d.info())
            return Cd.cpu().numpy()
        base = product(Bd)
        check_bound(read_out(torch.from_numpy(base), v.rows, n, False), a["L"], a["R"], None, "unit operands, %s %s %s" % (key, DT_ID[dtype], forced or "stream"))
        for s, t in SCALES:
            d.set_values(torch.from_numpy(mab * np.float32(2.0 ** s)).cuda())
            assert same_bits(product(Bd * (2.0 ** t)), base * np.float32(2.0 ** (s + t))), (key, DT_ID[dtype], forced, "scaling", s, t)
        d.set_values(torch.from_numpy(-mab).cuda())
        assert same_bits(product(Bd), negated(base)), (key, DT_ID[dtype], forced, "negation")
    finally:
        d.close()


@pytest.mark.parametrize("key,dtype", TRAIN, ids=TRAIN_IDS)
def test_scaling_and_negation_are_exact_spmm_t_and_sddmm(key, dtype):
    n = 128
    a, g = U.accuracy_set(("t", key, dtype, "unit", n)), U.accuracy_set(("sddmm", key, dtype, "unit", n))
    v, mab = a["v"], np.array(a["mab"])
    d = vbr_of(v, mab).to_device(0, dtype=dtype, updatable=True, transposable=True)
    try:
        base = run_spmm_t(d, v, a["R"], n, dtype)
        baseG = run_sddmm(d, v, g["X"], g["Y"], n, dtype)
        assert np.isfinite(base).all() and np.isfinite(baseG).all()
        for s, t in SCALES:
            d.set_values(torch.from_numpy(mab * np.float32(2.0 ** s)).cuda())
            assert same_bits(run_spmm_t(d, v, a["R"] * 2.0 ** t, n, dtype), base * np.float32(2.0 ** (s + t))), (key, DT_ID[dtype], "spmm_t scaling", s, t)
            assert same_bits(run_sddmm(d, v, g["X"] * 2.0 ** s, g["Y"] * 2.0 ** t, n, dtype), baseG * np.float32(2.0 ** (s + t))), (key, DT_ID[dtype], "sddmm scaling", s, t)
        d.set_values(torch.from_numpy(-mab).cuda())
        assert same_bits(run_spmm_t(d, v, a["R"], n, dtype), negated(base)), (key, DT_ID[dtype], "spmm_t negation")
        assert same_bits(run_sddmm(d, v, -g["X"], g["Y"], n, dtype), negated(baseG)), (key, DT_ID[dtype], "sddmm negation")
    finally:
        d.close()


# ---- 7. exact: the stored 16-bit image, read back ------------------------------------------------------------------------------------------------------------
CSTAR = 2          # the block column that holds the special values (and nothing else)
SPECIAL = U.ACC_SPECIALS


def same_values(got, want):
    """bit for bit up to the payload of a NaN and the sign of a zero: NaN where NaN is wanted, else the same value.  (The read-back is a sum, x * 1 + 0 * 0 + ...,
    and (-0) + (+0) = +0: a stored -0 comes back as +0, so the sign of a zero -- alone among the special values -- is not observable this way.)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nn = ~np.isnan(want)
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[nn], want[nn])


def cstar_blocks(v):
    w = int(v.block_col_size)
    return [(off, r0, h, valid) for off, r0, h, c0, valid in U.edge_blocks(v) if c0 == CSTAR * w and h > 0]


def special_mab(v, dtype, one_hot=False):
    """(mab, rows, qs, values): ordinary unit values everywhere, except the blocks of block column CSTAR, where row i holds ONE non-zero, at stored column
    q: a special value (one_hot: 1.0 at q = i % valid and 0.0 everywhere else: C = A B then copies rows of B).  The N special values that the storage type
    holds as Inf or NaN go to the first N rows, the t-th to stored column q = t, which holds nothing else; every other row takes the finite ones in turn, in
    the columns q >= N.  A non-finite value then shares neither its row nor its column with another special value: it reaches the outputs of its own row
    (forward) and column (spmm_t) only, as the dependency contract allows, and every element read back is x * 1 + 0 * (finite values)."""
    w = int(v.block_col_size)
    mab = U.accuracy_draw(np.random.default_rng(77), len(v.mab), "unit", dtype).astype(np.float32) * np.float32(0.0 if one_hot else 1.0)
    finite = np.isfinite(U.edge_round(SPECIAL, dtype))
    fin, nonfin = SPECIAL[finite], list(SPECIAL[~finite])
    rows, qs, vals, N = [], [], [], len(nonfin)
    for off, r0, h, valid in cstar_blocks(v):
        assert valid > N
        mab[off:off + w * h] = 0.0
        for i in range(h):
            if one_hot:
                q, x = (r0 + i) % valid, np.float32(1.0)
            elif nonfin:
                q, x = N - len(nonfin), nonfin.pop(0)
            else:
                q, x = N + (r0 + i) % (valid - N), fin[(r0 + i) % len(fin)]
            mab[off + q * h + i] = x
            rows.append(r0 + i); qs.append(q); vals.append(x)
    assert one_hot or (not nonfin and len(set(np.array(vals, np.float32).view(np.uint32).tolist())) == len(SPECIAL)), "a special value found no row"
    return mab, np.array(rows), np.array(qs), np.array(vals, np.float32)


def read_back_forward(d, v, dtype, n=128):
    """C = A E with E[CSTAR w + q, j] = 1 for j % w == q and 0 elsewhere: C[i, j] = A[i, CSTAR w + j % w] as the handle holds it"""
    w = int(v.block_col_size)
    E = np.zeros((v.cols, n))
    for j in range(n):
        E[CSTAR * w + j % w, j] = 1.0
    return spmm(d, v.rows, v.cols, E, n, dtype)


def read_back_t(d, v, dtype):
    """Ct = A^T E with E = the first n columns of the identity: Ct[c, j] = A[j, c] as the spmm_t image holds it"""
    n = min(v.rows, 256)
    return run_spmm_t(d, v, np.eye(v.rows, n), n, dtype), n


IMAGES = {          # name -> (geometry, environment): the slice shapes (tile rows x k depth) of the 16-bit images that hold the special values, and the hub image
    # P32 with the pair plan: block column CSTAR is stored by the pairs (0, 1), (2, 3), (4, 5) and the 64-row block-row 6 -- 64 x 32 slices only (block-row 7, the
    # one <= 32-row tile left, does not store it).  Without pairs: the 32-row block-rows 0, 1, 3, 4, 5 in 32 x 32 slices, next to block-row 6
    "64x32-pair-tiles": ("P32", {}), "32x32-no-pairs": ("P32", {"SPARTA_H16_PAIR": "0"}), "64x64": ("P64", {}), "hub": ("P64", dict(HUB_ENV, SPARTA_HUB_G="2")), "32x64": ("w128h20", {}),
}


def assert_image_shape(d, v, image):
    """the plan that gives the image its slice shapes, from the handle's records (tiles16 / tiles32 / tiles64: block-rows of <= 16, <= 32 and <= 64 rows)"""
    info, hi = d.info(), d.hub_info()
    small, big, paired = info["tiles16"] + info["tiles32"], info["tiles64"], info["stream_steps"] < int(v.nzcount.sum())
    assert (hi["steps"] > 0) == (image == "hub"), hi
    assert int(v.block_col_size) % 64 == (32 if image in ("64x32-pair-tiles", "32x32-no-pairs") else 0)          # the k depth of a slice: 64 where w allows
    if image == "64x32-pair-tiles":
        assert paired and info["stream_steps"] > 0, info
    if image == "32x32-no-pairs":
        assert not paired and small >= 5 and big >= 1, info
    if image in ("64x64", "hub"):
        assert small == 0 and big > 0, info
    if image == "32x64":
        assert big == 0 and small > 0, info


@pytest.mark.parametrize("how", ["creation", "set_values"])
@pytest.mark.parametrize("image", list(IMAGES))
@pytest.mark.parametrize("dtype", H16, ids=["f16", "bf16"])
def test_stored_image_is_round_to_nearest_even(dtype, image, how, monkeypatch):
    """the values a 16-bit handle holds after creation (to_h16) and after sparta_vbs_set_values (vbs_update_h16_kernel; the spmm_t image: vbs_spmm_t_image_kernel),
    read back through one-hot columns of B / X and compared with edge_round on the special values: ties, the largest finite values, the fp16 threshold to Inf,
    subnormals, signed zeros, NaNs with only low mantissa bits set, Inf"""
    key, env = IMAGES[image]
    monkeypatch.setenv("SPARTA_SPARSE_K", "0")
    setenv(monkeypatch, env)
    v = (U.poison_geometries() if key.startswith("P") else U.train_geometries())[key]
    mab, rows, qs, vals = special_mab(v, dtype)
    w = int(v.block_col_size)
    if how == "creation":
        d = vbr_of(v, mab).to_device(0, dtype=dtype, transposable=True)
    else:
        d = vbr_of(v, U.accuracy_draw(np.random.default_rng(78), len(v.mab), "unit", dtype)).to_device(0, dtype=dtype, updatable=True, transposable=True)
    try:
        if how == "set_values":
            d.set_values(torch.from_numpy(mab).cuda())
        assert_image_shape(d, v, image)
        want = U.edge_round(vals, dtype)
        C = read_back_forward(d, v, dtype)
        got = np.array([C[i, q] for i, q in zip(rows, qs)])          # (column j = q < w <= 128 reads stored column q)
        bad = [(float(vals[t]), float(got[t]), float(want[t])) for t in range(len(vals)) if not same_values(got[t:t + 1], want[t:t + 1])]
        assert not bad, (DT_ID[dtype], image, how, "forward image: (input, held, wanted)", bad[:8])
        Ct, n = read_back_t(d, v, dtype)
        sel = rows < n
        got = np.array([Ct[CSTAR * w + q, i] for i, q in zip(rows[sel], qs[sel])])
        bad = [(float(x), float(g_), float(w_)) for x, g_, w_ in zip(vals[sel], got, want[sel]) if not same_values([g_], [w_])]
        assert len(set(vals[sel].view(np.uint32).tolist())) == len(SPECIAL) and not bad, (DT_ID[dtype], image, how, "spmm_t image: (input, held, wanted)", bad[:8])
    finally:
        d.close()


@pytest.mark.parametrize("key,dtype", [("P32", sa.F16), ("P32", sa.BF16), ("P64", sa.F16), ("P64", sa.BF16)], ids=["P32-f16", "P32-bf16", "P64-f16", "P64-bf16"])
def test_host_operands_are_converted_round_to_nearest_even(key, dtype, monkeypatch):
    """host-pointer fp32 B (sparta_vbs_spmm), X and Y (sparta_vbs_sddmm) on a 16-bit handle (vbs_convert_h16_kernel), read back through one-hot rows of A
    (value 1.0) resp. one-hot rows of the other operand"""
    monkeypatch.setenv("SPARTA_SPARSE_K", "0")
    v = U.poison_geometries()[key]
    w, n = int(v.block_col_size), 128
    mab, rows, qs, _ = special_mab(v, dtype, one_hot=True)
    d = vbr_of(v, mab).to_device(0, dtype=dtype)
    try:
        B = U.accuracy_draw(np.random.default_rng(79), (v.cols, n), "unit", dtype).astype(np.float32)
        for j in range(n):                            # column j holds ONE special value, in row CSTAR w + j % w
            B[CSTAR * w + j % w, j] = SPECIAL[(5 * (j % w) + j // w) % len(SPECIAL)]
        Ch = np.full(v.rows * n, np.nan, np.float32)
        d.spmm_host(np.ascontiguousarray(B.T).reshape(-1), n, Ch, accumulate=False)
        C = Ch.reshape(n, v.rows).T
        js = np.arange(n)
        got = np.array([C[i, j] for i, q in zip(rows, qs) for j in js[js % w == q]])
        src = np.array([B[CSTAR * w + q, j] for i, q in zip(rows, qs) for j in js[js % w == q]], np.float32)
        assert len(set(src.view(np.uint32).tolist())) >= len(SPECIAL) - 2
        bad = [(float(x), float(g_), float(w_)) for x, g_, w_ in zip(src, got, U.edge_round(src, dtype)) if not same_values([g_], [w_])]
        assert not bad, (key, DT_ID[dtype], "host B: (input, held, wanted)", bad[:8])
        # sddmm: G[i, c] = sum_k X[i, k] Y[c, k].  One operand one-hot in k (row r: 1.0 at k = r % kk), the other ordinary with ONE special value per row (row r: at
        # k = r % kk): G[i, c] is that special value where i % kk == c % kk
        kk = 37
        stored = U.stored_mask(v)
        ii, cc = np.nonzero(stored & (np.arange(v.rows)[:, None] % kk == np.arange(v.cols)[None, :] % kk))
        for special_in in ("X", "Y"):
            nr = {"X": v.rows, "Y": v.cols}
            ops = {}
            for name in ("X", "Y"):
                r = np.arange(nr[name])
                if name == special_in:
                    M = U.accuracy_draw(np.random.default_rng(80), (nr[name], kk), "unit", dtype).astype(np.float32)
                    M[r, r % kk] = SPECIAL[r % len(SPECIAL)]
                else:
                    M = np.zeros((nr[name], kk), np.float32)
                    M[r, r % kk] = 1.0
                ops[name] = M
            G = np.full(len(v.mab), np.nan, np.float32)
            d.sddmm_host(np.ascontiguousarray(ops["X"].T).reshape(-1), np.ascontiguousarray(ops["Y"].T).reshape(-1), kk, G, accumulate=False)
            Gd, _ = dense_of_g(v, G)
            src = ops["X"][ii, ii % kk] if special_in == "X" else ops["Y"][cc, cc % kk]
            assert len(set(src.view(np.uint32).tolist())) >= len(SPECIAL) - 2
            bad = [(float(x), float(g_), float(w_)) for x, g_, w_ in zip(src, Gd[ii, cc], U.edge_round(src, dtype)) if not same_values([g_], [w_])]
            assert not bad, (key, DT_ID[dtype], "host %s of sddmm: (input, held, wanted)" % special_in, bad[:8])
    finally:
        d.close()


# ---- 8. exact: subnormals in fp32 -----------------------------------------------------------------------------------------------------------------------
def with_subnormals(L, R, check, on_rows=True):
    """copies of L and R in which two K = 1 elements meet a subnormal: row i0 of L (one non-zero, at k0) becomes 2^-130 -- a subnormal OPERAND for the whole row
    of the output, with R[k0, j0] = 2^100 for one normal result (2^-30) -- and row i1 (one non-zero, at k1) 2^-70 with R[k1, j1] = 2^-70: a subnormal RESULT
    (2^-140).  on_rows=False: the same with the roles of L and R exchanged (columns of R with one non-zero).  Returns (L, R, mask of those elements)."""
    if not on_rows:
        Rt, Lt, sp = with_subnormals(np.ascontiguousarray(R.T), np.ascontiguousarray(L.T), np.ascontiguousarray(check.T))
        return np.ascontiguousarray(Lt.T), np.ascontiguousarray(Rt.T), np.ascontiguousarray(sp.T)
    L, R = L.copy(), R.copy()
    single = np.flatnonzero(((L != 0).sum(axis=1) == 1) & check.any(axis=1))
    i0 = int(single[0])
    k0 = int(np.flatnonzero(L[i0])[0])
    i1 = int(([i for i in single if np.flatnonzero(L[i])[0] != k0] or single[1:])[0])          # (sddmm: every such row has its non-zero in the same k; 2^-130 * 2^-70 is then 0 for any arithmetic)
    k1 = int(np.flatnonzero(L[i1])[0])
    j0 = int(np.flatnonzero(check[i0] & (R[k0] != 0))[0])
    j1 = int(np.flatnonzero(check[i1] & (R[k1] != 0))[-1])
    assert i1 != i0 and (k1 != k0 or j1 != j0)
    L[i0, k0], R[k0, j0] = 2.0 ** -130, 2.0 ** 100
    L[i1, k1], R[k1, j1] = 2.0 ** -70, 2.0 ** -70
    sp = np.zeros(check.shape, bool)
    sp[i0] = check[i0] & (R[k0] != 0)
    sp[i1, j1] = True
    return L, R, sp


def check_subnormals(got, L, R, sp, carrier, mask=None):
    """the elements of sp: gradual underflow, i.e. the correctly rounded fp32 product (what the CPU's multiply gives); every other element: the bound"""
    check_bound(got, L, R, None, carrier + ", next to subnormals", mask=mask, special=sp)
    want = fl32(L @ R)                                # (one product per element of sp: L @ R is exact in float64, then rounded once, into the subnormal range)
    assert ((np.abs(want[sp]) < 2.0 ** -126) & (want[sp] != 0)).sum() >= 2
    flushed = int((got[sp] == 0).sum())
    assert same_bits(got[sp], want[sp]), (carrier, "%d of %d products with a subnormal operand or result differ from the gradual-underflow value, %d of them are 0" % (
        int((got[sp].astype(np.float64) != want[sp]).sum()), int(sp.sum()), flushed))


@pytest.mark.parametrize("key,forced", [("P32", "stream"), ("P64", "class"), ("P13", "generic")], ids=["stream", "per-class", "generic"])
def test_subnormals_f32_tiles(key, forced, monkeypatch):
    monkeypatch.setenv("SPARTA_SPARSE_K", "0")
    monkeypatch.setenv("SPARTA_PATH", forced)
    a = U.accuracy_set(("fwd", key, 0, "unit", 128))
    v = a["v"]
    L, R, sp = with_subnormals(a["L"], a["R"], a["check"])
    d = vbr_of(v, U.edge_sample(v, L)).to_device(0)
    try:
        got = spmm(d, v.rows, v.cols, R, 128, sa.F32)
        carried = PATH_NAME[d.info()["last_path"]]
        assert carried == {"stream": "stream", "class": "per-class", "generic": "generic"}[forced], d.info()
        check_subnormals(got, L, R, sp, "forward f32 %s" % carried)
    finally:
        d.close()


@pytest.mark.parametrize("mode,n", [("short-rows-and-segments", 128), ("resident-columns", 8), ("union-tiles", 128)])
def test_subnormals_f32_from_csr(mode, n, monkeypatch):
    monkeypatch.setenv("SPARTA_SPARSE_MIN_STEPS", "0")
    monkeypatch.setenv("SPARTA_LAUNCH_NNZ", "0")
    which, env, _ = CSR_MODES[mode]
    setenv(monkeypatch, env)
    a = U.accuracy_set(("csr", which, 0, "wide", n))
    m, g = a["m"], a["g"]
    L, R, sp = with_subnormals(a["L"], a["R"], a["check"])
    perm = np.asarray(sa.get_permutation(g), np.int64)
    vals = m.vals.copy()
    for i, k in np.argwhere(L != a["L"]):
        r = int(perm[i])
        at = int(m.rowptr[r]) + int(np.searchsorted(m.colidx[m.rowptr[r]:m.rowptr[r + 1]], k))
        assert m.colidx[at] == k
        vals[at] = L[i, k]
    b = dict(a, m=sa.CSR(m.rows, m.cols, m.rowptr, m.colidx, vals))
    d = csr_handle(b, sa.F32, mode)
    try:
        got = spmm(d, L.shape[0], L.shape[1], R, n, sa.F32)
        assert (d.colres_info()["nc"] > 0) == (mode == "resident-columns"), d.colres_info()
        check_subnormals(got, L, R, sp, "f32 %s" % mode)
    finally:
        d.close()


def test_subnormals_f32_spmm_t_and_sddmm():
    a, g = U.accuracy_set(("t", "P32", 0, "unit", 128)), U.accuracy_set(("sddmm", "P32", 0, "unit", 128))
    v = a["v"]
    L, R, sp = with_subnormals(a["L"], a["R"], a["check"], on_rows=False)          # (the columns of X with one non-zero row)
    d = vbr_of(v, U.edge_sample(v, np.ascontiguousarray(L.T))).to_device(0, transposable=True)
    try:
        check_subnormals(run_spmm_t(d, v, R, 128, sa.F32), L, R, sp, "spmm_t f32")
        X, Yt, spg = with_subnormals(g["L"], g["R"], g["check"])
        got, _ = dense_of_g(v, run_sddmm(d, v, X, np.ascontiguousarray(Yt.T), 128, sa.F32))
        check_subnormals(got, X, Yt, spg, "sddmm f32 k=128", mask=g["check"])
    finally:
        d.close()
