"""The training entry points -- sparta_vbs_sddmm, sparta_vbs_set_values, sparta_vbs_spmm_t, sparta_amd.autograd.vbs_linear -- at the block widths, block-row
heights and forward product paths their own files (one fixture set: w in {1, 8, 32, 64}, heights 16 .. 48 and ~100) never reach.

Geometries: tests/_util.py: train_geometries() -- one seeded 500 x 1102 matrix with empty rows, w in {3, 13, 48, 96, 100, 128, 200, 256}, heights 1 .. 200 and 0,
a ragged last block column at every w.  Oracles: the float64 restatements of tests/test_sddmm_gpu.py, test_set_values_gpu.py and test_spmm_t_gpu.py, imported.
Integer data lies in -4 .. 4: every partial sum is an integer below 16 * 1102 < 2^24 and every value is exact in f16 / bf16, so the kernels must equal the
float64 oracle cast to float32 bit for bit.  Random data: |got - ref| <= 1e-5 * sum|a||b| (16-bit handles: against the oracle on the rounded inputs).

After sparta_vbs_set_values EVERY image of the handle is read: an fp32 forward product is forced onto each of its paths (SPARTA_PATH, read per call) in two
orders, the 16-bit one onto each of its kernels (SPARTA_H16_PATH / SPARTA_H16_DEPTH); the last test reports which path carried which product and fails when one
of the three fp32 paths carried none."""
import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd.autograd import vbs_linear

torch = pytest.importorskip("torch")

import _util as U  # noqa: E402
from test_sddmm_gpu import oracle as sddmm_oracle, operands as sd_operands, run as sd_run, check_close as sd_check_close  # noqa: E402
from test_set_values_gpu import DT_ID, values, oracle as fwd_oracle, dense_b, product, rounded, put  # noqa: E402
from test_spmm_t_gpu import oracle as t_oracle, run_t, dense_x, with_values, check_close as t_check_close  # noqa: E402
from test_vbs_linear_gpu import check_linear, operands as linear_operands, positions, dev  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(k, sa.F32) for k in U.TRAIN_F32] + [(k, dt) for dt in (sa.F16, sa.BF16) for k in U.TRAIN_H16]
CASE_IDS = ["%s-%s" % (k, DT_ID[dt]) for k, dt in CASES]
both = pytest.mark.parametrize("key,dtype", CASES, ids=CASE_IDS)

_HANDLES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for d in _HANDLES.values():
        d.close()
    _HANDLES.clear()


def geometry(key):
    return U.train_geometries()[key]


def handle(key, dtype, tag="plain", mab=None, **flags):
    """one handle per (geometry, dtype, flags, values) for the module; mab None: the matrix's own values"""
    k = (key, dtype, tag, tuple(sorted(flags.items())))
    if k not in _HANDLES:
        v = geometry(key)
        _HANDLES[k] = (v if mab is None else with_values(v, mab)).to_device(0, dtype=dtype, **flags)
    return _HANDLES[k]


def nonzero_integers(shape, seed):
    x = np.random.default_rng(seed).integers(-4, 5, shape).astype(np.float64)
    x[x == 0] = 3.0
    return x


def test_the_geometries_are_what_the_table_says():
    g = U.train_geometries()
    hts = {k: np.diff(v.row_part) for k, v in g.items()}
    assert hts["w13h1"].max() == 1 and (g["w13h1"].nzcount == 0).sum() == 35                   # every empty row is a block-row without a block
    assert (g["w3"].nzcount == 0).sum() == 2 and (g["w96"].nzcount == 0).sum() == 1
    assert hts["w100h200"].tolist() == [200, 200, 100] and set(hts["w128"]) == {100}
    assert set(hts["w128h20"]) == {20} and hts["w128h80"].tolist() == [80] * 6 + [20]
    assert (hts["w13z"] == 0).sum() == 2 and hts["w13z"][15] == hts["w13z"][16] == 0
    tall = hts["w200"][g["w200"].nzcount > 0]
    assert tall.max() > 128 and len(set(tall)) >= 3                                             # ragged: several different heights, one above 128
    assert set(hts["w96"]) == {20} and set(hts["w256"]) == {40, 20}
    for k, v in g.items():
        assert v.nzcount[v.nzcount > 0].min() >= 2, k                                           # several blocks in every block-row that has any
        assert (positions(k, v)[1] < 0).any(), k                                                # stored positions past cols exist


# ---- 1. SDDMM -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 33, 130])
@both
def test_sddmm_integer_bit_exact(key, dtype, k):
    """k = 130 on a 16-bit handle: ldy = 1102, not a multiple of 8 -- Y is gathered column by column; k = 1, 33: ldy = 1104, 16-byte loads of Y"""
    v = geometry(key)
    X, Y = sd_operands(v, k, seed=1000 + k, integer=True)
    G, _, _ = sd_run(handle(key, dtype), X, Y, dtype, ld_mult=2 if k == 130 else 8)         # (G starts as NaN)
    assert np.array_equal(G, sddmm_oracle(v, X, Y).astype(np.float32))
    assert not G[positions(key, v)[1] < 0].any()                                               # the positions past cols of the ragged last block column: 0


@both
def test_sddmm_random_within_bound(key, dtype):
    v = geometry(key)
    X, Y = sd_operands(v, 130, seed=1200, integer=False)
    G, Xr, Yr = sd_run(handle(key, dtype), X, Y, dtype)
    sd_check_close(v, G, Xr, Yr)


@both
def test_sddmm_accumulate_onto_a_nonzero_g(key, dtype):
    v = geometry(key)
    X, Y = sd_operands(v, 33, seed=1300, integer=True)
    G0 = nonzero_integers(int(v.nztot), 1301) * 11.0
    G, _, _ = sd_run(handle(key, dtype), X, Y, dtype, G=G0, accumulate=True)
    assert np.array_equal(G, (G0 + sddmm_oracle(v, X, Y)).astype(np.float32))


# ---- 2. spmm_t ------------------------------------------------------------------------------------------------------------------------------
def t_handle(key, dtype):
    """A non-zero at EVERY stored position, the ones past cols included"""
    v = geometry(key)
    V = nonzero_integers(int(v.nztot), 2000).astype(np.float32)
    return V, handle(key, dtype, "nonzero", V, transposable=True)


@pytest.mark.parametrize("n", [1, 33, 130])
@both
def test_spmm_t_integer_bit_exact(key, dtype, n):
    """A and X non-zero everywhere; run_t pads ldx / ldo and checks the sentinel rows of Ct beyond cols"""
    v = geometry(key)
    V, d = t_handle(key, dtype)
    X = nonzero_integers((v.rows, n), 2100 + n)
    Ct, _ = run_t(d, X, dtype, v.cols)
    assert np.array_equal(Ct, t_oracle(v, V, X).astype(np.float32))


@both
def test_spmm_t_random_within_bound(key, dtype):
    v = geometry(key)
    V = values(v, 22, integer=False)
    d = handle(key, dtype, "random", V, transposable=True)
    Ct, Xr = run_t(d, dense_x(v.rows, 33, 2200, integer=False), dtype, v.cols)
    t_check_close(Ct, v, rounded(V, dtype), Xr, key)


@both
def test_spmm_t_accumulate_adds(key, dtype):
    v = geometry(key)
    V, d = t_handle(key, dtype)
    X = nonzero_integers((v.rows, 33), 2300)
    C0 = nonzero_integers((v.cols, 33), 2301) * 7.0
    Ct, _ = run_t(d, X, dtype, v.cols, Ct0=C0, accumulate=True)
    assert np.array_equal(Ct, (C0 + t_oracle(v, V, X)).astype(np.float32))


# ---- 3. set_values on every image -----------------------------------------------------------------------------------------------------------
CARRIED = {}          # (geometry, dtype, handle flags) -> [(value set, forced path or kernel, info()["last_path"] after the column-major product, after the row-major one)], printed and checked by the last test
PATH_NAME = {0: "none", 1: "stream", 2: "per-class", 3: "generic"}
ORDERS = [(1, ("stream", "class", "generic", None)), (2, ("class", "stream", "generic", None))]
N = 128                # a full slab: the stream and the per-class kernels take whole 128-column slabs only


def check_updated_handle(H, v, V, dtype, seed, what):
    """what is left to check after the forced forward products: spmm_t on the new values (the handle is transposable)"""
    X = dense_x(v.rows, 33, seed, integer=True)
    Ct, _ = run_t(H, X, dtype, v.cols)
    assert np.array_equal(Ct, t_oracle(v, V, X).astype(np.float32)), (what, "spmm_t")


F32_UPD = [(k, True) for k in U.TRAIN_F32] + [(k, False) for k in ("w128", "w128h20", "w128h80")]      # (w % 32 == 0: the geometries with a stream plan)


@pytest.mark.parametrize("key,transposable", F32_UPD, ids=["%s-%s" % (k, "upd+t" if t else "upd") for k, t in F32_UPD])
def test_set_values_reaches_every_image_f32(key, transposable, monkeypatch):
    """The handle is made from the matrix's own values; two integer value sets with different zero patterns (whole columns and whole blocks empty: the fragment
    image compacts them away per step) follow.  After each, the forward product runs on the stream path, the per-class path, the generic path and the handle's
    own choice, the second time per-class first.  The handles that are updatable only (w % 32 == 0) let go of the reference-layout image after a column-major
    product on the stream path, so the two orders rebuild different images; the transposable ones keep both and multiply A^T X as well."""
    monkeypatch.delenv("SPARTA_F32_KEEP_LEGACY", raising=False)
    v = geometry(key)
    w = v.block_col_size
    H = v.to_device(0, updatable=True, transposable=transposable)
    created = H.info()
    if key in ("w128h20", "w128h80"):                                # the two geometries that are here for the fragment image: tiles of <= 32 rows on a stream plan
        assert created["tiles16"] + created["tiles32"] > 0 and created["stream_steps"] > 0, created
    # the path a forced call must end on: the stream plan needs w % 32 == 0, the per-class kernels w % 64 == 0 (N = 128 is a whole slab); else generic
    want = {"stream": (1,) if w % 32 == 0 else (3,), "class": (2,) if w % 64 == 0 else (3,), "generic": (3,), None: (1, 2) if w % 32 == 0 else (3,)}
    log = CARRIED.setdefault((key, "f32", "upd+t" if transposable else "upd"), [])
    for seed, order in ORDERS:
        V = values(v, seed, integer=True)
        put(H, V)
        B = dense_b(v, N, 3000 + seed, integer=True)
        ref = fwd_oracle(v, V, B).astype(np.float32)
        for forced in order:
            if forced is None:
                monkeypatch.delenv("SPARTA_PATH", raising=False)
            else:
                monkeypatch.setenv("SPARTA_PATH", forced)
            C, _ = product(H, v, B, sa.F32)
            p_cm = H.info()["last_path"]
            assert np.array_equal(C, ref), (key, seed, forced, "column-major B")
            C, _ = product(H, v, B, sa.F32, row_major=True)
            p_rm = H.info()["last_path"]
            log.append((seed, forced or "unset", p_cm, p_rm))
            assert np.array_equal(C, ref), (key, seed, forced, "row-major B")
            assert p_cm in want[forced] and p_rm in want[forced], (key, seed, forced, p_cm, p_rm)
        if transposable:
            check_updated_handle(H, v, V, sa.F32, 3100 + seed, (key, seed))
        F = with_values(v, V).to_device(0)
        Ch, _ = product(H, v, B, sa.F32, algo=sa.SPMM_EXACT)
        Cf, _ = product(F, v, B, sa.F32, algo=sa.SPMM_EXACT)
        F.close()
        assert np.array_equal(Ch.view(np.uint32), Cf.view(np.uint32)), (key, seed, "exact-order kernel against a fresh handle")
        assert np.array_equal(Ch, ref), (key, seed, "exact-order kernel")
    H.close()


H16_UPD = [(k, dt) for dt in (sa.F16, sa.BF16) for k in U.TRAIN_H16]


@pytest.mark.parametrize("kernel", ["auto", "lds", "lds-depth4", "direct"])
@pytest.mark.parametrize("key,dtype", H16_UPD, ids=["%s-%s" % (k, DT_ID[dt]) for k, dt in H16_UPD])
def test_set_values_reaches_every_image_h16(key, dtype, kernel, monkeypatch):
    """the 16-bit slices under each kernel that reads them (the selection of test_16bit_storage_vs_oracle_on_rounded_inputs), and the image of spmm_t"""
    if kernel != "auto":
        monkeypatch.setenv("SPARTA_H16_PATH", kernel.split("-")[0])
    if kernel == "lds-depth4":
        monkeypatch.setenv("SPARTA_H16_DEPTH", "4")
    v = geometry(key)
    H = v.to_device(0, dtype=dtype, updatable=True, transposable=True)
    log = CARRIED.setdefault((key, DT_ID[dtype], "upd+t"), [])
    for seed in (1, 2):
        V = values(v, seed, integer=True)
        put(H, V)
        B = dense_b(v, N, 3000 + seed, integer=True)
        C, _ = product(H, v, B, dtype)
        log.append((seed, kernel, H.info()["last_path"], None))
        assert np.array_equal(C, fwd_oracle(v, V, B).astype(np.float32)), (key, seed, kernel)
        check_updated_handle(H, v, V, dtype, 3100 + seed, (key, seed, kernel))
    H.close()


# ---- 4. vbs_linear --------------------------------------------------------------------------------------------------------------------------
LINEAR = [("w48", sa.F32), ("w100h200", sa.F32), ("w96", sa.BF16)]


@pytest.mark.parametrize("key,dtype", LINEAR, ids=["%s-%s" % (k, DT_ID[dt]) for k, dt in LINEAR])
def test_vbs_linear_against_dense_linear(key, dtype):
    """forward, grad_x and grad_values against float64 F.linear on the dense matrix, the gradient masked to the stored positions: integers, exact equality"""
    v = geometry(key)
    n = 33
    H = handle(key, dtype, "linear", updatable=True, transposable=True)
    V = values(v, 40, integer=True)
    W = dev(V).requires_grad_(True)
    x, gy = linear_operands(v, dtype, n, 4000, integer=True)
    x.requires_grad_(True)
    y = vbs_linear(x, H, W)
    assert y.shape == (n, v.rows) and y.dtype == torch.float32
    y.backward(gy)
    torch.cuda.synchronize()
    check_linear(key, v, dtype, V, x, gy, y, x.grad, W.grad, True, key)


# ---- last in the file -----------------------------------------------------------------------------------------------------------------------
def test_zz_paths_after_set_values_report():
    """which forward path carried each product after set_values (printed: pytest -s, or the captured output of a failure); across the fp32 geometries the
    stream path (1), the per-class path (2) and the generic path (3) must each have carried at least one"""
    if not CARRIED:
        pytest.skip("the set_values tests were deselected")
    for k in sorted(CARRIED):
        print("after set_values | %-9s %-4s %-5s | %s" % (k + (" ".join("V%d/%s:%s" % (s, f, PATH_NAME[p] + ("" if q is None else "," + PATH_NAME[q])) for s, f, p, q in CARRIED[k]),)))
    seen = {p for k, log in CARRIED.items() if k[1] == "f32" for _, _, p, _ in log}
    assert {1, 2, 3} <= seen, seen
