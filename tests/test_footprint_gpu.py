"""Footprint tests: the products at offset bases inside guarded arenas (the operand alignment contract of include/sparta_amd.h, "WHERE A DEVICE OPERAND MAY START").

Every operand of every call is a slice out of the middle of an arena the test owns (tests/_footprint.py): at least 16384 elements in front and behind, the
base at a chosen byte residue modulo 128, the leading dimension from a chosen class.  The margins and the padding of an OUTPUT hold a canary NaN and must come
back bit for bit (check_untouched sees the whole arena); its defined elements hold another NaN (overwrite) or a seeded integer C0 (accumulate) and must come
back as the reference, bit for bit, no NaN left.  The margins, the padding and -- for a gathered B -- the gap between the slabs of an INPUT hold NaN: whatever
a kernel loads from there must not reach the result.  ALIGN_CASES (12 cases) covers every pair (residue of C, class of ldc) and (residue of B, class of ldb);
tests/test_footprint_host.py proves that it takes both sides of every alignment predicate of the dispatch, and that check_untouched fails on one changed word.

Matrices: the poison geometries of tests/_util.py (ragged heights, a ragged last block column, cols % w != 0: the smallest on which every carrier runs) with
the integer values of tests/test_edge_geometry_gpu.py (-3 .. 3, operands -3 .. 3, C0 -15 .. 15: every partial sum is an integer below 2^24 and exact in f16 and
bf16).  Reference: plain numpy float64 on U.edge_dense(), cast to float32.  The carriers are forced and asserted from the handle's records as in
tests/test_poison_gpu.py, whose tables this file imports.  A 16-bit operand on an odd element is refused (the last tests): it is never run through a kernel.

Each arm prints `FOOTPRINT <arm> | <carrier> | cases | products | <predicate>=<sides taken>` (pytest -s; profiles/footprint/README.md is written from it)."""
import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd import _lib

torch = pytest.importorskip("torch")

import _footprint as F  # noqa: E402
import _util as U  # noqa: E402
from test_poison_gpu import ENV as POISON_ENV  # noqa: E402
from test_poison_gpu import CSR_MODES, PATH_NAME, f32_paths, gathered_image  # noqa: E402

pytestmark = pytest.mark.gpu

ENV = POISON_ENV + ("SPARTA_F32_PLAN", "SPARTA_CSTAGE", "SPARTA_F32_KEEP_LEGACY", "SPARTA_STREAM_ALIGN", "SPARTA_C_NT", "SPARTA_NO_VEC", "SPARTA_FORCE_GENERIC",
                    "SPARTA_SP_INPLACE", "SPARTA_SP_VEC", "SPARTA_SP_SCALAR", "SPARTA_SP_ROW_BYTES", "SPARTA_COLRES_SMALL")
DT_ID = {sa.F32: "f32", sa.F16: "f16", sa.BF16: "bf16"}
TDT = {sa.F32: torch.float32, sa.F16: torch.float16, sa.BF16: torch.bfloat16}
H16 = [sa.F16, sa.BF16]
HUB_ENV = {"SPARTA_HUB_MIN_TOTAL": "1", "SPARTA_HUB_MIN_STEPS": "1", "SPARTA_HUB_TAU": "0.25"}          # (tests/test_poison_gpu.py: test_forward_h16_p64)
RECORD = {}          # arm -> {"carrier": set, "cases": set, "products": int, "sides": {predicate: set}}


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module", autouse=True)
def _print_record():
    yield
    print()
    for arm, r in sorted(RECORD.items()):
        sides = " ".join("%s=%s" % (k, "".join(sorted("T" if x else "F" for x in v))) for k, v in sorted(r["sides"].items()))
        print("FOOTPRINT %-46s | %-34s | %2d cases | %3d products | %s" % (arm, "+".join(sorted(r["carrier"])), len(r["cases"]), r["products"], sides))


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a test that left the device in an error state ends the session: nothing more is started on a GPU that has faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:          # noqa: BLE001
        pytest.exit("the device reports an error after this test, stopping: %s" % e, returncode=3)


def setenv(monkeypatch, env):
    for k, val in env.items():
        monkeypatch.setenv(k, val)


def note(arm, carrier, case, sides=None):
    r = RECORD.setdefault(arm, {"carrier": set(), "cases": set(), "products": 0, "sides": {}})
    r["carrier"].add(carrier)
    r["cases"].add(case)
    r["products"] += 1
    for k, val in (sides or {}).items():
        r["sides"].setdefault(k, set()).add(bool(val))


def esz_of(dtype):
    return 4 if dtype == sa.F32 else 2


# ---- arenas on the device ----------------------------------------------------------------------------------------------------------------------------------
def to_dev(a, dtype=sa.F32):
    """the arena (uint32 / uint16 bits) as a device tensor of the operand's type; the allocation starts on a multiple of 256 bytes, so the residue of the
    operand is what the case says"""
    t = torch.from_numpy(a.view(np.float32)).cuda() if a.dtype == np.uint32 else torch.from_numpy(a.view(np.int16)).cuda().view(TDT[dtype])
    assert t.data_ptr() % 256 == 0, "an arena must start on a multiple of 256 bytes"
    return t


def in_arena(M, ld, residue, dtype):
    """M (lines x used, float64, exact in dtype) at byte `residue` of an arena of NaN: (the arena, the operand = its slice)"""
    esz = esz_of(dtype)
    lines = M.shape[0]
    front = F.front_for(residue, esz)
    a = F.arena(lines * ld, np.float32 if esz == 4 else np.float16, front, F.MARGIN, F.QNAN[DT_ID[dtype]])
    F.place(a, front, F.bits_of(M, esz, dtype == sa.BF16), ld)
    t = to_dev(a, dtype)
    op = t[front:front + lines * ld]
    assert op.data_ptr() % 128 == residue and bool(torch.isnan(t[:front]).all()) and bool(torch.isnan(t[front + lines * ld:]).all())
    return t, op


class Out:
    """an output of lines x used with leading dimension ld at byte `residue` of an arena of canaries; the defined elements hold INTERIOR or C0"""

    def __init__(self, lines, used, ld, residue, C0=None, dead=None):
        self.lines, self.used, self.ld = lines, used, ld
        self.front = F.front_for(residue, 4)
        self.before = F.arena(lines * ld, np.float32, self.front, F.MARGIN, F.CANARY)
        inside = np.full((lines, used), F.INTERIOR, np.uint32) if C0 is None else F.bits_of(C0).reshape(lines, used).copy()
        if dead is not None:
            inside[dead.reshape(lines, used)] = F.DEAD
        self.mask = F.place(self.before, self.front, inside, ld)
        self.t = to_dev(self.before)
        self.op = self.t[self.front:self.front + lines * ld]
        assert self.op.data_ptr() % 128 == residue

    def bits(self):
        torch.cuda.synchronize()
        return self.t.cpu().numpy().view(np.uint32)

    def check(self, want, what, keep=None):
        """the whole arena: everything outside the defined elements untouched, the defined elements the bits of `want` (lines x used float64), no NaN;
        keep (bool, lines x used): elements that must still hold what they held before the call"""
        after = self.bits()
        F.check_untouched(after, self.before, self.mask, self.front, self.ld, what)
        got = after[self.mask].reshape(self.lines, self.used)
        ref = F.bits_of(want).reshape(self.lines, self.used)
        if keep is not None:
            was = self.before[self.mask].reshape(self.lines, self.used)
            assert np.array_equal(got[keep], was[keep]), (what, "%d elements that must keep their bits changed" % int((got[keep] != was[keep]).sum()))
            got, ref = got[~keep], ref[~keep]
        gf = got.view(np.float32)
        assert not np.isnan(gf).any(), (what, "%d NaN left in the output, first at (line, position) %s" % (int(np.isnan(gf).sum()), np.argwhere(np.isnan(gf))[:4].tolist()))
        if not np.array_equal(got, ref):
            diff = got != ref
            zero_sign = int((diff & (gf == ref.view(np.float32))).sum())
            raise AssertionError((what, "%d elements differ from the reference (%d of them only in the sign of a zero), first at %s: got %s, want %s"
                                  % (int(diff.sum()), zero_sign, np.argwhere(diff)[:4].tolist(), gf[diff][:4].tolist(), ref.view(np.float32)[diff][:4].tolist())))

    def same_bits_everywhere(self, what):
        after = self.bits()
        assert np.array_equal(after, self.before), (what, "%d words of the output arena changed" % int((after != self.before).sum()))


# ---- the forward sweep ---------------------------------------------------------------------------------------------------------------------------------------
def forward(arm, d, D, cols, dtype, n, seed, expect, call=None, b_row_major=False, layouts=(False, True), cases=F.ALIGN_CASES, algo=sa.SPMM_MFMA,
            preds=("c_nt",)):
    """every alignment case x C column- / row-major x overwrite / accumulate: d's product of n columns against D @ B.  expect(d, what, c_row_major) asserts the
    carrier from the handle's records and returns its name.  preds: the alignment predicates (F.predicates) that steer this arm's
    launches, recorded with the sides the cases took.  call(Bop, ldb, Cop, ldc, c_row_major, accumulate): the entry, if not DeviceVBS.spmm"""
    rows, esz = D.shape[0], esz_of(dtype)
    B = F.int_operand((cols, n), seed)
    want, C0 = D @ B, F.int_c0((rows, n), seed + 1)
    for case in cases:
        cr, cc, br, bc = case
        ldb = F.ldb_of(n if b_row_major else cols, bc, esz)
        Bt, Bop = in_arena(B if b_row_major else B.T, ldb, br, dtype)
        for crm in layouts:
            lines, used = (rows, n) if crm else (n, rows)
            ldc = F.ldc_of(used, cc)
            for acc in (False, True):
                what = (arm, "n=%d" % n, case, "ldb=%d ldc=%d" % (ldb, ldc), "C row-major" if crm else "C column-major", "accumulate" if acc else "overwrite")
                out = Out(lines, used, ldc, cr, (C0 if crm else C0.T) if acc else None)
                if call is not None:
                    call(Bop, ldb, out.op, ldc, crm, acc)
                else:
                    d.spmm(Bop, out.op, n, accumulate=acc, algo=algo, b_layout=sa.ROW_MAJOR if b_row_major else sa.COL_MAJOR,
                           c_layout=sa.ROW_MAJOR if crm else sa.COL_MAJOR, ldb=ldb, ldc=ldc)
                ref = want + C0 if acc else want
                out.check(ref if crm else ref.T, what)
                sides = F.predicates(out.op.data_ptr(), ldc, Bop.data_ptr(), ldb, n, crm, b_row_major, esz)
                note(arm, expect(d, what, crm), case, {k: sides[k] for k in preds})
        del Bt


def path_is(*names):
    def expect(d, what, crm):
        carried = PATH_NAME[d.info()["last_path"]]
        assert carried in names, (what, "carried by", carried, d.info())
        return carried
    return expect


# ---- 1. forward product, fp32 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cstage", ["1", "0"], ids=["ring", "direct-stores"])
@pytest.mark.parametrize("key", ["P32", "P64"])
def test_forward_f32_stream(key, cstage, monkeypatch):
    """SPARTA_PATH=stream at n = 128.  P32: the no-barrier kernel on the fragment image (k_f32_direct.hip), finished tiles parked in the C ring (SPARTA_CSTAGE=1:
    aligned blocks of 32 rows, the partial block at a range's end) or stored directly (0); P64: the LDS-staged stream kernel (tiles of 33..64 rows).  Each with
    and without the non-temporal stores (c_nt), by the alignment case.  Fix-up and zero-range launches ride along where the plan has them."""
    setenv(monkeypatch, {"SPARTA_SPARSE_K": "0", "SPARTA_PATH": "stream", "SPARTA_CSTAGE": cstage, "SPARTA_F32_PLAN": "direct"})
    v = F.int_geometry(key)
    d = v.to_device(0)
    try:
        assert d.sparse_info()["rows"] == 0 and d.info()["stream_workers"] > 0 and d.packed_info()["packed"] == 0, (d.info(), d.packed_info())
        forward("f32 %s stream CSTAGE=%s" % (key, cstage), d, U.edge_dense(v), v.cols, sa.F32, 128, 100, path_is("stream"))
    finally:
        d.close()


def test_forward_f32_stream_row_major_b(monkeypatch):
    """a row-major B on P32: the LDS-staged stream kernels read it where it is (k_f32_stream.hip, BRM)"""
    setenv(monkeypatch, {"SPARTA_SPARSE_K": "0", "SPARTA_PATH": "stream"})
    v = F.int_geometry("P32")
    d = v.to_device(0)
    try:
        forward("f32 P32 stream row-major B", d, U.edge_dense(v), v.cols, sa.F32, 128, 110, path_is("stream"), b_row_major=True)
    finally:
        d.close()


def test_forward_f32_class(monkeypatch):
    """P64 at n = 128 under SPARTA_PATH=class: the per-class kernels (vec_ok = 1 whatever the pointers are: they read through 4-byte aligned vector types)"""
    setenv(monkeypatch, {"SPARTA_SPARSE_K": "0", "SPARTA_PATH": "class"})
    v = F.int_geometry("P64")
    d = v.to_device(0)
    try:
        forward("f32 P64 per-class", d, U.edge_dense(v), v.cols, sa.F32, 128, 120, path_is("per-class"), preds=())
        forward("f32 P64 per-class row-major B", d, U.edge_dense(v), v.cols, sa.F32, 128, 121, path_is("per-class"), b_row_major=True, cases=F.ALIGN_CASES[::3], preds=())
    finally:
        d.close()


@pytest.mark.parametrize("key,n", [("P13", 128), ("P13", 40), ("P32", 40)], ids=["P13-n128", "P13-n40", "P32-n40"])
def test_forward_f32_generic(key, n, monkeypatch):
    """the generic kernels: P13 (w = 13) whatever n is, P32 at n = 40 (no whole slab)"""
    monkeypatch.setenv("SPARTA_SPARSE_K", "0")
    v = F.int_geometry(key)
    d = v.to_device(0)
    try:
        assert f32_paths(d, v, n, None) == {"generic"}
        forward("f32 %s generic n=%d" % (key, n), d, U.edge_dense(v), v.cols, sa.F32, n, 130 + n, path_is("generic"), preds=())
        if key == "P13" and n == 40:
            forward("f32 P13 generic n=40 row-major B", d, U.edge_dense(v), v.cols, sa.F32, n, 131, path_is("generic"), b_row_major=True, cases=F.ALIGN_CASES[::3], preds=())
    finally:
        d.close()


def test_forward_f32_exact_order(monkeypatch):
    """P32 at n = 40 with SPARTA_SPMM_EXACT: the exact-order kernel is asked for by the call and has no fallback; the handle has run no other product, so its
    record of the last MFMA path must still say 'none'"""
    monkeypatch.setenv("SPARTA_SPARSE_K", "0")
    v = F.int_geometry("P32")
    d = v.to_device(0)
    try:
        def expect(d, what, crm):
            assert PATH_NAME[d.info()["last_path"]] == "none", (what, d.info())
            return "exact-order"
        forward("f32 P32 exact-order n=40", d, U.edge_dense(v), v.cols, sa.F32, 40, 140, expect, algo=sa.SPMM_EXACT, preds=())
    finally:
        d.close()


@pytest.mark.parametrize("name", ["heights", "tail"])
def test_forward_f32_packed(name, monkeypatch):
    """a packed-plan handle (k_f32_packed.hip), forced and asserted as tests/test_packed_gpu.py does, on its geometries `heights` (tiles of 1, 17, 31 and 32 rows:
    none but the first starts on a multiple of 32 rows -- the C ring) and `tail` (a ragged last block column); ring and direct stores"""
    import test_packed_gpu as PK
    setenv(monkeypatch, {"SPARTA_SPARSE_K": "0", "SPARTA_PATH": "stream", "SPARTA_F32_PLAN": "packed"})
    heights, present, masks, cols, _ = PK.CASES[name]
    v = PK.build(heights, present, masks, cols, "int", 3)
    d = v.to_device(0)
    try:
        assert d.packed_info()["packed"] == 1, d.packed_info()
        for cstage in ("1", "0"):
            monkeypatch.setenv("SPARTA_CSTAGE", cstage)
            forward("f32 packed %s CSTAGE=%s" % (name, cstage), d, U.edge_dense(v), v.cols, sa.F32, 128, 150, path_is("stream"))
            assert d.packed_info()["packed"] == 1
    finally:
        d.close()


# ---- 2. forward product, 16-bit --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h16_path", ["lds", "direct"])
@pytest.mark.parametrize("pair", ["pair-tiles", "no-pairs"])
@pytest.mark.parametrize("dtype", H16, ids=["f16", "bf16"])
def test_forward_h16_p32(dtype, pair, h16_path, monkeypatch):
    """P32 on a 16-bit handle, LDS and direct kernels, with and without pair tiles; n = 128 and n = 200 (a whole slab and the padded tail slab, whose scratch C is
    merged into the caller's)"""
    setenv(monkeypatch, {"SPARTA_SPARSE_K": "0", "SPARTA_H16_PATH": h16_path})
    if pair == "no-pairs":
        monkeypatch.setenv("SPARTA_H16_PAIR", "0")
    v = F.int_geometry("P32")
    d = v.to_device(0, dtype=dtype)
    try:
        info = d.info()
        assert (info["stream_steps"] < int(v.nzcount.sum())) == (pair == "pair-tiles") and info["stream_steps"] > 0 and d.sparse_info()["rows"] == 0, info
        for n in (128, 200):
            forward("%s P32 %s %s n=%d" % (DT_ID[dtype], h16_path, pair, n), d, U.edge_dense(v, dtype), v.cols, dtype, n, 200 + n, path_is("stream"))
    finally:
        d.close()


@pytest.mark.parametrize("plan", ["stream", "hub-2", "hub-4"])
@pytest.mark.parametrize("dtype", H16, ids=["f16", "bf16"])
def test_forward_h16_p64(dtype, plan, monkeypatch):
    """P64 on a 16-bit handle: the stream plan, and the hub plan (k_hub16.hip, B straight into LDS) forced to groups of 2 and 4; n = 128 and 256"""
    monkeypatch.setenv("SPARTA_SPARSE_K", "0")
    if plan != "stream":
        setenv(monkeypatch, dict(HUB_ENV, SPARTA_HUB_G=plan[-1]))
    v = F.int_geometry("P64")
    d = v.to_device(0, dtype=dtype)
    try:
        hi = d.hub_info()
        if plan == "stream":
            assert hi["steps"] == 0, hi
        else:
            assert hi["steps"] > 0 and hi["groups"] >= 1 and hi["tiles_per_group"] == int(plan[-1]) and hi["union_area"] > hi["stored_area"] > 0, hi
        for n in (128, 256):
            forward("%s P64 %s n=%d" % (DT_ID[dtype], plan, n), d, U.edge_dense(v, dtype), v.cols, dtype, n, 300 + n, path_is("stream"))
    finally:
        d.close()


# ---- 3. handles made from a CSR ------------------------------------------------------------------------------------------------------------------------------
CSR_CASES = [(dt, mode) for mode, (_, _, dts) in CSR_MODES.items() for dt in dts]


@pytest.mark.parametrize("dtype,mode", CSR_CASES, ids=["%s-%s" % (DT_ID[dt], mode) for dt, mode in CSR_CASES])
def test_forward_from_csr(dtype, mode, monkeypatch):
    """every mode of tests/test_poison_gpu.py: CSR_MODES -- the row gather (n = 40: one element per lane; n = 256: four, two or one by the alignment of a row-major
    C and of a row-major B), the window plan, the resident-column kernel (n = 8, column-major C; a row-major C takes the row gather), block-rows split into tiles
    and sparse rows that add, the column-compacted tiles (a row-major fp32 B is read in place when its rows are 16-byte aligned, else copied: ensure_brm)"""
    setenv(monkeypatch, {"SPARTA_SPARSE_MIN_STEPS": "0", "SPARTA_LAUNCH_NNZ": "0"})
    which, env, _ = CSR_MODES[mode]
    setenv(monkeypatch, env)
    m, g, w = F.int_csr(which)
    d = sa.DeviceVBS.from_csr(m, g, w, device=0, dtype=dtype)
    try:
        sp, ui, info = d.sparse_info(), d.union_info(), d.info()
        tiles = info["tiles16"] + info["tiles32"] + info["tiles64"]
        if which == "PCSR":
            assert sp["rows"] > 0 and sp["nnz"] == m.nztot() and tiles == 0 and ui["nnz"] == 0, (sp, ui, info)
        if mode == "windows":
            assert sp["hub_rows"] > 0, sp
        if mode == "tiles-and-sparse-rows":
            assert tiles >= m.rows // 32 and 0 < sp["nnz"] < m.nztot() and sp["rows"] > m.rows * 2 // 3 and ui["nnz"] == 0, (sp, ui, info)
        if mode == "union-tiles":
            assert ui["tiles32"] + ui["tiles64"] >= len(np.unique(g)) and ui["nnz"] > 0.7 * m.nztot() and ui["nnz"] + sp["nnz"] == m.nztot() and tiles == 0, (sp, ui, info)
        assert (d.colres_info()["slices"] > 0) == (mode == "resident-columns"), d.colres_info()
        D, _ = U.csr_dense_and_stored(m, g, w)
        assert np.array_equal(U.edge_round(D, dtype), D)

        def expect(d, what, crm):
            nc = d.colres_info()["nc"]
            assert (nc > 0) == (mode == "resident-columns" and not crm), (what, d.colres_info())
            return "resident-columns" if nc > 0 else mode if mode != "resident-columns" else "row-gather"
        arm = "%s %s %s" % (DT_ID[dtype], which, mode)
        preds = ("colres_vec_in", "colres_vec_out") if mode == "resident-columns" else ("sparse_aligned4", "sparse_aligned2")
        for n in (8,) if mode == "resident-columns" else (40, 256):
            forward("%s n=%d" % (arm, n), d, D, m.cols, dtype, n, 400 + n, expect, preds=preds)
        if dtype == sa.F32 and mode in ("row-gather", "union-tiles"):
            forward("%s n=256 row-major B" % arm, d, D, m.cols, dtype, 256, 470, expect, b_row_major=True, preds=preds + (("brm_in_place",) if mode == "union-tiles" else ()))
    finally:
        d.close()


def test_forward_resident_columns_smallest_matrix(monkeypatch):
    """the resident-column kernel on the smallest matrix of tests/test_colres_gpu.py (63 x 5, every second row empty), for the residues of B and C it has not seen:
    vec_in and vec_out both ways; n = 5 and 8"""
    from test_colres_gpu import _matrix
    A = _matrix(63, 5, 0.6, 0, 63 + 5, 2)
    A.data = np.random.default_rng(7470).integers(1, 4, A.nnz).astype(np.float32)
    g = np.arange(63, dtype=np.int64) // 4
    d = sa.DeviceVBS.from_csr(sa.CSR.from_scipy(A), g, 64, device=0)
    try:
        assert d.colres_info()["slices"] > 0 and d.colres_info()["nnz"] == A.nnz, d.colres_info()
        D = np.asarray(A.todense(), np.float64)[np.asarray(sa.get_permutation(g), np.int64)]

        def expect(d, what, crm):
            assert d.colres_info()["nc"] > 0, (what, d.colres_info())
            return "resident-columns"
        for n in (5, 8):
            forward("f32 63x5 resident-columns n=%d" % n, d, D, 5, sa.F32, n, 480 + n, expect, layouts=(False,), preds=("colres_vec_in", "colres_vec_out"))
    finally:
        d.close()


# ---- 4. gathered and prepared B ----------------------------------------------------------------------------------------------------------------------------
GP_CASES = [("P32", sa.F32), ("P64", sa.F32), ("P32", sa.F16), ("P64", sa.BF16)]
gp = pytest.mark.parametrize("key,dtype", GP_CASES, ids=["%s-%s" % (k, DT_ID[dt]) for k, dt in GP_CASES])


@gp
def test_gathered_ld(key, dtype, monkeypatch):
    """sparta_vbs_spmm_gathered_ld on P32G / P64G: two slabs of 4 w rows, shard_ld from the ldb class, 72 elements between the slabs; the padding of shard_ld and
    the gap hold NaN and Inf (gathered_image), the margins NaN.  C has ldc = rows (the entry's Python form takes no ldc): its residues only"""
    monkeypatch.setenv("SPARTA_SPARSE_K", "0")
    v = F.int_geometry(key + "G")
    d = v.to_device(0, dtype=dtype)
    esz = esz_of(dtype)
    try:
        D, rows, shard_rows = U.edge_dense(v, dtype), v.rows, v.cols // 2
        cases = sorted({(cr, br, bc) for cr, _, br, bc in F.ALIGN_CASES})
        for n in (40, 128):
            arm = "%s %s gathered_ld n=%d" % (DT_ID[dtype], key + "G", n)
            want_path = f32_paths(d, v, n, None) if dtype == sa.F32 else {"stream"}
            B = F.int_operand((v.cols, n), 500 + n)
            want, C0 = D @ B, F.int_c0((rows, n), 501 + n)
            for cr, br, bc in cases:
                shard_ld = F.ldb_of(shard_rows, bc, esz)
                stride = shard_ld * n + 72
                img = gathered_image(B, shard_rows, shard_ld, stride, dtype)
                front = F.front_for(br, esz)
                a = F.arena(img.numel(), np.float32 if esz == 4 else np.float16, front, F.MARGIN, F.QNAN[DT_ID[dtype]])
                Bt = to_dev(a, dtype)
                Bop = Bt[front:front + img.numel()]
                Bop.copy_(img)
                assert Bop.data_ptr() % 128 == br and not bool(torch.isfinite(Bop[shard_rows:shard_ld]).any()) and bool(torch.isnan(Bt[:front]).all())
                for crm in (False, True):
                    lines, used = (rows, n) if crm else (n, rows)
                    for acc in (False, True):
                        what = (arm, (cr, br, bc), "shard_ld=%d stride=%d" % (shard_ld, stride), "C row-major" if crm else "C column-major", "accumulate" if acc else "overwrite")
                        out = Out(lines, used, used, cr, (C0 if crm else C0.T) if acc else None)
                        d.spmm_gathered(Bop, shard_rows, out.op, n, accumulate=acc, c_layout=sa.ROW_MAJOR if crm else sa.COL_MAJOR, shard_stride=stride, shard_ld=shard_ld)
                        ref = want + C0 if acc else want
                        out.check(ref if crm else ref.T, what)
                        carried = PATH_NAME[d.info()["last_path"]]
                        assert carried in want_path, (what, d.info())
                        note(arm, carried, (cr, br, bc), {"c_nt": F.predicates(out.op.data_ptr(), used, 0, 4, n, crm, False, esz)["c_nt"]})
    finally:
        d.close()


@gp
def test_prepared_b(key, dtype, monkeypatch):
    """sparta_vbs_prepare_b + sparta_vbs_spmm_prepared on P32 / P64 at n = 128"""
    monkeypatch.setenv("SPARTA_SPARSE_K", "0")
    v = F.int_geometry(key)
    d = v.to_device(0, dtype=dtype)
    try:
        n = 128
        want_path = f32_paths(d, v, n, None) if dtype == sa.F32 else {"stream"}
        held = []

        def call(Bop, ldb, Cop, ldc, crm, acc):
            if not held or held[0][0] is not Bop:
                for _, P in held:
                    P.close()
                held[:] = [(Bop, d.prepare_b(Bop, n, ldb=ldb))]
            d.spmm_prepared(held[0][1], Cop, accumulate=acc, c_layout=sa.ROW_MAJOR if crm else sa.COL_MAJOR, ldc=ldc)
        try:
            forward("%s %s prepared n=%d" % (DT_ID[dtype], key, n), d, U.edge_dense(v, dtype), v.cols, dtype, n, 600, path_is(*want_path), call=call)
        finally:
            for _, P in held:
                P.close()
    finally:
        d.close()


# ---- 5. the training entry points ------------------------------------------------------------------------------------------------------------------------
RANGE = (2, 6)
TRAIN = [(k, dt) for dt in (sa.F32, sa.F16, sa.BF16) for k in ("P32", "P64")]
train = pytest.mark.parametrize("key,dtype", TRAIN, ids=["%s-%s" % (k, DT_ID[dt]) for k, dt in TRAIN])
ranges = pytest.mark.parametrize("br", [None, RANGE], ids=["whole", "range"])
_TRAIN = {}


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for d in _TRAIN.values():
        d.close()
    _TRAIN.clear()


def vbr_of(v, mab):
    return U.sa_vbr((v.rows, v.cols, int(v.block_col_size), v.row_part, v.nzcount, v.jab), np.ascontiguousarray(mab, np.float32))


def train_handle(key, dtype, br):
    if (key, dtype, br) not in _TRAIN:
        _TRAIN[(key, dtype, br)] = F.int_geometry(key).to_device(0, dtype=dtype, block_row_range=br, updatable=True, transposable=True)
    return _TRAIN[(key, dtype, br)]


@ranges
@train
def test_spmm_t(key, dtype, br):
    """Ct (+)= A^T X at n = 40 and 128: X at the residues and leading dimensions of B's cases, Ct with the padded ldo and the residues of C's"""
    v = F.int_geometry(key)
    d = train_handle(key, dtype, br)
    D, esz = U.edge_dense(v, dtype, br=br), esz_of(dtype)
    rows = D.shape[0]
    for n in (40, 128):
        arm = "%s %s %s spmm_t n=%d" % (DT_ID[dtype], key, "range" if br else "whole", n)
        X = F.int_operand((rows, n), 700 + n)
        want, C0 = D.T @ X, F.int_c0((v.cols, n), 701 + n)
        for case in F.ALIGN_CASES:
            cr, cc, xr, xc = case
            ldx, ldo = F.ldb_of(rows, xc, esz), F.ldc_of(v.cols, cc)
            Xt, Xop = in_arena(X.T, ldx, xr, dtype)
            for acc in (False, True):
                what = (arm, case, "ldx=%d ldo=%d" % (ldx, ldo), "accumulate" if acc else "overwrite")
                out = Out(n, v.cols, ldo, cr, C0.T if acc else None)
                d.spmm_t(Xop, out.op, n, accumulate=acc, ldx=ldx, ldo=ldo)
                out.check((want + C0 if acc else want).T, what)
                note(arm, "spmm_t", case)


def block_mask(v, br, blocks):
    """bool over the mab slice of the block-rows br: True on every element (the positions past cols included) of the stored blocks numbered in `blocks`"""
    w = int(v.block_col_size)
    lo, hi = U.edge_mab_slice(v, br or (0, v.block_rows))
    m = np.zeros(hi - lo, bool)
    for b, (off, _, h, _, _) in enumerate(U.edge_blocks(v, br)):
        if b in blocks:
            m[off:off + h * w] = True
    return m


@ranges
@train
def test_sddmm(key, dtype, br):
    """G (+)= (X Y^T) on the stored blocks at k = 40 and 128: X and Y at offset bases with padded ldx / ldy, G a slice with canaries on both sides.  Then with a
    live set that kills every third block: overwrite stores +0.0 there, accumulate leaves the bits of the dead blocks (a NaN payload here) as they are"""
    v = F.int_geometry(key)
    d = train_handle(key, dtype, br)
    esz = esz_of(dtype)
    b0, b1 = br or (0, v.block_rows)
    rows = int(v.row_part[b1] - v.row_part[b0])
    lo, hi = U.edge_mab_slice(v, (b0, b1))
    nz = hi - lo
    n_blocks = len(U.edge_blocks(v, br))
    assert d.n_blocks == n_blocks and d.info()["nztot"] == nz
    dead_ids = set(range(1, n_blocks, 3))
    dead = block_mask(v, br, dead_ids)
    keep = torch.from_numpy(np.array([b not in dead_ids for b in range(n_blocks)], np.uint8)).cuda()
    try:
        for k in (40, 128):
            arm = "%s %s %s sddmm k=%d" % (DT_ID[dtype], key, "range" if br else "whole", k)
            X, Y = F.int_operand((rows, k), 800 + k), F.int_operand((v.cols, k), 801 + k)
            want, G0 = U.edge_sample(v, X @ Y.T, br), F.int_c0((nz,), 802 + k)
            for q, case in enumerate(F.ALIGN_CASES):
                gr, _, xr, xc = case
                _, _, yr, yc = F.ALIGN_CASES[(q + 5) % len(F.ALIGN_CASES)]                    # Y: another case's residue and class
                ldx, ldy = F.ldb_of(rows, xc, esz), F.ldb_of(v.cols, yc, esz)
                Xt, Xop = in_arena(X.T, ldx, xr, dtype)
                Yt, Yop = in_arena(Y.T, ldy, yr, dtype)
                for live in (False, True) if q % 3 == 0 else (False,):
                    d.set_live_blocks(keep if live else None)
                    for acc in (False, True):
                        what = (arm, case, "ldx=%d ldy=%d Y at %d" % (ldx, ldy, yr), "live set" if live else "no live set", "accumulate" if acc else "overwrite")
                        out = Out(1, nz, nz, gr, G0[None, :] if acc else None, dead=dead[None, :] if live and acc else None)
                        d.sddmm(Xop, Yop, out.op, k, accumulate=acc, ldx=ldx, ldy=ldy)
                        ref = want + G0 if acc else want
                        if live and not acc:
                            ref = np.where(dead, 0.0, ref)
                        out.check(ref[None, :], what, keep=dead[None, :] if live and acc else None)
                        note(arm, "sddmm" + (" live" if live else ""), case, {"Y % 16 == 0 and ldy % 8 == 0": Yop.data_ptr() % 16 == 0 and ldy % 8 == 0})
    finally:
        d.set_live_blocks(None)


@ranges
@train
def test_set_values(key, dtype, br):
    """set_values from a mab at the four residues, NaN on both sides of it: afterwards the forward product (through the arenas, two alignment cases) and spmm_t are
    the reference's, bit for bit, and bit-identical to a fresh handle created from the same values"""
    v = F.int_geometry(key)
    d = train_handle(key, dtype, br)
    lo, hi = U.edge_mab_slice(v, br or (0, v.block_rows))
    first = v.mab[lo:hi].astype(np.float32)
    try:
        for residue in F.C_RESIDUES:
            V = np.random.default_rng(900 + residue).integers(1, 4, len(v.mab)).astype(np.float32) * (-1.0 if residue % 8 else 1.0)
            Vt, Vop = in_arena(V[None, lo:hi], hi - lo, residue, sa.F32)
            assert Vop.numel() == hi - lo
            d.set_values(Vop)
            fresh = vbr_of(v, V).to_device(0, dtype=dtype, block_row_range=br, updatable=True, transposable=True)
            try:
                D = U.edge_dense(v, dtype, mab=V, br=br)
                n = 128
                arm = "%s %s %s set_values" % (DT_ID[dtype], key, "range" if br else "whole")
                want_path = f32_paths(d, v, n, None) if dtype == sa.F32 else {"stream"}
                for h, tag in ((d, arm), (fresh, arm + " (fresh handle)")):
                    forward(tag, h, D, v.cols, dtype, n, 910, path_is(*want_path), cases=F.ALIGN_CASES[1::6])
                X = F.int_operand((D.shape[0], 40), 920)
                ldx = F.ldb_of(D.shape[0], "odd", esz_of(dtype))
                Xt, Xop = in_arena(X.T, ldx, 4, dtype)
                outs = []
                for h in (d, fresh):
                    out = Out(40, v.cols, v.cols + 3, 16)
                    h.spmm_t(Xop, out.op, 40, ldx=ldx, ldo=v.cols + 3)
                    out.check((D.T @ X).T, (arm, residue, "spmm_t"))
                    outs.append(out.bits())
                assert np.array_equal(outs[0], outs[1]), (arm, residue, "spmm_t differs from a fresh handle")
                note(arm, "set_values", residue, {"mab % 16 == 0": Vop.data_ptr() % 16 == 0})
            finally:
                fresh.close()
    finally:
        d.set_values(torch.from_numpy(first).cuda())


# ---- 6. a 16-bit operand on an odd element is refused, with nothing launched ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", H16, ids=["f16", "bf16"])
def test_an_odd_element_base_of_a_16_bit_operand_is_refused(dtype, monkeypatch):
    """include/sparta_amd.h: 16-bit device operands start on a 4-byte boundary.  Every entry returns the code it uses for an odd leading dimension, and the
    output arena keeps every bit -- the defined elements too: nothing was launched.  No odd-element base reaches a kernel here.  (sparta_vbs_sddmm_block_ssq is
    the stated exception: it accepts any element, and tests/test_sddmm_score_gpu.py: test_operand_placement holds it to the bits of the aligned call.)"""
    monkeypatch.setenv("SPARTA_SPARSE_K", "0")
    v = F.int_geometry("P32G")
    d = v.to_device(0, dtype=dtype, updatable=True, transposable=True)
    try:
        n, rows, cols = 128, v.rows, v.cols
        nz = d.info()["nztot"]
        ld = cols + 24

        def odd(lines, ldim):
            """an operand of `lines` lines one element past a 4-byte boundary, and the same one element further (even: accepted)"""
            front = F.front_for(4, 2)
            a = F.arena(lines * ldim + 2, np.float16, front, F.MARGIN, F.bits_of(np.ones(1), 2, dtype == sa.BF16)[0])          # finite everywhere: a kernel that ran would write numbers
            t = to_dev(a, dtype)
            op = t[front + 1:front + 1 + lines * ldim]
            assert op.data_ptr() % 4 == 2
            return t, op, t[front + 2:front + 2 + lines * ldim]
        Bt, Bodd, Beven = odd(n, ld)
        Xt, Xodd, Xeven = odd(n, rows + 1)          # (rows = 251: ldx = 252)

        def refused(code, what, fn):
            with pytest.raises(_lib.SpartaError) as e:
                fn()
            assert e.value.code == code and "4-byte" in str(e.value), (what, e.value.code, str(e.value))
        for acc in (False, True):
            out = Out(n, rows, rows, 0, F.int_c0((n, rows), 1) if acc else None)
            refused(_lib.ERR_UNSUPPORTED, "spmm", lambda: d.spmm(Bodd, out.op, n, accumulate=acc, ldb=ld))
            refused(_lib.ERR_UNSUPPORTED, "spmm_gathered", lambda: d.spmm_gathered(Bodd, cols // 2, out.op, n, accumulate=acc))
            refused(_lib.ERR_UNSUPPORTED, "spmm_gathered_ld", lambda: d.spmm_gathered(Bodd, cols // 2, out.op, n, accumulate=acc, shard_ld=cols // 2 + 8, shard_stride=(cols // 2 + 8) * n))
            refused(_lib.ERR_UNSUPPORTED, "prepare_b", lambda: d.prepare_b(Bodd, n, ldb=ld))
            out.same_bits_everywhere("forward entries")
            g = Out(1, nz, nz, 4, F.int_c0((1, nz), 2) if acc else None)
            refused(_lib.ERR_INVALID, "sddmm X", lambda: d.sddmm(Xodd, Beven, g.op, n, accumulate=acc, ldx=rows + 1, ldy=ld))
            refused(_lib.ERR_INVALID, "sddmm Y", lambda: d.sddmm(Xeven, Bodd, g.op, n, accumulate=acc, ldx=rows + 1, ldy=ld))
            g.same_bits_everywhere("sddmm")
            ct = Out(n, cols, cols + 3, 16, F.int_c0((n, cols), 3) if acc else None)
            refused(_lib.ERR_INVALID, "spmm_t", lambda: d.spmm_t(Xodd, ct.op, n, accumulate=acc, ldx=rows + 1, ldo=cols + 3))
            ct.same_bits_everywhere("spmm_t")
        # the same operands one element further are accepted: the refusal is about the base, nothing else
        out = Out(n, rows, rows, 0)
        d.spmm(Beven, out.op, n, ldb=ld)
        torch.cuda.synchronize()
        assert not np.isnan(out.bits()[out.mask].view(np.float32)).any()
    finally:
        d.close()
