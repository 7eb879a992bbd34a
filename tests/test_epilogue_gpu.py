"""sparta_epilogue_fwd / sparta_epilogue_bwd on the GPU (k_epilogue.hip), at the level of the C-ABI: raw column-major buffers with a leading dimension.

None / ReLU: Y, dZ and dbias equal fwd_ref / bwd_ref (tests/_epilogue.py) bit for bit, for every output and input type, with and without bias, on data with
-0.0, values straddling 0, Inf and a NaN.  Every comparison is of the WHOLE buffer: outputs are prefilled with a sentinel, so the padding [rows, ld), the
elements in front of an offset base and -- dbias and scratch start as NaN -- any accumulation into old content show as a mismatch; the padding of the inputs
holds NaN.  16-bit outputs are the nearest-even rounding of the same call's fp32 output, GELU included.  GELU is held to an fp64 reference within 4x the
error of torch's CPU float32 gelu + 1 unit, its dbias to the fixed-order fp64 sum of the kernel's own fp32 dz, bit for bit.

Measured on MI355X (in units of 2^-24 max(|u|, 2^-10) for y, 2^-24 |dy| max(1, |u|) for dz; printed by test_gelu_against_float64): kernel 1.70 / 2.51
without a bias and 1.71 / 2.42 with one, torch CPU float32 5.02 / 4.76 and 5.17 / 4.59 (profiles/epilogue/README.md)."""
import ctypes as C
import math

import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd._lib import lib

import _epilogue as E
from _epilogue import f32, F32, F16, BF16, NONE, RELU, GELU

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

_f32p = C.POINTER(C.c_float)
DTS = (F32, F16, BF16)
DT_ID = {F32: "f32", F16: "f16", BF16: "bf16"}
SENTINEL = {F32: f32(-77.25), F16: np.uint16(0xd4d4), BF16: np.uint16(0xc29a)}
ROWS = (1, 3, 64, 67, 261)
NCOLS = (1, 2, 31, 32, 33, 129)


class Buf:
    """a device buffer holding a column-major rows x n matrix (stored form of `dtype`) with leading dimension ld behind `offset` elements"""

    def __init__(self, M, ld, dtype, offset=0, pad=None):
        self.rows, self.n = M.shape
        self.ld, self.dtype, self.offset = ld, dtype, offset
        self.host0 = E.store(M, ld, dtype, offset, pad)
        self.t = torch.from_numpy(self.host0.view(np.int16) if dtype != F32 else self.host0.copy()).cuda()
        assert self.t.data_ptr() % 16 == 0

    def ptr(self, typ=None):
        p = C.c_void_p(self.t.data_ptr() + self.offset * E.ESIZE[self.dtype])
        return C.cast(p, typ) if typ else p

    def read(self):
        a = self.t.cpu().numpy()
        return a.view(np.uint16) if self.dtype != F32 else a

    def write(self, M):
        self.host0 = E.store(M, self.ld, self.dtype, self.offset)
        self.t.copy_(torch.from_numpy(self.host0.view(np.int16) if self.dtype != F32 else self.host0))


def out_buf(rows, n, ld, dtype, offset):
    return Buf(np.full((rows, n), SENTINEL[dtype], E.NP_STORE[dtype]), ld, dtype, offset, pad=SENTINEL[dtype])


def expect(M_stored, ld, dtype, offset):
    return E.store(M_stored, ld, dtype, offset, pad=SENTINEL[dtype])


def vec(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def vptr(t, typ=_f32p):
    return C.cast(C.c_void_p(t.data_ptr() if t is not None else None), typ)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def scratch_for(rows, n):
    nb = sa.epilogue.scratch_bytes(rows, n)
    return torch.full((nb // 8,), float("nan"), dtype=torch.float64, device="cuda") if nb else None


def call_fwd(Z, bias_t, act, Y):
    sa._lib.check(lib.sparta_epilogue_fwd(Z.ptr(_f32p), Z.ld, vptr(bias_t), act, Y.ptr(), Y.ld, Y.dtype, Z.rows, Z.n, stream(), None))


def call_bwd(dY, Z, bias_t, act, dZ, dbias_t, scratch_t):
    sa._lib.check(lib.sparta_epilogue_bwd(dY.ptr(), dY.ld, dY.dtype, Z.ptr(_f32p) if Z is not None else None, Z.ld if Z is not None else dY.ld, vptr(bias_t), act,
                                          dZ.ptr(), dZ.ld, dZ.dtype, vptr(dbias_t), vptr(scratch_t, C.c_void_p), dY.rows, dY.n, stream(), None))


def same(a, b):
    return np.array_equal(E.bits(a), E.bits(b))


def operands(rows, n, seed):
    rng = np.random.default_rng(seed)
    Z, dY = E.special_values(rng, (rows, n)), E.special_values(rng, (rows, n))
    b = rng.standard_normal(rows).astype(f32)
    b[::3] = 0.0
    return Z, dY, b


GEOMETRY = [(0, 0), (3, 0), (0, 1), (3, 1)]            # (ld - rows, elements the base is offset by)


# ---- 1. none / relu, bit for bit, every type, every geometry; the whole buffers (guard bands, no accumulation) ------------------------------------------
@pytest.mark.parametrize("n", NCOLS)
@pytest.mark.parametrize("rows", ROWS)
def test_none_and_relu_bit_for_bit(rows, n):
    Z, dY32, b = operands(rows, n, 1000 * rows + n)
    bias_t = vec(b)
    for extra, off in GEOMETRY:
        ld = rows + extra
        Zb = Buf(Z, ld, F32, off)
        dYb = {dt: Buf(E.rne_bits(dY32, dt), ld + (4 if dt == F16 else 0), dt, off) for dt in DTS}           # (leading dimensions need not agree)
        dYw = {dt: E.widen(E.rne_bits(dY32, dt), dt) for dt in DTS}
        for act in (NONE, RELU):
            for bias, bt in ((b, bias_t), (None, None)):
                for yt in DTS:
                    Y = out_buf(rows, n, ld, yt, off)
                    call_fwd(Zb, bt, act, Y)
                    assert same(Y.read(), expect(E.fwd_ref(Z, bias, act, yt), ld, yt, off)), ("fwd", act, bias is None, yt, extra, off)
                for dyt in DTS:
                    dz32 = E.bwd_f32(dYw[dyt], Z, bias, act)
                    want_db = E.dbias_of(dz32)
                    for dzt in DTS:
                        zoff = 1 - off if dzt == BF16 else off                                             # (nor the bases: then no row is 16-byte aligned in all three)
                        dZ = out_buf(rows, n, ld, dzt, zoff)
                        dbias_t = torch.full((rows,), float("nan"), device="cuda")
                        call_bwd(dYb[dyt], Zb, bt, act, dZ, dbias_t, scratch_for(rows, n))
                        what = ("bwd", act, bias is None, dyt, dzt, extra, off)
                        assert same(dZ.read(), expect(E.rne_bits(dz32, dzt), ld, dzt, zoff)), what
                        assert same(dbias_t.cpu().numpy(), want_db), what
        assert same(Zb.read(), Zb.host0) and all(same(dYb[dt].read(), dYb[dt].host0) for dt in DTS)          # the inputs are inputs


def test_z_may_be_null_without_an_activation_and_dbias_may_be_skipped():
    rows, n, ld = 67, 33, 70
    Z, dY32, b = operands(rows, n, 5)
    dYb = Buf(dY32, ld, F32)
    dZ = out_buf(rows, n, ld, BF16, 1)
    call_bwd(dYb, None, None, NONE, dZ, None, None)
    assert same(dZ.read(), expect(E.rne_bits(dY32, BF16), ld, BF16, 1))
    dbias_t = torch.full((rows,), float("nan"), device="cuda")
    dZ = out_buf(rows, n, ld, F32, 0)
    call_bwd(dYb, None, vec(b), NONE, dZ, dbias_t, scratch_for(rows, n))                                    # (a bias without an activation does not reach dz)
    assert same(dZ.read(), expect(dY32, ld, F32, 0)) and same(dbias_t.cpu().numpy(), E.dbias_of(dY32))


# ---- 2. 16-bit outputs are the rounding of the same call's fp32 output, GELU included -------------------------------------------------------------------
@pytest.mark.parametrize("act", [NONE, RELU, GELU], ids=["none", "relu", "gelu"])
def test_16bit_outputs_round_the_fp32_output(act):
    rows, n, ld, off = 261, 33, 264, 1
    rng = np.random.default_rng(act)
    Z = np.concatenate([rng.uniform(-6, 6, (rows, n - 8)), rng.uniform(-0.01, 0.01, (rows, 8))], 1).astype(f32)
    dY32 = (rng.standard_normal((rows, n)) * 10.0 ** rng.integers(-4, 5, (rows, n))).astype(f32)
    b = rng.uniform(-0.5, 0.5, rows).astype(f32)
    Zb, bias_t = Buf(Z, ld, F32, off), vec(b)
    out = {}
    for yt in DTS:
        Y = out_buf(rows, n, ld, yt, off)
        call_fwd(Zb, bias_t, act, Y)
        out[yt] = E.unstore(Y.read(), rows, n, ld, off)
    for yt in (F16, BF16):
        assert same(out[yt], E.rne_bits(out[F32], yt)), yt
    for dyt in DTS:
        dYb = Buf(E.rne_bits(dY32, dyt), ld, dyt, off)
        out, db = {}, {}
        for dzt in DTS:
            dZ = out_buf(rows, n, ld, dzt, off)
            dbias_t = torch.full((rows,), float("nan"), device="cuda")
            call_bwd(dYb, Zb, bias_t, act, dZ, dbias_t, scratch_for(rows, n))
            out[dzt], db[dzt] = E.unstore(dZ.read(), rows, n, ld, off), dbias_t.cpu().numpy()
        for dzt in (F16, BF16):
            assert same(out[dzt], E.rne_bits(out[F32], dzt)), (dyt, dzt)
            assert same(db[dzt], db[F32]), (dyt, dzt)                                                       # the sums are of the fp32 dz, whatever is stored
        assert same(db[F32], E.dbias_of(out[F32])), dyt                                                     # ... in the pinned order, GELU included


# ---- 3. GELU against float64 ---------------------------------------------------------------------------------------------------------------------------
def gelu_measures(u, dy, y, dz):
    """the error measures of the issue, against fp64 on the float32 u"""
    u64, dy64 = u.astype(np.float64), dy.astype(np.float64)
    erf = np.vectorize(math.erf, otypes=[np.float64])(u64 / math.sqrt(2.0))
    y_ref = 0.5 * u64 * (1.0 + erf)
    dz_ref = dy64 * (0.5 * (1.0 + erf) + u64 * np.exp(-0.5 * u64 * u64) / math.sqrt(2.0 * math.pi))
    my = np.max(np.abs(y.astype(np.float64) - y_ref) / (2.0 ** -24 * np.maximum(np.abs(u64), 2.0 ** -10)))
    mdz = np.max(np.abs(dz.astype(np.float64) - dz_ref) / (2.0 ** -24 * np.abs(dy64) * np.maximum(1.0, np.abs(u64))))
    return float(my), float(mdz)


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
def test_gelu_against_float64(with_bias):
    rows, n, ld = 261, 129, 264
    rng = np.random.default_rng(11 + with_bias)
    Z = rng.uniform(-6, 6, (rows, n))
    Z[:, ::3] = rng.uniform(-0.05, 0.05, (rows, (n + 2) // 3))                                             # dense around 0
    Z[:, 1::9] = rng.uniform(-1e-3, 1e-3, (rows, len(range(1, n, 9)))) * 10.0 ** rng.integers(-4, 1, (rows, len(range(1, n, 9))))
    Z = Z.astype(f32)
    b = rng.uniform(-0.25, 0.25, rows).astype(f32) if with_bias else None
    dY = (rng.standard_normal((rows, n)) * 10.0 ** rng.integers(-3, 4, (rows, n))).astype(f32)
    dY[dY == 0] = 1.0
    u = E._u(Z, b)
    assert np.abs(u).max() <= 6.25
    Zb, dYb, bias_t = Buf(Z, ld, F32), Buf(dY, ld, F32), vec(b)
    Y, dZ = out_buf(rows, n, ld, F32, 0), out_buf(rows, n, ld, F32, 0)
    dbias_t = torch.full((rows,), float("nan"), device="cuda")
    call_fwd(Zb, bias_t, GELU, Y)
    call_bwd(dYb, Zb, bias_t, GELU, dZ, dbias_t, scratch_for(rows, n))
    y, dz = E.unstore(Y.read(), rows, n, ld), E.unstore(dZ.read(), rows, n, ld)
    ut = torch.from_numpy(u.copy()).requires_grad_(True)
    yt = torch.nn.functional.gelu(ut)
    yt.backward(torch.from_numpy(dY))
    ours, torchs = gelu_measures(u, dY, y, dz), gelu_measures(u, dY, yt.detach().numpy(), ut.grad.numpy())
    print("gelu measures (y, dz): kernel %.3f %.3f   torch CPU float32 %.3f %.3f" % (ours + torchs))
    assert ours[0] <= 4 * torchs[0] + 1, (ours, torchs)
    assert ours[1] <= 4 * torchs[1] + 1, (ours, torchs)
    assert same(dbias_t.cpu().numpy(), E.dbias_of(dz))                                                      # the fixed-order fp64 sum of the kernel's own fp32 dz


# ---- 4. poison -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [NONE, RELU, GELU], ids=["none", "relu", "gelu"])
def test_a_nan_in_a_row_of_dy_reaches_exactly_that_dbias(act):
    rows, n, ld = 67, 129, 70
    rng = np.random.default_rng(3)
    Z = rng.uniform(0.5, 3, (rows, n)).astype(f32)                       # u > 0: nothing is masked
    dY = rng.standard_normal((rows, n)).astype(f32)
    hit = {5: 0, 31: 31, 40: 32, 66: 128}                                # row -> column of its NaN: the ends of runs, the tail run
    for r, c in hit.items():
        dY[r, c] = np.nan
    dZ = out_buf(rows, n, ld, F32, 0)
    dbias_t = torch.full((rows,), float("nan"), device="cuda")
    call_bwd(Buf(dY, ld, F32), Buf(Z, ld, F32), None, act, dZ, dbias_t, scratch_for(rows, n))
    db, dz = dbias_t.cpu().numpy(), E.unstore(dZ.read(), rows, n, ld)
    assert sorted(np.flatnonzero(np.isnan(db)).tolist()) == sorted(hit)
    assert sorted(zip(*[a.tolist() for a in np.nonzero(np.isnan(dz))])) == sorted(hit.items())
    # ... and under a masked position it reaches nothing
    if act == RELU:
        Z2 = Z.copy()
        for r, c in hit.items():
            Z2[r, c] = -1.0
        dbias_t.fill_(float("nan"))
        call_bwd(Buf(dY, ld, F32), Buf(Z2, ld, F32), None, act, dZ, dbias_t, scratch_for(rows, n))
        assert np.isfinite(dbias_t.cpu().numpy()).all() and np.isfinite(E.unstore(dZ.read(), rows, n, ld)).all()


# ---- 5. in place -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [NONE, RELU, GELU], ids=["none", "relu", "gelu"])
def test_in_place_gives_the_bits_of_out_of_place(act):
    for rows, n, extra, off in ((261, 33, 3, 0), (64, 129, 0, 0), (67, 2, 0, 1)):
        ld = rows + extra
        Z, dY32, b = operands(rows, n, 77 + rows)
        if act == GELU:
            Z, dY32 = np.nan_to_num(Z, nan=0.5, posinf=3.0, neginf=-3.0), np.nan_to_num(dY32, nan=0.5, posinf=3.0, neginf=-3.0)
        bias_t = vec(b)
        Y = out_buf(rows, n, ld, F32, off)
        call_fwd(Buf(Z, ld, F32, off), bias_t, act, Y)
        Zb = Buf(Z, ld, F32, off, pad=SENTINEL[F32])
        call_fwd(Zb, bias_t, act, Zb)
        assert same(Zb.read(), Y.read()), ("fwd", rows, n)
        for dt in DTS:
            dYs = E.rne_bits(dY32, dt)
            dZ = out_buf(rows, n, ld, dt, off)
            d1, d2 = (torch.full((rows,), float("nan"), device="cuda") for _ in range(2))
            Zin = Buf(Z, ld, F32, off)
            call_bwd(Buf(dYs, ld, dt, off), Zin, bias_t, act, dZ, d1, scratch_for(rows, n))
            dYb = Buf(dYs, ld, dt, off, pad=SENTINEL[dt])
            call_bwd(dYb, Zin, bias_t, act, dYb, d2, scratch_for(rows, n))
            assert same(dYb.read(), dZ.read()) and same(d1.cpu().numpy(), d2.cpu().numpy()), ("bwd", rows, n, dt)


# ---- 6. determinism and capture ------------------------------------------------------------------------------------------------------------------------
def test_two_eager_calls_and_a_replay_agree_bit_for_bit():
    """fwd + bwd captured on a side stream as the very first calls of this shape (nothing to warm up: the entries only launch), one linear capture; the inputs
    rewritten in place, then the replay gives the bits of eager calls on the new inputs"""
    rows, n, ld = 259, 131, 260                                           # (a shape no other test uses)
    sets = []
    for seed in (1, 2):
        Z, dY32, b = operands(rows, n, 900 + seed)
        dY32 = np.clip(np.nan_to_num(dY32, nan=0.25, posinf=2.0, neginf=-2.0), -1000, 1000)                # (finite, also as fp16: dbias must come out finite)
        sets.append((np.nan_to_num(Z, nan=0.25, posinf=2.0, neginf=-2.0), E.rne_bits(dY32, F16), b))
    Zb, dYb, bias_t = Buf(sets[0][0], ld, F32), Buf(sets[0][1], ld, F16), vec(sets[0][2])
    Y, dZ = out_buf(rows, n, ld, BF16, 0), out_buf(rows, n, ld, F16, 0)
    dbias_t = torch.full((rows,), float("nan"), device="cuda")
    scratch = scratch_for(rows, n)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph, stream=s):
            call_fwd(Zb, bias_t, GELU, Y)
            call_bwd(dYb, Zb, bias_t, GELU, dZ, dbias_t, scratch)
            dt = C.c_float(0)
            rc = lib.sparta_epilogue_fwd(Zb.ptr(_f32p), ld, vptr(bias_t), GELU, Y.ptr(), ld, BF16, rows, n, stream(), C.byref(dt))
        assert rc == sa._lib.ERR_UNSUPPORTED and "sparta_epilogue_fwd" in lib.sparta_last_error().decode() and "captured" in lib.sparta_last_error().decode()
        torch.cuda.synchronize()
        assert same(Y.read(), Y.host0) and same(dZ.read(), dZ.host0)     # a capture runs nothing
        Zb.write(sets[1][0]); dYb.write(sets[1][1]); bias_t.copy_(torch.from_numpy(sets[1][2]))
        gph.replay()
        torch.cuda.synchronize()
    replayed = (Y.read(), dZ.read(), dbias_t.cpu().numpy())
    eager = []
    for _ in range(2):
        Y2, dZ2 = out_buf(rows, n, ld, BF16, 0), out_buf(rows, n, ld, F16, 0)
        d2 = torch.full((rows,), float("nan"), device="cuda")
        call_fwd(Zb, bias_t, GELU, Y2)
        call_bwd(dYb, Zb, bias_t, GELU, dZ2, d2, scratch_for(rows, n))
        eager.append((Y2.read(), dZ2.read(), d2.cpu().numpy()))
    for a, b_, c in zip(replayed, eager[0], eager[1]):
        assert same(a, b_) and same(b_, c)
    assert np.isfinite(replayed[2]).all()
    dt = C.c_float(-1.0)                                                  # ... and outside a capture dt_ms times the kernels
    sa._lib.check(lib.sparta_epilogue_fwd(Zb.ptr(_f32p), ld, vptr(bias_t), GELU, Y.ptr(), ld, BF16, rows, n, stream(), C.byref(dt)))
    assert dt.value > 0.0


# ---- 7. edge sizes -----------------------------------------------------------------------------------------------------------------------------------------
def test_edge_sizes():
    rows = 67
    dbias_t = torch.full((rows,), float("nan"), device="cuda")
    any_t = torch.zeros(8, device="cuda")
    p = C.c_void_p(any_t.data_ptr())
    pf = C.cast(p, _f32p)
    # n_cols == 0 with dbias: zeros (+0.0f); without: nothing
    sa._lib.check(lib.sparta_epilogue_bwd(p, rows, F32, pf, rows, None, RELU, p, rows, F32, vptr(dbias_t), None, rows, 0, stream(), None))
    assert not E.bits(dbias_t.cpu().numpy()).any()
    sa._lib.check(lib.sparta_epilogue_bwd(None, rows, F32, None, rows, None, RELU, None, rows, F32, None, None, rows, 0, stream(), None))
    sa._lib.check(lib.sparta_epilogue_fwd(None, rows, None, RELU, None, rows, F16, rows, 0, stream(), None))
    # rows == 0
    sa._lib.check(lib.sparta_epilogue_fwd(None, 0, None, GELU, None, 0, F32, 0, 5, stream(), None))
    sa._lib.check(lib.sparta_epilogue_bwd(None, 0, BF16, None, 0, None, GELU, None, 0, F32, None, None, 0, 40, stream(), None))
    torch.cuda.synchronize()
    assert not any_t.cpu().numpy().any()
    # the torch layer: shapes with nothing in them
    y = sa.epilogue_fwd(torch.zeros((0, rows), device="cuda"), None, "relu", torch.float16)
    dz, db = sa.epilogue_bwd(torch.zeros((0, rows), device="cuda"), torch.zeros((0, rows), device="cuda"), None, "relu", torch.float32, True)
    assert y.shape == (0, rows) and y.dtype == torch.float16 and dz.shape == (0, rows) and not E.bits(db.cpu().numpy()).any()


# ---- 8. the torch functions ------------------------------------------------------------------------------------------------------------------------------
def test_torch_functions_match_the_entries():
    rows, n = 67, 33
    Z, dY32, b = operands(rows, n, 21)
    zt, bt = vec(Z.T), vec(b)
    for act in (NONE, RELU):
        for dt, tdt in ((F32, torch.float32), (F16, torch.float16), (BF16, torch.bfloat16)):
            y = sa.epilogue_fwd(zt, bt, E.ACT_NAME[act], tdt)
            got = y.view(torch.int16).cpu().numpy().view(np.uint16) if dt != F32 else y.cpu().numpy()
            assert same(got.T, E.fwd_ref(Z, b, act, dt))
            gy = vec(E.widen(E.rne_bits(dY32, dt), dt).T).to(tdt)
            dz, db = sa.epilogue_bwd(gy, zt, bt, E.ACT_NAME[act], tdt, True)
            dz_ref, db_ref = E.bwd_ref(E.widen(E.rne_bits(dY32, dt), dt), Z, b, act, dt)
            got = dz.view(torch.int16).cpu().numpy().view(np.uint16) if dt != F32 else dz.cpu().numpy()
            assert same(got.T, dz_ref) and same(db.cpu().numpy(), db_ref)
            assert sa.epilogue_bwd(gy, zt, bt, E.ACT_NAME[act], tdt, False)[1] is None
    z2 = zt.clone()
    assert sa.epilogue_fwd(z2, bt, "relu", out=z2) is z2 and same(z2.cpu().numpy().T, E.fwd_ref(Z, b, RELU))
    with pytest.raises(ValueError):
        sa.epilogue_fwd(zt, bt, "tanh")
    with pytest.raises(ValueError):
        sa.epilogue_fwd(zt, bt[:-1], "relu")
    with pytest.raises(ValueError):
        sa.epilogue_bwd(zt, None, None, "relu", torch.float32, False)


# ---- 9. the cached scratch of the bias gradient outlives the graph that captured it ------------------------------------------------------------------------
def test_scratch_outlives_the_capture_that_took_its_address(monkeypatch):
    """a graph that captured epilogue_bwd at (90, 33) has the scratch tensor's address in its node; an eager call at (200, 65) then needs a larger scratch.
    The first tensor must stay alive: freed, its block goes back to torch's allocator and a replay writes fp64 partials into whatever lives there next.
    The host-side assertion (a weakref taken before the growth) stands in front of the replay, so code that frees the tensor fails here without a write to
    freed memory; then a sentinel of the old scratch's size is allocated and filled, and the replay gives the bits of dbias_of and leaves the sentinel alone."""
    import weakref
    monkeypatch.setattr(sa.epilogue, "_SCRATCH", {})                      # a cache of this test's own: what earlier tests grew it to does not matter
    rows, n = 90, 33
    sets = []
    for seed in (31, 32):
        Z, dY32, b = operands(rows, n, seed)
        sets.append((np.nan_to_num(Z, nan=0.25, posinf=2.0, neginf=-2.0), np.clip(np.nan_to_num(dY32, nan=0.25, posinf=2.0, neginf=-2.0), -1000, 1000), b))
    z, gy, bt = vec(sets[0][0].T), vec(sets[0][1].T), vec(sets[0][2])
    big = torch.zeros((65, 200), device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        sa.epilogue_bwd(gy, z, bt, "relu", torch.float32, True)           # eager: the scratch is made here (a capture refuses to)
        first = sa.epilogue._SCRATCH[gy.device.index]
        nbytes = first.numel() * 8
        assert nbytes == sa.epilogue.scratch_bytes(rows, n) > 0
        alive = weakref.ref(first)
        del first
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph, stream=s):
            dz, db = sa.epilogue_bwd(gy, z, bt, "relu", torch.float32, True)
        sa.epilogue_bwd(big, big, None, "relu", torch.float32, True)      # eager, larger: the cache takes a new tensor
        assert sa.epilogue._SCRATCH[gy.device.index].numel() * 8 >= sa.epilogue.scratch_bytes(200, 65) > nbytes
        assert alive() is not None, "the scratch a captured epilogue_bwd writes to was freed when the cache grew"
        sentinel = torch.full((nbytes // 8,), 7.25, dtype=torch.float64, device="cuda")
        z.copy_(vec(sets[1][0].T)); gy.copy_(vec(sets[1][1].T)); bt.copy_(vec(sets[1][2]))
        gph.replay()
        torch.cuda.synchronize()
    dz_ref, db_ref = E.bwd_ref(sets[1][1], sets[1][0], sets[1][2], RELU)
    assert same(dz.cpu().numpy().T, dz_ref) and same(db.cpu().numpy(), db_ref)
    assert bool((sentinel == 7.25).all())
