"""sparta_epilogue_fwd / sparta_epilogue_bwd (k_epilogue.hip) and vbs_linear's bias / activation / out_dtype without a GPU: fwd_ref and bwd_ref
(tests/_epilogue.py), the numpy float32 restatement that tests/test_epilogue_gpu.py holds the kernels to bit for bit, are float32 at every intermediate and
give torch's relu(z + b) and an fp64-accurate bias gradient; the entries are exported with the declared prototypes; every refusal comes with a message that
names the entry and before anything touches a device; sparta_amd.epilogue imports without torch; vbs_linear refuses bad arguments with ValueError."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd import _lib
from sparta_amd._lib import lib

import _epilogue as E
from _epilogue import f32, F32, F16, BF16, NONE, RELU, GELU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the references ------------------------------------------------------------------------------------------------------------------------------------
def test_refs_are_float32_at_every_intermediate():
    """_f inside the references asserts it on the way; a float64 operand must trip it"""
    rng = np.random.default_rng(0)
    Z, dY, b = E.special_values(rng, (67, 33)), E.special_values(rng, (67, 33)), rng.standard_normal(67).astype(f32)
    for act in (NONE, RELU, GELU):
        for dt in (F32, F16, BF16):
            y = E.fwd_ref(Z, b, act, dt)
            dz, db = E.bwd_ref(dY, Z, b, act, dt)
            assert y.dtype == E.NP_STORE[dt] and dz.dtype == E.NP_STORE[dt] and db.dtype == f32 and y.shape == dz.shape == (67, 33) and db.shape == (67,)
    with pytest.raises(AssertionError):
        E.fwd_ref(Z.astype(np.float64), b, RELU)
    with pytest.raises(AssertionError):
        E.bwd_ref(dY, Z, b.astype(np.float64), RELU)
    # the conversions: exact widening, nearest even, Inf stays Inf, a NaN stays a NaN
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65520.0, np.inf, -np.inf, np.nan, -0.0], f32)
    assert E.rne_bits(x, BF16).tolist() == [0x3f80, 0x3f80, 0x3f82, 0x3f80, 0x3f80, 0x4780, 0x7f80, 0xff80, 0x7fc0, 0x8000]
    assert E.rne_bits(x, F16).tolist() == [0x3c00, 0x3c00 + 4, 0x3c00 + 12, 0x3c00, 0x3c00 + 2, 0x7c00, 0x7c00, 0xfc00, 0x7e00, 0x8000]
    for dt in (F16, BF16):
        again = E.rne_bits(E.widen(E.rne_bits(x, dt), dt), dt)
        assert np.array_equal(again, E.rne_bits(x, dt))


@pytest.mark.parametrize("act", [NONE, RELU])
def test_fwd_ref_is_torch_relu_of_z_plus_b_bit_for_bit(act):
    """... with ONE exception, which the pinned table decides: u = -0.0 gives +0.0f ((u <= 0) ? +0.0f : u), where torch's CPU relu hands the -0.0 through.
    The data hold -0.0 on purpose (under no bias, and under a zero bias where u = -0.0 + 0.0 = +0.0); everywhere else the bits are torch's."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(1)
    Z = (rng.standard_normal((261, 33)) * 3).astype(f32)
    Z[rng.integers(261, size=40), rng.integers(33, size=40)] = rng.choice(np.array([0.0, -0.0, 1e-30, -1e-30], f32), 40)
    b = rng.standard_normal(261).astype(f32)
    b[::7] = 0.0
    for bias in (b, None):
        t = torch.from_numpy(Z.T.copy())                                     # (n, rows), as the layer holds it
        if bias is not None:
            t = t + torch.from_numpy(bias)
        want = (torch.relu(t) if act == RELU else t).numpy().T
        got = E.fwd_ref(Z, bias, act)
        neg_zero = (E.bits(np.ascontiguousarray(t.numpy().T)) == 0x80000000) & (act == RELU)
        assert neg_zero.any() == (bias is None and act == RELU)             # (the case is in the data, and only there)
        assert np.array_equal(E.bits(got)[~neg_zero], E.bits(np.ascontiguousarray(want))[~neg_zero])
        assert not E.bits(got)[neg_zero].any()                               # +0.0f where u is -0.0
        for dt, tdt in ((F16, torch.float16), (BF16, torch.bfloat16)):
            want16 = (torch.relu(t) if act == RELU else t).to(tdt).view(torch.int16).numpy().view(np.uint16).T
            assert np.array_equal(E.fwd_ref(Z, bias, act, dt)[~neg_zero], want16[~neg_zero])


def test_relu_backward_is_a_select():
    Z = np.array([[-1.0, 0.0, -0.0, 2.0, np.nan]], f32)
    dY = np.array([[np.nan, np.inf, 5.0, np.nan, 7.0]], f32)
    dz, db = E.bwd_ref(dY, Z, None, RELU)
    assert E.bits(dz).tolist() == [[0, 0, 0, 0x7fc00000, E.bits(np.array([7.0], f32))[0]]] and np.isnan(db[0])
    y = E.fwd_ref(Z, None, RELU)
    assert E.bits(y).tolist() == [[0, 0, 0, 0x40000000, 0x7fc00000]]


@pytest.mark.parametrize("n", [1, 31, 32, 33, 129])
def test_dbias_of_bwd_ref_is_an_fp64_sum(n):
    rng = np.random.default_rng(n)
    rows = 67
    dY = (rng.standard_normal((rows, n)) * 10.0 ** rng.integers(-3, 4, (rows, n))).astype(f32)
    Z = rng.standard_normal((rows, n)).astype(f32)
    b = rng.standard_normal(rows).astype(f32)
    for act in (NONE, RELU, GELU):
        dz = E.bwd_f32(dY, Z, b, act)
        _, db = E.bwd_ref(dY, Z, b, act)
        for i in range(rows):
            s = math.fsum(float(v) for v in dz[i])
            bound = 2.0 ** -24 * abs(s) + n * 2.0 ** -53 * float(np.abs(dz[i].astype(np.float64)).sum())
            assert abs(float(db[i]) - s) <= bound, (act, i, float(db[i]), s, bound)
    assert E.bits(E.dbias_of(np.zeros((3, 0), f32))).tolist() == [0, 0, 0]
    assert E.bits(E.dbias_of(np.full((2, 40), -0.0, f32))).tolist() == [0, 0]          # (0.0 + -0.0 = +0.0)


def test_gelu_refs_against_float64():
    u = np.linspace(-6, 6, 4001).astype(f32)[None, :]
    y = E.fwd_ref(u, None, GELU)[0].astype(np.float64)
    u64 = u[0].astype(np.float64)
    erf = np.array([math.erf(v / math.sqrt(2.0)) for v in u64])
    want = 0.5 * u64 * (1.0 + erf)
    assert np.max(np.abs(y - want) / (2.0 ** -24 * np.maximum(np.abs(u64), 2.0 ** -10))) < 64
    dz, _ = E.bwd_ref(np.ones_like(u), u, None, GELU)
    wantd = 0.5 * (1.0 + erf) + u64 * np.exp(-0.5 * u64 * u64) / math.sqrt(2.0 * math.pi)
    assert np.max(np.abs(dz[0].astype(np.float64) - wantd) / (2.0 ** -24 * np.maximum(1.0, np.abs(u64)))) < 64


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_prototypes():
    f32p, vp, i64, i32 = C.POINTER(C.c_float), C.c_void_p, C.c_int64, C.c_int32
    for name in ("sparta_epilogue_fwd", "sparta_epilogue_scratch_bytes", "sparta_epilogue_bwd"):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert list(lib.sparta_epilogue_fwd.argtypes) == [f32p, i64, f32p, i32, vp, i64, i32, i64, i64, vp, f32p]
    assert list(lib.sparta_epilogue_scratch_bytes.argtypes) == [i64, i64, C.POINTER(i64)]
    assert list(lib.sparta_epilogue_bwd.argtypes) == [vp, i64, i32, f32p, i64, f32p, i32, vp, i64, i32, f32p, vp, i64, i64, vp, f32p]
    assert (_lib.ACT_NONE, _lib.ACT_RELU, _lib.ACT_GELU, _lib.EPILOGUE_RUN) == (0, 1, 2, 32) == (NONE, RELU, GELU, E.RUN)
    hdr = open(os.path.join(ROOT, "include", "sparta_amd.h")).read()
    for text in ("#define SPARTA_ACT_NONE 0\n#define SPARTA_ACT_RELU 1\n#define SPARTA_ACT_GELU 2\n#define SPARTA_EPILOGUE_RUN 32\n",
                 "int sparta_epilogue_fwd(const float* Z, int64_t ldz, const float* bias, int32_t act,\n"
                 "                        void* Y, int64_t ldy, int32_t y_dtype, int64_t rows, int64_t n_cols, void* stream, float* dt_ms);",
                 "int sparta_epilogue_scratch_bytes(int64_t rows, int64_t n_cols, int64_t* bytes_out);",
                 "int sparta_epilogue_bwd(const void* dY, int64_t lddy, int32_t dy_dtype, const float* Z, int64_t ldz, const float* bias, int32_t act,\n"
                 "                        void* dZ, int64_t lddz, int32_t dz_dtype, float* dbias, void* scratch,\n"
                 "                        int64_t rows, int64_t n_cols, void* stream, float* dt_ms);",
                 "Y[i,j] depends on Z[i,j] and bias[i] only", "dZ[i,j] depends on dY[i,j], Z[i,j] and bias[i] only", "are neither read into a result nor written"):
        assert text in hdr, text
    assert sa.epilogue_fwd is sa.epilogue.epilogue_fwd and sa.epilogue_bwd is sa.epilogue.epilogue_bwd


def _f32p(addr):
    return C.cast(C.c_void_p(addr), C.POINTER(C.c_float))


def test_refusals_name_the_entry_and_launch_nothing():
    """every refusal comes before anything touches the device: the pointers below are never dereferenced (this machine may have no GPU at all)"""
    A, B, D, S = 0x10000, 0x20000, 0x30000, 0x40000                   # "device pointers", 16-byte aligned
    R, N = 8, 4

    def refused(rc, entry, word):
        msg = lib.sparta_last_error().decode()
        assert rc == _lib.ERR_INVALID and entry in msg and word in msg, (rc, msg, word)

    def fwd(Z=A, ldz=R, bias=B, act=RELU, Y=D, ldy=R, yt=F32, rows=R, n=N):
        return lib.sparta_epilogue_fwd(_f32p(Z), ldz, _f32p(bias), act, C.c_void_p(Y), ldy, yt, rows, n, None, None)

    e = "sparta_epilogue_fwd"
    refused(fwd(Z=None), e, "Z is NULL")
    refused(fwd(Y=None), e, "Y is NULL")
    refused(fwd(ldz=R - 1), e, "ld < rows")
    refused(fwd(ldy=R - 1), e, "ld < rows")
    refused(fwd(rows=-1), e, "rows < 0")
    refused(fwd(n=-1), e, "n_cols < 0")
    refused(fwd(act=3), e, "act")
    refused(fwd(act=-1), e, "act")
    refused(fwd(yt=3), e, "dtype")
    refused(fwd(yt=-1), e, "dtype")
    refused(fwd(Z=A + 2), e, "Z is not aligned")
    refused(fwd(Y=D + 2), e, "Y is not aligned")
    refused(fwd(Y=D + 1, yt=F16), e, "Y is not aligned")
    refused(fwd(bias=B + 2), e, "bias is not aligned")

    def bwd(dY=A, lddy=R, dyt=F32, Z=B, ldz=R, bias=None, act=RELU, dZ=D, lddz=R, dzt=F32, dbias=None, scratch=None, rows=R, n=N):
        return lib.sparta_epilogue_bwd(C.c_void_p(dY), lddy, dyt, _f32p(Z), ldz, _f32p(bias), act, C.c_void_p(dZ), lddz, dzt, _f32p(dbias), C.c_void_p(scratch),
                                       rows, n, None, None)

    e = "sparta_epilogue_bwd"
    refused(bwd(dY=None), e, "dY is NULL")
    refused(bwd(dZ=None), e, "dZ is NULL")
    refused(bwd(Z=None, act=RELU), e, "Z is NULL")
    refused(bwd(Z=None, act=GELU), e, "Z is NULL")
    refused(bwd(lddy=R - 1), e, "ld < rows")
    refused(bwd(ldz=R - 1), e, "ld < rows")
    refused(bwd(lddz=R - 1), e, "ld < rows")
    refused(bwd(rows=-2), e, "rows < 0")
    refused(bwd(n=-2), e, "n_cols < 0")
    refused(bwd(act=7), e, "act")
    refused(bwd(dyt=3), e, "dtype")
    refused(bwd(dzt=9), e, "dtype")
    refused(bwd(dY=A + 1, dyt=BF16), e, "dY is not aligned")
    refused(bwd(dY=A + 2), e, "dY is not aligned")
    refused(bwd(Z=B + 2), e, "Z is not aligned")
    refused(bwd(dZ=D + 1, dzt=F16), e, "dZ is not aligned")
    refused(bwd(bias=S + 1), e, "bias is not aligned")
    refused(bwd(dbias=S + 2), e, "dbias is not aligned")
    refused(bwd(dbias=S, scratch=None, n=E.RUN + 1), e, "scratch is NULL")
    refused(bwd(dbias=S, scratch=S + 0x1004, n=E.RUN + 1), e, "scratch")
    out = C.c_int64(-1)
    assert lib.sparta_epilogue_scratch_bytes(-1, 4, C.byref(out)) == _lib.ERR_INVALID and "sparta_epilogue_scratch_bytes" in lib.sparta_last_error().decode()
    assert lib.sparta_epilogue_scratch_bytes(4, 4, None) == _lib.ERR_INVALID and "sparta_epilogue_scratch_bytes" in lib.sparta_last_error().decode()


def test_scratch_bytes_is_a_function_of_the_shape():
    seen = {}
    for _ in range(2):
        for rows in (0, 1, 3, 64, 67, 261, 62464):
            for n in (0, 1, 2, 31, 32, 33, 128, 129):
                b = sa.epilogue.scratch_bytes(rows, n)
                assert b >= 0 and b % 8 == 0 and seen.setdefault((rows, n), b) == b
                if n <= E.RUN or rows == 0:
                    assert b == 0                                        # one run: the sums need no partials
                else:
                    assert b >= 8 * rows                                 # (at least one fp64 partial per row)


# ---- imports and arguments -------------------------------------------------------------------------------------------------------------------------------
def test_epilogue_imports_without_torch():
    """sparta_amd with the epilogue in a process where `import torch` fails: the modules load and the handle-free entry that needs no tensor works"""
    code = ("import sys; sys.modules['torch'] = None\n"
            "import sparta_amd.epilogue as e, sparta_amd.autograd as a, sparta_amd as sa\n"
            "assert sa.epilogue_fwd is e.epilogue_fwd and sa.epilogue_bwd is e.epilogue_bwd and sa._lib.EPILOGUE_RUN == 32\n"
            "assert e.scratch_bytes(10, 64) == e.scratch_bytes(10, 64) and e.activation_code('gelu') == 2\n"
            "try:\n"
            "    e.epilogue_fwd(None)\n"
            "except ImportError:\n"
            "    print('ok')\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)
    for mod in ("epilogue.py", "autograd.py"):
        src = open(os.path.join(ROOT, "sparta_amd", mod)).read()
        assert not [ln for ln in src.splitlines() if ln.startswith(("import torch", "from torch"))], mod


def test_vbs_linear_refuses_bad_epilogue_arguments():
    torch = pytest.importorskip("torch")
    from test_vbs_linear_host import StubHandle, ROWS, COLS, NZ, N, ints

    class Stub(StubHandle):
        updatable = transposable = True
        device = 0

    H, x, W = Stub(), ints((N, COLS), 1), ints(NZ, 2)
    good = torch.zeros(ROWS)
    with pytest.raises(ValueError, match="activation"):
        sa.autograd.vbs_linear(x, H, W, activation="silu")
    with pytest.raises(ValueError, match="activation"):
        sa.autograd.vbs_linear(x, H, W, activation=None)
    with pytest.raises(ValueError, match="out_dtype"):
        sa.autograd.vbs_linear(x, H, W, out_dtype=torch.float64)
    with pytest.raises(ValueError, match="out_dtype"):
        sa.autograd.vbs_linear(x, H, W, out_dtype="float16")
    for bad in (torch.zeros(ROWS + 1), torch.zeros(ROWS, 1), torch.zeros(ROWS, dtype=torch.float64), torch.zeros(ROWS, dtype=torch.float16),
                torch.zeros(2 * ROWS)[::2], np.zeros(ROWS, f32), good):                    # (the last: a good bias, but not on the handle's device)
        with pytest.raises(ValueError, match="bias"):
            sa.autograd.vbs_linear(x, H, W, bias=bad, activation="relu")
    with pytest.raises(TypeError):
        sa.autograd.vbs_linear(x, H, W, False, good)                                       # the new arguments are keyword-only: `refresh` keeps its place
    assert H.calls == {}                                                                   # nothing reached the handle
