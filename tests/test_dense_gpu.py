"""sparta_dense_block_ssq / sparta_vbs_gather_dense / sparta_vbs_scatter_dense (k_dense.hip) on the GPU, through DeviceVBS.gather_dense / scatter_dense /
to_dense, sparta_amd.dense_block_ssq and sparta_amd.sparsify.

Geometries: every fp32 edge geometry of tests/_util.py, plus the interior block-row range (1, block_rows - 1) of those with at least three block-rows.  D is
float32, float16 and bfloat16, row- and column-major, with the minimal leading dimension and that plus 3, starting 0, 1, 2, 3 and 5 elements past a 16-byte
boundary; T starts 0 .. 3 floats past one; both sit inside canary buffers whose every word is checked.  (A matrix with one column or one row has only one
memory layout: torch strides cannot tell row- from column-major there, and the wrapper takes the first that fits.)

References, by numpy alone: the gather is U.edge_sample -- applied to the matrix of flat element numbers, so that the bits of D can be looked up without
passing through float64, which would quieten a signalling NaN; the scatter is U.edge_dense / U.edge_round; the scores are tests/_dense.py::grid_ssq.  The
score bound 2 * n_in * 2^-53 * ssq is the header's bound of any order of n_in fp64 additions of non-negative terms, once for the kernel and once for
numpy's own summation."""
import ctypes as C
import functools

import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd import _lib
from sparta_amd._lib import lib

torch = pytest.importorskip("torch")

import _dense as DN  # noqa: E402
import _util as U  # noqa: E402

pytestmark = pytest.mark.gpu

DTS = (sa.F32, sa.F16, sa.BF16)
DT_ID = {sa.F32: "f32", sa.F16: "f16", sa.BF16: "bf16"}
NP_BITS = {sa.F32: np.uint32, sa.F16: np.uint16, sa.BF16: np.uint16}
D_CANARY = {sa.F32: 0x7FA5C3E1, sa.F16: 0x7DA5, sa.BF16: 0x7FA5}
T_CANARY = 0x7FC0DEAD
PAD = 64                                                            # elements in front of and behind an operand: a multiple of 16 bytes in every type
EXTRA_LD = (0, 3)
D_OFFS = (0, 1, 2, 3, 5)
T_OFFS = (0, 1, 2, 3)
SPECIALS = {sa.F32: (0x7FC00001, 0x7F800001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00000000),
            sa.F16: (0x7E01, 0x7C01, 0xFE55, 0x7C00, 0xFC00, 0x8000, 0x0001, 0x83FF, 0x0000),
            sa.BF16: (0x7FC1, 0x7F81, 0xFFD5, 0x7F80, 0xFF80, 0x8000, 0x0001, 0x807F, 0x0000)}


def torch_dt(dt):
    return {sa.F32: torch.float32, sa.F16: torch.float16, sa.BF16: torch.bfloat16}[dt]


def to_device_bits(bits, dt):
    """a flat numpy array of element bit patterns as a device tensor of the element type"""
    if dt == sa.F32:
        return torch.from_numpy(bits.view(np.int32).copy()).cuda().view(torch.float32)
    return torch.from_numpy(bits.view(np.int16).copy()).cuda().view(torch_dt(dt))


def bits_of(t, dt):
    return t.view(torch.int32 if dt == sa.F32 else torch.int16).cpu().numpy().view(NP_BITS[dt])


def widen(bits, dt):
    """element bit patterns -> the bits of the float32 with the same value"""
    if dt == sa.F32:
        return bits.astype(np.uint32)
    if dt == sa.BF16:
        return bits.astype(np.uint32) << 16
    return bits.view(np.float16).astype(np.float32).view(np.uint32)


def narrow_bits(x64, dt):
    """a float64 array that holds values of the element type -> their bit patterns"""
    with np.errstate(over="ignore", invalid="ignore"):
        if dt == sa.F16:
            return x64.astype(np.float16).view(np.uint16)
        u = x64.astype(np.float32).view(np.uint32)
    return u if dt == sa.F32 else (u >> 16).astype(np.uint16)


class DenseBuf:
    """a rows x cols matrix of element bit patterns inside a canary buffer on the device: .t is the strided 2-D view the entries are given"""

    def __init__(self, bits2d, dt, row_major, extra_ld, off):
        rows, cols = bits2d.shape
        self.dt, self.shape = dt, (rows, cols)
        self.ld = (cols if row_major else rows) + extra_ld
        self.strides = (self.ld, 1) if row_major else (1, self.ld)
        span = ((rows - 1) * self.strides[0] + (cols - 1) * self.strides[1] + 1) if rows and cols else 0
        self.start = PAD + off
        host = np.full(self.start + span + PAD, D_CANARY[dt], NP_BITS[dt])
        self._view(host)[...] = bits2d
        self.inside = np.zeros(len(host), bool)
        self._view(self.inside)[...] = True
        self.flat = to_device_bits(host, dt)
        self.t = torch.as_strided(self.flat, (rows, cols), self.strides, self.start)

    def _view(self, flat):
        isz = flat.itemsize
        return np.lib.stride_tricks.as_strided(flat[self.start:], self.shape, (self.strides[0] * isz, self.strides[1] * isz))

    def read(self):
        """(the matrix, True if every word outside it still holds the canary)"""
        host = bits_of(self.flat, self.dt)
        return self._view(host).copy(), bool(np.all(host[~self.inside] == D_CANARY[self.dt]))


class MabBuf:
    def __init__(self, bits, off):
        self.n, self.start = len(bits), PAD + off
        host = np.full(self.start + self.n + PAD, T_CANARY, np.uint32)
        host[self.start:self.start + self.n] = bits
        self.flat = to_device_bits(host, sa.F32)
        self.t = self.flat[self.start:self.start + self.n]

    def read(self):
        host = bits_of(self.flat, sa.F32)
        inside = np.zeros(len(host), bool)
        inside[self.start:self.start + self.n] = True
        return host[inside], bool(np.all(host[~inside] == T_CANARY))


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------------
def geo(key, values="int"):
    return U.edge_geometries(values)[key]


CASES = [(k, None) for k in U.EDGE_F32] + [(k, (1, geo(k).block_rows - 1)) for k in U.EDGE_F32 if geo(k).block_rows >= 3]
CASE_IDS = ["%s%s" % (k, "" if br is None else "-range") for k, br in CASES]
grid = [pytest.mark.parametrize("case", CASES, ids=CASE_IDS), pytest.mark.parametrize("dt", DTS, ids=[DT_ID[d] for d in DTS]),
        pytest.mark.parametrize("row_major", (True, False), ids=("rm", "cm"))]

_HANDLES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for d in _HANDLES.values():
        d.close()
    _HANDLES.clear()


def handle(case):
    if case not in _HANDLES:
        key, br = case
        _HANDLES[case] = geo(key).to_device(0, block_row_range=br, updatable=True)
    return _HANDLES[case]


def row_range(case):
    v, br = geo(case[0]), case[1]
    b0, b1 = (0, v.block_rows) if br is None else br
    return int(v.row_part[b0]), int(v.row_part[b1])


@functools.lru_cache(maxsize=None)
def dense_bits(key, dt):
    """rows x cols random element bit patterns (NaN payloads of both kinds, Inf, -0.0, denormals among them and planted)"""
    v = geo(key)
    rng = np.random.default_rng(8100 + 10 * U.EDGE_F32.index(key) + dt)
    bits = rng.integers(0, 1 << (32 if dt == sa.F32 else 16), v.rows * v.cols, dtype=np.uint64).astype(NP_BITS[dt])
    sp = SPECIALS[dt]
    for k in range(min(bits.size, 4 * len(sp))):
        bits[(k * 7) % bits.size] = sp[k % len(sp)]
    return bits.reshape(v.rows, v.cols)


@functools.lru_cache(maxsize=None)
def sample_numbers(case):
    """per element of the mab layout of the case: 1 + the flat number of the element of the (range's) dense matrix it samples, 0 for a position past cols"""
    v, br = geo(case[0]), case[1]
    r0, r1 = row_range(case)
    numbers = 1.0 + np.arange((r1 - r0) * v.cols, dtype=np.float64).reshape(r1 - r0, v.cols)
    return U.edge_sample(v, numbers, br=br).astype(np.int64)


@functools.lru_cache(maxsize=None)
def mab_values(case):
    """nztot float32 values for the scatter: uniform values with rounding ties of both 16-bit types, 1e5 (Inf in fp16), denormals of fp32 and fp16, -0.0, Inf
    and NaN among them; the positions past cols hold 7.0 and NaN by turns"""
    idx = sample_numbers(case)
    rng = np.random.default_rng(8300 + len(idx))
    x = rng.uniform(-4, 4, len(idx)).astype(np.float32)
    special = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 3 * 2.0 ** -11), 1.0e5, -1.0e5, 65520.0, 1.0e-40, -1.0e-40,
                        1.0e-6, 2.0 ** -25, 3 * 2.0 ** -25, -0.0, np.inf, -np.inf, np.nan, 3.3895314e38, 3.4e38], np.float32)
    pos = np.arange(0, len(x), 3)
    x[pos] = special[np.arange(len(pos)) % len(special)]
    past = np.flatnonzero(idx == 0)
    x[past] = np.where(np.arange(len(past)) % 2 == 0, np.float32(7.0), np.float32(np.nan))
    return x


# ---- 1. gather -----------------------------------------------------------------------------------------------------------------------------------------
@grid[0]
@grid[1]
@grid[2]
def test_gather_dense(case, dt, row_major):
    h = handle(case)
    r0, r1 = row_range(case)
    bits = dense_bits(case[0], dt)[r0:r1]
    idx = sample_numbers(case)
    wide = widen(bits, dt).reshape(-1)
    want = np.where(idx > 0, wide[np.maximum(idx - 1, 0)] if wide.size else 0, 0).astype(np.uint32)
    f16_nan = (want & 0x7FFFFFFF) > 0x7F800000 if dt == sa.F16 else np.zeros(len(want), bool)
    assert len(want) == h.info()["nztot"]
    for extra in EXTRA_LD:
        for off in D_OFFS:
            D = DenseBuf(bits, dt, row_major, extra, off)
            for toff in T_OFFS:
                T = MabBuf(np.full(len(want), 0x7FABCDEF, np.uint32), toff)               # (every element is written)
                out = h.gather_dense(D.t, out=T.t)
                torch.cuda.synchronize()
                got, clean = T.read()
                assert out is T.t and clean, (extra, off, toff)
                assert np.array_equal(got[~f16_nan], want[~f16_nan]), (extra, off, toff, np.flatnonzero(got != want)[:8])
                assert np.all((got[f16_nan] & 0x7FFFFFFF) > 0x7F800000), (extra, off, toff)
                assert np.all(got[idx == 0] == 0), (extra, off, toff)                      # the bits of +0.0 past cols
            back, clean = D.read()
            assert clean and np.array_equal(back, bits), (extra, off)


# ---- 2. scatter ----------------------------------------------------------------------------------------------------------------------------------------
@grid[0]
@grid[1]
@grid[2]
def test_scatter_dense(case, dt, row_major):
    v, br = geo(case[0]), case[1]
    h = handle(case)
    r0, r1 = row_range(case)
    vals = mab_values(case)
    with np.errstate(invalid="ignore", over="ignore"):
        want64 = U.edge_dense(v, dtype=dt, mab=vals, br=br)
    stored = U.stored_mask(v, br=br)
    want, nan = narrow_bits(want64, dt), np.isnan(want64)
    nan_bits = (lambda b: (b & 0x7FFFFFFF) > 0x7F800000) if dt == sa.F32 else (lambda b: (b & 0x7FFF) > (0x7C00 if dt == sa.F16 else 0x7F80))
    canary = np.full((r1 - r0, v.cols), D_CANARY[dt], NP_BITS[dt])
    for extra in EXTRA_LD:
        for off in D_OFFS:
            for toff in T_OFFS:
                D = DenseBuf(canary, dt, row_major, extra, off)
                T = MabBuf(vals.view(np.uint32), toff)
                for fill in (False, True):                                                 # (the second call finds the stored blocks written and the rest canary)
                    h.scatter_dense(T.t, D.t, fill=fill)
                    torch.cuda.synchronize()
                    got, clean = D.read()
                    where = (extra, off, toff, fill)
                    assert clean, where                                                    # the ld padding and everything around the matrix
                    assert np.array_equal(got[stored & ~nan], want[stored & ~nan]), where
                    assert np.all(nan_bits(got[stored & nan])), where                      # (a float64 reference names no payload)
                    assert np.all(got[~stored] == (0 if fill else D_CANARY[dt])), where
                back, clean = T.read()
                assert clean and np.array_equal(back, vals.view(np.uint32)), (extra, off, toff)


# ---- 3. scores -----------------------------------------------------------------------------------------------------------------------------------------
def as_dense(x32, dt, row_major):
    """a float32 numpy matrix as a device tensor of the element type (rounded to nearest) in the layout; returns (tensor, the values it holds as float64)"""
    t = torch.from_numpy(np.ascontiguousarray(x32)).cuda().to(torch_dt(dt))
    held = t.to(torch.float64).cpu().numpy()
    if not row_major:
        t = t.t().contiguous().t()
    return t, held


@pytest.mark.parametrize("key", U.EDGE_F32)
@grid[1]
@grid[2]
def test_dense_block_ssq(key, dt, row_major):
    v = geo(key)
    w, rp = int(v.block_col_size), v.row_part
    rng = np.random.default_rng(8500 + U.EDGE_F32.index(key))
    n_in = DN.grid_n_in(v.rows, v.cols, rp, w)
    # small integers: every order of additions gives the same bits
    D, held = as_dense(rng.integers(-3, 4, (v.rows, v.cols)).astype(np.float32), dt, row_major)
    got = sa.dense_block_ssq(D, rp, w)
    assert got.dtype == torch.float64 and tuple(got.shape) == n_in.shape
    assert np.array_equal(got.cpu().numpy(), DN.grid_ssq(held, rp, w))
    # uniform data: the header's bound, for the kernel and for numpy's summation
    D, held = as_dense(rng.uniform(-1, 1, (v.rows, v.cols)).astype(np.float32), dt, row_major)
    ref = DN.grid_ssq(held, rp, w)
    got = sa.dense_block_ssq(D, torch.as_tensor(rp, device="cuda"), w)
    again = sa.dense_block_ssq(D, list(rp), w)
    g = got.cpu().numpy()
    assert np.all(np.abs(g - ref) <= 2 * n_in * 2.0 ** -53 * ref), np.abs(g - ref).max()
    assert np.array_equal(g.view(np.uint64), again.cpu().numpy().view(np.uint64))          # run to run
    assert np.all(g[n_in == 0] == 0.0)
    # a handle that stores every grid block and holds the gathered values scores alike
    full = sa.VBR.from_block_mask(v.rows, v.cols, rp, w, np.ones(n_in.shape, np.uint8))
    hf = full.to_device(0)
    try:
        s = hf.block_ssq(hf.gather_dense(D)).cpu().numpy().reshape(n_in.shape)
        assert np.all(np.abs(g - s) <= 2 * n_in * 2.0 ** -53 * ref), np.abs(g - s).max()
    finally:
        hf.close()
    # one NaN and one Inf change their own blocks' scores alone
    live = np.argwhere(n_in > 0)
    if len(live) >= 2:
        (ia, ja), (ib, jb) = live[0], live[-1]
        x = held.copy()
        x[rp[ia + 1] - 1, min(v.cols, ja * w + w) - 1] = np.nan
        x[rp[ib], jb * w] = np.inf
        Dp, _ = as_dense(x.astype(np.float32), dt, row_major)
        p = sa.dense_block_ssq(Dp, rp, w).cpu().numpy()
        assert np.isnan(p[ia, ja]) and np.isposinf(p[ib, jb])
        rest = np.ones(n_in.shape, bool)
        rest[ia, ja] = rest[ib, jb] = False
        assert np.array_equal(p[rest].view(np.uint64), g[rest].view(np.uint64))


def test_dense_block_ssq_strided_operand():
    """a leading dimension above the minimum and a start off the 16-byte grid, in every type and layout"""
    v = geo("heights")
    w, rp = int(v.block_col_size), v.row_part
    x = np.random.default_rng(8600).integers(-3, 4, (v.rows, v.cols)).astype(np.float32)
    want = DN.grid_ssq(x, rp, w)
    for dt in DTS:
        bits = bits_of(torch.from_numpy(x).to(torch_dt(dt)).cuda().reshape(-1), dt).reshape(x.shape)
        for row_major in (True, False):
            D = DenseBuf(bits, dt, row_major, 3, 5)
            assert np.array_equal(sa.dense_block_ssq(D.t, rp, w).cpu().numpy(), want), (dt, row_major)
            assert D.read()[1]


# ---- 4. products -----------------------------------------------------------------------------------------------------------------------------------------
PRODUCTS = [(k, sa.F32) for k in ("zeros", "heights", "tall")] + [(k, dt) for dt in (sa.F16, sa.BF16) for k in ("zeros", "heights32", "tall")]


@pytest.mark.parametrize("key,hdt", PRODUCTS, ids=["%s-%s" % (k, DT_ID[d]) for k, d in PRODUCTS])
def test_a_gathered_handle_multiplies_like_a_created_one(key, hdt):
    v = geo(key)
    arr = (v.rows, v.cols, int(v.block_col_size), v.row_part, v.nzcount, v.jab)
    rng = np.random.default_rng(8700 + len(key))
    Dn = rng.integers(-3, 4, (v.rows, v.cols)).astype(np.float32)
    ref_vbr = U.sa_vbr(arr, U.edge_sample(v, Dn).astype(np.float32))
    pattern = U.sa_vbr(arr, np.zeros(v.nztot, np.float32))
    a = pattern.to_device(0, dtype=hdt, updatable=True, transposable=True)
    b = ref_vbr.to_device(0, dtype=hdt, updatable=True, transposable=True)
    try:
        vals = a.gather_dense(torch.from_numpy(Dn).cuda())
        a.set_values(vals)
        assert np.array_equal(vals.cpu().numpy().view(np.uint32), ref_vbr.mab.view(np.uint32))
        n, op = 40, torch_dt(hdt)
        B = torch.from_numpy(rng.integers(-2, 3, v.cols * n).astype(np.float32)).cuda().to(op)
        ldx = v.rows + v.rows % 2                                                          # (16-bit handles read X with an even leading dimension)
        X = torch.from_numpy(rng.integers(-2, 3, ldx * n).astype(np.float32)).cuda().to(op)
        outs = []
        for d in (a, b):
            Cm = torch.full((v.rows * n,), 5.0, device="cuda")
            Ct = torch.full((v.cols * n,), 5.0, device="cuda")
            G = torch.full((v.nztot,), 5.0, device="cuda")
            d.spmm(B, Cm, n)
            d.spmm_t(X, Ct, n, ldx=ldx)
            d.sddmm(X, B, G, n, ldx=ldx)
            torch.cuda.synchronize()
            outs.append([t.cpu().numpy().view(np.uint32) for t in (Cm, Ct, G)])
        for name, x, y in zip(("spmm", "spmm_t", "sddmm"), *outs):
            assert np.array_equal(x, y), name
    finally:
        a.close()
        b.close()


# ---- 5. sparsify -----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sparsify_matrix():
    """96 x 160, heights 24, w 32: +-1 everywhere, and in grid block k (a shuffled numbering) k + 1 elements of +-2: normalised scores (768 + 3 (k + 1)) / 768,
    pairwise distinct -- checked here, on the CPU, so that the order of select does not hinge on its tie rule"""
    rng = np.random.default_rng(8800)
    D = rng.choice(np.array([-1.0, 1.0], np.float32), (96, 160))
    rp, w = np.arange(0, 97, 24), 32
    for k, g in enumerate(rng.permutation(20)):
        ib, jb = divmod(int(g), 5)
        D[rp[ib], jb * w:jb * w + k + 1] *= 2
    scores = DN.grid_ssq(D, rp, w) / DN.grid_n_in(96, 160, rp, w)
    assert len(np.unique(scores)) == 20
    return D, rp, w, scores


def masked_dense(D, rp, w, mask):
    return D * np.kron(mask, np.ones((1, w)))[np.repeat(np.arange(len(rp) - 1), np.diff(rp))][:, :D.shape[1]]


@grid[1]
def test_sparsify(dt):
    D, rp, w, scores = sparsify_matrix()
    Dd = torch.from_numpy(D).cuda().to(torch_dt(dt))
    mask = DN.select_mask(scores, 0.5)
    assert mask.sum() == 10
    vbmat, hd, values = sa.sparsify(Dd, w, row_block_size=24, sparsity=0.5)
    try:
        nzcount, jab, nztot = DN.block_mask_arrays(96, 160, rp, w, mask)
        assert np.array_equal(vbmat.nzcount, nzcount) and np.array_equal(vbmat.jab, jab) and np.array_equal(vbmat.row_part, rp) and vbmat.nztot == nztot
        assert values.is_leaf and values.requires_grad and values.dtype == torch.float32 and hd.updatable and hd.transposable
        assert np.array_equal(values.detach().cpu().numpy(), U.edge_sample(vbmat, D).astype(np.float32))
        Dm = masked_dense(D, rp, w, mask)
        x = np.random.default_rng(8801).integers(-2, 3, (8, 160)).astype(np.float32)
        y = sa.autograd.vbs_linear(torch.from_numpy(x).cuda(), hd, values)
        assert np.array_equal(y.detach().cpu().numpy().astype(np.float64), x.astype(np.float64) @ Dm.T.astype(np.float64))
        back = hd.to_dense(values, dtype=torch_dt(dt))
        assert back.dtype == torch_dt(dt) and tuple(back.shape) == (96, 160) and back.is_contiguous()
        assert np.array_equal(back.to(torch.float64).cpu().numpy(), Dm)
        cm = hd.to_dense(values, row_major=False)
        assert cm.stride() == (1, 96) and np.array_equal(cm.cpu().numpy().astype(np.float64), Dm)
    finally:
        hd.close()
    # nothing dropped: the dense matrix comes back bit for bit (random bit patterns, NaN payloads included, for the types that travel as bits)
    bits = dense_bits("zeros", dt)
    Db = to_device_bits(bits.reshape(-1), dt).view(96, 160)
    vb0, h0, vals0 = sa.sparsify(Db, w, row_part=rp, sparsity=0.0)
    try:
        assert vb0.nztot == 96 * 160 and int(vb0.nzcount.sum()) == 20
        back = bits_of(h0.to_dense(vals0, dtype=torch_dt(dt)).reshape(-1), dt).reshape(96, 160)
        if dt == sa.F16:                                                                   # (fp16 NaNs: a NaN comes back a NaN)
            nan = (bits & 0x7FFF) > 0x7C00
            assert np.array_equal(back[~nan], bits[~nan]) and np.all((back[nan] & 0x7FFF) > 0x7C00)
        elif dt == sa.BF16:                                                                # (the rounding of creation sets the quiet bit of a NaN)
            nan = (bits & 0x7FFF) > 0x7F80
            assert np.array_equal(back, np.where(nan, bits | 0x40, bits))
        else:
            assert np.array_equal(back, bits)
    finally:
        h0.close()
    # a pattern from elsewhere
    given = np.random.default_rng(8802).integers(0, 2, (4, 5)).astype(np.uint8)
    for m in (given, torch.from_numpy(given).cuda()):
        vb1, h1, vals1 = sa.sparsify(Dd, w, row_part=torch.as_tensor(rp), mask=m)
        try:
            assert np.array_equal(DN.geometry_block_mask(vb1), given)
            assert np.array_equal(h1.to_dense(vals1).cpu().numpy().astype(np.float64), masked_dense(D, rp, w, given))
        finally:
            h1.close()
    # a handle that takes no new values is created from the gathered ones
    vb2, h2, vals2 = sa.sparsify(Dd, w, row_block_size=24, sparsity=0.5, updatable=False, transposable=False)
    try:
        assert not h2.updatable and np.array_equal(vb2.mab, vals2.detach().cpu().numpy()) and np.array_equal(vb2.jab, jab)
        B = torch.from_numpy(np.random.default_rng(8803).integers(-2, 3, 160 * 8).astype(np.float32)).cuda()
        Cm = torch.zeros(96 * 8, device="cuda")
        h2.spmm(B, Cm, 8)
        assert np.array_equal(Cm.cpu().numpy().reshape(8, 96).T.astype(np.float64), Dm @ B.cpu().numpy().reshape(8, 160).T.astype(np.float64))
    finally:
        h2.close()
    with pytest.raises(ValueError):
        sa.sparsify(Dd, w, row_block_size=24)
    with pytest.raises(ValueError):
        sa.sparsify(Dd, w, row_block_size=24, row_part=rp, sparsity=0.5)
    with pytest.raises(ValueError):
        sa.sparsify(Dd[:, ::2], w, row_block_size=24, sparsity=0.5)                        # no stride of 1: nothing is copied silently


# ---- 6. capture ------------------------------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay():
    v = geo("zeros")
    arr = (v.rows, v.cols, int(v.block_col_size), v.row_part, v.nzcount, v.jab)
    rng = np.random.default_rng(8900)
    D1, D2 = (rng.integers(-3, 4, (v.rows, v.cols)).astype(np.float32) for _ in range(2))
    n = 16
    Bn = rng.integers(-2, 3, v.cols * n).astype(np.float32)
    D = torch.from_numpy(D1).cuda()
    B = torch.from_numpy(Bn).cuda()
    Cm = torch.zeros(v.rows * n, device="cuda")
    out = torch.full((v.rows, v.cols), 9.0, device="cuda")
    vals = torch.zeros(v.nztot, device="cuda")
    scratch = torch.zeros(8, device="cuda")
    a = U.sa_vbr(arr, np.zeros(v.nztot, np.float32)).to_device(0, updatable=True)
    s = torch.cuda.Stream()
    try:
        # a first call under capture is refused, and nothing is written
        for first in (lambda: a.gather_dense(D, out=vals), lambda: a.scatter_dense(vals, out)):
            caught = []
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                gph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gph, stream=s):
                    scratch.add_(1.0)                               # (the capture is not empty)
                    try:
                        first()
                    except sa.SpartaError as err:
                        caught.append(err)
            torch.cuda.synchronize()
            assert len(caught) == 1 and caught[0].code == _lib.ERR_UNSUPPORTED and "captured" in str(caught[0]) and "_dense" in str(caught[0])
            del gph
        assert not vals.cpu().numpy().any() and np.all(out.cpu().numpy() == 9.0)
        # one eager call, then gather + set_values + product and a scatter in one graph on one stream
        a.gather_dense(D, out=vals)
        a.set_values(vals)
        a.spmm(B, Cm, n)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            gph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gph, stream=s):
                a.gather_dense(D, out=vals)
                a.set_values(vals)
                a.spmm(B, Cm, n)
                a.scatter_dense(vals, out, fill=True)
                with pytest.raises(sa.SpartaError) as ei:           # timing synchronises
                    a.gather_dense(D, out=vals, timed=True)
                assert ei.value.code == _lib.ERR_UNSUPPORTED
        torch.cuda.synchronize()
        stored = U.stored_mask(v)
        for Dn in (D1, D2, D1):
            D.copy_(torch.from_numpy(Dn))
            Cm.fill_(7.0)
            out.fill_(9.0)
            torch.cuda.synchronize()
            gph.replay()
            torch.cuda.synchronize()
            b = U.sa_vbr(arr, U.edge_sample(v, Dn).astype(np.float32)).to_device(0)
            try:
                Cb = torch.zeros(v.rows * n, device="cuda")
                b.spmm(B, Cb, n)
                torch.cuda.synchronize()
                assert np.array_equal(Cm.cpu().numpy().view(np.uint32), Cb.cpu().numpy().view(np.uint32))
            finally:
                b.close()
            assert np.array_equal(out.cpu().numpy(), np.where(stored, Dn, np.float32(0.0)))
        # the score is capturable from its first call and replays to the same bits
        rp = torch.as_tensor(v.row_part, device="cuda")
        ssq = torch.zeros((v.block_rows, 5), dtype=torch.float64, device="cuda")
        with torch.cuda.stream(s):
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2, stream=s):
                sa.dense_block_ssq(D, rp, int(v.block_col_size), out=ssq)
        torch.cuda.synchronize()
        g2.replay()
        torch.cuda.synchronize()
        eager = sa.dense_block_ssq(D, rp, int(v.block_col_size))
        assert np.array_equal(ssq.cpu().numpy().view(np.uint64), eager.cpu().numpy().view(np.uint64))
        assert np.array_equal(eager.cpu().numpy(), DN.grid_ssq(D1, v.row_part, int(v.block_col_size)))
    finally:
        a.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------------------
def _vp(t, byte_off=0):
    return C.c_void_p(t.data_ptr() + byte_off)


def test_refusals_and_empty_work():
    v = geo("zeros")
    w = int(v.block_col_size)
    a = v.to_device(0, updatable=True)
    m = sa.gen.uniform_random(96, 160, 900, seed=3)
    csr = sa.DeviceVBS.from_csr(m, np.arange(96) // 24 * 24, 32, device=0)
    dup = sa.VBR.from_arrays(8, 96, 32, [0, 8], [3], [0, 1, 0], np.ones(8 * 32 * 3, np.float32)).to_device(0)
    empty = geo("empty").to_device(0)
    try:
        D = torch.full((96, 160), 3.0, device="cuda")
        D16 = torch.full((96, 160), 3.0, device="cuda", dtype=torch.float16)
        T = torch.full((v.nztot + 4,), 5.0, device="cuda")
        rp = torch.as_tensor(v.row_part, device="cuda")
        ssq = torch.full((4 * 5 + 1,), 11.0, dtype=torch.float64, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        RM, CM, F32, F16 = _lib.ROW_MAJOR, _lib.COL_MAJOR, _lib.F32, _lib.F16

        def untouched():
            torch.cuda.synchronize()
            return bool((D == 3.0).all() and (D16 == 3.0).all() and (T == 5.0).all() and (ssq == 11.0).all())

        gather, scatter, score = lib.sparta_vbs_gather_dense, lib.sparta_vbs_scatter_dense, lib.sparta_dense_block_ssq
        invalid = [
            gather(None, _vp(D), 160, RM, F32, _vp(T), st, None),                          # NULL handle
            gather(a.h, None, 160, RM, F32, _vp(T), st, None),                             # NULL operands with work to do
            gather(a.h, _vp(D), 160, RM, F32, None, st, None),
            gather(a.h, _vp(D), 160, 2, F32, _vp(T), st, None),                            # a layout code that does not exist
            gather(a.h, _vp(D), 160, -1, F32, _vp(T), st, None),
            gather(a.h, _vp(D), 160, RM, 3, _vp(T), st, None),                             # ... a dtype code
            gather(a.h, _vp(D), 159, RM, F32, _vp(T), st, None),                           # ldd too small
            gather(a.h, _vp(D), 95, CM, F32, _vp(T), st, None),
            gather(a.h, _vp(D, 2), 160, RM, F32, _vp(T), st, None),                        # misaligned pointers
            gather(a.h, _vp(D16, 1), 160, RM, F16, _vp(T), st, None),
            gather(a.h, _vp(D), 160, RM, F32, _vp(T, 2), st, None),
            scatter(None, _vp(T), _vp(D), 160, RM, F32, 1, st, None),
            scatter(a.h, None, _vp(D), 160, RM, F32, 1, st, None),
            scatter(a.h, _vp(T), None, 160, RM, F32, 0, st, None),
            scatter(a.h, _vp(T), _vp(D), 160, 7, F32, 1, st, None),
            scatter(a.h, _vp(T), _vp(D), 160, RM, 9, 1, st, None),
            scatter(a.h, _vp(T), _vp(D), 159, RM, F32, 1, st, None),
            scatter(a.h, _vp(T), _vp(D), 95, CM, F32, 1, st, None),
            scatter(a.h, _vp(T), _vp(D, 2), 160, RM, F32, 1, st, None),
            scatter(a.h, _vp(T), _vp(D16, 1), 160, RM, F16, 1, st, None),
            scatter(a.h, _vp(T, 1), _vp(D), 160, RM, F32, 1, st, None),
            scatter(empty.h, None, None, 200, RM, F32, 1, st, None),                       # fill on an empty pattern is work
            score(None, 160, RM, F32, 96, 160, 4, w, _vp(rp), _vp(ssq), st, None),
            score(_vp(D), 160, RM, F32, 96, 160, 4, w, None, _vp(ssq), st, None),          # row_part NULL with block_rows > 0
            score(_vp(D), 160, RM, F32, 96, 160, 4, w, _vp(rp), None, st, None),
            score(_vp(D), 160, 5, F32, 96, 160, 4, w, _vp(rp), _vp(ssq), st, None),
            score(_vp(D), 160, RM, 4, 96, 160, 4, w, _vp(rp), _vp(ssq), st, None),
            score(_vp(D), 159, RM, F32, 96, 160, 4, w, _vp(rp), _vp(ssq), st, None),
            score(_vp(D), 95, CM, F32, 96, 160, 4, w, _vp(rp), _vp(ssq), st, None),
            score(_vp(D, 2), 160, RM, F32, 96, 160, 4, w, _vp(rp), _vp(ssq), st, None),
            score(_vp(D16, 1), 160, RM, F16, 96, 160, 4, w, _vp(rp), _vp(ssq), st, None),
            score(_vp(D), 160, RM, F32, 96, 160, 4, w, _vp(rp, 4), _vp(ssq), st, None),
            score(_vp(D), 160, RM, F32, 96, 160, 4, w, _vp(rp), _vp(ssq, 4), st, None),
            score(_vp(D), 160, RM, F32, 96, 160, 4, 0, _vp(rp), _vp(ssq), st, None),
            score(_vp(D), 160, RM, F32, -1, 160, 4, w, _vp(rp), _vp(ssq), st, None),
        ]
        assert invalid == [_lib.ERR_INVALID] * len(invalid), invalid
        assert untouched()
        # handles that do not hold the caller's blocks; a block column stored twice (scatter only)
        assert gather(csr.h, _vp(D), 160, RM, F32, _vp(T), st, None) == _lib.ERR_UNSUPPORTED
        assert scatter(csr.h, _vp(T), _vp(D), 160, RM, F32, 1, st, None) == _lib.ERR_UNSUPPORTED
        Dd = torch.full((8, 96), 3.0, device="cuda")
        Td = torch.arange(8 * 32 * 3, dtype=torch.float32, device="cuda")
        for _ in range(2):                                                                 # (the first call builds the table, the second finds it)
            with pytest.raises(sa.SpartaError) as ei:
                dup.scatter_dense(Td, Dd)
            assert ei.value.code == _lib.ERR_UNSUPPORTED and "twice" in str(ei.value)
        assert untouched() and bool((Dd == 3.0).all())
        Dd.copy_(torch.arange(8 * 96, dtype=torch.float32, device="cuda").view(8, 96))
        got = dup.gather_dense(Dd).cpu().numpy()
        cols = np.arange(8 * 96, dtype=np.float32).reshape(8, 96)
        assert np.array_equal(got, np.concatenate([cols[:, :32].T.reshape(-1), cols[:, 32:64].T.reshape(-1), cols[:, :32].T.reshape(-1)]))
        # the Python layer refuses what it cannot describe, before the library is asked
        for bad in (D[:, ::2], D.view(96, 16, 10), D.to(torch.float64), D.cpu(), D[:50]):
            with pytest.raises(ValueError):
                a.gather_dense(bad)
            with pytest.raises(ValueError):
                a.scatter_dense(T[:v.nztot], bad)
        with pytest.raises(ValueError):
            a.gather_dense(D, out=T)                                                       # nztot + 4 elements
        with pytest.raises(ValueError):
            sa.dense_block_ssq(D[:, ::2], v.row_part, w)
        assert untouched()
        # empty work succeeds and launches nothing; fill on an empty pattern still fills (and keeps the padding)
        E = DenseBuf(np.full((130, 200), D_CANARY[sa.F32], np.uint32), sa.F32, True, 3, 1)
        none = torch.empty(0, device="cuda")
        assert empty.gather_dense(E.t).numel() == 0
        assert gather(empty.h, None, 200, RM, F32, None, st, None) == _lib.OK
        assert scatter(empty.h, None, None, 200, RM, F32, 0, st, None) == _lib.OK
        empty.scatter_dense(none, E.t, fill=False)
        torch.cuda.synchronize()
        assert np.all(E.read()[0] == D_CANARY[sa.F32]) and E.read()[1]
        empty.scatter_dense(none, E.t, fill=True)
        torch.cuda.synchronize()
        assert np.all(E.read()[0] == 0) and E.read()[1]
        assert score(None, 160, RM, F32, 96, 160, 0, w, None, None, st, None) == _lib.OK   # no grid block
        assert tuple(sa.dense_block_ssq(D, [0], w).shape) == (0, 5)
    finally:
        for d in (a, csr, dup, empty):
            d.close()
