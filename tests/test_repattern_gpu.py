"""sparta_vbs_move_blocks (k_repattern.hip) and sparta_amd.repattern on the GPU.

The move: every word of every destination tensor against the numpy restatement of tests/_repattern.py, as uint32 -- NaN payloads, +-Inf, -0.0 and
denormals travel; the destinations are pre-filled with NaN and sit inside canary buffers at all four 4-byte alignments, as do the sources, which must come
back unchanged.  The products: on small-integer values (exact in every type, any order of additions) the forward product, spmm_t and sddmm of the handle
sparta_amd.repattern returns equal, bit for bit, the float64 oracle of the new pattern's dense matrix and what a handle created directly from
VBR.repattern's host arrays computes."""
import ctypes as C
import functools

import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd import _lib
from sparta_amd._lib import lib

torch = pytest.importorskip("torch")

import _util as U  # noqa: E402
import _repattern as R  # noqa: E402
from test_repattern_host import geometry as host_geometry, add_candidates, keep_mask  # noqa: E402
from test_sgd_step_gpu import CANARY  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
_f32p, _i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
DT_ID = {sa.F32: "f32", sa.F16: "f16", sa.BF16: "bf16"}
TDT = {sa.F32: torch.float32, sa.F16: torch.float16, sa.BF16: torch.bfloat16}
PADS = (64, 65, 66, 67)                                             # floats in front of an operand: 0, 4, 8, 12 bytes past a 16-byte boundary


@functools.lru_cache(maxsize=None)
def geometry(key):
    if key in ("small", "zrows"):
        return host_geometry(key)
    if key in U.TRAIN_F32 or key in U.TRAIN_H16:
        return U.train_geometries()[key]
    return U.edge_geometries("int")[key]


class Buf:
    """n float32 elements at `pad` elements into a canary buffer"""

    def __init__(self, x, pad, n=None):
        n = len(x) if n is None else n
        self.n, self.pad = n, pad
        self.buf = torch.full((n + 2 * pad,), CANARY, dtype=torch.float32, device="cuda")
        self.t = self.buf[pad:pad + n]
        if n:
            assert self.t.data_ptr() % 16 == (4 * pad) % 16
        if x is not None and n:
            self.t.view(torch.int32).copy_(torch.from_numpy(np.ascontiguousarray(x).view(np.int32)))

    def read(self):
        """(the words, True if every canary is intact)"""
        h = self.buf.cpu().numpy()
        return h[self.pad:self.pad + self.n].copy().view(np.uint32), bool(np.all(h[:self.pad] == CANARY) and np.all(h[self.pad + self.n:] == CANARY))


SPECIALS = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800001, 0x7FBFFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x00000001, 0x807FFFFF,
                     0x00400000, 0x3F800000, 0xBF800000], np.uint32)       # quiet and signalling NaNs with payloads, +-Inf, -0.0, +0.0, denormals, +-1


def special_words(n, seed):
    """n words: random bit patterns with the specials sprinkled in (every fourth word) -- most random words are ordinary floats, some are NaN"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    x[::4] = SPECIALS[rng.integers(0, len(SPECIALS), len(x[::4]))]
    return x


def run_move(dst, src, v_old, new_arrays, bmap, br, n_pairs, pad_s, pad_d, seed):
    """one move_blocks call of n_pairs pairs inside canary buffers; every word checked"""
    b0, b1 = br or (0, v_old.block_rows)
    n_old, n_new = src.info()["nztot"], dst.info()["nztot"]
    words = [special_words(n_old, seed + q) for q in range(n_pairs)]
    S = [Buf(w, pad_s) for w in words]
    D = [Buf(np.full(n_new, 0x7FC0DEAD, np.uint32), pad_d) for _ in range(n_pairs)]       # NaN everywhere: nothing of it may survive
    dst.move_blocks(src, bmap, *[(s.t, d.t) for s, d in zip(S, D)])
    torch.cuda.synchronize()
    for q in range(n_pairs):
        got, ok = D[q].read()
        assert ok, "a write outside destination %d" % q
        want = R.move_vbr(v_old, new_arrays, bmap, b0, b1, words[q])
        assert np.array_equal(got, want), (q, np.flatnonzero(got != want)[:8])
        back, ok = S[q].read()
        assert ok and np.array_equal(back, words[q]), "source %d changed" % q
    return words, D


def test_small_every_alignment_and_pair_count():
    """`small` onto its own pattern with map = [0, -1, 2, -1]: every second block kept, the two others NEW (zeros), and onto the compacted pattern"""
    v = geometry("small")
    src = v.to_device(0)
    same = v.to_device(0)
    new_v, cmap = v.repattern(keep=np.array([1, 0, 1, 0], np.uint8))
    compact = new_v.to_device(0)
    try:
        assert list(cmap) == [0, 2] and compact.n_blocks == 2
        bmap = np.array([0, -1, 2, -1], np.int32)
        for pad_s in PADS:
            for pad_d in PADS:
                for n_pairs in (1, 3, 4):
                    words, D = run_move(same, src, v, (v.nzcount, v.jab), bmap, None, n_pairs, pad_s, pad_d, 100 * pad_s + pad_d)
                    got = D[0].read()[0]
                    assert not got[4:8].any() and not got[16:24].any() and np.array_equal(got[8:16], words[0][8:16])         # +0.0, not -0.0
                    run_move(compact, src, v, (new_v.nzcount, new_v.jab), cmap, None, n_pairs, pad_s, pad_d, 7 + 100 * pad_s + pad_d)
        # five pairs: two launches
        run_move(same, src, v, (v.nzcount, v.jab), bmap, None, 5, 65, 66, 4242)
    finally:
        for d in (src, same, compact):
            d.close()


MOVE_CASES = [("zrows", sa.F32, None), ("w200", sa.F32, None), ("heights", sa.F32, (3, 9)), ("heights32", sa.F16, (3, 9)), ("heights32", sa.BF16, (3, 9)),
              ("tall64", sa.F16, None), ("empty", sa.F32, None)]


@pytest.mark.parametrize("case", MOVE_CASES, ids=["%s-%s%s" % (k, DT_ID[dt], "" if br is None else "-range") for k, dt, br in MOVE_CASES])
def test_move_on_other_geometries(case):
    """blocks without an element, blocks longer than one pass of a wave (w200: 266 x 200), a range handle, 16-bit handles; growth out of an empty handle"""
    key, dtype, br = case
    v = geometry(key)
    keep = keep_mask(v, br, "rand0")
    add = sorted(set(add_candidates(v, br).values()))
    new_v, bmap = v.repattern(keep=keep, add=add, block_row_range=br)
    assert (bmap < 0).sum() == len(add) and (len(add) > 0 or key in ("w200", "tall64"))
    src, dst = v.to_device(0, dtype=dtype, block_row_range=br), new_v.to_device(0, dtype=dtype, block_row_range=br)
    try:
        for pad_s, pad_d in ((65, 67), (66, 66)):
            run_move(dst, src, v, (new_v.nzcount, new_v.jab), bmap, br, 2, pad_s, pad_d, 31 + pad_s)
        assert dst.move_blocks(src, bmap, timed=True) >= 0.0                                # no pair: valid, nothing to move
    finally:
        src.close()
        dst.close()


def test_w200_holds_blocks_longer_than_one_pass():
    T = geometry("w200").block_table()
    assert int(T[:, 2].max()) > 4 * 256 * 4 * 8                     # the four-deep loop of 16-byte accesses turns many times


def _raw_move(dst, src, bmap, ptrs, stream=None):
    bmap = np.ascontiguousarray(bmap, np.int32)
    args = [None if p is None else C.cast(C.c_void_p(p), _f32p) for p in ptrs] + [None] * (8 - len(ptrs))
    return lib.sparta_vbs_move_blocks(dst.h, src.h, bmap.ctypes.data_as(_i32p), *args, C.c_void_p(stream), None)


def test_refusals_launch_nothing():
    v = geometry("heights")
    new_v, bmap = v.repattern(keep=keep_mask(v, None, "second"))
    src, dst = v.to_device(0), new_v.to_device(0)
    m = sa.gen.uniform_random(200, 180, 2000, seed=5)
    csr = sa.DeviceVBS.from_csr(m, sa.BlockingEngine(tau=0.5, col_block_size=16).GetGrouping(m), 16, device=0)
    try:
        n_old, n_new = src.info()["nztot"], dst.info()["nztot"]
        S = Buf(special_words(n_old, 1), 65)
        D = Buf(np.full(n_new, 0x7FC0DEAD, np.uint32), 66)
        sp, dp = S.t.data_ptr(), D.t.data_ptr()
        T_old, T_new = v.block_table(), new_v.block_table()

        def refused(rc, code=_lib.ERR_INVALID):
            torch.cuda.synchronize()
            assert rc == code, (rc, lib.sparta_last_error())
            assert np.all(D.read()[0] == 0x7FC0DEAD) and D.read()[1]

        bad = bmap.copy()
        bad[0] = src.n_blocks
        refused(_raw_move(dst, src, bad, [sp, dp]))
        bad[0] = -2
        refused(_raw_move(dst, src, bad, [sp, dp]))
        b = next(i for i in range(len(bmap)) if T_new[i, 2] > 0)
        other = next(q for q in range(len(T_old)) if T_old[q, 2] != T_new[b, 2])
        bad = bmap.copy()
        bad[b] = other
        refused(_raw_move(dst, src, bad, [sp, dp]))                                          # unequal n_all
        refused(_raw_move(dst, src, bmap, [sp, None]))                                       # half-NULL pairs
        refused(_raw_move(dst, src, bmap, [None, dp]))
        refused(_raw_move(dst, src, bmap, [sp, dp, sp, None]))
        refused(_raw_move(dst, src, bmap, [sp, dp + 2]))                                     # misaligned
        refused(_raw_move(dst, src, bmap, [sp, dp, sp, dp]))                                 # two destinations overlap
        refused(_raw_move(dst, src, bmap, [sp, dp, sp, dp + 4 * (n_new - 1)]))
        refused(_raw_move(dst, src, bmap, [dp + 4, dp]))                                     # a destination overlaps a source
        refused(_raw_move(dst, src, bmap, [sp, sp + 4 * (n_old - 1)]))
        refused(_raw_move(dst, csr, bmap, [sp, dp]), _lib.ERR_UNSUPPORTED)                   # not made from VBS arrays
        refused(_raw_move(csr, src, bmap, [sp, dp]), _lib.ERR_UNSUPPORTED)
        with pytest.raises(ValueError):
            dst.move_blocks(src, bmap[:-1], (S.t, D.t))
        # under capture
        s = torch.cuda.Stream()
        scratch = torch.zeros(8, device="cuda")
        caught = []
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            gph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gph, stream=s):
                scratch.add_(1.0)                                   # (the capture is not empty)
                try:
                    dst.move_blocks(src, bmap, (S.t, D.t))
                except sa.SpartaError as err:
                    caught.append(err)
            torch.cuda.synchronize()
        assert len(caught) == 1 and caught[0].code == _lib.ERR_UNSUPPORTED and "captured" in str(caught[0]) and "sparta_vbs_move_blocks" in str(caught[0])
        assert np.all(D.read()[0] == 0x7FC0DEAD)
        # ... and the same call outside the capture is taken
        dst.move_blocks(src, bmap, (S.t, D.t))
        torch.cuda.synchronize()
        assert np.array_equal(D.read()[0], R.move_vbr(v, (new_v.nzcount, new_v.jab), bmap, 0, v.block_rows, S.read()[0])) and D.read()[1]
    finally:
        for d in (src, dst, csr):
            d.close()


# ---- the products --------------------------------------------------------------------------------------------------------------------------------------
PRODUCT_GEOS = [("heights", sa.F32), ("dense", sa.F32), ("w13z", sa.F32), ("tall64", sa.F16), ("heights32", sa.BF16), ("w96", sa.F16)]
KEEP_CASES = ("all", "none", "rand1", "rand0+add")


def int_values(n, seed):
    return np.random.default_rng(seed).integers(-4, 5, n).astype(f32)


def dev_op(M, dtype):
    """M (r x n, float64 small integers) as a column-major device operand with an even leading dimension"""
    r, n = M.shape
    ld = r + (r & 1)
    buf = np.zeros((n, ld), f32)
    buf[:, :r] = M.T
    return torch.from_numpy(buf.reshape(-1)).to(TDT[dtype]).cuda(), ld


def products(d, v, dtype, seed):
    """(C for two widths of B, Ct, G) of handle d, whose pattern is v's, as numpy"""
    rng = np.random.default_rng(seed)
    out = {}
    for n in (64, 40):
        B = rng.integers(-4, 5, (v.cols, n)).astype(np.float64)
        Bd, ldb = dev_op(B, dtype)
        Cd = torch.full((v.rows * n,), float("nan"), dtype=torch.float32, device="cuda")
        d.spmm(Bd, Cd, n, ldb=ldb)
        out["C%d" % n] = (Cd.cpu().numpy().reshape(n, v.rows).T, B)
    k = 24
    X, Y = rng.integers(-4, 5, (v.rows, k)).astype(np.float64), rng.integers(-4, 5, (v.cols, k)).astype(np.float64)
    Xd, ldx = dev_op(X, dtype)
    Yd, ldy = dev_op(Y, dtype)
    Ct = torch.full((v.cols * k,), float("nan"), dtype=torch.float32, device="cuda")
    d.spmm_t(Xd, Ct, k, ldx=ldx)
    out["Ct"] = (Ct.cpu().numpy().reshape(k, v.cols).T, X)
    G = torch.full((max(d.info()["nztot"], 1),), float("nan"), dtype=torch.float32, device="cuda")
    d.sddmm(Xd, Yd, G, k, ldx=ldx, ldy=ldy)
    out["G"] = (G.cpu().numpy()[:d.info()["nztot"]], (X, Y))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("kcase", KEEP_CASES)
@pytest.mark.parametrize("geo", PRODUCT_GEOS, ids=["%s-%s" % (k, DT_ID[dt]) for k, dt in PRODUCT_GEOS])
def test_products_of_the_repatterned_handle(geo, kcase):
    key, dtype = geo
    g = geometry(key)
    v = sa.VBR.from_arrays(g.rows, g.cols, g.block_col_size, g.row_part, g.nzcount, g.jab, int_values(g.nztot, 600 + len(key)))
    keep = keep_mask(v, None, kcase.split("+")[0])
    add = sorted(set(add_candidates(v, None).values())) if "+add" in kcase else []
    old = v.to_device(0, dtype=dtype, updatable=True, transposable=True)
    W = torch.from_numpy(v.mab.copy()).cuda()
    M = torch.from_numpy(int_values(v.nztot, 77)).cuda()
    new_v, new_h, (W2, M2), bmap = sa.repattern(v, old, [W, M], keep=keep, add=add)
    host_v, host_map = v.repattern(keep=keep, add=add)
    fresh = host_v.to_device(0, dtype=dtype, updatable=True, transposable=True)
    try:
        assert np.array_equal(bmap, host_map) and np.array_equal(new_v.jab, host_v.jab) and not new_v.mab.any()
        assert new_h.info()["nztot"] == host_v.nztot == W2.numel() == M2.numel() and new_h.n_blocks == len(host_v.jab)
        assert new_h.updatable and new_h.transposable and new_h.dtype == dtype
        assert np.array_equal(W2.cpu().numpy().view(np.uint32), host_v.mab.view(np.uint32))
        assert np.array_equal(M2.cpu().numpy().view(np.uint32), R.move_vbr(v, (host_v.nzcount, host_v.jab), bmap, 0, v.block_rows, M.cpu().numpy()))
        assert np.array_equal(W.cpu().numpy(), v.mab) and old.info()["nztot"] == v.nztot                # the old side is as it was
        if kcase == "all":
            assert np.array_equal(host_v.mab, v.mab)
        if kcase == "none":
            assert host_v.nztot == 0 and new_h.n_blocks == 0
        D = U.edge_dense(host_v, dtype)
        got, ref = products(new_h, host_v, dtype, 900), products(fresh, host_v, dtype, 900)
        for name in ("C64", "C40", "Ct", "G"):
            a, b = got[name][0], ref[name][0]
            assert not np.isnan(a).any(), name
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, "differs from the handle created from the host arrays")
        for name in ("C64", "C40"):
            assert np.array_equal(got[name][0], (D @ got[name][1]).astype(f32)), name
        assert np.array_equal(got["Ct"][0], (D.T @ got["Ct"][1]).astype(f32))
        X, Y = got["G"][1]
        assert np.array_equal(got["G"][0], U.edge_sample(host_v, X @ Y.T).astype(f32))
    finally:
        for d in (old, new_h, fresh):
            d.close()


def test_the_fp8_switch_travels():
    g = geometry("w96")
    v = sa.VBR.from_arrays(g.rows, g.cols, g.block_col_size, g.row_part, g.nzcount, g.jab, int_values(g.nztot, 611) / 4)
    keep = keep_mask(v, None, "rand1")
    old = v.to_device(0, dtype=sa.F16, updatable=True, transposable=True)
    W = torch.from_numpy(v.mab.copy()).cuda()
    old.set_forward_a8(True, values=W)
    new_v, new_h, (W2,), bmap = sa.repattern(v, old, [W], keep=keep)
    host_v, _ = v.repattern(keep=keep)
    fresh = host_v.to_device(0, dtype=sa.F16, updatable=True, transposable=True)
    try:
        fresh.set_forward_a8(True, values=torch.from_numpy(host_v.mab.copy()).cuda())
        fi = new_h.a8_info()
        assert fi["switch"] == 1 and fi["valid"] == 1 and old.a8_info()["switch"] == 1
        rng = np.random.default_rng(5)
        n = 64
        Bd, ldb = dev_op(rng.integers(-4, 5, (v.cols, n)).astype(np.float64), sa.F16)
        out = []
        for d in (new_h, fresh):
            Cd = torch.full((v.rows * n,), float("nan"), dtype=torch.float32, device="cuda")
            d.spmm(Bd, Cd, n, ldb=ldb)
            out.append(Cd.cpu().numpy())
        assert not np.isnan(out[0]).any() and np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
        forms = new_h.a8_info()
        assert 3 in (forms["form_one_tile"], forms["form_pair"]), forms                      # the product ran on the fp8 image
    finally:
        for d in (old, new_h, fresh):
            d.close()


# ---- repattern under the fp8 switch: the new handle must qualify for the image, or the call refuses and changes nothing -----------------------------------
# Whether a 16-bit handle has the ONE stream image that holds every element depends on the pattern: two adjacent 32-row block-rows become a pair tile (the
# 64-row image) only when both store a block, and a 32-row block-row left alone gets tiles of the one-tile image -- a handle with both images has no fp8 form,
# nor has a handle without a block.  Failing cases: `pairs` (eight 32-row block-rows) with block-row 1 or block-row 0 emptied, `pairs` with nothing kept,
# `rows3` (32, 32, 32, the last block-row empty) grown by one block into the empty block-row.  Controls: the same geometries with a mask that keeps three
# blocks in every block-row, and a block added to a block-row of the pair.
from test_adam_step_host import adam_ref  # noqa: E402

A8_DT = (sa.F16, sa.BF16)
A8_CASES = [("pairs", "empty1", (), False), ("pairs", "empty0", (), False), ("pairs", "none", (), False), ("rows3", None, ((2, 1),), False),
            ("pairs", "second", (), True), ("rows3", None, ((0, 3),), True)]
a8_cases = pytest.mark.parametrize("case", A8_CASES, ids=["%s-%s" % (k, m or "grow%d" % a[0][0]) for k, m, a, _ in A8_CASES])
a8_dtypes = pytest.mark.parametrize("dtype", A8_DT, ids=[DT_ID[d] for d in A8_DT])
ADAM = dict(lr=1e-2, weight_decay=0.01)


@functools.lru_cache(maxsize=None)
def a8_geometry(key):
    if key == "pairs":
        a = U._edge_arrays(8 * 32, 8 * 32 - 11, 32, [32] * 8, [U.poison_present(ib) for ib in range(8)])
    elif key == "rows3":
        a = U._edge_arrays(96, 128, 32, [32, 32, 32], [[0, 1, 2], [1, 3], []])
    else:
        return geometry(key)
    n = int((np.diff(a[3]) * a[4]).sum()) * a[2]
    return U.sa_vbr(a, (np.random.default_rng(8800 + len(key)).integers(-8, 9, n) / 8.0).astype(f32))


def a8_keep(v, name):
    T = v.block_table()
    brow = T[:, 3] >> 32
    if name is None:
        return None
    if name in ("empty0", "empty1"):
        return (brow != int(name[-1])).astype(np.uint8)
    if name == "none":
        return np.zeros(len(T), np.uint8)
    keep = np.ones(len(T), np.uint8)
    keep[1::2] = 0
    assert name == "second" and all((keep[brow == ib] != 0).any() for ib in np.unique(brow))
    return keep


def a8_product(d, v):
    """the forward product of handle d on a seeded small-integer B of 64 columns, as uint32 words"""
    Bd, ldb = dev_op(np.random.default_rng(5).integers(-4, 5, (v.cols, 64)).astype(np.float64), d.dtype)
    Cd = torch.full((v.rows * 64,), float("nan"), dtype=torch.float32, device="cuda")
    d.spmm(Bd, Cd, 64, ldb=ldb)
    return Cd.cpu().numpy().view(np.uint32)


def a8_form(d):
    fi = d.a8_info()
    return max(fi["form_one_tile"], fi["form_pair"])


def a8_fresh_check(host_v, dtype, W2, new_h, ok, form=3):
    """a fresh handle on the new pattern says whether the pattern qualifies -- the premise of the case -- and, where it does, the repatterned handle's
    product under the switch equals its product bit for bit; form: 4 where the caller gave the new handle a live set and the a8 live switch (every block of
    it live: the same product)"""
    fresh = host_v.to_device(0, dtype=dtype, updatable=True, transposable=True)
    try:
        assert (fresh.a8_info()["capable"] > 0) == ok, (fresh.a8_info(), "the case does not test what it says")
        if ok:
            fresh.set_forward_a8(True, values=W2.detach().clone())
            fi = new_h.a8_info()
            assert fi["switch"] == 1 and fi["valid"] == 1, fi
            a, b = a8_product(new_h, host_v), a8_product(fresh, host_v)
            assert not np.isnan(a.view(f32)).any() and np.array_equal(a, b)
            assert a8_form(new_h) == form and a8_form(fresh) == 3
    finally:
        fresh.close()


def refused(err):
    assert err.value.code == _lib.ERR_UNSUPPORTED and "fp8" in str(err.value) and "repattern" in str(err.value), str(err.value)


@pytest.fixture
def created(monkeypatch):
    """every DeviceVBS made while the test runs"""
    made = []
    init = sa.DeviceVBS.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        made.append(self)

    monkeypatch.setattr(sa.DeviceVBS, "__init__", spy)
    return made


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


@a8_dtypes
@a8_cases
def test_fp8_repattern_qualifies_or_refuses(case, dtype, created):
    """sparta_amd.repattern"""
    key, kname, add, ok = case
    v = a8_geometry(key)
    keep = a8_keep(v, kname)
    old = v.to_device(0, dtype=dtype, updatable=True, transposable=True)
    W = torch.from_numpy(v.mab.copy()).cuda()
    M = torch.from_numpy(int_values(v.nztot, 78)).cuda()
    old.set_forward_a8(True, values=W)
    host_v, host_map = v.repattern(keep=keep, add=list(add))
    before = a8_product(old, v)
    del created[:]
    new_h = None
    try:
        if ok:
            new_v, new_h, (W2, M2), bmap = sa.repattern(v, old, [W, M], keep=keep, add=list(add))
            assert np.array_equal(bmap, host_map) and np.array_equal(new_v.jab, host_v.jab)
            assert np.array_equal(M2.cpu().numpy().view(np.uint32), R.move_vbr(v, (host_v.nzcount, host_v.jab), bmap, 0, v.block_rows, M.cpu().numpy()))
            a8_fresh_check(host_v, dtype, W2, new_h, True)
        else:
            with pytest.raises(sa.SpartaError) as err:
                sa.repattern(v, old, [W, M], keep=keep, add=list(add))
            refused(err)
            assert len(created) == 1 and not created[0].h, "the new handle was left open"
            free0 = free_bytes()                                                             # (the runtime's own pools are warm now: the same call once more)
            with pytest.raises(sa.SpartaError):
                sa.repattern(v, old, [W, M], keep=keep, add=list(add))
            assert free_bytes() == free0, "device memory is not back after the refusal"
            a8_fresh_check(host_v, dtype, None, None, False)
        # the old side is as it was, and still multiplies with its image
        assert np.array_equal(W.cpu().numpy(), v.mab) and old.a8_info()["switch"] == 1 and old.a8_info()["valid"] == 1
        assert np.array_equal(a8_product(old, v), before) and a8_form(old) == 3
    finally:
        for d in [old] + ([new_h] if new_h is not None else []):
            d.close()


class A8Train:
    """pairs under one VbsAdamW (and a BlockPruner with the live switches of the fp8 product), every handle with its fp8 image on, one step taken so that the
    optimizer's state exists"""

    def __init__(self, vs, dtype):
        self.vs, self.dtype = list(vs), dtype
        handles = [v.to_device(0, dtype=dtype, updatable=True, transposable=True) for v in vs]
        self.opened = list(handles)
        Ws = [torch.from_numpy(v.mab.copy()).cuda().requires_grad_(True) for v in vs]
        for h, w in zip(handles, Ws):
            h.set_forward_a8(True, values=w.detach())
        self.opt = sa.VbsAdamW(list(zip(handles, Ws)), **ADAM)
        self.pruner = sa.BlockPruner(self.opt, skip_pruned=True, live_steps=True, a8_live=True)
        self.t = 0
        self.step()

    def grads(self):
        self.t += 1
        return [(np.random.default_rng(4100 + 10 * self.t + i).integers(-8, 9, w.numel()) / 8.0).astype(f32) for i, (_, w) in enumerate(self.opt.pairs)]

    def step(self):
        """one AdamW step on seeded gradients (zero in the pruned blocks, as vbs_linear leaves them), every pair held to adam_ref bit for bit"""
        G = self.grads()
        keeps = [k.cpu().numpy() for k in self.pruner.keep_masks()]
        want = []
        for i, (h, w) in enumerate(self.opt.pairs):
            T = self.vs[i].block_table()
            for q in np.flatnonzero(keeps[i] == 0):
                G[i][T[q, 0]:T[q, 0] + T[q, 2]] = 0
            s = self.opt._state[i]
            old = (w.detach().cpu().numpy(),) + ((np.zeros(w.numel(), f32),) * 2 + (np.zeros(8, np.uint32),) if s is None else
                                                 (s["exp_avg"].cpu().numpy(), s["exp_avg_sq"].cpu().numpy(), s["state"].cpu().numpy().view(np.uint32)))
            want.append(adam_ref(old[0], G[i], old[1], old[2], old[3], ADAM))
            w.grad = torch.from_numpy(G[i]).cuda()
        self.opt.step()
        self.opt.zero_grad()
        torch.cuda.synchronize()
        for i, (h, w) in enumerate(self.opt.pairs):
            s = self.opt._state[i]
            got = (w.detach(), s["exp_avg"], s["exp_avg_sq"], s["state"])
            for name, g, r in zip("WMVS", got, want[i]):
                assert np.array_equal(g.cpu().numpy().view(np.uint32), np.asarray(r).view(np.uint32)), (i, name, "the step differs from adam_ref")
            assert h.a8_info()["valid"] == 1

    def identity(self):
        """the objects a refused call must leave in place"""
        out = [id(self.opt.pairs), id(self.pruner.pairs)]
        for (h, w), (ph, pw), s, k, p in zip(self.opt.pairs, self.pruner.pairs, self.opt._state, self.pruner._keep, self.pruner._probes):
            out += [id(h), id(w), id(ph), id(pw), id(s), id(s["exp_avg"]), id(s["exp_avg_sq"]), id(s["state"]), id(k), id(p), id(p.sel), id(p.out), h.h.value]
        return out, [k.cpu().numpy().copy() for k in self.pruner._keep], list(self.pruner._live)

    def close(self):
        for h in self.opened + [h for h, _ in self.opt.pairs]:
            h.close()


def same_identity(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1])) and a[2] == b[2]


@a8_dtypes
@a8_cases
def test_fp8_repattern_through_the_optimizer(case, dtype, created):
    """VbsAdamW.repattern"""
    key, kname, add, ok = case
    v = a8_geometry(key)
    keep = a8_keep(v, kname)
    host_v, _ = v.repattern(keep=keep, add=list(add))
    run = A8Train([v], dtype)
    try:
        ident = run.identity()
        del created[:]
        if ok:
            new_v, new_h, new_w = run.opt.repattern(0, v, keep=keep, add=list(add))
            assert run.opt.pairs[0] == (new_h, new_w) and new_w.numel() == host_v.nztot
            a8_fresh_check(host_v, dtype, new_w, new_h, True)
        else:
            with pytest.raises(sa.SpartaError) as err:
                run.opt.repattern(0, v, keep=keep, add=list(add))
            refused(err)
            assert len(created) == 1 and not created[0].h, "the new handle was left open"
            free0 = free_bytes()
            with pytest.raises(sa.SpartaError):
                run.opt.repattern(0, v, keep=keep, add=list(add))
            assert free_bytes() == free0, "device memory is not back after the refusal"
            assert same_identity(run.identity(), ident), "the refused call changed the optimizer"
            run.step()                                                                       # the old handle still trains
    finally:
        run.close()


@a8_dtypes
@a8_cases
def test_fp8_compact_and_grow_move_every_pair_or_none(case, dtype, created):
    """BlockPruner.compact / .grow on two pairs; the pair of the case is the SECOND: a refusal finds the first one already prepared"""
    key, kname, add, ok = case
    first, v = a8_geometry("rows3"), a8_geometry(key)
    keep0, keep = a8_keep(first, "second"), a8_keep(v, kname)
    run = A8Train([first, v], dtype)
    try:
        if keep is not None:
            run.pruner.load_state_dict({"keep": [torch.from_numpy(keep0), torch.from_numpy(keep)]})
            assert [h.live_info()["installed"] for h, _ in run.opt.pairs] == [1, 1]
            run.step()
        ident = run.identity()
        call = (lambda: run.pruner.compact([first, v])) if keep is not None else (lambda: run.pruner.grow(1, v, list(add)))
        del created[:]
        if ok:
            out = call()
            new_v = out[1] if keep is not None else out
            host_v, _ = v.repattern(keep=keep, add=list(add))
            assert np.array_equal(new_v.jab, host_v.jab) and run.opt.pairs[1][1].numel() == host_v.nztot
            assert len(created) == (2 if keep is not None else 1) and all(d.h for d in created)
            a8_fresh_check(host_v, dtype, run.opt.pairs[1][1], run.opt.pairs[1][0], True, form=3 if keep is not None else 4)    # (grow hands the live set on)
            run.vs = ([first.repattern(keep=keep0)[0], host_v] if keep is not None else [first, host_v])
            run.step()
        else:
            with pytest.raises(sa.SpartaError) as err:
                call()
            refused(err)
            assert len(created) == (2 if keep is not None else 1) and not any(d.h for d in created), "a new handle was left open"
            free0 = free_bytes()
            with pytest.raises(sa.SpartaError):
                call()
            assert free_bytes() == free0, "device memory is not back after the refusal"
            assert same_identity(run.identity(), ident), "the refused call changed the optimizer or the pruner: compact moves every pair or none"
            run.step()                                                                       # both old handles still train
    finally:
        run.close()
