"""sparta_vbs_block_ssq / sparta_vbs_mask_blocks (k_prune.hip) on the GPU, through DeviceVBS.block_ssq / mask_blocks.

Handles: every edge geometry of tests/_util.py (fp32 keys in fp32, 16-bit keys in f16 and bf16), w200 / w13h1 / w13z of train_geometries(), one geometry written
out here (blocks of 1, 2, 4 and 8 elements, two of them ragged) and a range handle of `heights`.  The reference of a score is math.fsum over the exact fp64
squares (24 x 24 bits) of the block's first n_in elements, computed once per case and value set; the bound, n_in * 2^-53 * ssq, is that of ANY order of n_in
additions of non-negative terms in fp64 (each addition a relative 2^-53 on a partial sum that never exceeds the total).  Operands sit at all four 4-byte
alignments inside canary buffers; the mask kernel is held to the bits of every element, inside and outside the tensors."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd import _lib
from sparta_amd._lib import lib

torch = pytest.importorskip("torch")

import _util as U  # noqa: E402
from test_sgd_step_gpu import CANARY  # noqa: E402
from test_set_values_gpu import tall_groups  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
_f32p = C.POINTER(C.c_float)
DT_ID = {sa.F32: "f32", sa.F16: "f16", sa.BF16: "bf16"}
PADS = (64, 65, 66, 67)                                             # floats in front of an operand: 0, 4, 8, 12 bytes past a 16-byte boundary


def _small():
    """3 x 5, w 4: heights 1 and 2, both block columns stored, the second ragged (one column): blocks of 4, 1, 8 and 2 elements inside the matrix"""
    a = U._edge_arrays(3, 5, 4, [1, 2], [[0, 1], [0, 1]])
    return U.sa_vbr(a, U._edge_values(a, "real", 7290))


def _zrows():
    """10 x 40, w 16: heights 4, 0, 6, 0 with blocks IN the block-rows of height 0 (blocks without an element: block b is still entry b of jab)"""
    a = U._edge_arrays(10, 40, 16, [4, 0, 6, 0], [[0, 2], [1, 2], [2], [0]])
    return U.sa_vbr(a, U._edge_values(a, "real", 7291))


@functools.lru_cache(maxsize=None)
def geometry(key):
    if key == "small":
        return _small()
    if key == "zrows":
        return _zrows()
    if key in U.TRAIN_F32:
        return U.train_geometries()[key]
    return U.edge_geometries("real")[key]


CASES = ([(k, sa.F32, None) for k in U.EDGE_F32] + [(k, dt, None) for dt in (sa.F16, sa.BF16) for k in U.EDGE_H16]
         + [(k, sa.F32, None) for k in ("w200", "w13h1", "w13z", "small", "zrows")] + [("heights", sa.F32, (3, 9))])
CASE_IDS = ["%s-%s%s" % (k, DT_ID[dt], "" if br is None else "-range") for k, dt, br in CASES]
cases = pytest.mark.parametrize("case", CASES, ids=CASE_IDS)

_HANDLES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for d in _HANDLES.values():
        d.close()
    _HANDLES.clear()


def handle(case):
    if case not in _HANDLES:
        key, dtype, br = case
        _HANDLES[case] = geometry(key).to_device(0, dtype=dtype, block_row_range=br, updatable=dtype != sa.F32, transposable=dtype == sa.F32 and key in ("dense", "tall"))
    return _HANDLES[case]


@functools.lru_cache(maxsize=None)
def table(case):
    key, _, br = case
    T = geometry(key).block_table(br)
    T.setflags(write=False)
    return T


@functools.lru_cache(maxsize=None)
def drawn(case, kind):
    """(values of the range in the mab layout, per block math.fsum of the exact squares of its first n_in elements); never changed.
    'real': the geometry's own values where it is an edge geometry (non-zero past cols, the zero blocks of `zeros`), seeded uniform(-1, 1) otherwise;
    'mixed': 1e-30 and 1e18 in turn with random signs -- the squares (about 1e-60 and 1e36) are exact in fp64; in fp32 the first is 0 and the second lies
    within a factor 340 of overflow"""
    key, _, br = case
    v, T = geometry(key), table(case)
    lo, hi = U.edge_mab_slice(v, br or (0, v.block_rows))
    rng = np.random.default_rng(8100 + len(key) + (hi - lo) % 977)
    if kind == "real":
        x = np.array(v.mab[lo:hi], f32) if key not in U.TRAIN_F32 else rng.uniform(-1, 1, hi - lo).astype(f32)
    else:
        x = (np.where(np.arange(hi - lo) % 2 == 0, 1e-30, 1e18) * np.where(rng.random(hi - lo) < 0.5, -1.0, 1.0)).astype(f32)
    sq = x.astype(np.float64) ** 2                                  # exact: 24 x 24 bits
    want = np.array([math.fsum(sq[o:o + n]) for o, n in zip(T[:, 0], T[:, 1])], np.float64).reshape(-1)
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


class Buf:
    """n elements at `pad` elements into a canary buffer"""

    def __init__(self, x, pad, dtype=torch.float32, n=None):
        n = len(x) if n is None else n
        self.n, self.pad = n, pad
        self.fill = 0xA5 if dtype == torch.uint8 else CANARY
        self.buf = torch.full((n + 2 * pad,), self.fill, dtype=dtype, device="cuda")
        self.t = self.buf[pad:pad + n]
        if dtype == torch.float32 and n:
            assert self.t.data_ptr() % 16 == (4 * pad) % 16
        if x is not None:
            self.t.copy_(torch.from_numpy(np.array(x)))

    def read(self):
        """(the elements, True if every canary is intact)"""
        h = self.buf.cpu().numpy()
        return h[self.pad:self.pad + self.n].copy(), bool(np.all(h[:self.pad] == self.fill) and np.all(h[self.pad + self.n:] == self.fill))


def ssq(d, x, pad, out=None):
    w = Buf(x, pad)
    out = out or Buf(None, 3, torch.float64, d.n_blocks)
    d.block_ssq(w.t, out=out.t)
    torch.cuda.synchronize()
    got, ok = out.read()
    assert ok, "a write outside ssq_out"
    assert w.read()[1]
    return got


def test_the_cases_cover_the_sizes_the_lane_scheme_turns_on():
    n_in = set()
    for c in CASES:
        n_in |= set(int(n) for n in table(c)[:, 1])
    # head only, head + tail, one 16-byte load, whole loads of every lane, the four-deep loop with a remainder; a block-row of height 0 and an empty handle
    tallest = int(table(("w200", sa.F32, None))[:, 1].max())        # w200's tallest block-row x 200 columns (the grouping makes it 268 rows)
    assert {0, 1, 2, 5, 16, 7 * 1, 257 * 32, tallest} <= n_in and tallest >= 266 * 200, sorted(n_in)
    assert table(("empty", sa.F32, None)).shape[0] == 0 and (table(("zrows", sa.F32, None))[:, 2] == 0).sum() == 3
    assert any((table(c)[:, 1] < table(c)[:, 2]).any() for c in CASES)                      # ragged blocks


# ---- 1. block_ssq ------------------------------------------------------------------------------------------------------------------------------------
@cases
def test_block_ssq_alignment_and_bound(case):
    d, T = handle(case), table(case)
    assert d.n_blocks == len(T)
    for kind in ("real", "mixed"):
        x, want = drawn(case, kind)
        for pad in PADS:
            got = ssq(d, x, pad)
            err, bound = np.abs(got - want), T[:, 1] * 2.0 ** -53 * want
            if len(T):
                worst = int(np.argmax(err - bound))
                print("%s %s pad %d: worst block %d n_in %d |diff| %.3g bound %.3g" % (CASE_IDS[CASES.index(case)], kind, pad, worst, T[worst, 1], err[worst], bound[worst]))
            assert np.all(np.isfinite(got)) and np.all(err <= bound), (kind, pad)
            assert np.all(got[T[:, 1] == 0] == 0.0) and not np.signbit(got).any()
            if kind == "real" and case[0] == "zeros":
                assert (got[0::2] == 0.0).all() and (got[1::2] > 0).all()
            if kind == "mixed":
                assert np.all((got > 1e35) | (T[:, 1] < 2))         # the 1e36 terms are there (a block of one element may hold 1e-30 alone)
                tiny = (T[:, 1] == 1) & (want < 1.0)
                assert np.all(got[tiny] == want[tiny]) and np.all(got[tiny] > 0)          # ... and 1e-60 is not flushed


@cases
def test_block_ssq_ignores_what_lies_past_cols(case):
    """the reference never reads past n_in, and the values there are non-zero already; with NaN there the scores keep their bits"""
    d, T = handle(case), table(case)
    x, _ = drawn(case, "real")
    y = x.copy()
    for o, n_in, n_all, _ in T:
        y[o + n_in:o + n_all] = np.nan
    for pad in (65, 66):
        a, b = ssq(d, x, pad), ssq(d, y, pad)
        assert np.all(np.isfinite(b)) and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    if (T[:, 1] < T[:, 2]).any():
        assert np.isnan(y).any() and (x[np.isnan(y)] != 0).all()


@pytest.mark.parametrize("case", [("heights", sa.F32, None), ("tall", sa.BF16, None), ("w200", sa.F32, None), ("heights", sa.F32, (3, 9))],
                         ids=["heights", "tall-bf16", "w200", "heights-range"])
def test_block_ssq_nonfinite_inside_marks_that_block_only(case):
    d, T = handle(case), table(case)
    x, _ = drawn(case, "real")
    live = np.flatnonzero(T[:, 1] > 0)
    hit = {int(live[0]): np.nan, int(live[len(live) // 2]): np.inf, int(live[-1]): -np.inf}
    y = x.copy()
    for k, (b, val) in enumerate(hit.items()):
        y[T[b, 0] + (0, T[b, 1] // 2, T[b, 1] - 1)[k]] = val                               # first, middle, last element inside the matrix
    a, b = ssq(d, x, 67), ssq(d, y, 67)
    bad = np.zeros(len(T), bool)
    bad[list(hit)] = True
    assert not np.isfinite(b[bad]).any() and np.isnan(b[int(live[0])]) and b[int(live[-1])] == np.inf
    assert np.array_equal(a[~bad].view(np.uint64), b[~bad].view(np.uint64))


@pytest.mark.parametrize("case", [("heights64", sa.F32, None), ("tall64", sa.F16, None), ("w200", sa.F32, None)], ids=["heights64", "tall64-f16", "w200"])
def test_block_ssq_repeats_and_replays_bit_for_bit(case):
    d, T = handle(case), table(case)
    x, _ = drawn(case, "real")
    w = Buf(x, 65)
    outs = [Buf(None, 3, torch.float64, len(T)) for _ in range(3)]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        d.block_ssq(w.t, out=outs[0].t)
        d.block_ssq(w.t, out=outs[1].t)
        torch.cuda.synchronize()
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph, stream=s):
            d.block_ssq(w.t, out=outs[2].t)
        torch.cuda.synchronize()
        assert np.all(outs[2].read()[0] == CANARY)                  # a capture runs nothing
        gph.replay()
    torch.cuda.synchronize()
    got = [o.read() for o in outs]
    assert all(ok for _, ok in got)
    assert np.array_equal(got[0][0].view(np.uint64), got[1][0].view(np.uint64)) and np.array_equal(got[0][0].view(np.uint64), got[2][0].view(np.uint64))
    out, ms = d.block_ssq(w.t, timed=True)
    assert ms >= 0.0 and np.array_equal(out.cpu().numpy().view(np.uint64), got[0][0].view(np.uint64))


# ---- 2. mask_blocks ----------------------------------------------------------------------------------------------------------------------------------
def keep_patterns(n):
    pats = {"none": np.ones(n, np.uint8), "all": np.zeros(n, np.uint8), "alternate": (np.arange(n) % 2).astype(np.uint8),
            "first": np.ones(n, np.uint8), "last": np.ones(n, np.uint8)}
    if n:
        pats["first"][0] = 0
        pats["last"][-1] = 0
    return pats


def run_mask(d, T, x, keep, n_tensors, keep_dtype=torch.uint8, keep_value=1, seed=0):
    """n_tensors canary-framed copies of x (each with its own alignment, the pruned blocks holding NaN, Inf and -1 in turn), masked in one mask_blocks call;
    asserts the bits of every element of every buffer"""
    bufs, wants = [], []
    for i in range(n_tensors):
        y = (x + f32(i)).astype(f32) if len(x) else x.copy()
        for b in np.flatnonzero(keep == 0):
            o, n_all = int(T[b, 0]), int(T[b, 2])
            y[o:o + n_all] = np.resize(np.array([np.nan, np.inf, -1.0], f32), n_all)
        want = y.copy()
        for b in np.flatnonzero(keep == 0):
            want[int(T[b, 0]):int(T[b, 0]) + int(T[b, 2])] = 0.0
        bufs.append(Buf(y, PADS[(i + seed) % 4]))
        wants.append(want)
    k = torch.from_numpy((keep * keep_value).astype(np.uint8)).cuda()
    kb = Buf(None, 5, torch.uint8, len(keep))
    kb.t.copy_(k)
    kt = kb.t if keep_dtype == torch.uint8 else (kb.t != 0)
    d.mask_blocks(kt, *[b.t for b in bufs])
    torch.cuda.synchronize()
    for i, (b, want) in enumerate(zip(bufs, wants)):
        got, ok = b.read()
        assert ok, "tensor %d: a write outside the tensor" % i
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "tensor %d" % i
    kk, ok = kb.read()
    assert ok and np.array_equal(kk, (keep * keep_value).astype(np.uint8))


@cases
def test_mask_blocks_bits(case):
    d, T = handle(case), table(case)
    x, _ = drawn(case, "real")
    full = case in (("heights", sa.F32, None), ("small", sa.F32, None), ("narrow32", sa.BF16, None))
    for q, (name, keep) in enumerate(keep_patterns(len(T)).items()):
        for n_tensors in ((1, 3, 4, 6) if full else ((1, 3, 4, 6)[q % 4],)):
            run_mask(d, T, x, keep, n_tensors, seed=q)
    with pytest.raises(ValueError):
        d.mask_blocks(torch.ones(len(T), dtype=torch.uint8, device="cuda"))                  # no tensor
    with pytest.raises(ValueError):
        d.mask_blocks(torch.ones(len(T) + 1, dtype=torch.uint8, device="cuda"), torch.zeros(len(x), device="cuda"))
    with pytest.raises(ValueError):
        d.mask_blocks(torch.ones(len(T), dtype=torch.int32, device="cuda"), torch.zeros(len(x), device="cuda"))
    with pytest.raises(ValueError):
        d.mask_blocks(torch.ones(len(T), dtype=torch.uint8, device="cuda"), torch.zeros(len(x) + 1, device="cuda"))


@pytest.mark.parametrize("case", [("heights", sa.F32, None), ("heights32", sa.F16, None), ("w13z", sa.F32, None)], ids=["heights", "heights32-f16", "w13z"])
def test_mask_blocks_keep_as_bool_and_as_other_bytes(case):
    d, T = handle(case), table(case)
    x, _ = drawn(case, "real")
    keep = keep_patterns(len(T))["alternate"]
    run_mask(d, T, x, keep, 2, keep_dtype=torch.bool)
    run_mask(d, T, x, keep, 2, keep_value=255)
    run_mask(d, T, x, keep, 3, keep_value=2)


def test_mask_blocks_first_call_under_capture_is_refused_then_replays():
    v = geometry("heights32")
    d = v.to_device(0, dtype=sa.BF16)                                # a fresh handle: no table yet
    T = v.block_table()
    x, _ = drawn(("heights32", sa.F16, None), "real")
    keep = torch.from_numpy(keep_patterns(len(T))["alternate"]).cuda()
    a, b = Buf(x, 65), Buf(x, 67)
    out = Buf(None, 3, torch.float64, len(T))
    scratch = torch.zeros(4, device="cuda")
    caught = []
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph, stream=s):
            scratch.add_(1.0)                                        # (the capture is not empty)
            for call in (lambda: d.mask_blocks(keep, a.t), lambda: d.block_ssq(a.t, out=out.t)):
                try:
                    call()
                except sa.SpartaError as err:
                    caught.append(err)
        torch.cuda.synchronize()
        assert len(caught) == 2 and all(e.code == _lib.ERR_UNSUPPORTED and "captured" in str(e) for e in caught), caught
        assert "sparta_vbs_mask_blocks" in str(caught[0]) and "sparta_vbs_block_ssq" in str(caught[1])
        d.mask_blocks(keep, b.t)                                     # once outside a capture
        torch.cuda.synchronize()
        g2, caught = torch.cuda.CUDAGraph(), []
        with torch.cuda.graph(g2, stream=s):
            d.mask_blocks(keep, a.t)
            try:
                d.mask_blocks(keep, a.t, timed=True)
            except sa.SpartaError as err:
                caught.append(err)
        torch.cuda.synchronize()
        assert len(caught) == 1 and caught[0].code == _lib.ERR_UNSUPPORTED
        assert np.array_equal(a.read()[0].view(np.uint32), x.view(np.uint32))            # a capture runs nothing
        g2.replay()
    torch.cuda.synchronize()
    (ga, oka), (gb, okb) = a.read(), b.read()
    assert oka and okb and np.array_equal(ga.view(np.uint32), gb.view(np.uint32)) and not np.array_equal(ga, x)
    assert d.mask_blocks(keep, a.t, timed=True) >= 0.0
    d.close()


def test_prune_refusals():
    t = tall_groups()
    dc = sa.DeviceVBS.from_csr(t, sa.BlockingEngine(tau=0.6, col_block_size=32).GetGrouping(t), 32, device=0)
    dt = sa.DeviceVBS.transposed_of(geometry("dense"), device=0)
    one = torch.ones(8, dtype=torch.float32, device="cuda")
    out = torch.zeros(8, dtype=torch.float64, device="cuda")
    keep = torch.ones(8, dtype=torch.uint8, device="cuda")
    fp, dp, kp = C.cast(C.c_void_p(one.data_ptr()), _f32p), C.cast(C.c_void_p(out.data_ptr()), C.POINTER(C.c_double)), C.cast(C.c_void_p(keep.data_ptr()), C.POINTER(C.c_uint8))
    n = C.c_int64(-5)
    for h in (dc, dt):
        assert lib.sparta_vbs_block_ssq(h.h, fp, dp, None, None) == _lib.ERR_UNSUPPORTED
        assert lib.sparta_vbs_mask_blocks(h.h, kp, fp, None, None, None, None, None) == _lib.ERR_UNSUPPORTED
        assert lib.sparta_vbs_block_count(h.h, C.byref(n)) == _lib.ERR_UNSUPPORTED and n.value == -5
        with pytest.raises(sa.SpartaError):
            h.n_blocks
        h.close()
    case = ("corner", sa.F32, None)
    d, T = handle(case), table(case)
    x, _ = drawn(case, "real")
    w = Buf(x, 65)
    wp = C.cast(C.c_void_p(w.t.data_ptr()), _f32p)
    assert lib.sparta_vbs_block_ssq(d.h, None, dp, None, None) == _lib.ERR_INVALID
    assert lib.sparta_vbs_block_ssq(d.h, wp, None, None, None) == _lib.ERR_INVALID
    assert lib.sparta_vbs_mask_blocks(d.h, None, wp, None, None, None, None, None) == _lib.ERR_INVALID
    assert lib.sparta_vbs_block_ssq(None, wp, dp, None, None) == _lib.ERR_INVALID
    assert lib.sparta_vbs_mask_blocks(d.h, C.cast(C.c_void_p(keep.data_ptr()), C.POINTER(C.c_uint8)), None, None, None, None, None, None) == _lib.OK   # no tensor: valid, nothing launched
    torch.cuda.synchronize()
    got, ok = w.read()
    assert ok and np.array_equal(got.view(np.uint32), x.view(np.uint32)) and (out.cpu().numpy() == 0).all()
    e = handle(("empty", sa.F32, None))                              # no block: both succeed with NULL everywhere and launch nothing
    assert e.n_blocks == 0
    assert lib.sparta_vbs_block_ssq(e.h, None, None, None, None) == _lib.OK
    assert lib.sparta_vbs_mask_blocks(e.h, None, None, None, None, None, None, None) == _lib.OK
    with pytest.raises(ValueError):
        d.block_ssq(w.t, out=torch.zeros(len(T) + 1, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        d.block_ssq(w.t.double())
