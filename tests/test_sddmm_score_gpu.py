"""DeviceVBS.sddmm_block_ssq on the GPU (sparta_vbs_sddmm_block_ssq, the contract of include/sparta_amd.h): the fp64 block scores of X * Y^T on the stored
blocks that `sel` selects, without the gradient being written.

The reference is the handle's own two-pass form: G = sddmm(accumulate=False) without a live set, then block_ssq(G), with +0.0 where sel is 0.  The score form
runs the body of the SDDMM kernel, so the values it squares are the bits of G: on small-integer operands every square and every sum is exact in fp64 and the
two forms must agree bit for bit; on uniform operands both are sums of the same non-negative fp64 terms in different orders, each within n_in * 2^-53 of the
exact sum, which is what is asserted -- the exact sum being math.fsum (correctly rounded) over the float64 squares of the downloaded
G, so that the reference's own rounding takes no part of the bound."""
import math

import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd import _lib
from sparta_amd.autograd import vbs_linear

torch = pytest.importorskip("torch")

import _util as U  # noqa: E402
import _live as L  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
U53 = 2.0 ** -53
TDT = {sa.F32: torch.float32, sa.F16: torch.float16, sa.BF16: torch.bfloat16}
DT_ID = {sa.F32: "f32", sa.F16: "f16", sa.BF16: "bf16"}
H16 = (sa.F16, sa.BF16)
CASES = [(k, sa.F32, br) for k, br in L.F32_CASES] + [(k, dt, None) for dt in H16 for k in U.EDGE_H16]
case_id = lambda c: "%s-%s%s" % (c[0], DT_ID[c[1]], "" if c[2] is None else "-range")  # noqa: E731
cases = pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
KS = (1, 32, 33, 70)
SELS = L.MASKS + (None,)

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
        _HANDLES[case] = L.geometry(key).to_device(0, dtype=dtype, block_row_range=br, updatable=True, transposable=True)
    return _HANDLES[case]


def dims(case):
    key, _, br = case
    v = L.geometry(key)
    b0, b1 = br or (0, v.block_rows)
    return int(v.row_part[b1] - v.row_part[b0]), int(v.cols)


def nztot(case):
    key, _, br = case
    v = L.geometry(key)
    lo, hi = U.edge_mab_slice(v, br or (0, v.block_rows))
    return hi - lo


def dev_in(M, ld, dtype, lead=0):
    """M (r x n float64) as a column-major device operand with leading dimension ld (padding rows: 1.0), `lead` elements into its buffer"""
    r, n = M.shape
    buf = np.ones((n, ld), f32)
    with np.errstate(all="ignore"):
        buf[:, :r] = M.T
    t = torch.ones(lead + n * ld, dtype=TDT[dtype], device="cuda")
    t[lead:].copy_(torch.from_numpy(buf.reshape(-1)).to(TDT[dtype]))
    return t[lead:]


def even(n, dtype):
    return n + (n & 1 if dtype != sa.F32 else 0)          # (16-bit handles need even leading dimensions)


def ld_variants(case):
    """(name, ldy): 16-bit handles once with ldy % 8 == 0 (the VEC kernels where w % 8 == 0) and once with ldy % 8 == 2; fp32 with ldy > cols"""
    _, dtype, _ = case
    cols = dims(case)[1]
    if dtype == sa.F32:
        return [("", cols + 3)]
    ld8 = (cols + 7) // 8 * 8
    return [("vec", ld8), ("novec", ld8 + 2)]


def sel_of(case, name):
    key, _, br = case
    return None if name is None else np.array(L.mask(key, br, name))


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def gradient(d, case, Xd, Yd, k, ldx, ldy):
    """(G, block_ssq(G)) of the handle's own sddmm without a live set, downloaded"""
    G = torch.full((max(nztot(case), 1),), 7.5, dtype=torch.float32, device="cuda")
    d.sddmm(Xd, Yd, G, k, accumulate=False, ldx=ldx, ldy=ldy)
    ref = d.block_ssq(G[:nztot(case)])
    torch.cuda.synchronize()
    return G[:nztot(case)].cpu().numpy(), ref.cpu().numpy()


def score(d, Xd, Yd, k, ldx, ldy, sel, out=None):
    st = None if sel is None else torch.from_numpy(np.ascontiguousarray(sel, np.uint8)).cuda()
    got = d.sddmm_block_ssq(Xd, Yd, k, sel=st, out=out, ldx=ldx, ldy=ldy)
    torch.cuda.synchronize()
    assert out is None or got is out
    return got.cpu().numpy()


def operands(case, k, seed, ints):
    _, dtype, _ = case
    rows, cols = dims(case)
    rng = np.random.default_rng(seed)
    if ints:
        return rng.integers(-3, 4, (rows, k)).astype(np.float64), rng.integers(-3, 4, (cols, k)).astype(np.float64)
    return U.edge_round(rng.uniform(-1, 1, (rows, k)), dtype), U.edge_round(rng.uniform(-1, 1, (cols, k)), dtype)


@cases
def test_small_integers_bit_for_bit(case):
    """values -3 .. 3: every g is an integer below 2^10, every square and every sum exact in fp64 -- all n_blocks outputs carry the bits of block_ssq(G),
    +0.0 where sel is 0, for every mask, sel = None, and k = 1, 32, 33, 70 (one chunk, a full one, two, three)"""
    _, dtype, _ = case
    d = handle(case)
    rows, cols = dims(case)
    d.set_live_blocks(None)
    for k in KS:
        X, Y = operands(case, k, 8100 + k, True)
        ldx = even(rows + 5, dtype)
        Xd = dev_in(X, ldx, dtype)
        for vname, ldy in ld_variants(case):
            Yd = dev_in(Y, ldy, dtype)
            _, ref = gradient(d, case, Xd, Yd, k, ldx, ldy)
            assert len(ref) == d.n_blocks
            for name in SELS:
                sel = sel_of(case, name)
                want = ref.copy() if sel is None else np.where(sel != 0, ref, 0.0)
                got = score(d, Xd, Yd, k, ldx, ldy, sel)
                assert np.array_equal(u64(got), u64(want)), (case_id(case), vname, k, name)


@cases
def test_uniform_operands_within_the_summation_bound(case):
    """uniform(-1, 1): |score - ref| <= 2 n_in 2^-53 ref against block_ssq(G), and |score - exact| <= n_in 2^-53 exact against the exact sum of the float64
    squares of the downloaded G; unselected blocks are +0.0 bits"""
    key, dtype, br = case
    d = handle(case)
    rows, cols = dims(case)
    T = L.table(key, br)
    d.set_live_blocks(None)
    for k in KS:
        X, Y = operands(case, k, 8200 + k, False)
        ldx = even(rows + 5, dtype)
        Xd = dev_in(X, ldx, dtype)
        for vname, ldy in ld_variants(case):
            Yd = dev_in(Y, ldy, dtype)
            G, ref = gradient(d, case, Xd, Yd, k, ldx, ldy)
            sq = G.astype(np.float64) ** 2
            exact = np.array([math.fsum(sq[int(o):int(o) + int(n)]) for o, n in zip(T[:, 0], T[:, 1])])
            n_in = T[:, 1].astype(np.float64)
            for name in ("all", "second", "rand50", None):
                sel = sel_of(case, name)
                on = np.ones(len(T), bool) if sel is None else sel != 0
                got = score(d, Xd, Yd, k, ldx, ldy, sel)
                what = (case_id(case), vname, k, name)
                assert not u64(got)[~on].any(), what
                err_ref, err_exact = np.abs(got - ref)[on], np.abs(got - exact)[on]
                print(what, "max |score - ref| / (n_in u ref) = %.3g, max |score - exact| / (n_in u exact) = %.3g"
                      % (np.max(err_ref / np.maximum(n_in[on] * U53 * ref[on], 1e-300), initial=0.0),
                         np.max(err_exact / np.maximum(n_in[on] * U53 * exact[on], 1e-300), initial=0.0)))
                assert np.all(err_ref <= 2 * n_in[on] * U53 * ref[on]), what
                assert np.all(err_exact <= n_in[on] * U53 * exact[on]), what


@pytest.mark.parametrize("case", [("w48", sa.F32, None), ("w13z", sa.F32, None), ("heights", sa.F32, (3, 9)), ("heights32", sa.F16, None), ("tall64", sa.BF16, None)],
                         ids=["w48-f32", "w13z-f32", "heights-f32-range", "heights32-f16", "tall64-bf16"])
def test_operand_placement(case):
    """ldx > rows, ldy > cols, X and Y starting one element (fp32: 4 bytes, 16-bit: 2 bytes) and 16 bytes past a 16-byte boundary, out given and not given:
    the same bits as the tight, aligned call"""
    _, dtype, _ = case
    d = handle(case)
    rows, cols = dims(case)
    k = 33
    X, Y = operands(case, k, 8300, False)
    sel = sel_of(case, "rand50")
    base = score(d, dev_in(X, even(rows, dtype), dtype), dev_in(Y, even(cols, dtype), dtype), k, even(rows, dtype), even(cols, dtype), sel)
    esz = 4 if dtype == sa.F32 else 2
    for ldx, ldy, lead_x, lead_y in ((even(rows + 7, dtype), even(cols + 9, dtype), 0, 0), (even(rows, dtype), even(cols, dtype), 1, 1),
                                     (even(rows + 2, dtype), (cols + 7) // 8 * 8, 16 // esz, 16 // esz), (even(rows + 2, dtype), (cols + 7) // 8 * 8, 3, 1)):
        Xd, Yd = dev_in(X, ldx, dtype, lead_x), dev_in(Y, ldy, dtype, lead_y)
        for given in (False, True):
            buf = torch.full((d.n_blocks + 2,), 3.25, dtype=torch.float64, device="cuda")
            got = score(d, Xd, Yd, k, ldx, ldy, sel, out=buf[1:1 + d.n_blocks] if given else None)
            assert np.array_equal(u64(got), u64(base)), (case_id(case), ldx, ldy, lead_x, lead_y, given)
            assert float(buf[0]) == 3.25 and float(buf[-1]) == 3.25


POISON = [(k, sa.F32) for k in U.POISON_F32] + [(k, dt) for dt in H16 for k in U.POISON_H16]


@pytest.mark.parametrize("key,dtype", POISON, ids=["%s-%s" % (k, DT_ID[dt]) for k, dt in POISON])
def test_scores_depend_on_the_selected_blocks_alone(key, dtype):
    """Inf / NaN in Y's rows of a block column whose blocks are all unselected, and in X's rows of a block-row whose blocks are all unselected, shows nowhere:
    the scores are those of the clean operands, bit for bit.  With one block of that block-row selected, exactly that block's score is non-finite."""
    case = (key, dtype, None)
    d, v = handle(case), L.geometry(key)
    rows, cols = dims(case)
    T = L.table(key, None)
    brow, bcol = T[:, 3] >> 32, T[:, 3] & 0xffffffff
    k = 40
    X, Y = operands(case, k, 8400, False)
    ldx = even(rows + 4, dtype)
    for vname, ldy in ld_variants(case):
        Xd, Yd = dev_in(X, ldx, dtype), dev_in(Y, ldy, dtype)
        for kind in ("mix", "nan", "-inf"):
            for c in (1, 7):
                sel = (bcol != c).astype(np.uint8)
                clean = score(d, Xd, Yd, k, ldx, ldy, sel)
                got = score(d, Xd, dev_in(U.poisoned(Y, U.block_col_rows(v, c), kind), ldy, dtype), k, ldx, ldy, sel)
                assert np.isfinite(got).all() and np.array_equal(u64(got), u64(clean)) and not u64(got)[sel == 0].any(), (key, vname, kind, "Y", c)
            for r in (3, 6):
                Xp = dev_in(U.poisoned(X, U.block_row_rows(v, r), kind), ldx, dtype)
                sel = (brow != r).astype(np.uint8)
                clean = score(d, Xd, Yd, k, ldx, ldy, sel)
                got = score(d, Xp, Yd, k, ldx, ldy, sel)
                assert np.isfinite(got).all() and np.array_equal(u64(got), u64(clean)) and not u64(got)[sel == 0].any(), (key, vname, kind, "X", r)
                one = int(np.flatnonzero(brow == r)[2])
                sel[one] = 1
                clean = score(d, Xd, Yd, k, ldx, ldy, sel)
                got = score(d, Xp, Yd, k, ldx, ldy, sel)
                others = np.arange(len(T)) != one
                assert not np.isfinite(got[one]) and np.isfinite(clean[one]), (key, vname, kind, "X", r, one)
                assert np.isfinite(got[others]).all() and np.array_equal(u64(got)[others], u64(clean)[others]), (key, vname, kind, "X", r, one)


@pytest.mark.parametrize("case", [("w48", sa.F32, None), ("w13z", sa.F32, None), ("heights32", sa.F16, None)], ids=["w48-f32", "w13z-f32", "heights32-f16"])
def test_the_live_set_plays_no_part(case):
    """rand50 installed as the live set, then no live set, then the set that keeps nothing: the same bits for sel = the dead blocks of rand50, None and rand90;
    live_info and the G of sddmm are what they were before the calls"""
    key, dtype, br = case
    d = handle(case)
    rows, cols = dims(case)
    k = 33
    X, Y = operands(case, k, 8500, False)
    ldx, ldy = even(rows + 2, dtype), (cols + 7) // 8 * 8
    Xd, Yd = dev_in(X, ldx, dtype), dev_in(Y, ldy, dtype)
    rand50 = np.array(L.mask(key, br, "rand50"))
    sels = (1 - rand50, None, np.array(L.mask(key, br, "rand90")))

    def g_now():
        G = torch.full((nztot(case),), 7.5, dtype=torch.float32, device="cuda")
        d.sddmm(Xd, Yd, G, k, accumulate=False, ldx=ldx, ldy=ldy)
        torch.cuda.synchronize()
        return G.cpu().numpy().view(np.uint32)

    results = []
    try:
        for installed in (rand50, None, np.array(L.mask(key, br, "none"))):
            d.set_live_blocks(None if installed is None else torch.from_numpy(installed).cuda())
            info, G0 = d.live_info(), g_now()
            results.append([score(d, Xd, Yd, k, ldx, ldy, s) for s in sels])
            assert d.live_info() == info and np.array_equal(g_now(), G0), (case_id(case), installed is None)
    finally:
        d.set_live_blocks(None)
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert np.array_equal(u64(a), u64(b)), case_id(case)
    assert np.any(results[0][1] > 0)


@pytest.mark.parametrize("dtype", [sa.F32, sa.F16], ids=["f32", "f16"])
def test_repeat_and_capture(dtype):
    """a fresh handle: the first call is refused under capture (SPARTA_ERR_UNSUPPORTED) and leaves the capture usable; after one eager call ten repeats and a
    graph replay carry the same bits, and a replay after sel was rewritten in place gives the new selection's scores"""
    key = "w48" if dtype == sa.F32 else "heights32"
    case = (key, dtype, None)
    v = L.geometry(key)
    d = v.to_device(0, dtype=dtype, updatable=True, transposable=True)          # no helper arrays yet
    try:
        rows, cols, k = v.rows, v.cols, 70
        X, Y = operands(case, k, 8600, False)
        ldx, ldy = even(rows, dtype), (cols + 7) // 8 * 8
        Xd, Yd = dev_in(X, ldx, dtype), dev_in(Y, ldy, dtype)
        m1, m2 = np.array(L.mask(key, None, "second")), np.array(L.mask(key, None, "rand90"))
        sel = torch.from_numpy(m1).cuda()
        out = torch.zeros(d.n_blocks, dtype=torch.float64, device="cuda")
        scratch = torch.zeros(4, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        caught = []
        with torch.cuda.stream(s):
            g1 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g1, stream=s):
                scratch.add_(1.0)
                try:
                    d.sddmm_block_ssq(Xd, Yd, k, sel=sel, out=out, ldx=ldx, ldy=ldy)
                except sa.SpartaError as err:
                    caught.append(err)
                scratch.add_(1.0)
            torch.cuda.synchronize()
            assert len(caught) == 1 and caught[0].code == _lib.ERR_UNSUPPORTED and "captured" in str(caught[0]) and "sparta_vbs_sddmm_block_ssq" in str(caught[0])
            g1.replay()
            torch.cuda.synchronize()
            assert float(scratch[0]) == 2.0
            first = u64(score(d, Xd, Yd, k, ldx, ldy, m1))
            for _ in range(10):
                assert np.array_equal(u64(score(d, Xd, Yd, k, ldx, ldy, m1)), first)
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2, stream=s):
                d.sddmm_block_ssq(Xd, Yd, k, sel=sel, out=out, ldx=ldx, ldy=ldy)
            torch.cuda.synchronize()
            for m in (m1, m2, m1):
                sel.copy_(torch.from_numpy(m).cuda())
                out.fill_(-1.0)
                g2.replay()
                torch.cuda.synchronize()
                assert np.array_equal(u64(out.cpu().numpy()), u64(score(d, Xd, Yd, k, ldx, ldy, m)))
            assert np.array_equal(u64(score(d, Xd, Yd, k, ldx, ldy, m1)), first) and first[m1 != 0].any()
    finally:
        d.close()


def test_refusals_and_argument_checks():
    m = sa.gen.uniform_random(300, 200, 3000, seed=3)
    dc = sa.DeviceVBS.from_csr(m, sa.BlockingEngine(tau=0.6, col_block_size=32).GetGrouping(m), 32, device=0)
    try:
        with pytest.raises(sa.SpartaError) as e:
            dc.sddmm_block_ssq(torch.zeros(dc.rows * 4, device="cuda"), torch.zeros(dc.cols * 4, device="cuda"), 4)
        assert e.value.code == _lib.ERR_UNSUPPORTED
    finally:
        dc.close()
    case = ("w48", sa.F32, None)
    d = handle(case)
    rows, cols = dims(case)
    n, k = d.n_blocks, 4
    X, Y = torch.zeros(rows * k, device="cuda"), torch.zeros(cols * k, device="cuda")
    ok_sel, ok_out = torch.ones(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
    for bad in (torch.ones(n + 1, dtype=torch.uint8, device="cuda"), torch.ones(n, dtype=torch.int32, device="cuda"), torch.ones(n, dtype=torch.uint8),
                torch.ones(2 * n, dtype=torch.uint8, device="cuda")[::2]):
        with pytest.raises(ValueError):
            d.sddmm_block_ssq(X, Y, k, sel=bad)
    for bad in (torch.zeros(n + 1, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float32, device="cuda"), torch.zeros(n, dtype=torch.float64),
                torch.zeros(2 * n, dtype=torch.float64, device="cuda")[::2]):
        with pytest.raises(ValueError):
            d.sddmm_block_ssq(X, Y, k, sel=ok_sel, out=bad)
    for bx, by, kk in ((X.half(), Y, k), (X, Y.double(), k), (X[:-1], Y, k), (X, Y[:-1], k), (X.cpu(), Y, k), (X, Y, 0), (X, Y, -3)):
        with pytest.raises(ValueError):
            d.sddmm_block_ssq(bx, by, kk, sel=ok_sel, out=ok_out)
    with pytest.raises(ValueError):
        d.sddmm_block_ssq(X, Y, k, ldx=rows + 1)                      # (X too small for the stated leading dimension)
    with pytest.raises(sa.SpartaError) as e:                         # ldx < rows reaches the library
        d.sddmm_block_ssq(X, Y, k, ldx=rows - 1)
    assert e.value.code == _lib.ERR_INVALID
    got = d.sddmm_block_ssq(X, Y, k, sel=torch.ones(n, dtype=torch.bool, device="cuda"), timed=True)          # bool is taken; timed returns (out, ms)
    assert got[0].dtype == torch.float64 and got[0].numel() == n and got[1] >= 0.0 and not got[0].cpu().numpy().any()


@pytest.mark.parametrize("key,dtype", [("w48", sa.F32), ("w128", sa.F16)], ids=["w48-f32", "w128-f16"])
@pytest.mark.parametrize("form", ["plain", "epilogue"])
def test_vbs_linear_probe(key, dtype, form):
    """with a live set installed: grad_x, grad_values and grad_bias of vbs_linear(probe=...) are the bits of the call without a probe, on both Functions, and
    probe.out is what the direct call gives on the same dz and x"""
    v = U.train_geometries()[key]
    H = v.to_device(0, dtype=dtype, updatable=True, transposable=True)
    try:
        n = 8
        rng = np.random.default_rng(8700)
        W0 = rng.uniform(-1, 1, int(v.nztot)).astype(f32)
        keep = np.array(L.mask(key, None, "rand50"))
        x0 = torch.from_numpy(U.edge_round(rng.uniform(-1, 1, (n, v.cols)), dtype)).to(TDT[dtype]).cuda()
        gy = torch.from_numpy(rng.uniform(-1, 1, (n, v.rows)).astype(f32)).cuda()
        b0 = torch.from_numpy(rng.uniform(-1, 1, v.rows).astype(f32)).cuda()
        kt = torch.from_numpy(keep).cuda()
        Wm = torch.from_numpy(W0).cuda()
        H.mask_blocks(kt, Wm)
        H.set_live_blocks(kt)
        probe = sa.BlockProbe(torch.from_numpy(1 - keep).cuda(), torch.full((H.n_blocks,), -1.0, dtype=torch.float64, device="cuda"))

        def run(p):
            x, W, b = x0.clone().requires_grad_(True), Wm.clone().requires_grad_(True), b0.clone().requires_grad_(True)
            y = vbs_linear(x, H, W, probe=p) if form == "plain" else vbs_linear(x, H, W, bias=b, probe=p)
            y.backward(gy)
            torch.cuda.synchronize()
            return [t.grad.float().cpu().numpy().view(np.uint32) for t in ((x, W) if form == "plain" else (x, W, b))]

        without, with_probe = run(None), run(probe)
        for a, b in zip(without, with_probe):
            assert np.array_equal(a, b), (key, form)
        direct = H.sddmm_block_ssq(gy.to(TDT[dtype]), x0, n, sel=probe.sel)
        torch.cuda.synchronize()
        assert np.array_equal(u64(probe.out.cpu().numpy()), u64(direct.cpu().numpy())), (key, form)
        got = probe.out.cpu().numpy()
        assert not u64(got)[keep != 0].any() and np.all(got[(keep == 0) & (v.block_table()[:, 1] > 0)] > 0), (key, form)
        # values that need no gradient: backward (for x) still fills the probe
        probe.out.fill_(-1.0)
        x = x0.clone().requires_grad_(True)
        y = vbs_linear(x, H, Wm, probe=probe) if form == "plain" else vbs_linear(x, H, Wm, bias=b0, probe=probe)
        y.backward(gy)
        torch.cuda.synchronize()
        assert np.array_equal(u64(probe.out.cpu().numpy()), u64(direct.cpu().numpy())), (key, form)
    finally:
        H.close()
