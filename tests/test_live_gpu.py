"""The live-block set of a handle on the GPU: DeviceVBS.set_live_blocks / live_info / live_lists, and what sddmm and spmm_t do with it (the contract of
include/sparta_amd.h, "WITH A LIVE-BLOCK SET INSTALLED").

Handles: the geometries and masks of tests/test_live_host.py in fp32, the 16-bit edge and training geometries in f16 and bf16, all made updatable and
transposable.  The references are the handle's own unmasked kernels (live blocks: the same bits), the host rule (tests/_live.py) and, for spmm_t, the
float64 product over the live blocks with the suite's bound 1e-5 * |A|^T |X|.  Every output sits inside a canary buffer at pads 64..67."""
import contextlib

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
TOL = 1e-5
CANARY = 7654.25
TDT = {sa.F32: torch.float32, sa.F16: torch.float16, sa.BF16: torch.bfloat16}
DT_ID = {sa.F32: "f32", sa.F16: "f16", sa.BF16: "bf16"}
H16 = (sa.F16, sa.BF16)
CASES = [(k, sa.F32, br) for k, br in L.F32_CASES] + [(k, dt, None) for dt in H16 for k in U.EDGE_H16 + U.TRAIN_H16]
case_id = lambda c: "%s-%s%s" % (c[0], DT_ID[c[1]], "" if c[2] is None else "-range")  # noqa: E731
cases = pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
K_CASES = [("w48", sa.F32, None), ("heights", sa.F32, None), ("w128", sa.F16, None), ("w128", sa.BF16, None), ("w96", sa.F16, None)]

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


def values(case):
    """the range's values in the mab layout (fp32)"""
    key, _, br = case
    v = L.geometry(key)
    lo, hi = U.edge_mab_slice(v, br or (0, v.block_rows))
    return np.array(v.mab[lo:hi], f32)


def dims(case):
    key, _, br = case
    v = L.geometry(key)
    b0, b1 = br or (0, v.block_rows)
    return int(v.row_part[b1] - v.row_part[b0]), int(v.cols)


@contextlib.contextmanager
def live(d, keep, case=None):
    """the live set `keep` (numpy) on d; afterwards no live set, and the handle's own values again if `case` is given"""
    kt = torch.from_numpy(np.array(keep)).cuda()
    try:
        d.set_live_blocks(kt)
        yield kt
    finally:
        d.set_live_blocks(None)
        if case is not None and len(values(case)):
            d.set_values(torch.from_numpy(values(case)).cuda())
        torch.cuda.synchronize()


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def operand(shape, seed, dtype):
    return U.edge_round(np.random.default_rng(seed).uniform(-1, 1, shape), dtype)


def dev_in(M, ld, dtype):
    """M (r x n float64) as a column-major device operand with leading dimension ld (padding rows: 1.0)"""
    r, n = M.shape
    buf = np.ones((n, ld), f32)
    with np.errstate(all="ignore"):
        buf[:, :r] = M.T
    return torch.from_numpy(buf.reshape(-1)).to(TDT[dtype]).cuda()


class Buf:
    """a float32 output of n elements at `pad` elements into a canary buffer, prefilled with x (or the canary)"""

    def __init__(self, n, pad, x=None):
        self.n, self.pad = n, pad
        self.buf = torch.full((n + 2 * pad,), CANARY, dtype=torch.float32, device="cuda")
        self.t = self.buf[pad:pad + n]
        self.arg = self.buf[pad:]                  # what a call is handed: never an empty tensor (the rear canaries are behind the n elements)
        if x is not None and n:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(x, f32)))

    def read(self):
        torch.cuda.synchronize()
        a = self.buf.cpu().numpy()
        assert np.all(a[:self.pad] == f32(CANARY)) and np.all(a[self.pad + self.n:] == f32(CANARY)), "a canary around the output is gone"
        return a[self.pad:self.pad + self.n].copy()


def ld_variants(case):
    """(name, ldy) of the SDDMM: 16-bit handles once with ldy % 8 == 0 (the VEC path where w % 8 == 0: Y is 16-byte aligned) and once with ldy % 8 == 2"""
    _, dtype, _ = case
    cols = dims(case)[1]
    if dtype == sa.F32:
        return [("", cols + 3)]
    ld8 = (cols + 7) // 8 * 8
    return [("vec", ld8), ("novec", ld8 + 2)]


def sddmm(d, case, Xd, Yd, k, ldx, ldy, pad, G0=None):
    n = len(values(case))
    out = Buf(n, pad, G0)
    d.sddmm(Xd, Yd, out.arg, k, accumulate=G0 is not None, ldx=ldx, ldy=ldy)
    return out.read()


def prefill(case, keep, seed):
    """a previous G: seeded values; -0.0, NaN and the canary in turn in the dead blocks"""
    key, _, br = case
    n = len(values(case))
    g = np.random.default_rng(seed).uniform(-2, 2, n).astype(f32)
    dead = ~L.element_keep(L.table(key, br), keep)
    g[dead] = np.array([-0.0, np.nan, CANARY], f32)[np.arange(int(dead.sum())) % 3]
    return g, dead


def check_sddmm(d, case, k, masks, seed):
    key, dtype, br = case
    rows, cols = dims(case)
    X, Y = operand((rows, k), seed, dtype), operand((cols, k), seed + 1, dtype)
    ldx = rows + 5 + ((rows + 5) & 1 if dtype != sa.F32 else 0)          # (16-bit handles need an even ldx)
    Xd = dev_in(X, ldx, dtype)
    for vname, ldy in ld_variants(case):
        Yd = dev_in(Y, ldy, dtype)
        d.set_live_blocks(None)
        plain = sddmm(d, case, Xd, Yd, k, ldx, ldy, 64)
        for i, name in enumerate(masks):
            keep = L.mask(key, br, name)
            G0, dead = prefill(case, keep, seed + 2 + i)
            d.set_live_blocks(None)
            plain_acc = sddmm(d, case, Xd, Yd, k, ldx, ldy, 65, G0)
            with live(d, keep):
                got = sddmm(d, case, Xd, Yd, k, ldx, ldy, 64 + i % 4)
                got_acc = sddmm(d, case, Xd, Yd, k, ldx, ldy, 64 + (i + 1) % 4, G0)
            what = (case_id(case), vname, k, name)
            # accumulate = 0: live blocks as without a live set, dead blocks +0.0f in every element (the positions past cols included)
            assert np.array_equal(bits(got)[~dead], bits(plain)[~dead]), what
            assert not bits(got)[dead].any(), what
            # accumulate = 1: dead blocks neither read nor written
            assert np.array_equal(bits(got_acc)[~dead], bits(plain_acc)[~dead]), what
            assert np.array_equal(bits(got_acc)[dead], bits(G0)[dead]), what


@cases
def test_lists_and_info_follow_the_host_rule(case):
    key, _, br = case
    d, v = handle(case), L.geometry(key)
    assert d.live_info()["installed"] == 0
    for name in L.MASKS:
        keep = L.mask(key, br, name)
        if len(keep) == 0:
            continue
        want = L.rule(v, keep, br)
        with live(d, keep):
            got, info = d.live_lists(), d.live_info()
        for k, w in zip(("sd_groups", "sd_count", "t_blocks", "t_count"), want):
            assert np.array_equal(got[k], w), (case_id(case), name, k)
        assert info == {"installed": 1, "n_blocks": len(keep), "live_blocks": int(np.count_nonzero(keep)), "sd_groups": len(want[0]),
                        "live_sd_groups": int(want[1].sum()), "t_entries": len(want[2]), "live_t_entries": int(want[3].sum())}, (case_id(case), name)
    assert d.live_info()["installed"] == 0


@cases
def test_sddmm_skips_dead_blocks(case):
    check_sddmm(handle(case), case, 33, L.MASKS, 5000)


@pytest.mark.parametrize("k", [1, 31, 32, 33, 70])
@pytest.mark.parametrize("case", K_CASES, ids=[case_id(c) for c in K_CASES])
def test_sddmm_k_chunks(case, k):
    """the k loop runs 1, 2 and 3 chunks of 32, the last one partial"""
    check_sddmm(handle(case), case, k, ("second", "rand50"), 5100 + k)


@cases
def test_spmm_t_sums_live_blocks_only(case):
    key, dtype, br = case
    d, v = handle(case), L.geometry(key)
    rows, cols = dims(case)
    T = L.table(key, br)
    W = values(case)
    ldx = rows + 4 + ((rows + 4) & 1)
    ldo = cols + 1
    ops = {}
    for n in (1, 33, 128, 130):
        X = operand((rows, n), 5200 + n, dtype)
        C0 = np.random.default_rng(5300 + n).uniform(-3, 3, (cols, n)).astype(f32)
        ops[n] = (X, dev_in(X, ldx, dtype), C0)

    def run(n, acc, pad):
        X, Xd, C0 = ops[n]
        size = ldo * (n - 1) + cols
        img = None
        if acc:
            img = np.full((n, ldo), CANARY, f32)
            img[:, :cols] = C0.T
            img = img.reshape(-1)[:size]
        out = Buf(size, pad, img)
        d.spmm_t(Xd, out.arg, n, accumulate=acc, ldx=ldx, ldo=ldo)
        full = np.concatenate([out.read(), np.full(ldo * n - size, CANARY, f32)]).reshape(n, ldo)
        assert np.all(full[:, cols:] == f32(CANARY)), "the padding of ldo was written"
        return full[:, :cols].T.copy()

    for i, name in enumerate(L.MASKS):
        keep = L.mask(key, br, name)
        ek = L.element_keep(T, keep)
        Wz = np.where(ek, W, f32(0.0)).astype(f32)
        D = U.edge_dense(v, dtype, mab=Wz, br=br)
        stored = U.edge_dense(v, mab=ek.astype(f32), br=br) != 0
        try:
            # the unmasked product on the values with the dead blocks zeroed: the same MFMAs, less those whose products are exact zeros
            if len(W):
                d.set_values(torch.from_numpy(Wz).cuda())
            d.set_live_blocks(None)
            plain = {(n, acc): run(n, acc, 64) for n in ops for acc in (False, True)}
        finally:
            if len(W):
                d.set_values(torch.from_numpy(W).cuda())
        with live(d, keep):
            for n in ops:
                X, _, C0 = ops[n]
                want, clean, _, _ = U.poison_reference_t(D, stored, X)
                assert clean.all()
                bound = np.abs(D).T @ np.abs(X)
                for acc in (False, True):
                    got = run(n, acc, 64 + (i + n) % 4)
                    what = (case_id(case), name, n, acc)
                    assert np.isfinite(got).all() and np.array_equal(got, plain[(n, acc)]), what
                    base = C0.astype(np.float64) if acc else 0.0
                    assert np.all(np.abs(got - (want + base)) <= TOL * (bound + np.abs(base)) + 1e-30), what


def test_sddmm_half_alone_on_a_handle_without_transpose():
    case = ("w48", sa.F32, None)
    v = L.geometry("w48")
    d = v.to_device(0, updatable=True)
    try:
        keep = L.mask("w48", None, "rand50")
        with live(d, keep):
            got, info = d.live_lists(), d.live_info()
        want = L.rule(v, keep)
        assert np.array_equal(got["sd_groups"], want[0]) and np.array_equal(got["sd_count"], want[1]) and got["t_blocks"].size == 0 and got["t_count"].size == 0
        assert info["t_entries"] == 0 and info["live_t_entries"] == 0 and info["live_sd_groups"] == int(want[1].sum())
        check_sddmm(d, case, 33, ("rand50",), 5400)
    finally:
        d.close()


POISON_CASES = [("P32", sa.F32), ("P13", sa.F32), ("P32", sa.F16), ("P32", sa.BF16)]


@pytest.mark.parametrize("kind", list(U.POISON_VALUES))
@pytest.mark.parametrize("key,dtype", POISON_CASES, ids=["%s-%s" % (k, DT_ID[dt]) for k, dt in POISON_CASES])
def test_dead_blocks_read_nothing(key, dtype, kind):
    """spmm_t: block (r, c) dead and X's rows of block-row r poisoned -- block column c sees r only through the dead block: Ct's rows of c are those of the
    clean X, bit for bit, while a block column that r reaches through a live block turns non-finite.  sddmm: every block of block column c dead and Y's rows
    of c poisoned -- G is that of the clean Y, bit for bit, in both modes."""
    case = (key, dtype, None)
    d, v = handle(case), L.geometry(key)
    rows, cols = dims(case)
    T = L.table(key, None)
    brow, bcol = T[:, 3] >> 32, T[:, 3] & 0xffffffff
    r = 3
    c, c_live = U.poison_present(r)[0], U.poison_present(r)[1]
    n = 40
    X = operand((rows, n), 5500, dtype)
    Xp = U.poisoned(X, U.block_row_rows(v, r), kind)
    ldx = rows + 4 + (rows & 1)
    keep = np.ones(len(T), np.uint8)
    keep[(brow == r) & (bcol == c)] = 0
    with live(d, keep):
        outs = []
        for M in (X, Xp):
            out = Buf(cols * n, 66)
            d.spmm_t(dev_in(M, ldx, dtype), out.t, n, ldx=ldx)
            outs.append(out.read().reshape(n, cols).T)
    rc = U.block_col_rows(v, c)
    assert np.isfinite(outs[1][rc]).all() and np.array_equal(bits(outs[1][rc]), bits(outs[0][rc])), (key, kind)
    assert not np.isfinite(outs[1][U.block_col_rows(v, c_live)]).any()
    # sddmm
    k = 40
    Xs, Y = operand((rows, k), 5501, dtype), operand((cols, k), 5502, dtype)
    Yp = U.poisoned(Y, U.block_col_rows(v, c), kind)
    ldy = (cols + 7) // 8 * 8
    keep = (bcol != c).astype(np.uint8)
    G0, dead = prefill(case, keep, 5503)
    Xd = dev_in(Xs, ldx, dtype)
    with live(d, keep):
        res = [[sddmm(d, case, Xd, dev_in(M, ldy, dtype), k, ldx, ldy, 67, acc) for acc in (None, G0)] for M in (Y, Yp)]
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(bits(a), bits(b)), (key, kind)
    assert np.isfinite(res[1][0]).all() and not bits(res[1][0])[dead].any()


@pytest.mark.parametrize("case", [("w48", sa.F32, None), ("w128", sa.F16, None)], ids=["w48-f32", "w128-f16"])
def test_live_set_state(case):
    key, dtype, br = case
    d, v = handle(case), L.geometry(key)
    rows, cols = dims(case)
    T = L.table(key, br)
    k = 33
    X, Y = operand((rows, k), 5600, dtype), operand((cols, k), 5601, dtype)
    ldx, ldy = rows + 2, (cols + 7) // 8 * 8
    Xd, Yd = dev_in(X, ldx, dtype), dev_in(Y, ldy, dtype)
    m1, m2 = L.mask(key, br, "second"), L.mask(key, br, "rand50")
    W = torch.from_numpy(values(case)).cuda()

    def products():
        out = Buf(cols * k, 64)
        d.spmm_t(Xd, out.t, k, ldx=ldx)
        return sddmm(d, case, Xd, Yd, k, ldx, ldy, 64), out.read()

    def same(a, b):
        return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))

    d.set_live_blocks(None)
    plain = products()
    try:
        k1 = torch.from_numpy(np.array(m1)).cuda()
        d.set_live_blocks(k1)
        first = products()
        assert not same(first, plain)
        # writes to the caller's tensor change nothing until the next call
        k1.copy_(torch.from_numpy(np.array(m2)).cuda())
        torch.cuda.synchronize()
        assert same(products(), first) and np.array_equal(d.live_lists()["sd_groups"], L.rule(v, m1, br)[0])
        # set_values and a step between two products do not disturb the live set
        d.set_values(W)
        Wc, G, M, V = W.clone(), torch.zeros_like(W), torch.zeros_like(W), torch.zeros_like(W)
        d.adam_step(Wc, G, M, V, torch.zeros(8, dtype=torch.int32, device="cuda"), lr=0.0)
        assert np.array_equal(bits(Wc.cpu().numpy()), bits(W.cpu().numpy()))
        assert same(products(), first)
        # a second call replaces the first
        d.set_live_blocks(k1)
        second = products()
        got = d.live_lists()
        for name, w in zip(("sd_groups", "sd_count", "t_blocks", "t_count"), L.rule(v, m2, br)):
            assert np.array_equal(got[name], w), name
        dead = ~L.element_keep(T, m2)
        assert not bits(second[0])[dead].any() and np.array_equal(bits(second[0])[~dead], bits(plain[0])[~dead]) and not same(second, first)
        # None restores the unmasked products
        d.set_live_blocks(None)
        assert d.live_info()["installed"] == 0 and same(products(), plain)
    finally:
        d.set_live_blocks(None)
        d.set_values(W)
        torch.cuda.synchronize()


def test_live_set_under_capture():
    """the first set_live_blocks is refused under capture and leaves the capture usable; after one eager call set_live_blocks + sddmm + spmm_t replay from
    one graph and follow keep, rewritten in place between replays"""
    key = "w48"
    v = L.geometry(key)
    d = v.to_device(0, updatable=True, transposable=True)             # a fresh handle: no helper arrays yet
    try:
        T = L.table(key, None)
        rows, cols, k = v.rows, v.cols, 33
        X, Y = operand((rows, k), 5700, sa.F32), operand((cols, k), 5701, sa.F32)
        Xd, Yd = dev_in(X, rows, sa.F32), dev_in(Y, cols, sa.F32)
        m1, m2 = L.mask(key, None, "second"), L.mask(key, None, "rand90")
        keep = torch.from_numpy(np.array(m1)).cuda()
        G, Ct = Buf(int(v.nztot), 65), Buf(cols * k, 66)
        scratch = torch.zeros(4, device="cuda")
        want = {}
        for name, m in (("m1", m1), ("m2", m2)):                     # eager references from a second handle
            with live(handle((key, sa.F32, None)), m):
                a, b = Buf(int(v.nztot), 64), Buf(cols * k, 64)
                handle((key, sa.F32, None)).sddmm(Xd, Yd, a.t, k)
                handle((key, sa.F32, None)).spmm_t(Xd, b.t, k)
                want[name] = (a.read(), b.read())
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        caught = []
        with torch.cuda.stream(s):
            d.sddmm(Xd, Yd, G.t, k)                                   # (its work list is built outside the capture)
            torch.cuda.synchronize()
            g1 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g1, stream=s):
                scratch.add_(1.0)
                try:
                    d.set_live_blocks(keep)
                except sa.SpartaError as err:
                    caught.append(err)
                scratch.add_(1.0)
            torch.cuda.synchronize()
            assert len(caught) == 1 and caught[0].code == _lib.ERR_UNSUPPORTED and "captured" in str(caught[0]) and "sparta_vbs_set_live_blocks" in str(caught[0])
            g1.replay()
            torch.cuda.synchronize()
            assert float(scratch[0]) == 2.0 and d.live_info()["installed"] == 0
            d.set_live_blocks(keep)                                   # once outside a capture
            torch.cuda.synchronize()
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2, stream=s):
                d.set_live_blocks(keep)
                d.sddmm(Xd, Yd, G.t, k)
                d.spmm_t(Xd, Ct.t, k)
            torch.cuda.synchronize()
            for name, m in (("m1", m1), ("m2", m2), ("m1", m1)):
                keep.copy_(torch.from_numpy(np.array(m)).cuda())
                G.t.fill_(CANARY)
                Ct.t.fill_(CANARY)
                torch.cuda.synchronize()
                g2.replay()
                torch.cuda.synchronize()
                assert np.array_equal(bits(G.read()), bits(want[name][0])) and np.array_equal(bits(Ct.read()), bits(want[name][1])), name
                assert np.array_equal(d.live_lists()["t_blocks"], L.rule(v, m)[2])
        torch.cuda.synchronize()
    finally:
        d.close()


def test_refusals_and_argument_checks():
    m = sa.gen.uniform_random(300, 200, 3000, seed=3)
    dc = sa.DeviceVBS.from_csr(m, sa.BlockingEngine(tau=0.6, col_block_size=32).GetGrouping(m), 32, device=0)
    try:
        with pytest.raises(sa.SpartaError) as e:
            dc.live_info()
        assert e.value.code == _lib.ERR_UNSUPPORTED
    finally:
        dc.close()
    d = handle(("w48", sa.F32, None))
    n = d.n_blocks
    for bad in (torch.ones(n + 1, dtype=torch.uint8, device="cuda"), torch.ones(n, dtype=torch.int32, device="cuda"), torch.ones(n, dtype=torch.uint8),
                torch.ones(2 * n, dtype=torch.uint8, device="cuda")[::2]):
        with pytest.raises(ValueError):
            d.set_live_blocks(bad)
    with pytest.raises(ValueError):
        d.live_lists()
    d.set_live_blocks(torch.ones(n, dtype=torch.bool, device="cuda"))          # bool is taken
    assert d.live_info()["live_blocks"] == n
    d.set_live_blocks(None)


@pytest.mark.parametrize("dtype", [sa.F32, sa.F16], ids=["f32", "f16"])
def test_training_without_mask_grads(dtype):
    """w128: vbs_linear + VbsAdamW + BlockPruner for four steps, prune(0.5) after the first and prune(0.75) after the third: with skip_pruned=True and no
    mask_grads the weights, both moments and the step state equal, bit for bit, those of skip_pruned=False with mask_grads every step; grad_x agrees up to the
    sign of a zero; the pruned blocks are all-zero bits"""
    v = U.train_geometries()["w128"]
    T = v.block_table()
    W0 = np.random.default_rng(5800).uniform(-1, 1, int(v.nztot)).astype(f32)
    n = 8
    xs = [torch.from_numpy(operand((n, v.cols), 5810 + s, dtype)).to(TDT[dtype]).cuda() for s in range(4)]
    gys = [torch.from_numpy(operand((n, v.rows), 5820 + s, sa.F32)).float().cuda() for s in range(4)]

    def train(skip):
        H = v.to_device(0, dtype=dtype, updatable=True, transposable=True)
        try:
            W = torch.from_numpy(W0.copy()).cuda().requires_grad_(True)
            opt = sa.VbsAdamW([(H, W)], lr=1e-2, weight_decay=0.01)
            pruner = sa.BlockPruner(opt, skip_pruned=skip)
            trace = []
            for step in range(4):
                x = xs[step].clone().requires_grad_(True)
                opt.zero_grad()
                y = vbs_linear(x, H, W)
                y.backward(gys[step].to(y.dtype))
                if not skip:
                    pruner.mask_grads()
                opt.step()
                st = opt._state[0]
                trace.append([t.detach().cpu().numpy().copy() for t in (W, st["exp_avg"], st["exp_avg_sq"], st["state"], x.grad.float(), W.grad)])
                if step in (0, 2):
                    pruner.prune(0.5 if step == 0 else 0.75)
            return trace, pruner.keep_masks()[0].cpu().numpy(), H.live_info()["installed"]
        finally:
            H.close()

    (a, keep_a, on_a), (b, keep_b, on_b) = train(True), train(False)
    assert on_a == 1 and on_b == 0 and np.array_equal(keep_a, keep_b) and int((keep_a == 0).sum()) == int(0.75 * len(T))
    for step, (ta, tb) in enumerate(zip(a, b)):
        for name, x, y in zip(("W", "exp_avg", "exp_avg_sq", "grad_W"), ta[:3] + [ta[5]], tb[:3] + [tb[5]]):
            assert np.array_equal(bits(x), bits(y)), (step, name)
        assert np.array_equal(ta[3], tb[3]), (step, "state")
        assert np.isfinite(ta[4]).all() and np.array_equal(ta[4], tb[4]), (step, "grad_x")
    dead = ~L.element_keep(T, keep_a)
    for t in a[-1][:3]:
        assert not bits(t)[dead].any()
