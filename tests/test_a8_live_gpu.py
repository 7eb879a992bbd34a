"""The fp8 weight image with a live-block set on the GPU: DeviceVBS.set_a8_live -- the contract of include/sparta_amd.h, "THE FP8 IMAGE WITH A LIVE-BLOCK SET".

Handles: the LIVE_FORM geometries of tests/test_live_forward_gpu.py, f16 and bf16, made updatable and transposable.  Three handles per case: "d" has the fp8
switch and the new switch, "p" is a plain handle under live forward that is given the dequantised values (contract (i): bit for bit), "q" has the fp8 switch
alone, no live set, and is given values whose dead blocks are +0.0 (contract (ii): equal as numbers).  Everything is tolerance-free except the one float64
bound, which is the suite's TOL for 16-bit handles."""
import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd import _lib
from sparta_amd.autograd import vbs_linear

torch = pytest.importorskip("torch")

import _util as U  # noqa: E402
import _a8 as A8  # noqa: E402
import _live as L  # noqa: E402
from test_live_forward_gpu import LIVE_FORM, ENV, N_COLS, geometry, values, rhs, b_tensor, product, mask, install, table, H16, DT_ID, TDT  # noqa: E402,F401
from test_a8_gpu import planted, dequantised, groups_of, same_bits, gathered  # noqa: E402
from test_poison_gpu import TOL  # noqa: E402  (the suite's bound for 16-bit handles: TOL * sum|a||b|)

pytestmark = pytest.mark.gpu

f32 = np.float32
MASKS = ("all", "none", "second", "one_per_row", "row_dead", "col_dead", "rand50", "rand90")
CASES = [(k, dt) for dt in H16 for k in LIVE_FORM]
case_id = lambda c: "%s-%s" % (c[0], DT_ID[c[1]])  # noqa: E731
cases = pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
masks = pytest.mark.parametrize("name", MASKS)
TWO_IMAGES = ("tall",)
HUB_ENV = (("SPARTA_HUB_MIN_TOTAL", "1"), ("SPARTA_HUB_MIN_STEPS", "1"), ("SPARTA_HUB_G", "2"), ("SPARTA_HUB_TAU", "0.25"))

_HANDLES, _GROUPS, _W = {}, {}, {}


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ENV + ("SPARTA_SGD_FUSE", "SPARTA_ADAM_FUSE"):
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for d in _HANDLES.values():
        d.close()
    _HANDLES.clear()


def dev(a):
    """a device copy (the shared host arrays are read-only and stay as they are)"""
    return torch.from_numpy(np.array(a, f32)).cuda()


def make(key, dtype):
    return geometry(key).to_device(0, dtype=dtype, updatable=True, transposable=True)


def handle(case, which):
    """three handles per case: "d" the fp8 switch and the new one, "p" plain under live forward, "q" the fp8 switch alone"""
    if (case, which) not in _HANDLES:
        _HANDLES[(case, which)] = make(*case)
    return _HANDLES[(case, which)]


def groups(case):
    """the group number of every stored element of the case (pattern only); leaves the fp8 switch of "d" on"""
    if case not in _GROUPS:
        _GROUPS[case] = groups_of(handle(case, "d"), case[0])
    return _GROUPS[case]


def weights(case):
    """(W, the dequantised W): the planted values of tests/test_a8_gpu.py without the non-finite plants, computed once per case and left unchanged"""
    if case not in _W:
        W = planted(case[0], groups(case), case[1], False)
        Wq = dequantised(W, groups(case))
        W.setflags(write=False)
        Wq.setflags(write=False)
        _W[case] = (W, Wq)
    return _W[case]


def keep_t(keep):
    return torch.from_numpy(np.array(keep)).cuda()


def a8_form(d):
    fi = d.a8_info()
    return max(fi["form_one_tile"], fi["form_pair"])


def forms(d):
    """the form fields of both info calls must agree"""
    a, l = d.a8_info(), d.live_forward_info()
    assert (a["form_one_tile"], a["form_pair"]) == (l["form_one_tile"], l["form_pair"]), (a, l)
    return max(a["form_one_tile"], a["form_pair"])


def setup_d(d, W, keep):
    """the issue's order: a8 on (groups() did that), the values, the live set, the new switch -- enabled with a set installed"""
    d.set_a8_live(False)
    d.set_values(dev(W))
    d.set_live_blocks(keep_t(keep))
    d.set_a8_live(True)


def setup_p(p, Wq, keep):
    p.set_values(dev(Wq))
    p.set_live_blocks(keep_t(keep))
    p.set_live_forward(True)


def layouts(rows):
    """(n, row_major, C0 or None) of every product the equalities are checked on"""
    C0 = np.random.default_rng(9900).uniform(-1, 1, (rows, 256)).astype(f32)
    for n in N_COLS:
        for row_major in (False, True):
            for acc in (False, True):
                yield n, row_major, (C0[:, :n] if acc else None)


def check_equals_live_forward(d, p, case, name, W, Wq):
    key, dtype = case
    keep = mask(key, name)
    setup_d(d, W, keep)
    setup_p(p, Wq, keep)
    rows = int(geometry(key).rows)
    Bt, ldb = b_tensor(rhs(key, dtype), dtype)
    for n, rm, c0 in layouts(rows):
        x, y = product(d, key, Bt, ldb, n, rm, c0), product(p, key, Bt, ldb, n, rm, c0)
        assert same_bits(x, y), (name, n, rm, c0 is not None, np.argwhere(x.view(np.uint32) != y.view(np.uint32))[:4].tolist())
        assert forms(d) == 4 and forms(p) == 2, (d.a8_info(), p.live_forward_info())
        if name == "none":                                 # all dead: every segment keeps one dead step, C is +0.0 (or C0)
            assert same_bits(x, np.zeros_like(x) if c0 is None else np.ascontiguousarray(c0)), (n, rm)
    fi = d.a8_info()
    assert (fi["form_pair"] if LIVE_FORM[key] == 2 else fi["form_one_tile"]) == 4, fi
    li = d.a8_live_info()
    assert li["switch"] == 1 and li["active"] == 1 and li["capable"] == LIVE_FORM[key] and li["kept_steps"] == p.live_forward_info()["kept_steps"], li
    assert li["steps"] == p.live_forward_info()["steps"] and 0 < li["kept_steps"] <= li["steps"], li


@masks
@cases
def test_equals_live_forward_on_the_dequantised_values(case, name):
    """contract (i), tolerance-free: the product equals, bit for bit, the live forward product of a plain handle with the same live set that was given the
    dequantised values -- 8 / 128 / 256 columns, both layouts of C, overwriting and accumulating.  `all`: the form costs nothing in correctness when nothing
    is pruned; `none`: C is +0.0, or C0 under accumulate."""
    W, Wq = weights(case)
    check_equals_live_forward(handle(case, "d"), handle(case, "p"), case, name, W, Wq)


@masks
@cases
def test_equals_the_a8_product_on_dead_zero_values_and_float64(case, name):
    """contract (ii): equal as numbers (the sign of a zero aside) to the a8 product, no live set, on values whose dead blocks are +0.0; and within the suite's
    bound of float64 numpy on the dequantised, masked dense matrix.  The switch of "d" stays on here: set_live_blocks places the scales by itself."""
    key, dtype = case
    group = groups(case)
    d, q = handle(case, "d"), handle(case, "q")
    W, Wq = weights(case)
    keep = mask(key, name)
    ek = L.element_keep(table(key), keep)
    d.set_values(dev(W))
    d.set_a8_live(True)
    d.set_live_blocks(keep_t(keep))
    q.set_forward_a8(True, values=dev(np.where(ek, W, f32(0))))
    v = geometry(key)
    rows = int(v.rows)
    B = rhs(key, dtype)
    Bt, ldb = b_tensor(B, dtype)
    Dm = U.edge_dense(v, dtype, mab=np.where(ek, Wq, f32(0)))
    assert group.size == W.size
    for n, rm, c0 in layouts(rows):
        x, y = product(d, key, Bt, ldb, n, rm, c0), product(q, key, Bt, ldb, n, rm, c0)
        assert np.array_equal(x + f32(0), y + f32(0)), (name, n, rm, c0 is not None)
        assert forms(d) == 4 and a8_form(q) == 3
        ref, bound = Dm @ B[:, :n], np.abs(Dm) @ np.abs(B[:, :n])
        want = ref + (c0 if c0 is not None else 0)
        err = np.abs(x - want)
        assert (err <= TOL * (bound + (np.abs(c0) if c0 is not None else 0)) + 1e-30).all(), (name, n, rm, c0 is not None, float(err.max()))


def poison_choice(key, keep):
    """from block_table, on the host: P = the block columns of the dead blocks of the first block-row that has one; `free` = the rows of C of the block-rows
    that have no LIVE block in P (their elements may not see the rows of B under P), `hit` = those among them that have a dead block in P"""
    v, T = geometry(key), table(key)
    brow, bcol = T[:, 3] >> 32, T[:, 3] & 0xffffffff
    dead = np.asarray(keep) == 0
    assert dead.any(), "the mask prunes nothing"
    ib0 = int(brow[dead].min())
    P = np.unique(bcol[dead & (brow == ib0)])
    r0 = np.asarray(v.row_part, np.int64)
    free, hit = np.zeros(int(v.rows), bool), np.zeros(int(v.rows), bool)
    for ib in range(int(v.block_rows)):
        mine = brow == ib
        live_in_p = np.isin(bcol[mine & ~dead], P).any()
        dead_in_p = np.isin(bcol[mine & dead], P).any()
        free[r0[ib]:r0[ib + 1]] = not live_in_p
        hit[r0[ib]:r0[ib + 1]] = dead_in_p and not live_in_p
    return P, free, hit


@pytest.mark.parametrize("dtype", H16, ids=[DT_ID[t] for t in H16])
@pytest.mark.parametrize("key", ["pairs", "w96", "split", "short64"])
def test_dead_blocks_depend_on_nothing(key, dtype):
    """NaN, +Inf, -Inf and 3e38 in the values of dead blocks only, NaN in rows of B that only dead blocks of some block-rows read: those rows of C are finite
    and equal, bit for bit, the product with clean dead blocks and a clean B.  An Inf in a LIVE block still becomes NaN in C (e4m3fn has no Inf)."""
    case = (key, dtype)
    groups(case)
    d = handle(case, "d")
    v, T = geometry(key), table(key)
    w, cols = int(v.block_col_size), int(v.cols)
    W, _ = weights(case)
    B = rhs(key, dtype)
    Bt, ldb = b_tensor(B, dtype)
    checked = 0
    for name in ("second", "rand50"):
        keep = mask(key, name)
        P, free, hit = poison_choice(key, keep)
        if not hit.any():                                  # (never silently: the sum below must end up positive)
            continue
        ek = L.element_keep(T, keep)
        brow, bcol = T[:, 3] >> 32, T[:, 3] & 0xffffffff
        # the host-side check the choice rests on: no live block of the rows concerned lies in a poisoned block column
        r0 = np.asarray(v.row_part, np.int64)
        for ib in range(int(v.block_rows)):
            if hit[r0[ib]:r0[ib + 1]].any():
                assert not np.isin(bcol[(brow == ib) & (np.asarray(keep) != 0)], P).any()
        setup_d(d, W, keep)
        clean = {(n, rm): product(d, key, Bt, ldb, n, rm) for n in N_COLS for rm in (False, True)}
        assert forms(d) == 4 and all(np.isfinite(c).all() for c in clean.values())
        Wp = np.array(W)
        idx = np.flatnonzero(~ek)
        Wp[idx] = np.array([np.nan, np.inf, -np.inf, 3e38], f32)[np.arange(idx.size) % 4]
        Bp = B.copy()
        for jb in P:
            Bp[jb * w:min((jb + 1) * w, cols)] = np.nan
        Bpt, ldbp = b_tensor(Bp, dtype)
        d.set_values(dev(Wp))
        for (n, rm), want in clean.items():
            got = product(d, key, Bpt, ldbp, n, rm)
            assert np.isfinite(got[free]).all(), (name, n, rm, int((~np.isfinite(got[free])).sum()))
            assert same_bits(np.ascontiguousarray(got[free]), np.ascontiguousarray(want[free])), (name, n, rm)
            if not free.all():
                assert not np.isfinite(got[~free]).all(), (name, n, rm, "the poisoned rows of B do not bite")
        assert forms(d) == 4
        # with the new switch off the poison of the dead blocks shows: the inputs bite
        d.set_a8_live(False)
        got = product(d, key, Bt, ldb, 128)
        assert forms(d) == 3 and not np.isfinite(got[hit]).all(), name
        # an Inf in a live block is NaN in C
        Wi = np.array(W)
        li = int(np.flatnonzero(ek)[0])
        Wi[li] = np.inf
        d.set_a8_live(True)
        d.set_values(dev(Wi))
        got = product(d, key, Bt, ldb, 128)
        assert forms(d) == 4 and np.isnan(got).any(), name
        checked += int(hit.sum())
    assert checked > 0, "no row of B that only dead blocks read under either mask"


@pytest.mark.parametrize("case", [("pairs", sa.F16), ("w96", sa.BF16), ("short64", sa.F16), ("tiles64", sa.BF16)], ids=case_id)
def test_scales_sit_with_their_slices(case):
    """after set_live_blocks(rand50) -> set_values(W1) -> set_live_blocks(second) -> adam_step, the last word of every kept compacted record holds the biased
    exponents of the slice its a_off names (one-tile records: the one group of the slice in the low half, the high half 0, as the quantise kernel writes it),
    and those exponents are the rule applied to the current master values"""
    key, dtype = case
    group = groups(case)
    d = handle(case, "d")
    d.set_a8_live(True)
    nz = int(geometry(key).nztot)
    rng = np.random.default_rng(9910)
    d.set_live_blocks(keep_t(mask(key, "rand50")))
    Wt = dev(rng.uniform(-1, 1, nz) * np.exp2((group % 9) - 4.0))          # (magnitudes that differ from group to group: so do the exponents)
    d.set_values(Wt)
    d.set_live_blocks(keep_t(mask(key, "second")))
    G = dev(rng.uniform(-1, 1, nz))
    EA, EV = (torch.zeros(nz, device="cuda") for _ in range(2))
    S = torch.zeros(8, dtype=torch.int32, device="cuda")
    d.adam_step(Wt, G, EA, EV, S, lr=5e-2, weight_decay=0.01)
    lists = d.live_forward_lists()
    _, exps, group2 = d.a8_get()
    assert np.array_equal(group, group2)
    want_e = A8.quantize(Wt.cpu().numpy(), group)[1]
    assert np.array_equal(exps, want_e)
    pair = lists["pair"]
    tms, kp = (64 if pair else 32), (64 if int(geometry(key).block_col_size) % 64 == 0 else 32)
    ng = d.a8_info()["groups"]
    e_of = np.zeros(ng, np.int64)                          # (a group without rows has e = 0)
    e_of[group] = exps
    base = int(lists["steps"]["a_off"][0])
    assert np.array_equal(lists["steps"]["a_off"], base + np.arange(len(lists["steps"]), dtype=np.int64) * tms * kp)
    n_kept = 0
    for b, e in lists["ranges_live"]:
        for pos in range(int(b), int(e)):
            rec = lists["steps_live"][pos]
            s, rem = divmod(int(rec["a_off"]) - base, tms * kp)
            assert rem == 0 and 0 <= s < len(lists["steps"])
            want = (int(e_of[2 * s]) + 127) | ((int(e_of[2 * s + 1]) + 127) << 16) if pair else int(e_of[s]) + 127
            assert (int(rec["pad"]) & 0xffffffff) == want, (pos, s, hex(int(rec["pad"]) & 0xffffffff), hex(want))
            n_kept += 1
    assert n_kept == d.a8_live_info()["kept_steps"] > 0
    assert len(set(exps.tolist())) > 1                     # (the check can tell slices apart)


@pytest.mark.parametrize("case", [("pairs", sa.F16), ("w96", sa.BF16), ("short64", sa.F16)], ids=case_id)
def test_never_stale(case, monkeypatch):
    """after every event that moves the mask, the values or a switch, the product is that of a fresh reference pair built from the current values and mask"""
    key, dtype = case
    group = groups(case)
    d, p = handle(case, "d"), handle(case, "p")
    n = 128
    Bt, ldb = b_tensor(rhs(key, dtype), dtype)
    rng = np.random.default_rng(9920)
    nz = int(geometry(key).nztot)
    Wt = dev(np.array(values(key)))
    G = dev(rng.uniform(-1, 1, nz))
    M, EA, EV = (torch.zeros(nz, device="cuda") for _ in range(3))
    S = torch.zeros(8, dtype=torch.int32, device="cuda")
    state = {"keep": mask(key, "second")}

    def check(what, form=4):
        W = Wt.cpu().numpy()
        setup_p(p, dequantised(W, group), state["keep"])
        if form == 3:
            p.set_live_forward(False)                      # every block multiplied: the plain product of the dequantised values
        assert same_bits(product(d, key, Bt, ldb, n), product(p, key, Bt, ldb, n)), what
        assert forms(d) == form, (what, d.a8_info())
        return W

    d.set_a8_live(False)
    d.set_values(Wt)
    d.set_live_blocks(keep_t(state["keep"]))
    d.set_a8_live(True)
    last = check("start")
    # the mask changes, the values stay
    for name in ("rand50", "none", "one_per_row", "all", "rand90", "second"):
        state["keep"] = mask(key, name)
        before = d.a8_live_info()["scale_launches"]
        d.set_live_blocks(keep_t(state["keep"]))
        assert d.a8_live_info()["scale_launches"] == before + 1
        check("mask " + name)
    # the values change, the mask stays
    d.set_values(dev(rng.uniform(-3, 3, nz)))
    Wt.copy_(dev(np.array(values(key))))
    before = d.a8_live_info()["scale_launches"]
    d.set_values(Wt)
    assert d.a8_live_info()["scale_launches"] == before + 1
    last = check("set_values")
    for fuse in ("0", "1"):
        monkeypatch.setenv("SPARTA_SGD_FUSE", fuse)
        monkeypatch.setenv("SPARTA_ADAM_FUSE", fuse)
        d.sgd_step(Wt, G, M, lr=0.05, momentum=0.9)
        assert d.step_info()["fused"] == int(fuse)
        W = check("sgd_step fuse=" + fuse)
        assert not np.array_equal(W, last)
        last = W
        d.adam_step(Wt, G, EA, EV, S, lr=1e-2, weight_decay=0.01)
        assert d.step_info()["fused"] == int(fuse)
        W = check("adam_step fuse=" + fuse)
        assert not np.array_equal(W, last)
        last = W
        ctl = sa.GradCtl()
        bad = G.clone()
        bad[nz // 2] = float("inf")
        ctl.collect(bad)
        before = d.a8_live_info()["scale_launches"]
        d.adam_step(Wt, bad, EA, EV, S, lr=1e-2, ctl=ctl)
        assert ctl.read()["skip"] == 1 and d.a8_live_info()["scale_launches"] == before + 1
        W = check("skipped adam_step_ctl fuse=" + fuse)
        assert same_bits(W, last)
        d.sgd_step(Wt, bad, M, lr=0.05, momentum=0.9, ctl=ctl)
        W = check("skipped sgd_step_ctl fuse=" + fuse)
        assert same_bits(W, last)
    # the new switch off (form 3, all blocks multiplied) and on again (form 4, no write of values in between)
    d.set_a8_live(False)
    assert d.a8_live_info()["switch"] == 0 and d.a8_live_info()["active"] == 0
    check("switch off", form=3)
    state["keep"] = mask(key, "rand50")
    d.set_live_blocks(keep_t(state["keep"]))               # (a compaction with the switch off: the enabling call must place the scales again)
    check("switch off, new mask", form=3)
    d.set_a8_live(True)
    check("switch on again")
    # a8 off clears the new switch; on again, the switch, a write of values: form 4
    d.set_forward_a8(False)
    assert d.a8_live_info()["switch"] == 0 and d.a8_info()["switch"] == 0
    setup_p(p, Wt.cpu().numpy(), state["keep"])
    p.set_live_forward(False)
    assert same_bits(product(d, key, Bt, ldb, n), product(p, key, Bt, ldb, n)) and forms(d) == 1
    with pytest.raises(sa.SpartaError):
        d.set_a8_live(True)
    d.set_forward_a8(True)
    assert d.a8_live_info()["switch"] == 0
    d.set_a8_live(True)
    product(d, key, Bt, ldb, n)
    assert forms(d) == 1                                   # invalid until the next write
    d.set_values(Wt)
    check("a8 off and on")


def _refused(fn, *needles):
    with pytest.raises(sa.SpartaError) as e:
        fn()
    assert e.value.code == _lib.ERR_UNSUPPORTED, e.value
    for s in needles:
        assert s in str(e.value), (s, str(e.value))


def test_refusals(monkeypatch):
    v = geometry("zeros")
    # through the a8 requirement: fp32, not updatable, two stream images, a hub plan
    for kw in (dict(dtype=sa.F32, updatable=True, transposable=True), dict(dtype=sa.F16, transposable=True)):
        d = v.to_device(0, **kw)
        try:
            _refused(lambda: d.set_a8_live(True), "sparta_vbs_set_forward_a8")
            assert d.a8_live_info()["switch"] == 0
        finally:
            d.close()
    for key in TWO_IMAGES + ("P64",):
        if key == "P64":                                   # the hub plan, forced onto this small matrix as tests/test_poison_gpu.py forces it
            for name, val in HUB_ENV:
                monkeypatch.setenv(name, val)
        d = geometry(key).to_device(0, dtype=sa.BF16, updatable=True, transposable=True)
        try:
            assert (d.hub_info()["steps"] > 0) == (key == "P64")
            _refused(lambda: d.set_forward_a8(True), "one stream image")
            _refused(lambda: d.set_a8_live(True), "sparta_vbs_set_forward_a8")
            li = d.a8_live_info()
            assert li["switch"] == 0 and li["active"] == 0 and li["capable"] == 0, (key, li)
        finally:
            d.close()
    for name, _ in HUB_ENV:
        monkeypatch.delenv(name, raising=False)
    d = v.to_device(0, dtype=sa.F16, updatable=True, transposable=True)
    try:
        li = d.a8_live_info()
        assert li == dict(li, switch=0, active=0, capable=1, kept_steps=0, scale_launches=0)
        _refused(lambda: d.set_a8_live(True), "sparta_vbs_set_forward_a8")          # a8 off
        d.set_a8_live(False)                                                         # (switching off is host state, always accepted)
        d.set_forward_a8(True)
        scratch = torch.zeros(4, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        caught = []
        with torch.cuda.stream(s):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                scratch.add_(1.0)
                try:
                    d.set_a8_live(True)
                except sa.SpartaError as err:
                    caught.append(err)
                scratch.add_(1.0)
            torch.cuda.synchronize()
            assert len(caught) == 1 and caught[0].code == _lib.ERR_UNSUPPORTED and "captured" in str(caught[0]) and "sparta_vbs_set_a8_live" in str(caught[0])
            g.replay()
            torch.cuda.synchronize()
        assert float(scratch[0]) == 2.0 and d.a8_live_info()["switch"] == 0
        d.set_a8_live(True)
        assert d.a8_live_info()["switch"] == 1
        # live forward stays refused while a8 is on, whatever the new switch says
        _refused(lambda: d.set_live_forward(True), "sparta_vbs_set_forward_a8")
        assert d.live_forward_info()["switch"] == 0
        d.set_a8_live(False)
        _refused(lambda: d.set_live_forward(True), "sparta_vbs_set_forward_a8")
        d.set_a8_live(True)
        d.set_forward_a8(False)                                                      # clears the new switch; live forward is accepted as before
        assert d.a8_live_info()["switch"] == 0
        d.set_live_forward(True)
        _refused(lambda: d.set_forward_a8(True), "sparta_vbs_set_live_forward")
    finally:
        d.close()


def test_forms_taken(monkeypatch):
    """which kernels ran: the plain ones with an invalid image, under SPARTA_H16_PATH=lds and SPARTA_H16_AHEAD=7 and for a gathered B -- their products equal
    a plain handle's on the same values, bit for bit --; the a8 kernels on every block without a live set; the new form otherwise"""
    key, dtype = "zeros", sa.F16
    d, p = make(key, dtype), make(key, dtype)
    try:
        W = np.array(values(key))
        keep = mask(key, "second")
        Bt, ldb = b_tensor(rhs(key, dtype), dtype)
        p.set_values(dev(W))
        d.set_values(dev(W))
        d.set_forward_a8(True)
        d.set_a8_live(True)
        d.set_live_blocks(keep_t(keep))
        li = d.a8_live_info()
        assert li["switch"] == 1 and li["active"] == 0 and li["kept_steps"] > 0, li
        assert same_bits(product(d, key, Bt, ldb, 128), product(p, key, Bt, ldb, 128)) and forms(d) == 1         # a8 invalid: no write yet
        d.set_values(dev(W))
        assert d.a8_live_info()["active"] == 1
        got4 = product(d, key, Bt, ldb, 128)
        assert forms(d) == 4
        # (seven steps ahead is a choice of the launches outside the C ring: a row-major C here, the tiles of `zeros` are 24 rows tall)
        for env, rm in ((("SPARTA_H16_PATH", "lds"), False), (("SPARTA_H16_AHEAD", "7"), True)):
            monkeypatch.setenv(*env)
            assert same_bits(product(d, key, Bt, ldb, 128, rm), product(p, key, Bt, ldb, 128, rm)) and forms(d) == 1, env
            monkeypatch.delenv(env[0])
            product(d, key, Bt, ldb, 128, rm)
            assert forms(d) == 4, env
        # without a live set: the a8 kernels, every block
        d.set_live_blocks(None)
        group = d.a8_get()[2]
        p.set_values(dev(dequantised(W, group)))
        assert same_bits(product(d, key, Bt, ldb, 128), product(p, key, Bt, ldb, 128)) and forms(d) == 3
        li = d.a8_live_info()
        assert li["switch"] == 1 and li["active"] == 0 and li["kept_steps"] == 0, li
        d.set_live_blocks(keep_t(keep))
        assert same_bits(product(d, key, Bt, ldb, 128), got4) and forms(d) == 4
    finally:
        d.close()
        p.close()
    # a gathered B keeps the plain kernels (tiles64: cols = 4 x 64, two shards)
    key = "tiles64"
    v = geometry(key)
    d, p = make(key, dtype), make(key, dtype)
    try:
        W = np.array(values(key))
        d.set_forward_a8(True, values=dev(W))
        d.set_live_blocks(keep_t(mask(key, "second")))
        d.set_a8_live(True)
        p.set_values(dev(W))
        n, shard_rows = 128, int(v.cols) // 2
        Bg = gathered(rhs(key, dtype)[:, :n], shard_rows, dtype)
        out = []
        for h in (d, p):
            C = torch.full((n * int(v.rows),), float("nan"), device="cuda")
            h.spmm_gathered(Bg, shard_rows, C, n)
            torch.cuda.synchronize()
            out.append(C.cpu().numpy())
        assert same_bits(out[0], out[1]) and forms(d) == 1 and d.a8_live_info()["active"] == 1
        Bt, ldb = b_tensor(rhs(key, dtype), dtype)
        product(d, key, Bt, ldb, n)
        assert forms(d) == 4
    finally:
        d.close()
        p.close()


@masks
@pytest.mark.parametrize("key", ["split", "w96"])
def test_two_sub_workers_per_workgroup(key, name, monkeypatch):
    """the one-tile plan of 32-wide blocks with two sub-worker ranges per workgroup (SPARTA_H16_WIDE=1 at creation): the 64-column-wave kernel on the
    compacted sub-worker ranges, with 256 columns too -- contract (i) holds and the form is 4"""
    monkeypatch.setenv("SPARTA_H16_WIDE", "1")
    case = (key, sa.BF16)
    wide = ("wide",) + case
    if (wide, "d") not in _HANDLES:
        _HANDLES[(wide, "d")], _HANDLES[(wide, "p")] = make(*case), make(*case)
        _GROUPS[wide] = groups_of(_HANDLES[(wide, "d")], key)            # (the plan differs from the default one: its own group numbers and values)
        W = planted(key, _GROUPS[wide], case[1], False)
        _W[wide] = (W, dequantised(W, _GROUPS[wide]))
    d, p = _HANDLES[(wide, "d")], _HANDLES[(wide, "p")]
    assert d.live_forward_info()["capable"] == 1
    check_equals_live_forward(d, p, case, name, *_W[wide])
    assert d.live_forward_info()["ranges"] == 2 * d.info()["stream_workers"]
    assert d.a8_info()["form_one_tile"] == 4


@pytest.mark.parametrize("key", ["zeros", "pairs"])
def test_capture(key):
    """set_live_blocks + set_values + product in one graph: a replay follows keep and W rewritten in place and equals the eager product of a fresh handle set
    up with those; the capture holds two scale placements and no first-call allocation"""
    dtype = sa.F16
    v = geometry(key)
    d, e = make(key, dtype), make(key, dtype)
    try:
        rows, n, nz = int(v.rows), 128, int(v.nztot)
        Bt, ldb = b_tensor(rhs(key, dtype), dtype)
        rng = np.random.default_rng(9930)
        rounds = [(mask(key, m), rng.uniform(-s, s, nz).astype(f32)) for m, s in (("second", 1), ("rand90", 4), ("none", 1), ("one_per_row", 0.01), ("all", 2))]
        keep = keep_t(rounds[0][0])
        Wt = dev(rounds[0][1])
        C = torch.zeros(n * rows, device="cuda")
        s = torch.cuda.Stream()
        for h in (d, e):
            h.set_forward_a8(True)
            h.set_a8_live(True)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            d.set_live_blocks(keep)                              # the eager round: helper arrays
            d.set_values(Wt)
            d.spmm(Bt, C, n, ldb=ldb, ldc=rows)
            torch.cuda.synchronize()
            before = d.a8_live_info()["scale_launches"]
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                d.set_live_blocks(keep)
                d.set_values(Wt)
                d.spmm(Bt, C, n, ldb=ldb, ldc=rows)
            torch.cuda.synchronize()
            assert d.a8_live_info()["scale_launches"] == before + 2
            for m, W in rounds[1:] + rounds[:1]:
                keep.copy_(keep_t(m))
                Wt.copy_(dev(W))
                C.fill_(7.0)
                torch.cuda.synchronize()
                g.replay()
                torch.cuda.synchronize()
                got = C.cpu().numpy().reshape(n, rows).T
                e.set_live_blocks(keep_t(m))
                e.set_values(dev(W))
                want = product(e, key, Bt, ldb, n)
                assert same_bits(np.ascontiguousarray(got), want), int(np.count_nonzero(m))
                assert d.live_info()["live_blocks"] == int(np.count_nonzero(m))
        assert forms(d) == 4 and forms(e) == 4
    finally:
        d.close()
        e.close()


@pytest.mark.parametrize("dtype", H16, ids=[DT_ID[t] for t in H16])
@pytest.mark.parametrize("key", ["w128", "w96"])          # (pair / 64-row tiles; one-tile records with split tiles; vbs_linear wants even rows and cols)
def test_through_the_layer(key, dtype):
    """three steps of vbs_linear + VbsAdamW with the fp8 switch on under BlockPruner(skip_pruned=True, a8_live=True), pruned to 50 % before the first step and
    to 75 % after the second, against the same run with a8_live=False (the pruner keeps the dead blocks at zero): losses, W and both moments equal as numbers;
    the forward form is 4 in the first run and 3 in the second"""
    v = geometry(key)
    W0 = np.random.default_rng(9940).uniform(-1, 1, int(v.nztot)).astype(f32)
    n = 8
    rnd = lambda shape, seed, dt: U.edge_round(np.random.default_rng(seed).uniform(-1, 1, shape), dt)  # noqa: E731
    xs = [torch.from_numpy(rnd((n, v.cols), 9950 + s, dtype)).to(TDT[dtype]).cuda() for s in range(3)]
    gys = [torch.from_numpy(rnd((n, v.rows), 9960 + s, sa.F32)).float().cuda() for s in range(3)]

    def train(a8_live):
        H = make(key, dtype)
        try:
            W = torch.from_numpy(W0.copy()).cuda().requires_grad_(True)
            opt = sa.VbsAdamW([(H, W)], lr=1e-2, weight_decay=0.01)
            H.set_forward_a8(True)
            pruner = sa.BlockPruner(opt, skip_pruned=True, a8_live=a8_live)
            pruner.prune(0.5)
            trace, seen, losses = [], [], []
            for step in range(3):
                x = xs[step].clone().requires_grad_(True)
                opt.zero_grad()
                y = vbs_linear(x, H, W)
                seen.append(forms(H))
                loss = (y.float() * gys[step]).sum()
                losses.append(loss.detach().cpu().numpy() + f32(0))
                loss.backward()
                opt.step()
                st = opt._state[0]
                trace.append([t.detach().cpu().numpy() + f32(0) for t in (W, st["exp_avg"], st["exp_avg_sq"])])
                if step == 1:
                    pruner.prune(0.75)
            return trace, seen, losses, H.a8_live_info()
        finally:
            H.close()

    (a, fa, la, ia), (b, fb, lb, ib) = train(True), train(False)
    assert fa == [4, 4, 4] and fb == [3, 3, 3] and ia["switch"] == 1 and ib["switch"] == 0, (fa, fb, ia, ib)
    for step, (ta, tb) in enumerate(zip(a, b)):
        assert np.array_equal(la[step], lb[step]), (step, la[step], lb[step])
        for what, x, y in zip(("W", "exp_avg", "exp_avg_sq"), ta, tb):
            assert np.array_equal(x, y), (step, what)
