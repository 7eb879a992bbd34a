"""The fp8 weight image on the GPU: DeviceVBS.set_forward_a8 -- the contract of include/sparta_amd.h, "THE FP8 WEIGHT IMAGE".

Handles: the geometries of tests/test_live_forward_gpu.py whose 16-bit handle has one stream image (its LIVE_FORM set: one-tile records with and without the
C ring, 64-column tiles, split tiles, pair tiles with absent halves over a ragged last block column, short tiles of 64-deep steps), f16 and bf16, made
updatable and transposable.  References: the numpy restatement of the rule (tests/_a8.py), applied group by group with the group numbers the handle
returns; a second handle of the same geometry that never gets the switch and is given the dequantised values -- the two products must agree bit for bit
(same kernel body, same MFMA order); and float64 numpy within the suite's bound for 16-bit handles."""
import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd import _lib
from sparta_amd.autograd import vbs_linear

torch = pytest.importorskip("torch")

import _util as U  # noqa: E402
import _a8 as A8  # noqa: E402
from test_live_forward_gpu import LIVE_FORM, ENV, H16, DT_ID, TDT, N_COLS, geometry, values, rhs, b_tensor, product, dev  # noqa: E402
from test_poison_gpu import TOL  # noqa: E402  (the suite's bound for 16-bit handles: TOL * sum|a||b|)

pytestmark = pytest.mark.gpu

f32 = np.float32
CASES = [(k, dt) for dt in H16 for k in LIVE_FORM]
case_id = lambda c: "%s-%s" % (c[0], DT_ID[c[1]])  # noqa: E731
cases = pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
TWO_IMAGES = ("tall", "heights32", "w256", "P32")

_HANDLES = {}


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


def handle(case, which):
    """two handles per case: "a8" gets the switch, "ref" never does"""
    if (case, which) not in _HANDLES:
        key, dtype = case
        _HANDLES[(case, which)] = geometry(key).to_device(0, dtype=dtype, updatable=True, transposable=True)
    return _HANDLES[(case, which)]


def groups_of(d, key):
    """the group number of every stored element (pattern only), checked once per call: every element has one, no group holds more than 32 x KP elements"""
    d.set_forward_a8(True, values=dev(np.array(values(key))))
    _, _, group = d.a8_get()
    fi = d.a8_info()
    assert group.min() >= 0 and group.max() < fi["groups"], (group.min(), group.max(), fi)
    kp = 64 if int(geometry(key).block_col_size) % 64 == 0 else 32
    assert np.bincount(group).max() <= 32 * kp
    return group


def planted(key, group, dtype, non_finite):
    """uniform(-1, 1) without a zero, plus groups planted where the rule can go wrong: all zero, one 3e4 element, -0.0 elements, (bf16) one at e ~ -100, and with
    non_finite one NaN and one Inf element.  Everything else stays inside the ranges in which the dequantised value is exact in the handle's type."""
    W = np.array(values(key))
    ids = np.unique(group)
    pick = [int(ids[(i * len(ids)) // 7]) for i in range(7)]          # (small handles: some of these coincide, later plants override earlier ones)
    first = lambda g: int(np.flatnonzero(group == g)[0])  # noqa: E731
    W[group == pick[0]] = 0.0
    W[first(pick[1])] = 3e4
    W[np.flatnonzero(group == pick[2])[::3]] = -0.0
    if dtype == sa.BF16:
        W[group == pick[3]] *= f32(2.0 ** -92)
    if non_finite:
        W[first(pick[4])] = np.nan
        W[np.flatnonzero(group == pick[5])[-1]] = -np.inf
        W[np.flatnonzero(group == pick[6])[-1]] = np.inf
    return W


def dequantised(W, group):
    codes, e = A8.quantize(W, group)
    Wq = A8.dequantize(codes, e)
    with np.errstate(all="ignore"):
        assert np.array_equal(Wq.astype(f32).astype(np.float64), Wq, equal_nan=True)
    return Wq.astype(f32)


def same_bits(x, y):
    return np.array_equal(x.view(np.uint32), y.view(np.uint32))


def form_of(d):
    fi = d.a8_info()
    return max(fi["form_one_tile"], fi["form_pair"]), fi


@cases
def test_image(case):
    """codes and exponents of the device image equal the restatement applied group by group, bit for bit"""
    key, dtype = case
    d = handle(case, "a8")
    group = groups_of(d, key)
    W = planted(key, group, dtype, True)
    before = d.a8_info()["quantize_launches"]
    d.set_values(dev(W))
    codes, exps, group2 = d.a8_get()
    fi = d.a8_info()
    assert np.array_equal(group, group2) and fi["quantize_launches"] == before + 1 and fi["valid"] == 1 and fi["switch"] == 1
    assert fi["capable"] == LIVE_FORM[key] and fi["image_bytes"] >= W.size, fi
    want_codes, want_e = A8.quantize(W, group)
    assert np.array_equal(exps, want_e), np.flatnonzero(exps != want_e)[:8]
    assert np.array_equal(codes, want_codes), (np.flatnonzero(codes != want_codes)[:8], codes[codes != want_codes][:8], want_codes[codes != want_codes][:8])
    # a second write of the same values gives the same bits
    d.set_values(dev(W))
    c2, e2, _ = d.a8_get()
    assert np.array_equal(c2, codes) and np.array_equal(e2, exps)


@cases
def test_product_equals_a_plain_handle_on_the_dequantised_values(case):
    """tolerance-free: the a8 product of W equals, bit for bit, the 16-bit product of a handle given the dequantised values -- 8 / 128 / 256 columns, both
    layouts of C, overwriting and accumulating -- and both lie within the suite's bound of float64 numpy on those values"""
    key, dtype = case
    d, p = handle(case, "a8"), handle(case, "ref")
    group = groups_of(d, key)
    W = planted(key, group, dtype, False)
    Wq = dequantised(W, group)
    if dtype == sa.F16:
        e = A8.quantize(W, group)[1]
        assert e.min() >= -15 and e.max() <= 7
    d.set_values(dev(W))
    p.set_values(dev(Wq))
    v = geometry(key)
    rows = int(v.rows)
    B = rhs(key, dtype)
    Bt, ldb = b_tensor(B, dtype)
    C0 = np.random.default_rng(9400).uniform(-1, 1, (rows, 256)).astype(f32)
    D = U.edge_dense(v, dtype, mab=Wq)
    for n in N_COLS:
        ref, bound = D @ B[:, :n], np.abs(D) @ np.abs(B[:, :n])
        for row_major in (False, True):
            for acc in (False, True):
                c0 = C0[:, :n] if acc else None
                x, y = product(d, key, Bt, ldb, n, row_major, c0), product(p, key, Bt, ldb, n, row_major, c0)
                assert same_bits(x, y), (n, row_major, acc, np.argwhere(x.view(np.uint32) != y.view(np.uint32))[:4].tolist())
                assert form_of(d)[0] == 3 and max(p.a8_info()["form_one_tile"], p.a8_info()["form_pair"]) == 1
                want = ref + (c0 if acc else 0)
                assert (np.abs(x - want) <= TOL * (bound + (np.abs(c0) if acc else 0)) + 1e-30).all(), (n, row_major, acc, float(np.abs(x - want).max()))
    fi = d.a8_info()
    assert (fi["form_pair"] if LIVE_FORM[key] == 2 else fi["form_one_tile"]) == 3, fi


@pytest.mark.parametrize("key", ["split", "w96"])
def test_two_sub_workers_per_workgroup(key, monkeypatch):
    """the one-tile plan of 32-wide blocks with two sub-worker ranges per workgroup (SPARTA_H16_WIDE=1 at creation): the a8 64-column-wave kernel"""
    monkeypatch.setenv("SPARTA_H16_WIDE", "1")
    dtype = sa.BF16
    d, p = (geometry(key).to_device(0, dtype=dtype, updatable=True, transposable=True) for _ in range(2))
    try:
        assert d.live_forward_info()["capable"] == 1
        group = groups_of(d, key)
        W = planted(key, group, dtype, False)
        d.set_values(dev(W))
        p.set_values(dev(dequantised(W, group)))
        codes, exps, _ = d.a8_get()
        want_codes, want_e = A8.quantize(W, group)
        assert np.array_equal(codes, want_codes) and np.array_equal(exps, want_e)
        Bt, ldb = b_tensor(rhs(key, dtype), dtype)
        for n in N_COLS:
            for rm in (False, True):
                assert same_bits(product(d, key, Bt, ldb, n, rm), product(p, key, Bt, ldb, n, rm)), (n, rm)
                assert d.a8_info()["form_one_tile"] == 3
    finally:
        d.close()
        p.close()


def gathered(B, shard_rows, dtype):
    """B (cols x n) as an all-gather result: cols / shard_rows column-major slabs back to back"""
    cols, n = B.shape
    buf = np.concatenate([np.ascontiguousarray(B[s * shard_rows:(s + 1) * shard_rows].T, f32).reshape(-1) for s in range(cols // shard_rows)])
    return torch.from_numpy(buf).to(TDT[dtype]).cuda()


def test_forms_taken(monkeypatch):
    """a8_info says which kernels ran: plain before the first write of values, a8 after it, plain under SPARTA_H16_AHEAD=7, SPARTA_H16_PATH=lds and a gathered
    B, plain with the switch off -- and with the switch off the product is that of a handle that never had it"""
    key, dtype = "zeros", sa.F16
    v = geometry(key)
    d, p = (v.to_device(0, dtype=dtype, updatable=True, transposable=True) for _ in range(2))
    try:
        W = np.array(values(key))
        Bt, ldb = b_tensor(rhs(key, dtype), dtype)
        d.set_values(dev(W))
        p.set_values(dev(W))
        plain = product(p, key, Bt, ldb, 128)
        assert d.a8_info() == dict(d.a8_info(), switch=0, valid=0, capable=1, quantize_launches=0, image_bytes=0)
        d.set_forward_a8(True)
        assert same_bits(product(d, key, Bt, ldb, 128), plain)          # invalid until the next write of values: the 16-bit weights
        form, fi = form_of(d)
        assert form == 1 and fi["switch"] == 1 and fi["valid"] == 0 and fi["quantize_launches"] == 0 and fi["image_bytes"] > 0, fi
        d.set_values(dev(W))
        group = d.a8_get()[2]
        p.set_values(dev(dequantised(W, group)))
        want = product(p, key, Bt, ldb, 128)
        assert not same_bits(want, plain)                              # the numerics are the point
        assert same_bits(product(d, key, Bt, ldb, 128), want) and form_of(d)[0] == 3 and d.a8_info()["valid"] == 1
        p.set_values(dev(W))
        # (seven steps ahead is a choice of the launches outside the C ring: a row-major C here, the tiles of `zeros` are 24 rows tall)
        for env, rm in ((("SPARTA_H16_PATH", "lds"), False), (("SPARTA_H16_AHEAD", "7"), True)):
            monkeypatch.setenv(*env)
            assert same_bits(product(d, key, Bt, ldb, 128, rm), product(p, key, Bt, ldb, 128, rm)) and form_of(d)[0] == 1, env
            monkeypatch.delenv(env[0])
            product(d, key, Bt, ldb, 128, rm)
            assert form_of(d)[0] == 3, env
        d.set_forward_a8(False)
        assert same_bits(product(d, key, Bt, ldb, 128), plain) and form_of(d)[0] == 1 and d.a8_info()["switch"] == 0
        for n in (8, 256):
            for rm in (False, True):
                assert same_bits(product(d, key, Bt, ldb, n, rm), product(p, key, Bt, ldb, n, rm)), (n, rm)
        d.set_forward_a8(True)
        product(d, key, Bt, ldb, 128)
        assert form_of(d)[0] == 1                                      # switched on again: invalid until the next write
        d.set_values(dev(W))
        product(d, key, Bt, ldb, 128)
        assert form_of(d)[0] == 3
    finally:
        d.close()
        p.close()
    # a gathered B keeps the plain kernels (tiles64: cols = 4 x 64, two shards)
    key = "tiles64"
    v = geometry(key)
    d, p = (v.to_device(0, dtype=dtype, updatable=True, transposable=True) for _ in range(2))
    try:
        W = np.array(values(key))
        d.set_forward_a8(True, values=dev(W))
        p.set_values(dev(W))
        n, shard_rows = 128, int(v.cols) // 2
        Bg = gathered(rhs(key, dtype)[:, :n], shard_rows, dtype)
        out = []
        for h in (d, p):
            C = torch.full((n * int(v.rows),), float("nan"), device="cuda")
            h.spmm_gathered(Bg, shard_rows, C, n)
            torch.cuda.synchronize()
            out.append(C.cpu().numpy())
        assert same_bits(out[0], out[1]) and form_of(d)[0] == 1 and d.a8_info()["valid"] == 1
        Bt, ldb = b_tensor(rhs(key, dtype), dtype)
        product(d, key, Bt, ldb, n)
        assert form_of(d)[0] == 3
    finally:
        d.close()
        p.close()


def _refused(fn, *needles):
    with pytest.raises(sa.SpartaError) as e:
        fn()
    assert e.value.code == _lib.ERR_UNSUPPORTED, e.value
    for s in needles:
        assert s in str(e.value), (s, str(e.value))


def test_refusals(monkeypatch):
    v = geometry("zeros")
    for kw in (dict(dtype=sa.F32, updatable=True, transposable=True), dict(dtype=sa.F16, transposable=True)):
        d = v.to_device(0, **kw)
        try:
            _refused(lambda: d.set_forward_a8(True), "SPARTA_CREATE_UPDATABLE")
            assert d.a8_info()["switch"] == 0
        finally:
            d.close()
    for key in TWO_IMAGES + ("P64",):
        if key == "P64":                                   # the hub plan, forced onto this small matrix as tests/test_poison_gpu.py forces it
            for name, val in (("SPARTA_HUB_MIN_TOTAL", "1"), ("SPARTA_HUB_MIN_STEPS", "1"), ("SPARTA_HUB_G", "2"), ("SPARTA_HUB_TAU", "0.25")):
                monkeypatch.setenv(name, val)
        d = geometry(key).to_device(0, dtype=sa.BF16, updatable=True, transposable=True)
        try:
            assert (d.hub_info()["steps"] > 0) == (key == "P64")
            _refused(lambda: d.set_forward_a8(True), "one stream image")
            fi = d.a8_info()
            assert fi["switch"] == 0 and fi["capable"] == 0 and fi["image_bytes"] == 0, (key, fi)
        finally:
            d.close()
    for name in ("SPARTA_HUB_MIN_TOTAL", "SPARTA_HUB_MIN_STEPS", "SPARTA_HUB_G", "SPARTA_HUB_TAU"):
        monkeypatch.delenv(name, raising=False)
    d = v.to_device(0, dtype=sa.F16, updatable=True, transposable=True)
    try:
        scratch = torch.zeros(4, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        caught = []
        with torch.cuda.stream(s):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                scratch.add_(1.0)
                try:
                    d.set_forward_a8(True)
                except sa.SpartaError as err:
                    caught.append(err)
                scratch.add_(1.0)
            torch.cuda.synchronize()
            assert len(caught) == 1 and caught[0].code == _lib.ERR_UNSUPPORTED and "captured" in str(caught[0]) and "sparta_vbs_set_forward_a8" in str(caught[0])
            g.replay()
            torch.cuda.synchronize()
        assert float(scratch[0]) == 2.0 and d.a8_info()["switch"] == 0
        # the two switches exclude each other, either way round
        d.set_live_forward(True)
        _refused(lambda: d.set_forward_a8(True), "sparta_vbs_set_live_forward")
        d.set_live_forward(False)
        d.set_forward_a8(True)
        _refused(lambda: d.set_live_forward(True), "sparta_vbs_set_forward_a8")
        assert d.a8_info()["switch"] == 1 and d.live_forward_info()["switch"] == 0
        d.set_forward_a8(False)
        d.set_live_forward(True)
    finally:
        d.close()


@pytest.mark.parametrize("case", [("pairs", sa.F16), ("w96", sa.BF16), ("short64", sa.F16)], ids=case_id)
def test_never_stale(case, monkeypatch):
    """after set_values, sgd_step with momentum and adam_step in both forms, and a step skipped by a non-finite gradient, the product is that of the reference
    handle given the restatement of the new W; every one of them adds one quantise launch"""
    key, dtype = case
    d, p = handle(case, "a8"), handle(case, "ref")
    group = groups_of(d, key)
    n = 128
    Bt, ldb = b_tensor(rhs(key, dtype), dtype)
    rng = np.random.default_rng(9600)
    nz = int(geometry(key).nztot)
    Wt = dev(np.array(values(key)))
    G = dev(rng.uniform(-1, 1, nz))
    M, EA, EV = (torch.zeros(nz, device="cuda") for _ in range(3))
    S = torch.zeros(8, dtype=torch.int32, device="cuda")
    launches = [d.a8_info()["quantize_launches"]]

    def check(what, changed=True):
        W = Wt.cpu().numpy()
        p.set_values(dev(dequantised(W, group)))
        assert same_bits(product(d, key, Bt, ldb, n), product(p, key, Bt, ldb, n)), what
        assert form_of(d)[0] == 3, what
        launches.append(d.a8_info()["quantize_launches"])
        assert launches[-1] == launches[-2] + 1, (what, launches)
        return W

    d.set_values(Wt)
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
        # a step the control record skips: W stays, the image stays right
        ctl = sa.GradCtl()
        bad = G.clone()
        bad[nz // 2] = float("inf")
        ctl.collect(bad)
        d.adam_step(Wt, bad, EA, EV, S, lr=1e-2, ctl=ctl)
        assert ctl.read()["skip"] == 1
        W = check("skipped adam_step_ctl fuse=" + fuse)
        assert same_bits(W, last)
        d.sgd_step(Wt, bad, M, lr=0.05, momentum=0.9, ctl=ctl)
        W = check("skipped sgd_step_ctl fuse=" + fuse)
        assert same_bits(W, last)


@pytest.mark.parametrize("dtype", H16, ids=[DT_ID[t] for t in H16])
def test_poison(dtype):
    """pair tiles with absent halves (`pairs`: block-row ib stores neither block column ib nor (ib + 3) % 8): a NaN weight reaches only the rows of its
    block-row; an Inf in the rows of B that face block column 0 does not reach the block-rows that do not store it"""
    key = "pairs"
    case = (key, dtype)
    d, p = handle(case, "a8"), handle(case, "ref")
    v = geometry(key)
    group = groups_of(d, key)
    W = np.array(values(key))
    r0 = np.asarray(v.row_part, np.int64)
    B = rhs(key, dtype)
    Bt, ldb = b_tensor(B, dtype)
    d.set_values(dev(W))
    p.set_values(dev(dequantised(W, group)))
    clean = product(p, key, Bt, ldb, 128)
    assert np.isfinite(clean).all() and same_bits(product(d, key, Bt, ldb, 128), clean)
    # a NaN in the first stored element of block-row 2 (its row 0)
    off = int(sum((r0[ib + 1] - r0[ib]) * int(v.nzcount[ib]) * int(v.block_col_size) for ib in range(2)))
    Wn = W.copy()
    Wn[off] = np.nan
    d.set_values(dev(Wn))
    for n in (128, 256):
        for rm in (False, True):
            got = product(d, key, Bt, ldb, n, rm)
            inside = np.zeros(int(v.rows), bool)
            inside[r0[2]:r0[3]] = True
            assert np.isnan(got[r0[2]]).all(), (n, rm)
            assert np.isfinite(got[~inside]).all(), (n, rm)
            assert same_bits(np.ascontiguousarray(got[~inside]), np.ascontiguousarray(product(p, key, Bt, ldb, n, rm)[~inside])), (n, rm)
    # Inf in B under block column 0: block-rows 0 and 5 do not store it
    d.set_values(dev(W))
    Bp = B.copy()
    Bp[:int(v.block_col_size)] = np.inf
    Bpt, ldbp = b_tensor(Bp, dtype)
    free = np.zeros(int(v.rows), bool)
    for ib in (0, 5):
        assert 0 not in U.poison_present(ib)
        free[r0[ib]:r0[ib + 1]] = True
    for n in (128, 256):
        for rm in (False, True):
            got = product(d, key, Bpt, ldbp, n, rm)
            assert np.isfinite(got[free]).all(), (n, rm, int((~np.isfinite(got[free])).sum()))
            assert same_bits(np.ascontiguousarray(got[free]), np.ascontiguousarray(product(p, key, Bt, ldb, n, rm)[free])), (n, rm)
            assert not np.isfinite(got[~free]).all()                     # the input bites
    assert form_of(d)[0] == 3 and d.a8_info()["form_pair"] == 3


@pytest.mark.parametrize("key", ["zeros", "pairs"])
def test_capture(key):
    """adam_step + product in one graph, replayed three times, equals three eager rounds on a second handle: a replay requantises"""
    dtype = sa.F16
    v = geometry(key)
    d, e = (v.to_device(0, dtype=dtype, updatable=True, transposable=True) for _ in range(2))
    try:
        rows, n, nz = int(v.rows), 128, int(v.nztot)
        Bt, ldb = b_tensor(rhs(key, dtype), dtype)
        G = dev(np.random.default_rng(9700).uniform(-1, 1, nz))
        W0 = np.array(values(key))

        def state():
            return [dev(W0)] + [torch.zeros(nz, device="cuda") for _ in range(2)] + [torch.zeros(8, dtype=torch.int32, device="cuda")]

        sd, se = state(), state()
        saved = [t.clone() for t in sd]
        C = torch.zeros(n * rows, device="cuda")
        s = torch.cuda.Stream()
        for h in (d, e):
            h.set_forward_a8(True)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            d.adam_step(sd[0], G, sd[1], sd[2], sd[3], lr=1e-2)       # the eager warm-up; then the state it moved is put back
            d.spmm(Bt, C, n, ldb=ldb, ldc=rows)
            for t, t0 in zip(sd, saved):
                t.copy_(t0)
            torch.cuda.synchronize()
            before = d.a8_info()["quantize_launches"]
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                d.adam_step(sd[0], G, sd[1], sd[2], sd[3], lr=1e-2)
                d.spmm(Bt, C, n, ldb=ldb, ldc=rows)
            torch.cuda.synchronize()
            assert d.a8_info()["quantize_launches"] == before + 1
            for rnd in range(3):
                C.fill_(7.0)
                torch.cuda.synchronize()
                g.replay()
                torch.cuda.synchronize()
                got = C.cpu().numpy().reshape(n, rows).T
                e.adam_step(se[0], G, se[1], se[2], se[3], lr=1e-2)
                want = product(e, key, Bt, ldb, n)
                assert same_bits(sd[0].cpu().numpy(), se[0].cpu().numpy()), rnd
                assert same_bits(np.ascontiguousarray(got), want), rnd
                cd, ed, _ = d.a8_get()
                ce, ee, _ = e.a8_get()
                assert np.array_equal(cd, ce) and np.array_equal(ed, ee), rnd
        assert form_of(d)[0] == 3 and form_of(e)[0] == 3
    finally:
        d.close()
        e.close()


@pytest.mark.parametrize("dtype", H16, ids=[DT_ID[t] for t in H16])
@pytest.mark.parametrize("key", ["w128", "w96"])          # (pair / 64-row tiles; one-tile records with split tiles; vbs_linear wants even rows and cols)
def test_vbs_linear(key, dtype):
    """with the switch on y equals the reference handle on the dequantised values; grad_x and grad_values equal those of a plain handle on W, bit for bit"""
    v = geometry(key)
    a, r, p = (v.to_device(0, dtype=dtype, updatable=True, transposable=True) for _ in range(3))
    try:
        group = groups_of(a, key)
        W0 = np.array(values(key))
        n = 8
        x0 = torch.from_numpy(U.edge_round(np.random.default_rng(9800).uniform(-1, 1, (n, v.cols)), dtype)).to(TDT[dtype]).cuda()
        gy = torch.from_numpy(U.edge_round(np.random.default_rng(9801).uniform(-1, 1, (n, v.rows)), sa.F32)).float().cuda()

        def run(h, Wnp):
            x = x0.clone().requires_grad_(True)
            W = dev(Wnp).requires_grad_(True)
            y = vbs_linear(x, h, W)
            y.backward(gy)
            torch.cuda.synchronize()
            return y.detach().cpu().numpy(), x.grad.float().cpu().numpy(), W.grad.cpu().numpy()

        ya, gxa, gwa = run(a, W0)
        assert form_of(a)[0] == 3 and a.a8_info()["valid"] == 1
        yr, _, _ = run(r, dequantised(W0, group))
        yp, gxp, gwp = run(p, W0)
        assert same_bits(ya, yr) and not same_bits(ya, yp)
        assert same_bits(gxa, gxp) and same_bits(gwa, gwp)
    finally:
        for h in (a, r, p):
            h.close()
