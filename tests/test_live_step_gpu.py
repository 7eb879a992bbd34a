"""Live steps on the GPU: DeviceVBS.set_live_steps and what sgd_step / adam_step (plain and under a control record, fused and two-pass) do with a live-block
set installed -- the contract of include/sparta_amd.h, "WITH A LIVE-BLOCK SET INSTALLED AND LIVE STEPS ON".

Handles: the geometries and masks of tests/_live.py in fp32 (block widths 3, 13, 48, 100, 200, a ragged last block column, block-rows of height 0 that hold
blocks, a range handle, handles with and without a fused image), the 16-bit edge and training geometries in f16 and bf16 (pair tiles under `one_per_row` and
`row_dead`: halves that disagree), all made updatable and transposable.  References: a second handle of the same geometry with the switch off (bit for bit),
and live_step_ref of tests/test_live_step_host.py."""
import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd import _lib
from sparta_amd.autograd import vbs_linear

torch = pytest.importorskip("torch")

import _util as U  # noqa: E402
import _live as L  # noqa: E402
from test_adam_step_host import fresh_state  # noqa: E402
from test_live_step_host import live_step_ref  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
TDT = {sa.F32: torch.float32, sa.F16: torch.float16, sa.BF16: torch.bfloat16}
DT_ID = {sa.F32: "f32", sa.F16: "f16", sa.BF16: "bf16"}
H16 = (sa.F16, sa.BF16)


def _nztot(case):
    key, _, br = case
    return int(L.table(key, br)[:, 2].sum())


CASES = [c for c in [(k, sa.F32, br) for k, br in L.F32_CASES] + [(k, dt, None) for dt in H16 for k in U.EDGE_H16 + U.TRAIN_H16] if _nztot(c) > 0]
case_id = lambda c: "%s-%s%s" % (c[0], DT_ID[c[1]], "" if c[2] is None else "-range")  # noqa: E731
cases = pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
forms = pytest.mark.parametrize("form", ["fused", "twopass"])

# (entry, hyper-parameters, control record (coef, skip) or None, the masks of the three steps)
CHANGING = ("second", "rand50", "row_dead")
PAIRS = ("one_per_row", "row_dead", "one_per_row")
RUNS = [("sgd", dict(lr=0.5), None, ("all",) * 3),
        ("sgd", dict(lr=0.25, momentum=0.9, weight_decay=0.01), None, CHANGING),
        ("sgd", dict(lr=0.25, momentum=0.9), (0.5, 0), PAIRS),
        ("adam", dict(lr=1e-2, decoupled=False, weight_decay=0.01), None, ("none",) * 3),
        ("adam", dict(lr=1e-2, weight_decay=0.01), None, CHANGING),
        ("adam", dict(lr=1e-2, weight_decay=0.01), (0.25, 0), PAIRS),
        ("adam", dict(lr=1e-2), (0.25, 1), CHANGING),
        ("sgd", dict(lr=0.5, momentum=0.9), (0.25, 1), CHANGING)]

_HANDLES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for d in _HANDLES.values():
        d.close()
    _HANDLES.clear()


@pytest.fixture
def form_env(form, monkeypatch):
    for name in ("SPARTA_SGD_FUSE", "SPARTA_ADAM_FUSE"):
        if form == "twopass":
            monkeypatch.setenv(name, "0")
        else:
            monkeypatch.delenv(name, raising=False)
    return form


def handle(case, which):
    """two handles per case: "live" gets the switch, "plain" never does"""
    if (case, which) not in _HANDLES:
        key, dtype, br = case
        _HANDLES[(case, which)] = L.geometry(key).to_device(0, dtype=dtype, block_row_range=br, updatable=True, transposable=True)
    return _HANDLES[(case, which)]


def dims(case):
    key, _, br = case
    v = L.geometry(key)
    b0, b1 = br or (0, v.block_rows)
    return int(v.row_part[b1] - v.row_part[b0]), int(v.cols)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, f32)).cuda()


def record(ctl):
    """a control record with the given (coef, skip), or None"""
    if ctl is None:
        return None
    R = torch.zeros(_lib.GRAD_CTL_BYTES // 4, dtype=torch.int32, device="cuda")
    R[7] = int(np.array([ctl[0]], f32).view(np.int32)[0])
    R[8] = int(ctl[1])
    return R


@pytest.fixture(scope="module")
def operands():
    """per case: the dense operands of the three products, made once (the handle's dtype; 16-bit handles want an even leading dimension)"""
    cache = {}

    def get(case):
        if case not in cache:
            _, dtype, _ = case
            rows, cols = dims(case)
            n = 8
            rng = np.random.default_rng(8300)
            ldr, ldc = rows + (rows & 1), cols + (cols & 1)

            def op(r, ld):
                buf = np.zeros((n, ld), f32)
                buf[:, :r] = U.edge_round(rng.uniform(-1, 1, (n, r)), dtype)
                return torch.from_numpy(buf.reshape(-1)).to(TDT[dtype]).cuda()

            cache[case] = dict(n=n, ldr=ldr, ldc=ldc, B=op(cols, ldc), X=op(rows, ldr), Y=op(cols, ldc))
        return cache[case]

    return get


def products(d, case, o):
    """(spmm, spmm_t, sddmm) of the handle as it stands, device tensors"""
    rows, cols = dims(case)
    n = o["n"]
    C = torch.full((n * rows,), 3.5, dtype=torch.float32, device="cuda")
    Ct = torch.full((n * cols,), 3.5, dtype=torch.float32, device="cuda")
    G = torch.full((_nztot(case),), 3.5, dtype=torch.float32, device="cuda")
    d.spmm(o["B"], C, n, ldb=o["ldc"], ldc=rows)
    d.spmm_t(o["X"], Ct, n, ldx=o["ldr"], ldo=cols)
    d.sddmm(o["X"], o["Y"], G, n, ldx=o["ldr"], ldy=o["ldc"])
    return C, Ct, G


class State:
    """W, M, V, S of one handle on the device"""

    def __init__(self, W, M, V):
        self.W, self.M, self.V = dev(W), dev(M), dev(V)
        self.S = torch.zeros(8, dtype=torch.int32, device="cuda")

    def step(self, d, entry, cfg, G, R):
        if entry == "sgd":
            d.sgd_step(self.W, G, self.M if cfg.get("momentum", 0.0) != 0 else None, ctl=R, **cfg)
        else:
            d.adam_step(self.W, G, self.M, self.V, self.S, ctl=R, **cfg)

    def host(self):
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (self.W, self.M, self.V, self.S)]


def install(d, st, keep, G=None):
    """what BlockPruner does: the dead blocks zeroed in W, M, V (and G), the handle given the values and the mask"""
    kt = torch.from_numpy(np.array(keep)).cuda()
    d.mask_blocks(kt, *([st.W, st.M, st.V] + ([G] if G is not None else [])))
    d.set_values(st.W)
    d.set_live_blocks(kt)
    return kt


def draw(case, seed):
    n = _nztot(case)
    rng = np.random.default_rng(seed)
    W, M = (rng.uniform(-1, 1, n).astype(f32) for _ in range(2))
    V = rng.uniform(0.01, 1, n).astype(f32)
    Gs = [rng.uniform(-1, 1, n).astype(f32) for _ in range(3)]
    return W, M, V, Gs


@forms
@cases
def test_equivalence_on_dead_zero_tensors(case, form_env, operands):
    """dead blocks +0 in W, M, V and G: three live steps leave W, M, V, S and every product bit-identical to three plain steps on a second handle"""
    key, dtype, br = case
    a, b = handle(case, "live"), handle(case, "plain")
    o = operands(case)
    W, M, V, Gs = draw(case, 8400)
    a.set_live_steps(True)
    try:
        for entry, cfg, ctl, seq in RUNS:
            sa_, sb = State(W, M, V), State(W, M, V)
            R = record(ctl)
            for step, name in enumerate(seq):
                keep = L.mask(key, br, name)
                Ga, Gb = dev(Gs[step]), dev(Gs[step])
                install(a, sa_, keep, Ga)
                install(b, sb, keep, Gb)
                b.set_live_blocks(None)                               # the reference steps AND multiplies without a live set: its dead blocks are zeros
                sa_.step(a, entry, cfg, Ga, R)
                sb.step(b, entry, cfg, Gb, R)
                what = (case_id(case), form_env, entry, cfg, ctl, step, name)
                assert a.step_info()["live"] == 1 and b.step_info()["live"] == 0, what
                assert a.step_info() == b.step_info(), what           # the form taken and the launch count are those of the plain step
                for x, y in zip(sa_.host(), sb.host()):
                    assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), what
                a.set_live_blocks(None)                               # the products themselves without the live set: the images the steps wrote
                for x, y in zip(products(a, case, o), products(b, case, o)):
                    assert torch.equal(x, y), what
    finally:
        a.set_live_steps(False)
        a.set_live_blocks(None)


POISON_MASKS = ("second", "row_dead", "one_per_row", "rand90")


@forms
@cases
def test_dead_blocks_depend_on_nothing(case, form_env, operands):
    """NaN / Inf / 1e30 in the dead blocks of G, M and V: the live elements get the bits of the clean run (and of live_step_ref), the dead blocks of M and V
    keep the poison bit for bit, W stays +0 there, the forward product is finite and that of the clean run -- and with the switch off the same inputs give
    non-finite weights"""
    key, dtype, br = case
    a, b = handle(case, "live"), handle(case, "plain")
    o = operands(case)
    W, M, V, Gs = draw(case, 8500)
    T = L.table(key, br)
    poison = np.array([np.nan, np.inf, 1e30], f32)
    a.set_live_steps(True)
    try:
        for i, (entry, cfg, ctl) in enumerate([("sgd", dict(lr=0.25, momentum=0.9, weight_decay=0.01), None), ("adam", dict(lr=1e-2, weight_decay=0.01), (0.5, 0)),
                                               ("adam", dict(lr=1e-2), (0.5, 1))]):
            name = POISON_MASKS[(i + len(T)) % len(POISON_MASKS)]
            keep = L.mask(key, br, name)
            live = L.element_keep(T, keep)
            dead = ~live
            Wz = np.where(live, W, f32(0.0)).astype(f32)
            clean = [np.where(live, x, f32(0.0)).astype(f32) for x in (Gs[0], M, V)]
            dirty = [x.copy() for x in clean]
            for x in dirty:
                x[dead] = poison[np.arange(int(dead.sum())) % 3]
            R = record(ctl)
            kt = torch.from_numpy(np.array(keep)).cuda()
            res = []
            for G0, M0, V0 in (clean, dirty):
                st = State(Wz, M0, V0)
                a.set_values(st.W)
                a.set_live_blocks(kt)
                st.step(a, entry, cfg, dev(G0), R)
                assert a.step_info()["live"] == 1
                a.set_live_blocks(None)
                res.append((st.host(), products(a, case, o)[0].cpu().numpy()))
            what = (case_id(case), form_env, entry, name)
            (cw, cm, cv, cs), cprod = res[0]
            (gw, gm, gv, gs), gprod = res[1]
            for x, y in ((gw, cw), (gm, cm), (gv, cv)):
                assert np.array_equal(bits(x)[live], bits(y)[live]), what
            assert np.array_equal(gs, cs), what
            assert not bits(gw)[dead].any(), what
            assert np.array_equal(bits(gm)[dead], bits(dirty[1])[dead]) and np.array_equal(bits(gv)[dead], bits(dirty[2])[dead]), what
            assert np.isfinite(gprod).all() and np.array_equal(gprod, cprod), what
            # the oracle
            ref = live_step_ref(entry, Wz, dirty[0], dirty[1], dirty[2], fresh_state(), dict(cfg), live, coef=None if ctl is None else ctl[0],
                                skip=bool(ctl and ctl[1]))
            assert np.array_equal(bits(gw), bits(ref[0])) and np.array_equal(bits(gm), bits(ref[1])), what
            if entry == "adam":
                assert np.array_equal(bits(gv), bits(ref[2])) and np.array_equal(gs.view(np.uint32), ref[3]), what
            # the switch off: the poison reaches the weights (not under a skipped step, which touches nothing either way)
            if dead.any() and not (ctl and ctl[1]):
                st = State(Wz, dirty[1], dirty[2])
                b.set_values(st.W)
                b.set_live_blocks(kt)
                st.step(b, entry, cfg, dev(dirty[0]), R)
                assert b.step_info()["live"] == 0
                assert not np.isfinite(st.host()[0][dead]).all(), what
                b.set_live_blocks(None)
    finally:
        a.set_live_steps(False)
        a.set_live_blocks(None)
        a.set_values(dev(W))
        b.set_values(dev(W))
        torch.cuda.synchronize()


def test_forms_taken(monkeypatch):
    """a handle without a fused image takes the blocks kernel (fused 0, live 1); one with a fused image takes it live in both forms"""
    for name in ("SPARTA_SGD_FUSE", "SPARTA_ADAM_FUSE"):
        monkeypatch.delenv(name, raising=False)
    seen = set()
    for case in [("w48", sa.F32, None), ("heights64", sa.F32, None), ("w128", sa.F32, None), ("w128", sa.F16, None), ("heights32", sa.BF16, None)]:
        key, dtype, br = case
        d = handle(case, "live")
        W, M, V, Gs = draw(case, 8600)
        st = State(W, M, V)
        d.set_live_steps(True)
        try:
            install(d, st, L.mask(key, br, "second"))
            st.step(d, "adam", dict(lr=1e-2), dev(Gs[0]), None)
            info = d.step_info()
            assert info["live"] == 1
            seen.add(info["fused"])
            if key in ("w48", "heights64"):
                assert info["fused"] == 0 and info["live"] == 1, case_id(case)
            monkeypatch.setenv("SPARTA_ADAM_FUSE", "0")
            st.step(d, "adam", dict(lr=1e-2), dev(Gs[1]), None)
            assert d.step_info()["fused"] == 0 and d.step_info()["live"] == 1
            monkeypatch.delenv("SPARTA_ADAM_FUSE")
        finally:
            d.set_live_steps(False)
            d.set_live_blocks(None)
            d.set_values(dev(W))
    assert seen == {0, 1}


def test_switches():
    key = "w128"
    v = L.geometry(key)
    for dtype in (sa.F32, sa.F16):
        case = (key, dtype, None)
        d = v.to_device(0, dtype=dtype, updatable=True, transposable=True)     # a fresh handle: nothing built yet
        try:
            W, M, V, Gs = draw(case, 8700)
            keep = L.mask(key, None, "rand50")
            live = L.element_keep(L.table(key, None), keep)
            G = np.where(live, Gs[0], f32(np.nan)).astype(f32)                  # NaN in the dead blocks of G: a plain step shows it in W

            def run(expect_live):
                st = State(np.where(live, W, f32(0.0)), np.where(live, M, f32(0.0)), np.where(live, V, f32(0.0)))
                d.set_values(st.W)
                st.step(d, "adam", dict(lr=1e-2), dev(G), None)
                w = st.host()[0]
                assert d.step_info()["live"] == expect_live
                assert np.isfinite(w).all() == bool(expect_live)
                return w

            assert d.live_info()["live_steps"] == 0
            kt = torch.from_numpy(np.array(keep)).cuda()
            d.set_live_blocks(kt)
            run(0)                                                  # a live set without the switch: the plain step
            d.set_live_steps(True)                                  # enabling after a set is installed: no new set_live_blocks needed
            assert d.live_info()["live_steps"] == 1 and d.live_info()["installed"] == 1
            first = run(1)
            d.set_live_blocks(None)                                 # no live set: the plain step again, the switch stays
            assert d.live_info()["live_steps"] == 1
            run(0)
            d.set_live_blocks(kt)
            assert np.array_equal(bits(run(1)), bits(first))
            d.set_live_steps(False)
            assert d.live_info()["live_steps"] == 0
            run(0)
        finally:
            d.close()
    # a handle that takes no steps, and one that takes no live set
    d = v.to_device(0, transposable=True)
    try:
        with pytest.raises(sa.SpartaError) as e:
            d.set_live_steps(True)
        assert e.value.code == _lib.ERR_UNSUPPORTED and "sparta_vbs_set_live_steps" in str(e.value)
    finally:
        d.close()
    m = sa.gen.uniform_random(300, 200, 3000, seed=3)
    dc = sa.DeviceVBS.from_csr(m, sa.BlockingEngine(tau=0.6, col_block_size=32).GetGrouping(m), 32, device=0)
    try:
        with pytest.raises(sa.SpartaError) as e:
            dc.set_live_steps(True)
        assert e.value.code == _lib.ERR_UNSUPPORTED
    finally:
        dc.close()


@pytest.mark.parametrize("dtype", [sa.F32, sa.F16], ids=["f32", "f16"])
def test_capture(dtype):
    """the first enabling call is refused under capture and leaves the capture usable; after one eager warm-up set_live_blocks + an Adam step replay from one
    graph, follow keep rewritten in place between replays, and advance t in S per replay"""
    key = "w128"
    case = (key, dtype, None)
    v = L.geometry(key)
    d, ref = v.to_device(0, dtype=dtype, updatable=True, transposable=True), handle(case, "plain")
    try:
        T = L.table(key, None)
        W, M, V, Gs = draw(case, 8800)
        m1, m2 = L.mask(key, None, "second"), L.mask(key, None, "rand90")
        # (W, G, M, V are non-zero everywhere: only the state is compared, and a dead block's W, M, V are untouched whatever they hold)
        G = dev(Gs[0])
        st = State(W, M, V)
        keep = torch.from_numpy(np.array(m1)).cuda()
        scratch = torch.zeros(4, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        caught = []
        cfg = dict(lr=1e-2, weight_decay=0.01)
        with torch.cuda.stream(s):
            g1 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g1, stream=s):
                scratch.add_(1.0)
                try:
                    d.set_live_steps(True)
                except sa.SpartaError as err:
                    caught.append(err)
                scratch.add_(1.0)
            torch.cuda.synchronize()
            assert len(caught) == 1 and caught[0].code == _lib.ERR_UNSUPPORTED and "captured" in str(caught[0]) and "sparta_vbs_set_live_steps" in str(caught[0])
            g1.replay()
            torch.cuda.synchronize()
            assert float(scratch[0]) == 2.0 and d.live_info()["live_steps"] == 0
            d.set_live_steps(True)                                   # the eager warm-up: helper arrays, one set, one step
            d.set_values(st.W)
            d.set_live_blocks(keep)
            st.step(d, "adam", cfg, G, None)
            torch.cuda.synchronize()
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2, stream=s):
                d.set_live_blocks(keep)
                st.step(d, "adam", cfg, G, None)
            torch.cuda.synchronize()
            assert d.step_info()["live"] == 1
            want = State(W, M, V)                                  # the eager reference: plain steps on the second handle, the dead blocks put back by hand
            lv = L.element_keep(T, m1)
            want.step(ref, "adam", cfg, G, None)
            for t, x0 in zip((want.W, want.M, want.V), (W, M, V)):
                t.copy_(dev(np.where(lv, t.cpu().numpy(), x0)))
            for n, m in enumerate((m1, m2, m1)):
                keep.copy_(torch.from_numpy(np.array(m)).cuda())
                torch.cuda.synchronize()
                g2.replay()
                torch.cuda.synchronize()
                # the reference follows the mask by hand: a plain step, then the blocks dead under m put back (the live step never touched them)
                before = want.host()
                want.step(ref, "adam", cfg, G, None)
                after = want.host()
                lv = L.element_keep(T, m)
                for t, x0, x1 in zip((want.W, want.M, want.V), before, after):
                    t.copy_(dev(np.where(lv, x1, x0)))
                got = st.host()
                for x, y in zip(got, want.host()):
                    assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), n
                assert int(got[3][0]) == n + 2                      # t: the warm-up step, then one per replay
                assert d.live_info()["live_blocks"] == int(np.count_nonzero(m))
        torch.cuda.synchronize()
    finally:
        ref.set_values(dev(np.array(v.mab, f32)))
        d.close()


@pytest.mark.parametrize("dtype", [sa.F32, sa.F16], ids=["f32", "f16"])
def test_training_with_live_steps(dtype):
    """the w128 loop of tests/test_live_gpu.py: vbs_linear + VbsAdamW + BlockPruner for four steps, prune(0.5) after the first and prune(0.75) after the third.
    BlockPruner(skip_pruned=True, live_steps=True) against skip_pruned=True alone: W, both moments and S bit-identical"""
    v = U.train_geometries()["w128"]
    W0 = np.random.default_rng(5800).uniform(-1, 1, int(v.nztot)).astype(f32)
    n = 8
    rnd = lambda shape, seed, dt: U.edge_round(np.random.default_rng(seed).uniform(-1, 1, shape), dt)  # noqa: E731
    xs = [torch.from_numpy(rnd((n, v.cols), 5810 + s, dtype)).to(TDT[dtype]).cuda() for s in range(4)]
    gys = [torch.from_numpy(rnd((n, v.rows), 5820 + s, sa.F32)).float().cuda() for s in range(4)]

    def train(live_steps):
        H = v.to_device(0, dtype=dtype, updatable=True, transposable=True)
        try:
            W = torch.from_numpy(W0.copy()).cuda().requires_grad_(True)
            opt = sa.VbsAdamW([(H, W)], lr=1e-2, weight_decay=0.01)
            pruner = sa.BlockPruner(opt, skip_pruned=True, live_steps=live_steps)
            trace, lives = [], []
            for step in range(4):
                x = xs[step].clone().requires_grad_(True)
                opt.zero_grad()
                y = vbs_linear(x, H, W)
                y.backward(gys[step].to(y.dtype))
                opt.step()
                lives.append(H.step_info()["live"])
                st = opt._state[0]
                trace.append([t.detach().cpu().numpy().copy() for t in (W, st["exp_avg"], st["exp_avg_sq"], st["state"])])
                if step in (0, 2):
                    pruner.prune(0.5 if step == 0 else 0.75)
            return trace, lives, H.live_info()["live_steps"]
        finally:
            H.close()

    (a, la, on_a), (b, lb, on_b) = train(True), train(False)
    assert la == [0, 1, 1, 1] and lb == [0, 0, 0, 0] and on_a == 1 and on_b == 0
    for step, (ta, tb) in enumerate(zip(a, b)):
        for name, x, y in zip(("W", "exp_avg", "exp_avg_sq", "state"), ta, tb):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (step, name)
