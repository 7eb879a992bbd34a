"""sparta_vbs_adam_step on the GPU (k_update.hip): Adam / AdamW and set_values in one pass, the step count on the device.

After adam_step(W, G, M, V, S) the caller's W, M, V and the eight words of S must hold, bit for bit, what adam_ref (tests/test_adam_step_host.py: the numpy
float32 restatement of the arithmetic include/sparta_amd.h pins, division and square root correctly rounded) gives, on all nztot elements -- an element
updated twice or not at all shows there -- and every product of the handle must have the bits of a handle created from the W read back, with one product
path forced before both handles are made (the values are no small integers any more: two paths may sum in different orders).  The matrices, the canary
buffers, the table of handles with an owning image kernel and the product helpers are those of tests/test_sgd_step_gpu.py and the files it draws on."""
import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd.autograd import vbs_linear

torch = pytest.importorskip("torch")

from test_set_values_gpu import TDT, tall_groups, values, blocks_of, oracle, dense_b, product, check_close  # noqa: E402
from test_spmm_t_gpu import with_values, run_t, dense_x, hub_env, dense_and_mask  # noqa: E402
from test_sgd_step_gpu import (CANARY, PAD, CASES, CASE_IDS, FUSED, build_all, away_from_denormals, same_bits, make)  # noqa: E402
from test_adam_step_host import adam_ref, fresh_state  # noqa: E402

pytestmark = pytest.mark.gpu

F = torch.nn.functional
f32 = np.float32

CONFIGS = [dict(lr=1e-2),
           dict(lr=1e-2, weight_decay=0.01),
           dict(lr=1e-2, weight_decay=0.01, decoupled=False),
           dict(lr=0.25, betas=(0.5, 0.75), eps=1e-3, grad_scale=0.5)]


@pytest.fixture(scope="module")
def mats():
    return build_all()


class Operands:
    """W, G, M, V (n floats) and S (8 words) as slices of one device buffer each, PAD canary floats on both sides: every operand starts off a 16-byte boundary"""

    def __init__(self, n, W, G):
        self.n = n
        self.buf = [torch.full((k + 2 * PAD,), CANARY, dtype=torch.float32, device="cuda") for k in (n, n, n, n, 8)]
        self.W, self.G, self.M, self.V, self.S = (b[PAD:PAD + k] for b, k in zip(self.buf, (n, n, n, n, 8)))
        assert self.W.data_ptr() % 16 != 0 and self.S.data_ptr() % 16 != 0
        self.W.copy_(torch.from_numpy(np.ascontiguousarray(W, f32)))
        self.set_grad(G)
        for t in (self.M, self.V, self.S):
            t.zero_()

    def set_grad(self, G):
        self.G.copy_(torch.from_numpy(np.ascontiguousarray(G, f32)))

    def args(self):
        return self.W, self.G, self.M, self.V, self.S

    def read(self):
        """(W, M, V, S as uint32 words) on the host; asserts the canaries around all five"""
        torch.cuda.synchronize()
        for b in self.buf:
            h = b.cpu().numpy()
            assert np.all(h[:PAD] == CANARY) and np.all(h[-PAD:] == CANARY), "a write outside W, G, M, V or S"
        return tuple(t.cpu().numpy() for t in (self.W, self.M, self.V)) + (self.S.cpu().numpy().view(np.uint32),)


def draw_w(v, seed):
    return away_from_denormals(values(v, seed, integer=False) * 4)


def draw_g(rng, n):
    return away_from_denormals(rng.uniform(-4, 4, n) * (rng.random(n) < 0.8))


def assert_state(got, want, what):
    for name, a, b in zip(("W", "M", "V"), got, want):
        assert same_bits(a, b), what + (name, int((np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32)).sum()))
    assert np.array_equal(got[3], want[3]), what + ("S", got[3].tolist(), want[3].tolist())


# ---- 1. bit-exact state ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse", [None, "1", "0"], ids=["default", "fuse1", "fuse0"])
@pytest.mark.parametrize("key,dtype", CASES, ids=CASE_IDS)
def test_state_bit_exact(mats, key, dtype, fuse, monkeypatch):
    """every configuration on every geometry, under the default routing and with the image kernel asked for on every step / on none"""
    hub_env(monkeypatch, key)
    if fuse is None:
        monkeypatch.delenv("SPARTA_ADAM_FUSE", raising=False)
    else:
        monkeypatch.setenv("SPARTA_ADAM_FUSE", fuse)
    v = mats[key]
    n = int(v.nztot)
    H = make(v, dtype)
    assert H.step_info() == {"fused": -1, "launches": 0}
    if key == "hub":
        assert H.hub_info()["steps"] > 0
    rng = np.random.default_rng(100)
    forms = set()
    for ci, cfg in enumerate(CONFIGS):
        W = draw_w(v, 20 + ci)
        op = Operands(n, W, np.zeros(n, f32))
        ref = (W, np.zeros(n, f32), np.zeros(n, f32), fresh_state())
        for step in range(3):
            G = draw_g(rng, n)
            op.set_grad(G)
            H.adam_step(*op.args(), **cfg)
            ref = adam_ref(ref[0], G, ref[1], ref[2], ref[3], cfg)
            assert_state(op.read(), ref, (key, ci, step))
            info = H.step_info()
            forms.add(info["fused"])
            if fuse is not None:
                assert info["fused"] == (FUSED[(key, dtype)] if int(fuse) else 0), (key, cfg, info)
            # the tick is counted: tick + the owning image kernel (these handles are not transposable), or tick + elementwise + >= 1 set_values launch
            assert info["launches"] == 2 if info["fused"] else info["launches"] >= 3, (key, cfg, info)
    assert len(forms) == 1 and forms <= {0, FUSED[(key, dtype)]}, (key, forms)           # the same form on every step
    H.close()


# ---- 2. products follow ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,dtype", CASES, ids=CASE_IDS)
def test_products_follow(mats, key, dtype, monkeypatch):
    """the bits of a handle created from the W read back, after every step: every image holds what set_values(W_new) would have written"""
    hub_env(monkeypatch, key)
    monkeypatch.setenv("SPARTA_PATH", "stream")                      # one path for both handles (where the geometry has no stream plan: the generic kernels)
    monkeypatch.delenv("SPARTA_ADAM_FUSE", raising=False)
    v = mats[key]
    n = int(v.nztot)
    cfg = CONFIGS[1]
    rng = np.random.default_rng(200)
    B, X = dense_b(v, 128, 201, integer=False), dense_x(v.rows, 128, 202, integer=False)
    H = make(v, dtype, transposable=True)
    W = draw_w(v, 21)
    op = Operands(n, W, np.zeros(n, f32))
    ref = (W, np.zeros(n, f32), np.zeros(n, f32), fresh_state())
    for step in range(3):
        G = draw_g(rng, n)
        op.set_grad(G)
        H.adam_step(*op.args(), **cfg)
        ref = adam_ref(ref[0], G, ref[1], ref[2], ref[3], cfg)
        got = op.read()
        assert_state(got, ref, (key, step))
        Fh = with_values(v, got[0]).to_device(0, dtype=dtype, updatable=True, transposable=True)
        assert same_bits(product(H, v, B, dtype)[0], product(Fh, v, B, dtype)[0]), (key, step, "spmm")
        assert same_bits(run_t(H, X, dtype, v.cols)[0], run_t(Fh, X, dtype, v.cols)[0]), (key, step, "spmm_t")
        if dtype == sa.F32:
            assert same_bits(product(H, v, B, dtype, algo=sa.SPMM_EXACT)[0], product(Fh, v, B, dtype, algo=sa.SPMM_EXACT)[0]), (key, step, "exact")
        Fh.close()
    H.close()


# ---- 3. the zero pattern moves -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["grid32", "grid64", "padded", "pairs", "jaccard"])
def test_zero_pattern_moves_fp32(mats, key, monkeypatch):
    """lr = 0.5, weight_decay = 2, decoupled: dk = 1 - 1 is exactly 0, so W_new = W * 0 - step_size * (m / den).  One step from fresh state empties the
    columns whose G is zero (m = 0) and fills the all-zero columns whose G is not: the fragment image compacts the non-empty columns of every step, so its
    ballot must be taken on the COMPUTED values (STEP_KPAIRS)"""
    monkeypatch.setenv("SPARTA_PATH", "stream")
    monkeypatch.delenv("SPARTA_ADAM_FUSE", raising=False)
    v = mats[key]
    n, w = int(v.nztot), v.block_col_size
    cfg = dict(lr=0.5, weight_decay=2.0, decoupled=True)
    rng = np.random.default_rng(300)
    W = rng.integers(1, 5, n).astype(f32) * rng.choice([-1, 1], n).astype(f32)
    G = rng.integers(1, 5, n).astype(f32) * rng.choice([-1, 1], n).astype(f32)
    for off, h, _ in blocks_of(v):
        Wb, Gb = W[off:off + h * w].reshape(w, h), G[off:off + h * w].reshape(w, h)     # row c of the view = column c of the block
        kind = rng.integers(0, 3, w)
        Gb[kind == 0, :] = 0.0                                                           # the column empties
        Wb[kind == 1, :] = 0.0                                                           # an empty column that fills
    H = v.to_device(0, updatable=True)
    op = Operands(n, W, G)
    H.set_values(op.W)                                               # the handle holds W: its compaction is that of W's zero pattern
    B = dense_b(v, 128, 301, integer=True)
    assert np.array_equal(product(H, v, B, sa.F32)[0], oracle(v, W, B).astype(f32))
    H.adam_step(*op.args(), **cfg)
    ref = adam_ref(W, G, np.zeros(n, f32), np.zeros(n, f32), fresh_state(), cfg)
    was, now = (np.concatenate([(x[off:off + h * w].reshape(w, h) != 0).any(axis=1) for off, h, _ in blocks_of(v)]) for x in (W, ref[0]))
    assert (was & ~now).any() and (~was & now).any()
    got = op.read()
    assert_state(got, ref, (key,))
    Fh = with_values(v, got[0]).to_device(0)
    for n_cols in (32, 128):
        Bn = dense_b(v, n_cols, 302 + n_cols, integer=True)
        assert same_bits(product(H, v, Bn, sa.F32)[0], product(Fh, v, Bn, sa.F32)[0]), (key, n_cols)
    H.close(); Fh.close()


# ---- 4. range handle ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [sa.F32, sa.F16], ids=["f32", "f16"])
def test_range_handle_updates_its_slice(mats, dtype, monkeypatch):
    monkeypatch.delenv("SPARTA_ADAM_FUSE", raising=False)
    v = mats["grid32"]
    b0, b1 = 2, 5
    ends = np.concatenate([[0], np.cumsum(v.nzcount * np.diff(v.row_part) * v.block_col_size)])
    a0, a1 = int(ends[b0]), int(ends[b1])
    H = v.to_device(0, dtype=dtype, block_row_range=(b0, b1), updatable=True)
    n = a1 - a0
    assert H.info()["nztot"] == n
    cfg = CONFIGS[1]
    W, G = draw_w(v, 23)[a0:a1], draw_w(v, 24)[a0:a1]
    op = Operands(n, W, G)
    ref = (W, np.zeros(n, f32), np.zeros(n, f32), fresh_state())
    for step in range(2):
        H.adam_step(*op.args(), **cfg)
        ref = adam_ref(ref[0], G, ref[1], ref[2], ref[3], cfg)
        assert_state(op.read(), ref, (step,))                        # (asserts the canaries: only the slice's n elements were touched)
    B = dense_b(v, 128, 501, integer=False)
    C, Br = product(H, v, B, dtype)
    Wh = torch.from_numpy(ref[0]).to(TDT[dtype]).float().numpy()     # the values the handle stores
    Cref, bound = oracle(v, Wh, Br, b0, b1), oracle(v, np.abs(Wh), np.abs(Br), b0, b1)
    assert np.all(np.abs(C - Cref) <= 1e-5 * bound + 1e-30)
    full = [torch.zeros(int(v.nztot), dtype=torch.float32, device="cuda") for _ in range(4)]
    with pytest.raises(ValueError):
        H.adam_step(*full, op.S, lr=1e-2)
    H.close()


# ---- 5. capture --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [sa.F32, sa.F16], ids=["f32", "f16"])
def test_capture_from_the_first_call(mats, dtype, monkeypatch):
    """adam_step + spmm as one graph, the capture holding the handle's very first adam_step (the product ran once before: its first call tunes and
    allocates).  The step count lives in S: every replay advances it, and the bias corrections with it -- a count kept on the host would be baked in."""
    monkeypatch.delenv("SPARTA_ADAM_FUSE", raising=False)
    v = mats["padded"]
    n, nz = 128, int(v.nztot)
    cfg = CONFIGS[1]
    B = dense_b(v, n, 601, integer=True)
    ldb = v.cols + (v.cols & 1)
    t = torch.zeros((n, ldb), dtype=torch.float64)
    t[:, :v.cols] = torch.from_numpy(np.ascontiguousarray(B.T))
    Bt = t.cuda().to(TDT[dtype]).reshape(-1)
    W0, G = draw_w(v, 25), draw_w(v, 26)
    out = {}
    for mode in ("eager", "graph"):
        H = make(v, dtype)
        op = Operands(nz, W0, G)
        Ct = torch.zeros(v.rows * n, dtype=torch.float32, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            H.spmm(Bt, Ct, n, ldb=ldb)
            torch.cuda.synchronize()
            assert H.step_info()["fused"] == -1

            def step():
                H.adam_step(*op.args(), **cfg)
                H.spmm(Bt, Ct, n, ldb=ldb)
            if mode == "graph":
                gph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gph, stream=s):
                    step()
                torch.cuda.synchronize()
                got = op.read()                                      # a capture runs nothing
                assert same_bits(got[0], W0) and not got[1].any() and not got[2].any() and not got[3].any()
            res = []
            for _ in range(3):
                gph.replay() if mode == "graph" else step()
                torch.cuda.synchronize()
                res.append(op.read() + (Ct.cpu().numpy(),))
        out[mode] = res
        H.close()
    ref = (W0, np.zeros(nz, f32), np.zeros(nz, f32), fresh_state())
    for i in range(3):
        ref = adam_ref(ref[0], G, ref[1], ref[2], ref[3], cfg)
        for mode in ("eager", "graph"):
            assert int(out[mode][i][3][0]) == i + 1, (mode, i)
            assert_state(out[mode][i][:4], ref, (mode, i))
        assert same_bits(out["eager"][i][4], out["graph"][i][4]), (i, "C")


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(mats, monkeypatch):
    monkeypatch.delenv("SPARTA_ADAM_FUSE", raising=False)
    v = mats["jaccard"]
    n = 128
    B = dense_b(v, n, 701, integer=True)
    t = tall_groups()
    handles = {
        "plain": v.to_device(0),
        "from_csr": sa.DeviceVBS.from_csr(t, sa.BlockingEngine(tau=0.6, col_block_size=32).GetGrouping(t), 32, device=0),
        "transposed": sa.DeviceVBS.transposed_of(v, device=0),
    }
    state = torch.zeros(8, dtype=torch.int32, device="cuda")
    for name, d in handles.items():
        nz = d.info()["nztot"]
        z = [torch.zeros(max(nz, 1), dtype=torch.float32, device="cuda")[:nz] for _ in range(4)]
        with pytest.raises(sa.SpartaError) as e:
            d.adam_step(*z, state, lr=1e-2)
        assert e.value.code == sa._lib.ERR_UNSUPPORTED, name
        assert "sparta_vbs_adam_step" in str(e.value) and "SPARTA_CREATE_UPDATABLE" in str(e.value), name
        assert d.step_info()["fused"] == -1
    assert not state.cpu().numpy().any()
    for name in ("plain", "from_csr"):                              # (the same matrix: v is the VBS of t under the same grouping)
        C, Br = product(handles[name], v, B, sa.F32)
        check_close(C, v, v.mab, Br, name)
    # an updatable handle: missing operands, operands of the wrong kind, hyper-parameters out of range, a timed call inside a capture
    H = make(v, sa.F32)
    nz = int(v.nztot)
    W0, G0 = draw_w(v, 27), draw_w(v, 28)
    op = Operands(nz, W0, G0)
    H.set_values(op.W)
    W, G, M, V, S = op.args()
    for bad in ((W, G, None, V, S), (W, G, M, None, S), (W, G, M, V, None), (W.half(), G, M, V, S), (W, G[:-1], M, V, S), (W, G, M, V[:-1], S),
                (W, G, M, V, S[:-1]), (W, G, M, V, S.double()), (W, G, M, V, S.cpu())):
        with pytest.raises(ValueError):
            H.adam_step(*bad, lr=1e-2)
    with pytest.raises(ValueError):
        H.adam_step(W, G, M, V, S)                                   # no lr
    for kw in (dict(betas=(1.0, 0.999)), dict(betas=(0.9, 1.0)), dict(betas=(-0.1, 0.999)), dict(eps=0.0)):
        with pytest.raises(sa.SpartaError) as e:
            H.adam_step(W, G, M, V, S, lr=1e-2, **kw)
        assert e.value.code == sa._lib.ERR_INVALID and "sparta_vbs_adam_step" in str(e.value), kw
    cfg = sa._lib.AdamCfg(1e-2, 0.9, 0.999, 1e-8, 0.0, 1.0, 1, 5)    # reserved != 0, through the C entry itself
    import ctypes as C
    f32p = C.POINTER(C.c_float)
    rc = sa._lib.lib.sparta_vbs_adam_step(H.h, *(C.cast(C.c_void_p(x.data_ptr()), f32p) for x in (W, G, M, V)), C.c_void_p(S.data_ptr()), C.byref(cfg),
                                          None, None)
    assert rc == sa._lib.ERR_INVALID and "reserved" in sa._lib.lib.sparta_last_error().decode()
    assert H.step_info()["fused"] == -1                              # nothing ran
    got = op.read()
    assert same_bits(got[0], W0) and not got[1].any() and not got[2].any() and not got[3].any()
    Bi = dense_b(v, n, 702, integer=False)
    C_, Br = product(H, v, Bi, sa.F32)
    check_close(C_, v, W0, Br, "after the refused calls")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    caught = []
    with torch.cuda.stream(s):
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph, stream=s):
            try:
                H.adam_step(W, G, M, V, S, lr=1e-2, timed=True)
            except sa.SpartaError as err:
                caught.append(err)
            H.adam_step(W, G, M, V, S, lr=1e-2)                      # (the capture goes on: the refusal launched nothing)
        torch.cuda.synchronize()
        assert len(caught) == 1 and caught[0].code == sa._lib.ERR_UNSUPPORTED and "captured" in str(caught[0])
        assert same_bits(op.read()[0], W0)
        gph.replay()
        torch.cuda.synchronize()
    ref = adam_ref(W0, G0, np.zeros(nz, f32), np.zeros(nz, f32), fresh_state(), dict(lr=1e-2))
    assert_state(op.read(), ref, ("replay",))
    C_, Br = product(H, v, Bi, sa.F32)
    check_close(C_, v, ref[0], Br, "after the replay")
    assert H.adam_step(W, G, M, V, S, lr=1e-2, timed=True) > 0.0     # outside a capture the timed call is taken
    for h in list(handles.values()) + [H]:
        h.close()


# ---- 7. vbs_linear + VbsAdamW ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [sa.F32, sa.BF16], ids=["f32", "bf16"])
def test_vbs_linear_with_vbs_adamw(mats, dtype, monkeypatch):
    """four training steps, n = 2, x and grad_y in -1, 0, 1: the gradient of the values is exact small integers in every type (it does not depend on the
    values), so W must be adam_ref fed with the dense gradient masked to the stored positions, bit for bit, and as close to torch.optim.AdamW on a float64
    dense parameter as torch's own float32 run (the self-calibrating bound of tests/test_adam_step_host.py).  The state dict carries the step on."""
    monkeypatch.delenv("SPARTA_ADAM_FUSE", raising=False)
    v = mats["padded"]
    n, nz = 2, int(v.nztot)
    hyper = dict(lr=1e-2, weight_decay=0.01)
    _, rr, cc = dense_and_mask(v, v.mab)
    inside = cc >= 0
    mask = np.zeros((v.rows, v.cols))
    mask[rr[inside], cc[inside]] = 1.0
    mask = torch.from_numpy(mask)
    V0 = draw_w(v, 70)
    V0[~inside] = 0.0
    H = v.to_device(0, dtype=dtype, updatable=True, transposable=True)
    calls = []
    monkeypatch.setattr(H, "set_values", lambda *a, _f=H.set_values, **k: (calls.append(1), _f(*a, **k))[1])
    W = torch.from_numpy(V0.copy()).cuda().requires_grad_(True)
    D = {dt: torch.from_numpy(oracle(v, V0, np.eye(v.cols))).to(dt).requires_grad_(True) for dt in (torch.float64, torch.float32)}
    opt_w = sa.VbsAdamW([(H, W)], **hyper)
    opt_d = {dt: torch.optim.AdamW([p], **hyper) for dt, p in D.items()}
    x64 = np.ascontiguousarray(np.sign(dense_b(v, n, 71, integer=True).T))
    x = torch.from_numpy(x64).cuda().to(TDT[dtype]).requires_grad_(True)
    ref = (V0, np.zeros(nz, f32), np.zeros(nz, f32), fresh_state())
    H2 = W2 = opt_2 = None
    for step in range(4):
        gy64 = np.sign(dense_x(v.rows, n, 72 + step, integer=True).T)
        opt_w.zero_grad()
        y = vbs_linear(x, H, W)
        assert len(calls) == 1, step                                 # the first forward wrote the values; every later one finds the handle up to date
        y.backward(torch.from_numpy(gy64).float().cuda())
        gd = torch.from_numpy(gy64.T @ x64) * mask                   # the dense gradient of y = x D^T, masked to the stored positions
        gw = W.grad.cpu().numpy()
        assert np.array_equal(gw[inside], gd.numpy()[rr[inside], cc[inside]].astype(f32)) and not gw[~inside].any(), step
        if step == 2:                                                # a second optimizer and handle take the state over and go on beside the first
            H2 = v.to_device(0, dtype=dtype, updatable=True, transposable=True)
            W2 = W.detach().clone().requires_grad_(True)
            opt_2 = sa.VbsAdamW([(H2, W2)], lr=1.0)
            opt_2.load_state_dict(opt_w.state_dict())
        if opt_2 is not None:
            opt_2.zero_grad()
            vbs_linear(x, H2, W2).backward(torch.from_numpy(gy64).float().cuda())
            assert same_bits(W2.grad.cpu().numpy(), gw), step
            opt_2.step()
        opt_w.step()
        for dt, p in D.items():
            p.grad = gd.to(dt)
            opt_d[dt].step()
        ref = adam_ref(ref[0], gw, ref[1], ref[2], ref[3], hyper)
        Wh = W.detach().cpu().numpy()
        assert same_bits(Wh, ref[0]), step
        st = opt_w.state_dict()["state"][0]
        assert same_bits(st["exp_avg"].cpu().numpy(), ref[1]) and same_bits(st["exp_avg_sq"].cpu().numpy(), ref[2]), step
        assert np.array_equal(st["state"].cpu().numpy().view(np.uint32), ref[3]), step
        if opt_2 is not None:
            assert same_bits(W2.detach().cpu().numpy(), Wh), step
            assert np.array_equal(opt_2.state_dict()["state"][0]["state"].cpu().numpy().view(np.uint32), ref[3]), step
        t64 = D[torch.float64].detach().numpy()[rr[inside], cc[inside]]
        e_w = float(np.abs(Wh[inside].astype(np.float64) - t64).max())
        e_t32 = float(np.abs(D[torch.float32].detach().numpy()[rr[inside], cc[inside]].astype(np.float64) - t64).max())
        print("step %d: |W - torch64| = %.3e   |torch32 - torch64| = %.3e" % (step, e_w, e_t32))
        assert e_w <= 2 * e_t32, (step, e_w, e_t32)
    assert H.step_info()["fused"] in (0, 1) and len(calls) == 1
    # a backward whose forward saw the values before the step
    y = vbs_linear(x, H, W)
    assert len(calls) == 1
    y.backward(torch.ones_like(y), retain_graph=True)
    opt_w.step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward(torch.ones_like(y))
    H.close(); H2.close()
