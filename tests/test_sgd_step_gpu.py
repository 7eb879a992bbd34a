"""sparta_vbs_sgd_step on the GPU (k_update.hip): the optimizer update and set_values in one pass.

After sgd_step(W, G, M) the caller's W and M must hold, bit for bit, what a numpy float32 restatement of the pinned arithmetic gives (every operation
rounded once, in the order include/sparta_amd.h states), on all nztot elements -- an element updated twice or not at all shows there -- and every product
of the handle must be what a handle created from the W read back computes: SPARTA_SPMM_EXACT on fp32, MFMA spmm and spmm_t on small-integer data (W, G
integers with |.| <= 4, lr = 0.5, momentum 0 / 0.5, three steps: values multiples of 1/8 below 16, exact in f16, bf16 and fp32; every partial sum exact).
The matrices, the zero-pattern value generator and the product helpers are those of tests/test_set_values_gpu.py and tests/test_spmm_t_gpu.py."""
import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd.autograd import vbs_linear

torch = pytest.importorskip("torch")

from test_set_values_gpu import (TDT, DT_ID, build_mats, tall_groups, vbr_of, values, blocks_of, oracle, dense_b, product, rounded,  # noqa: E402
                                 check_close)
from test_spmm_t_gpu import with_values, run_t, dense_x, hub_env, dense_and_mask  # noqa: E402

pytestmark = pytest.mark.gpu

F = torch.nn.functional
f32 = np.float32
CANARY = 7654.25
PAD = 67                                                             # floats in front of and behind each operand: odd, so W, G, M start off 16-byte boundaries


def build_all():
    out = build_mats()
    # blocks of 7 rows x 1 column: no stream plan (the elementwise kernel + the set_values launches), nztot not a multiple of 4 (its one-by-one tail)
    m = sa.gen.uniform_random(77, 60, 300, seed=47)
    out["odd"] = vbr_of(m, np.arange(m.rows, dtype=np.int64) // 7, 1)
    assert out["odd"].nztot % 4 != 0
    return out


@pytest.fixture(scope="module")
def mats():
    return build_all()


F32_KEYS = ["grid1", "grid8", "grid32", "grid64", "jaccard", "padded", "pairs", "odd"]
H16_KEYS = ["grid32", "grid64", "jaccard", "padded", "pairs", "hub"]           # 16-bit handles only where w % 32 == 0
CASES = [(k, sa.F32) for k in F32_KEYS] + [(k, dt) for dt in (sa.F16, sa.BF16) for k in H16_KEYS]
CASE_IDS = ["%s-%s" % (k, DT_ID[dt]) for k, dt in CASES]

# Every step asks for the image kernel by default (it measured faster on the headline handle with and without momentum);
# SPARTA_SGD_FUSE=0 asks for the two-pass form on every step, 1 is the default spelled out.
def wants_image_kernel(fuse):
    return fuse is None or bool(int(fuse))


# step_info()["fused"] of a step that asks for the image kernel, read off the plan code (build_stream_plans, vbs_plan.cpp):
#   fp32    1 where every block-row is at most 32 rows tall and w % 32 == 0 (one-tile plan with a fragment image, no 33..64-row tiles); 0 for jaccard
#           (block-rows of 100 rows: tiles of 64 + 36 rows), and for w = 1, 8 (no stream plan at all)
#   16-bit  1 where ONE stream image holds everything: grid32 / grid64 (block-rows of 16 rows: <= 32-row tiles only), jaccard (64 + 36 rows: 33..64-row
#           tiles only), padded / pairs (32-row block-rows walked as pair tiles, which are tiles of the 33..64-row plan); 0 with a hub plan
FUSED = {("grid1", sa.F32): 0, ("grid8", sa.F32): 0, ("odd", sa.F32): 0, ("grid32", sa.F32): 1, ("grid64", sa.F32): 1, ("jaccard", sa.F32): 0,
         ("padded", sa.F32): 1, ("pairs", sa.F32): 1}
for _dt in (sa.F16, sa.BF16):
    FUSED.update({("grid32", _dt): 1, ("grid64", _dt): 1, ("jaccard", _dt): 1, ("padded", _dt): 1, ("pairs", _dt): 1, ("hub", _dt): 0})

CONFIGS = [dict(lr=0.5),                                             # plain
           dict(lr=0.25, momentum=0.9),
           dict(lr=0.5, momentum=0.9, weight_decay=0.01),
           dict(lr=0.25, momentum=0.9, weight_decay=0.01, grad_scale=0.5)]


def sgd_ref(W, G, M, lr, momentum=0.0, weight_decay=0.0, grad_scale=1.0):
    """the arithmetic of include/sparta_amd.h in numpy float32: one rounding per operation, no fused multiply-add.  Returns (W, M) after the step."""
    W, g = np.asarray(W, f32), np.asarray(G, f32)
    if grad_scale != 1:
        g = g * f32(grad_scale)
    if weight_decay != 0:
        g = g + f32(weight_decay) * W
    if momentum != 0:
        M = f32(momentum) * np.asarray(M, f32) + g
        g = M
    return W - f32(lr) * g, M


def away_from_denormals(x):
    """|x| in {0} u [2^-8, 4]"""
    x = np.asarray(x, f32).copy()
    small = (x != 0) & (np.abs(x) < 2.0 ** -8)
    x[small] = np.sign(x[small]) * f32(2.0 ** -8)
    return np.clip(x, -4, 4)


class Operands:
    """W, G, M as slices of one device buffer each, PAD canary floats on both sides"""

    def __init__(self, n, W, G, momentum=True):
        self.n = n
        self.buf = [torch.full((n + 2 * PAD,), CANARY, dtype=torch.float32, device="cuda") for _ in range(3)]
        self.W, self.G, self.M = (b[PAD:PAD + n] for b in self.buf)
        assert self.W.data_ptr() % 16 != 0
        self.W.copy_(torch.from_numpy(np.ascontiguousarray(W, f32)))
        self.set_grad(G)
        self.M.zero_()
        if not momentum:
            self.M = None

    def set_grad(self, G):
        self.G.copy_(torch.from_numpy(np.ascontiguousarray(G, f32)))

    def read(self):
        torch.cuda.synchronize()
        for b in self.buf:
            h = b.cpu().numpy()
            assert np.all(h[:PAD] == CANARY) and np.all(h[PAD + self.n:] == CANARY), "a write outside W, G or M"
        return self.W.cpu().numpy(), None if self.M is None else self.M.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


def make(v, dtype, **kw):
    return v.to_device(0, dtype=dtype, updatable=True, **kw)


# ---- 1. bit-exact state (+ 4. the path report) --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse", [None, "1", "0"], ids=["default", "fuse1", "fuse0"])
@pytest.mark.parametrize("key,dtype", CASES, ids=CASE_IDS)
def test_w_and_m_bit_exact(mats, key, dtype, fuse, monkeypatch):
    """every configuration on every geometry, under the default routing and with the image kernel asked for on every step / on none"""
    hub_env(monkeypatch, key)
    if fuse is None:
        monkeypatch.delenv("SPARTA_SGD_FUSE", raising=False)
    else:
        monkeypatch.setenv("SPARTA_SGD_FUSE", fuse)
    v = mats[key]
    n = int(v.nztot)
    H = make(v, dtype)
    assert H.step_info() == {"fused": -1, "launches": 0}
    if key == "hub":
        assert H.hub_info()["steps"] > 0
    rng = np.random.default_rng(100)
    W = away_from_denormals(values(v, 20, integer=False) * 4)
    op = Operands(n, W, np.zeros(n, f32))
    M = np.zeros(n, f32)
    for ci, cfg in enumerate(CONFIGS):
        for step in range(3):
            G = away_from_denormals(rng.uniform(-4, 4, n) * (rng.random(n) < 0.8))
            op.set_grad(G)
            mom = cfg.get("momentum", 0.0) != 0
            H.sgd_step(op.W, op.G, op.M if mom else None, **cfg)
            W, Mn = sgd_ref(W, G, M, **cfg)
            if mom:
                M = Mn
            Wd, Md = op.read()
            assert same_bits(Wd, W), (key, ci, step, "W", int((Wd.view(np.uint32) != W.view(np.uint32)).sum()))
            assert same_bits(Md, M), (key, ci, step, "M", int((Md.view(np.uint32) != M.view(np.uint32)).sum()))
            info = H.step_info()
            assert info["fused"] == (FUSED[(key, dtype)] if wants_image_kernel(fuse) else 0), (key, cfg, info)
            assert info["launches"] == 1 if info["fused"] else info["launches"] >= 2, (key, cfg, info)
    H.close()


@pytest.mark.parametrize("dtype", [sa.F32, sa.F16, sa.BF16], ids=["f32", "f16", "bf16"])
def test_path_report(mats, dtype, monkeypatch):
    """step_info == 1 on padded and pairs in every type, with and without momentum: the arithmetic runs inside an image kernel on the one-tile fp32 plan and on
    the pair-tile 16-bit plan (the headline handle's geometry); in the elementwise kernel where an fp32 handle has 33..64-row tiles; a transposable 16-bit
    handle adds the launch of its spmm_t image"""
    monkeypatch.delenv("SPARTA_SGD_FUSE", raising=False)
    G = {k: torch.zeros(int(mats[k].nztot), dtype=torch.float32, device="cuda") for k in ("padded", "pairs", "jaccard")}
    for key in ("padded", "pairs"):
        for tr in (False, True):
            H = make(mats[key], dtype, transposable=tr)
            W = torch.from_numpy(mats[key].mab).cuda()
            H.sgd_step(W, G[key], torch.zeros_like(W), lr=0.5, momentum=0.5)
            assert H.step_info() == {"fused": 1, "launches": 2 if (tr and dtype != sa.F32) else 1}, (key, tr)
            H.sgd_step(W, G[key], lr=0.5)
            assert H.step_info() == {"fused": 1, "launches": 2 if (tr and dtype != sa.F32) else 1}, (key, tr)
            H.close()
    if dtype == sa.F32:
        H = make(mats["jaccard"], dtype)
        W = torch.from_numpy(mats["jaccard"].mab).cuda()
        H.sgd_step(W, G["jaccard"], torch.zeros_like(W), lr=0.5, momentum=0.5)
        assert H.step_info() == {"fused": 0, "launches": 2}                  # the elementwise kernel, then the copy into the reference-layout image
        H.close()
    torch.cuda.synchronize()


# ---- 2. products follow --------------------------------------------------------------------------------------------------------------------------
def products(d, v, dtype, B, X, exact=False):
    out = [product(d, v, B, dtype)[0], run_t(d, X, dtype, v.cols)[0]]
    if exact:
        out.append(product(d, v, B, dtype, algo=sa.SPMM_EXACT)[0])
    return out


@pytest.mark.parametrize("key,dtype", CASES, ids=CASE_IDS)
def test_products_follow(mats, key, dtype, monkeypatch):
    hub_env(monkeypatch, key)
    v = mats[key]
    n = int(v.nztot)
    rng = np.random.default_rng(200)
    B, X = dense_b(v, 128, 201, integer=True), dense_x(v.rows, 128, 202, integer=True)
    for momentum in (0.0, 0.5):
        H = make(v, dtype, transposable=True)
        W = values(v, 21, integer=True)
        M = np.zeros(n, f32)
        op = Operands(n, W, np.zeros(n, f32), momentum=momentum != 0)
        for step in range(3):
            G = values(v, 30 + step, integer=True) if step != 1 else rng.integers(-4, 5, n).astype(f32)
            op.set_grad(G)
            H.sgd_step(op.W, op.G, op.M, lr=0.5, momentum=momentum)
            W, M = sgd_ref(W, G, M, 0.5, momentum)
            Wd, _ = op.read()
            assert same_bits(Wd, W), (key, momentum, step)
            assert same_bits(rounded(Wd, dtype), Wd) and np.abs(Wd).max() <= 64           # exact in the handle's type
            Fh = with_values(v, Wd).to_device(0, dtype=dtype, updatable=True, transposable=True)
            for a, b, what in zip(products(H, v, dtype, B, X), products(Fh, v, dtype, B, X), ("spmm", "spmm_t")):
                assert same_bits(a, b), (key, momentum, step, what)
            assert np.array_equal(product(H, v, B, dtype)[0], oracle(v, Wd, B).astype(f32)), (key, momentum, step)
            Fh.close()
        H.close()
    if dtype != sa.F32:
        return
    # fp32, random values, the exact-order kernel: the bits of a fresh handle after every step
    H = make(v, dtype)
    W = away_from_denormals(values(v, 22, integer=False) * 4)
    op = Operands(n, W, np.zeros(n, f32))
    Br = dense_b(v, 128, 203, integer=False)
    for step in range(3):
        op.set_grad(away_from_denormals(values(v, 40 + step, integer=False) * 4))
        H.sgd_step(op.W, op.G, op.M, lr=0.25, momentum=0.9, weight_decay=0.01)
        Wd, _ = op.read()
        Fh = with_values(v, Wd).to_device(0)
        a, b = (product(d, v, Br, dtype, algo=sa.SPMM_EXACT)[0] for d in (H, Fh))
        assert same_bits(a, b), (key, step)
        Fh.close()
    H.close()


# ---- 3. the zero pattern moves -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["grid32", "grid64", "padded", "pairs", "jaccard"])
def test_zero_pattern_moves_fp32(mats, key):
    """one step empties whole 32-deep columns of some blocks (W = lr G there) and fills columns that were all zero (W = 0, G != 0): the fragment image
    compacts the non-empty columns of every step, so its ballot must be taken on the COMPUTED values (STEP_KPAIRS)"""
    v = mats[key]
    n, w, lr = int(v.nztot), v.block_col_size, 0.5
    rng = np.random.default_rng(300)
    W = rng.integers(1, 5, n).astype(f32) * rng.choice([-1, 1], n).astype(f32)
    G = rng.integers(-4, 5, n).astype(f32)
    emptied = filled = 0
    for q, (off, h, _) in enumerate(blocks_of(v)):
        Wb, Gb = W[off:off + h * w].reshape(w, h), G[off:off + h * w].reshape(w, h)     # row c of the view = column c of the block
        kind = rng.integers(0, 3, w)
        Gb[kind == 0, :] = Wb[kind == 0, :] / f32(lr)                                    # W - lr G == 0: the column empties
        Wb[kind == 1, :] = 0.0                                                           # an empty column ...
        Gb[kind == 1, :] = rng.integers(1, 5, (int((kind == 1).sum()), h)).astype(f32)   # ... that fills
        emptied += int((kind == 0).sum()); filled += int((kind == 1).sum())
    assert emptied > 0 and filled > 0
    H = v.to_device(0, updatable=True)
    op = Operands(n, W, G)                                           # (M = 0: with momentum 0.5 the first step is m = g, W -= lr g, and the image kernel owns it)
    H.set_values(op.W)                                               # the handle holds W: its compaction is that of W's zero pattern
    B = dense_b(v, 128, 301, integer=True)
    assert np.array_equal(product(H, v, B, sa.F32)[0], oracle(v, W, B).astype(f32))
    H.sgd_step(op.W, op.G, op.M, lr=lr, momentum=0.5)
    assert H.step_info()["fused"] == FUSED[(key, sa.F32)]
    Wn, _ = sgd_ref(W, G, np.zeros(n, f32), lr, 0.5)
    Wd, _ = op.read()
    assert same_bits(Wd, Wn)
    was, now = (np.concatenate([(x[off:off + h * w].reshape(w, h) != 0).any(axis=1) for off, h, _ in blocks_of(v)]) for x in (W, Wn))
    assert (was & ~now).any() and (~was & now).any()
    Fh = with_values(v, Wd).to_device(0)
    for n_cols in (32, 128):
        Bn = dense_b(v, n_cols, 302 + n_cols, integer=True)
        a, b = product(H, v, Bn, sa.F32)[0], product(Fh, v, Bn, sa.F32)[0]
        assert same_bits(a, b), (key, n_cols)
        assert np.array_equal(a, oracle(v, Wd, Bn).astype(f32)), (key, n_cols)
    H.close(); Fh.close()


# ---- 5. range handle ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [sa.F32, sa.F16], ids=["f32", "f16"])
def test_range_handle_updates_its_slice(mats, dtype):
    v = mats["grid32"]
    b0, b1 = 2, 5
    ends = np.concatenate([[0], np.cumsum(v.nzcount * np.diff(v.row_part) * v.block_col_size)])
    a0, a1 = int(ends[b0]), int(ends[b1])
    H = v.to_device(0, dtype=dtype, block_row_range=(b0, b1), updatable=True)
    n = a1 - a0
    assert H.info()["nztot"] == n
    W = values(v, 23, integer=True)[a0:a1]
    G = values(v, 24, integer=True)[a0:a1]
    op = Operands(n, W, G)
    M = np.zeros(n, f32)
    for step in range(2):
        H.sgd_step(op.W, op.G, op.M, lr=0.5, momentum=0.5)
        W, M = sgd_ref(W, G, M, 0.5, 0.5)
        Wd, Md = op.read()                                           # (asserts the canaries around the three buffers)
        assert same_bits(Wd, W) and same_bits(Md, M), step
    assert H.step_info()["fused"] == 1
    B = dense_b(v, 128, 501, integer=True)
    C, _ = product(H, v, B, dtype)
    assert np.array_equal(C, oracle(v, W, B, b0, b1).astype(f32))
    with pytest.raises(ValueError):
        H.sgd_step(torch.zeros(int(v.nztot), dtype=torch.float32, device="cuda"), torch.zeros(int(v.nztot), dtype=torch.float32, device="cuda"), lr=0.5)
    H.close()


# ---- 6. capture -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [sa.F32, sa.F16], ids=["f32", "f16"])
def test_capture_from_the_first_call(mats, dtype):
    """sgd_step + spmm as one graph, the capture holding the handle's very first sgd_step (the product ran once before: its first call tunes and allocates)"""
    v = mats["padded"]
    n, nz = 128, int(v.nztot)
    B = dense_b(v, n, 601, integer=True)
    ldb = v.cols + (v.cols & 1)
    t = torch.zeros((n, ldb), dtype=torch.float64)
    t[:, :v.cols] = torch.from_numpy(np.ascontiguousarray(B.T))
    Bt = t.cuda().to(TDT[dtype]).reshape(-1)
    W0, G = values(v, 25, integer=True), values(v, 26, integer=True)
    out = {}
    for mode in ("eager", "graph"):
        H = make(v, dtype)
        W, Gd, M = (torch.from_numpy(a.copy()).cuda() for a in (W0, G, np.zeros(nz, f32)))
        Ct = torch.zeros(v.rows * n, dtype=torch.float32, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            H.spmm(Bt, Ct, n, ldb=ldb)
            torch.cuda.synchronize()
            assert H.step_info()["fused"] == -1

            def step():
                H.sgd_step(W, Gd, M, lr=0.5, momentum=0.5)
                H.spmm(Bt, Ct, n, ldb=ldb)
            if mode == "graph":
                gph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gph, stream=s):
                    step()
                torch.cuda.synchronize()
                assert np.array_equal(W.cpu().numpy(), W0)           # a capture runs nothing
            res = []
            for _ in range(3):
                gph.replay() if mode == "graph" else step()
                torch.cuda.synchronize()
                res.append((W.cpu().numpy(), Ct.cpu().numpy()))
        out[mode] = res
        H.close()
    Wr, Mr = W0, np.zeros(nz, f32)
    for i in range(3):
        Wr, Mr = sgd_ref(Wr, G, Mr, 0.5, 0.5)
        for mode in ("eager", "graph"):
            assert same_bits(out[mode][i][0], Wr), (mode, i, "W")
            assert np.array_equal(out[mode][i][1].reshape(n, v.rows).T, oracle(v, Wr, B).astype(f32)), (mode, i, "C")


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(mats):
    v = mats["jaccard"]
    n = 128
    B = dense_b(v, n, 701, integer=True)
    t = tall_groups()
    handles = {
        "plain": v.to_device(0),
        "from_csr": sa.DeviceVBS.from_csr(t, sa.BlockingEngine(tau=0.6, col_block_size=32).GetGrouping(t), 32, device=0),
        "transposed": sa.DeviceVBS.transposed_of(v, device=0),
    }
    for name, d in handles.items():
        nz = d.info()["nztot"]
        z = torch.zeros(max(nz, 1), dtype=torch.float32, device="cuda")[:nz]
        with pytest.raises(sa.SpartaError) as e:
            d.sgd_step(z, z.clone(), lr=0.5)
        assert e.value.code == sa._lib.ERR_UNSUPPORTED, name
        assert "sparta_vbs_sgd_step" in str(e.value) and "SPARTA_CREATE_UPDATABLE" in str(e.value), name
        assert d.step_info()["fused"] == -1
    for name in ("plain", "from_csr"):                              # (the same matrix: v is the VBS of t under the same grouping)
        C, Br = product(handles[name], v, B, sa.F32)
        check_close(C, v, v.mab, Br, name)
    Cba = np.zeros(16 * v.cols, f32)
    handles["transposed"].spmm_BA_host(np.ones(16 * v.rows, f32), 16, Cba, accumulate=False)
    assert np.all(np.isfinite(Cba))
    # an updatable handle: momentum without a buffer, operands of the wrong kind, a timed call inside a capture
    H = make(v, sa.F32)
    W0 = values(v, 27, integer=True)
    W, G = torch.from_numpy(W0.copy()).cuda(), torch.from_numpy(values(v, 28, integer=True)).cuda()
    with pytest.raises(sa.SpartaError) as e:
        H.sgd_step(W, G, None, lr=0.5, momentum=0.5)
    assert e.value.code == sa._lib.ERR_INVALID and "momentum" in str(e.value)
    with pytest.raises(ValueError):
        H.sgd_step(W.half(), G, lr=0.5)
    with pytest.raises(ValueError):
        H.sgd_step(W, G[:-1], lr=0.5)
    with pytest.raises(ValueError):
        H.sgd_step(W, G)                                             # no lr
    Bi = dense_b(v, n, 702, integer=True)
    C, Br = product(H, v, Bi, sa.F32)
    check_close(C, v, v.mab, Br, "after the refused calls")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    caught = []
    with torch.cuda.stream(s):
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph, stream=s):
            try:
                H.sgd_step(W, G, lr=0.5, timed=True)
            except sa.SpartaError as err:
                caught.append(err)
            H.sgd_step(W, G, lr=0.5)                                 # (the capture goes on: the refusal launched nothing)
        torch.cuda.synchronize()
        assert len(caught) == 1 and caught[0].code == sa._lib.ERR_UNSUPPORTED and "captured" in str(caught[0])
        assert np.array_equal(W.cpu().numpy(), W0)
        gph.replay()
        torch.cuda.synchronize()
    Wn, _ = sgd_ref(W0, G.cpu().numpy(), None, 0.5)
    assert same_bits(W.cpu().numpy(), Wn)
    assert np.array_equal(product(H, v, Bi, sa.F32)[0], oracle(v, Wn, Bi).astype(f32))
    assert H.sgd_step(W, G, lr=0.5, timed=True) > 0.0                # outside a capture the timed call is taken
    for h in list(handles.values()) + [H]:
        h.close()


# ---- 8. vbs_linear + VbsSGD -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("momentum", [0.5, 0.0], ids=["momentum", "plain"])
@pytest.mark.parametrize("dtype", [sa.F32, sa.BF16], ids=["f32", "bf16"])
def test_vbs_linear_with_vbs_sgd(mats, dtype, momentum, monkeypatch):
    """four training steps against torch.optim.SGD(lr=0.5, momentum=0.5 / 0) on a float64 dense parameter whose gradient is masked to the stored positions, the
    comparison and the bound (exact) of tests/test_vbs_linear_gpu.py::test_three_steps_of_sgd_with_momentum.  n = 2, x and grad_y in -1, 0, 1: |grad| <= 2,
    the momentum buffer stays below 4 and after four steps the values are multiples of 1/16 below 4 + 0.5 (2 + 3 + 3.5 + 3.75) < 16: exact in bf16
    (8 bits) -- asserted on the reference at every step, not assumed."""
    v = mats["padded"]
    n = 2
    _, rr, cc = dense_and_mask(v, v.mab)
    inside = cc >= 0
    mask = np.zeros((v.rows, v.cols))
    mask[rr[inside], cc[inside]] = 1.0
    mask = torch.from_numpy(mask)
    V = values(v, 70, integer=True)
    H = v.to_device(0, dtype=dtype, updatable=True, transposable=True)
    calls = []
    monkeypatch.setattr(H, "set_values", lambda *a, _f=H.set_values, **k: (calls.append(1), _f(*a, **k))[1])
    W = torch.from_numpy(V.copy()).cuda().requires_grad_(True)
    D = torch.from_numpy(oracle(v, V, np.eye(v.cols))).requires_grad_(True)
    monkeypatch.delenv("SPARTA_SGD_FUSE", raising=False)
    opt_w = sa.VbsSGD([(H, W)], lr=0.5, momentum=momentum)
    opt_d = torch.optim.SGD([D], lr=0.5, momentum=momentum)
    x64 = np.ascontiguousarray(np.sign(dense_b(v, n, 71, integer=True).T))
    x = torch.from_numpy(x64).cuda().to(TDT[dtype]).requires_grad_(True)
    for step in range(4):
        gy64 = np.sign(dense_x(v.rows, n, 72 + step, integer=True).T)
        opt_w.zero_grad()
        opt_d.zero_grad()
        x.grad = None
        y = vbs_linear(x, H, W)
        assert len(calls) == 1, step                                 # the first forward wrote the values; every later one finds the handle up to date
        yd = F.linear(torch.from_numpy(x64), D)
        assert np.array_equal(y.detach().cpu().numpy(), yd.detach().numpy().astype(f32)), step
        y.backward(torch.from_numpy(gy64).float().cuda())
        yd.backward(torch.from_numpy(gy64))
        gx_ref = torch.from_numpy(gy64 @ D.detach().numpy()).to(TDT[dtype]).float().numpy()       # (returned in x.dtype: the exact result rounded to it)
        assert np.array_equal(x.grad.float().cpu().numpy(), gx_ref), step
        D.grad *= mask
        gw = W.grad.cpu().numpy()
        assert np.array_equal(gw[inside], D.grad.numpy()[rr[inside], cc[inside]].astype(f32)) and not gw[~inside].any(), step
        opt_w.step()
        opt_d.step()
        assert H.step_info()["fused"] == 1     # (whichever form the step took, the handle is up to date afterwards)
        cur = D.detach().numpy()
        assert np.array_equal(rounded(cur, dtype).astype(np.float64), cur), step      # every value of the reference is exact in the handle's type
        assert np.array_equal(W.detach().cpu().numpy()[inside], cur[rr[inside], cc[inside]].astype(f32)), step
    assert np.any(cur != np.round(cur))                               # the steps did move the values, to fractions too
    y = vbs_linear(x, H, W)
    assert len(calls) == 1
    assert np.array_equal(y.detach().cpu().numpy(), F.linear(torch.from_numpy(x64), D).detach().numpy().astype(f32))
    # a backward whose forward saw the values before the step
    y.backward(torch.ones_like(y), retain_graph=True)
    opt_w.step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward(torch.ones_like(y))
    # ... and another set_values of the caller's own drops the record: the next forward writes W again
    H.set_values(torch.zeros_like(W))
    n_calls = len(calls)
    y = vbs_linear(x, H, W)
    assert len(calls) == n_calls + 1
    assert np.array_equal(y.detach().cpu().numpy(), oracle(v, rounded(W.detach().cpu().numpy(), dtype), x64.T).T.astype(f32))
    H.close()
