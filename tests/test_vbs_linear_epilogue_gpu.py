"""vbs_linear(..., bias=, activation=, out_dtype=) on the GPU: the layer with its epilogue (sparta_amd/autograd.py, sparta_amd/epilogue.py, k_epilogue.hip).

Plumbing: y and the three gradients are, bit for bit, what epilogue_fwd / epilogue_bwd and the handle's spmm / spmm_t / sddmm give when called directly.
Against today's layer: for "none" and "relu" the pinned select and the nearest-even rounding make the dz of both paths the same bits, so y, x.grad and
W.grad equal act(vbs_linear(x, H, W) + bias).to(out_dtype) differentiated by torch bit for bit; bias.grad, an fp64 sum rounded once on both sides, lies
within 2^-23 |ref| + n 2^-52 sum|dz| of torch's float64 row sum of that dz.  The matrices and helpers are those of tests/test_vbs_linear_gpu.py."""
import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd.autograd import vbs_linear

torch = pytest.importorskip("torch")

from test_set_values_gpu import TDT, DT_ID, values  # noqa: E402
from test_vbs_linear_gpu import mats, dev, handle, operands  # noqa: E402,F401  (mats: the module fixture)
from test_spmm_t_gpu import dense_x  # noqa: E402
from test_set_values_gpu import dense_b  # noqa: E402

pytestmark = pytest.mark.gpu

F = torch.nn.functional
HANDLES = [("grid8", sa.F32), ("padded", sa.F32), ("jaccard", sa.F16), ("padded", sa.BF16)]
HANDLE_IDS = ["%s-%s" % (k, DT_ID[dt]) for k, dt in HANDLES]
ACTS = ["none", "relu", "gelu"]
TORCH_ACT = {"none": lambda t: t, "relu": torch.relu, "gelu": F.gelu}


def bits(t):
    t = t.detach().contiguous()
    return (t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)).cpu().numpy()


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def setup(v, dtype, n, seed):
    """x, grad_y in `gy_dtype` to be chosen by the caller (float32 here), W and bias with uniform data: nothing is exact, everything is compared in bits"""
    x, gy = operands(v, dtype, n, seed, integer=False)
    W = dev(values(v, seed + 2, integer=False))
    bias = dev(np.random.default_rng(seed + 3).uniform(-1, 1, v.rows).astype(np.float32))
    return x, gy, W, bias


# ---- 1. plumbing ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("key,dtype", HANDLES, ids=HANDLE_IDS)
def test_layer_is_the_kernels_called_directly(mats, key, dtype, n, act):
    v = mats[key]
    H = handle(v, dtype)
    x, gy, W, bias = setup(v, dtype, n, 300)
    for out_dtype in {torch.float32, TDT[dtype]}:
        gyo = gy.to(out_dtype)
        xg, Wg, bg = x.clone().requires_grad_(True), W.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        y = vbs_linear(xg, H, Wg, bias=bg, activation=act, out_dtype=out_dtype)
        assert type(y.grad_fn).__name__ == "_VbsLinearEpilogueBackward"
        y.backward(gyo)
        z = torch.empty((n, v.rows), dtype=torch.float32, device="cuda")
        H.spmm(x, z, n, accumulate=False)
        assert same(y, sa.epilogue_fwd(z, bias, act, out_dtype)), (out_dtype, "y")
        dz, db = sa.epilogue_bwd(gyo, z, bias, act, x.dtype, True)
        gx = torch.empty((n, v.cols), dtype=torch.float32, device="cuda")
        H.spmm_t(dz, gx, n, accumulate=False)
        gv = torch.empty(H._nztot(), dtype=torch.float32, device="cuda")
        H.sddmm(dz, x, gv, n, accumulate=False)
        assert dz.dtype == x.dtype and same(xg.grad, gx.to(x.dtype)) and same(Wg.grad, gv) and same(bg.grad, db), out_dtype
        assert bg.grad.shape == (v.rows,) and bg.grad.dtype == torch.float32
    H.close()


# ---- 2. against today's layer + torch ops ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("key,dtype", HANDLES, ids=HANDLE_IDS)
def test_against_todays_layer_with_torch_ops(mats, key, dtype, n, act):
    v = mats[key]
    H, H0 = handle(v, dtype), handle(v, dtype)
    x, gy, W, bias = setup(v, dtype, n, 400)
    for out_dtype in {torch.float32, TDT[dtype]}:
        gyo = gy.to(out_dtype)
        xg, Wg, bg = x.clone().requires_grad_(True), W.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        y = vbs_linear(xg, H, Wg, bias=bg, activation=act, out_dtype=out_dtype)
        y.backward(gyo)
        x0, W0, b0 = x.clone().requires_grad_(True), W.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        z0 = vbs_linear(x0, H0, W0)
        z0.retain_grad()
        y0 = TORCH_ACT[act](z0 + b0).to(out_dtype)
        y0.backward(gyo)
        assert same(y, y0) and same(xg.grad, x0.grad) and same(Wg.grad, W0.grad), (out_dtype, act)
        dz64 = z0.grad.double()                                          # the dz of the reference, before the old layer rounds it to the handle's type
        ref, mag = dz64.sum(0).cpu().numpy(), dz64.abs().sum(0).cpu().numpy()
        got = bg.grad.double().cpu().numpy()
        assert np.all(np.abs(got - ref) <= 2.0 ** -23 * np.abs(ref) + n * 2.0 ** -52 * mag), (out_dtype, act, np.abs(got - ref).max())
        if act == "relu":
            assert (z0.grad == 0).any() and (z0.grad != 0).any()             # (the mask is at work)
    H.close(); H0.close()


# ---- 3. argument combinations ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [sa.F32, sa.F16], ids=["f32", "f16"])
def test_argument_combinations(mats, dtype, monkeypatch):
    v = mats["padded"]
    n = 33
    H = handle(v, dtype)
    x, gy, W, bias = setup(v, dtype, n, 500)
    # an activation without a bias
    xg, Wg = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    y = vbs_linear(xg, H, Wg, activation="relu")
    y.backward(gy)
    x0, W0 = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    y0 = torch.relu(vbs_linear(x0, H, W0))
    y0.backward(gy)
    assert same(y, y0) and same(xg.grad, x0.grad) and same(Wg.grad, W0.grad)
    # out_dtype alone
    y16 = vbs_linear(x, H, W, out_dtype=torch.bfloat16)
    assert same(y16, vbs_linear(x, H, W).to(torch.bfloat16))
    # a bias alone: one launch, in place on z
    seen = []
    monkeypatch.setattr(sa.epilogue, "epilogue_fwd", lambda z, *a, _f=sa.epilogue.epilogue_fwd, **k: (seen.append(k.get("out") is z), _f(z, *a, **k))[1])
    yb = vbs_linear(x, H, W, bias=bias)
    assert seen == [True] and same(yb, vbs_linear(x, H, W) + bias)
    del seen[:]
    vbs_linear(x, H, W, bias=bias, activation="relu")
    vbs_linear(x, H, W, bias=bias, out_dtype=torch.float16)
    assert seen == [False, False]
    monkeypatch.undo()
    # only the bias requires grad: neither backward product runs
    calls = []
    for name in ("spmm_t", "sddmm"):
        monkeypatch.setattr(H, name, lambda *a, _f=getattr(H, name), _n=name, **k: (calls.append(_n), _f(*a, **k))[1])
    bg = bias.clone().requires_grad_(True)
    vbs_linear(x, H, W, bias=bg, activation="relu").backward(gy)
    z = vbs_linear(x, H, W)
    assert calls == [] and same(bg.grad, sa.epilogue_bwd(gy, z, bias, "relu", x.dtype, True)[1])
    # ... and without a bias gradient each product alone, as in the plain layer
    xg = x.clone().requires_grad_(True)
    vbs_linear(xg, H, W, bias=bias, activation="relu").backward(gy)
    assert calls == ["spmm_t"] and xg.grad.dtype == x.dtype
    del calls[:]
    Wg = W.clone().requires_grad_(True)
    vbs_linear(x, H, Wg, bias=bias, activation="gelu", out_dtype=TDT[dtype]).backward(gy.to(TDT[dtype]))
    assert calls == ["sddmm"]
    H.close()


# ---- 4. defaults -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,dtype", HANDLES, ids=HANDLE_IDS)
def test_defaults_are_the_old_call(mats, key, dtype, monkeypatch):
    v = mats[key]
    H = handle(v, dtype)
    x, gy, W, _ = setup(v, dtype, 33, 600)
    launched = []
    monkeypatch.setattr(sa.epilogue, "epilogue_fwd", lambda *a, **k: launched.append("fwd"))
    monkeypatch.setattr(sa.epilogue, "epilogue_bwd", lambda *a, **k: launched.append("bwd"))
    res = []
    for kw in ({}, dict(bias=None, activation="none", out_dtype=None)):
        xg, Wg = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
        y = vbs_linear(xg, H, Wg, **kw)
        assert type(y.grad_fn).__name__ == "_VbsLinearBackward" and y.dtype == torch.float32
        y.backward(gy)
        res.append((y, xg.grad, Wg.grad))
    assert all(same(a, b) for a, b in zip(*res)) and launched == []
    assert same(vbs_linear(x, H, W, True), res[0][0])                    # `refresh` keeps its place
    H.close()


# ---- 5. a training step ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [sa.F32, sa.F16], ids=["f32", "f16"])
def test_three_steps_of_vbs_sgd_with_bias_and_relu(mats, dtype, monkeypatch):
    """the same loop twice -- the layer with its epilogue / today's layer with torch ops on top -- on two handles, VbsSGD on the values and torch's SGD on the
    bias: y, every gradient and every parameter agree bit for bit at every step (n = 2: a bias gradient is ONE addition, rounded once in fp32 as in fp64), and
    the stale-values record still works: the first forward writes the values, every later one finds the handle up to date"""
    v = mats["padded"]
    n = 2
    monkeypatch.delenv("SPARTA_SGD_FUSE", raising=False)
    V = values(v, 70, integer=True)
    b0 = np.random.default_rng(7).integers(-2, 3, v.rows).astype(np.float32)
    x = dev(np.ascontiguousarray(np.sign(dense_b(v, n, 71, integer=True).T)), dtype)
    sides = []
    for fused in (True, False):
        H = handle(v, dtype)
        calls = []
        monkeypatch.setattr(H, "set_values", lambda *a, _f=H.set_values, _c=calls, **k: (_c.append(1), _f(*a, **k))[1])
        W, b = dev(V).requires_grad_(True), dev(b0).requires_grad_(True)
        sides.append(dict(H=H, W=W, b=b, calls=calls, opt=sa.VbsSGD([(H, W)], lr=0.5, momentum=0.5), opt_b=torch.optim.SGD([b], lr=0.25), fused=fused))
    for step in range(3):
        gy = dev(np.sign(dense_x(v.rows, n, 72 + step, integer=True).T))
        out = []
        for s in sides:
            s["opt"].zero_grad(); s["opt_b"].zero_grad()
            xg = x.clone().requires_grad_(True)
            if s["fused"]:
                y = vbs_linear(xg, s["H"], s["W"], bias=s["b"], activation="relu")
            else:
                y = torch.relu(vbs_linear(xg, s["H"], s["W"]) + s["b"])
            assert len(s["calls"]) == 1, (step, s["fused"])               # set_values is skipped from the second step on
            y.backward(gy)
            out.append((y, xg.grad, s["W"].grad.clone(), s["b"].grad.clone()))
            s["opt"].step(); s["opt_b"].step()
            out[-1] += (s["W"].detach().clone(), s["b"].detach().clone())
        assert all(same(a, b_) for a, b_ in zip(*out)), step
        assert out[0][0].count_nonzero() > 0 and (out[0][0] == 0).any() and out[0][3].count_nonzero() > 0
    for s in sides:
        s["H"].close()
