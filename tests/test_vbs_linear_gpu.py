"""sparta_amd.autograd.vbs_linear on the GPU: the layer as a PyTorch user drives it.

Reference: float64 torch.nn.functional.linear on the dense matrix of the values as the handle stores them (rounded to its type), built from the VBS arrays --
and, in test_against_the_original_matrix, from the CSR the VBS was made from, through get_permutation.  Small-integer data are exact in every type and must
match bit for bit (a 16-bit grad_x is returned in x.dtype: the exact fp32 result rounded to it); uniform data within 1e-5 * sum|a||b| per element, the
project's bound for the MFMA kernels, a 16-bit grad_x through the rounding interval.  The state cases of tests/test_vbs_linear_host.py run again on a real
handle.  The 16-bit combinations of the grid all have even rows and cols, so nothing skips; the refusal of odd ones is asserted on the 517-column matrix."""
import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd.autograd import vbs_linear

torch = pytest.importorskip("torch")

from test_set_values_gpu import TDT, DT_ID, build_mats, tall_groups, vbr_of, values, oracle as fwd_oracle, dense_b, rounded  # noqa: E402
from test_sddmm_gpu import oracle as sddmm_oracle  # noqa: E402
from test_spmm_t_gpu import oracle as t_oracle, dense_x, dense_and_mask  # noqa: E402

pytestmark = pytest.mark.gpu

F = torch.nn.functional


@pytest.fixture(scope="module")
def mats():
    return build_mats()


_POSITIONS = {}


def positions(key, v):
    """(row, column) of every stored position of mats[key], column -1 past cols; computed once per matrix"""
    if key not in _POSITIONS:
        _POSITIONS[key] = dense_and_mask(v, v.mab)[1:]
    return _POSITIONS[key]


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.float() if dtype is None else t.to(TDT[dtype])


def host(t):
    return t.detach().float().cpu().numpy()


def handle(v, dtype):
    return v.to_device(0, dtype=dtype, updatable=True, transposable=True)


def check_linear(key, v, dtype, V, x, gy, y, gx, gv, integer, what=""):
    """y, grad_x, grad_values of the device (tensors, or None where not asked for) against float64 F.linear on the dense matrix of the rounded V; x and gy
    are the device tensors the layer got (gy float32: the layer rounds it to the handle's type)"""
    tdt = TDT[dtype]
    rr, cc = positions(key, v)
    A = fwd_oracle(v, rounded(V, dtype), np.eye(v.cols))
    xr, gyr = x.detach().double().cpu(), gy.to(tdt).double().cpu()
    At, xt = torch.from_numpy(A).requires_grad_(True), xr.clone().requires_grad_(True)
    yt = F.linear(xt, At)
    yt.backward(gyr)
    absA, absx, absg = np.abs(A), np.abs(xr.numpy()), np.abs(gyr.numpy())
    inside = cc >= 0
    gv_ref = np.where(inside, At.grad.numpy()[rr, np.maximum(cc, 0)], 0.0)
    gx_ref = xt.grad.numpy()
    if integer:
        assert np.array_equal(host(y), yt.detach().numpy().astype(np.float32)), (what, "y")
        if gx is not None:
            assert np.array_equal(host(gx), torch.from_numpy(gx_ref).to(tdt).float().numpy()), (what, "grad_x")
        if gv is not None:
            assert np.array_equal(host(gv), gv_ref.astype(np.float32)), (what, "grad_values")
        return
    assert np.all(np.abs(host(y) - yt.detach().numpy()) <= 1e-5 * (absx @ absA.T) + 1e-30), (what, "y")
    if gx is not None:
        b = 1e-5 * (absg @ absA)
        if dtype == sa.F32:
            assert np.all(np.abs(host(gx) - gx_ref) <= b + 1e-30), (what, "grad_x")
        else:                                                         # (rounded to x.dtype on return: compared through that rounding)
            lo, hi = (torch.from_numpy(gx_ref + s * b).to(tdt).float().numpy() for s in (-1, 1))
            assert np.all((host(gx) >= lo) & (host(gx) <= hi)), (what, "grad_x")
    if gv is not None:
        gv_bound = np.where(inside, (absg.T @ absx)[rr, np.maximum(cc, 0)], 0.0)
        assert np.all(np.abs(host(gv) - gv_ref) <= 1e-5 * gv_bound + 1e-30), (what, "grad_values")


def operands(v, dtype, n, seed, integer):
    """x (n, cols) in the handle's type and grad_y (n, rows) float32, on the device"""
    x = dev(dense_b(v, n, seed, integer).T, dtype)
    gy = dev(dense_x(v.rows, n, seed + 1, integer).T)
    return x, gy


GRID = [("grid8", sa.F32), ("grid32", sa.F32), ("padded", sa.F32), ("jaccard", sa.F16), ("jaccard", sa.BF16), ("padded", sa.F16), ("padded", sa.BF16)]
GRID_IDS = ["%s-%s" % (k, DT_ID[dt]) for k, dt in GRID]


@pytest.mark.parametrize("n", [1, 24, 130])
@pytest.mark.parametrize("key,dtype", GRID, ids=GRID_IDS)
def test_grid_against_dense_linear(mats, key, dtype, n):
    """n = 1, a width below one slab, and 130 = one 128-column slab + a tail of 2"""
    v = mats[key]
    assert dtype == sa.F32 or not ((v.rows | v.cols) & 1)
    H = handle(v, dtype)
    for integer in (True, False):
        V = values(v, 30 + integer, integer)
        W = dev(V).requires_grad_(True)
        x, gy = operands(v, dtype, n, 31, integer)
        x.requires_grad_(True)
        y = vbs_linear(x, H, W)
        assert y.shape == (n, v.rows) and y.dtype == torch.float32
        y.backward(gy)
        assert x.grad.dtype == x.dtype and x.grad.shape == x.shape and W.grad.dtype == torch.float32 and W.grad.shape == W.shape
        torch.cuda.synchronize()
        check_linear(key, v, dtype, V, x, gy, y, x.grad, W.grad, integer, "integer" if integer else "uniform")
    H.close()


def test_16bit_handle_with_odd_cols_is_refused(mats):
    v = mats["grid32"]
    assert v.cols & 1
    H = handle(v, sa.F16)
    x = torch.zeros((4, v.cols), dtype=torch.float16, device="cuda")
    W = torch.zeros(int(v.nztot), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="even rows and cols"):
        vbs_linear(x, H, W)
    H.close()


ORIGINAL = [("grid32", sa.F32), ("jaccard", sa.BF16)]


@pytest.mark.parametrize("key,dtype", ORIGINAL, ids=["%s-%s" % (k, DT_ID[dt]) for k, dt in ORIGINAL])
def test_against_the_original_matrix(mats, key, dtype):
    """the dense M of the CSR itself (rowptr / colidx / vals, integer values), rows mapped through get_permutation(grouping): nothing here is rebuilt from the VBS arrays"""
    if key == "grid32":
        m = sa.gen.uniform_random(300, 517, 9000, seed=41)
        g = np.arange(m.rows, dtype=np.int64) // 16
    else:
        m = tall_groups()
        g = sa.BlockingEngine(tau=0.6, col_block_size=32).GetGrouping(m)
    vals = np.random.default_rng(50).integers(1, 5, len(m.colidx)).astype(np.float32)
    vals[::3] *= -1
    m = sa.CSR(m.rows, m.cols, m.rowptr, m.colidx, vals)
    v = vbr_of(m, g, 32)
    assert all(np.array_equal(getattr(v, a), getattr(mats[key], a)) for a in ("row_part", "nzcount", "jab"))      # the module's matrix, other values
    perm = sa.get_permutation(g)
    assert sorted(perm) == list(range(m.rows))
    if key == "jaccard":
        assert not np.array_equal(perm, np.arange(m.rows))
    ri = np.repeat(np.arange(m.rows), np.diff(m.rowptr))
    M = np.zeros((m.rows, m.cols))
    M[ri, m.colidx] = vals
    n = 24
    H = handle(v, dtype)
    W = dev(v.mab).requires_grad_(True)
    x, gy = operands(v, dtype, n, 51, integer=True)
    y = vbs_linear(x, H, W)
    y.backward(gy)
    torch.cuda.synchronize()
    x64, gy64 = x.double().cpu().numpy(), gy.double().cpu().numpy()
    assert np.array_equal(host(y), (x64 @ M.T)[:, perm].astype(np.float32))
    # the gradient of M, dense, in the CSR's row order: grad_y of original row perm[r] is column r of gy
    gyo = np.zeros_like(gy64)
    gyo[:, perm] = gy64
    gM = gyo.T @ x64
    rr, cc = positions(key, v)
    at = np.full((m.rows, m.cols), -1, np.int64)                      # stored position of every (original row, column)
    inside = cc >= 0
    at[perm[rr[inside]], cc[inside]] = np.flatnonzero(inside)
    p = at[ri, m.colidx]
    assert np.all(p >= 0) and len(set(p)) == len(p)
    assert np.array_equal(v.mab[p], vals)
    assert np.array_equal(host(W.grad)[p], gM[ri, m.colidx].astype(np.float32))
    H.close()


# ---- the state cases of tests/test_vbs_linear_host.py on a real handle ---------------------------------------------------------------------
STATE = [sa.F32, sa.F16]
STATE_IDS = ["f32", "f16"]


class Case:
    """the small padded matrix, integer data: every reference is exact"""

    def __init__(self, mats, dtype, n=8):
        self.v, self.dtype, self.n = mats["padded"], dtype, n
        self.H = handle(self.v, dtype)
        self.x, self.gy = operands(self.v, dtype, n, 61, integer=True)
        self.x64, self.gy64 = self.x.double().cpu().numpy(), self.gy.double().cpu().numpy()

    def V(self, seed):
        return values(self.v, seed, integer=True)

    def y_ref(self, V):
        return fwd_oracle(self.v, V, self.x64.T).T.astype(np.float32)

    def gx_ref(self, V, gy64=None):
        g = t_oracle(self.v, V, (self.gy64 if gy64 is None else gy64).T).T
        return torch.from_numpy(g).to(TDT[self.dtype]).float().numpy()

    def gv_ref(self, gy64=None):
        return sddmm_oracle(self.v, (self.gy64 if gy64 is None else gy64).T, self.x64.T).astype(np.float32)


@pytest.mark.parametrize("dtype", STATE, ids=STATE_IDS)
def test_same_values_twice_and_in_place_update(mats, dtype):
    c = Case(mats, dtype)
    V1, V2 = c.V(1), c.V(2)
    W = dev(V1).requires_grad_(True)
    y1, y2 = vbs_linear(c.x, c.H, W), vbs_linear(c.x, c.H, W)
    assert np.array_equal(host(y1), c.y_ref(V1)) and np.array_equal(host(y2), c.y_ref(V1))
    with torch.no_grad():
        W.copy_(dev(V2))
    assert np.array_equal(host(vbs_linear(c.x, c.H, W)), c.y_ref(V2))
    assert not np.array_equal(c.y_ref(V1), c.y_ref(V2))
    c.H.close()


@pytest.mark.parametrize("dtype", STATE, ids=STATE_IDS)
def test_set_values_on_the_handle_between_two_forwards(mats, dtype):
    c = Case(mats, dtype)
    V1, other = c.V(1), c.V(3)
    W = dev(V1).requires_grad_(True)
    assert np.array_equal(host(vbs_linear(c.x, c.H, W)), c.y_ref(V1))
    c.H.set_values(dev(other))
    assert np.array_equal(host(vbs_linear(c.x, c.H, W)), c.y_ref(V1))
    c.H.set_values_host(other)
    assert np.array_equal(host(vbs_linear(c.x, c.H, W)), c.y_ref(V1))
    c.H.close()


@pytest.mark.parametrize("dtype", STATE, ids=STATE_IDS)
def test_another_tensor_with_the_same_address_and_version(mats, dtype):
    """two tensor objects on one storage with a version counter each, as in the host test"""
    c = Case(mats, dtype)
    V1, V2 = c.V(1), c.V(4)
    nz = int(c.v.nztot)
    storage = torch.zeros(nz, dtype=torch.float32, device="cuda").untyped_storage()
    W1 = torch.empty(0, dtype=torch.float32, device="cuda").set_(storage, 0, (nz,))
    W1.copy_(dev(V1))
    W1.requires_grad_(True)
    assert np.array_equal(host(vbs_linear(c.x, c.H, W1)), c.y_ref(V1))
    W2 = torch.empty(0, dtype=torch.float32, device="cuda").set_(storage, 0, (nz,))
    W2.copy_(dev(V2))
    W2.requires_grad_(True)
    assert W2 is not W1 and W2.data_ptr() == W1.data_ptr() and W2._version == W1._version
    assert np.array_equal(host(vbs_linear(c.x, c.H, W2)), c.y_ref(V2))
    c.H.close()


@pytest.mark.parametrize("dtype", STATE, ids=STATE_IDS)
def test_new_tensor_after_the_old_one_was_freed(mats, dtype):
    """del W, then a tensor of the same size: the caching allocator may hand the address out again, with a fresh version counter"""
    c = Case(mats, dtype)
    V1, V2 = c.V(1), c.V(5)
    W = dev(V1).requires_grad_(True)
    y = vbs_linear(c.x, c.H, W)
    assert np.array_equal(host(y), c.y_ref(V1))
    old = (W.data_ptr(), W._version)
    del W, y
    W = dev(V2).requires_grad_(True)
    reused = "data_ptr %s, version %s" % ("reused" if W.data_ptr() == old[0] else "not reused", "equal" if W._version == old[1] else "different")
    assert np.array_equal(host(vbs_linear(c.x, c.H, W)), c.y_ref(V2)), reused
    c.H.close()


@pytest.mark.parametrize("dtype", STATE, ids=STATE_IDS)
def test_refresh_after_a_write_the_version_counter_does_not_see(mats, dtype):
    c = Case(mats, dtype)
    V1, V2, V3 = c.V(1), c.V(6), c.V(7)
    W = dev(V1).requires_grad_(True)
    vbs_linear(c.x, c.H, W)
    version = W._version
    W.data.copy_(dev(V2))
    assert W._version == version
    assert np.array_equal(host(vbs_linear(c.x, c.H, W, refresh=True)), c.y_ref(V2))
    W.data -= dev(V2 - V3)                                            # the old SGD idiom
    assert W._version == version
    assert np.array_equal(host(vbs_linear(c.x, c.H, W, True)), c.y_ref(V3))
    c.H.close()


@pytest.mark.parametrize("dtype", STATE, ids=STATE_IDS)
def test_backward_of_an_earlier_forward_after_the_handle_moved_on(mats, dtype):
    c = Case(mats, dtype)
    V1, V2 = c.V(1), c.V(8)
    W1, W2 = dev(V1).requires_grad_(True), dev(V2).requires_grad_(True)
    x = c.x.clone().requires_grad_(True)
    gy2_64 = dense_x(c.v.rows, c.n, 63, integer=True).T
    y1 = vbs_linear(x, c.H, W1)
    y2 = vbs_linear(x, c.H, W2)
    assert np.array_equal(host(y2), c.y_ref(V2))
    y1.backward(c.gy)
    assert np.array_equal(host(x.grad), c.gx_ref(V1)) and np.array_equal(host(W1.grad), c.gv_ref()) and W2.grad is None
    assert not np.array_equal(c.gx_ref(V1), c.gx_ref(V2))
    x.grad = None
    y2.backward(dev(gy2_64))                                          # the second graph, after the handle went back to W1 for the first
    assert np.array_equal(host(x.grad), c.gx_ref(V2, gy2_64)) and np.array_equal(host(W2.grad), c.gv_ref(gy2_64))
    assert np.array_equal(host(vbs_linear(x, c.H, W1)), c.y_ref(V1))
    # and a set_values of the caller's own between forward and backward
    x.grad = None
    y = vbs_linear(x, c.H, W1)
    c.H.set_values(dev(V2))
    y.backward(c.gy)
    assert np.array_equal(host(x.grad), c.gx_ref(V1))
    c.H.close()


@pytest.mark.parametrize("dtype", STATE, ids=STATE_IDS)
def test_in_place_change_between_forward_and_backward_raises(mats, dtype):
    c = Case(mats, dtype)
    W = dev(c.V(1)).requires_grad_(True)
    x = c.x.clone().requires_grad_(True)
    y = vbs_linear(x, c.H, W)
    with torch.no_grad():
        W += 1
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward(c.gy)
    c.H.close()


@pytest.mark.parametrize("dtype", STATE, ids=STATE_IDS)
def test_only_one_input_requires_grad(mats, dtype, monkeypatch):
    c = Case(mats, dtype)
    V1 = c.V(1)
    calls = []
    for name in ("spmm_t", "sddmm"):
        monkeypatch.setattr(c.H, name, lambda *a, _f=getattr(c.H, name), _n=name, **k: (calls.append(_n), _f(*a, **k))[1])
    x = c.x.clone().requires_grad_(True)
    W = dev(V1)
    vbs_linear(x, c.H, W).backward(c.gy)
    assert np.array_equal(host(x.grad), c.gx_ref(V1)) and W.grad is None and calls == ["spmm_t"]
    del calls[:]
    W.requires_grad_(True)
    vbs_linear(c.x, c.H, W).backward(c.gy)
    assert np.array_equal(host(W.grad), c.gv_ref()) and c.x.grad is None and calls == ["sddmm"]
    c.H.close()


@pytest.mark.parametrize("dtype", STATE, ids=STATE_IDS)
def test_expanded_and_non_contiguous_grad_y(mats, dtype):
    c = Case(mats, dtype)
    V1 = c.V(1)
    W = dev(V1).requires_grad_(True)
    x = c.x.clone().requires_grad_(True)
    ones = np.ones((c.n, c.v.rows))
    vbs_linear(x, c.H, W).sum().backward()                            # grad_y: a stride-0 expansion of one element
    assert np.array_equal(host(x.grad), c.gx_ref(V1, ones)) and np.array_equal(host(W.grad), c.gv_ref(ones))
    x.grad = W.grad = None
    g = dev(c.gy64.T).t()                                             # (n, rows) with strides (1, n)
    assert not g.is_contiguous()
    vbs_linear(x, c.H, W).backward(g)
    assert np.array_equal(host(x.grad), c.gx_ref(V1)) and np.array_equal(host(W.grad), c.gv_ref())
    x.grad = W.grad = None
    vbs_linear(x, c.H, W).t().contiguous().backward(g.t())            # autograd hands in the transposed view of a contiguous (rows, n) tensor
    assert np.array_equal(host(x.grad), c.gx_ref(V1)) and np.array_equal(host(W.grad), c.gv_ref())
    c.H.close()


@pytest.mark.parametrize("dtype", STATE, ids=STATE_IDS)
def test_gradients_accumulate_over_two_passes_before_one_update(mats, dtype):
    c = Case(mats, dtype)
    V1 = c.V(1)
    W = dev(V1).requires_grad_(True)
    gy2_64 = dense_x(c.v.rows, c.n, 64, integer=True).T
    vbs_linear(c.x, c.H, W).backward(c.gy)
    vbs_linear(c.x, c.H, W).backward(dev(gy2_64))
    total = c.gv_ref().astype(np.float64) + c.gv_ref(gy2_64)
    assert np.array_equal(host(W.grad), total.astype(np.float32))
    with torch.no_grad():
        W -= torch.sign(W.grad)                                       # (the values stay small integers)
    V2 = (V1 - np.sign(total)).astype(np.float32)
    assert np.array_equal(host(vbs_linear(c.x, c.H, W)), c.y_ref(V2))
    c.H.close()


OPT = [("grid32", sa.F32), ("jaccard", sa.F16)]


@pytest.mark.parametrize("key,dtype", OPT, ids=["%s-%s" % (k, DT_ID[dt]) for k, dt in OPT])
def test_three_steps_of_sgd_with_momentum(mats, key, dtype):
    """torch.optim.SGD(lr=0.5, momentum=0.5) on W against the same optimizer on a float64 dense parameter whose gradient is masked to the stored positions.
    x in -4 .. 4 at n = 8 and grad_y in -1, 0, 1: |grad| <= 32, and after three steps the values are multiples of 1/8 below 4 + 16 + 24 + 28 = 72, exact in
    f16 (11 bits: multiples of 1/8 below 256) -- asserted on the reference at every step, not assumed; the products, sums of <= 700 multiples of 1/8 below
    4 * 72, are exact in fp32."""
    v = mats[key]
    n = 8
    rr, cc = positions(key, v)
    inside = cc >= 0
    mask = np.zeros((v.rows, v.cols))
    mask[rr[inside], cc[inside]] = 1.0
    mask = torch.from_numpy(mask)
    V = values(v, 70, integer=True)
    H = handle(v, dtype)
    W = dev(V).requires_grad_(True)
    D = torch.from_numpy(fwd_oracle(v, V, np.eye(v.cols))).requires_grad_(True)
    opt_w = torch.optim.SGD([W], lr=0.5, momentum=0.5)
    opt_d = torch.optim.SGD([D], lr=0.5, momentum=0.5)
    x64 = dense_b(v, n, 71, integer=True).T.copy()
    x = dev(x64, dtype)
    for step in range(3):
        gy64 = np.sign(dense_x(v.rows, n, 72 + step, integer=True).T)
        opt_w.zero_grad()
        opt_d.zero_grad()
        y = vbs_linear(x, H, W)
        yd = F.linear(torch.from_numpy(x64), D)
        assert np.array_equal(host(y), yd.detach().numpy().astype(np.float32)), step
        y.backward(dev(gy64))
        yd.backward(torch.from_numpy(gy64))
        D.grad *= mask
        assert np.array_equal(host(W.grad)[inside], D.grad.numpy()[rr[inside], cc[inside]].astype(np.float32)), step
        assert not host(W.grad)[~inside].any(), step
        opt_w.step()
        opt_d.step()
        cur = D.detach().numpy()
        assert np.array_equal(rounded(cur, dtype).astype(np.float64), cur), step      # every value of the reference is exact in the handle's type
        assert np.array_equal(host(W)[inside], cur[rr[inside], cc[inside]].astype(np.float32)), step
    assert np.abs(cur).max() > 8 and np.any(cur != np.round(cur))    # the steps did move the values, to fractions too
    y = vbs_linear(x, H, W)
    assert np.array_equal(host(y), F.linear(torch.from_numpy(x64), D).detach().numpy().astype(np.float32))
    H.close()


@pytest.mark.parametrize("dtype", STATE, ids=STATE_IDS)
def test_two_handles_one_tensor(mats, dtype):
    v = mats["jaccard"]
    n = 24
    H1, H2 = handle(v, dtype), handle(v, dtype)
    x, gy = operands(v, dtype, n, 81, integer=False)
    V = values(v, 80, integer=False)
    W = dev(V).requires_grad_(True)
    for step in range(2):
        out = []
        for H in (H1, H2):
            xh = x.clone().requires_grad_(True)
            W.grad = None
            y = vbs_linear(xh, H, W)
            y.backward(gy)
            out.append((y.detach(), xh.grad, W.grad))
        torch.cuda.synchronize()
        for a, b in zip(*out):
            assert torch.equal(a, b), step
        check_linear("jaccard", v, dtype, host(W), x, gy, *out[1], integer=False, what=step)
        with torch.no_grad():
            W -= 0.25 * W.grad
    H1.close(); H2.close()


# ---- graph capture: last in the file --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", STATE, ids=STATE_IDS)
def test_graph_capture(mats, dtype):
    """(1) forward, backward and W -= W.grad captured after an eager pass on a side stream: two replays after x.copy_(), one after W.copy_() from outside the
    graph.  (2) forward alone, captured after an eager forward with no update in between: a replay after W.copy_() multiplies with the new values.
    Every check stands before the next device work of the test: a failed one ends it."""
    c = Case(mats, dtype)
    v, n = c.v, c.n
    cur = c.V(90).astype(np.float64)
    W = dev(cur).requires_grad_(True)
    x = c.x.clone().requires_grad_(True)
    gy = dev(np.sign(c.gy64))
    gy64 = gy.double().cpu().numpy()

    def step():
        y = vbs_linear(x, c.H, W)
        y.backward(gy)
        with torch.no_grad():
            W.sub_(W.grad)
        return y

    def expect(x64):
        """what one step gives from `cur`: y, grad_x, and the values after it"""
        y = fwd_oracle(v, cur, x64.T).T.astype(np.float32)
        gx = torch.from_numpy(t_oracle(v, cur, gy64.T).T).to(TDT[dtype]).float().numpy()
        return y, gx, cur - sddmm_oracle(v, gy64.T, x64.T)

    s = torch.cuda.Stream()
    torch.cuda.synchronize()                                          # (the operands were made on the default stream)
    with torch.cuda.stream(s):
        y = step()                                                    # eager, once (tuning, work lists, scratch)
        torch.cuda.synchronize()
        ey, egx, cur = expect(c.x64)
        assert np.array_equal(host(y), ey) and np.array_equal(host(x.grad), egx) and np.array_equal(host(W), cur.astype(np.float32)), "eager pass"
        x.grad = W.grad = None
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph, stream=s):
            y = step()
        for i, seed in enumerate((91, 92, 93)):
            x64 = dense_b(v, n, seed, integer=True).T.copy()
            with torch.no_grad():
                x.copy_(dev(x64, dtype))
                if i == 2:
                    cur = c.V(94).astype(np.float64)
                    W.copy_(dev(cur))
            gph.replay()
            torch.cuda.synchronize()
            ey, egx, cur = expect(x64)
            assert np.array_equal(host(y), ey), ("y", i)
            assert np.array_equal(host(x.grad), egx), ("grad_x", i)
            assert np.array_equal(host(W), cur.astype(np.float32)), ("W", i)
        assert np.abs(cur).max() < 256                                # (exact in f16 all along)
    c.H.close()

    # (2) forward only
    H = handle(v, dtype)
    V1, V2 = c.V(95), c.V(96)
    W = dev(V1).requires_grad_(True)
    xs = c.x.clone()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        y = vbs_linear(xs, H, W)
        torch.cuda.synchronize()
        assert np.array_equal(host(y), c.y_ref(V1)), "eager forward"
        gph2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph2, stream=s):
            y = vbs_linear(xs, H, W)
        with torch.no_grad():
            W.copy_(dev(V2))
        gph2.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(y), c.y_ref(V2)), "replay after W.copy_()"
        # after a capture nothing is skipped on the handle: an eager call with another tensor, a replay, the eager call again
        W3 = dev(V1).requires_grad_(True)
        assert np.array_equal(host(vbs_linear(xs, H, W3)), c.y_ref(V1))
        gph2.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(vbs_linear(xs, H, W3)), c.y_ref(V1)), "eager forward after a replay"
    H.close()
