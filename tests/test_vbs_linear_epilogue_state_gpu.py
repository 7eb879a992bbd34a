"""The stale-values cases of tests/test_vbs_linear_gpu.py once more, through _VbsLinearEpilogue: its forward and backward repeat the values logic of the plain
Function line by line (sparta_amd/autograd.py), and nothing else runs the copy through these cases.

Every call passes bias = zeros(rows, requires_grad=True): y = z + 0 keeps every integer reference of `Case` exact, the layer is the epilogue Function (asserted
on grad_fn), and bias.grad must equal the column sums of grad_y -- integer data at n = 8, exact in fp32 and in the fp64 sum alike.  The references, the data
and the assertions are those of the plain cases; what is added is the bias gradient."""
import numpy as np
import pytest

from sparta_amd.autograd import vbs_linear

torch = pytest.importorskip("torch")

import _epilogue as E  # noqa: E402
from test_set_values_gpu import values  # noqa: E402
from test_spmm_t_gpu import dense_x  # noqa: E402
from test_vbs_linear_gpu import mats, dev, host, handle, operands, check_linear, Case, STATE, STATE_IDS  # noqa: E402,F401  (mats: the module fixture)

pytestmark = pytest.mark.gpu

state = pytest.mark.parametrize("dtype", STATE, ids=STATE_IDS)


class Layer:
    """vbs_linear with a zero bias that requires grad; keeps the bias of every call"""

    def __init__(self):
        self.biases = []

    def __call__(self, x, H, W, refresh=False):
        b = torch.zeros(H.rows, dtype=torch.float32, device="cuda", requires_grad=True)
        self.biases.append(b)
        y = vbs_linear(x, H, W, refresh, bias=b)
        assert type(y.grad_fn).__name__ == "_VbsLinearEpilogueBackward" and y.dtype == torch.float32
        return y

    def grad(self, i=-1):
        g = self.biases[i].grad
        return None if g is None else host(g)


def colsum(gy64):
    """the bias gradient of grad_y (n, rows) float64 of small integers: exact"""
    return gy64.sum(0).astype(np.float32)


@state
def test_same_values_twice_and_in_place_update(mats, dtype):
    c, layer = Case(mats, dtype), Layer()
    V1, V2 = c.V(1), c.V(2)
    W = dev(V1).requires_grad_(True)
    y1, y2 = layer(c.x, c.H, W), layer(c.x, c.H, W)
    assert np.array_equal(host(y1), c.y_ref(V1)) and np.array_equal(host(y2), c.y_ref(V1))
    with torch.no_grad():
        W.copy_(dev(V2))
    assert np.array_equal(host(layer(c.x, c.H, W)), c.y_ref(V2))
    assert not np.array_equal(c.y_ref(V1), c.y_ref(V2))
    c.H.close()


@state
def test_set_values_on_the_handle_between_two_forwards(mats, dtype):
    c, layer = Case(mats, dtype), Layer()
    V1, other = c.V(1), c.V(3)
    W = dev(V1).requires_grad_(True)
    assert np.array_equal(host(layer(c.x, c.H, W)), c.y_ref(V1))
    c.H.set_values(dev(other))
    assert np.array_equal(host(layer(c.x, c.H, W)), c.y_ref(V1))
    c.H.set_values_host(other)
    assert np.array_equal(host(layer(c.x, c.H, W)), c.y_ref(V1))
    c.H.close()


@state
def test_another_tensor_with_the_same_address_and_version(mats, dtype):
    c, layer = Case(mats, dtype), Layer()
    V1, V2 = c.V(1), c.V(4)
    nz = int(c.v.nztot)
    storage = torch.zeros(nz, dtype=torch.float32, device="cuda").untyped_storage()
    W1 = torch.empty(0, dtype=torch.float32, device="cuda").set_(storage, 0, (nz,))
    W1.copy_(dev(V1))
    W1.requires_grad_(True)
    assert np.array_equal(host(layer(c.x, c.H, W1)), c.y_ref(V1))
    W2 = torch.empty(0, dtype=torch.float32, device="cuda").set_(storage, 0, (nz,))
    W2.copy_(dev(V2))
    W2.requires_grad_(True)
    assert W2 is not W1 and W2.data_ptr() == W1.data_ptr() and W2._version == W1._version
    assert np.array_equal(host(layer(c.x, c.H, W2)), c.y_ref(V2))
    c.H.close()


@state
def test_new_tensor_after_the_old_one_was_freed(mats, dtype):
    c, layer = Case(mats, dtype), Layer()
    V1, V2 = c.V(1), c.V(5)
    W = dev(V1).requires_grad_(True)
    y = layer(c.x, c.H, W)
    assert np.array_equal(host(y), c.y_ref(V1))
    old = (W.data_ptr(), W._version)
    del W, y
    W = dev(V2).requires_grad_(True)
    reused = "data_ptr %s, version %s" % ("reused" if W.data_ptr() == old[0] else "not reused", "equal" if W._version == old[1] else "different")
    assert np.array_equal(host(layer(c.x, c.H, W)), c.y_ref(V2)), reused
    c.H.close()


@state
def test_refresh_after_a_write_the_version_counter_does_not_see(mats, dtype):
    c, layer = Case(mats, dtype), Layer()
    V1, V2, V3 = c.V(1), c.V(6), c.V(7)
    W = dev(V1).requires_grad_(True)
    layer(c.x, c.H, W)
    version = W._version
    W.data.copy_(dev(V2))
    assert W._version == version
    assert np.array_equal(host(layer(c.x, c.H, W, refresh=True)), c.y_ref(V2))
    W.data -= dev(V2 - V3)
    assert W._version == version
    assert np.array_equal(host(layer(c.x, c.H, W, True)), c.y_ref(V3))
    c.H.close()


@state
def test_backward_of_an_earlier_forward_after_the_handle_moved_on(mats, dtype):
    """the case that reaches the load(handle, values) branch of _VbsLinearEpilogue.backward"""
    c, layer = Case(mats, dtype), Layer()
    V1, V2 = c.V(1), c.V(8)
    W1, W2 = dev(V1).requires_grad_(True), dev(V2).requires_grad_(True)
    x = c.x.clone().requires_grad_(True)
    gy2_64 = dense_x(c.v.rows, c.n, 63, integer=True).T
    y1 = layer(x, c.H, W1)
    y2 = layer(x, c.H, W2)
    assert np.array_equal(host(y2), c.y_ref(V2))
    y1.backward(c.gy)
    assert np.array_equal(host(x.grad), c.gx_ref(V1)) and np.array_equal(host(W1.grad), c.gv_ref()) and W2.grad is None
    assert np.array_equal(layer.grad(0), colsum(c.gy64)) and layer.grad(1) is None
    assert not np.array_equal(c.gx_ref(V1), c.gx_ref(V2))
    x.grad = None
    y2.backward(dev(gy2_64))                                          # the second graph, after the handle went back to W1 for the first
    assert np.array_equal(host(x.grad), c.gx_ref(V2, gy2_64)) and np.array_equal(host(W2.grad), c.gv_ref(gy2_64))
    assert np.array_equal(layer.grad(1), colsum(gy2_64)) and not np.array_equal(colsum(gy2_64), colsum(c.gy64))
    assert np.array_equal(host(layer(x, c.H, W1)), c.y_ref(V1))
    # and a set_values of the caller's own between forward and backward
    x.grad = None
    y = layer(x, c.H, W1)
    c.H.set_values(dev(V2))
    y.backward(c.gy)
    assert np.array_equal(host(x.grad), c.gx_ref(V1)) and np.array_equal(layer.grad(), colsum(c.gy64))
    c.H.close()


@state
def test_in_place_change_between_forward_and_backward_raises(mats, dtype):
    c, layer = Case(mats, dtype), Layer()
    W = dev(c.V(1)).requires_grad_(True)
    x = c.x.clone().requires_grad_(True)
    y = layer(x, c.H, W)
    with torch.no_grad():
        W += 1
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward(c.gy)
    y = layer(x, c.H, W)                                              # ... and so does the bias, which the Function saves too
    with torch.no_grad():
        layer.biases[-1] += 1
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward(c.gy)
    c.H.close()


@state
def test_only_one_input_requires_grad(mats, dtype, monkeypatch):
    c, layer = Case(mats, dtype), Layer()
    V1 = c.V(1)
    calls = []
    for name in ("spmm_t", "sddmm"):
        monkeypatch.setattr(c.H, name, lambda *a, _f=getattr(c.H, name), _n=name, **k: (calls.append(_n), _f(*a, **k))[1])
    x = c.x.clone().requires_grad_(True)
    W = dev(V1)
    layer(x, c.H, W).backward(c.gy)
    assert np.array_equal(host(x.grad), c.gx_ref(V1)) and W.grad is None and calls == ["spmm_t"]
    assert np.array_equal(layer.grad(), colsum(c.gy64))
    del calls[:]
    W.requires_grad_(True)
    layer(c.x, c.H, W).backward(c.gy)
    assert np.array_equal(host(W.grad), c.gv_ref()) and c.x.grad is None and calls == ["sddmm"]
    assert np.array_equal(layer.grad(), colsum(c.gy64))
    c.H.close()


@state
def test_expanded_and_non_contiguous_grad_y(mats, dtype):
    c, layer = Case(mats, dtype), Layer()
    V1 = c.V(1)
    W = dev(V1).requires_grad_(True)
    x = c.x.clone().requires_grad_(True)
    ones = np.ones((c.n, c.v.rows))
    layer(x, c.H, W).sum().backward()                                 # grad_y: a stride-0 expansion of one element
    assert np.array_equal(host(x.grad), c.gx_ref(V1, ones)) and np.array_equal(host(W.grad), c.gv_ref(ones))
    assert np.array_equal(layer.grad(), colsum(ones))
    x.grad = W.grad = None
    g = dev(c.gy64.T).t()                                             # (n, rows) with strides (1, n)
    assert not g.is_contiguous()
    layer(x, c.H, W).backward(g)
    assert np.array_equal(host(x.grad), c.gx_ref(V1)) and np.array_equal(host(W.grad), c.gv_ref())
    assert np.array_equal(layer.grad(), colsum(c.gy64))
    x.grad = W.grad = None
    layer(x, c.H, W).t().contiguous().backward(g.t())                 # autograd hands in the transposed view of a contiguous (rows, n) tensor
    assert np.array_equal(host(x.grad), c.gx_ref(V1)) and np.array_equal(host(W.grad), c.gv_ref())
    assert np.array_equal(layer.grad(), colsum(c.gy64))
    c.H.close()


@state
def test_gradients_accumulate_over_two_passes_before_one_update(mats, dtype):
    c = Case(mats, dtype)
    V1 = c.V(1)
    W = dev(V1).requires_grad_(True)
    b = torch.zeros(c.v.rows, dtype=torch.float32, device="cuda", requires_grad=True)          # one bias for both passes: its gradient accumulates too
    gy2_64 = dense_x(c.v.rows, c.n, 64, integer=True).T
    vbs_linear(c.x, c.H, W, bias=b).backward(c.gy)
    vbs_linear(c.x, c.H, W, bias=b).backward(dev(gy2_64))
    total = c.gv_ref().astype(np.float64) + c.gv_ref(gy2_64)
    assert np.array_equal(host(W.grad), total.astype(np.float32))
    assert np.array_equal(host(b.grad), colsum(c.gy64 + gy2_64))
    with torch.no_grad():
        W -= torch.sign(W.grad)                                       # (the values stay small integers)
    V2 = (V1 - np.sign(total)).astype(np.float32)
    y = vbs_linear(c.x, c.H, W, bias=b)
    assert type(y.grad_fn).__name__ == "_VbsLinearEpilogueBackward" and np.array_equal(host(y), c.y_ref(V2))
    c.H.close()


@state
def test_two_handles_one_tensor(mats, dtype):
    v = mats["jaccard"]
    n = 24
    H1, H2 = handle(v, dtype), handle(v, dtype)
    x, gy = operands(v, dtype, n, 81, integer=False)
    V = values(v, 80, integer=False)
    W = dev(V).requires_grad_(True)
    layer = Layer()
    want_db = E.dbias_of(np.ascontiguousarray(host(gy).T))             # activation "none": the fp32 dz is grad_y itself
    for step in range(2):
        out = []
        for H in (H1, H2):
            xh = x.clone().requires_grad_(True)
            W.grad = None
            y = layer(xh, H, W)
            y.backward(gy)
            out.append((y.detach(), xh.grad, W.grad))
            assert np.array_equal(E.bits(layer.grad()), E.bits(want_db)), step
        torch.cuda.synchronize()
        for a, b in zip(*out):
            assert torch.equal(a, b), step
        check_linear("jaccard", v, dtype, host(W), x, gy, *out[1], integer=False, what=step)
        with torch.no_grad():
            W -= 0.25 * W.grad
    H1.close(); H2.close()

