"""The state logic of sparta_amd.autograd.vbs_linear without a device: which values the forward multiplies with and which ones the backward differentiates,
when the tensor, its contents or the handle change between the calls.

The autograd Function is driven directly (the is_cuda checks live in vbs_linear) with CPU tensors and a stub handle that keeps a dense float64 matrix
and does set_values / spmm / spmm_t / sddmm in plain torch on exactly the buffers the Function passes, counting every call.  Reference: float64
torch.nn.functional.linear on the dense matrix of the values; all data are small integers, so every comparison is exact."""
import collections

import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd.autograd import _function
from sparta_amd.device import DeviceVBS, ValuesRecord

torch = pytest.importorskip("torch")

ROWS, COLS, NZ, N = 5, 7, 16, 3


class StubHandle(ValuesRecord):
    """a `rows` x `cols` matrix with `nztot` stored positions (rr[p], cc[p]); operands and results in the layouts DeviceVBS takes them from vbs_linear"""

    def __init__(self, seed=0):
        rng = np.random.default_rng(seed)
        pos = rng.permutation(ROWS * COLS)[:NZ]
        self.rr, self.cc = torch.from_numpy(pos // COLS), torch.from_numpy(pos % COLS)
        self.rows, self.cols, self.dtype = ROWS, COLS, sa.F32
        self.A = torch.zeros((ROWS, COLS), dtype=torch.float64)
        self.calls = collections.Counter()

    def _nztot(self):
        return NZ

    def dense(self, values):
        """the dense float64 matrix of `values` (differentiable)"""
        return torch.zeros((ROWS, COLS), dtype=torch.float64).index_put((self.rr, self.cc), values.double())

    def set_values(self, mab):
        assert mab.dtype == torch.float32 and mab.shape == (NZ,) and mab.is_contiguous() and not mab.requires_grad
        self.calls["set_values"] += 1
        self._values_replaced()
        self.A = self.dense(mab)                                     # (a copy: later writes to mab are not seen, as on the device)

    def spmm(self, B, C_out, n_cols, accumulate=False):
        assert B.dtype == torch.float32 and B.shape == (n_cols, COLS) and B.is_contiguous() and not B.requires_grad and not accumulate
        assert C_out.dtype == torch.float32 and C_out.shape == (n_cols, ROWS) and C_out.is_contiguous()
        self.calls["spmm"] += 1
        C_out.copy_(B.double() @ self.A.T)

    def spmm_t(self, X, Ct_out, n_cols, accumulate=False):
        assert X.dtype == torch.float32 and X.shape == (n_cols, ROWS) and X.is_contiguous() and not accumulate
        assert Ct_out.dtype == torch.float32 and Ct_out.shape == (n_cols, COLS) and Ct_out.is_contiguous()
        self.calls["spmm_t"] += 1
        Ct_out.copy_(X.double() @ self.A)

    def sddmm(self, X, Y, G_out, k, accumulate=False):
        assert X.dtype == torch.float32 and X.shape == (k, ROWS) and X.is_contiguous() and not accumulate
        assert Y.dtype == torch.float32 and Y.shape == (k, COLS) and Y.is_contiguous() and not Y.requires_grad
        assert G_out.dtype == torch.float32 and G_out.shape == (NZ,) and G_out.is_contiguous()
        self.calls["sddmm"] += 1
        G_out.copy_((X.double().T @ Y.double())[self.rr, self.cc])


def ints(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(-4, 5, shape).astype(np.float32))


def linear(x, H, W, refresh=False):
    return _function().apply(x, W, H, True) if refresh else _function().apply(x, W, H)


def ref(H, x, W, gy=None):
    """float64 F.linear on the dense matrix of W: y, and with gy also (grad_x, grad_values)"""
    x64, W64 = x.detach().double().requires_grad_(True), W.detach().double().requires_grad_(True)
    y = torch.nn.functional.linear(x64, H.dense(W64))
    if gy is None:
        return y.detach().float()
    y.backward(gy.double())
    return y.detach().float(), x64.grad.float(), W64.grad.float()


def test_same_values_twice():
    H, x, W = StubHandle(), ints((N, COLS), 1), ints(NZ, 2).requires_grad_(True)
    y1, y2 = linear(x, H, W), linear(x, H, W)
    assert torch.equal(y1, ref(H, x, W)) and torch.equal(y2, y1)
    assert H.calls["set_values"] == 1 and H.calls["spmm"] == 2        # the unchanged tensor is not written again


def test_in_place_update_under_no_grad_is_seen():
    H, x, W = StubHandle(), ints((N, COLS), 1), ints(NZ, 2).requires_grad_(True)
    y1 = linear(x, H, W).detach()
    with torch.no_grad():
        W -= ints(NZ, 3)
    y2 = linear(x, H, W)
    assert torch.equal(y2, ref(H, x, W)) and not torch.equal(y2, y1)


def test_set_values_on_the_handle_between_two_forwards():
    H, x, W, other = StubHandle(), ints((N, COLS), 1), ints(NZ, 2).requires_grad_(True), ints(NZ, 4)
    y1 = linear(x, H, W)
    H.set_values(other)
    y2 = linear(x, H, W)
    assert torch.equal(y1, ref(H, x, W)) and torch.equal(y2, y1)
    assert not torch.equal(y2, ref(H, x, other))


def test_another_tensor_with_the_same_address_and_version():
    """two tensor objects on ONE storage, each with its own version counter: equal data_ptr() by construction and equal _version after the same history"""
    H, x = StubHandle(), ints((N, COLS), 1)
    storage = torch.zeros(NZ, dtype=torch.float32).untyped_storage()
    V1, V2 = ints(NZ, 2), ints(NZ, 5)
    W1 = torch.empty(0, dtype=torch.float32).set_(storage, 0, (NZ,))
    W1.copy_(V1)
    W1.requires_grad_(True)
    y1 = linear(x, H, W1)
    assert torch.equal(y1, ref(H, x, V1))
    W2 = torch.empty(0, dtype=torch.float32).set_(storage, 0, (NZ,))
    W2.copy_(V2)                                                      # (through W2: W1's counter does not move)
    W2.requires_grad_(True)
    assert W2 is not W1 and W2.data_ptr() == W1.data_ptr() and W2._version == W1._version
    y2 = linear(x, H, W2)
    assert torch.equal(y2, ref(H, x, V2)) and not torch.equal(y2, y1)


def test_refresh_after_a_write_the_version_counter_does_not_see():
    H, x, W, new = StubHandle(), ints((N, COLS), 1), ints(NZ, 2).requires_grad_(True), ints(NZ, 6)
    linear(x, H, W)
    version = W._version
    W.data.copy_(new)
    assert W._version == version
    y = linear(x, H, W, refresh=True)
    assert torch.equal(y, ref(H, x, new))
    assert H.calls["set_values"] == 2
    linear(x, H, W, refresh=True)                                     # refresh always writes
    assert H.calls["set_values"] == 3


def test_backward_of_an_earlier_forward_after_the_handle_moved_on():
    H, x = StubHandle(), ints((N, COLS), 1).requires_grad_(True)
    W1, W2 = ints(NZ, 2).requires_grad_(True), ints(NZ, 7).requires_grad_(True)
    g1, g2 = ints((N, ROWS), 8), ints((N, ROWS), 9)
    y1 = linear(x, H, W1)
    y2 = linear(x, H, W2)
    assert torch.equal(y2, ref(H, x, W2))
    y1.backward(g1)
    _, gx1, gv1 = ref(H, x, W1, g1)
    assert torch.equal(x.grad, gx1) and torch.equal(W1.grad, gv1) and W2.grad is None
    x.grad = None
    y2.backward(g2)                                                   # the second graph, after the handle went back to W1 for the first
    _, gx2, gv2 = ref(H, x, W2, g2)
    assert torch.equal(x.grad, gx2) and torch.equal(W2.grad, gv2)
    y3 = linear(x, H, W1)                                             # and a forward after all that
    assert torch.equal(y3, ref(H, x, W1))


def test_backward_after_set_values_on_the_handle():
    H, x, W = StubHandle(), ints((N, COLS), 1).requires_grad_(True), ints(NZ, 2).requires_grad_(True)
    g = ints((N, ROWS), 8)
    y = linear(x, H, W)
    H.set_values(ints(NZ, 4))
    y.backward(g)
    _, gx, gv = ref(H, x, W, g)
    assert torch.equal(x.grad, gx) and torch.equal(W.grad, gv)


def test_in_place_change_between_forward_and_backward_raises():
    H, x, W = StubHandle(), ints((N, COLS), 1).requires_grad_(True), ints(NZ, 2).requires_grad_(True)
    y = linear(x, H, W)
    with torch.no_grad():
        W += 1
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward(ints((N, ROWS), 8))


def test_only_x_requires_grad():
    H, x, W, g = StubHandle(), ints((N, COLS), 1).requires_grad_(True), ints(NZ, 2), ints((N, ROWS), 8)
    linear(x, H, W).backward(g)
    assert torch.equal(x.grad, ref(H, x, W, g)[1]) and W.grad is None
    assert H.calls == {"set_values": 1, "spmm": 1, "spmm_t": 1}       # no sddmm


def test_only_values_require_grad():
    H, x, W, g = StubHandle(), ints((N, COLS), 1), ints(NZ, 2).requires_grad_(True), ints((N, ROWS), 8)
    y = linear(x, H, W)
    H.set_values(ints(NZ, 4))                                         # grad_values does not depend on the handle's values: nothing is written back
    y.backward(g)
    assert torch.equal(W.grad, ref(H, x, W, g)[2]) and x.grad is None
    assert H.calls == {"set_values": 2, "spmm": 1, "sddmm": 1}        # no spmm_t


def test_expanded_and_non_contiguous_grad_y():
    H, x, W = StubHandle(), ints((N, COLS), 1).requires_grad_(True), ints(NZ, 2).requires_grad_(True)
    linear(x, H, W).sum().backward()                                  # grad_y: a stride-0 expansion of one element
    _, gx, gv = ref(H, x, W, torch.ones((N, ROWS)))
    assert torch.equal(x.grad, gx) and torch.equal(W.grad, gv)
    x.grad = W.grad = None
    g = ints((ROWS, N), 8).t()                                        # (N, ROWS) with strides (1, N)
    assert not g.is_contiguous()
    linear(x, H, W).backward(g)
    _, gx, gv = ref(H, x, W, g)
    assert torch.equal(x.grad, gx) and torch.equal(W.grad, gv)
    x.grad = W.grad = None
    linear(x, H, W).t().contiguous().backward(g.t())                  # autograd hands in the transposed view of a contiguous (ROWS, N) tensor
    assert torch.equal(x.grad, gx) and torch.equal(W.grad, gv)


def test_gradients_accumulate_over_two_passes_before_one_update():
    H, W = StubHandle(), ints(NZ, 2).requires_grad_(True)
    total = torch.zeros(NZ)
    for seed in (10, 11):
        x, g = ints((N, COLS), seed), ints((N, ROWS), seed + 10)
        linear(x, H, W).backward(g)
        total += ref(H, x, W, g)[2]
    assert torch.equal(W.grad, total)
    assert H.calls["set_values"] == 1
    with torch.no_grad():
        W -= W.grad
    x = ints((N, COLS), 12)
    assert torch.equal(linear(x, H, W), ref(H, x, W))
    assert H.calls["set_values"] == 2


def test_a_device_handle_starts_without_a_record_and_close_drops_it():
    d = DeviceVBS(None)                                               # (an empty handle: nothing on a device)
    assert d._autograd_values is None
    d._autograd_values = (None, None)
    d.close()
    assert d._autograd_values is None
