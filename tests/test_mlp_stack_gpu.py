"""Two stacked vbs_linear layers through the whole training stack, teacher-forced, against independent references.

    h = act1(x @ A1^T + b1) in out_dtype        y = h @ A2^T + b2        loss = (y * gy).sum() * ctl.loss_scale

with VbsAdamW over both (handle, values) pairs, GradCtl (loss scale 1024, max_norm 1, growth every 2 steps), BlockPruner(scope="global") and a test-side
device update of the biases.  Five steps: prune(0.5) after step 1, one +Inf planted in gy at step 3 (the step skips, the scale backs off), prune(0.75) after
step 3, and by step 5 the scale has grown again.  Three arms on identical inputs: mask_grads() with no live set, skip_pruned, skip_pruned + live_steps.

Every check takes the DEVICE's own tensors of the link before it as its inputs, so no error accumulates and every bound is one the project already has:
the products within 1e-5 * sum|a||b| of float64 on the values as the handle's type stores them (check_linear of tests/test_vbs_linear_gpu.py), the epilogue
bit for bit against tests/_epilogue.py (GELU by the measure and criterion of tests/test_epilogue_gpu.py::test_gelu_against_float64), the bias gradient bit
for bit against dbias_of, the control record against stats_ref / grad_ctl_ref, the step bit for bit against adam_ref, the masks against scores recomputed on
the host.  On the skipped step the gradients hold Inf and NaN: an element whose reference is finite is held as on every other step, one whose reference is
not must be non-finite on the device too, except where the device may skip the product (a pruned block, a position past cols).

Geometries (IN 130, HID 200, OUT 90, n 33: a ragged last block column in both layers, even rows and cols, two runs of 32 columns in the bias gradient):
    h16   layer 1 f16 h 40 w 64, GELU, out float16;   layer 2 f16  h 30 w 96: both take the fused image step
    f32   layer 1 f32 h 20 w 32, ReLU, out bfloat16;  layer 2 bf16 h 40 w 32: the fused step (tiles of at most 32 rows: the fragment image), and the
          two-pass step -- block-rows of 40, 40 and 10 rows put elements into both stream images of a 16-bit handle, so no one image kernel owns the step
          (sgd_fused_image, vbs_capi.cpp; a 16-bit handle needs w % 32 == 0, so there is no width without an image kernel to take instead)
The grouping is rows // h, as in train_geometries(): the reordered row order of h is the original one.  The initial values of one whole block column of
layer 2 and of one whole block-row of layer 1 are scaled by 2^-8: after the last prune all their blocks are dead (asserted), so spmm_t meets an empty list
and sddmm an item without a live group.  The Inf sits in a row of layer 2 whose block-row does not store the weak block column and whose blocks score
highest, so that it meets live blocks only: a pruned block times Inf is NaN where the block is multiplied (no live set) and nothing where it is left out
(DESIGN.md section 4 leaves a stored zero times a non-finite operand open), and the statistics of the skipped step would differ between the arms for
that reason alone.  tests/test_mlp_stack_host.py checks these conditions on a float64 model of the loop, without a GPU."""
import math

import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd.autograd import vbs_linear

torch = pytest.importorskip("torch")

import _util as U  # noqa: E402
import _epilogue as E  # noqa: E402
from test_adam_step_host import adam_ref  # noqa: E402
from test_grad_ctl_host import stats_ref, grad_ctl_ref, record_fields  # noqa: E402

f32 = np.float32
IN, HID, OUT, N = 130, 200, 90, 33
STEPS = 5
PRUNE_AFTER = {1: 0.5, 3: 0.75}
INF_STEP, INF_SAMPLE = 3, 5                                          # the step and the row of gy (a sample) of the planted Inf; its column (a row of layer 2): inf_row
LOSS_SCALE, MAX_NORM, GROWTH_INTERVAL = 1024.0, 1.0, 2
ADAM = dict(lr=1e-2, weight_decay=0.01)
LR_B = 2.0 ** -6                                                     # a power of two: LR_B * coef is exact, so the bias update has two roundings whatever the order
CTL_CFG = dict(max_norm=MAX_NORM, growth_interval=GROWTH_INTERVAL)
ARMS = ("mask", "skip", "live")
EDT = {torch.float32: E.F32, torch.float16: E.F16, torch.bfloat16: E.BF16}
ACT = {"none": E.NONE, "relu": E.RELU, "gelu": E.GELU}
CONFIGS = {
    "h16": dict(l1=dict(dtype=sa.F16, h=40, w=64, act="gelu", out=torch.float16, nnz=150, fused=1, weak=("row", 1)),
                l2=dict(dtype=sa.F16, h=30, w=96, act="none", out=torch.float32, nnz=150, fused=1, weak=("col", 1), strong=2), seed=20261104, inf_row=67),
    "f32": dict(l1=dict(dtype=sa.F32, h=20, w=32, act="relu", out=torch.bfloat16, nnz=120, fused=1, weak=("row", 3)),
                l2=dict(dtype=sa.BF16, h=40, w=32, act="none", out=torch.float32, nnz=150, fused=0, weak=("col", 2), strong=1), seed=20261103, inf_row=71),
}
TDT = {sa.F32: torch.float32, sa.F16: torch.float16, sa.BF16: torch.bfloat16}
_GEOM, _EAGER = {}, {}
GELU_SEEN = {"y": 0.0, "dz": 0.0, "torch_y": 0.0, "torch_dz": 0.0}   # the largest measures of the run, in the units of tests/test_epilogue_gpu.py


# ---- geometry and inputs: numpy only ----------------------------------------------------------------------------------------------------------------------
class Geometry:
    """one layer: the VBR, its block table, per block (block-row, block column), the initial values"""

    def __init__(self, rows, cols, spec, seed, layer):
        m = sa.gen.uniform_random(rows, cols, spec["nnz"], seed=seed)
        kind, which = spec["weak"]
        self.strong = strong = spec.get("strong")                    # layer 2: the block-row of the planted Inf does not store the weak block column
        if strong is not None:
            r = np.repeat(np.arange(rows), np.diff(m.rowptr))
            sel = ~((r // spec["h"] == strong) & (m.colidx // spec["w"] == which))
            m = sa.CSR(rows, cols, np.concatenate([[0], np.cumsum(np.bincount(r[sel], minlength=rows))]).astype(np.int64), m.colidx[sel], m.vals[sel])
        self.v = v = sa.VBR().fill_from_CSR_inplace(m, np.arange(rows, dtype=np.int64) // spec["h"], spec["w"])
        self.T = T = v.block_table()
        self.nb, self.nz, self.w = len(T), int(v.nztot), int(spec["w"])
        self.blocks = U.edge_blocks(v)
        assert [b[0] for b in self.blocks] == T[:, 0].tolist() and sum(h * self.w for _, _, h, _, _ in self.blocks) == self.nz
        self.brow, self.bcol = T[:, 3] >> 32, T[:, 3] & 0xffffffff
        self.inside = U.edge_sample(v, np.ones((rows, cols))) != 0     # per stored element: inside the matrix (False past cols)
        rng = np.random.default_rng(seed + 1)
        D = rng.uniform(-1, 1, (rows, cols))
        D[D == 0] = 0.5
        # every block gets a root mean square of its own, 0.12 * 1.005^e with a different e for every block of the two layers: the scores start 1 % apart,
        # so the cut of a prune falls into a gap that the last bits of a sum cannot close (tests/test_mlp_stack_host.py asserts the gap at every cut)
        order = rng.permutation(self.nb)
        if strong is not None:                                       # ... and its blocks score highest: they are live when the Inf comes
            mine = np.flatnonzero(self.brow == strong)
            order = np.argsort(np.argsort(np.where(np.isin(np.arange(self.nb), mine), self.nb + order, order)))
        assert self.nb <= 50
        for e, (_, r0, h, c0, valid) in zip(2 * ((order * 50) // self.nb) + layer, self.blocks):          # (both layers spread over the same range)
            blk = D[r0:r0 + h, c0:c0 + valid]
            blk *= 0.12 * 1.005 ** int(e) / math.sqrt(float((blk * blk).mean()))
        self.weak = np.flatnonzero((self.brow if kind == "row" else self.bcol) == which)          # the blocks that start 2^-8 times as large
        if kind == "row":
            D[int(v.row_part[which]):int(v.row_part[which + 1])] *= 2.0 ** -8
        else:
            D[:, which * self.w:(which + 1) * self.w] *= 2.0 ** -8
        self.W0 = U.edge_sample(v, D).astype(f32)
        assert rows % 2 == 0 and cols % 2 == 0 and cols % self.w != 0 and (self.bcol == cols // self.w).any()          # even; a ragged last block column that holds blocks
        assert len(self.weak) >= 2 and (kind == "row" or which != cols // self.w)
        assert strong is None or (len(mine) >= 2 and not np.isin(mine, self.weak).any())

    def element_dead(self, keep):
        m = np.zeros(self.nz, bool)
        for b in np.flatnonzero(np.asarray(keep) == 0):
            m[int(self.T[b, 0]):int(self.T[b, 0] + self.T[b, 2])] = True
        return m

    def scores(self, W):
        sq = np.asarray(W, np.float64) ** 2
        return np.array([math.fsum(sq[o:o + n]) / n for o, n in zip(self.T[:, 0], self.T[:, 1])])

    def dense(self, W, dtype):
        return U.edge_dense(self.v, dtype, mab=np.asarray(W, f32))

    def sample(self, M):
        return U.edge_sample(self.v, M)


def geometry(name):
    if name not in _GEOM:
        cfg = CONFIGS[name]
        g1, g2 = Geometry(HID, IN, cfg["l1"], cfg["seed"], 0), Geometry(OUT, HID, cfg["l2"], cfg["seed"] + 10, 1)
        rng = np.random.default_rng(cfg["seed"] + 20)
        xs = [U.edge_round(rng.uniform(-1, 1, (N, IN)), cfg["l1"]["dtype"]).astype(f32) for _ in range(STEPS)]
        gys = [U.edge_round(rng.uniform(-1, 1, (N, OUT)), cfg["l2"]["dtype"]).astype(f32) for _ in range(STEPS)]
        gys[INF_STEP - 1][INF_SAMPLE, cfg["inf_row"]] = np.inf
        assert cfg["inf_row"] // cfg["l2"]["h"] == g2.strong
        b1, b2 = rng.uniform(-0.25, 0.25, HID).astype(f32), rng.uniform(-0.25, 0.25, OUT).astype(f32)
        _GEOM[name] = (g1, g2, xs, gys, b1, b2)
    return _GEOM[name]


def bias_runs(n):
    """the runs of E.RUN columns the bias gradient is summed in: above one, the fold kernel runs and the scratch is used"""
    return (n + E.RUN - 1) // E.RUN


def select_host(scores, keeps, sparsity):
    """the masks sa.prune.select gives on host scores (pure torch, CPU)"""
    new = sa.prune.select([torch.from_numpy(s) for s in scores], [torch.from_numpy(np.asarray(k, np.uint8)) for k in keeps], sparsity, "global")
    return [k.numpy().astype(np.uint8) for k in new]


# ---- small helpers ------------------------------------------------------------------------------------------------------------------------------------------
def np32(t):
    """a device tensor as float32 numpy, 16-bit types widened exactly"""
    return t.detach().float().cpu().numpy()


def ubits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def stored(t):
    """the stored form of a device tensor as tests/_epilogue.py has it: float32, or the uint16 bits"""
    t = t.detach().contiguous()
    return t.cpu().numpy() if t.dtype == torch.float32 else t.view(torch.int16).cpu().numpy().view(np.uint16)


def same_where_finite(got, ref):
    """bit for bit where the reference is finite; where it is not, the device's element is not either (the bits of a NaN are not pinned across processors)"""
    got, ref = np.asarray(got, f32), np.asarray(ref, f32)
    fin = np.isfinite(ref)
    return got.shape == ref.shape and np.array_equal(ubits(got)[fin], ubits(ref)[fin]) and not np.isfinite(got[~fin]).any()


def close_where_finite(got, ref, bound, free=None):
    """|got - ref| <= bound + 1e-30 where ref and bound are finite; elsewhere got is non-finite too, unless `free` (the device may skip the product there)"""
    fin = np.isfinite(ref) & np.isfinite(bound)
    ok = np.abs(np.where(fin, got, 0.0) - np.where(fin, ref, 0.0)) <= np.where(fin, bound, 0.0) + 1e-30
    rest = ~fin if free is None else ~fin & ~free
    return bool(ok.all()) and not np.isfinite(got[rest]).any()


def gelu_fwd_ok(u, y32):
    from test_epilogue_gpu import gelu_measures
    one, zero = np.ones_like(u), np.zeros_like(u)
    ours = gelu_measures(u, one, y32, zero)[0]
    ref = gelu_measures(u, one, torch.nn.functional.gelu(torch.from_numpy(u.copy())).numpy(), zero)[0]
    GELU_SEEN["y"], GELU_SEEN["torch_y"] = max(GELU_SEEN["y"], ours), max(GELU_SEEN["torch_y"], ref)
    return ours <= 4 * ref + 1, (ours, ref)


def gelu_bwd_ok(u, dy, dz32):
    """over the elements with a finite non-zero dy (the measure divides by |dy|); elsewhere: dy == 0 gives a zero, a non-finite dy a non-finite dz"""
    from test_epilogue_gpu import gelu_measures
    sel = np.isfinite(dy) & (dy != 0)
    us, dys = np.ascontiguousarray(u[sel]), np.ascontiguousarray(dy[sel])
    ut = torch.from_numpy(us.copy()).requires_grad_(True)
    torch.nn.functional.gelu(ut).backward(torch.from_numpy(dys))
    ours, ref = gelu_measures(us, dys, us, dz32[sel])[1], gelu_measures(us, dys, us, ut.grad.numpy())[1]
    GELU_SEEN["dz"], GELU_SEEN["torch_dz"] = max(GELU_SEEN["dz"], ours), max(GELU_SEEN["torch_dz"], ref)
    rest = not dz32[dy == 0].any() and not np.isfinite(dz32[~np.isfinite(dy)]).any()
    return ours <= 4 * ref + 1 and rest, (ours, ref)


# ---- the model on the device ----------------------------------------------------------------------------------------------------------------------------------
class Layer:
    def __init__(self, g, spec, b0):
        self.g, self.spec, self.dtype = g, spec, spec["dtype"]
        self.H = g.v.to_device(0, dtype=self.dtype, updatable=True, transposable=True)
        self.W = torch.from_numpy(g.W0.copy()).cuda().requires_grad_(True)
        self.b = torch.from_numpy(b0.copy()).cuda().requires_grad_(True)
        self.act, self.out = spec["act"], spec["out"]

    def forward(self, x):
        return vbs_linear(x, self.H, self.W, bias=self.b, activation=self.act, out_dtype=self.out)


class Model:
    def __init__(self, name, arm):
        g1, g2, self.xs, self.gys, b1, b2 = geometry(name)
        cfg = CONFIGS[name]
        self.name, self.arm = name, arm
        self.l1, self.l2 = Layer(g1, cfg["l1"], b1), Layer(g2, cfg["l2"], b2)
        self.layers = (self.l1, self.l2)
        self.opt = sa.VbsAdamW([(l.H, l.W) for l in self.layers], **ADAM)
        self.ctl = sa.GradCtl(loss_scale=LOSS_SCALE, max_norm=MAX_NORM, growth_interval=GROWTH_INTERVAL)
        self.pruner = sa.BlockPruner(self.opt, scope="global", skip_pruned=arm != "mask", live_steps=arm == "live")
        self.x = torch.empty((N, IN), dtype=TDT[cfg["l1"]["dtype"]], device="cuda")
        self.gy = torch.empty((N, OUT), dtype=torch.float32, device="cuda")
        self.h = self.y = None

    def load(self, step):
        with torch.no_grad():
            self.x.copy_(torch.from_numpy(self.xs[step - 1]).cuda())
            self.gy.copy_(torch.from_numpy(self.gys[step - 1]).cuda())

    def step(self, observe=None):
        """one whole step, device work only (launches and torch device operations: it can be captured).  observe(point): the eager run looks at the device
        between the links"""
        see = observe or (lambda point: None)
        self.opt.zero_grad()
        self.l1.b.grad = self.l2.b.grad = None
        self.h = self.l1.forward(self.x)
        self.h.retain_grad()
        see("fwd1")
        self.y = self.l2.forward(self.h)
        self.y.retain_grad()
        see("fwd2")
        ((self.y * self.gy).sum() * self.ctl.loss_scale).backward()
        see("bwd")
        if self.arm == "mask":
            self.pruner.mask_grads()
        see("masked")
        self.ctl.collect([self.opt, self.l1.b, self.l2.b])
        see("collected")
        self.opt.step(ctl=self.ctl)
        with torch.no_grad():
            coef, skip = self.ctl._f32[7], self.ctl.R[8]
            for l in self.layers:
                l.b.copy_(torch.where(skip != 0, l.b, l.b - (LR_B * coef) * l.b.grad))

    def state_tensors(self):
        """every tensor a step or a prune changes, by name (the optimizer's state exists after the first step)"""
        out = {"R": self.ctl.R}
        for i, l in enumerate(self.layers):
            s = self.opt._state[i]
            out.update({"W%d" % i: l.W, "b%d" % i: l.b, "M%d" % i: s["exp_avg"], "V%d" % i: s["exp_avg_sq"], "S%d" % i: s["state"],
                        "keep%d" % i: self.pruner.keep_masks()[i]})
        return out

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: t.detach().cpu().numpy().copy() for k, t in self.state_tensors().items()}

    def close(self):
        for l in self.layers:
            l.H.close()


def same_state(a, b):
    """the names of the state tensors that differ in any bit"""
    return [k for k in a if not np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8))]


# ---- the checks of one eager step -----------------------------------------------------------------------------------------------------------------------------
class Checker:
    """looks at the device between the links of Model.step and holds each link to its reference"""

    def __init__(self, m, step, keeps):
        self.m, self.step, self.keeps = m, step, keeps
        self.seen = {}
        self.finite_step = step != INF_STEP

    def __call__(self, point):
        with np.errstate(invalid="ignore", over="ignore"):          # (the skipped step's references hold Inf and NaN)
            getattr(self, point)()

    def what(self, *a):
        return (self.m.name, self.m.arm, self.step) + a

    # 1 + 2: products and epilogue, forward
    def _forward(self, i, x, y):
        l = self.m.layers[i]
        g = l.g
        z = torch.empty((N, g.v.rows), dtype=torch.float32, device="cuda")
        l.H.spmm(x.detach(), z, N, accumulate=False)
        Wh, bh, xh, zh = np32(l.W), np32(l.b), np32(x).astype(np.float64), np32(z)
        A = g.dense(Wh, l.dtype)
        assert np.isfinite(zh).all() and np.isfinite(np32(y)).all(), self.what(i, "non-finite forward")
        assert np.all(np.abs(zh - xh @ A.T) <= 1e-5 * (np.abs(xh) @ np.abs(A).T) + 1e-30), self.what(i, "z")
        dead = g.element_dead(self.keeps[i])
        assert not ubits(Wh)[dead].any(), self.what(i, "a pruned block is not zero in W")
        act, odt = ACT[l.act], EDT[l.out]
        Z = np.ascontiguousarray(zh.T)
        y32 = sa.epilogue_fwd(z, l.b.detach(), l.act, torch.float32)
        if act == E.GELU:
            ok, m = gelu_fwd_ok(E._u(Z, bh), np.ascontiguousarray(np32(y32).T))
            assert ok, self.what(i, "gelu y", m)
        else:
            assert np.array_equal(E.bits(np32(y32).T), E.bits(E.fwd_ref(Z, bh, act, E.F32))), self.what(i, "y32")
            assert np.array_equal(E.bits(stored(y).T), E.bits(E.fwd_ref(Z, bh, act, odt))), self.what(i, "y")
        assert y.dtype == l.out and np.array_equal(E.bits(stored(y).T), E.bits(E.rne_bits(np.ascontiguousarray(np32(y32).T), odt))), self.what(i, "y rounds y32")
        self.seen["z%d" % i], self.seen["x%d" % i] = z, x.detach()

    def fwd1(self):
        self._forward(0, self.m.x, self.m.h)

    def fwd2(self):
        self._forward(1, self.m.h, self.m.y)

    # 3 + 4: epilogue and products, backward
    def bwd(self):
        m = self.m
        self.raw = [l.W.grad.detach().clone() for l in m.layers]
        for i, (l, grad_y) in enumerate(((m.l1, m.h.grad), (m.l2, m.y.grad))):
            g, act, x, z = l.g, ACT[l.act], self.seen["x%d" % i], self.seen["z%d" % i]
            op = TDT[l.dtype]
            assert grad_y is not None and grad_y.dtype == l.out, self.what(i, "grad_y")
            zz = None if l.act == "none" else z
            dz32, _ = sa.epilogue_bwd(grad_y, zz, l.b.detach(), l.act, torch.float32, True)
            dzop, _ = sa.epilogue_bwd(grad_y, zz, l.b.detach(), l.act, op, True)
            dY, Z, bh = np.ascontiguousarray(np32(grad_y).T), np.ascontiguousarray(np32(z).T), np32(l.b)
            d32 = np.ascontiguousarray(np32(dz32).T)
            if self.finite_step:
                assert np.isfinite(dY).all() and np.isfinite(np32(l.W.grad)).all() and np.isfinite(np32(l.b.grad)).all(), self.what(i, "non-finite backward")
            if act == E.GELU:
                ok, meas = gelu_bwd_ok(E._u(Z, bh), dY, d32)
                assert ok, self.what(i, "gelu dz", meas)
            else:
                assert same_where_finite(d32, E.bwd_f32(dY, Z, bh, act)), self.what(i, "dz32")
            assert same_where_finite(np32(l.b.grad), E.dbias_of(d32)), self.what(i, "bias.grad")
            fin = np.isfinite(d32)
            got, want = E.bits(stored(dzop).T), E.bits(E.rne_bits(d32, EDT[op]))
            assert dzop.dtype == op and np.array_equal(got[fin], want[fin]), self.what(i, "dz rounds dz32")
            # the products on dz in the operand type
            with np.errstate(invalid="ignore", over="ignore"):
                d64, x64 = np32(dzop).astype(np.float64), np32(x).astype(np.float64)
                ref, bound = g.sample(d64.T @ x64), 1e-5 * g.sample(np.abs(d64).T @ np.abs(x64))
                ref[~g.inside], bound[~g.inside] = 0.0, 0.0
            G = np32(l.W.grad).astype(np.float64)
            dead = g.element_dead(self.keeps[i])
            skipped = dead if m.arm != "mask" else np.zeros_like(dead)
            assert not ubits(G)[~g.inside].any(), self.what(i, "W.grad past cols")
            if m.arm != "mask":
                assert not ubits(G)[dead].any(), self.what(i, "W.grad of a dead block, straight out of backward")
            assert close_where_finite(G, np.where(skipped, 0.0, ref), np.where(skipped, 0.0, bound), free=skipped | ~g.inside), self.what(i, "W.grad")
            # grad_x = dz @ A, returned in x.dtype: through the rounding interval
            A = g.dense(np32(l.W), l.dtype)
            with np.errstate(invalid="ignore", over="ignore"):
                gx_ref, gx_bound = d64 @ A, 1e-5 * (np.abs(d64) @ np.abs(A))
            gx = (m.x.grad if i == 0 else m.h.grad)
            assert gx is not None and gx.dtype == x.dtype, self.what(i, "grad_x")
            fin = np.isfinite(gx_ref) & np.isfinite(gx_bound)
            lo, hi = (torch.from_numpy(np.where(fin, gx_ref + s * gx_bound, 0.0)).to(x.dtype).float().numpy() for s in (-1, 1))
            gxh = np32(gx)
            assert np.all(((gxh >= lo) & (gxh <= hi))[fin]), self.what(i, "grad_x")
            if self.finite_step:
                assert fin.all() and np.isfinite(gxh).all(), self.what(i, "non-finite grad_x")
        if not self.finite_step:
            assert all(not np.isfinite(np32(l.W.grad)).all() for l in m.layers), self.what("the planted Inf did not reach the gradients")

    def masked(self):
        m = self.m
        self.G = [np32(l.W.grad) for l in m.layers]
        for i, l in enumerate(m.layers):
            dead = l.g.element_dead(self.keeps[i])
            assert not ubits(self.G[i])[dead].any(), self.what(i, "the gradient of a dead block")
            assert np.array_equal(ubits(self.G[i])[~dead], ubits(np32(self.raw[i]))[~dead]), self.what(i, "the gradient of a live block changed")
        if m.arm == "mask" and any(k.min() == 0 for k in self.keeps):
            assert any(np32(r)[l.g.element_dead(k)].any() for r, l, k in zip(self.raw, m.layers, self.keeps)), self.what("no dead block had a gradient to mask")

    # 5: control
    def collected(self):
        m = self.m
        grads = self.G + [np32(l.b.grad) for l in m.layers]
        all_g = np.concatenate([g.reshape(-1) for g in grads])
        want_ssq, want_bad = stats_ref(all_g)
        r = m.ctl.read()
        assert r["nonfinite"] == want_bad and (want_bad == 0) == self.finite_step, self.what("nonfinite", r["nonfinite"], want_bad)
        assert abs(r["ssq"] - want_ssq) <= len(all_g) * 2.0 ** -53 * want_ssq, self.what("ssq", r["ssq"], want_ssq)          # (`within` of tests/test_grad_ctl_gpu.py)
        before = self.words_before.copy()
        before[0:4] = r["words"][0:4]                                # the device's own statistics
        want = grad_ctl_ref(before, CTL_CFG)
        assert np.array_equal(r["words"], want), self.what("record", record_fields(r["words"]), record_fields(want))
        assert r["skip"] == (0 if self.finite_step else 1)
        if self.finite_step:
            assert 0.0 < r["coef"] < 1.0 / record_fields(before)["loss_scale"], self.what("the clip is not at work", r["coef"])
        self.record = r


def run_eager(name, arm):
    """the five steps with every check; returns the trace: per step the state after the step and after its prune (None without one)"""
    m = Model(name, arm)
    trace = []
    keeps = [np.ones(l.g.nb, np.uint8) for l in m.layers]
    try:
        assert [l.H.n_blocks for l in m.layers] == [l.g.nb for l in m.layers]
        words = m.ctl.read()["words"]
        prev = None
        for step in range(1, STEPS + 1):
            m.load(step)
            m.x.requires_grad_(True)
            m.x.grad = None
            chk = Checker(m, step, keeps)
            chk.words_before = words
            if step == INF_STEP:
                assert keeps[1][m.l2.g.brow == m.l2.g.strong].all() and min(k.min() for k in keeps) == 0, (name, arm, "the Inf must meet live blocks only")
            before = {"b%d" % i: np32(l.b) for i, l in enumerate(m.layers)}
            m.step(chk)
            snap = m.snapshot()
            r = chk.record
            words = snap["R"][:16].view(np.uint32).copy()
            assert np.array_equal(words, r["words"]), (name, arm, step, "the step wrote the record")
            # 6: the step
            for i, l in enumerate(m.layers):
                dead = l.g.element_dead(keeps[i])
                names = ["%s%d" % (c, i) for c in "WMVS"]
                if prev is None:
                    old = (l.g.W0, np.zeros(l.g.nz, f32), np.zeros(l.g.nz, f32), np.zeros(8, np.uint32))
                else:
                    old = tuple(prev[k] for k in names)
                if r["skip"]:
                    want = old
                else:
                    want = adam_ref(old[0], np.asarray(chk.G[i], f32) * f32(r["coef"]), old[1], old[2], old[3], ADAM)          # (`scaled(G, 1, coef)` of tests/test_grad_ctl_gpu.py)
                for k, wv in zip(names, want):
                    assert np.array_equal(snap[k].view(np.uint32), np.asarray(wv).view(np.uint32)), (name, arm, step, k)
                    assert np.isfinite(snap[k]).all() if k[0] != "S" else True, (name, arm, step, k, "non-finite")
                    if k[0] != "S":
                        assert not snap[k].view(np.uint32)[dead].any(), (name, arm, step, k, "a dead block is not +0")
                info = l.H.step_info()
                assert info["fused"] == l.spec["fused"], (name, arm, step, i, info)
                assert info["live"] == (1 if arm == "live" and step > min(PRUNE_AFTER) else 0), (name, arm, step, i, info)          # a live step once a live set is installed
                # the bias: b - (LR_B * coef) * grad, two roundings; untouched on a skipped step
                b0, gb = before["b%d" % i], np32(l.b.grad)
                wb = b0 if r["skip"] else b0 - (f32(LR_B) * f32(r["coef"])) * gb
                assert np.array_equal(ubits(snap["b%d" % i]), ubits(wb)), (name, arm, step, "b%d" % i)
            entry = {"step": snap, "prune": None}
            # 7: pruning
            if step in PRUNE_AFTER:
                s = PRUNE_AFTER[step]
                scores = [l.g.scores(snap["W%d" % i]) for i, l in enumerate(m.layers)]
                m.pruner.prune(s)
                after = m.snapshot()
                new = [after["keep%d" % i] for i in range(2)]
                total = sum(l.g.nb for l in m.layers)
                assert all(np.all(n <= k) for n, k in zip(new, keeps)) and sum(int((n == 0).sum()) for n in new) == math.floor(s * total), (name, arm, step)
                sc, gone, newly = np.concatenate(scores), np.concatenate(new) == 0, (np.concatenate(new) == 0) & (np.concatenate(keeps) == 1)
                assert sc[newly].max() <= sc[~gone].min() * (1 + 1e-12), (name, arm, step, "a kept block scores below a pruned one")
                assert all(np.array_equal(a, b) for a, b in zip(new, select_host(scores, keeps, s))), (name, arm, step, "the masks are not those of select")
                keeps = [n.copy() for n in new]
                for i, l in enumerate(m.layers):
                    dead = l.g.element_dead(keeps[i])
                    for k in ("W%d" % i, "M%d" % i, "V%d" % i):
                        assert not after[k].view(np.uint32)[dead].any(), (name, arm, step, k, "after prune")
                        assert np.array_equal(after[k].view(np.uint32)[~dead], snap[k].view(np.uint32)[~dead]), (name, arm, step, k, "prune changed a live block")
                    assert not ubits(np32(l.W.grad))[dead].any()
                    assert l.H.live_info()["installed"] == (0 if arm == "mask" else 1)
                entry["prune"] = after
                snap = after
            trace.append(entry)
            prev = snap
        # the conditions on the inputs
        skips = [int(e["step"]["R"][8]) for e in trace]
        scales = [float(e["step"]["R"][4:5].view(f32)[0]) for e in trace]
        assert skips == [0, 0, 1, 0, 0] and int(trace[-1]["step"]["R"][9]) == 1
        assert scales == [1024.0, 2048.0, 1024.0, 1024.0, 2048.0], scales          # grown after step 2, backed off at step 3, grown again by step 5
        for l, k in zip(m.layers, keeps):
            assert not k[l.g.weak].any(), (name, arm, "the weak block-row / block column is not wholly dead")
            assert k.max() == 1 and int((k == 0).sum()) > len(l.g.weak), (name, arm, "both layers lose blocks beyond the weak ones, and keep some")
        # 1, once more: the images the last step wrote, through the next forward
        m.load(STEPS)
        with torch.no_grad():
            chk = Checker(m, STEPS + 1, keeps)
            m.h = m.l1.forward(m.x.detach())
            chk.fwd1()
            m.y = m.l2.forward(m.h)
            chk.fwd2()
        return trace
    finally:
        m.close()


def eager(name, arm):
    if (name, arm) not in _EAGER:
        _EAGER[(name, arm)] = run_eager(name, arm)
    return _EAGER[(name, arm)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_mlp_step(name, monkeypatch):
    for var in ("SPARTA_SGD_FUSE", "SPARTA_ADAM_FUSE"):
        monkeypatch.delenv(var, raising=False)
    traces = {arm: eager(name, arm) for arm in ARMS}
    # 8: across the arms
    for arm in ARMS[1:]:
        for step, (a, b) in enumerate(zip(traces[ARMS[0]], traces[arm]), 1):
            assert same_state(a["step"], b["step"]) == [], (name, arm, step)
            assert (a["prune"] is None) == (b["prune"] is None) and (a["prune"] is None or same_state(a["prune"], b["prune"]) == []), (name, arm, step, "prune")
    print("mlp stack %s: largest GELU measures so far (y, dz): kernel %.3f %.3f   torch CPU float32 %.3f %.3f"
          % (name, GELU_SEEN["y"], GELU_SEEN["dz"], GELU_SEEN["torch_y"], GELU_SEEN["torch_dz"]))


# ---- graph capture: last in the file ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_mlp_step_replays(name, monkeypatch):
    """the live arm once more: steps 1 and 2 and the first prune eagerly on a side stream (first calls allocate; whether a live set is installed is host
    state that a capture fixes), then ONE whole step captured -- forward, backward, collect, opt.step(ctl=), the bias update -- and replayed for the steps
    3 to 5 with new x and gy and the eager prune(0.75) in between.  After every replay, and after the prune, all state equals the eager run's bit for bit: the
    skipped step, the back-off of the scale and the second prune included.  Every check stands before the next device work: a failed one ends the test."""
    for var in ("SPARTA_SGD_FUSE", "SPARTA_ADAM_FUSE"):
        monkeypatch.delenv(var, raising=False)
    trace = eager(name, "live")
    m = Model(name, "live")
    try:
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for step in (1, 2):
                m.load(step)
                m.step()
                assert same_state(m.snapshot(), trace[step - 1]["step"]) == [], (name, step, "eager")
                if step in PRUNE_AFTER:
                    m.pruner.prune(PRUNE_AFTER[step])
                    assert same_state(m.snapshot(), trace[step - 1]["prune"]) == [], (name, step, "eager prune")
            saved = {k: t.detach().clone() for k, t in m.state_tensors().items()}
            m.opt.zero_grad()
            m.l1.b.grad = m.l2.b.grad = None
            m.h = m.y = None
            torch.cuda.synchronize()
            gph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gph, stream=s):
                m.step()
            with torch.no_grad():
                for k, t in m.state_tensors().items():
                    t.copy_(saved[k])
            torch.cuda.synchronize()
            assert same_state(m.snapshot(), trace[1]["step"]) == [], (name, "a capture runs nothing, and the snapshot is back")
            for step in range(3, STEPS + 1):
                m.load(step)
                torch.cuda.synchronize()
                gph.replay()
                assert same_state(m.snapshot(), trace[step - 1]["step"]) == [], (name, step, "replay")
                if step in PRUNE_AFTER:
                    m.pruner.prune(PRUNE_AFTER[step])
                    assert same_state(m.snapshot(), trace[step - 1]["prune"]) == [], (name, step, "prune between replays")
            assert [l.H.step_info()["live"] for l in m.layers] == [1, 1]
        torch.cuda.synchronize()
    finally:
        m.close()
