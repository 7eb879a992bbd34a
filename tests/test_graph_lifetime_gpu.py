"""A graph captured from a call on a handle stays valid for as long as the handle lives (include/sparta_amd.h, under sparta_vbs_spmm): it replays
with the result of the eager call it was captured from, whatever other calls -- other n_cols, leading dimensions, layouts, slab heights, host-pointer calls --
are made on the handle between replays.  What could break it: scratch that a larger shape outgrows (freed while the graph holds its address), the step lists of
a gathered B (rewritten for another slab height), the reference-layout image of an fp32 handle (dropped once the no-barrier kernel carries the products).

One helper runs every case: shape S eagerly and captured, the larger shape L eagerly (held to the oracle under the suite's bound, 1e-5 * sum |a||b|, on
16-bit handles over the rounded operands, as tests/test_spmm_gpu.py does), then the GUARD, then replays with poisoned outputs, then close().  The guard reads
sparta_debug_device_allocs around L: the bytes rose (the case did make scratch grow) and the count of live allocations rose (the outgrown buffer was retired,
not freed: free-and-allocate leaves the count where it was) -- by more than on a twin handle that makes the same two calls and is never captured, since a
call may also make fresh allocations.  It stands BEFORE the first replay, so a library that frees never replays a graph with a dangling address here: the
test ends at the guard.  The gathered case is the exception the kernels allow: with the larger height's lists the captured launch reads rows of wrong slabs
but stays inside its own buffer, so there the replay itself is the check.

Shapes are the smallest the suite already uses for each kind of scratch; every case first asserts, from the handle's own records, that it has the plan the
case is about."""
import numpy as np
import pytest

import sparta_amd as sa
from oracle import oracle as O
import _util as U
import _lifecycle as L
from test_device_alloc_gpu import allocs
from test_union_host import clustered, true_grouping

pytestmark = pytest.mark.gpu
f32 = np.float32
TOL = 1e-5
ID = {sa.F32: "f32", sa.F16: "f16", sa.BF16: "bf16"}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU test on a box without a GPU"
    return torch


def _tdt(torch, dtype):
    return {sa.F32: torch.float32, sa.F16: torch.float16, sa.BF16: torch.bfloat16}[dtype]


def _round(x, dtype):
    return np.ascontiguousarray(x, f32) if dtype == sa.F32 else U.edge_round(x, dtype).astype(f32)


def _env(monkeypatch, **kv):
    """every block-row on the MFMA tiles unless a case says otherwise (the matrices are small: the library would keep them on one kind of launch)"""
    base = {"SPARTA_SPARSE_K": "0", "SPARTA_LAUNCH_NNZ": "0", "SPARTA_COLRES": "0"}
    base.update(kv)
    for k in ("SPARTA_PATH", "SPARTA_STREAM_ALIGN", "SPARTA_SPARSE_MIN_STEPS", "SPARTA_H16_PATH", "SPARTA_CSTAGE", "SPARTA_SP_INPLACE"):
        monkeypatch.delenv(k, raising=False)
    for k, val in base.items():
        if val is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, val)


class Ref:
    """the oracle's side of one matrix: the five arrays, the values as the handle's type holds them, and per (n, seed) the operand, the product, the bound"""

    def __init__(self, arrays, dtype):
        self.rows, self.cols, self.w, self.row_part, self.nzcount, self.jab, mab = arrays
        self.dtype = dtype
        self.mab = _round(mab, dtype)
        self._made = {}

    @classmethod
    def of_vbr(cls, v, dtype, mab=None):
        return cls((int(v.rows), int(v.cols), int(v.block_col_size), v.row_part, v.nzcount, v.jab, v.mab if mab is None else mab), dtype)

    def operand(self, n, seed):
        """(B as the device rounds it, flat column-major cols x n; the oracle's C; the bound) -- computed once per (n, seed)"""
        if (n, seed) not in self._made:
            B = _round(sa.gen.dense_rhs(self.cols, n, seed=seed), self.dtype)
            a = (self.rows, self.cols, self.w, self.row_part, self.nzcount, self.jab)
            self._made[(n, seed)] = (B, O.vbr_multiply(*a, self.mab, B, n, None), U.abs_bound(*a, self.mab, B, n))
        return self._made[(n, seed)]

    def check(self, C, n, seed, what):
        _, Co, bound = self.operand(n, seed)
        err = np.abs(np.asarray(C, f32) - Co)
        print("%s: max |err| %.3e, max bound %.3e" % (what, float(err.max()), float(TOL * bound.max())))
        bad = err > TOL * bound + 1e-30
        assert not bad.any(), "%s: %d elements outside tolerance, max err %.3e" % (what, int(bad.sum()), float(err.max()))


def _device_b(torch, B, cols, n, ldb, dtype):
    """the column-major operand with leading dimension ldb, in the handle's type (B holds representable values: the conversion is exact)"""
    Bt = torch.zeros(ldb * n, dtype=_tdt(torch, dtype), device="cuda")
    Bt.view(n, ldb)[:, :cols] = torch.from_numpy(B.reshape(n, cols)).cuda().to(_tdt(torch, dtype))
    return Bt


def _gathered_b(torch, B, cols, n, shard_rows, dtype):
    """the all-gather form: cols / shard_rows column-major slabs of shard_rows x n, back to back"""
    Bg = torch.zeros(cols * n, dtype=_tdt(torch, dtype), device="cuda")
    full = torch.from_numpy(B.reshape(n, cols)).cuda().to(_tdt(torch, dtype))
    for s in range(cols // shard_rows):
        Bg[s * shard_rows * n:(s + 1) * shard_rows * n].view(n, shard_rows)[:] = full[:, s * shard_rows:(s + 1) * shard_rows]
    return Bg


class Call:
    """one product on a handle: run(C) launches it on the current stream into the device tensor C (c_elems float32); check(C): against the oracle, or None"""

    def __init__(self, run, c_elems, check=None, capturable=True):
        self.run, self.c_elems, self.check, self.capturable = run, c_elems, check, capturable


def spmm_call(torch, h, ref, n, seed, ldb=None, what=""):
    B, _, _ = ref.operand(n, seed)
    ldb = ref.cols if ldb is None else ldb
    Bt = _device_b(torch, B, ref.cols, n, ldb, ref.dtype)
    return Call(lambda C: h.spmm(Bt, C, n, ldb=ldb), ref.rows * n, lambda C: ref.check(C.cpu().numpy(), n, seed, what or "n = %d, ldb = %d" % (n, ldb)))


def gathered_call(torch, h, ref, n, seed, shard_rows):
    B, _, _ = ref.operand(n, seed)
    Bg = _gathered_b(torch, B, ref.cols, n, shard_rows, ref.dtype)
    return Call(lambda C: h.spmm_gathered(Bg, shard_rows, C, n), ref.rows * n, lambda C: ref.check(C.cpu().numpy(), n, seed, "gathered, slabs of %d rows" % shard_rows))


def host_call(torch, h, ref, n, seed):
    """a host-pointer product (fp32 B in, rounded on the device): its result goes through a host array into C"""
    B, _, _ = ref.operand(n, seed)

    def run(C):
        Ch = np.zeros(ref.rows * n, f32)
        h.spmm_host(B, n, Ch, accumulate=False)
        C.copy_(torch.from_numpy(Ch))
    return Call(run, ref.rows * n, lambda C: ref.check(C.cpu().numpy(), n, seed, "host pointers, n = %d" % n), capturable=False)


RETIRED = {}          # case -> bytes its handle retired (printed; profiles/graph_lifetime/README.md records them)


def scratch_grew(h, a0, a1, t0, t1, what):
    """the guard of a scratch case (module docstring).  (t0, t1): the same larger call on the twin that was never captured, where outgrown scratch is freed --
    the captured handle must hold MORE allocations than that (a call that also makes fresh allocations, as a host-pointer call does, raises the count either
    way); None: the call makes no fresh allocation"""
    assert a1[1] > a0[1], "%s: the larger shape allocated nothing (%s -> %s): the case does not make scratch grow" % (what, a0, a1)
    assert a1[0] > a0[0], ("%s: scratch grew but the count of live allocations did not (%s -> %s): the outgrown buffer was freed while a captured graph "
                           "holds its address" % (what, a0, a1))
    if t0 is not None:
        kept, kept_bytes = (a1[0] - a0[0]) - (t1[0] - t0[0]), (a1[1] - a0[1]) - (t1[1] - t0[1])
        assert kept > 0 and kept_bytes > 0, ("%s: the captured handle holds no more than one that was never captured (%s -> %s against %s -> %s): it freed "
                                             "what it outgrew" % (what, a0, a1, t0, t1))
        RETIRED[what] = kept_bytes
        print("%s: %d buffers retired, %d bytes" % (what, kept, kept_bytes))


def lists_added(h, a0, a1, t0, t1, what):
    """the gathered case: the second slab height allocated lists of its own"""
    assert a1[1] > a0[1], "%s: the second slab height allocated nothing (%s -> %s)" % (what, a0, a1)


def never_captured(torch, open_case):
    """S, then L, eagerly on a handle of the case that is never captured: allocs() around L, and the handle's a_bytes after it"""
    h, small, large = open_case()
    try:
        small.run(torch.empty(small.c_elems, dtype=torch.float32, device="cuda"))
        t0 = allocs()
        large.run(torch.empty(large.c_elems, dtype=torch.float32, device="cuda"))
        torch.cuda.synchronize()
        return t0, allocs(), h.info()["a_bytes"]
    finally:
        h.close()


def lifetime(torch, open_case, guard, what):
    """steps 1 to 9 of the module docstring on the handle open_case() returns with its two calls (closed here, whatever happens)"""
    new = lambda k: torch.empty(k, dtype=torch.float32, device="cuda")      # noqa: E731
    nan = float("nan")
    t0, t1, _ = never_captured(torch, open_case)
    opened_at = allocs()
    h, small, large = open_case()
    try:
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            C_ref, C_g1 = new(small.c_elems), new(small.c_elems)
            small.run(C_ref)                                                 # 1: eager (tuning, scratch, lists)
            torch.cuda.synchronize()
            small.check(C_ref)
            g1 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g1, stream=s):                             # 2
                small.run(C_g1)
            a0 = allocs()                                                    # 3
            C_L = new(large.c_elems)
            large.run(C_L)                                                   # 4: the larger shape, eagerly
            torch.cuda.synchronize()
            large.check(C_L)
            a1 = allocs()                                                    # 5
            print("%s: device allocations (count, bytes) %s before the larger shape, %s after" % (what, a0, a1))
            guard(h, a0, a1, t0, t1, what)                                   # 6: BEFORE any replay
            C_g1.fill_(nan)                                                  # 7
            g1.replay()
            torch.cuda.synchronize()
            assert torch.equal(C_g1, C_ref), what + ": the first replay after the larger shape"
            replays = [(g1, C_g1, C_ref)]                                    # 8
            if large.capturable:
                C_g2 = new(large.c_elems)
                g2 = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g2, stream=s):
                    large.run(C_g2)
                replays = [(g1, C_g1, C_ref), (g2, C_g2, C_L), (g1, C_g1, C_ref)]
            else:
                large.run(C_L)                                               # (a host-pointer call cannot be captured: once more between two replays)
                replays = replays * 2
            for i, (g, out, want) in enumerate(replays):
                out.fill_(nan)
                g.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, want), "%s: replay %d of the second round" % (what, i)
        torch.cuda.synchronize()
    finally:
        h.close()
    assert allocs() == opened_at, what + ": the handle kept device memory (retired buffers included)"    # 9


_GEO_REFS = {}


def _training_geometry(geo):
    """(dtype, pattern and values, the oracle's side) of a geometry of tests/_lifecycle.py; the oracle's products are shared by the tests that use it"""
    dtype, v = L.GEOS[geo][0], L.geometry(geo)
    if geo not in _GEO_REFS:
        _GEO_REFS[geo] = Ref.of_vbr(v, dtype)
    return dtype, v, _GEO_REFS[geo]


def _uniform_vbr(rows, cols, nnz, w, blk):
    m = sa.gen.uniform_random(rows, cols, nnz, seed=rows + w)
    return sa.VBR().fill_from_CSR_inplace(m, np.arange(rows) // blk, w)


# ---- d_Bt: the zero-padded tail slab of a 16-bit product with n_cols % 128 != 0 grows with the leading dimension of B -------------------------------------
@pytest.mark.parametrize("geo", ["w96", "w128"])
def test_tail_slab_outgrown_by_a_wider_leading_dimension(monkeypatch, geo):
    torch = _torch()
    _env(monkeypatch)
    dtype, v, ref = _training_geometry(geo)

    def open_case():
        h = v.to_device(0, dtype=dtype)
        assert h.info()["stream_steps"] > 0
        return h, spmm_call(torch, h, ref, 72, 61), spmm_call(torch, h, ref, 72, 61, ldb=2 * ref.cols)
    lifetime(torch, open_case, scratch_grew, "tail slab, %s %s" % (ID[dtype], geo))


# ---- the same handle, a host-pointer call in between: it allocates d_B, d_C, d_B16 and, at its larger n_cols, outgrows the tail panel the graph launches with ---
def test_host_pointer_call_between_replays(monkeypatch):
    torch = _torch()
    _env(monkeypatch)
    dtype, v, ref = _training_geometry("w96")

    def open_case():
        h = v.to_device(0, dtype=dtype)
        assert h.info()["stream_steps"] > 0
        return h, spmm_call(torch, h, ref, 72, 61), host_call(torch, h, ref, 384, 62)
    lifetime(torch, open_case, scratch_grew, "host-pointer call in between")


# ---- d_btail: the zero-padded copy of B's last block row (cols % w != 0) grows with n_cols --------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [sa.F32, sa.BF16], ids=["f32", "bf16"])
def test_tail_panel_outgrown_by_more_columns(monkeypatch, dtype):
    torch = _torch()
    _env(monkeypatch, SPARTA_PATH="stream")
    v = _uniform_vbr(1500, 1000 - 7, 40000, 32, 32)
    ref = Ref.of_vbr(v, dtype)
    ldb = ref.cols + 1                                                           # (even: what a 16-bit operand needs)

    def open_case():
        h = v.to_device(0, dtype=dtype)
        info = h.info()
        assert info["stream_steps"] > 0 and info["sparse_rows"] == 0 and ref.cols % ref.w != 0, info
        return h, spmm_call(torch, h, ref, 128, 63, ldb=ldb), spmm_call(torch, h, ref, 384, 64, ldb=ldb)
    lifetime(torch, open_case, scratch_grew, "tail panel, " + ID[dtype])


# ---- d_ws: the partial images of split tiles grow with n_cols -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [sa.F32, sa.F16], ids=["f32", "f16"])
def test_split_tile_workspace_outgrown_by_more_columns(monkeypatch, dtype):
    torch = _torch()
    _env(monkeypatch, SPARTA_PATH="stream", SPARTA_STREAM_ALIGN="0")
    v = _uniform_vbr(64, 6400, 30000, 64, 64)                                    # ONE long tile (tests/test_spmm_gpu.py, test_stream_plan_modes): split between the workers
    ref = Ref.of_vbr(v, dtype)

    def open_case():
        h = v.to_device(0, dtype=dtype)
        assert h.info()["split_tiles"] > 0, h.info()
        return h, spmm_call(torch, h, ref, 128, 65), spmm_call(torch, h, ref, 384, 66)
    lifetime(torch, open_case, scratch_grew, "split-tile workspace, " + ID[dtype])


# ---- d_sp_part and d_Brm: the partial rows of the long sparse rows and the row-major copy of a column-major B grow with n_cols -------------------------------------
def _power_law(long_=16, win=512):
    """the 600 x 9013 matrix of test_sparse_rows_cut_at_column_windows_and_taken_window_by_window (tests/test_spmm_gpu.py), its (512, 16, 4) case"""
    rng = np.random.Generator(np.random.PCG64(win + long_))
    rows, cols = 600, 9000 + 13
    rr, cc = [], []
    for i in range(rows - 10):
        k = int(rng.integers(0, 4 * long_ + 40)) if i % 7 else 0
        c = np.unique(np.minimum((cols * rng.random(k) ** 2.5).astype(np.int64), cols - 1))
        rr.append(np.full(len(c), i)); cc.append(c)
    rr.append(np.full(7000, rows - 10)); cc.append(rng.choice(cols, 7000, replace=False))
    r, c = np.concatenate(rr), np.concatenate(cc)
    order = np.lexsort((c, r))
    r, c = r[order], c[order]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=rows))])
    return sa.CSR(rows, cols, rowptr, c.astype(np.int32), rng.uniform(-1, 1, len(c)).astype(f32))


@pytest.mark.parametrize("dtype", [sa.F32, sa.BF16], ids=["f32", "bf16"])
def test_sparse_row_scratch_outgrown_by_more_columns(monkeypatch, dtype):
    torch = _torch()
    _env(monkeypatch, SPARTA_SPARSE_K=None, SPARTA_SPARSE_MIN_STEPS="0", SPARTA_SP_WINDOW_COLS="512", SPARTA_SP_LONG="16", SPARTA_SP_MINSEG="4")
    m, w = _power_law(), 32
    g = np.arange(m.rows) // 32
    ref = Ref.of_vbr(sa.VBR().fill_from_CSR_inplace(m, g, w), dtype)
    ldb = (ref.cols + 7) // 8 * 8

    def open_case():
        h = sa.DeviceVBS.from_csr(m, g, w, 0, False, device=0, dtype=dtype)
        sp = h.sparse_info()
        assert sp["hub_rows"] > 0 and sp["nnz"] * 8 >= ref.cols, sp              # long rows (partial rows), and too many nonzeros to gather a column-major B in place
        return h, spmm_call(torch, h, ref, 128, 67, ldb=ldb), spmm_call(torch, h, ref, 256, 68, ldb=ldb)
    lifetime(torch, open_case, scratch_grew, "sparse rows, " + ID[dtype])


# ---- d_Brm under the column-compacted tiles -------------------------------------------------------------------------------------------------------------------------
def test_row_major_copy_for_union_tiles_outgrown_by_more_columns(monkeypatch):
    torch = _torch()
    _env(monkeypatch, SPARTA_SPARSE_K=None, SPARTA_COLRES=None, SPARTA_SPARSE_MIN_STEPS="0")      # the settings of csr_union in tests/test_device_alloc_gpu.py
    m, order = clustered(40, 5, 5000, 100, 3, seed=16, integer=True)
    g = true_grouping(order, 5)
    ov = O.OracleVBR(m.rows, m.cols, m.rowptr, m.colidx, m.vals, g, 1)
    ref = Ref((ov.rows, ov.cols, 1, ov.row_part, ov.nzcount, ov.jab, ov.mab), sa.F32)

    def open_case():
        h = sa.DeviceVBS.from_csr(m, g, 1, device=0)
        assert h.union_info()["area"] > 0, h.union_info()
        return h, spmm_call(torch, h, ref, 72, 69), spmm_call(torch, h, ref, 384, 70)
    lifetime(torch, open_case, scratch_grew, "union tiles")


# ---- the step lists of a gathered B: one set per slab height, never rewritten ---------------------------------------------------------------------------------------------
def _hub_vbr(monkeypatch):
    """the smallest hub shape of test_16bit_hub_group_tiles_against_the_oracle (tests/test_spmm_gpu.py), groups of two"""
    for k, val in (("SPARTA_HUB", "1"), ("SPARTA_HUB_G", "2"), ("SPARTA_HUB_MIN_TOTAL", "0"), ("SPARTA_HUB_MIN_STEPS", "16"), ("SPARTA_HUB_DEAL", "0"), ("SPARTA_HUB_TAU", "0.25")):
        monkeypatch.setenv(k, val)
    rows, cols, nnz, n = 640, 6400, 260000, 256
    m = sa.gen.uniform_random(rows, cols, nnz, seed=rows + cols + n)
    return sa.VBR().fill_from_CSR_inplace(m, np.arange(rows) // 64, 64)


@pytest.mark.parametrize("kind,dtype", [("stream", sa.F32), ("stream", sa.F16), ("hub", sa.F16)], ids=["f32", "f16", "f16-hub"])
def test_gathered_step_lists_of_two_slab_heights(monkeypatch, kind, dtype):
    """smaller height captured first: with the lists of the larger height the captured launch stays inside its own buffer (module docstring)"""
    torch = _torch()
    _env(monkeypatch, SPARTA_PATH="stream")
    v = _hub_vbr(monkeypatch) if kind == "hub" else _uniform_vbr(3000, 640, 20000, 32, 32)
    ref = Ref.of_vbr(v, dtype)
    assert ref.cols % (4 * ref.w) == 0

    def open_case():
        h = v.to_device(0, dtype=dtype)
        assert h.info()["stream_steps"] > 0 or kind == "hub", h.info()
        assert (h.hub_info()["steps"] > 0) == (kind == "hub"), h.hub_info()
        return h, gathered_call(torch, h, ref, 128, 71, ref.cols // 4), gathered_call(torch, h, ref, 128, 71, ref.cols // 2)
    lifetime(torch, open_case, lists_added, "gathered step lists, %s %s" % (ID[dtype], kind))


# ---- the reference-layout image of an fp32 handle: dropped once the no-barrier kernel carries the products, unless a graph may read it ----------------------------------------
def test_reference_layout_image_is_kept_once_a_graph_may_read_it(monkeypatch):
    """S reads the reference-layout image of A (a row-major B); L is the first product of the no-barrier kernel (a column-major B), after which a handle that
    was never captured drops that image (drop_legacy_image, vbs_capi.cpp) -- the twin shows it, or the case is vacuous.  The guard: the captured handle
    freed nothing."""
    torch = _torch()
    _env(monkeypatch, SPARTA_PATH="stream")
    v = _uniform_vbr(1500, 1000 - 7, 40000, 32, 32)
    ref = Ref.of_vbr(v, sa.F32)
    n, legacy = 128, (int(v.mab.size) + 128) * 4
    B, _, _ = ref.operand(n, 72)
    Bcm = torch.from_numpy(B).cuda()
    Brm = torch.from_numpy(np.ascontiguousarray(B.reshape(n, ref.cols).T).reshape(-1)).cuda()
    check = lambda C: ref.check(C.cpu().numpy(), n, 72, "reference-layout image")      # noqa: E731
    two = []

    def open_case():
        h = v.to_device(0)
        two.append(h.info()["a_bytes"])
        return h, Call(lambda C: h.spmm(Brm, C, n, b_layout=sa.ROW_MAJOR), ref.rows * n, check), Call(lambda C: h.spmm(Bcm, C, n), ref.rows * n, check)

    def kept(h, a0, a1, t0, t1, what):
        assert t1[1] == t0[1] - legacy and t1[0] == t0[0] - 1, "%s: a handle that was never captured keeps the image anyway (%s -> %s): the case is vacuous" % (what, t0, t1)
        assert h.info()["a_bytes"] == two[-1] and a1 == a0, \
            "%s: the handle freed device memory (%s -> %s, a_bytes %d -> %d) while a captured graph reads the reference-layout image" % (what, a0, a1, two[-1], h.info()["a_bytes"])
    lifetime(torch, open_case, kept, "reference-layout image")


# ---- end to end: a captured training step of one vbs_linear layer, a larger eager evaluation batch between its replays -----------------------------------------------------
def test_captured_training_step_survives_a_larger_eager_forward(monkeypatch):
    """f16 w96, bias + GELU, VbsAdamW: forward, backward (both products) and the optimizer step at batch 72, captured after one eager step and replayed three
    times with new x.  Between the second and the third replay the handle runs an eager forward product at batch 328 with twice the leading dimension (it outgrows
    the tail slab and the tail panel the graph launches with), held to the oracle on the values the handle has by then.  A twin handle and optimizer replay the
    same recipe with no interruption: W, exp_avg, exp_avg_sq and the step words are the same bits after every replay."""
    torch = _torch()
    _env(monkeypatch)
    from sparta_amd.autograd import vbs_linear
    from sparta_amd.optim import VbsAdamW
    v, dtype, n = L.geometry("w96"), sa.F16, 72
    rows, cols = int(v.rows), int(v.cols)
    rng = np.random.default_rng(96)
    W0 = rng.uniform(-1, 1, int(v.nztot)).astype(f32)
    bias = torch.from_numpy(rng.uniform(-1, 1, rows).astype(f32)).cuda()
    gy = torch.from_numpy(rng.uniform(-1, 1, (n, rows)).astype(f32)).cuda()
    xs = [torch.from_numpy(rng.uniform(-1, 1, (n, cols)).astype(f32)).cuda().to(torch.float16) for _ in range(4)]
    before = allocs()

    class Side:
        def __init__(self):
            fresh = sa.VBR.from_arrays(v.rows, v.cols, v.block_col_size, v.row_part, v.nzcount, v.jab, W0)
            self.H = fresh.to_device(0, dtype=dtype, updatable=True, transposable=True)
            self.W = torch.from_numpy(W0).cuda().requires_grad_(True)
            self.x = xs[0].clone().requires_grad_(True)
            self.opt = VbsAdamW([(self.H, self.W)], lr=1e-2, weight_decay=0.01)
            self.g = None

        def step(self):
            y = vbs_linear(self.x, self.H, self.W, bias=bias, activation="gelu")
            y.backward(gy)
            self.opt.step()

        def state(self):
            s = self.opt._state[0]
            return [self.W.detach(), s["exp_avg"], s["exp_avg_sq"], s["state"]]

    a, b = Side(), Side()
    try:
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for side in (a, b):
                side.step()                                                      # eager, once
                side.opt.zero_grad()
                side.x.grad = None
                torch.cuda.synchronize()
                side.g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(side.g, stream=s):
                    side.step()

            def replay(i):
                for side in (a, b):
                    with torch.no_grad():
                        side.x.copy_(xs[i])
                    side.g.replay()
                torch.cuda.synchronize()
                for name, p, q in zip(("W", "exp_avg", "exp_avg_sq", "step words"), a.state(), b.state()):
                    assert torch.equal(p, q), "replay %d: %s differs from the uninterrupted twin's" % (i, name)
            replay(1)
            replay(2)
            # the larger eager forward on `a` alone: the product of the layer at batch 328, ldb = 2 cols
            ne, ldb = 328, 2 * cols
            ref = Ref.of_vbr(v, dtype, mab=a.W.detach().cpu().numpy())
            Be, _, _ = ref.operand(ne, 73)
            Bt = _device_b(torch, Be, cols, ne, ldb, dtype)
            Ce = torch.empty(rows * ne, dtype=torch.float32, device="cuda")
            a0 = allocs()
            with torch.no_grad():
                a.H.spmm(Bt, Ce, ne, ldb=ldb)
            torch.cuda.synchronize()
            ref.check(Ce.cpu().numpy(), ne, 73, "eager forward at batch 328 between two replays")
            a1 = allocs()
            print("captured training step: device allocations (count, bytes) %s before the larger forward, %s after" % (a0, a1))
            scratch_grew(a.H, a0, a1, None, None, "captured training step")      # the guard, before the third replay (no fresh allocation in this call: d_Ct exists)
            replay(3)
            assert not torch.equal(a.W.detach().cpu(), torch.from_numpy(W0))     # (the steps did move the values)
        torch.cuda.synchronize()
    finally:
        a.H.close(); b.H.close()
    assert allocs() == before, "a handle kept device memory"
