"""Training across a repattern: BlockPruner.compact and BlockPruner.grow under VbsAdamW and VbsSGD(momentum=0.9), through vbs_linear.

x holds small integers and the loss is (y * T).sum() with a small-integer T: the gradient of the values is T^T x sampled on the stored blocks -- exact in
fp32 whatever the order of additions, and independent of the forward values.  The steps are elementwise, so a block's values, momentum and Adam moments
depend on its own gradients alone: a run that compacts must hold, bit for bit, the live blocks of the run that does not; a run that grows must equal a run
on a handle created from scratch on the grown pattern, and the checkpoints must carry the new sizes."""
import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd.autograd import vbs_linear

torch = pytest.importorskip("torch")

import _util as U  # noqa: E402
import _repattern as R  # noqa: E402

pytestmark = pytest.mark.gpu

TDT = {sa.F32: torch.float32, sa.F16: torch.float16, sa.BF16: torch.bfloat16}
GEOS = [("w96", sa.F16), ("w13z", sa.F32)]
OPTS = ("adamw", "sgd")
N = 8
cases = pytest.mark.parametrize("geo,opt_kind", [(g, o) for g in GEOS for o in OPTS], ids=["%s-%s" % (g[0], o) for g in GEOS for o in OPTS])


def start_values(v):
    return (np.random.default_rng(515).integers(-8, 9, v.nztot) / 8.0).astype(np.float32)


def make_opt(kind, pairs):
    if kind == "adamw":
        return sa.VbsAdamW(pairs, lr=1e-2, weight_decay=0.01)
    return sa.VbsSGD(pairs, lr=1e-2, momentum=0.9)


def state_tensors(opt):
    """the optimizer's tensors in the values' layout, then the others"""
    if hasattr(opt, "_bufs"):
        return [opt._bufs[0]], []
    s = opt._state[0]
    return [s["exp_avg"], s["exp_avg_sq"]], [s["state"]]


class Run:
    def __init__(self, v, dtype, kind, values=None):
        self.v, self.dtype, self.t = v, dtype, 0
        handle = v.to_device(0, dtype=dtype, updatable=True, transposable=True)
        w = torch.from_numpy(start_values(v) if values is None else values).cuda().requires_grad_(True)
        self.opt = make_opt(kind, [(handle, w)])
        self.pruner = sa.BlockPruner(self.opt, skip_pruned=True)
        self.closed = [handle]

    @property
    def handle(self):
        return self.opt.pairs[0][0]

    @property
    def values(self):
        return self.opt.pairs[0][1]

    def steps(self, n):
        for _ in range(n):
            rng = np.random.default_rng(7000 + self.t)
            x = torch.from_numpy(rng.integers(-3, 4, (N, self.v.cols)).astype(np.float32)).to(TDT[self.dtype]).cuda()
            T = torch.from_numpy(rng.integers(-3, 4, (N, self.v.rows)).astype(np.float32)).cuda()
            handle, values = self.opt.pairs[0]
            y = vbs_linear(x, handle, values)
            (y * T).sum().backward()
            self.opt.step()
            self.opt.zero_grad()
            self.t += 1

    def words(self):
        """values and the state tensors in their layout as uint32, then the other state"""
        lay, other = state_tensors(self.opt)
        torch.cuda.synchronize()
        return [t.detach().cpu().numpy().view(np.uint32) for t in [self.values] + lay], [t.cpu().numpy() for t in other]

    def close(self):
        for h in self.closed + [self.handle]:
            h.close()


def geometry(key):
    return U.train_geometries()[key]


def two_free_blocks(v):
    """two blocks the pattern does not store, in block-rows of height > 0: the first free block column of the first block-row that has one, and the last free
    block column (the ragged one where it is free) of that block-row or, if it has no second one, of the next"""
    block_cols = (v.cols - 1) // int(v.block_col_size) + 1
    first = np.concatenate([[0], np.cumsum(v.nzcount)])
    out = []
    for ib in range(v.block_rows):
        stored = set(int(j) for j in v.jab[first[ib]:first[ib + 1]])
        free = [j for j in range(block_cols) if j not in stored]
        if v.row_part[ib + 1] > v.row_part[ib] and free:
            out += [(ib, free[0])] if not out else []
            if (ib, free[-1]) not in out:
                out.append((ib, free[-1]))
        if len(out) >= 2:
            return out[:2]
    raise AssertionError("the geometry stores all blocks but one")


@cases
def test_compaction_keeps_the_live_blocks_bit_for_bit(geo, opt_kind):
    key, dtype = geo
    v = geometry(key)
    a, b = Run(v, dtype, opt_kind), Run(v, dtype, opt_kind)
    try:
        for r in (a, b):
            r.steps(3)
            r.pruner.prune(0.5)
            r.steps(2)
        old_bytes, old_nztot = a.handle.info()["a_bytes"], a.handle.info()["nztot"]
        a.closed.append(a.handle)
        keep = a.pruner.keep_masks()[0].cpu().numpy()
        (new_v,) = a.pruner.compact([v])
        bmap = a.opt.last_map
        assert a.handle is not a.closed[-1] and a.values.grad is None and a.values.requires_grad and a.values.is_leaf
        assert np.array_equal(bmap, np.flatnonzero(keep)) and len(bmap) == len(keep) - len(keep) // 2
        assert a.pruner.keep_masks()[0].numel() == len(bmap) and bool(a.pruner.keep_masks()[0].all()) and a.pruner.sparsity() == 0.0
        assert a.pruner.probe(0).sel.numel() == len(bmap) and a.pruner.pairs[0][0] is a.handle
        assert a.handle.live_info()["installed"] == 0
        a.v = new_v
        a.steps(3)
        b.steps(3)
        (wa, oa), (wb, ob) = a.words(), b.words()
        assert len(wa) == (3 if opt_kind == "adamw" else 2)
        for ta, tb in zip(wa, wb):
            assert ta.size == new_v.nztot == a.handle.info()["nztot"] < old_nztot
            assert np.array_equal(ta, R.move_vbr(v, (new_v.nzcount, new_v.jab), bmap, 0, v.block_rows, tb))
        # what the other run holds outside the live blocks is zero: nothing was lost
        T = v.block_table()
        for q in np.flatnonzero(keep == 0):
            assert not wb[0][T[q, 0]:T[q, 0] + T[q, 2]].any()
        for sa_, sb_ in zip(oa, ob):
            assert np.array_equal(sa_, sb_)                                                  # Adam's step words: eight steps in both runs
        assert a.handle.info()["a_bytes"] < old_bytes
    finally:
        a.close()
        b.close()


@cases
def test_growth_equals_a_handle_created_on_the_grown_pattern(geo, opt_kind):
    key, dtype = geo
    v = geometry(key)
    a = Run(v, dtype, opt_kind)
    b = None
    try:
        a.steps(2)
        a.pruner.prune(0.5)
        a.steps(1)
        old_keep = a.pruner.keep_masks()[0].cpu().numpy()
        add = two_free_blocks(v)
        a.closed.append(a.handle)
        new_v = a.pruner.grow(0, v, add)
        bmap = a.opt.last_map
        a.v = new_v
        assert (bmap < 0).sum() == 2 and a.values.numel() == new_v.nztot and a.values.grad is None
        keep = a.pruner.keep_masks()[0].cpu().numpy()
        assert np.array_equal(keep[bmap >= 0], old_keep[bmap[bmap >= 0]]) and keep[bmap < 0].all()
        assert np.array_equal(a.pruner.probe(0).sel.cpu().numpy(), (keep == 0).astype(np.uint8))
        li = a.handle.live_info()
        assert li["installed"] == 1 and li["live_blocks"] == int(keep.sum())
        T = new_v.block_table()
        added = np.flatnonzero(bmap < 0)
        w0 = a.words()[0]
        for t in w0:
            assert all(not t[T[q, 0]:T[q, 0] + T[q, 2]].any() for q in added)                 # added blocks start as zeros, in values and in the state
        # the other run: a handle created from scratch on the grown pattern, everything loaded through the state dicts
        b = Run(sa.VBR.from_arrays(v.rows, v.cols, v.block_col_size, new_v.row_part, new_v.nzcount, new_v.jab, np.zeros(new_v.nztot, np.float32)), dtype, opt_kind,
                values=a.values.detach().cpu().numpy())
        b.t = a.t
        b.opt.load_state_dict(a.opt.state_dict())
        b.pruner.load_state_dict(a.pruner.state_dict())
        a.steps(1)
        first = a.words()[0][0]
        assert all(first[T[q, 0]:T[q, 0] + T[q, 1]].any() for q in added)                    # ... and have left zero after the first step
        a.steps(2)
        b.steps(3)
        (wa, oa), (wb, ob) = a.words(), b.words()
        for ta, tb in zip(wa, wb):
            assert np.array_equal(ta, tb)
        for sa_, sb_ in zip(oa, ob):
            assert np.array_equal(sa_, sb_)
        dead = np.flatnonzero(keep == 0)
        assert len(dead) and all(not wa[0][T[q, 0]:T[q, 0] + T[q, 2]].any() for q in dead)   # the pruned blocks stayed stored and zero
    finally:
        a.close()
        if b is not None:
            b.close()


@cases
def test_checkpoints_round_trip_on_the_new_sizes(geo, opt_kind):
    key, dtype = geo
    v = geometry(key)
    a = Run(v, dtype, opt_kind)
    b = None
    try:
        a.steps(2)
        a.pruner.prune(0.5)
        a.steps(1)
        a.closed.append(a.handle)
        (new_v,) = a.pruner.compact([v])
        a.v = new_v
        a.steps(1)
        a.pruner.prune(0.25)                                                                 # a mask of the new size that is not all ones
        osd, psd = a.opt.state_dict(), a.pruner.state_dict()
        assert psd["keep"][0].numel() == len(new_v.jab) and int((psd["keep"][0] == 0).sum()) == len(new_v.jab) // 4
        lay = osd["momentum_buffer"] if opt_kind == "sgd" else [osd["state"][0]["exp_avg"], osd["state"][0]["exp_avg_sq"]]
        assert all(t.numel() == new_v.nztot for t in lay)
        b = Run(new_v, dtype, opt_kind, values=a.values.detach().cpu().numpy())
        b.t = a.t
        b.opt.load_state_dict(osd)
        b.pruner.load_state_dict(psd)
        (wa, oa), (wb, ob) = a.words(), b.words()
        assert all(np.array_equal(x, y) for x, y in zip(wa + oa, wb + ob))
        assert torch.equal(a.pruner.keep_masks()[0], b.pruner.keep_masks()[0])
        old = Run(v, dtype, opt_kind)
        try:
            with pytest.raises(ValueError):
                old.pruner.load_state_dict(psd)                                              # the old sizes no longer fit
        finally:
            old.close()
        a.steps(2)
        b.steps(2)
        (wa, oa), (wb, ob) = a.words(), b.words()
        assert all(np.array_equal(x, y) for x, y in zip(wa + oa, wb + ob))
    finally:
        a.close()
        if b is not None:
            b.close()
