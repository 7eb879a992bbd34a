"""A numpy model of the life of block-sparse layers under dynamic sparse training -- step, prune, regrow, compact, grow, checkpoint -- keyed by BLOCK, not by
layout: per (handle, values) pair a dict (block-row, block column) -> {W, M, V, live} plus Adam's step words, and one control record for the run.  The
reference of tests/test_lifecycle_host.py (the conditions on the inputs) and tests/test_lifecycle_gpu.py (every arm of the device against it).

It rests on two facts tests/test_repattern_train_gpu.py already uses.  With small-integer x and the loss (y * T).sum() * loss_scale, the gradient of the
values is (T * loss_scale)^T x sampled on the stored blocks: integers, exact in fp32 and in the 16-bit operand types in any order of additions, and
independent of the forward values.  And the steps are elementwise.  So the state of a block depends on its own gradients alone: it is the same bits whether
the pruned blocks are masked, skipped by the backward products, skipped by the steps, or dropped from the pattern, and whether the forward product reads the
16-bit image or the fp8 image (whose backward is straight-through on the exact gradient).  The statistics of the control record are sums of squares of
integers below 2^53: exact in fp64 in any order, so the record is the same bits too.  Nothing here calls the library's repattern or move code: compact and
grow are dict operations, and layout() places the dict into the mab order of whatever VBR the device says it has."""
import math

import numpy as np

import sparta_amd as sa

import _util as U
from test_adam_step_host import adam_ref
from test_live_step_host import sgd_ref
from test_grad_ctl_host import stats_ref, grad_ctl_ref, fresh_record, record_fields

f32 = np.float32
N = 8
STEPS = 10
LOSS_SCALE, MAX_NORM, GROWTH_INTERVAL = 4.0, 1.0, 2
CTL_CFG = dict(max_norm=MAX_NORM, growth_interval=GROWTH_INTERVAL)
HYPER = {"adamw": dict(lr=1e-2, weight_decay=0.01), "sgd": dict(lr=1e-2, momentum=0.9)}
INF_STEP, INF_SAMPLE = 5, 3
# what follows a step; compact and grow only in the runs that repattern, the checkpoint only in the runs that ask for it
AFTER = {2: ("prune", 0.5), 4: ("regrow", 0.25), 5: ("compact",), 6: ("grow",), 7: ("prune_to", 0.75), 8: ("regrow", 0.25), 9: ("checkpoint",)}
# name -> (dtype of the handle, the partner pair); the seeds were chosen on the CPU (tests/test_lifecycle_host.py holds them to the conditions)
GEOS = {"w96": (sa.F16, "w96", 31), "w128": (sa.BF16, "w96", 32), "pairs_even": (sa.F16, "w96", 33), "w13z": (sa.F32, "w128h20", 34)}
PARTNER_DTYPE = {"w96": sa.F16, "w128h20": sa.F32}
_geo = {}


def geometry(key):
    """the pattern of a pair: three training geometries, and `pairs_even` -- eight 32-row block-rows of 32-wide blocks over a ragged last block column, block-row
    ib without the block columns ib and (ib + 3) % 8: pair tiles with absent halves; rows and cols even, as vbs_linear needs on a 16-bit handle"""
    if key not in _geo:
        if key == "pairs_even":
            a = U._edge_arrays(256, 246, 32, [32] * 8, [U.poison_present(ib) for ib in range(8)])
            _geo[key] = U.sa_vbr(a, np.zeros(int((np.diff(a[3]) * a[4]).sum()) * 32, f32))
        else:
            _geo[key] = U.train_geometries()[key]
    return _geo[key]


def two_free_blocks(v):
    """two_free_blocks of tests/test_repattern_train_gpu.py (restated: that file needs a GPU to import)"""
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


def block_keys(v):
    """(block-row, block column) of every stored block of v, in mab order"""
    ibs = np.repeat(np.arange(v.block_rows), np.asarray(v.nzcount, np.int64))
    return [(int(ib), int(jb)) for ib, jb in zip(ibs, v.jab)]


def layout(v, blocks, field, dtype=f32):
    """the dict laid out in the mab order of the VBR v, through U.edge_blocks: v must store exactly the dict's blocks"""
    keys = block_keys(v)
    assert len(keys) == len(blocks) and set(keys) == set(blocks), "the pattern does not store the model's blocks"
    w = int(v.block_col_size)
    out = np.zeros(int(v.nztot), dtype)
    for (off, _, h, c0, _), key in zip(U.edge_blocks(v), keys):
        assert key[1] == c0 // w
        out[off:off + h * w] = blocks[key][field]
    return out


def one_image(v):
    """The rule of the 16-bit planner, restated for the patterns of these tests (no hub plan: blocks narrower than 64, or few): which stream images the handle
    of pattern v gets.  Two adjacent block-rows become a pair tile (image 1) when the first has 32 rows, the second 1..32, and BOTH store a block; any other
    block-row that stores a block is cut into 64-row tiles (image 1 for 33..64 rows, image 0 for <= 32).  The fp8 weight image needs exactly one image."""
    h = np.diff(np.asarray(v.row_part, np.int64))
    nz = np.asarray(v.nzcount, np.int64)
    images, ib = set(), 0
    while ib < v.block_rows:
        if ib + 1 < v.block_rows and h[ib] == 32 and 1 <= h[ib + 1] <= 32 and nz[ib] > 0 and nz[ib + 1] > 0:
            images.add(1)
            ib += 2
            continue
        if nz[ib] > 0 and h[ib] > 0:
            if h[ib] >= 64:
                images.add(1)
            if h[ib] % 64:
                images.add(0 if h[ib] % 64 <= 32 else 1)
        ib += 1
    return len(images) == 1


class PairModel:
    """one (handle, values) pair: the blocks and, for Adam, the step words"""

    def __init__(self, key, dtype, seed, kind, weak_row=None):
        v = geometry(key)
        self.key, self.dtype, self.kind = key, dtype, kind
        self.rows, self.cols, self.w = int(v.rows), int(v.cols), int(v.block_col_size)
        self.row_part = np.asarray(v.row_part, np.int64).copy()
        D = np.random.default_rng(seed).uniform(-1, 1, (self.rows, self.cols))
        D[D == 0] = 0.5
        if weak_row is not None:                                     # one block-row starts 2^-8 times as large: the first prune takes all of it
            D[int(self.row_part[weak_row]):int(self.row_part[weak_row + 1])] *= 2.0 ** -8
        W0 = U.edge_sample(v, D).astype(f32)
        self.blocks = {}
        for (off, _, h, _, _), k in zip(U.edge_blocks(v), block_keys(v)):
            n = h * self.w
            self.blocks[k] = {"W": W0[off:off + n].copy(), "M": np.zeros(n, f32), "V": np.zeros(n, f32), "live": True}
        self.S = np.zeros(8, np.uint32)
        self.stepped = False                                         # the optimizer allocates its state at the first step
        self._v = None
        self.G_raw = None                                            # the unmasked gradient of the last step, in the layout of pattern()

    def pattern(self):
        """the VBR (pattern only) of the blocks the dict holds"""
        if self._v is None:
            keys = sorted(self.blocks)
            nzcount = np.bincount([k[0] for k in keys], minlength=len(self.row_part) - 1).astype(np.int64)
            nztot = int((np.diff(self.row_part) * nzcount).sum()) * self.w
            self._v = sa.VBR.from_arrays(self.rows, self.cols, self.w, self.row_part, nzcount, np.array([k[1] for k in keys], np.int64), np.zeros(nztot, f32))
        return self._v

    def keys(self):
        return sorted(self.blocks)

    def keep(self):
        return np.array([1 if self.blocks[k]["live"] else 0 for k in self.keys()], np.uint8)

    def flat(self, field):
        return layout(self.pattern(), self.blocks, field)

    def n_in(self):
        """per block the elements inside the matrix"""
        return np.array([h * valid for _, _, h, _, valid in U.edge_blocks(self.pattern())], np.int64)

    def element_dead(self):
        v = self.pattern()
        m = np.zeros(int(v.nztot), bool)
        for (off, _, h, _, _), k in zip(U.edge_blocks(v), self.keys()):
            if not self.blocks[k]["live"]:
                m[off:off + h * self.w] = True
        return m

    def mag_scores(self):
        """BlockPruner.scores() on the host: fsum of the squares of the elements inside the matrix, over their number (+Inf for a block without any)"""
        out = []
        for (_, _, h, _, valid), k in zip(U.edge_blocks(self.pattern()), self.keys()):
            sq = self.blocks[k]["W"][:h * valid].astype(np.float64) ** 2
            out.append(math.fsum(sq.tolist()) / (h * valid) if h * valid else float("inf"))
        return np.array(out, np.float64)

    def grad_scores(self):
        """what the probe holds after the last backward, as regrow reads it: per DEAD block the exact integer sum of squares of its gradient inside the matrix,
        over the number of those elements (-Inf for a block without any); 0 for a live block"""
        out = []
        for (off, _, h, _, valid), k in zip(U.edge_blocks(self.pattern()), self.keys()):
            if h * valid == 0:
                out.append(float("-inf"))
            elif self.blocks[k]["live"]:
                out.append(0.0)
            else:
                g = self.G_raw[off:off + h * valid]
                ssq = int((g.astype(np.int64) ** 2).sum())
                assert np.isfinite(g).all() and ssq < 2 ** 53
                out.append(float(ssq) / (h * valid))
        return np.array(out, np.float64)

    def kill(self, k):
        b = self.blocks[k]
        b["live"] = False
        for name in "WMV":
            b[name] = np.zeros_like(b[name])

    def dense(self, Wflat):
        return U.edge_dense(self.pattern(), self.dtype, mab=np.asarray(Wflat, f32))


def _torch_lists(scores, keeps):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(s)) for s in scores], [torch.from_numpy(np.ascontiguousarray(k)) for k in keeps]


def rel_gap(lo, hi):
    """how far apart the two scores next to a cut are, relative to the larger"""
    if not (np.isfinite(lo) and np.isfinite(hi)):
        return float("inf") if lo != hi else 0.0
    return (hi - lo) / max(abs(hi), abs(lo)) if max(abs(hi), abs(lo)) > 0 else 0.0


class Lifecycle:
    """the run: two independent pairs under ONE optimizer, GradCtl and BlockPruner(scope="global")"""

    def __init__(self, geo, kind, repattern):
        dtype, partner, seed = GEOS[geo]
        self.geo, self.kind, self.repattern = geo, kind, bool(repattern)
        self.seed = 1000 * seed
        self.pairs = [PairModel(geo, dtype, self.seed + 1, kind), PairModel(partner, PARTNER_DTYPE[partner], self.seed + 2, kind, weak_row=0)]
        self.words = fresh_record(loss_scale=LOSS_SCALE)
        self.n0 = sum(len(p.blocks) for p in self.pairs)             # the original block count
        self.inf_row = None
        self.gaps = []                                               # (event, which cut, relative gap) at every cut
        self.notes = []                                              # what the host test reads: per step and event a dict

    # ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------
    def inputs(self, t):
        """per pair (x, T): small integers; at INF_STEP one +Inf in T of pair 0, in the first row of its first block-row that holds a live block"""
        out = []
        for i, p in enumerate(self.pairs):
            rng = np.random.default_rng(self.seed + 100 * t + 10 * i)
            x = rng.integers(-3, 4, (N, p.cols)).astype(f32)
            T = rng.integers(-3, 4, (N, p.rows)).astype(f32)
            if t == INF_STEP and i == 0:
                if self.inf_row is None:
                    ib = min(k[0] for k in p.keys() if p.blocks[k]["live"] and p.row_part[k[0] + 1] > p.row_part[k[0]])
                    self.inf_row = int(p.row_part[ib])
                T[INF_SAMPLE, self.inf_row] = np.inf
            out.append((x, T))
        return out

    def events_after(self, t):
        ev = AFTER.get(t)
        if ev is None or (ev[0] in ("compact", "grow") and not self.repattern):
            return []
        return [ev]

    def loss_scale(self):
        return record_fields(self.words)["loss_scale"]

    # ---- a step -----------------------------------------------------------------------------------------------------------------------------------------------
    def step(self, t):
        """one training step of both pairs; returns what the device is held to besides the state: {"G": the gradients after masking, "skip", "coef", ...}"""
        scale = f32(self.loss_scale())
        G, note = [], {"t": t, "scale": float(scale), "max_int": 0.0}
        for p, (x, T) in zip(self.pairs, self.inputs(t)):
            with np.errstate(invalid="ignore", over="ignore"):
                dY = T.astype(np.float64) * float(scale)
                full = dY.T @ x.astype(np.float64)
            v = p.pattern()
            raw = U.edge_sample(v, full)
            fin = raw[np.isfinite(raw)]
            note["max_int"] = max([note["max_int"], float(np.abs(dY[np.isfinite(dY)]).max()), float(np.abs(fin).max()) if fin.size else 0.0])
            assert np.array_equal(fin, np.rint(fin))
            p.G_raw = raw
            g = raw.astype(f32)
            g[p.element_dead()] = 0.0
            G.append(g)
        ssq, bad = stats_ref(np.concatenate(G))
        w = self.words.copy()
        w[0:2].view(np.float64)[0] = ssq
        w[2:3].view(np.int32)[0] = bad
        w[3] = 0
        self.words = grad_ctl_ref(w, CTL_CFG)
        r = record_fields(self.words)
        if not r["skip"]:
            for p, g in zip(self.pairs, G):
                self._update(p, g * f32(r["coef"]))
        for p in self.pairs:
            p.stepped = True
        note.update(skip=r["skip"], coef=float(r["coef"]), scale_before=float(scale), nonfinite=bad, ssq=ssq)
        self.notes.append(note)
        return {"G": G, "skip": r["skip"], "coef": r["coef"], "words": self.words.copy()}

    def _update(self, p, g):
        """the elementwise step on the live blocks (a dead block is +0 in W, M, V and g: both optimizers keep it there)"""
        v = p.pattern()
        spans = [(off, h * p.w, k) for (off, _, h, _, _), k in zip(U.edge_blocks(v), p.keys()) if p.blocks[k]["live"]]
        if self.kind == "adamw":
            if spans:
                cat = lambda f: np.concatenate([p.blocks[k][f] for _, _, k in spans])  # noqa: E731
                Wn, Mn, Vn, S = adam_ref(cat("W"), np.concatenate([g[o:o + n] for o, n, _ in spans]), cat("M"), cat("V"), p.S, HYPER["adamw"])
            else:
                z = np.zeros(0, f32)
                Wn, Mn, Vn, S = adam_ref(z, z, z, z, p.S, HYPER["adamw"])
            p.S = S
        else:
            if not spans:
                return
            cat = lambda f: np.concatenate([p.blocks[k][f] for _, _, k in spans])  # noqa: E731
            Wn, Mn = sgd_ref(cat("W"), np.concatenate([g[o:o + n] for o, n, _ in spans]), cat("M"), HYPER["sgd"])
            Vn = np.zeros_like(Wn)
        at = 0
        for _, n, k in spans:
            p.blocks[k]["W"], p.blocks[k]["M"], p.blocks[k]["V"] = Wn[at:at + n].copy(), Mn[at:at + n].copy(), Vn[at:at + n].copy()
            at += n

    # ---- the events ---------------------------------------------------------------------------------------------------------------------------------------------
    def live_total(self):
        return sum(int(p.keep().sum()) for p in self.pairs)

    def total(self):
        return sum(len(p.blocks) for p in self.pairs)

    def sparsity_of(self, ev):
        """the `sparsity` argument of BlockPruner.prune for the event: prune 0.5 is itself; prune_to 0.75 prunes as many live blocks as take the dead blocks from
        floor(0.5 n0) to floor(0.75 n0) of the ORIGINAL count n0 -- on whatever sizes the run has by then"""
        if ev[0] == "prune":
            return ev[1]
        newly = math.floor(ev[1] * self.n0) - math.floor(0.5 * self.n0)
        total, dead = self.total(), self.total() - self.live_total()
        s = (dead + newly + 0.5) / total
        assert math.floor(s * total) == dead + newly and 0 < s < 1
        return s

    def apply(self, ev):
        getattr(self, "_" + ev[0])(ev)

    def _apply_masks(self, new, what):
        changed = 0
        for p, k_new in zip(self.pairs, new):
            for key, was, now in zip(p.keys(), p.keep(), k_new):
                if was and not now:
                    p.kill(key)
                    changed += 1
                elif now and not was:
                    p.blocks[key]["live"] = True
                    changed += 1
        self.notes.append({"event": what, "changed": changed, "dead_rows": self.dead_block_rows(), "live": self.live_total(), "total": self.total()})

    def _prune(self, ev):
        s = self.sparsity_of(ev)
        scores, keeps = [p.mag_scores() for p in self.pairs], [p.keep() for p in self.pairs]
        ts, tk = _torch_lists(scores, keeps)
        new = [k.numpy().astype(np.uint8) for k in sa.prune.select(ts, tk, s, "global")]
        live = np.sort(np.concatenate(scores)[np.concatenate(keeps) != 0])
        n = int(np.concatenate(keeps).sum()) - int(np.concatenate(new).sum())
        assert 0 < n < len(live)
        self.gaps.append((ev, "prune", rel_gap(live[n - 1], live[n])))
        self._apply_masks(new, ev)

    _prune_to = _prune

    def _regrow(self, ev):
        n_swap = int(math.floor(ev[1] * self.live_total()))
        mag, grad, keeps = [p.mag_scores() for p in self.pairs], [p.grad_scores() for p in self.pairs], [p.keep() for p in self.pairs]
        tm, tk = _torch_lists(mag, keeps)
        tg, _ = _torch_lists(grad, keeps)
        new = [k.numpy().astype(np.uint8) for k in sa.prune.select_swap(tm, tg, tk, n_swap, "global")]
        kc, mc, gc = np.concatenate(keeps), np.concatenate(mag), np.concatenate(grad)
        live, cand = np.sort(mc[kc != 0]), np.sort(gc[(kc == 0) & (gc != -np.inf)])[::-1]
        count = min(n_swap, len(live), len(cand))
        assert count > 0
        if count < len(live):
            self.gaps.append((ev, "drop", rel_gap(live[count - 1], live[count])))
        if count < len(cand):
            self.gaps.append((ev, "grow", rel_gap(cand[count], cand[count - 1])))
        self._apply_masks(new, ev)
        self.notes[-1]["swapped"] = count

    def _compact(self, ev):
        for p in self.pairs:
            p.blocks = {k: b for k, b in p.blocks.items() if b["live"]}
            p._v, p.G_raw = None, None
        self.notes.append({"event": ev, "patterns": [p.pattern() for p in self.pairs]})

    def grow_list(self):
        return two_free_blocks(self.pairs[0].pattern())

    def _grow(self, ev):
        p = self.pairs[0]
        for ib, jb in self.grow_list():
            n = int(p.row_part[ib + 1] - p.row_part[ib]) * p.w
            assert (ib, jb) not in p.blocks
            p.blocks[(ib, jb)] = {"W": np.zeros(n, f32), "M": np.zeros(n, f32), "V": np.zeros(n, f32), "live": True}
        p._v, p.G_raw = None, None
        self.notes.append({"event": ev, "patterns": [q.pattern() for q in self.pairs]})

    def _checkpoint(self, ev):
        """a deep copy: nothing of the model changes"""

    def dead_block_rows(self):
        """per pair the block-rows that store blocks, all of them dead"""
        out = []
        for p in self.pairs:
            rows = {}
            for k in p.keys():
                rows.setdefault(k[0], []).append(p.blocks[k]["live"])
            out.append([ib for ib, lives in rows.items() if not any(lives)])
        return out


def run_model(geo, kind, repattern, watch=None):
    """the whole schedule on the model alone; watch(model, what) is called after every step and event"""
    m = Lifecycle(geo, kind, repattern)
    for t in range(1, STEPS + 1):
        m.step(t)
        if watch:
            watch(m, ("step", t))
        for ev in m.events_after(t):
            m.apply(ev)
            if watch:
                watch(m, ev)
    return m
