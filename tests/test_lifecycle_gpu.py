"""Prune -> regrow -> compact -> grow -> prune -> regrow -> checkpoint, under every switch, against the numpy model of tests/_lifecycle.py.

Two independent pairs under ONE optimizer (VbsAdamW(lr=1e-2, weight_decay=0.01); VbsSGD(lr=1e-2, momentum=0.9) on a subset), GradCtl(loss_scale=4, max_norm=1,
growth_interval=2) and BlockPruner(scope="global"); each pair has its own small-integer x and T, the loss is (y * T).sum() * loss_scale through
vbs_linear(..., probe=pruner.probe(i)).  Ten steps: prune to 50 % after step 2, regrow(0.25) after 4, one +Inf in T at step 5 (the step skips), compact after
5 and grow of two free blocks on pair 0 after 6 (the runs that repattern), a prune after 7 that takes the dead blocks to 75 % of the original count,
regrow(0.25) after 8, and in some runs a checkpoint after 9: the state dicts of optimizer, pruner and GradCtl go into fresh objects on fresh handles.

Arms, each without and with the repattern events: mask (mask_grads, no live set), skip (skip_pruned), live_steps, live_forward, fp8 (+ skip + live_steps)
and fp8_live (+ a8_live).  The fp8 arms run where both pairs are 16-bit; the fp32 run takes the first four and must keep the plain kernels.

The gradient is exact (integers) and the steps are elementwise, so after every step and every event W, the moments or the momentum buffer, Adam's step words,
the control record and the masks equal the model BIT FOR BIT in every arm, through the model's layout helper on the pattern the device reports.  The forward
product of every step (not exact) lies within the suite's bound, TOL * sum|a||b| of tests/test_poison_gpu.py, of float64 numpy on the values the product
claims to use -- W as the handle's type rounds it, or the dequantised fp8 image -- and the form fields say which product ran, so that no arm passes by
falling back.  tests/test_lifecycle_host.py checks the conditions on the inputs without a GPU.  No graph capture here: repattern refuses it by contract."""
import hashlib

import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd.autograd import vbs_linear

torch = pytest.importorskip("torch")

import _util as U  # noqa: E402
import _a8 as A8  # noqa: E402
import _lifecycle as LC  # noqa: E402
from test_poison_gpu import TOL  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
TDT = {sa.F32: torch.float32, sa.F16: torch.float16, sa.BF16: torch.bfloat16}
ARMS = {"mask": {}, "skip": dict(skip_pruned=True), "live_steps": dict(skip_pruned=True, live_steps=True),
        "live_forward": dict(skip_pruned=True, live_steps=True, live_forward=True),
        "fp8": dict(skip_pruned=True, live_steps=True), "fp8_live": dict(skip_pruned=True, live_steps=True, a8_live=True)}
PLAIN_ARMS = ("mask", "skip", "live_steps", "live_forward")


def runs():
    out = []
    for geo, (dtype, _, _) in LC.GEOS.items():
        for rep in (False, True):
            out += [(geo, "adamw", arm, rep) for arm in (PLAIN_ARMS if dtype == sa.F32 else tuple(ARMS))]
    for rep in (False, True):
        out += [("w96", "sgd", "live_steps", rep), ("w96", "sgd", "fp8_live", rep), ("w13z", "sgd", "mask", rep), ("w13z", "sgd", "live_forward", rep)]
    return out


RUNS = runs()
_FINAL = {}                                                          # run -> the digest of its final state


def checkpointed(arm, rep):
    """the runs that go through the checkpoint after step 9"""
    return (arm in ("live_forward", "fp8_live") and rep) or (arm == "mask" and not rep)


def words(t):
    return t.detach().cpu().numpy().reshape(-1).view(np.uint32)


class Run:
    def __init__(self, geo, kind, arm, rep):
        self.model = LC.Lifecycle(geo, kind, rep)
        self.kind, self.arm, self.flags, self.fp8 = kind, arm, ARMS[arm], arm.startswith("fp8")
        self.vs = [LC.geometry(p.key) for p in self.model.pairs]    # the VBR of every handle: after compact and grow, the one the library returned
        self.opened = []
        pairs = []
        for p, v in zip(self.model.pairs, self.vs):
            h = v.to_device(0, dtype=p.dtype, updatable=True, transposable=True)
            self.opened.append(h)
            w = torch.from_numpy(p.flat("W")).cuda().requires_grad_(True)
            if self.fp8:
                h.set_forward_a8(True, values=w.detach())
            pairs.append((h, w))
        self.opt = self.make_opt(pairs)
        self.ctl = sa.GradCtl(loss_scale=LC.LOSS_SCALE, max_norm=LC.MAX_NORM, growth_interval=LC.GROWTH_INTERVAL)
        self.pruner = sa.BlockPruner(self.opt, scope="global", **self.flags)
        self.installed = [False, False]                              # per pair: whether the handle holds a live set, by the arm's own book
        self.what = (geo, kind, arm, rep)

    def make_opt(self, pairs):
        return (sa.VbsAdamW if self.kind == "adamw" else sa.VbsSGD)(pairs, **LC.HYPER[self.kind])

    def close(self):
        for h in self.opened:
            h.close()

    # ---- the forward product ---------------------------------------------------------------------------------------------------------------------------------
    def claimed(self, i, h, w):
        """the dense float64 matrix of the values the product claims to use"""
        W = w.detach().cpu().numpy()
        if self.fp8:
            codes, exps, group = h.a8_get()
            qc, qe = A8.quantize(W, group)
            assert np.array_equal(codes, qc) and np.array_equal(exps, qe), (self.what, i, "the fp8 image does not follow W")
            W = A8.dequantize(qc, qe).astype(f32)
        return U.edge_dense(self.vs[i], self.model.pairs[i].dtype, mab=W)

    def expected_form(self, i, h):
        """(field that must hold it, value) for a 16-bit pair"""
        cap = (h.a8_info() if self.fp8 else h.live_forward_info())["capable"]
        assert (cap > 0) == LC.one_image(self.vs[i]) and cap > 0, (self.what, i, cap, "the planner's rule, as the model restates it")
        live = self.installed[i] and bool(self.flags.get("skip_pruned"))
        if self.fp8:
            form = 4 if live and self.flags.get("a8_live") else 3
        else:
            form = 2 if live and self.flags.get("live_forward") else 1
        return cap, form

    def check_forward(self, t, i, h, w, x, y):
        p = self.model.pairs[i]
        z = torch.empty((LC.N, p.rows), dtype=torch.float32, device="cuda")
        h.spmm(x.detach(), z, LC.N, accumulate=False)
        A = self.claimed(i, h, w)
        xh = x.detach().float().cpu().numpy().astype(np.float64)
        ref, bound = xh @ A.T, TOL * (np.abs(xh) @ np.abs(A).T) + 1e-30
        for name, got in (("spmm", z), ("vbs_linear", y)):
            g = got.detach().float().cpu().numpy()
            assert not np.isnan(g).any(), (self.what, t, i, name, "NaN")
            assert np.all(np.abs(g - ref) <= bound), (self.what, t, i, name, float(np.abs(g - ref).max()))
        fi = h.a8_info()
        forms = (fi["form_one_tile"], fi["form_pair"])
        assert forms == (h.live_forward_info()["form_one_tile"], h.live_forward_info()["form_pair"])
        if p.dtype == sa.F32:
            assert h.live_forward_info()["capable"] == 0 and max(forms) <= 1, (self.what, t, i, forms, "an fp32 handle keeps the plain kernels")
        else:
            cap, form = self.expected_form(i, h)
            assert forms == ((form, 0) if cap == 1 else (0, form)), (self.what, t, i, forms, cap, form)
        if self.fp8:
            assert fi["switch"] == 1 and fi["valid"] == 1, (self.what, t, i, fi)

    # ---- one step -----------------------------------------------------------------------------------------------------------------------------------------------
    def step(self, t):
        m = self.model
        inputs = m.inputs(t)
        self.opt.zero_grad()
        xs = []
        for i, ((h, w), (x_np, T_np)) in enumerate(zip(self.opt.pairs, inputs)):
            p = m.pairs[i]
            x = torch.from_numpy(x_np).to(TDT[p.dtype]).cuda().requires_grad_(True)
            T = torch.from_numpy(T_np).cuda()
            y = vbs_linear(x, h, w, out_dtype=None if p.dtype == sa.F32 else torch.float32, probe=self.pruner.probe(i))
            self.check_forward(t, i, h, w, x, y)
            ((y * T).sum() * self.ctl.loss_scale).backward()
            xs.append(x)
        dead = [p.element_dead() for p in m.pairs]
        if self.arm == "mask":
            self.pruner.mask_grads()
        else:                                                        # straight out of backward
            for i, (_, w) in enumerate(self.opt.pairs):
                assert not words(w.grad)[dead[i]].any(), (self.what, t, i, "the gradient of a dead block")
        A_before = [self.claimed(i, h, w) if t != LC.INF_STEP else None for i, (h, w) in enumerate(self.opt.pairs)] if not self.fp8 else None
        exp = m.step(t)
        for i, (_, w) in enumerate(self.opt.pairs):
            g, want = w.grad.detach().cpu().numpy(), exp["G"][i]
            fin = np.isfinite(want)
            assert not words(w.grad)[dead[i]].any(), (self.what, t, i, "the gradient of a dead block")
            assert np.array_equal(g[fin], want[fin]) and not np.isfinite(g[~fin]).any(), (self.what, t, i, "the gradient is not the model's")
            assert (t == LC.INF_STEP and i == 0) == bool((~fin).any())
        # grad_x = dY A through the transposed product (empty lists where a block column or a block-row is wholly dead), in x's type
        if A_before is not None and t != LC.INF_STEP:
            for i, (x, (x_np, T_np)) in enumerate(zip(xs, inputs)):
                dY = T_np.astype(np.float64) * exp_scale(m, t)
                ref, bound = dY @ A_before[i], TOL * (np.abs(dY) @ np.abs(A_before[i])) + 1e-30
                lo, hi = (torch.from_numpy(ref + s * bound).to(x.dtype).float().numpy() for s in (-1, 1))
                gx = x.grad.float().cpu().numpy()
                assert np.isfinite(gx).all() and np.all((gx >= lo) & (gx <= hi)), (self.what, t, i, "grad_x")
        self.ctl.collect(self.opt)
        self.opt.step(ctl=self.ctl)
        torch.cuda.synchronize()
        r = self.ctl.read()
        assert np.array_equal(r["words"], exp["words"]), (self.what, t, LC.record_fields(r["words"]), LC.record_fields(exp["words"]))
        assert r["skip"] == (1 if t == LC.INF_STEP else 0)
        for i, (h, _) in enumerate(self.opt.pairs):
            assert h.step_info()["live"] == (1 if self.flags.get("live_steps") and self.installed[i] else 0), (self.what, t, i, h.step_info())
        self.compare(("step", t))

    # ---- the state against the model -------------------------------------------------------------------------------------------------------------------------
    def state_of(self, i):
        """(names, device tensors in the values' layout), then Adam's step words or None"""
        if self.kind == "sgd":
            return [("M", self.opt._bufs[i])], None
        s = self.opt._state[i]
        return ([("M", s["exp_avg"]), ("V", s["exp_avg_sq"])], s["state"]) if s is not None else ([], None)

    def compare(self, at, record=True):
        torch.cuda.synchronize()
        m = self.model
        digest = hashlib.sha256()
        assert [h for h, _ in self.opt.pairs] == [h for h, _ in self.pruner.pairs] and all(a[1] is b[1] for a, b in zip(self.opt.pairs, self.pruner.pairs))
        for i, ((h, w), p) in enumerate(zip(self.opt.pairs, m.pairs)):
            v = self.vs[i]
            keys = LC.block_keys(v)
            assert w.numel() == h.info()["nztot"] == int(v.nztot) and h.n_blocks == len(keys) == len(p.blocks), (self.what, at, i, "sizes")
            lay, S = self.state_of(i)
            assert bool(lay) == p.stepped and all(t_ is not None and t_.numel() == w.numel() for _, t_ in lay), (self.what, at, i, "state sizes")
            dead = p.element_dead()
            for name, t_ in [("W", w)] + lay:
                got, want = words(t_), LC.layout(v, p.blocks, name).view(np.uint32)
                assert np.array_equal(got, want), (self.what, at, i, name, int((got != want).sum()), "differs from the model")
                assert not got[dead].any(), (self.what, at, i, name, "a dead block is not +0")
                digest.update(got.tobytes())
            if self.kind == "adamw" and p.stepped:
                assert np.array_equal(words(S), p.S), (self.what, at, i, "Adam's step words", words(S), p.S)
            keep = self.pruner.keep_masks()[i].cpu().numpy()
            want_keep = np.array([1 if p.blocks[k]["live"] else 0 for k in keys], np.uint8)
            assert np.array_equal(keep, want_keep), (self.what, at, i, "the keep mask", int((keep != want_keep).sum()))
            assert np.array_equal(self.pruner.probe(i).sel.cpu().numpy(), 1 - want_keep), (self.what, at, i, "the probe's selection")
            digest.update(keep.tobytes())
            li = h.live_info()
            assert li["installed"] == (1 if self.installed[i] and self.flags.get("skip_pruned") else 0), (self.what, at, i, li)
            if li["installed"]:
                assert li["live_blocks"] == int(want_keep.sum()) and li["live_steps"] == (1 if self.flags.get("live_steps") else 0), (self.what, at, i, li)
            if self.fp8:
                fi = h.a8_info()
                assert fi["switch"] == 1 and fi["valid"] == 1, (self.what, at, i, fi)
        if record:
            got = self.ctl.read()["words"]
            assert np.array_equal(got, m.words), (self.what, at, "the control record")
            digest.update(got.tobytes())
        return digest.hexdigest()

    # ---- the events ------------------------------------------------------------------------------------------------------------------------------------------------
    def event(self, ev):
        m = self.model
        record = True
        if ev[0] in ("prune", "prune_to"):
            self.pruner.prune(m.sparsity_of(ev))
            self.installed = [True, True]
        elif ev[0] == "regrow":
            self.pruner.regrow(ev[1])
            self.installed = [True, True]
        elif ev[0] == "compact":
            self.vs = self.pruner.compact(self.vs)
            self.opened += [h for h, _ in self.opt.pairs]
            self.installed = [False, False]                          # fresh handles without a dead block: the next prune installs a set
        elif ev[0] == "grow":
            self.vs[0] = self.pruner.grow(0, self.vs[0], m.grow_list())
            self.opened.append(self.opt.pairs[0][0])
            self.installed[0] = True                                 # grow hands the new handle the set again (every block of it live); pair 1 stays as compact left it
        elif ev[0] == "checkpoint":
            self.checkpoint()
            record = False                                           # a fresh GradCtl: statistics, norm and coef come with the next step
        m.apply(ev)
        self.compare(ev, record)
        if self.fp8 and ev[0] in ("compact", "grow"):
            for i, (h, w) in enumerate(self.opt.pairs):
                self.claimed(i, h, w)                                # codes and exponents equal A8.quantize of the moved W

    def checkpoint(self):
        """state dicts of optimizer, pruner and GradCtl into fresh objects on handles created from the current vbmats"""
        osd, psd, csd = self.opt.state_dict(), self.pruner.state_dict(), self.ctl.state_dict()
        pairs = []
        for (h, w), p, v in zip(self.opt.pairs, self.model.pairs, self.vs):
            fresh_v = sa.VBR.from_arrays(v.rows, v.cols, v.block_col_size, v.row_part, v.nzcount, v.jab, np.zeros(int(v.nztot), f32))
            nh = fresh_v.to_device(0, dtype=p.dtype, updatable=True, transposable=True)
            self.opened.append(nh)
            nw = w.detach().clone().requires_grad_(True)
            if self.fp8:
                nh.set_forward_a8(True, values=nw.detach())
            pairs.append((nh, nw))
        self.opt = self.make_opt(pairs)
        self.opt.load_state_dict(osd)
        self.pruner = sa.BlockPruner(self.opt, scope="global", **self.flags)
        self.pruner.load_state_dict(psd)
        self.ctl = sa.GradCtl(loss_scale=1.0, max_norm=LC.MAX_NORM, growth_interval=LC.GROWTH_INTERVAL)
        self.ctl.load_state_dict(csd)
        r, want = self.ctl.read(), LC.record_fields(self.model.words)
        assert (r["loss_scale"], r["growth_tracker"], r["skipped_total"]) == (float(want["loss_scale"]), want["growth_tracker"], want["skipped_total"])
        self.installed = [True, True]                                # load_state_dict applies the masks as prune does


def exp_scale(m, t):
    return [n for n in m.notes if n.get("t") == t][0]["scale_before"]


@pytest.mark.parametrize("run", RUNS, ids=["%s-%s-%s-%s" % (g, k, a, "repattern" if r else "plain") for g, k, a, r in RUNS])
def test_lifecycle(run):
    geo, kind, arm, rep = run
    r = Run(geo, kind, arm, rep)
    try:
        final = None
        for t in range(1, LC.STEPS + 1):
            r.step(t)
            for ev in r.model.events_after(t):
                if ev[0] == "checkpoint" and not checkpointed(arm, rep):
                    continue
                r.event(ev)
        final = r.compare("end")
        # a cross-check of the harness: the model says that every arm of one (geometry, optimizer, schedule) ends in the same bits
        for (g2, k2, a2, r2), d in _FINAL.items():
            assert (g2, k2, r2) != (geo, kind, rep) or d == final, (run, "ends in other bits than", a2)
        _FINAL[run] = final
    finally:
        r.close()
