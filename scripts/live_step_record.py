"""Live steps (sparta_vbs_set_live_steps) on the handle bench.py builds for its headline config (cant-like FEM, Jaccard -a 5 -t 0.6, w = 32, row_block 32,
force_fixed_size), made updatable and transposable.  The method of scripts/live_record.py: HIP events around each arm on an idle stream (the host side of an
arm is inside its window), all arms interleaved call by call in one process in a new seeded order every round, median and 10th / 90th percentile of the timed
calls.  Arms (S = 0 / 50 / 75 / 90 % of the blocks pruned by BlockPruner(skip_pruned=True).prune, a handle of its own per level and form):
  adam / sgd                     adam_step / sgd_step(momentum=0.9) on a handle that never had a live set
  adam_S / sgd_S                 the same with the live set of level S installed and the switch off: the parent's step on that handle and mask
  adam_live_S / sgd_live_S       the switch on
  adam_2p / adam_live2p_S        the two-pass forms (SPARTA_ADAM_FUSE=0 around the call), plain and live
  set_live_blocks / _steps_on    the call alone on the 50 % handle, switch off / on
  step_skip_S / step_live_S      one whole training step at S = 50 / 90 %: vbs_linear forward + backward and the clipped AdamW step (GradCtl.collect + step(ctl=)),
                                 BlockPruner(skip_pruned=True) without / with live_steps=True
After the timing: per live handle, whether its forward product equals that of a fresh handle given the same values ("product_equal").
On a checkout without the feature (SPARTA_AMD_ROOT pointing at a build of the parent commit) only the arms that exist there run.
One JSON line, appended to profiles/live_step/<--out> with --save.

    python scripts/live_step_record.py [--dtype f32|f16|bf16] [--reps 50] [--commit REV] [--out live_step_record.jsonl] [--save]"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("SPARTA_AMD_ROOT") or HERE
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=["f32", "f16", "bf16"], default="f32")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--commit", default="", help="revision the numbers are taken on (recorded as given)")
    ap.add_argument("--out", default="live_step_record.jsonl")
    ap.add_argument("--save", action="store_true")
    args = ap.parse_args()
    import torch
    import sparta_amd as sa
    from sparta_amd.autograd import vbs_linear
    sdt = {"f32": sa.F32, "f16": sa.F16, "bf16": sa.BF16}[args.dtype]
    tdt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[args.dtype]
    has_live_steps = hasattr(sa.DeviceVBS, "set_live_steps")
    w, N = 32, 128
    m = sa.gen.cant_like(seed=2)
    eng = sa.BlockingEngine(blocking_algo=5, tau=0.6, col_block_size=w, row_block_size=32, force_fixed_size=True, sim_measure=1)
    vb = sa.VBR().fill_from_CSR_inplace(m, eng.GetGrouping(m), w, 32, True)
    nztot = int(vb.nztot)
    rng = np.random.default_rng(1)
    W0 = torch.from_numpy(np.ascontiguousarray(vb.mab, np.float32)).cuda()
    G0 = torch.from_numpy(rng.uniform(-1e-2, 1e-2, nztot).astype(np.float32)).cuda()
    adam_cfg = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    sgd_cfg = dict(lr=1e-3, momentum=0.9)

    class Arm:
        """a handle, its values and state, pruned to s (s=None: no pruner, no live set); live: the switch"""

        def __init__(self, s, live):
            self.H = vb.to_device(0, dtype=sdt, updatable=True, transposable=True)
            self.W = W0.clone().requires_grad_(True)
            self.G = G0.clone()
            self.M, self.V, self.buf = torch.zeros_like(W0), torch.zeros_like(W0), torch.zeros_like(W0)
            self.S = torch.zeros(8, dtype=torch.int32, device="cuda")
            self.p = None
            if s is not None:
                self.p = sa.BlockPruner([(self.H, self.W)], skip_pruned=True)
                self.p.prune(s)
                self.H.mask_blocks(self.p.keep_masks()[0], self.G)
                if live:
                    self.H.set_live_steps(True)

        def adam(self):
            self.H.adam_step(self.W.detach(), self.G, self.M, self.V, self.S, **adam_cfg)

        def sgd(self):
            self.H.sgd_step(self.W.detach(), self.G, self.buf, **sgd_cfg)

        def adam_2p(self):
            os.environ["SPARTA_ADAM_FUSE"] = "0"
            try:
                self.adam()
            finally:
                del os.environ["SPARTA_ADAM_FUSE"]

    arms, info, live_arms = {}, {}, {}
    base = Arm(None, False)
    arms["adam"], arms["sgd"], arms["adam_2p"] = base.adam, base.sgd, base.adam_2p
    for s in (0.0, 0.5, 0.75, 0.9):
        tag = "%g" % (100 * s)
        a = Arm(s, False)
        arms["adam_" + tag], arms["sgd_" + tag] = a.adam, a.sgd
        if s == 0.5:
            arms["set_live_blocks"] = lambda a=a: a.H.set_live_blocks(a.p.keep_masks()[0])
        if has_live_steps:
            b = Arm(s, True)
            arms["adam_live_" + tag], arms["sgd_live_" + tag], arms["adam_live2p_" + tag] = b.adam, b.sgd, b.adam_2p
            live_arms[tag] = b
            if s == 0.5:
                arms["set_live_blocks_steps_on"] = lambda b=b: b.H.set_live_blocks(b.p.keep_masks()[0])
    x_in = torch.from_numpy(rng.uniform(-1, 1, (N, vb.cols)).astype(np.float32)).cuda().to(tdt)
    gy = torch.from_numpy(rng.uniform(-1, 1, (N, vb.rows)).astype(np.float32)).cuda()
    keep = []

    def step_arm(s, live):
        H = vb.to_device(0, dtype=sdt, updatable=True, transposable=True)
        W = W0.clone().requires_grad_(True)
        opt = sa.VbsAdamW([(H, W)], **adam_cfg)
        p = sa.BlockPruner(opt, skip_pruned=True, live_steps=True) if live else sa.BlockPruner(opt, skip_pruned=True)
        p.prune(s)
        ctl = sa.GradCtl(loss_scale=1.0, max_norm=1.0, growth_interval=2000)
        x = x_in.clone().requires_grad_(True)

        def step():
            opt.zero_grad()
            x.grad = None
            y = vbs_linear(x, H, W)
            y.backward(gy.to(y.dtype))
            ctl.collect(opt)
            opt.step(ctl=ctl)
        keep.append((H, p))
        return step

    for s in (0.5, 0.9):
        arms["step_skip_%g" % (100 * s)] = step_arm(s, False)
        if has_live_steps:
            arms["step_live_%g" % (100 * s)] = step_arm(s, True)

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def call(k, timed=None):
        if timed is None:
            arms[k]()
        else:
            e0.record(); arms[k](); e1.record(); e1.synchronize()
            timed.append(e0.elapsed_time(e1))

    for _ in range(5):
        for k in arms:
            call(k)
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    order = np.random.default_rng(2)
    for _ in range(args.reps):
        for k in order.permutation(list(arms)):
            call(str(k), times[str(k)])
    torch.cuda.synchronize()
    # the forward product after live steps against a fresh handle given the same values
    B = torch.from_numpy(rng.uniform(-1, 1, vb.cols * N).astype(np.float32)).cuda().to(tdt)
    for tag, b in live_arms.items():
        b.adam()
        info[tag] = dict(b.H.step_info(), live=b.H.step_info()["live"], live_blocks=b.H.live_info()["live_blocks"])
        fresh = vb.to_device(0, dtype=sdt, updatable=True)
        fresh.set_values(b.W.detach())
        C1, C2 = (torch.zeros(vb.rows * N, dtype=torch.float32, device="cuda") for _ in range(2))
        b.H.spmm(B, C1, N)
        fresh.spmm(B, C2, N)
        torch.cuda.synchronize()
        info[tag]["product_equal"] = bool(torch.equal(C1, C2))
        info[tag]["finite"] = bool(torch.isfinite(C1).all())
        fresh.close()
    r5 = lambda x: round(float(x), 5)      # noqa: E731
    rec = {"dtype": args.dtype, "commit": args.commit, "has_live_steps": has_live_steps, "rows": int(vb.rows), "cols": int(vb.cols), "nztot": nztot, "N": N,
           "reps": args.reps, "ms_med_p10_p90": {k: [r5(np.median(t)), r5(np.percentile(t, 10)), r5(np.percentile(t, 90))] for k, t in times.items()},
           "live": info}
    line = json.dumps(rec)
    print(line)
    if args.save:
        out = os.path.join(HERE, "profiles", "live_step")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, args.out), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
