"""The live-block set (sparta_vbs_set_live_blocks) on the handle bench.py builds for its headline config (cant-like FEM, Jaccard -a 5 -t 0.6, w = 32, row_block
32, force_fixed_size), made updatable and transposable, N = k = 128.  The method of scripts/prune_record.py: HIP events around each arm on an idle stream (the
host side of an arm is inside its window), all arms interleaved call by call in one process in a new seeded order every round, median and 10th / 90th
percentile of the timed calls.  Arms:
  sddmm / spmm_t             the two backward products on a handle that never had a live set
  sddmm_S / spmm_t_S         the same on a handle pruned to S = 0 / 50 / 75 / 90 % of its blocks by BlockPruner(skip_pruned=True).prune: live set installed
  set_live_blocks            the call alone (the mask of the 50 % handle)
  step_mask_S / step_skip_S  one whole training step at S = 50 / 90 %: vbs_linear forward + backward, then mask_grads (step_mask only: a pruner with
                             skip_pruned=False) and the clipped AdamW step (GradCtl.collect + step(ctl=))
On a checkout without the feature (SPARTA_AMD_ROOT pointing at a build of the parent commit) only the arms that exist there run: sddmm, spmm_t, step_mask_S.
One JSON line, appended to profiles/live/live_record.jsonl with --save.

    python scripts/live_record.py [--dtype f32|f16|bf16] [--reps 50] [--commit REV] [--save]"""
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
    ap.add_argument("--save", action="store_true")
    args = ap.parse_args()
    import torch
    import sparta_amd as sa
    from sparta_amd.autograd import vbs_linear
    sdt = {"f32": sa.F32, "f16": sa.F16, "bf16": sa.BF16}[args.dtype]
    tdt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[args.dtype]
    has_live = hasattr(sa.DeviceVBS, "set_live_blocks")
    w, N = 32, 128
    m = sa.gen.cant_like(seed=2)
    eng = sa.BlockingEngine(blocking_algo=5, tau=0.6, col_block_size=w, row_block_size=32, force_fixed_size=True, sim_measure=1)
    vb = sa.VBR().fill_from_CSR_inplace(m, eng.GetGrouping(m), w, 32, True)
    nztot = int(vb.nztot)
    rng = np.random.default_rng(1)
    X = torch.from_numpy(rng.uniform(-1, 1, vb.rows * N).astype(np.float32)).cuda().to(tdt)
    Y = torch.from_numpy(rng.uniform(-1, 1, vb.cols * N).astype(np.float32)).cuda().to(tdt)
    G = torch.zeros(nztot, dtype=torch.float32, device="cuda")
    Ct = torch.zeros(vb.cols * N, dtype=torch.float32, device="cuda")
    W0 = torch.from_numpy(np.ascontiguousarray(vb.mab, np.float32)).cuda()

    def pruned_handle(s, skip):
        """(handle, values, pruner): the headline handle pruned to s by a BlockPruner of its own"""
        H = vb.to_device(0, dtype=sdt, updatable=True, transposable=True)
        W = W0.clone().requires_grad_(True)
        opt = sa.VbsAdamW([(H, W)], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
        p = sa.BlockPruner(opt, skip_pruned=True) if skip else sa.BlockPruner(opt)
        p.prune(s)
        return H, W, opt, p

    arms, info = {}, {}
    H_plain = vb.to_device(0, dtype=sdt, updatable=True, transposable=True)
    arms["sddmm"] = lambda: H_plain.sddmm(X, Y, G, N)
    arms["spmm_t"] = lambda: H_plain.spmm_t(X, Ct, N)
    keep = []
    if has_live:
        for s in (0.0, 0.5, 0.75, 0.9):
            H, _, _, p = pruned_handle(s, True)
            tag = "%g" % (100 * s)
            arms["sddmm_" + tag] = lambda H=H: H.sddmm(X, Y, G, N)
            arms["spmm_t_" + tag] = lambda H=H: H.spmm_t(X, Ct, N)
            info[tag] = H.live_info()
            keep.append((H, p))                      # (alive for the run)
            if s == 0.5:
                arms["set_live_blocks"] = lambda H=H, k=p.keep_masks()[0]: H.set_live_blocks(k)
    x_in = torch.from_numpy(rng.uniform(-1, 1, (N, vb.cols)).astype(np.float32)).cuda().to(tdt)
    gy = torch.from_numpy(rng.uniform(-1, 1, (N, vb.rows)).astype(np.float32)).cuda()

    def step_arm(s, skip):
        H, W, opt, p = pruned_handle(s, skip)
        ctl = sa.GradCtl(loss_scale=1.0, max_norm=1.0, growth_interval=2000)
        x = x_in.clone().requires_grad_(True)

        def step():
            opt.zero_grad()
            x.grad = None
            y = vbs_linear(x, H, W)
            y.backward(gy.to(y.dtype))
            if not skip:
                p.mask_grads()
            ctl.collect(opt)
            opt.step(ctl=ctl)
        keep.append((H, p))
        return step

    for s in (0.5, 0.9):
        arms["step_mask_%g" % (100 * s)] = step_arm(s, False)
        if has_live:
            arms["step_skip_%g" % (100 * s)] = step_arm(s, True)

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
    r5 = lambda x: round(float(x), 5)      # noqa: E731
    rec = {"dtype": args.dtype, "commit": args.commit, "has_live": has_live, "rows": int(vb.rows), "cols": int(vb.cols), "nztot": nztot, "N": N, "reps": args.reps,
           "ms_med_p10_p90": {k: [r5(np.median(t)), r5(np.percentile(t, 10)), r5(np.percentile(t, 90))] for k, t in times.items()}, "live_info": info}
    line = json.dumps(rec)
    print(line)
    if args.save:
        out = os.path.join(HERE, "profiles", "live")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "live_record.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
