"""The block scores of the SDDMM (sparta_vbs_sddmm_block_ssq) and BlockPruner.regrow on the handle bench.py builds for its headline config (cant-like FEM,
Jaccard -a 5 -t 0.6, w = 32, row_block 32, force_fixed_size), made updatable and transposable, N = k = 128.  The method of scripts/prune_record.py and
scripts/live_record.py: HIP events around each arm on an idle stream (the host side of an arm is inside its window), all arms interleaved call by call in one
process in a new seeded order every round, median and 10th / 90th percentile of the timed calls.  Arms, at S = 50 / 75 / 90 % of the blocks pruned by
BlockPruner(skip_pruned=True, live_steps=True).prune:
  score_S        (a) sddmm_block_ssq(sel = the pruned blocks) on the pruned handle, live set installed: the lists of sel, the product, the final sums
  two_pass       (b) what it replaces, on a handle without a live set: sddmm into a scratch G of nztot floats, then block_ssq(G); the two parts also alone
                 (two_pass_sddmm, two_pass_block_ssq).  The same work at every S: the dead blocks have to be computed to be scored.
  score_all      sddmm_block_ssq(sel = None): every block scored
  regrow_S       (c) one BlockPruner.regrow(0.3) call (scores, select_swap, masks, set_values, the live set and its switches); the probe holds the scores of one
                 backward, left as they are between the calls
One JSON line, appended to profiles/regrow/regrow_record.jsonl with --save.

    python scripts/regrow_record.py [--dtype f32|f16|bf16] [--reps 50] [--commit REV] [--save]"""
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
    sdt = {"f32": sa.F32, "f16": sa.F16, "bf16": sa.BF16}[args.dtype]
    tdt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[args.dtype]
    w, N = 32, 128
    m = sa.gen.cant_like(seed=2)
    eng = sa.BlockingEngine(blocking_algo=5, tau=0.6, col_block_size=w, row_block_size=32, force_fixed_size=True, sim_measure=1)
    vb = sa.VBR().fill_from_CSR_inplace(m, eng.GetGrouping(m), w, 32, True)
    nztot = int(vb.nztot)
    rng = np.random.default_rng(1)
    X = torch.from_numpy(rng.uniform(-1, 1, vb.rows * N).astype(np.float32)).cuda().to(tdt)
    Y = torch.from_numpy(rng.uniform(-1, 1, vb.cols * N).astype(np.float32)).cuda().to(tdt)
    G = torch.zeros(nztot, dtype=torch.float32, device="cuda")
    W0 = torch.from_numpy(np.ascontiguousarray(vb.mab, np.float32)).cuda()

    arms, info, alive = {}, {}, []
    H_plain = vb.to_device(0, dtype=sdt, updatable=True, transposable=True)
    out_plain = torch.zeros(H_plain.n_blocks, dtype=torch.float64, device="cuda")
    arms["two_pass_sddmm"] = lambda: H_plain.sddmm(X, Y, G, N)
    arms["two_pass_block_ssq"] = lambda: H_plain.block_ssq(G, out=out_plain)
    arms["two_pass"] = lambda: (H_plain.sddmm(X, Y, G, N), H_plain.block_ssq(G, out=out_plain))
    arms["score_all"] = lambda: H_plain.sddmm_block_ssq(X, Y, N, out=out_plain)
    for s in (0.5, 0.75, 0.9):
        H = vb.to_device(0, dtype=sdt, updatable=True, transposable=True)
        W = W0.clone().requires_grad_(True)
        opt = sa.VbsAdamW([(H, W)], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
        p = sa.BlockPruner(opt, skip_pruned=True, live_steps=True)
        p.prune(s)
        W.grad = torch.zeros_like(W)
        H.sddmm(X, Y, W.grad, N)
        opt.step()                                               # (the optimizer's state exists: regrow masks it too)
        probe = p.probe(0)
        H.sddmm_block_ssq(X, Y, N, sel=probe.sel, out=probe.out)
        tag = "%g" % (100 * s)
        arms["score_" + tag] = lambda H=H, probe=probe: H.sddmm_block_ssq(X, Y, N, sel=probe.sel, out=probe.out)
        arms["regrow_" + tag] = lambda p=p: p.regrow(0.3)
        info[tag] = H.live_info()
        alive.append((H, W, opt, p))

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
    live_after = {tag: int(H.live_info()["live_blocks"]) for tag, (H, _, _, _) in zip(info, alive)}
    r5 = lambda x: round(float(x), 5)      # noqa: E731
    rec = {"dtype": args.dtype, "commit": args.commit, "rows": int(vb.rows), "cols": int(vb.cols), "nztot": nztot, "n_blocks": int(H_plain.n_blocks), "N": N,
           "reps": args.reps, "ms_med_p10_p90": {k: [r5(np.median(t)), r5(np.percentile(t, 10)), r5(np.percentile(t, 90))] for k, t in times.items()},
           "live_info": info, "live_blocks_after": live_after}
    line = json.dumps(rec)
    print(line)
    if args.save:
        out = os.path.join(HERE, "profiles", "regrow")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "regrow_record.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
