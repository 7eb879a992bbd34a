"""The live forward product (sparta_vbs_set_live_forward) on the handle bench.py builds for its headline config (cant-like FEM, Jaccard -a 5 -t 0.6, w = 32,
row_block 32, force_fixed_size), made updatable and transposable, 16-bit, N = 128.  The method of scripts/live_record.py: HIP events around each arm on an idle
stream (the host side of an arm is inside its window), all arms interleaved call by call in one process in a new seeded order every round, median and 10th /
90th percentile of the timed calls.  Arms:
  plain                  the forward product on a handle that never had a live set
  live_S                 the forward product on a handle pruned to S = 0 / 50 / 75 / 90 % of its blocks by BlockPruner(skip_pruned=True, live_forward=True).prune
  off_S                  the same handle class pruned to S = 90 % with live_forward=False: the plain kernels on the full records
  set_live_blocks        the call alone on a handle without live forward (the mask of a 50 % handle): what it cost before
  set_live_blocks_fwd    the same on a handle with live forward built: one more kernel (the compaction; the word kernel too if live steps never built the words)
On a checkout without the feature (SPARTA_AMD_ROOT pointing at a build of the parent commit) only `plain`, `off_90` and `set_live_blocks` run.  The record also
holds, per level, the kept steps and their spread over the worker ranges (the ranges stay as creation balanced them: the range with the most kept steps
bounds the kernel).  One JSON line, appended to profiles/live_forward/live_forward_record.jsonl with --save.

    python scripts/live_forward_record.py [--dtype f16|bf16] [--reps 50] [--commit REV] [--save]"""
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
    ap.add_argument("--dtype", choices=["f16", "bf16"], default="f16")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--commit", default="", help="revision the numbers are taken on (recorded as given)")
    ap.add_argument("--save", action="store_true")
    args = ap.parse_args()
    import torch
    import sparta_amd as sa
    sdt = {"f16": sa.F16, "bf16": sa.BF16}[args.dtype]
    tdt = {"f16": torch.float16, "bf16": torch.bfloat16}[args.dtype]
    has_fwd = hasattr(sa.DeviceVBS, "set_live_forward")
    w, N = 32, 128
    m = sa.gen.cant_like(seed=2)
    eng = sa.BlockingEngine(blocking_algo=5, tau=0.6, col_block_size=w, row_block_size=32, force_fixed_size=True, sim_measure=1)
    vb = sa.VBR().fill_from_CSR_inplace(m, eng.GetGrouping(m), w, 32, True)
    rng = np.random.default_rng(1)
    ldb = vb.cols + (vb.cols & 1)
    B = torch.from_numpy(rng.uniform(-1, 1, ldb * N).astype(np.float32)).cuda().to(tdt)
    C = torch.zeros(vb.rows * N, dtype=torch.float32, device="cuda")
    W0 = torch.from_numpy(np.ascontiguousarray(vb.mab, np.float32)).cuda()

    def pruned_handle(s, fwd):
        H = vb.to_device(0, dtype=sdt, updatable=True, transposable=True)
        W = W0.clone().requires_grad_(True)
        opt = sa.VbsAdamW([(H, W)], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
        p = sa.BlockPruner(opt, skip_pruned=True, live_forward=True) if fwd else sa.BlockPruner(opt, skip_pruned=True)
        p.prune(s)
        return H, p

    arms, info, keepalive = {}, {}, []
    H_plain = vb.to_device(0, dtype=sdt, updatable=True, transposable=True)
    spmm = lambda H: H.spmm(B, C, N, ldb=ldb, ldc=vb.rows)  # noqa: E731
    arms["plain"] = lambda: spmm(H_plain)
    H, p = pruned_handle(0.9, False)
    arms["off_90"] = lambda H=H: spmm(H)
    keepalive.append((H, p))
    H, p = pruned_handle(0.5, False)
    arms["set_live_blocks"] = lambda H=H, k=p.keep_masks()[0]: H.set_live_blocks(k)
    keepalive.append((H, p))
    if has_fwd:
        for s in (0.0, 0.5, 0.75, 0.9):
            H, p = pruned_handle(s, True)
            tag = "%g" % (100 * s)
            arms["live_" + tag] = lambda H=H: spmm(H)
            spmm(H)
            torch.cuda.synchronize()
            fi = H.live_forward_info()
            lists = H.live_forward_lists()
            kept = (lists["ranges_live"][:, 1] - lists["ranges_live"][:, 0]).astype(np.int64)
            full = (lists["ranges"][:, 1] - lists["ranges"][:, 0]).astype(np.int64)
            info[tag] = {"info": fi, "kept_max": int(kept.max()), "kept_mean": round(float(kept.mean()), 2), "kept_min": int(kept.min()),
                         "range_max": int(full.max()), "range_mean": round(float(full.mean()), 2)}
            keepalive.append((H, p))
            if s == 0.5:
                arms["set_live_blocks_fwd"] = lambda H=H, k=p.keep_masks()[0]: H.set_live_blocks(k)

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
    rec = {"dtype": args.dtype, "commit": args.commit, "has_live_forward": has_fwd, "rows": int(vb.rows), "cols": int(vb.cols), "nztot": int(vb.nztot), "N": N,
           "reps": args.reps, "ms_med_p10_p90": {k: [r5(np.median(t)), r5(np.percentile(t, 10)), r5(np.percentile(t, 90))] for k, t in times.items()}, "levels": info}
    line = json.dumps(rec)
    print(line)
    if args.save:
        out = os.path.join(HERE, "profiles", "live_forward")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "live_forward_record.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
