"""The fp8 image with a live-block set (DeviceVBS.set_a8_live) on the handle bench.py builds for its headline config (cant-like FEM, Jaccard -a 5 -t 0.6,
w = 32, N = 128, made updatable and transposable).  Arms, interleaved in one process in a seeded random order, HIP events, medians of --reps calls with the
10th and 90th percentile.  With the new switch off (these run on a tree without the switch too -- the parent commit: SPARTA_AMD_ROOT=<its checkout>):
  spmm_plain                     the 16-bit product, no switch
  spmm_a8                        the product under set_forward_a8, no live set (form 3)
  spmm_live_P                    the product under set_live_forward with P % of the blocks pruned, P = 0 / 50 / 75 / 90 (form 2)
  set_values_a8 / adam_a8        sparta_vbs_set_values / sparta_vbs_adam_step with the fp8 switch on (one quantise launch behind each)
  set_live_blocks_live           sparta_vbs_set_live_blocks under live forward (word kernel + compaction), 50 % pruned
With the new switch on:
  spmm_a8live_P                  the product under set_forward_a8 + set_a8_live with P % pruned (form 4)
  set_values_a8live / adam_a8live / set_live_blocks_a8live     the same calls with the scale-placement launch behind them, 50 % pruned
Appended to profiles/a8_live/<--out> with --save.

--switch 0 leaves the arms of the new switch out: the same arms as the parent's run, for the comparison with it (more arms in the rotation mean colder caches
for every one of them).  One JSON line per run.

    python scripts/a8_live_record.py [--dtype f16|bf16] [--reps 50] [--switch 1] [--commit REV] [--out a8_live_record.jsonl] [--save]"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("SPARTA_AMD_ROOT") or HERE
sys.path.insert(0, ROOT)

PRUNED = (0, 50, 75, 90)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=["f16", "bf16"], default="f16")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--commit", default="", help="revision the numbers are taken on (recorded as given)")
    ap.add_argument("--switch", type=int, default=1, help="0: leave the arms of the new switch out (the parent's arms only)")
    ap.add_argument("--out", default="a8_live_record.jsonl")
    ap.add_argument("--save", action="store_true")
    args = ap.parse_args()
    import torch
    import sparta_amd as sa
    sdt = {"f16": sa.F16, "bf16": sa.BF16}[args.dtype]
    tdt = {"f16": torch.float16, "bf16": torch.bfloat16}[args.dtype]
    has_switch = hasattr(sa.DeviceVBS, "set_a8_live") and args.switch != 0
    w, N = 32, 128
    arms, info, hold = {}, {}, []

    m = sa.gen.fem3d(9, 9, 257, 3, 2)                          # gen.cant_like(seed=2), the headline matrix
    eng = sa.BlockingEngine(blocking_algo=5, tau=0.6, col_block_size=w, row_block_size=32, force_fixed_size=True, sim_measure=1)
    vb = sa.VBR().fill_from_CSR_inplace(m, eng.GetGrouping(m), w, 32, True)
    rng = np.random.default_rng(1)
    ldb = vb.cols + (vb.cols & 1)
    nz = int(vb.nztot)
    B = torch.from_numpy(rng.uniform(-1, 1, ldb * N).astype(np.float32)).cuda().to(tdt)
    C = torch.zeros(vb.rows * N, dtype=torch.float32, device="cuda")
    W0 = torch.from_numpy(np.ascontiguousarray(vb.mab, np.float32)).cuda()
    G = torch.from_numpy(rng.uniform(-1e-3, 1e-3, nz).astype(np.float32)).cuda()

    def handle():
        H = vb.to_device(0, dtype=sdt, updatable=True, transposable=True)
        W = W0.clone()
        hold.append((H, W))
        return H, W

    def keep_of(H, pruned):
        k = np.ones(H.n_blocks, np.uint8)
        k[np.random.default_rng(100 + pruned).permutation(H.n_blocks)[:(H.n_blocks * pruned) // 100]] = 0
        return torch.from_numpy(k).cuda()

    def spmm(H):
        return lambda: H.spmm(B, C, N, ldb=ldb, ldc=vb.rows)

    def steps(tag, H, W):
        M, V = torch.zeros_like(W), torch.zeros_like(W)
        S = torch.zeros(8, dtype=torch.int32, device="cuda")
        hold.append((M, V, S))
        arms["set_values_" + tag] = lambda: H.set_values(W)
        arms["adam_" + tag] = lambda: H.adam_step(W, G, M, V, S, lr=1e-4)

    H, W = handle()
    H.set_values(W)
    arms["spmm_plain"] = spmm(H)
    H, W = handle()
    H.set_forward_a8(True, values=W)
    arms["spmm_a8"] = spmm(H)
    steps("a8", H, W)
    for pruned in PRUNED:
        H, W = handle()
        H.set_values(W)
        k = keep_of(H, pruned)
        H.set_live_blocks(k)
        H.set_live_forward(True)
        arms["spmm_live_%d" % pruned] = spmm(H)
        if pruned == 50:
            arms["set_live_blocks_live"] = lambda H=H, k=k: H.set_live_blocks(k)
        hold.append(k)
        H.spmm(B, C, N, ldb=ldb, ldc=vb.rows)
        torch.cuda.synchronize()
        info["live_%d" % pruned] = H.live_forward_info()
    if has_switch:
        for pruned in PRUNED:
            H, W = handle()
            H.set_forward_a8(True, values=W)
            k = keep_of(H, pruned)
            H.set_live_blocks(k)
            H.set_a8_live(True)
            arms["spmm_a8live_%d" % pruned] = spmm(H)
            if pruned == 50:
                arms["set_live_blocks_a8live"] = lambda H=H, k=k: H.set_live_blocks(k)
                steps("a8live", H, W)
            hold.append(k)
            H.spmm(B, C, N, ldb=ldb, ldc=vb.rows)
            torch.cuda.synchronize()
            info["a8live_%d" % pruned] = dict(H.a8_live_info(), form=max(H.a8_info()["form_one_tile"], H.a8_info()["form_pair"]))
    info["handle"] = {"rows": int(vb.rows), "cols": int(vb.cols), "nztot": nz, "n_blocks": int(hold[0][0].n_blocks)}

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
    rec = {"dtype": args.dtype, "commit": args.commit, "has_switch": has_switch, "N": N, "reps": args.reps,
           "ms_med_p10_p90": {k: [r5(np.median(t)), r5(np.percentile(t, 10)), r5(np.percentile(t, 90))] for k, t in times.items()}, "info": info}
    line = json.dumps(rec)
    print(line)
    if args.save:
        out = os.path.join(HERE, "profiles", "a8_live")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, os.path.basename(args.out)), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
