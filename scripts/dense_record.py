"""Dense <-> blocks (DeviceVBS.gather_dense / scatter_dense, sparta_amd.dense_block_ssq, sparta_amd.sparsify; k_dense.hip) on one layer: 8192 x 8192, blocks of
64 x 64, with 0 / 50 / 90 % of the 16384 grid blocks dropped (a seeded random block mask per level), D row-major in float32 and bfloat16.  The method of
scripts/repattern_record.py: HIP events around each arm on an idle stream, all arms of the process interleaved call by call in a new seeded order every
round, median and 10th / 90th percentile of the timed calls.  Per level S and type of D:
  gather_S_T         gather_dense into a preallocated values tensor
  scatter_S_T        scatter_dense with fill=False;  scatter_fill_S_T  with fill=True (the fill launch stores the whole rows x cols region first)
  copy_S_T           the floor: ONE torch copy that moves as many bytes as the gather (reads nztot elements of D, writes nztot floats)
  torch_S_T          the torch restatement for uniform blocks: D.view(br, h, bc, w).permute(0, 2, 3, 1)[mask].float() (allocates its result)
  ssq_T              dense_block_ssq of the whole matrix (once per type: it does not depend on the level)
and, wall clock around a synchronised call (median of --reps-d runs):
  sparsify_S_T       the whole sparta_amd.sparsify(D, 64, row_block_size=64, sparsity=S): scores, select, the mask download, the pattern, the handle,
                     gather_dense, set_values
  host_S             the route a checkout without this feature offers (float32 only): download D, mask it and build a CSR with numpy,
                     VBR.fill_from_CSR_inplace_fixed, to_device, upload mab
One JSON line, appended to profiles/dense/dense_record.jsonl with --save.

    python scripts/dense_record.py [--reps 50] [--reps-d 3] [--levels 0,50,90] [--size 8192] [--commit REV] [--save]"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("SPARTA_AMD_ROOT") or HERE
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--reps-d", type=int, default=3)
    ap.add_argument("--levels", default="0,50,90")
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--commit", default="", help="revision the numbers are taken on (recorded as given)")
    ap.add_argument("--save", action="store_true")
    args = ap.parse_args()
    import torch
    import sparta_amd as sa
    n, hb, w = args.size, 64, 64
    nb = n // hb
    rng = np.random.default_rng(1)
    D32 = torch.from_numpy(rng.uniform(-1, 1, (n, n)).astype(np.float32)).cuda()
    Ds = {"f32": D32, "bf16": D32.to(torch.bfloat16)}
    esz = {"f32": 4, "bf16": 2}
    rp = np.arange(0, n + 1, hb, dtype=np.int64)
    rp_dev = torch.as_tensor(rp, device="cuda")
    arms, wall, sizes, keepalive = {}, {}, {}, []

    def timed_wall(fn):
        ts = []
        for _ in range(args.reps_d):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return ts

    def host_route(mask):
        Dh = D32.cpu().numpy()
        Dm = Dh * np.kron(mask, np.ones((hb, w), np.float32))
        r, c = np.nonzero(Dm)
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int64)
        cm = sa.CSR(n, n, rowptr, c.astype(np.int32), Dm[r, c])
        vb = sa.VBR().fill_from_CSR_inplace_fixed(cm, hb, w)
        H = vb.to_device(0, updatable=True, transposable=True)
        W = torch.from_numpy(vb.mab).cuda()
        torch.cuda.synchronize()
        H.close()
        return W

    for name, D in Ds.items():
        ssq = torch.empty((nb, nb), dtype=torch.float64, device="cuda")
        arms["ssq_" + name] = lambda D=D, ssq=ssq: sa.dense_block_ssq(D, rp_dev, w, out=ssq)
    for s in [int(x) for x in args.levels.split(",")]:
        mask = (np.random.default_rng(100 + s).permutation(nb * nb) >= (s * nb * nb) // 100).astype(np.uint8).reshape(nb, nb)
        mask_dev = torch.from_numpy(mask).cuda().bool()
        vb, H, W = sa.sparsify(D32, w, row_part=rp, mask=mask, transposable=False)
        W = W.detach()
        nz = W.numel()
        sizes["%d" % s] = {"blocks": int(mask.sum()), "nztot": int(nz)}
        for name, D in Ds.items():
            tag = "%d_%s" % (s, name)
            out = torch.empty_like(D)
            moved = nz * (esz[name] + 4) // 2
            src, dst = torch.empty(moved, dtype=torch.uint8, device="cuda"), torch.empty(moved, dtype=torch.uint8, device="cuda")
            Wg = torch.empty_like(W)
            arms["gather_" + tag] = lambda H=H, D=D, Wg=Wg: H.gather_dense(D, out=Wg)
            arms["scatter_" + tag] = lambda H=H, W=W, out=out: H.scatter_dense(W, out, fill=False)
            arms["scatter_fill_" + tag] = lambda H=H, W=W, out=out: H.scatter_dense(W, out, fill=True)
            arms["copy_" + tag] = lambda src=src, dst=dst: dst.copy_(src)
            arms["torch_" + tag] = lambda D=D, m=mask_dev: D.view(nb, hb, nb, w).permute(0, 2, 3, 1)[m].float()
            keepalive.append((out, src, dst, Wg))
            wall["sparsify_" + tag] = timed_wall(lambda D=D: sa.sparsify(D, w, row_block_size=hb, sparsity=s / 100.0)[1].close())
        wall["host_%d" % s] = timed_wall(lambda: host_route(mask))
        keepalive.append((vb, H, W, mask_dev))
        print("level %d set up" % s, file=sys.stderr, flush=True)

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def call(k, timed=None):
        if timed is None:
            arms[k]()
        else:
            e0.record(); arms[k](); e1.record(); e1.synchronize()
            timed.append(e0.elapsed_time(e1))

    for _ in range(3):
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
    mp = lambda t: [r5(np.median(t)), r5(np.percentile(t, 10)), r5(np.percentile(t, 90))]      # noqa: E731
    rec = {"commit": args.commit, "rows": n, "cols": n, "h": hb, "w": w, "reps": args.reps, "reps_d": args.reps_d, "sizes": sizes,
           "ms_med_p10_p90": {k: mp(t) for k, t in times.items()},
           "wall_ms_med_min_max": {k: [r5(np.median(t)), r5(min(t)), r5(max(t))] for k, t in wall.items()}}
    line = json.dumps(rec)
    print(line)
    if args.save:
        out = os.path.join(HERE, "profiles", "dense")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "dense_record.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
