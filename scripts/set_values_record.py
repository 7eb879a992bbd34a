"""sparta_vbs_set_values on the handle bench.py builds for its headline config (cant-like FEM, Jaccard -a 5 -t 0.6, w = 32, row_block 32,
force_fixed_size), made updatable: the time of an update on the device-pointer path (events around the launches, median of the timed calls)
against (a) a device-to-device copy of nztot floats in the same process -- the update reads mab once and writes every image once, so its floor is
copy_ms * (bytes_read + bytes_written) / (2 * 4 * nztot) -- (b) destroying and re-creating the handle, which is what a caller had to do before,
and (c) the forward product on the updated handle against the product on a fresh handle of the same values, interleaved, three repetitions
(the spread of the fresh handle's figure is the run-to-run noise).  One JSON line, appended to profiles/set_values/set_values_record.jsonl with --save.

    python scripts/set_values_record.py [--dtype f32|f16|bf16] [--reps 50] [--commit REV] [--parent-recreate-ms MS] [--save]

Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times (profiles/set_values/kernel_stats_*.csv)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=["f32", "f16", "bf16"], default="f32")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--commit", default="", help="revision the numbers are taken on (recorded as given)")
    ap.add_argument("--parent-recreate-ms", type=float, default=None, help="destroy + create of the same handle measured on the parent commit")
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
    V1 = (vb.mab * rng.uniform(0.5, 1.5, nztot)).astype(np.float32)           # new values, the zero pattern of the old ones
    H = vb.to_device(0, dtype=sdt, updatable=True)
    a_bytes_created = H.info()["a_bytes"]
    B = torch.from_numpy(rng.uniform(-1, 1, vb.cols * N).astype(np.float32)).cuda().to(tdt)
    C = torch.zeros(vb.rows * N, dtype=torch.float32, device="cuda")
    W = torch.from_numpy(V1).cuda()
    W2 = torch.empty_like(W)
    for _ in range(5):
        H.spmm(B, C, N)
        H.set_values(W)
        W2.copy_(W)
    torch.cuda.synchronize()
    info = H.info()
    # bytes: mab read once; every image the handle holds written once
    if sdt == sa.F32:
        frag_bytes = info["stream_steps"] * 1040 * 4
        legacy_held = info["a_bytes"] >= frag_bytes + 4 * nztot
        bytes_written = (4 * nztot if legacy_held else 0) + frag_bytes
    else:
        legacy_held = None
        bytes_written = info["a_bytes"] - 8 * 64 * 64 * 2                     # (the pad behind the last slice is not written)
    bytes_read = 4 * nztot
    t_set = float(np.median([H.set_values(W, timed=True) for _ in range(args.reps)]))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tc = []
    for _ in range(args.reps):
        e0.record(); W2.copy_(W); e1.record(); e1.synchronize()
        tc.append(e0.elapsed_time(e1))
    t_copy = float(np.median(tc))
    floor = t_copy * (bytes_read + bytes_written) / (2.0 * 4.0 * nztot)
    # recreate on THIS commit (the plain entry; --parent-recreate-ms carries the parent's figure into the record)
    tr = []
    d = vb.to_device(0, dtype=sdt)
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d.close()
        d = vb.to_device(0, dtype=sdt)
        torch.cuda.synchronize()
        tr.append((time.perf_counter() - t0) * 1e3)
    d.close()
    # the product after an update against the product of a fresh handle of the same values
    v2 = sa.VBR()
    v2.__dict__.update(vb.__dict__)
    v2.mab, v2._dev, v2._dev_t = V1, None, None
    F = v2.to_device(0, dtype=sdt)
    for _ in range(5):
        H.spmm(B, C, N); F.spmm(B, C, N)
    after, fresh = [], []
    for _ in range(3):
        a, f = [], []
        for _ in range(args.reps):
            a.append(H.spmm(B, C, N, timed=True)); f.append(F.spmm(B, C, N, timed=True))
        after.append(float(np.median(a))); fresh.append(float(np.median(f)))
    rec = {"dtype": args.dtype, "commit": args.commit, "rows": int(vb.rows), "cols": int(vb.cols), "nztot": nztot, "N": N, "reps": args.reps,
           "a_bytes_created": int(a_bytes_created), "a_bytes": int(info["a_bytes"]), "legacy_image_held": legacy_held,
           "bytes_read": int(bytes_read), "bytes_written": int(bytes_written),
           "set_values_ms": round(t_set, 5), "copy_ms": round(t_copy, 5), "floor_ms": round(floor, 5), "set_values_over_floor": round(t_set / floor, 3),
           "recreate_ms_this_commit": round(float(np.median(tr)), 3), "recreate_ms_parent": args.parent_recreate_ms,
           "recreate_over_set_values": round((args.parent_recreate_ms if args.parent_recreate_ms else float(np.median(tr))) / t_set, 1),
           "spmm_after_ms": [round(x, 5) for x in after], "spmm_fresh_ms": [round(x, 5) for x in fresh],
           "spmm_fresh_spread_ms": round(max(fresh) - min(fresh), 5), "fresh_sparse_rows": F.info()["sparse_rows"]}
    line = json.dumps(rec)
    print(line)
    if args.save:
        out = os.path.join(ROOT, "profiles", "set_values")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "set_values_record.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
