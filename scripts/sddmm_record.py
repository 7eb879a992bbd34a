"""SDDMM against the forward product on the handle bench.py builds for its headline config (cant-like FEM, Jaccard -a 5 -t 0.6, w = 32,
row_block 32, force_fixed_size; N = k = 128): the kernel time of each (events around the launches, median of the timed calls), the SDDMM's
2 * nztot * k / t and the ratio of the two times.  One JSON line.

    python scripts/sddmm_record.py [--dtype f32|f16|bf16] [--k 128] [--reps 50]

Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times (the events include the launch)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=["f32", "f16", "bf16"], default="f32")
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    import torch
    import sparta_amd as sa
    sdt = {"f32": sa.F32, "f16": sa.F16, "bf16": sa.BF16}[args.dtype]
    tdt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[args.dtype]
    w, N, k = 32, 128, args.k
    m = sa.gen.cant_like(seed=2)
    eng = sa.BlockingEngine(blocking_algo=5, tau=0.6, col_block_size=w, row_block_size=32, force_fixed_size=True, sim_measure=1)
    vb = sa.VBR().fill_from_CSR_inplace(m, eng.GetGrouping(m), w, 32, True)
    d = vb.to_device(0, dtype=sdt)
    rng = np.random.default_rng(1)
    B = torch.from_numpy(rng.uniform(-1, 1, vb.cols * N).astype(np.float32)).cuda().to(tdt)
    C = torch.zeros(vb.rows * N, dtype=torch.float32, device="cuda")
    X = torch.from_numpy(rng.uniform(-1, 1, vb.rows * k).astype(np.float32)).cuda().to(tdt)
    Y = torch.from_numpy(rng.uniform(-1, 1, vb.cols * k).astype(np.float32)).cuda().to(tdt)
    G = torch.zeros(int(vb.nztot), dtype=torch.float32, device="cuda")
    for _ in range(5):
        d.spmm(B, C, N)
        d.sddmm(X, Y, G, k)
    torch.cuda.synchronize()
    t_spmm = float(np.median([d.spmm(B, C, N, timed=True) for _ in range(args.reps)]))
    t_sddmm = float(np.median([d.sddmm(X, Y, G, k, timed=True) for _ in range(args.reps)]))
    print(json.dumps({"dtype": args.dtype, "rows": int(vb.rows), "cols": int(vb.cols), "nztot": int(vb.nztot), "block_rows": int(vb.block_rows),
                      "N": N, "k": k, "spmm_ms": round(t_spmm, 5), "sddmm_ms": round(t_sddmm, 5),
                      "sddmm_tflops": round(2.0 * vb.nztot * k / (t_sddmm * 1e-3) / 1e12, 2), "sddmm_over_spmm": round(t_sddmm / t_spmm, 3)}))


if __name__ == "__main__":
    main()
