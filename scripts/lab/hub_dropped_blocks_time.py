"""Time of a hub-carried 16-bit product whose group tiles have absent sub-tiles (k_hub16.hip): the configuration of profiles/poison/ab_timings.json,
"hub_product".  2048 x 8192, 64 x 64 blocks, a seeded 30 % of the blocks dropped, so that four block-rows of a group tile store different block columns
(union area ~ 1.4 x stored area); bf16, n = 512, SPARTA_HUB_G = 4.  Prints one JSON line: the hub plan and the median / min / max of the timed products in us.
For a before / after comparison run it once per library build, the builds interleaved, one process per run:

    python scripts/lab/hub_dropped_blocks_time.py [--products 60] [--warmup 10] [--seed 1]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--products", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--drop", type=float, default=0.3)
    ap.add_argument("--n", type=int, default=512)
    args = ap.parse_args()
    os.environ.setdefault("SPARTA_HUB_G", "4")
    os.environ.setdefault("SPARTA_HUB_MIN_TOTAL", "1")
    os.environ.setdefault("SPARTA_HUB_MIN_STEPS", "1")
    os.environ.setdefault("SPARTA_HUB_TAU", "0.25")
    os.environ.setdefault("SPARTA_SPARSE_K", "0")
    import torch
    import sparta_amd as sa

    rows, cols, w, h = 2048, 8192, 64, 64
    rng = np.random.default_rng(args.seed)
    keep = rng.random((rows // h, cols // w)) >= args.drop
    keep[:, 0] |= ~keep.any(axis=1)
    nzcount = keep.sum(axis=1).astype(np.int64)
    jab = np.concatenate([np.flatnonzero(k) for k in keep]).astype(np.int64)
    mab = rng.uniform(-1, 1, int(nzcount.sum()) * h * w).astype(np.float32)
    v = sa.VBR.from_arrays(rows, cols, w, np.arange(0, rows + 1, h, dtype=np.int64), nzcount, jab, mab)
    d = v.to_device(0, dtype=sa.BF16)
    hub = d.hub_info()
    n = args.n
    B = torch.from_numpy(rng.uniform(-1, 1, cols * n).astype(np.float32)).to(torch.bfloat16).cuda()
    C = torch.zeros(rows * n, dtype=torch.float32, device="cuda")
    for _ in range(args.warmup):
        d.spmm(B, C, n)
    us = sorted(1000.0 * d.spmm(B, C, n, timed=True) for _ in range(args.products))
    torch.cuda.synchronize()
    print(json.dumps({"hub": hub, "stored_blocks": int(nzcount.sum()), "n": n, "products": args.products,
                      "us_median": us[len(us) // 2], "us_min": us[0], "us_max": us[-1]}))
    d.close()


if __name__ == "__main__":
    main()
