"""Packed against direct fp32 plan (SPARTA_F32_PLAN) on matrices of the benchmark set: one JSON line per matrix -> profiles/packed/packed_record.jsonl.
Both handles of a matrix are made in one process, timed with HIP events in alternating rounds (N = 128, column-major B and C).

    python scripts/packed_record.py [--save]
    python scripts/packed_record.py --sweep [--save]      synthetic plans around the two constants of the plan rule -> profiles/packed/rule_sweep.jsonl:
                                                          (a) 20 000 block steps with 4 .. 23 % of them saved, (b) 23 % saved on 1000 .. 16 000 block steps"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench_suite  # noqa: E402
import sparta_amd as sa  # noqa: E402

N, ROUNDS, REPS = 128, 5, 200
WANT = ("FEM 3D 9x9x257", "FEM 3D 20x20x50", "banded 200k")


def timed(d, B, C):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        d.spmm(B, C, N)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def synthetic(n_tiles, nb, p_half, seed):
    """n_tiles tiles of 32 rows x nb stored 32 x 32 blocks near the diagonal; a share p_half of the blocks holds zeros in its columns 16 .. 31 (two of them share a step)"""
    rng = np.random.default_rng(seed)
    n_bcols = max(n_tiles, 64)
    jab = np.concatenate([np.sort(rng.choice(np.arange(max(0, min(t - 20, n_bcols - 41)), max(0, min(t - 20, n_bcols - 41)) + 41), nb, replace=False)) for t in range(n_tiles)]).astype(np.int64)
    mab = rng.uniform(-1, 1, (n_tiles * nb, 1024)).astype(np.float32)
    mab[rng.random(n_tiles * nb) < p_half, 512:] = 0.0
    return sa.VBR.from_arrays(32 * n_tiles, 32 * n_bcols, 32, np.arange(n_tiles + 1, dtype=np.int64) * 32, np.full(n_tiles, nb, np.int64), jab, mab.reshape(-1))


def sweep():
    os.environ["SPARTA_SPARSE_K"] = "0"
    lines = []
    grid = [("saving", 2000, p) for p in (0.1, 0.2, 0.3, 0.4, 0.5)] + [("size", t, 0.5) for t in (100, 200, 400, 800, 1600)]
    for what, n_tiles, p in grid:
        v = synthetic(n_tiles, 10, p, 7)
        hs = {}
        for plan in ("direct", "packed"):
            os.environ["SPARTA_F32_PLAN"] = plan
            hs[plan] = v.to_device(0)
        os.environ.pop("SPARTA_F32_PLAN")
        auto = v.to_device(0)
        B = torch.rand(v.cols * N, device="cuda") - 0.5
        C = {q: torch.zeros(v.rows * N, device="cuda") for q in hs}
        for q, d in hs.items():
            for _ in range(20):
                d.spmm(B, C[q], N)
        torch.cuda.synchronize()
        ms = {q: [] for q in hs}
        for _ in range(ROUNDS):
            for q, d in hs.items():
                ms[q].append(round(timed(d, B, C[q]), 5))
        pi = hs["packed"].packed_info()
        rec = {"sweep": what, "tiles": n_tiles, "share_of_half_blocks": p, "block_steps": pi["block_steps"], "packed_steps": pi["steps"],
               "steps_saved": round(1.0 - pi["steps"] / max(pi["block_steps"], 1), 4), "rule_packs": auto.packed_info()["packed"], "last_path": hs["packed"].info()["last_path"],
               "direct_ms": ms["direct"], "packed_ms": ms["packed"], "direct_median": float(np.median(ms["direct"])), "packed_median": float(np.median(ms["packed"])),
               "kernel_rev": sa.KERNEL_REV}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        for d in list(hs.values()) + [auto]:
            d.close()
    if "--save" in sys.argv:
        out = os.path.join(ROOT, "profiles", "packed")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "rule_sweep.jsonl"), "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


def main():
    if "--sweep" in sys.argv:
        return sweep()
    lines = []
    for name, kind, make, eng_kw, w in bench_suite.cases(sa):
        if not name.startswith(WANT):
            continue
        m = make()
        g = sa.BlockingEngine(col_block_size=w, **eng_kw).GetGrouping(m)
        hs = {}
        for plan in ("direct", "packed"):
            os.environ["SPARTA_F32_PLAN"] = plan
            hs[plan] = sa.DeviceVBS.from_csr(m, g, w, eng_kw.get("row_block_size", 0), eng_kw.get("force_fixed_size", False))
        os.environ.pop("SPARTA_F32_PLAN")
        auto = sa.DeviceVBS.from_csr(m, g, w, eng_kw.get("row_block_size", 0), eng_kw.get("force_fixed_size", False))
        B = torch.rand(auto.cols * N, device="cuda") - 0.5
        C = {p: torch.zeros(auto.rows * N, device="cuda") for p in hs}
        for p, d in hs.items():
            for _ in range(20):
                d.spmm(B, C[p], N)
        torch.cuda.synchronize()
        ms = {p: [] for p in hs}
        for _ in range(ROUNDS):
            for p, d in hs.items():
                ms[p].append(round(timed(d, B, C[p]), 5))
        pi = hs["packed"].packed_info()
        scale = float(C["direct"].abs().max())
        rec = {"name": name, "rows": int(m.rows), "nnz": int(m.nztot()), "n_cols": N, "block_steps": pi["block_steps"], "packed_steps": pi["steps"], "slots": pi["slots"],
               "steps_saved": round(1.0 - pi["steps"] / max(pi["block_steps"], 1), 4), "rule_packs": auto.packed_info()["packed"],
               "direct_ms": ms["direct"], "packed_ms": ms["packed"], "direct_median": float(np.median(ms["direct"])), "packed_median": float(np.median(ms["packed"])),
               "max_abs_diff_over_max_abs": float((C["direct"] - C["packed"]).abs().max()) / max(scale, 1e-30), "kernel_rev": sa.KERNEL_REV}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        for d in list(hs.values()) + [auto]:
            d.close()
    if "--save" in sys.argv:
        out = os.path.join(ROOT, "profiles", "packed")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "packed_record.jsonl"), "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
