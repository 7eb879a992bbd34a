"""sparta_vbs_spmm_t on the handle bench.py builds for its headline config (cant-like FEM, Jaccard -a 5 -t 0.6, w = 32, row_block 32,
force_fixed_size), N = 128: medians of event times (device-pointer calls, warm-up first) of
  spmm_t_ms                 the transposed product on a handle with both creation flags
  spmm_ms                   the forward product on the same handle, interleaved with it
  set_values_ms             with and without the transpose flag (16-bit: + the write of the second image), against a device copy of nztot floats
and, with --parent (only entries that exist before this feature: run it with SPARTA_AMD_ROOT pointing at a build of the parent commit),
  create_transposed_ms      sparta_vbs_create_transposed of the same matrix -- what a caller had to redo after every change of A's values
  transposed_product_ms     the static product on that handle (row-major operands, device pointers: what sparta_vbs_spmm_ba launches)
One JSON line, appended to profiles/spmm_t/spmm_t_record.jsonl with --save.

    python scripts/spmm_t_record.py [--dtype f32|f16|bf16] [--reps 50] [--commit REV] [--parent] [--save]

Kernel times: run it under `rocprofv3 --kernel-trace --stats`; counters in `rocprofv3 --pmc ...` runs of their own (no tracing beside them)."""
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
    ap.add_argument("--dtype", choices=["f32", "f16", "bf16"], default="f32")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--commit", default="", help="revision the numbers are taken on (recorded as given)")
    ap.add_argument("--parent", action="store_true", help="the route of the commit before the feature: create_transposed + its product")
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
    rec = {"dtype": args.dtype, "commit": args.commit, "rows": int(vb.rows), "cols": int(vb.cols), "nztot": nztot, "N": N, "reps": args.reps}

    def med(f):
        return round(float(np.median([f() for _ in range(args.reps)])), 5)

    if args.parent:
        tr = []
        d = None
        for _ in range(3):
            if d is not None:
                d.close()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d = sa.DeviceVBS.transposed_of(vb, device=0, dtype=sdt)
            torch.cuda.synchronize()
            tr.append((time.perf_counter() - t0) * 1e3)
        rec["create_transposed_ms"] = round(float(np.median(tr)), 3)
        X = torch.from_numpy(rng.uniform(-1, 1, vb.rows * N).astype(np.float32)).cuda().to(tdt)       # row-major rows(A) x N
        Ct = torch.zeros(vb.cols * N, dtype=torch.float32, device="cuda")
        try:
            for _ in range(5):
                d.spmm(X, Ct, N, b_layout=sa.ROW_MAJOR, c_layout=sa.ROW_MAJOR)
            rec["transposed_product_ms"] = med(lambda: d.spmm(X, Ct, N, b_layout=sa.ROW_MAJOR, c_layout=sa.ROW_MAJOR, timed=True))
        except sa.SpartaError as e:
            rec["transposed_product_ms"] = None
            rec["transposed_product_error"] = str(e)
            # (16-bit handles refuse row-major operands: sparta_vbs_spmm_ba has no 16-bit form; the column-major product of the same handle for scale)
            Ct2 = torch.zeros(vb.cols * N, dtype=torch.float32, device="cuda")
            for _ in range(5):
                d.spmm(X, Ct2, N)
            rec["transposed_product_colmajor_ms"] = med(lambda: d.spmm(X, Ct2, N, timed=True))
        d.close()
    else:
        V1 = (vb.mab * rng.uniform(0.5, 1.5, nztot)).astype(np.float32)
        H = vb.to_device(0, dtype=sdt, updatable=True, transposable=True)
        U = vb.to_device(0, dtype=sdt, updatable=True)
        B = torch.from_numpy(rng.uniform(-1, 1, vb.cols * N).astype(np.float32)).cuda().to(tdt)
        X = torch.from_numpy(rng.uniform(-1, 1, vb.rows * N).astype(np.float32)).cuda().to(tdt)
        C = torch.zeros(vb.rows * N, dtype=torch.float32, device="cuda")
        Ct = torch.zeros(vb.cols * N, dtype=torch.float32, device="cuda")
        W = torch.from_numpy(V1).cuda()
        W2 = torch.empty_like(W)
        for _ in range(5):
            H.set_values(W); U.set_values(W); H.spmm(B, C, N); U.spmm(B, C, N); H.spmm_t(X, Ct, N); W2.copy_(W)
        torch.cuda.synchronize()
        t_f, t_t, t_u = [], [], []
        for _ in range(3):                                          # three repetitions, interleaved: the spread is the run-to-run noise
            f, t, u = [], [], []
            for _ in range(args.reps):
                f.append(H.spmm(B, C, N, timed=True)); t.append(H.spmm_t(X, Ct, N, timed=True)); u.append(U.spmm(B, C, N, timed=True))
            t_f.append(round(float(np.median(f)), 5)); t_t.append(round(float(np.median(t)), 5)); t_u.append(round(float(np.median(u)), 5))
        rec["spmm_ms"], rec["spmm_t_ms"], rec["spmm_plain_flags_ms"] = t_f, t_t, t_u
        rec["spmm_t_over_spmm"] = round(float(np.median(t_t)) / float(np.median(t_f)), 3)
        rec["set_values_ms_transposable"] = med(lambda: H.set_values(W, timed=True))
        rec["set_values_ms"] = med(lambda: U.set_values(W, timed=True))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def copy_ms():
            e0.record(); W2.copy_(W); e1.record(); e1.synchronize()
            return e0.elapsed_time(e1)
        rec["copy_ms"] = med(copy_ms)
        rec["a_bytes_transposable"], rec["a_bytes"] = int(H.info()["a_bytes"]), int(U.info()["a_bytes"])
        extra = rec["a_bytes_transposable"] - rec["a_bytes"] if sdt != sa.F32 else 0
        rec["set_values_floor_ms_transposable"] = round(rec["copy_ms"] * (4 * nztot + rec["a_bytes_transposable"]) / (8.0 * nztot), 5) if sdt != sa.F32 else None
        rec["second_image_bytes"] = int(extra)
        # what the product computes, once: against float64 on a sample of columns of A
        Ch = Ct.cpu().numpy().reshape(N, vb.cols)
        rec["ct_finite"] = bool(np.isfinite(Ch).all())
        H.close(); U.close()
    line = json.dumps(rec)
    print(line)
    if args.save:
        out = os.path.join(HERE, "profiles", "spmm_t")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "spmm_t_record.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
