"""The fp8 weight image (DeviceVBS.set_forward_a8) on the handle bench.py builds for its headline config (cant-like FEM, Jaccard -a 5 -t 0.6, w = 32, N = 128,
made updatable and transposable) and on one handle of the same generator twelve times as long, whose 16-bit image lies above 512 MB and so outside the 256 MB
Infinity Cache.  Arms, interleaved in one process in a seeded random order, medians of --reps calls with the 10th and 90th percentile:
  spmm_off / spmm_a8             the forward product with the switch off and on (two handles with the same values)
  set_values_off / set_values_a8 sparta_vbs_set_values without and with the quantise launch behind it
  adam_off / adam_a8             sparta_vbs_adam_step likewise
  big_spmm_off / big_spmm_a8     the product arms on the large handle (--big 0 leaves them out)
A tree without the switch (the parent commit: SPARTA_AMD_ROOT=<its checkout>) runs the *_off arms only.  One JSON line, appended to
profiles/a8/a8_record.jsonl with --save.

    python scripts/a8_record.py [--dtype f16|bf16] [--reps 50] [--big 1] [--commit REV] [--save]"""
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
    ap.add_argument("--big", type=int, default=1)
    ap.add_argument("--commit", default="", help="revision the numbers are taken on (recorded as given)")
    ap.add_argument("--save", action="store_true")
    args = ap.parse_args()
    import torch
    import sparta_amd as sa
    sdt = {"f16": sa.F16, "bf16": sa.BF16}[args.dtype]
    tdt = {"f16": torch.float16, "bf16": torch.bfloat16}[args.dtype]
    has_a8 = hasattr(sa.DeviceVBS, "set_forward_a8")
    w, N = 32, 128
    arms, info, keep = {}, {}, []

    def build(tag, nz):
        m = sa.gen.fem3d(9, 9, nz, 3, 2)                       # nz = 257: gen.cant_like(seed=2), the headline matrix
        eng = sa.BlockingEngine(blocking_algo=5, tau=0.6, col_block_size=w, row_block_size=32, force_fixed_size=True, sim_measure=1)
        vb = sa.VBR().fill_from_CSR_inplace(m, eng.GetGrouping(m), w, 32, True)
        rng = np.random.default_rng(1)
        ldb = vb.cols + (vb.cols & 1)
        B = torch.from_numpy(rng.uniform(-1, 1, ldb * N).astype(np.float32)).cuda().to(tdt)
        C = torch.zeros(vb.rows * N, dtype=torch.float32, device="cuda")
        W0 = torch.from_numpy(np.ascontiguousarray(vb.mab, np.float32)).cuda()
        hs = {}
        for name in ("off", "a8") if has_a8 else ("off",):
            H = vb.to_device(0, dtype=sdt, updatable=True, transposable=tag == "")
            W = W0.clone()
            if name == "a8":
                H.set_forward_a8(True, values=W)
            else:
                H.set_values(W)
            hs[name] = (H, W)
            arms[tag + "spmm_" + name] = lambda H=H: H.spmm(B, C, N, ldb=ldb, ldc=vb.rows)
            if tag == "":
                G = torch.from_numpy(rng.uniform(-1e-3, 1e-3, int(vb.nztot)).astype(np.float32)).cuda()
                M, V = torch.zeros_like(W), torch.zeros_like(W)
                S = torch.zeros(8, dtype=torch.int32, device="cuda")
                arms["set_values_" + name] = lambda H=H, W=W: H.set_values(W)
                arms["adam_" + name] = lambda H=H, W=W, G=G, M=M, V=V, S=S: H.adam_step(W, G, M, V, S, lr=1e-4)
        H = hs["off"][0]
        info[tag + "handle"] = {"rows": int(vb.rows), "cols": int(vb.cols), "nztot": int(vb.nztot), "image16_bytes": int(H.info().get("a_bytes", 2 * int(vb.nztot)))}
        if has_a8:
            Ha = hs["a8"][0]
            Ha.spmm(B, C, N, ldb=ldb, ldc=vb.rows)
            torch.cuda.synchronize()
            info[tag + "a8_info"] = Ha.a8_info()
        keep.append((hs, B, C))

    build("", 257)
    if args.big:
        build("big_", 3084)

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
    rec = {"dtype": args.dtype, "commit": args.commit, "has_a8": has_a8, "N": N, "reps": args.reps,
           "ms_med_p10_p90": {k: [r5(np.median(t)), r5(np.percentile(t, 10)), r5(np.percentile(t, 90))] for k, t in times.items()}, "info": info}
    line = json.dumps(rec)
    print(line)
    if args.save:
        out = os.path.join(HERE, "profiles", "a8")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "a8_record.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
