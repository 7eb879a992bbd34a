"""The epilogue of vbs_linear on the handle bench.py builds for its headline config (cant-like FEM, Jaccard -a 5 -t 0.6, w = 32, row_block 32,
force_fixed_size), made updatable and transposable, N = 128: HIP events around each arm, median of the timed calls with the 10th and 90th percentile, the
arms interleaved call by call in one process, in a new seeded order every round --
  kernels alone    epilogue_fwd (bias + gelu, z fp32 -> y in the 16-bit type) and epilogue_bwd (grad_y in the 16-bit type, dz in the handle's operand type,
                   with the bias gradient), against a device-to-device copy of the fp32 z in the same process (copy_ms) and the bytes each arm moves;
  the torch passes the same two steps as torch runs them: (z + bias -> gelu -> .to(16 bit)), and autograd's backward of exactly that plus the .to(x.dtype) of
                   today's vbs_linear backward;
  the whole layer  forward + backward of vbs_linear(x, H, W, bias=b, activation="gelu", out_dtype=16 bit), x, W and b requiring grad, against the same layer
                   written as today's vbs_linear + torch ops (+ bias, F.gelu, .to()).
The 16-bit type is the handle's for f16 / bf16 handles and float16 for the fp32 handle.  One JSON line, appended to profiles/epilogue/epilogue_record.jsonl
with --save.

    python scripts/epilogue_record.py [--dtype f32|f16|bf16] [--reps 50] [--commit REV] [--save]"""
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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--commit", default="", help="revision the numbers are taken on (recorded as given)")
    ap.add_argument("--save", action="store_true")
    args = ap.parse_args()
    import torch
    import sparta_amd as sa
    from sparta_amd.autograd import vbs_linear
    F = torch.nn.functional
    sdt = {"f32": sa.F32, "f16": sa.F16, "bf16": sa.BF16}[args.dtype]
    tdt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[args.dtype]
    odt = torch.float16 if args.dtype == "f32" else tdt
    w, N = 32, 128
    m = sa.gen.cant_like(seed=2)
    eng = sa.BlockingEngine(blocking_algo=5, tau=0.6, col_block_size=w, row_block_size=32, force_fixed_size=True, sim_measure=1)
    vb = sa.VBR().fill_from_CSR_inplace(m, eng.GetGrouping(m), w, 32, True)
    rng = np.random.default_rng(1)
    H = vb.to_device(0, dtype=sdt, updatable=True, transposable=True)
    rows, cols = int(vb.rows), int(vb.cols)
    x = torch.from_numpy(rng.uniform(-1, 1, (N, cols)).astype(np.float32)).cuda().to(tdt).requires_grad_(True)
    W = torch.from_numpy(np.ascontiguousarray(vb.mab, np.float32)).cuda().requires_grad_(True)
    b = torch.from_numpy(rng.uniform(-1, 1, rows).astype(np.float32)).cuda().requires_grad_(True)
    z = torch.empty((N, rows), dtype=torch.float32, device="cuda")
    H.set_values(W.detach())
    H.spmm(x.detach(), z, N)
    gy = torch.from_numpy(rng.uniform(-1, 1, (N, rows)).astype(np.float32)).cuda().to(odt)
    z2 = torch.empty_like(z)
    y_out, dz_out = torch.empty((N, rows), dtype=odt, device="cuda"), torch.empty((N, rows), dtype=tdt, device="cuda")
    bd = b.detach()

    def torch_fwd():
        return F.gelu(z + bd).to(odt)

    zl = z.clone().requires_grad_(True)
    bl = bd.clone().requires_grad_(True)
    yl = F.gelu(zl + bl).to(odt)

    def torch_bwd():
        zl.grad = bl.grad = None
        yl.backward(gy, retain_graph=True)
        return zl.grad.to(tdt)

    def layer(fused):
        x.grad = W.grad = b.grad = None
        if fused:
            y = vbs_linear(x, H, W, bias=b, activation="gelu", out_dtype=odt)
        else:
            y = F.gelu(vbs_linear(x, H, W) + b).to(odt)
        y.backward(gy)

    arms = {"epilogue_fwd": lambda: sa.epilogue_fwd(z, bd, "gelu", odt, out=y_out),
            "epilogue_bwd": lambda: sa.epilogue_bwd(gy, z, bd, "gelu", tdt, True, out=dz_out),
            "torch_fwd": torch_fwd, "torch_bwd": torch_bwd,
            "layer_fused": lambda: layer(True), "layer_torch": lambda: layer(False),
            "copy": lambda: z2.copy_(z)}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        for k in arms:
            arms[k]()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    order = np.random.default_rng(2)
    for _ in range(args.reps):
        for k in order.permutation(list(arms)):                          # (what the previous arm left in the Infinity Cache differs by arm: no fixed predecessor)
            k = str(k)
            e0.record(); arms[k](); e1.record(); e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    med = {k: float(np.median(t)) for k, t in times.items()}
    p10_90 = {k: [float(np.percentile(t, 10)), float(np.percentile(t, 90))] for k, t in times.items()}
    # the kernels alone, on the device's own clock (dt_ms of the entries)
    kf = [sa.epilogue_fwd(z, bd, "gelu", odt, out=y_out, timed=True)[1] for _ in range(args.reps)]
    kb = [sa.epilogue_bwd(gy, z, bd, "gelu", tdt, True, out=dz_out, timed=True)[2] for _ in range(args.reps)]
    el = rows * N
    osz, tsz = y_out.element_size(), dz_out.element_size()
    fwd_bytes, bwd_bytes = el * (4 + osz), el * (osz + 4 + tsz)
    r5 = lambda v: round(v, 5)      # noqa: E731
    rec = {"dtype": args.dtype, "out_dtype": str(odt).replace("torch.", ""), "commit": args.commit, "rows": rows, "cols": cols, "N": N, "reps": args.reps,
           "activation": "gelu", "bias": True,
           "ms": {k: r5(v) for k, v in med.items()}, "p10_p90_ms": {k: [r5(a) for a in v] for k, v in p10_90.items()},
           "kernel_fwd_ms": r5(float(np.median(kf))), "kernel_bwd_ms": r5(float(np.median(kb))),
           "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes, "copy_bytes": 8 * el,
           "fwd_floor_ms": r5(med["copy"] * fwd_bytes / (8.0 * el)), "bwd_floor_ms": r5(med["copy"] * bwd_bytes / (8.0 * el)),
           "torch_fwd_over_epilogue_fwd": round(med["torch_fwd"] / med["epilogue_fwd"], 3),
           "torch_bwd_over_epilogue_bwd": round(med["torch_bwd"] / med["epilogue_bwd"], 3),
           "layer_torch_over_layer_fused": round(med["layer_torch"] / med["layer_fused"], 3)}
    line = json.dumps(rec)
    print(line)
    if args.save:
        out = os.path.join(ROOT, "profiles", "epilogue")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "epilogue_record.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
