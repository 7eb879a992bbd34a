"""sparta_vbs_sgd_step on the handle bench.py builds for its headline config (cant-like FEM, Jaccard -a 5 -t 0.6, w = 32, row_block 32,
force_fixed_size), made updatable: HIP events around each arm, median of the timed calls, the arms interleaved call by call in one process --
  (a) sgd_step, plain (lr only);
  (b) sgd_step with momentum 0.9;
      both as shipped (the default routing, step_info says which form that is) and with SPARTA_SGD_FUSE=1 / 0: the image kernel / the two-pass form asked for;
  (c) the same updates as in-place torch ops followed by set_values(W), the entry points the commit before this feature has:
      plain     W.add_(G, alpha=-lr); set_values(W)
      momentum  M.mul_(mu).add_(G); W.add_(M, alpha=-lr); set_values(W)
against a copy floor in the manner of DESIGN.md section 3.5: copy_ms * (bytes the step reads + writes) / (8 * nztot), copy_ms a device-to-device copy
of nztot floats in the same process (plain: W and G read, W and every image written; momentum: M read and written on top) -- and the forward product on
the handle stepped by the image kernel against the product on a fresh handle of the same values, interleaved, three repetitions (the spread of the fresh handle's figure is
the run-to-run noise).  One JSON line, appended to profiles/sgd_step/sgd_step_record.jsonl with --save.

    python scripts/sgd_step_record.py [--dtype f32|f16|bf16] [--reps 50] [--commit REV] [--save]"""
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
    sdt = {"f32": sa.F32, "f16": sa.F16, "bf16": sa.BF16}[args.dtype]
    tdt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[args.dtype]
    w, N = 32, 128
    m = sa.gen.cant_like(seed=2)
    eng = sa.BlockingEngine(blocking_algo=5, tau=0.6, col_block_size=w, row_block_size=32, force_fixed_size=True, sim_measure=1)
    vb = sa.VBR().fill_from_CSR_inplace(m, eng.GetGrouping(m), w, 32, True)
    nztot = int(vb.nztot)
    rng = np.random.default_rng(1)
    lr, mu = 1e-3, 0.9
    H = vb.to_device(0, dtype=sdt, updatable=True)
    B = torch.from_numpy(rng.uniform(-1, 1, vb.cols * N).astype(np.float32)).cuda().to(tdt)
    C = torch.zeros(vb.rows * N, dtype=torch.float32, device="cuda")
    W = torch.from_numpy(np.ascontiguousarray(vb.mab, np.float32)).cuda()
    G = torch.from_numpy((rng.uniform(-1, 1, nztot) * (vb.mab != 0)).astype(np.float32)).cuda()      # (the zero pattern of the values stays)
    M = torch.zeros_like(W)
    W2 = torch.empty_like(W)

    def torch_plain():
        W.add_(G, alpha=-lr)
        H.set_values(W)

    def torch_momentum():
        M.mul_(mu).add_(G)
        W.add_(M, alpha=-lr)
        H.set_values(W)

    def forced(fuse, f):
        """f under SPARTA_SGD_FUSE = fuse (the library reads it at every call): the image kernel for every step / for none, whatever the default routing is"""
        def run():
            os.environ["SPARTA_SGD_FUSE"] = fuse
            try:
                f()
            finally:
                del os.environ["SPARTA_SGD_FUSE"]
        return run

    def plain():
        H.sgd_step(W, G, None, lr=lr)

    def momentum():
        H.sgd_step(W, G, M, lr=lr, momentum=mu)

    arms = {"sgd_plain": plain, "sgd_momentum": momentum,                                     # as shipped: the default routing
            "sgd_plain_fused": forced("1", plain), "sgd_plain_two_pass": forced("0", plain),
            "sgd_momentum_fused": forced("1", momentum), "sgd_momentum_two_pass": forced("0", momentum),
            "torch_plain": torch_plain, "torch_momentum": torch_momentum,
            "copy": lambda: W2.copy_(W)}
    for _ in range(5):
        H.spmm(B, C, N)
        for f in arms.values():
            f()
    torch.cuda.synchronize()
    H.sgd_step(W, G, M, lr=lr, momentum=mu)
    step_info = {"momentum": H.step_info()}
    H.sgd_step(W, G, None, lr=lr)
    step_info["plain"] = H.step_info()
    info = H.info()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in arms}
    for _ in range(args.reps):
        for k, f in arms.items():
            e0.record(); f(); e1.record(); e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    med = {k: float(np.median(t)) for k, t in times.items()}
    # bytes: W and G read, W written, every image the handle holds written once (as scripts/set_values_record.py counts them)
    if sdt == sa.F32:
        frag_bytes = info["stream_steps"] * 1040 * 4
        legacy_held = info["a_bytes"] >= frag_bytes + 4 * nztot
        image_bytes = (4 * nztot if legacy_held else 0) + frag_bytes
    else:
        legacy_held = None
        image_bytes = info["a_bytes"] - 8 * 64 * 64 * 2
    bytes_plain = 12 * nztot + image_bytes
    bytes_momentum = 20 * nztot + image_bytes
    floor_plain = med["copy"] * bytes_plain / (8.0 * nztot)
    floor_momentum = med["copy"] * bytes_momentum / (8.0 * nztot)
    # the product after a step against the product of a fresh handle of the same values
    torch.cuda.synchronize()
    v2 = sa.VBR()
    v2.__dict__.update(vb.__dict__)
    v2.mab, v2._dev, v2._dev_t = W.cpu().numpy(), None, None
    F = v2.to_device(0, dtype=sdt)
    for _ in range(5):
        H.spmm(B, C, N); F.spmm(B, C, N)
    after, fresh = [], []
    Z, Z2 = torch.zeros_like(G), torch.zeros_like(G)
    for _ in range(3):
        os.environ["SPARTA_SGD_FUSE"] = "1"                              # (the image kernel writes the image the product then reads ...)
        H.sgd_step(W, Z, Z2, lr=lr, momentum=mu)                         # (... in a step that leaves the values of F: G = 0 and M = 0)
        del os.environ["SPARTA_SGD_FUSE"]
        assert H.step_info()["fused"] == 1 and not bool(Z2.any())
        a, f = [], []
        for _ in range(args.reps):
            a.append(H.spmm(B, C, N, timed=True)); f.append(F.spmm(B, C, N, timed=True))
        after.append(float(np.median(a))); fresh.append(float(np.median(f)))
    r5 = lambda x: round(x, 5)      # noqa: E731
    rec = {"dtype": args.dtype, "commit": args.commit, "rows": int(vb.rows), "cols": int(vb.cols), "nztot": nztot, "N": N, "reps": args.reps,
           "step_info": step_info, "a_bytes": int(info["a_bytes"]), "legacy_image_held": legacy_held, "image_bytes": int(image_bytes),
           "sgd_plain_ms": r5(med["sgd_plain"]), "sgd_momentum_ms": r5(med["sgd_momentum"]),
           "sgd_plain_fused_ms": r5(med["sgd_plain_fused"]), "sgd_plain_two_pass_ms": r5(med["sgd_plain_two_pass"]),
           "sgd_momentum_fused_ms": r5(med["sgd_momentum_fused"]), "sgd_momentum_two_pass_ms": r5(med["sgd_momentum_two_pass"]),
           "torch_plain_then_set_values_ms": r5(med["torch_plain"]), "torch_momentum_then_set_values_ms": r5(med["torch_momentum"]),
           "copy_ms": r5(med["copy"]), "floor_plain_ms": r5(floor_plain), "floor_momentum_ms": r5(floor_momentum),
           "sgd_plain_over_floor": round(med["sgd_plain"] / floor_plain, 3), "sgd_momentum_over_floor": round(med["sgd_momentum"] / floor_momentum, 3),
           "torch_over_sgd_plain": round(med["torch_plain"] / med["sgd_plain"], 3), "torch_over_sgd_momentum": round(med["torch_momentum"] / med["sgd_momentum"], 3),
           "spmm_after_ms": [r5(x) for x in after], "spmm_fresh_ms": [r5(x) for x in fresh], "spmm_fresh_spread_ms": r5(max(fresh) - min(fresh))}
    line = json.dumps(rec)
    print(line)
    if args.save:
        out = os.path.join(ROOT, "profiles", "sgd_step")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "sgd_step_record.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
