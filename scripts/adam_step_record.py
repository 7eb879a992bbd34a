"""sparta_vbs_adam_step on the handle bench.py builds for its headline config (cant-like FEM, Jaccard -a 5 -t 0.6, w = 32, row_block 32,
force_fixed_size), made updatable: HIP events around each arm, median of the timed calls, the arms interleaved call by call in one process, in a
new seeded order every round --
  (a)  adam_step as shipped (AdamW, lr 1e-3, weight decay 0.01; step_info says which form the default routing took);
  (a1) the same with SPARTA_ADAM_FUSE=1, (a0) with SPARTA_ADAM_FUSE=0: the image kernel / the two-pass form asked for (the variable is set outside the
       timed window: the events start on an idle stream, so whatever the host does between them counts -- for every arm, the Python of torch's optimizers too);
  (c1) torch.optim.AdamW(fused=True).step() followed by set_values(W), (c2) the same with foreach=True: what a user runs without the entry
against a copy floor in the manner of DESIGN.md section 3.5: copy_ms * bytes / (8 * nztot), copy_ms a device-to-device copy of nztot floats in the same
process, bytes = seven floats per element (W, G, M, V read; W, M, V written) plus every image the step writes -- and the forward product on the handle after a
step against the product on a fresh handle of the same values, interleaved, three repetitions (the spread of the fresh handle's figure is the run-to-run
noise).  Every arm also records the 10th and 90th percentile of its calls: the spread the comparison of (a) with (c1), (c2) is read against.  One JSON line,
appended to profiles/adam_step/adam_step_record.jsonl with --save.

    python scripts/adam_step_record.py [--dtype f32|f16|bf16] [--reps 50] [--commit REV] [--save]"""
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
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    H = vb.to_device(0, dtype=sdt, updatable=True)
    B = torch.from_numpy(rng.uniform(-1, 1, vb.cols * N).astype(np.float32)).cuda().to(tdt)
    C = torch.zeros(vb.rows * N, dtype=torch.float32, device="cuda")
    W = torch.from_numpy(np.ascontiguousarray(vb.mab, np.float32)).cuda().requires_grad_(True)
    G = torch.from_numpy((rng.uniform(-1, 1, nztot) * (vb.mab != 0)).astype(np.float32)).cuda()
    W.grad = G
    M, V = torch.zeros_like(G), torch.zeros_like(G)
    S = torch.zeros(8, dtype=torch.int32, device="cuda")
    W2 = torch.empty_like(G)

    def adam():
        H.adam_step(W, G, M, V, S, **hyper)

    def torch_arm(**kw):
        opt = torch.optim.AdamW([W], **hyper, **kw)

        def run():
            opt.step()
            H.set_values(W.detach())
        return run

    env = {"adam_fused": "1", "adam_two_pass": "0"}                      # SPARTA_ADAM_FUSE of the forced arms, set outside the timed window (read at every call)
    arms = {"adam": adam, "adam_fused": adam, "adam_two_pass": adam,
            "torch_fused": torch_arm(fused=True), "torch_foreach": torch_arm(foreach=True),
            "copy": lambda: W2.copy_(W.detach())}

    def call(k, timed=None):
        if k in env:
            os.environ["SPARTA_ADAM_FUSE"] = env[k]
        try:
            if timed is None:
                arms[k]()
            else:
                e0.record(); arms[k](); e1.record(); e1.synchronize()
                timed.append(e0.elapsed_time(e1))
        finally:
            os.environ.pop("SPARTA_ADAM_FUSE", None)

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    forms = {}
    for _ in range(5):
        H.spmm(B, C, N)
        for k in arms:
            call(k)
            forms[k] = H.step_info()
    assert forms["adam_fused"]["fused"] == 1 and forms["adam_two_pass"]["fused"] == 0, forms
    torch.cuda.synchronize()
    adam()
    step_info = H.step_info()
    info = H.info()
    times = {k: [] for k in arms}
    order = np.random.default_rng(2)
    for _ in range(args.reps):
        for k in order.permutation(list(arms)):                          # (what the previous arm left in the 256 MB Infinity Cache differs by arm: no fixed predecessor)
            call(str(k), times[str(k)])
    med = {k: float(np.median(t)) for k, t in times.items()}
    p10_90 = {k: [float(np.percentile(t, 10)), float(np.percentile(t, 90))] for k, t in times.items()}
    # bytes: W, G, M, V read, W, M, V written, every image the handle holds written once (as scripts/sgd_step_record.py counts them)
    if sdt == sa.F32:
        frag_bytes = info["stream_steps"] * 1040 * 4
        legacy_held = info["a_bytes"] >= frag_bytes + 4 * nztot
        image_bytes = (4 * nztot if legacy_held else 0) + frag_bytes
    else:
        legacy_held = None
        image_bytes = info["a_bytes"] - 8 * 64 * 64 * 2
    step_bytes = 28 * nztot + image_bytes
    floor = med["copy"] * step_bytes / (8.0 * nztot)
    # the product after a step against the product of a fresh handle of the same values
    torch.cuda.synchronize()
    v2 = sa.VBR()
    v2.__dict__.update(vb.__dict__)
    v2.mab, v2._dev, v2._dev_t = W.detach().cpu().numpy(), None, None
    F = v2.to_device(0, dtype=sdt)
    for _ in range(5):
        H.spmm(B, C, N); F.spmm(B, C, N)
    after, fresh = [], []
    Z, Zm, Zv = torch.zeros_like(G), torch.zeros_like(G), torch.zeros_like(G)
    for _ in range(3):
        Zs = torch.zeros(8, dtype=torch.int32, device="cuda")
        H.adam_step(W, Z, Zm, Zv, Zs, lr=hyper["lr"])                    # as shipped, in a step that leaves the values of F: G = 0, M = 0, V = 0, no decay
        assert H.step_info() == step_info and not bool(Zm.any())
        a, f = [], []
        for _ in range(args.reps):
            a.append(H.spmm(B, C, N, timed=True)); f.append(F.spmm(B, C, N, timed=True))
        after.append(float(np.median(a))); fresh.append(float(np.median(f)))
    assert np.array_equal(W.detach().cpu().numpy(), v2.mab)
    r5 = lambda x: round(x, 5)      # noqa: E731
    best_torch = min(med["torch_fused"], med["torch_foreach"])
    rec = {"dtype": args.dtype, "commit": args.commit, "rows": int(vb.rows), "cols": int(vb.cols), "nztot": nztot, "N": N, "reps": args.reps,
           "step_info": step_info, "a_bytes": int(info["a_bytes"]), "legacy_image_held": legacy_held, "image_bytes": int(image_bytes),
           "adam_ms": r5(med["adam"]), "adam_fused_ms": r5(med["adam_fused"]), "adam_two_pass_ms": r5(med["adam_two_pass"]),
           "torch_fused_then_set_values_ms": r5(med["torch_fused"]), "torch_foreach_then_set_values_ms": r5(med["torch_foreach"]),
           "p10_p90_ms": {k: [r5(x) for x in v] for k, v in p10_90.items()},
           "copy_ms": r5(med["copy"]), "step_bytes": int(step_bytes), "floor_ms": r5(floor), "adam_over_floor": round(med["adam"] / floor, 3),
           "best_torch_over_adam": round(best_torch / med["adam"], 3),
           "spmm_after_ms": [r5(x) for x in after], "spmm_fresh_ms": [r5(x) for x in fresh], "spmm_fresh_spread_ms": r5(max(fresh) - min(fresh))}
    line = json.dumps(rec)
    print(line)
    if args.save:
        out = os.path.join(ROOT, "profiles", "adam_step")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "adam_step_record.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
