"""Device-side gradient clipping and loss scaling (sparta_grad_stats, sparta_grad_ctl_finish, sparta_vbs_adam_step_ctl) on the handle bench.py builds for its
headline config (cant-like FEM, Jaccard -a 5 -t 0.6, w = 32, row_block 32, force_fixed_size), made updatable: the method of scripts/adam_step_record.py --
HIP events around each arm on an idle stream (the host side of an arm is inside its window), the arms interleaved call by call in one process in a new
seeded order every round, median and 10th / 90th percentile of the timed calls --
  (a) stats                 sparta_grad_stats over the nztot floats of G (two launches: the streaming pass and the fold)
      torch_norm            torch.linalg.vector_norm(G)
      torch_norm_isfinite   vector_norm(G) and torch.isfinite(G).all(): the two passes of torch's clip-plus-scaler path
      copy                  a device-to-device copy of nztot floats (reads and writes 4 bytes per element each): the streaming rate on this size
  (b) adam / adam_ctl       adam_step as shipped, without and with a control record (coef = 1, skip = 0)
  (c) ctl_step              stats + finish + adam_step_ctl
      torch_step            torch._amp_foreach_non_finite_check_and_unscale_ + clip_grad_norm_ + AdamW(fused=True).step() + set_values
  (d) spmm_after / spmm_fresh   the forward product on the handle after a step under control and on a fresh handle of the same values, three repetitions
One JSON line, appended to profiles/grad_ctl/grad_ctl_record.jsonl with --save.

    python scripts/grad_ctl_record.py [--dtype f32|f16|bf16] [--reps 50] [--commit REV] [--save]"""
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
    # max_norm far above the norm: both clipping arms do all their work and leave G as it is, call after call
    ctl = sa.GradCtl(loss_scale=1.0, max_norm=1e9, growth_interval=2000)
    ctl.collect(G)
    assert ctl.read()["skip"] == 0 and ctl.read()["coef"] == 1.0
    topt = torch.optim.AdamW([W], **hyper, fused=True)
    found_inf, inv_scale = torch.zeros(1, device="cuda"), torch.ones(1, device="cuda")

    def ctl_step():
        ctl.add(G, first=True)
        ctl.finish()
        H.adam_step(W, G, M, V, S, ctl=ctl, **hyper)

    def torch_step():
        torch._amp_foreach_non_finite_check_and_unscale_([G], found_inf, inv_scale)
        torch.nn.utils.clip_grad_norm_([W], 1e9)
        topt.step()
        H.set_values(W.detach())

    arms = {"stats": lambda: ctl.add(G, first=True),
            "torch_norm": lambda: torch.linalg.vector_norm(G),
            "torch_norm_isfinite": lambda: (torch.linalg.vector_norm(G), torch.isfinite(G).all()),
            "copy": lambda: W2.copy_(G),
            "adam": lambda: H.adam_step(W, G, M, V, S, **hyper),
            "adam_ctl": lambda: H.adam_step(W, G, M, V, S, ctl=ctl, **hyper),
            "ctl_step": ctl_step, "torch_step": torch_step}

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def call(k, timed=None):
        if timed is None:
            arms[k]()
        else:
            e0.record(); arms[k](); e1.record(); e1.synchronize()
            timed.append(e0.elapsed_time(e1))

    for _ in range(5):
        H.spmm(B, C, N)
        for k in arms:
            call(k)
    torch.cuda.synchronize()
    step_info = H.step_info()
    times = {k: [] for k in arms}
    order = np.random.default_rng(2)
    for _ in range(args.reps):
        for k in order.permutation(list(arms)):
            call(str(k), times[str(k)])
    rec_ctl = ctl.read()
    assert rec_ctl["skip"] == 0 and rec_ctl["skipped_total"] == 0 and float(found_inf) == 0.0
    med = {k: float(np.median(t)) for k, t in times.items()}
    p10_90 = {k: [float(np.percentile(t, 10)), float(np.percentile(t, 90))] for k, t in times.items()}
    # (d) the product after a step under control against the product of a fresh handle of the same values
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
        ctl.collect(Z)
        H.adam_step(W, Z, Zm, Zv, Zs, lr=hyper["lr"], ctl=ctl)           # a step that leaves the values of F: G = 0, M = 0, V = 0, no decay
        assert H.step_info() == step_info and not bool(Zm.any())
        a, f = [], []
        for _ in range(args.reps):
            a.append(H.spmm(B, C, N, timed=True)); f.append(F.spmm(B, C, N, timed=True))
        after.append(float(np.median(a))); fresh.append(float(np.median(f)))
    assert np.array_equal(W.detach().cpu().numpy(), v2.mab)
    r5 = lambda x: round(x, 5)      # noqa: E731
    gbs = lambda nbytes, ms: round(nbytes / (ms * 1e-3) / 1e9, 1)      # noqa: E731
    rec = {"dtype": args.dtype, "commit": args.commit, "rows": int(vb.rows), "cols": int(vb.cols), "nztot": nztot, "N": N, "reps": args.reps,
           "step_info": step_info, "ms": {k: r5(v) for k, v in med.items()}, "p10_p90_ms": {k: [r5(x) for x in v] for k, v in p10_90.items()},
           "stats_read_gbs": gbs(4 * nztot, med["stats"]), "torch_norm_read_gbs": gbs(4 * nztot, med["torch_norm"]),
           "copy_read_plus_write_gbs": gbs(8 * nztot, med["copy"]),
           "adam_ctl_minus_adam_ms": r5(med["adam_ctl"] - med["adam"]), "torch_step_over_ctl_step": round(med["torch_step"] / med["ctl_step"], 3),
           "spmm_after_ms": [r5(x) for x in after], "spmm_fresh_ms": [r5(x) for x in fresh], "spmm_fresh_spread_ms": r5(max(fresh) - min(fresh))}
    line = json.dumps(rec)
    print(line)
    if args.save:
        out = os.path.join(ROOT, "profiles", "grad_ctl")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "grad_ctl_record.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
