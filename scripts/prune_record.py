"""Block pruning (sparta_vbs_block_ssq, sparta_vbs_mask_blocks, sparta_amd.BlockPruner) on the handle bench.py builds for its headline config (cant-like
FEM, Jaccard -a 5 -t 0.6, w = 32, row_block 32, force_fixed_size), made updatable: the method of scripts/grad_ctl_record.py -- HIP events around each arm
on an idle stream (the host side of an arm is inside its window), the arms interleaved call by call in one process in a new seeded order every round, median
and 10th / 90th percentile of the timed calls --
  (a) block_ssq             sparta_vbs_block_ssq over the nztot floats of W (one launch, one wave per block)
      grad_stats            sparta_grad_stats over the same tensor: the same bytes read once by a kernel of the parent commit (two launches)
  (b) mask_wmv              sparta_vbs_mask_blocks of W + M + V with every second block pruned (one launch)
      memset_1 / memset_3   hipMemsetAsync of the same number of bytes: one call on one buffer / three calls, one per tensor's share
  (c) mask_grads            BlockPruner.mask_grads() at 50 % pruned
      ctl_step              stats + finish + adam_step_ctl, the clipped AdamW step of profiles/grad_ctl/
      masked_ctl_step       mask_grads + ctl_step
  (d) spmm_pruned / spmm_fresh   the forward product (N = 128) at 0 / 50 / 75 / 90 % of the blocks pruned by BlockPruner.prune, next to a fresh handle created
                            from the same pruned values, interleaved
One JSON line, appended to profiles/prune/prune_record.jsonl with --save.

    python scripts/prune_record.py [--dtype f32|f16|bf16] [--reps 50] [--commit REV] [--save]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def hip_runtime():
    """the HIP runtime this process already uses (the one torch loaded)"""
    with open("/proc/self/maps") as f:
        paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
    if not paths:
        raise RuntimeError("no libamdhip64 in this process")
    lib = C.CDLL(paths[0])
    lib.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    return lib


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
    table = vb.block_table()
    n_blocks = len(table)
    rng = np.random.default_rng(1)
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    H = vb.to_device(0, dtype=sdt, updatable=True)
    assert H.n_blocks == n_blocks
    B = torch.from_numpy(rng.uniform(-1, 1, vb.cols * N).astype(np.float32)).cuda().to(tdt)
    Cd = torch.zeros(vb.rows * N, dtype=torch.float32, device="cuda")
    W = torch.from_numpy(np.ascontiguousarray(vb.mab, np.float32)).cuda().requires_grad_(True)
    G = torch.from_numpy((rng.uniform(-1, 1, nztot) * (vb.mab != 0)).astype(np.float32)).cuda()
    W.grad = G
    M, V = torch.zeros_like(G), torch.zeros_like(G)
    S = torch.zeros(8, dtype=torch.int32, device="cuda")
    ctl = sa.GradCtl(loss_scale=1.0, max_norm=1e9, growth_interval=2000)
    stats_ctl = sa.GradCtl()
    ssq_out = torch.empty(n_blocks, dtype=torch.float64, device="cuda")
    # (b): three scratch tensors of their own (W stays as it is for (d)), every second block pruned
    T3 = [torch.ones_like(G) for _ in range(3)]
    half = torch.from_numpy((np.arange(n_blocks) % 2).astype(np.uint8)).cuda()
    pruned_bytes = 4 * int(table[0::2, 2].sum())
    hip = hip_runtime()
    target = torch.empty(3 * pruned_bytes, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    # (c): a pruner of its own on a copy of W, at 50 %
    Wc = W.detach().clone().requires_grad_(True)
    Wc.grad = G.clone()
    pc = sa.BlockPruner([(H, Wc)])
    pc.prune(0.5)
    H.set_values(W.detach())

    def ctl_step():
        ctl.add(G, first=True)
        ctl.finish()
        H.adam_step(W, G, M, V, S, ctl=ctl, **hyper)

    def memset_3():
        for i in range(3):
            hip.hipMemsetAsync(C.c_void_p(target.data_ptr() + i * pruned_bytes), 0, pruned_bytes, C.c_void_p(stream))

    arms = {"block_ssq": lambda: H.block_ssq(W.detach(), out=ssq_out),
            "grad_stats": lambda: stats_ctl.add(W.detach(), first=True),
            "mask_wmv": lambda: H.mask_blocks(half, *T3),
            "memset_1": lambda: hip.hipMemsetAsync(C.c_void_p(target.data_ptr()), 0, 3 * pruned_bytes, C.c_void_p(stream)),
            "memset_3": memset_3,
            "mask_grads": pc.mask_grads,
            "ctl_step": ctl_step,
            "masked_ctl_step": lambda: (pc.mask_grads(), ctl_step())}

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def call(k, timed=None):
        if timed is None:
            arms[k]()
        else:
            e0.record(); arms[k](); e1.record(); e1.synchronize()
            timed.append(e0.elapsed_time(e1))

    W_before = W.detach().clone()
    for _ in range(5):
        H.spmm(B, Cd, N)
        for k in arms:
            call(k)
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    order = np.random.default_rng(2)
    for _ in range(args.reps):
        for k in order.permutation(list(arms)):
            call(str(k), times[str(k)])
    torch.cuda.synchronize()
    assert ctl.read()["skip"] == 0
    # the score against the statistics of the same tensor: the blocks tile W, so the scores add up to its sum of squares (positions past cols: none at w | cols)
    stats_ctl.add(W.detach(), first=True)
    H.block_ssq(W.detach(), out=ssq_out)
    total, whole = float(ssq_out.sum()), stats_ctl.read()["ssq"]
    med = {k: float(np.median(t)) for k, t in times.items()}
    p10_90 = {k: [float(np.percentile(t, 10)), float(np.percentile(t, 90))] for k, t in times.items()}

    # (d) the forward product as blocks go: the values the steps above left, pruned further and further
    W.data.copy_(W_before)
    M.zero_(); V.zero_(); S.zero_()
    pd = sa.BlockPruner([(H, W)])
    H.set_values(W.detach())
    spmm = {}
    for s in (0.0, 0.5, 0.75, 0.9):
        pd.prune(s)
        torch.cuda.synchronize()
        v2 = sa.VBR()
        v2.__dict__.update(vb.__dict__)
        v2.mab, v2._dev, v2._dev_t = W.detach().cpu().numpy(), None, None
        F = v2.to_device(0, dtype=sdt)
        for _ in range(5):
            H.spmm(B, Cd, N); F.spmm(B, Cd, N)
        a, f = [], []
        for _ in range(args.reps):
            a.append(H.spmm(B, Cd, N, timed=True)); f.append(F.spmm(B, Cd, N, timed=True))
        pct = lambda t: [round(float(np.median(t)), 5), round(float(np.percentile(t, 10)), 5), round(float(np.percentile(t, 90)), 5)]      # noqa: E731
        spmm["%g" % s] = {"sparsity": pd.sparsity(), "zero_values": float((W.detach() == 0).float().mean()), "pruned_ms_med_p10_p90": pct(a),
                          "fresh_ms_med_p10_p90": pct(f), "fresh_packed": F.packed_info() if sdt == sa.F32 else None}
        F.close()
    r5 = lambda x: round(x, 5)      # noqa: E731
    gbs = lambda nbytes, ms: round(nbytes / (ms * 1e-3) / 1e9, 1)      # noqa: E731
    rec = {"dtype": args.dtype, "commit": args.commit, "rows": int(vb.rows), "cols": int(vb.cols), "nztot": nztot, "n_blocks": n_blocks, "N": N,
           "reps": args.reps, "ms": {k: r5(v) for k, v in med.items()}, "p10_p90_ms": {k: [r5(x) for x in v] for k, v in p10_90.items()},
           "block_ssq_read_gbs": gbs(4 * nztot, med["block_ssq"]), "grad_stats_read_gbs": gbs(4 * nztot, med["grad_stats"]),
           "ssq_sum_over_grad_stats_minus_1": (total - whole) / whole,
           "mask_pruned_bytes": 3 * pruned_bytes, "mask_wmv_write_gbs": gbs(3 * pruned_bytes, med["mask_wmv"]), "memset_1_write_gbs": gbs(3 * pruned_bytes, med["memset_1"]),
           "mask_grads_share_of_masked_ctl_step": round(med["mask_grads"] / med["masked_ctl_step"], 4),
           "masked_ctl_step_minus_ctl_step_ms": r5(med["masked_ctl_step"] - med["ctl_step"]), "spmm": spmm}
    line = json.dumps(rec)
    print(line)
    if args.save:
        out = os.path.join(ROOT, "profiles", "prune")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "prune_record.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
