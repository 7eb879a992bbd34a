"""Repattern (sparta_amd.repattern, BlockPruner.compact, sparta_vbs_move_blocks) on the handle bench.py builds for its headline config (cant-like FEM, Jaccard
-a 5 -t 0.6, w = 32, row_block 32, force_fixed_size), made updatable and transposable, N = 128, at 50 / 75 / 90 % of the blocks pruned.  The method of
scripts/live_forward_record.py: HIP events around each arm on an idle stream (the host side of an arm is inside its window), all arms of a process
interleaved call by call in a new seeded order every round, median and 10th / 90th percentile of the timed calls.  Per level S three layers that took the
same Adam step and the same BlockPruner.prune(S) (the same masks):
  plain_S     the old handle, pruned blocks stored as zeros, no live set
  live_S      the old handle with its live forms on (skip_pruned, live_steps, and live_forward on a 16-bit handle)
  compact_S   the handle BlockPruner.compact made: only the live blocks are stored
(a) fwd / spmm_t / sddmm / adam on each of the three (adam: VbsAdamW.step on a gradient in the handle's layout)
(b) info()["a_bytes"] and the bytes of W, M and V before and after the compaction
(c) move_S: one move_blocks call of W, M and V (event window: records built and uploaded, kernel) with its kernel time (dt_ms) next to it, against copy_S,
    three torch copies of the same number of bytes
(d) repattern_S: the whole sparta_amd.repattern call, wall clock, against host_S: what a checkout without it must do -- download W, M and V, move them with
    numpy, create a handle from the moved values and upload M and V again (median of --reps-d runs, each followed by a synchronize)
One JSON line, appended to profiles/repattern/repattern_record.jsonl with --save.

    python scripts/repattern_record.py [--dtype f16|f32] [--reps 50] [--reps-d 5] [--commit REV] [--save]"""
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
    ap.add_argument("--dtype", choices=["f16", "f32"], default="f16")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--reps-d", type=int, default=5)
    ap.add_argument("--levels", default="50,75,90")
    ap.add_argument("--commit", default="", help="revision the numbers are taken on (recorded as given)")
    ap.add_argument("--save", action="store_true")
    args = ap.parse_args()
    import torch
    import sparta_amd as sa
    sdt = {"f16": sa.F16, "f32": sa.F32}[args.dtype]
    tdt = {"f16": torch.float16, "f32": torch.float32}[args.dtype]
    w, N = 32, 128
    m = sa.gen.cant_like(seed=2)
    eng = sa.BlockingEngine(blocking_algo=5, tau=0.6, col_block_size=w, row_block_size=32, force_fixed_size=True, sim_measure=1)
    vb = sa.VBR().fill_from_CSR_inplace(m, eng.GetGrouping(m), w, 32, True)
    rng = np.random.default_rng(1)
    ldb, ldx = vb.cols + (vb.cols & 1), vb.rows + (vb.rows & 1)
    B = torch.from_numpy(rng.uniform(-1, 1, ldb * N).astype(np.float32)).cuda().to(tdt)
    X = torch.from_numpy(rng.uniform(-1, 1, ldx * N).astype(np.float32)).cuda().to(tdt)
    C = torch.zeros(vb.rows * N, dtype=torch.float32, device="cuda")
    Ct = torch.zeros(vb.cols * N, dtype=torch.float32, device="cuda")
    W0 = torch.from_numpy(np.ascontiguousarray(vb.mab, np.float32)).cuda()
    G0 = torch.from_numpy(rng.uniform(-1, 1, vb.nztot).astype(np.float32)).cuda()

    def layer(s, kind):
        """(optimizer, pruner) of a layer that took one Adam step and prune(s)"""
        H = vb.to_device(0, dtype=sdt, updatable=True, transposable=True)
        W = W0.clone().requires_grad_(True)
        opt = sa.VbsAdamW([(H, W)], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
        W.grad = G0.clone()
        opt.step()
        opt.zero_grad()
        live = kind == "live"
        p = sa.BlockPruner(opt, skip_pruned=kind != "plain", live_steps=live, live_forward=live and sdt != sa.F32)
        p.prune(s)
        return opt, p

    arms, sizes, kernel_ms, wall, keepalive = {}, {}, {}, {}, []

    def product_arms(tag, opt, keep=None):
        H, W = opt.pairs[0]
        G = torch.zeros(W.numel(), dtype=torch.float32, device="cuda")
        g = G0[:W.numel()].clone()
        if keep is not None:                   # the gradient of the pruned blocks is zero, as BlockPruner.mask_grads leaves it: they stay zero under the step
            H.mask_blocks(keep, g)

        def adam():
            W.grad = g
            opt.step()
        arms["fwd_" + tag] = lambda: H.spmm(B, C, N, ldb=ldb, ldc=vb.rows)
        arms["spmm_t_" + tag] = lambda: H.spmm_t(X, Ct, N, ldx=ldx)
        arms["sddmm_" + tag] = lambda: H.sddmm(X, B, G, N, ldx=ldx, ldy=ldb)
        arms["adam_" + tag] = adam

    def host_path(opt, keep):
        """what a checkout without repattern does: download, move with numpy, create, upload"""
        H, W = opt.pairs[0]
        st = opt._state[0]
        host = [t.detach().cpu().numpy() for t in (W, st["exp_avg"], st["exp_avg_sq"])]
        T = vb.block_table()
        first = np.concatenate([[0], np.cumsum(vb.nzcount)])
        rows_of = np.repeat(np.arange(vb.block_rows), vb.nzcount)
        sel = np.flatnonzero(keep)
        nz = np.bincount(rows_of[sel], minlength=vb.block_rows).astype(np.int64)
        idx = (T[sel, 0][:, None] + np.arange(int(T[0, 2]))[None, :]).reshape(-1) if len(sel) and (T[:, 2] == T[0, 2]).all() else \
            np.concatenate([np.arange(o, o + n) for o, n in zip(T[sel, 0], T[sel, 2])] or [np.zeros(0, np.int64)])
        moved = [h[idx] for h in host]
        nv = sa.VBR.from_arrays(vb.rows, vb.cols, vb.block_col_size, vb.row_part, nz, vb.jab[sel], moved[0])
        assert first[-1] == len(keep)
        H2 = nv.to_device(0, dtype=sdt, updatable=True, transposable=True)
        dev = [torch.from_numpy(x).cuda() for x in moved]
        torch.cuda.synchronize()
        H2.close()
        return dev

    for s in [int(x) for x in args.levels.split(",")]:
        tag = "%d" % s
        for kind in ("plain", "live"):
            opt, p = layer(s / 100.0, kind)
            product_arms("%s_%s" % (kind, tag), opt, p.keep_masks()[0])
            keepalive.append((opt, p))
        # the layer that is compacted; before that, arms (c) and (d) on it
        opt, p = layer(s / 100.0, "compact")
        H, W = opt.pairs[0]
        st = opt._state[0]
        keep = p.keep_masks()[0].cpu().numpy()
        olds = [W.detach(), st["exp_avg"], st["exp_avg_sq"]]
        for name, fn in (("repattern", lambda: [h.close() for h in [sa.repattern(vb, H, olds, keep=keep)[1]]]), ("host", lambda: host_path(opt, keep))):
            ts = []
            for _ in range(args.reps_d):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(1e3 * (time.perf_counter() - t0))
            wall["%s_%s" % (name, tag)] = ts
        before = {"a_bytes": H.info()["a_bytes"], "nztot": H.info()["nztot"], "blocks": H.n_blocks, "wmv_bytes": 12 * W.numel()}
        (nv,) = p.compact([vb])
        H2, W2 = opt.pairs[0]
        st2 = opt._state[0]
        after = {"a_bytes": H2.info()["a_bytes"], "nztot": H2.info()["nztot"], "blocks": H2.n_blocks, "wmv_bytes": 12 * W2.numel(),
                 "stream_steps": H2.info()["stream_steps"], "stream_workers": H2.info()["stream_workers"]}
        before.update(stream_steps=H.info()["stream_steps"], stream_workers=H.info()["stream_workers"])
        sizes[tag] = {"before": before, "after": after}
        product_arms("compact_" + tag, opt)
        bmap = opt.last_map
        news = [torch.empty_like(W2.detach()) for _ in range(3)]
        kernel_ms["move_" + tag] = []

        def move(H=H, H2=H2, bmap=bmap, olds=olds, news=news, out=kernel_ms["move_" + tag]):
            out.append(H2.move_blocks(H, bmap, *zip(olds, news), timed=True))

        def copy(olds=olds, news=news):
            for a, b in zip(olds, news):
                b.copy_(a[:b.numel()])
        arms["move_" + tag], arms["copy_" + tag] = move, copy
        keepalive.append((opt, p, H, olds, st2))

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
    for v in kernel_ms.values():
        del v[:]
    times = {k: [] for k in arms}
    order = np.random.default_rng(2)
    for _ in range(args.reps):
        for k in order.permutation(list(arms)):
            call(str(k), times[str(k)])
    torch.cuda.synchronize()
    r5 = lambda x: round(float(x), 5)      # noqa: E731
    mp = lambda t: [r5(np.median(t)), r5(np.percentile(t, 10)), r5(np.percentile(t, 90))]      # noqa: E731
    rec = {"dtype": args.dtype, "commit": args.commit, "rows": int(vb.rows), "cols": int(vb.cols), "nztot": int(vb.nztot), "N": N, "reps": args.reps,
           "reps_d": args.reps_d, "ms_med_p10_p90": {k: mp(t) for k, t in times.items()}, "kernel_ms_med_p10_p90": {k: mp(t) for k, t in kernel_ms.items()},
           "wall_ms_med_min_max": {k: [r5(np.median(t)), r5(min(t)), r5(max(t))] for k, t in wall.items()}, "sizes": sizes}
    line = json.dumps(rec)
    print(line)
    if args.save:
        out = os.path.join(HERE, "profiles", "repattern")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "repattern_record.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
