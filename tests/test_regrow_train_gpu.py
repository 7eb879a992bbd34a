"""BlockPruner.regrow through a short training run on the GPU: one vbs_linear layer with VbsAdamW, BlockPruner(skip_pruned=True, live_steps=True) -- and
live_forward=True on the 16-bit handle --, prune(0.5), then four steps with regrow(0.3) after the second and the fourth.

The reference is a second run that makes the same swaps by hand: it downloads the pruner's scores and the probe's gradient scores, runs select_swap on the
CPU and applies the masks with mask_blocks, set_values and set_live_blocks.  The two runs must end with the same bits in the weights, both moments and the step
state.

"w48" (fp32) goes through vbs_linear(probe=...).  "heights32" has 391 rows, which vbs_linear refuses on a 16-bit handle (its operands need an even leading
dimension), so that layer is driven through the calls vbs_linear makes -- spmm, sddmm and sddmm_block_ssq on the same operands -- with grad_y in a buffer of
leading dimension 392."""
import math

import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd.autograd import vbs_linear

torch = pytest.importorskip("torch")

import _util as U  # noqa: E402
import _live as L  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
TDT = {sa.F32: torch.float32, sa.F16: torch.float16}
N = 8
STEPS = 4
REGROW_AFTER = (1, 3)          # (0-based) after the second and the fourth step


def bits(t):
    return np.ascontiguousarray(t.detach().float().cpu().numpy(), f32).view(np.uint32)


def block_any(T, a):
    """per block: does any of its n_all elements of `a` have a bit set"""
    return np.array([bool(a[int(o):int(o) + int(n)].any()) for o, n in zip(T[:, 0], T[:, 2])])


def train(key, dtype, by_hand):
    v = L.geometry(key)
    T = L.table(key, None)
    rng = np.random.default_rng(9500)
    W0 = rng.uniform(-1, 1, int(v.nztot)).astype(f32)
    xs = [torch.from_numpy(U.edge_round(rng.uniform(-1, 1, (N, v.cols)), dtype)).to(TDT[dtype]).cuda() for _ in range(STEPS)]
    gys = [torch.from_numpy(rng.uniform(-1, 1, (N, v.rows)).astype(f32)).cuda() for _ in range(STEPS)]
    H = v.to_device(0, dtype=dtype, updatable=True, transposable=True)
    try:
        W = torch.from_numpy(W0.copy()).cuda().requires_grad_(True)
        opt = sa.VbsAdamW([(H, W)], lr=1e-2, weight_decay=0.01)
        pruner = sa.BlockPruner(opt, skip_pruned=True, live_steps=True, live_forward=dtype != sa.F32)
        pruner.prune(0.5)
        keep = pruner.keep_masks()[0]                                 # (updated in place by regrow; by hand: written below)
        probe = pruner.probe(0)
        n_in = torch.from_numpy(T[:, 1].astype(np.float64))
        log = {"keep": [keep.cpu().numpy().copy()], "after_regrow": [], "W_after_step": []}
        assert np.array_equal(probe.sel.cpu().numpy(), 1 - log["keep"][0])
        for step in range(STEPS):
            opt.zero_grad()
            if dtype == sa.F32:
                y = vbs_linear(xs[step], H, W, probe=probe)
                y.backward(gys[step])
            else:
                y = torch.empty((N, v.rows), dtype=torch.float32, device="cuda")
                H.spmm(xs[step], y, N, accumulate=False)              # (the handle holds W: prune, regrow and the step write it)
                ldx = v.rows + (v.rows & 1)
                dz = torch.zeros((N, ldx), dtype=TDT[dtype], device="cuda")
                dz[:, :v.rows] = gys[step].to(TDT[dtype])
                W.grad = torch.empty(int(v.nztot), dtype=torch.float32, device="cuda")
                H.sddmm(dz.reshape(-1), xs[step], W.grad, N, accumulate=False, ldx=ldx)
                H.sddmm_block_ssq(dz.reshape(-1), xs[step], N, sel=probe.sel, out=probe.out, ldx=ldx)
            opt.step()
            log["W_after_step"].append(bits(W))
            if step not in REGROW_AFTER:
                continue
            st = opt._state[0]
            if not by_hand:
                pruner.regrow(0.3)
            else:
                k_cpu = keep.cpu()
                mag = pruner.scores()[0].cpu()
                g = probe.out.cpu() / n_in
                g = torch.where(n_in > 0, g, torch.full_like(g, float("-inf")))
                new = sa.select_swap([mag], [g], [k_cpu], int(math.floor(0.3 * int(k_cpu.sum()))))[0]
                keep.copy_(new.cuda())
                H.mask_blocks(keep, W.detach(), W.grad, st["exp_avg"], st["exp_avg_sq"])
                H.set_values(W.detach())
                H.set_live_blocks(keep)
                probe.sel.copy_(keep == 0)
            torch.cuda.synchronize()
            log["keep"].append(keep.cpu().numpy().copy())
            log["after_regrow"].append([bits(W), bits(st["exp_avg"]), bits(st["exp_avg_sq"])])
            assert np.array_equal(probe.sel.cpu().numpy(), 1 - log["keep"][-1])
        st = opt._state[0]
        log["final"] = [bits(W), bits(st["exp_avg"]), bits(st["exp_avg_sq"]), st["state"].cpu().numpy().copy()]
        # the forward product of the trained handle against a fresh handle created from the final values
        out = torch.empty((N, v.rows), dtype=torch.float32, device="cuda")
        H.spmm(xs[0], out, N, accumulate=False)
        fresh = sa.VBR.from_arrays(v.rows, v.cols, int(v.block_col_size), v.row_part, v.nzcount, v.jab, W.detach().cpu().numpy()).to_device(0, dtype=dtype)
        try:
            ref = torch.empty_like(out)
            fresh.spmm(xs[0], ref, N, accumulate=False)
            torch.cuda.synchronize()
            log["forward"] = (out.cpu().numpy(), ref.cpu().numpy())
        finally:
            fresh.close()
        return log
    finally:
        H.close()


@pytest.mark.parametrize("key,dtype", [("w48", sa.F32), ("heights32", sa.F16)], ids=["w48-f32", "heights32-f16"])
def test_regrow_matches_the_swaps_made_by_hand(key, dtype):
    T = L.table(key, None)
    a, b = train(key, dtype, False), train(key, dtype, True)
    # the same masks, the same bits at the end
    assert len(a["keep"]) == 3 and all(np.array_equal(x, y) for x, y in zip(a["keep"], b["keep"]))
    for name, x, y in zip(("W", "exp_avg", "exp_avg_sq", "state"), a["final"], b["final"]):
        assert np.array_equal(x, y), name
    live0 = int(a["keep"][0].sum())
    assert live0 == len(T) - int(math.floor(0.5 * len(T)))
    grown_seen = 0
    for i, step in enumerate(REGROW_AFTER):
        before, after = a["keep"][i], a["keep"][i + 1]
        assert int(after.sum()) == live0                                                    # the live count is constant
        dropped, grown = (before == 1) & (after == 0), (before == 0) & (after == 1)
        assert int(dropped.sum()) == int(grown.sum()) and 0 < int(grown.sum()) <= int(math.floor(0.3 * live0))
        assert np.all(T[grown, 1] > 0)                                                      # a block without an element inside the matrix is never grown
        for name, t in zip(("W", "exp_avg", "exp_avg_sq"), a["after_regrow"][i]):
            assert not block_any(T, t)[after == 0].any(), (step, name)                      # dropped (and every other dead) block: all-zero bits
            assert not block_any(T, t)[grown].any(), (step, name)                           # grown blocks start at +0.0
        if step + 1 < STEPS:
            assert block_any(T, a["W_after_step"][step + 1])[grown].all(), step            # ... and train from the next step on
            grown_seen += int(grown.sum())
    assert grown_seen > 0
    dead = np.repeat(a["keep"][-1] == 0, T[:, 2])
    for t in a["final"][:3]:
        assert not t[dead].any()
    out, ref = a["forward"]
    assert np.isfinite(out).all() and np.abs(ref).max() > 0 and np.array_equal(out, ref)
