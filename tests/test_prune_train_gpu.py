"""sparta_amd.BlockPruner through real training steps: vbs_linear -> backward -> pruner.mask_grads() -> GradCtl.collect -> step(ctl=), with prune(0.5) after
the first step and prune(0.75) after the third, on w48, w128h20, w128h80 (fp32: both forms of a step occur) and w96 (f16) of train_geometries().

x and grad_y hold -1, 0, 1 and n = 2, as in the step suites' own vbs_linear tests: the gradient of the values is small integers whatever the values are, so
values and optimizer state must equal sgd_ref / adam_ref on the masked gradient (times the coef read back from the record) bit for bit.  The masks themselves
are checked against scores recomputed on the host in float64 (no pruned block scores above a kept one, beyond the rounding of the device's sum)."""
import math

import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd.autograd import vbs_linear

torch = pytest.importorskip("torch")

import _util as U  # noqa: E402
from test_set_values_gpu import TDT, dense_b, product, rounded, check_close  # noqa: E402
from test_spmm_t_gpu import with_values, dense_x  # noqa: E402
from test_sgd_step_gpu import sgd_ref, same_bits  # noqa: E402
from test_adam_step_gpu import draw_w  # noqa: E402
from test_adam_step_host import adam_ref, fresh_state  # noqa: E402
from test_grad_ctl_host import stats_ref  # noqa: E402
from test_grad_ctl_gpu import scaled, within  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
GEOMS = [("w48", sa.F32), ("w128h20", sa.F32), ("w128h80", sa.F32), ("w96", sa.F16)]
ARMS = {"adamw": dict(kind="adam", lr=1e-2, weight_decay=0.01, decoupled=True), "adam-l2": dict(kind="adam", lr=1e-2, weight_decay=0.01, decoupled=False),
        "sgd-momentum-wd": dict(kind="sgd", lr=0.25, momentum=0.9, weight_decay=0.01), "sgd-plain": dict(kind="sgd", lr=0.25)}
N = 2


def make_opt(arm, pairs):
    cfg = dict(ARMS[arm])
    if cfg.pop("kind") == "adam":
        return sa.VbsAdamW(pairs, **cfg), cfg
    return sa.VbsSGD(pairs, **cfg), cfg


def element_mask(T, keep):
    """per stored element: True where its block is pruned"""
    m = np.zeros(int(T[:, 2].sum()), bool)
    for b in np.flatnonzero(np.asarray(keep) == 0):
        m[int(T[b, 0]):int(T[b, 0] + T[b, 2])] = True
    return m


def host_scores(T, W):
    sq = np.asarray(W, np.float64) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.array([math.fsum(sq[o:o + n]) / n if n else np.inf for o, n in zip(T[:, 0], T[:, 1])])


def check_product(d, v, dtype, W, B, what):
    """the handle multiplies as a handle created from W does: product and check_close of tests/test_set_values_gpu.py, against the float64 oracle on the
    values as the handle's type stores them"""
    C, Br = product(d, v, B, dtype)
    check_close(C, v, W if dtype == sa.F32 else rounded(W, dtype), Br, what)


def optimizer_state(opt, kind, nz):
    if kind == "adam":
        s = opt._state[0]
        return (np.zeros(nz, f32), np.zeros(nz, f32)) if s is None else (s["exp_avg"].cpu().numpy(), s["exp_avg_sq"].cpu().numpy())
    return (None if opt._bufs[0] is None else opt._bufs[0].cpu().numpy(),)


@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("key,dtype", GEOMS, ids=["%s-%s" % (k, {sa.F32: "f32", sa.F16: "f16"}[dt]) for k, dt in GEOMS])
def test_pruned_blocks_stay_zero_through_training(key, dtype, arm, monkeypatch):
    for var in ("SPARTA_SGD_FUSE", "SPARTA_ADAM_FUSE"):
        monkeypatch.delenv(var, raising=False)
    v = U.train_geometries()[key]
    T = v.block_table()
    nz, nb = int(v.nztot), len(T)
    W0 = draw_w(v, 90)
    H = v.to_device(0, dtype=dtype, updatable=True, transposable=True)
    W = torch.from_numpy(W0.copy()).cuda().requires_grad_(True)
    opt, cfg = make_opt(arm, [(H, W)])
    kind = ARMS[arm]["kind"]
    pruner = sa.BlockPruner(opt)
    assert H.n_blocks == nb and pruner.sparsity() == 0.0
    assert np.array_equal(pruner._n_in[0].cpu().numpy(), T[:, 1].astype(np.float64))          # the elements inside the matrix, from the device
    ctl = sa.GradCtl(max_norm=1.0)
    x64 = np.ascontiguousarray(np.sign(dense_b(v, N, 91, integer=True).T))
    x = torch.from_numpy(x64).cuda().to(TDT[dtype])
    B = dense_b(v, 32, 92, integer=False)
    Wr, M, V, S = W0.copy(), np.zeros(nz, f32), np.zeros(nz, f32), fresh_state()
    keep = np.ones(nb, np.uint8)
    for step in range(1, 5):
        gy = torch.from_numpy(np.sign(dense_x(v.rows, N, 92 + step, integer=True).T)).float().cuda()
        opt.zero_grad()
        y = vbs_linear(x, H, W)
        # the forward multiplies with the values as they are now, pruned blocks included (whatever the handle recorded before)
        check_close(np.ascontiguousarray(y.detach().cpu().numpy().T), v, Wr if dtype == sa.F32 else rounded(Wr, dtype), x64.T, ("forward", step))
        y.backward(gy)
        G_raw = W.grad.cpu().numpy().copy()
        pruner.mask_grads()
        G = W.grad.cpu().numpy().copy()
        pruned = element_mask(T, keep)
        assert not G[pruned].view(np.uint32).any() and same_bits(G[~pruned], G_raw[~pruned]), step
        if step > 1:
            assert G_raw[pruned].any()                               # the SDDMM still computes the pruned blocks: the mask is what zeroes them
        ctl.collect(opt)
        opt.step(ctl=ctl)
        r = ctl.read()
        want_ssq, bad = stats_ref(G)
        assert bad == 0 and r["skip"] == 0 and within(r["ssq"], want_ssq, nz), (step, r, want_ssq)
        norm = f32(np.sqrt(want_ssq))                                # the norm of the MASKED gradient; the device's sum is within nz * 2^-53 of fsum: at most
        assert abs(f32(r["norm"]) - norm) <= np.spacing(norm), (step, r["norm"], norm)          # one fp32 ulp after the rounded square root
        assert step == 1 or r["norm"] < f32(np.sqrt(stats_ref(G_raw)[0]))
        assert 0 < r["coef"] < 1.0                                   # clipped
        g = scaled(G, 1.0, f32(r["coef"]))
        if kind == "adam":
            Wr, M, V, S = adam_ref(Wr, g, M, V, S, cfg)
            got = (W.detach().cpu().numpy(),) + optimizer_state(opt, kind, nz)
            for name, a, b in zip("WMV", got, (Wr, M, V)):
                assert same_bits(a, b), (step, name)
        else:
            Wr, Mn = sgd_ref(Wr, g, M, cfg["lr"], cfg.get("momentum", 0.0), cfg.get("weight_decay", 0.0))
            M = Mn if cfg.get("momentum", 0.0) != 0 else M
            got = (W.detach().cpu().numpy(),) + optimizer_state(opt, kind, nz)
            assert same_bits(got[0], Wr), step
            assert (got[1] is None) == (cfg.get("momentum", 0.0) == 0)
            if got[1] is not None:
                assert same_bits(got[1], M), step
        for a in got:
            if a is not None:
                assert not a[pruned].view(np.uint32).any(), step     # all-zero bits: +0.0, in values and in every state tensor
        if step in (1, 3):
            s = 0.5 if step == 1 else 0.75
            scores = host_scores(T, Wr)
            pruner.prune(s)
            new = pruner.keep_masks()[0].cpu().numpy()
            assert np.all(new <= keep) and int((new == 0).sum()) == math.floor(s * nb), step
            assert pruner.sparsity() == math.floor(s * nb) / nb
            newly = (new == 0) & (keep == 1)
            assert scores[newly].max() <= scores[new == 1].min() * (1 + 1e-12), step           # the lowest scores went (ties and the last bits of the sum aside)
            keep = new
            pruned = element_mask(T, keep)
            Wr, M, V = Wr.copy(), M.copy(), V.copy()
            Wr[pruned], M[pruned], V[pruned] = 0.0, 0.0, 0.0
            got = (W.detach().cpu().numpy(), W.grad.cpu().numpy()) + optimizer_state(opt, kind, nz)
            assert same_bits(got[0], Wr)
            for a in got:
                if a is not None:
                    assert not a[pruned].view(np.uint32).any(), step
        # the handle multiplies as a handle created from the values does
        check_product(H, v, dtype, Wr, B, ("product", step))
    assert (Wr[~pruned] != W0[~pruned]).any() and not Wr[pruned].any()

    # the masks travel: a new pruner on re-initialised pairs
    sd = pruner.state_dict()
    assert all(k.dtype == torch.uint8 and k.device.type == "cpu" for k in sd["keep"])
    H2 = v.to_device(0, dtype=dtype, updatable=True, transposable=True)
    W2 = torch.from_numpy(W0.copy()).cuda().requires_grad_(True)
    opt2, _ = make_opt(arm, [(H2, W2)])
    p2 = sa.BlockPruner(opt2)
    p2.load_state_dict(sd)
    assert np.array_equal(p2.keep_masks()[0].cpu().numpy(), keep) and p2.sparsity() == pruner.sparsity()
    W2h = W2.detach().cpu().numpy()
    want2 = W0.copy()
    want2[pruned] = 0.0
    assert same_bits(W2h, want2)
    check_product(H2, v, dtype, want2, B, "loaded")
    H3 = with_values(v, want2).to_device(0, dtype=dtype, updatable=True, transposable=True)          # ... and as a handle created from them, same plan, same path
    check_product(H3, v, dtype, want2, B, "fresh")
    H3.close()
    with pytest.raises(ValueError):
        p2.load_state_dict({"keep": []})
    H.close()
    H2.close()


def test_mask_grads_replays_in_a_graph_and_layer_scope():
    """two layers: mask_grads captured after its first call follows masks that prune() updates in place; scope 'layer' prunes each pair on its own"""
    vs = [U.train_geometries()[k] for k in ("w48", "w128h20")]
    pairs, W0s = [], []
    for i, v in enumerate(vs):
        W0s.append(draw_w(v, 95 + i) * f32(1.0 if i == 0 else 8.0))                                               # layer 1's scores 64 times what they would be
        W = torch.from_numpy(W0s[i].copy()).cuda().requires_grad_(True)
        W.grad = torch.ones_like(W)
        pairs.append((v.to_device(0, updatable=True), W))
    pg, pl = sa.BlockPruner(pairs, scope="global"), sa.BlockPruner([(h, w.detach().clone().requires_grad_(True)) for h, w in pairs], scope="layer")
    nbs = [len(v.block_table()) for v in vs]
    pl.prune(0.5)
    assert [int((k == 0).sum()) for k in pl.keep_masks()] == [nb // 2 for nb in nbs]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        pg.mask_grads()                                              # the first call uploads the tables (nothing pruned yet: nothing changes)
        torch.cuda.synchronize()
        assert all(bool((w.grad == 1).all()) for _, w in pairs)
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph, stream=s):
            pg.mask_grads()
        pg.prune(0.25)
        for _, w in pairs:
            w.grad.fill_(1.0)
        torch.cuda.synchronize()
        gph.replay()
    torch.cuda.synchronize()
    cut = [int((k == 0).sum()) for k in pg.keep_masks()]
    assert sum(cut) == math.floor(0.25 * sum(nbs)) and cut != [math.floor(0.25 * nb) for nb in nbs]          # global: the layer of small values pays more
    sc = np.concatenate([host_scores(v.block_table(), w0) for v, w0 in zip(vs, W0s)])
    gone = np.concatenate([k.cpu().numpy() for k in pg.keep_masks()]) == 0
    assert sc[gone].max() <= sc[~gone].min() * (1 + 1e-12)
    for (h, w), v, k in zip(pairs, vs, pg.keep_masks()):
        pruned = element_mask(v.block_table(), k.cpu().numpy())
        g = w.grad.cpu().numpy()
        assert not g[pruned].any() and (g[~pruned] == 1).all()
        assert not w.detach().cpu().numpy()[pruned].any()
    for h, _ in pairs:
        h.close()
