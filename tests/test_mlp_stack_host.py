"""The inputs of tests/test_mlp_stack_gpu.py, checked without a GPU on a float64 model of its loop (dense products, torch's Adam formula, select on the
host scores): the conditions that test asserts on the device must already hold here, with room -- the geometry (a ragged last block column that holds
blocks, the weak block-row / block column), both layers losing blocks beyond the weak ones and keeping some, the weak blocks wholly dead after the last
prune, the clip at work at every finished step, and every 16-bit intermediate (h, dz, grad_x under the loss scale) far inside fp16's range."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_mlp_stack_gpu as T  # noqa: E402

erf = np.vectorize(math.erf, otypes=[np.float64])


def act_and_slope(name, u):
    if name == "relu":
        return np.maximum(u, 0.0), (u > 0).astype(np.float64)
    if name == "gelu":
        cdf = 0.5 * (1.0 + erf(u / math.sqrt(2.0)))
        return u * cdf, cdf + u * np.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    return u, np.ones_like(u)


@pytest.mark.parametrize("name", list(T.CONFIGS))
def test_conditions_on_a_float64_model(name):
    g1, g2, xs, gys, b1, b2 = T.geometry(name)
    cfg = T.CONFIGS[name]
    gs, specs = (g1, g2), (cfg["l1"], cfg["l2"])
    assert (g1.v.rows, g1.v.cols, g2.v.rows, g2.v.cols) == (T.HID, T.IN, T.OUT, T.HID)
    assert T.bias_runs(T.N) == 2 and all(T.sa.epilogue.scratch_bytes(r, T.N) == 16 * r for r in (T.HID, T.OUT))
    W = [g.W0.astype(np.float64) for g in gs]
    M, V = [np.zeros(g.nz) for g in gs], [np.zeros(g.nz) for g in gs]
    b = [b1.astype(np.float64), b2.astype(np.float64)]
    keeps = [np.ones(g.nb, np.uint8) for g in gs]
    scale, tracker, t, big = T.LOSS_SCALE, 0, 0, 0.0
    lr, wd, b1m, b2m, eps = T.ADAM["lr"], T.ADAM["weight_decay"], 0.9, 0.999, 1e-8
    for step in range(1, T.STEPS + 1):
        x, gy = xs[step - 1].astype(np.float64), gys[step - 1].astype(np.float64)
        planted = not np.isfinite(gy).all()
        assert planted == (step == T.INF_STEP) and (~np.isfinite(gy)).sum() == int(planted)
        gy = np.where(np.isfinite(gy), gy, 0.0)                      # the model follows the finite part; the step is skipped below
        A = [g.dense(w, s["dtype"]) for g, w, s in zip(gs, W, specs)]
        u1 = x @ A[0].T + b[0]
        h, slope = act_and_slope(specs[0]["act"], u1)
        h = T.U.edge_round(h, {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}[specs[0]["out"]])
        dy = gy * scale
        dh = dy @ A[1]
        dz1 = dh * slope
        assert np.abs(u1).max() <= 6.25                              # the range tests/test_epilogue_gpu.py measures GELU on
        big = max(big, np.abs(dy).max(), np.abs(dh).max(), np.abs(dz1).max(), np.abs(h).max())
        if planted:
            assert keeps[1][g2.brow == g2.strong].all() and min(k.min() for k in keeps) == 0          # the Inf meets live blocks only, and blocks are dead by then
            scale, tracker = scale * 0.5, 0
        else:
            G = [g.sample(d.T @ xin) for g, d, xin in ((g1, dz1, x), (g2, dy, h))]
            for i, g in enumerate(gs):
                G[i][g.element_dead(keeps[i])] = 0.0
            db = [dz1.sum(0), dy.sum(0)]
            norm = math.sqrt(sum(float((a * a).sum()) for a in G + db)) / scale
            assert norm > 4.0 * T.MAX_NORM, (step, norm)                 # the clip is at work, with room
            coef = T.MAX_NORM / (norm + 1e-6) / scale
            t += 1
            for i in range(2):
                gi = G[i] * coef
                M[i] = b1m * M[i] + (1 - b1m) * gi
                V[i] = b2m * V[i] + (1 - b2m) * gi * gi
                W[i] = W[i] * (1 - lr * wd) - lr / (1 - b1m ** t) * M[i] / (np.sqrt(V[i]) / math.sqrt(1 - b2m ** t) + eps)
                b[i] = b[i] - T.LR_B * coef * db[i]
            tracker += 1
            if tracker >= T.GROWTH_INTERVAL:
                scale, tracker = scale * 2.0, 0
        if step in T.PRUNE_AFTER:
            scores = [g.scores(w) for g, w in zip(gs, W)]
            new = T.select_host(scores, keeps, T.PRUNE_AFTER[step])
            sc = np.sort(np.concatenate(scores)[np.concatenate(keeps) == 1])
            k = int((np.concatenate(new) == 0).sum() - (np.concatenate(keeps) == 0).sum())
            assert 0 < k < len(sc) and sc[k] > sc[k - 1] * 1.002      # the cut falls into a gap of the scores: the last bits of a sum do not move it
            keeps = new
            for i, g in enumerate(gs):
                dead = g.element_dead(keeps[i])
                W[i][dead], M[i][dead], V[i][dead] = 0.0, 0.0, 0.0
    assert scale == 2048.0
    assert big < 65504.0 / 4, big                                    # fp16's range, with room for what the rounded arithmetic does differently
    for g, k in zip(gs, keeps):
        assert not k[g.weak].any() and k.max() == 1 and int((k == 0).sum()) > len(g.weak), (name, k.tolist(), g.weak.tolist())
    assert sum(int((k == 0).sum()) for k in keeps) == math.floor(0.75 * sum(g.nb for g in gs))
