"""sparta_amd.prune.select_swap against a numpy restatement of its rule, on the CPU, and the refusals of sparta_vbs_sddmm_block_ssq that need no GPU.

The rule (one scope: all layers together, or one layer): the live blocks in ascending magnitude order -- ties to the lower index, non-finite scores last --
give the blocks to drop; the blocks that are dead before the call and whose gradient score is not -inf, in descending gradient order -- ties to the lower
index, non-finite scores behind every finite one -- give the blocks to grow; both lists are cut to min(n_swap, live blocks, candidates)."""
import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd import _lib
from sparta_amd.prune import select, select_swap

torch = pytest.importorskip("torch")


def swap_rule(mag, grad, keep, n_swap):
    """one scope, plain loops: returns (new keep, dropped indices, grown indices)"""
    n = len(keep)
    live = [i for i in range(n) if keep[i]]
    finite = [i for i in live if np.isfinite(mag[i])]
    drop_order = sorted(finite, key=lambda i: (mag[i], i)) + [i for i in live if not np.isfinite(mag[i])]
    cand = [i for i in range(n) if not keep[i] and not (grad[i] == -np.inf)]
    finite = [i for i in cand if np.isfinite(grad[i])]
    grow_order = sorted(finite, key=lambda i: (-grad[i], i)) + [i for i in cand if not np.isfinite(grad[i])]
    m = min(n_swap, len(drop_order), len(grow_order))
    new = np.array(keep, np.uint8).copy()
    new[drop_order[:m]] = 0
    new[grow_order[:m]] = 1
    return new, drop_order[:m], grow_order[:m]


def layers(seed, sizes, live_p, special):
    rng = np.random.default_rng(seed)
    mag, grad, keep = [], [], []
    for n in sizes:
        m = rng.integers(0, 6, n).astype(np.float64) / 4.0          # few distinct values: ties everywhere
        g = rng.integers(0, 5, n).astype(np.float64) / 8.0
        k = (rng.random(n) < live_p).astype(np.uint8)
        if special and n:
            m[rng.random(n) < 0.15] = np.nan
            m[rng.random(n) < 0.10] = np.inf
            m[rng.random(n) < 0.05] = -np.inf
            g[rng.random(n) < 0.15] = np.nan
            g[rng.random(n) < 0.10] = np.inf
            g[rng.random(n) < 0.20] = -np.inf                       # never grown
        mag.append(m); grad.append(g); keep.append(k)
    return mag, grad, keep


def as_t(arrs, dtype=None):
    return [torch.from_numpy(a.copy()) if dtype is None else torch.from_numpy(a.copy()).to(dtype) for a in arrs]


SETS = [(9400 + i, sizes, p, special) for i, (sizes, p, special) in enumerate([
    ((40,), 0.5, False), ((40,), 0.5, True), ((17, 1, 30), 0.6, True), ((25, 0, 12), 0.3, True), ((64, 64), 0.9, False), ((50, 9), 0.1, True), ((8,), 1.0, True),
    ((8,), 0.0, True)])]


@pytest.mark.parametrize("scope", ["global", "layer"])
@pytest.mark.parametrize("seed,sizes,p,special", SETS, ids=["s%d" % s[0] for s in SETS])
def test_select_swap_follows_the_rule(seed, sizes, p, special, scope):
    mag, grad, keep = layers(seed, sizes, p, special)
    total = sum(sizes)
    for n_swap in (0, 1, 3, total // 4, total + 5):
        if scope == "global":
            cat_new, dropped, grown = swap_rule(np.concatenate(mag), np.concatenate(grad), np.concatenate(keep), n_swap)
            want = np.split(cat_new, np.cumsum(sizes)[:-1])
            got = select_swap(as_t(mag), as_t(grad), as_t(keep), n_swap, "global")
        else:
            per = [min(n_swap, 2 + i) if n_swap else 0 for i in range(len(sizes))] if n_swap < total else [n_swap] * len(sizes)
            res = [swap_rule(m, g, k, n) for m, g, k, n in zip(mag, grad, keep, per)]
            want = [r[0] for r in res]
            dropped, grown = sum((r[1] for r in res), []), sum((r[2] for r in res), [])
            got = select_swap(as_t(mag), as_t(grad), as_t(keep), per, "layer")
        assert len(dropped) == len(grown)
        assert len(got) == len(sizes)
        for g, w, k, gr in zip(got, want, keep, grad):
            g = g.numpy()
            assert g.dtype == np.uint8 and np.array_equal(g, w), (seed, scope, n_swap)
            assert int(g.sum()) == int(k.sum()) or scope == "global"                     # per layer the live count stays ...
            assert not np.any((g == 1) & (k == 0) & (gr == -np.inf))                      # a block marked -inf is never grown
        assert sum(int(g.sum()) for g in got) == sum(int(k.sum()) for k in keep)          # ... and over all layers in either scope


def test_dropped_blocks_are_not_grown_and_ties_follow_select():
    """all scores equal: the swap drops the FIRST live blocks and grows the FIRST dead ones, and none of the dropped blocks comes back in the same call; the
    blocks dropped are the ones select would prune next"""
    n = 24
    keep = np.array([1, 0] * (n // 2), np.uint8)
    mag, grad = np.full(n, 0.5), np.full(n, 0.25)
    got = select_swap(as_t([mag]), as_t([grad]), as_t([keep]), 4)[0].numpy()
    dropped, grown = np.flatnonzero((keep == 1) & (got == 0)), np.flatnonzero((keep == 0) & (got == 1))
    assert dropped.tolist() == [0, 2, 4, 6] and grown.tolist() == [1, 3, 5, 7]
    # select at the sparsity that prunes four more blocks picks the same four (its order among the live blocks is the swap's drop order)
    pruned = select(as_t([mag]), as_t([keep]), (n // 2 + 4) / n)[0].numpy()
    assert np.flatnonzero((keep == 1) & (pruned == 0)).tolist() == dropped.tolist()
    # seeded scores with ties, float32 scores and bool masks: still select's choice
    rng = np.random.default_rng(9450)
    mag = rng.integers(0, 4, n).astype(np.float32)
    got = select_swap(as_t([mag]), as_t([grad]), as_t([keep], torch.bool), 5)[0].numpy()
    pruned = select(as_t([mag]), as_t([keep]), (n // 2 + 5) / n)[0].numpy()
    assert np.array_equal((keep == 1) & (got == 0), (keep == 1) & (pruned == 0))
    # more swaps than either side holds: everything live is dropped only as far as there are candidates, and the other way round
    keep = np.array([1] * 20 + [0] * 4, np.uint8)
    got = select_swap(as_t([np.arange(n, dtype=np.float64)]), as_t([np.ones(n)]), as_t([keep]), 100)[0].numpy()
    assert got.tolist() == [0] * 4 + [1] * 20
    grad = np.ones(n); grad[20:23] = -np.inf
    got = select_swap(as_t([np.arange(n, dtype=np.float64)]), as_t([grad]), as_t([keep]), 100)[0].numpy()
    assert got.tolist() == [0] + [1] * 19 + [0, 0, 0, 1]


def test_select_swap_argument_checks():
    one = [torch.zeros(4)]
    keep = [torch.ones(4, dtype=torch.uint8)]
    with pytest.raises(ValueError):
        select_swap(one, one, keep, 1, scope="row")
    with pytest.raises(ValueError):
        select_swap(one, [torch.zeros(5)], keep, 1)
    with pytest.raises(ValueError):
        select_swap(one, one, keep, 1, scope="layer")                # per layer n_swap is a list
    with pytest.raises(ValueError):
        select_swap(one, one, keep, -1)
    assert select_swap([], [], [], 3) == []
    assert sa.select_swap is select_swap and hasattr(sa, "BlockProbe")


def test_c_entry_refusals_without_a_gpu():
    f = _lib.lib.sparta_vbs_sddmm_block_ssq
    assert "sparta_vbs_sddmm_block_ssq" in _lib.SYMBOLS
    assert f(None, None, 1, None, 1, 4, None, None, None, None) == _lib.ERR_INVALID
    assert b"sparta_vbs_sddmm_block_ssq" in _lib.lib.sparta_last_error() and b"NULL" in _lib.lib.sparta_last_error()
    for k in (0, -1):
        assert f(None, None, 1, None, 1, k, None, None, None, None) == _lib.ERR_INVALID
        assert b"k must be > 0" in _lib.lib.sparta_last_error()
