"""The inputs of tests/test_lifecycle_gpu.py, checked without a GPU on the numpy model of tests/_lifecycle.py, for every geometry, optimizer and both
schedules (with and without compact / grow).  Where a seed fails a condition the seed changes (GEOS of tests/_lifecycle.py), never the condition:
  - at every prune and regrow cut the two scores next to the cut differ by more than 1e-9 relative, magnitude and gradient scores alike: the device's fp64
    block sums differ from fsum by about n * 2^-53 < 1e-12 for a block of at most 64 x 128 elements, so no mask can depend on the order of a sum;
  - every x, T * loss_scale and gradient element is an integer exact in the operand type and in fp32; the loss scale stays at or below 64;
  - the planted Inf is one element at step 5, that step alone skips, and it meets a live block in every arm (the masks are the same in every arm);
  - after the first prune a block-row of some pair is wholly dead (spmm_t and sddmm meet empty lists); the clip is at work at every finished step;
  - in the runs that repattern, no compact or grow leaves a 16-bit pair without the one stream image the fp8 weight image needs (an emptied 32-row
    block-row whose partner keeps blocks, a pair without a block): tests/test_repattern_gpu.py owns that case."""
import numpy as np
import pytest

import sparta_amd as sa

torch = pytest.importorskip("torch")

import _lifecycle as LC  # noqa: E402

RUNS = [(g, "adamw") for g in LC.GEOS] + [("w96", "sgd"), ("w13z", "sgd")]


@pytest.mark.parametrize("rep", [False, True], ids=["plain", "repattern"])
@pytest.mark.parametrize("geo,kind", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_conditions_of_the_schedule(geo, kind, rep):
    patterns = []

    def watch(m, what):
        if what[0] in ("compact", "grow"):
            patterns.append((what[0], [p.pattern() for p in m.pairs], [p.dtype for p in m.pairs]))

    m = LC.run_model(geo, kind, rep, watch)
    steps = [n for n in m.notes if "t" in n]
    events = [n for n in m.notes if "event" in n]
    assert [n["t"] for n in steps] == list(range(1, LC.STEPS + 1))
    # the cuts
    assert len(m.gaps) >= 6, m.gaps                                  # two prunes, two regrows with two cuts each
    for ev, which, gap in m.gaps:
        assert gap > 1e-9, (geo, kind, rep, ev, which, gap)
    # exactness
    for n in steps:
        assert n["scale_before"] <= 64.0 and n["max_int"] < 2.0 ** 24, n
        assert 3 * n["scale_before"] <= 256.0                        # T * loss_scale: an integer that bf16 (8 bits) and fp16 (11 bits) hold exactly
    assert [n["scale_before"] for n in steps] == [4.0, 4.0, 8.0, 8.0, 16.0, 8.0, 8.0, 16.0, 16.0, 32.0]
    # the Inf and the clip
    assert [n["skip"] for n in steps] == [1 if n["t"] == LC.INF_STEP else 0 for n in steps]
    assert [n["nonfinite"] > 0 for n in steps] == [n["t"] == LC.INF_STEP for n in steps]
    x, T = m.inputs(LC.INF_STEP)[0]
    assert int((~np.isfinite(T)).sum()) == 1 and np.isinf(T[LC.INF_SAMPLE, m.inf_row]) and all(np.isfinite(t).all() for _, t in m.inputs(LC.INF_STEP)[1:])
    for n in steps:
        if not n["skip"]:
            assert 0.0 < n["coef"] < 1.0 / n["scale_before"], ("the clip is not at work", n)
    # the events
    first = next(n for n in events if n["event"][0] == "prune")
    assert any(rows for rows in first["dead_rows"]), "no block-row is wholly dead after the first prune"
    assert first["total"] - first["live"] == m.n0 // 2
    assert all(n["changed"] > 0 for n in events if n["event"][0] in ("prune", "prune_to", "regrow"))
    assert all(n["swapped"] > 0 for n in events if n["event"][0] == "regrow")
    last = [n for n in events if n["event"][0] == "prune_to"][0]
    assert last["total"] - last["live"] == (3 * m.n0) // 4 - (m.n0 // 2 if rep else 0)
    # the fp8 arms that repattern never meet a pattern without the one image
    assert len(patterns) == (2 if rep else 0)
    if all(p.dtype != sa.F32 for p in m.pairs):
        assert all(LC.one_image(LC.geometry(p.key)) for p in m.pairs)
        for what, vs, _ in patterns:
            for i, v in enumerate(vs):
                assert int(v.nztot) > 0 and LC.one_image(v), (geo, kind, what, i, "this pattern has no fp8 form")


def test_layout_places_blocks_by_key():
    """the layout helper against edge_dense: a dict whose block (ib, jb) holds ib * 100 + jb everywhere comes out where the pattern stores that block"""
    v = LC.geometry("pairs_even")
    blocks = {k: {"W": np.full(32 * 32, 100 * k[0] + k[1], np.float32)} for k in LC.block_keys(v)}
    import _util as U
    D = U.edge_dense(v, 0, mab=LC.layout(v, blocks, "W"))
    for ib, jb in blocks:
        assert np.all(D[32 * ib:32 * ib + 32, 32 * jb:min(32 * jb + 32, v.cols)] == 100 * ib + jb)
    with pytest.raises(AssertionError):
        LC.layout(v, dict(list(blocks.items())[1:]), "W")


def test_one_image_rule():
    import _util as U
    mk = lambda hts, pres: U.sa_vbr(U._edge_arrays(sum(hts), 128, 32, hts, pres), np.zeros(sum(h * len(p) for h, p in zip(hts, pres)) * 32, np.float32))  # noqa: E731
    assert LC.one_image(mk([32, 32, 32], [[0], [1], []]))            # a pair, an empty block-row
    assert not LC.one_image(mk([32, 32, 32], [[0], [1], [2]]))       # a pair and a block-row left alone
    assert LC.one_image(mk([32, 32], [[0], []]))                     # one 32-row block-row: the one-tile image alone
    assert not LC.one_image(mk([32, 32, 32, 32], [[0], [], [1], [2]]))
    assert LC.one_image(mk([20, 20], [[0], [1]])) and LC.one_image(mk([100], [[0, 1]])) and not LC.one_image(mk([80], [[0]]))
    assert not LC.one_image(mk([32, 32], [[], []]))                  # no block: no image
