"""The packed fp32 plan on the device (vbs_plan.cpp "PACKED PLAN", k_f32_packed.hip): small handles of 32-wide blocks made with
SPARTA_F32_PLAN=packed against the same matrix made with SPARTA_F32_PLAN=direct and against float64.

Integer-valued operands (every sum far below 2^24) make every summation order exact, so packed, direct and the oracle must agree bit for bit
whatever step a block landed in; general values are held to U.gamma_bound.  The geometries sit on the boundaries of the packing rule: group
counts that just fit a step and just do not, blocks whose only group is the first or the last, short tiles, an empty block-row between two
tiles, a block of the zero-padded last block column (never packed), a tile long enough to be split across workers, tiles that do not start
on multiples of 32 rows (the C ring), block-row ranges, and the rebuild of the reference-layout image from the packed image."""
import numpy as np
import pytest

import sparta_amd as sa

torch = pytest.importorskip("torch")
import tests.test_poison_gpu as PG  # noqa: E402
from tests import _util as U  # noqa: E402

pytestmark = pytest.mark.gpu

ENV = PG.ENV + ("SPARTA_F32_PLAN", "SPARTA_CSTAGE", "SPARTA_F32_KEEP_LEGACY", "SPARTA_STREAM_ALIGN")
FULL = 0xff


@pytest.fixture(autouse=True)
def stream_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SPARTA_PATH", "stream")          # the plan under test, not the winner of the plan-time autotune
    monkeypatch.setenv("SPARTA_SPARSE_K", "0")           # every block-row stays in the dense-block plans


def build(heights, present, masks, cols, kind, seed):
    """VBR of 32-wide blocks: block-row ib has the block columns present[ib]; masks (one per stored block, in storage order): bit m set = the
    columns 4 m .. 4 m + 3 of the block hold non-zeros in every row, clear = they hold zeros.  kind 'int': -3 .. 3 without zero, 'real': uniform(-1, 1)"""
    arr = U._edge_arrays(int(sum(heights)), cols, 32, heights, present)
    rng = np.random.default_rng(seed)
    parts = []
    q = 0
    for h, p in zip(heights, present):
        for _ in p:
            x = rng.integers(-3, 4, (32, h)).astype(np.float32) if kind == "int" else rng.uniform(-1, 1, (32, h)).astype(np.float32)
            x[x == 0] = 2.0
            keep = np.repeat([(masks[q] >> m) & 1 for m in range(8)], 4).astype(bool)
            x[~keep] = 0.0
            parts.append(x.reshape(-1))                  # column-major h x 32: column k is h consecutive values
            q += 1
    assert q == len(masks)
    return U.sa_vbr(arr, np.concatenate(parts) if parts else np.zeros(0, np.float32))


def handle(v, plan, monkeypatch, br=None):
    monkeypatch.setenv("SPARTA_F32_PLAN", plan)
    d = v.to_device(0, block_row_range=br)
    assert d.packed_info()["packed"] == (1 if plan == "packed" else 0), (plan, d.packed_info())
    return d


def b_operand(cols, n, kind, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-3, 4, (cols, n)).astype(np.float64) if kind == "int" else U.edge_round(rng.uniform(-1, 1, (cols, n)), sa.F32)


def product(d, rows, B, ldb, n, row_major=False, C0=None):
    got = PG.spmm(d, rows, PG.dev_in(B, ldb, sa.F32), ldb, n, row_major=row_major, C0=C0)
    assert d.info()["last_path"] == 1
    return got


# name -> (heights, present, masks, cols, packed steps the plan must have)
CASES = {
    # 3 + 5 and 4 + 4 fill a step exactly (two tiles); 5 + 4 does not (two steps); 1 + 2 + 5 and 7 + 1
    "sum8": ([32, 32, 32], [[0, 3], [1, 2], [0, 1, 2, 4, 5]], [0x07, 0xf8, 0x0f, 0xf0, 0x80, 0x03, 0x1f, 0xfe, 0x01], 192, 1 + 1 + 2),
    "sum9": ([32, 32], [[0, 2], [1, 3, 5]], [0x1f, 0xf0, 0x3f, 0x07, 0x01], 192, 2 + 2),
    # blocks whose only group is the first or the last; eight of them make one step; a full block stays alone, an all-zero block takes no slot
    "edges": ([32, 32], [[0, 1, 2, 3, 4, 5, 6, 7], [0, 2, 4]], [0x01, 0x80, 0x80, 0x01, 0x01, 0x80, 0x01, 0x80, FULL, 0x00, 0x81], 256, 1 + 2),
    # tile heights 1, 17, 31 and 32
    "heights": ([1, 17, 31, 32], [[0, 1, 2], [1, 3], [0, 2, 3], [0, 1, 2, 3]], [0x03, 0x0c, 0xf0, 0x55, 0xaa, 0x18, 0x24, 0x42, 0x0f, 0x10, 0x20, 0xc0], 128, 1 + 1 + 1 + 1),
    # an empty block-row between two tiles
    "gap": ([32, 20, 32], [[0, 2], [], [1, 3]], [0x3c, 0xc3, 0x0f, 0xf1], 128, 1 + 2),
    # cols = 32 k + 19: the blocks of the last block column hang over the last row of B and keep a step of their own (4 + 2 + 2 groups would fit one step)
    "tail": ([32, 9], [[0, 2, 4], [1, 4]], [0x0f, 0x30, 0x03, 0x3f, 0x11], 32 * 4 + 19, 2 + 2),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_boundaries_are_exact(name, monkeypatch):
    heights, present, masks, cols, want_steps = CASES[name]
    v = build(heights, present, masks, cols, "int", 3)
    dp, dd = handle(v, "packed", monkeypatch), handle(v, "direct", monkeypatch)
    pi = dp.packed_info()
    assert pi["steps"] == want_steps and pi["block_steps"] == len(masks), pi
    assert pi["slots"] == sum(bin(m).count("1") for m in masks), pi
    D = U.edge_dense(v)
    ldb = cols + 5                                       # ldb > cols
    for n in (128, 256):
        B = b_operand(cols, n, "int", 10 + n)
        C0 = np.random.default_rng(n).integers(-9, 10, (v.rows, n)).astype(np.float32)
        for acc in (False, True):
            for row_major in (False, True):
                want = D @ B + (C0 if acc else 0.0)
                got_p = product(dp, v.rows, B, ldb, n, row_major, C0 if acc else None)
                got_d = product(dd, v.rows, B, ldb, n, row_major, C0 if acc else None)
                what = (name, n, acc, row_major)
                assert np.array_equal(got_p, want.astype(np.float32)), (what, float(np.abs(got_p - want).max()))
                assert np.array_equal(got_p, got_d), what


@pytest.mark.parametrize("name", ["heights", "tail", "sum9"])
def test_general_values_within_gamma_bound(name, monkeypatch):
    heights, present, masks, cols, _ = CASES[name]
    v = build(heights, present, masks, cols, "real", 5)
    dp = handle(v, "packed", monkeypatch)
    D = U.edge_dense(v)
    n = 128
    B = b_operand(cols, n, "real", 6)
    C0 = np.random.default_rng(7).uniform(-1, 1, (v.rows, n)).astype(np.float32)
    for acc in (False, True):
        c0 = C0.astype(np.float64) if acc else None
        got = product(dp, v.rows, B, cols + 1, n, False, C0 if acc else None).astype(np.float64)
        err, tol = np.abs(got - (D @ B + (c0 if acc else 0.0))), U.gamma_bound(D, B, c0)
        assert (err <= tol).all(), (name, acc, float((err / np.maximum(tol, 1e-300)).max()))


def test_split_tile(monkeypatch):
    """one tile of 2000 blocks with mixed fill: the plan cuts it across workers, every worker packs its own segment and the fix-up adds the partial images"""
    rng = np.random.default_rng(8)
    nb = 2000
    masks = [FULL if rng.random() < 0.4 else int(rng.integers(1, 256)) for _ in range(nb)]
    v = build([32], [list(range(nb))], masks, 32 * nb, "real", 9)
    dp = handle(v, "packed", monkeypatch)
    assert dp.info()["split_tiles"] >= 1 and dp.packed_info()["steps"] < nb, (dp.info(), dp.packed_info())
    D = U.edge_dense(v)
    B = b_operand(v.cols, 128, "real", 12)
    for acc in (False, True):
        C0 = np.random.default_rng(13).uniform(-1, 1, (32, 128)).astype(np.float32)
        c0 = C0.astype(np.float64) if acc else None
        got = product(dp, 32, B, v.cols, 128, False, C0 if acc else None).astype(np.float64)
        err, tol = np.abs(got - (D @ B + (c0 if acc else 0.0))), U.gamma_bound(D, B, c0)
        assert (err <= tol).all(), (acc, float((err / np.maximum(tol, 1e-300)).max()))


def ragged(seed, kind="real"):
    """14 short tiles that do not start on multiples of 32 rows, two to five partly empty blocks each"""
    rng = np.random.default_rng(seed)
    heights = [20, 28, 17, 31, 9, 32, 25, 12, 30, 7, 32, 19, 26, 5]
    present = [sorted(rng.choice(8, int(rng.integers(2, 6)), replace=False).tolist()) for _ in heights]
    masks = [int(rng.integers(1, 256)) for p in present for _ in p]
    return build(heights, present, masks, 256, kind, seed + 1)


def test_ring_and_direct_stores_agree(monkeypatch):
    v = ragged(20)
    dp = handle(v, "packed", monkeypatch)
    B = b_operand(v.cols, 128, "real", 21)
    got = {}
    for cst in ("1", "0"):
        monkeypatch.setenv("SPARTA_CSTAGE", cst)
        got[cst] = product(dp, v.rows, B, v.cols, 128)
    assert np.array_equal(got["1"], got["0"])
    D = U.edge_dense(v)
    assert (np.abs(got["1"] - D @ B) <= U.gamma_bound(D, B)).all()


def test_range_handles_give_the_whole_handles_rows(monkeypatch):
    v = ragged(30)
    B = b_operand(v.cols, 128, "real", 31)
    whole = product(handle(v, "packed", monkeypatch), v.rows, B, v.cols, 128)
    for br in ((0, 5), (5, 14), (3, 4)):
        d = handle(v, "packed", monkeypatch, br=br)
        r0, r1 = int(v.row_part[br[0]]), int(v.row_part[br[1]])
        got = product(d, r1 - r0, B, v.cols, 128)
        assert np.array_equal(got, whole[r0:r1]), br


def test_legacy_image_rebuilt_from_the_packed_image(monkeypatch):
    """a column-major product drops the reference-layout image; a row-major B needs it again.  The LDS-staged kernel then walks the SAME step list on both
    handles, so its products agree element for element exactly when the image rebuilt from the packed image equals the one rebuilt from the fragment image"""
    v = ragged(40)
    n = 128
    B = b_operand(v.cols, n, "real", 41)
    Brm = torch.from_numpy(np.ascontiguousarray(B, np.float32).reshape(-1)).cuda()          # row-major cols x n
    out = {}
    for plan in ("packed", "direct"):
        d = handle(v, plan, monkeypatch)
        before = d.info()["a_bytes"]
        product(d, v.rows, B, v.cols, n)
        assert d.info()["a_bytes"] < before, (plan, "the reference-layout image was not dropped")
        Cd = PG.out_tensor(v.rows, n, False, None)
        d.spmm(Brm, Cd, n, b_layout=sa.ROW_MAJOR)
        torch.cuda.synchronize()
        assert d.info()["last_path"] == 1 and d.info()["a_bytes"] == before
        out[plan] = PG.read_out(Cd, v.rows, n, False)
    assert np.array_equal(out["packed"], out["direct"])
    D = U.edge_dense(v)
    assert (np.abs(out["packed"] - D @ B) <= U.gamma_bound(D, B)).all()


def test_unstored_rows_of_b_are_never_read(monkeypatch):
    """NaN in every row of B of the block columns a tile does not store (the groups a packed step gathers come from the tile's own blocks only, and an unused
    slot reads nothing) leaves the tile's rows finite and right; so does NaN behind the last row of B (the padding of ldb)"""
    heights, present, masks, cols, _ = CASES["tail"]
    v = build(heights, present, masks, cols, "real", 50)
    dp = handle(v, "packed", monkeypatch)
    D, stored = U.edge_dense(v), U.stored_mask(v)
    n, ldb = 128, cols + 7
    B = b_operand(cols, n, "real", 51)
    for ib in range(v.block_rows):
        Bp = B.copy()
        for c in range(5):
            if c not in present[ib]:
                Bp[U.block_col_rows(v, c)] = np.nan
        buf = np.full((n, ldb), np.nan, np.float32)
        buf[:, :cols] = Bp.T
        Cd = PG.out_tensor(v.rows, n, False, None)
        dp.spmm(torch.from_numpy(buf.reshape(-1)).cuda(), Cd, n, ldb=ldb)
        torch.cuda.synchronize()
        got = PG.read_out(Cd, v.rows, n, False)[U.block_row_rows(v, ib)].astype(np.float64)
        rows = U.block_row_rows(v, ib)
        assert np.isfinite(got).all(), ib
        assert (np.abs(got - D[rows] @ B) <= U.gamma_bound(D[rows], B)).all(), ib
    assert stored.any()
