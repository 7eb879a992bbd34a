"""The packing rule of the packed fp32 plan (sparta_f32_pack_blocks: vbs_plan.cpp and k_f32_packed.hip rest on it), checked on the CPU: hand-made
tiles, invariants on random tiles against first-fit decreasing written in numpy, and the arithmetic of the flagship plan (cant-like FEM under
the fixed 32 x 32 grid: how many steps the packing removes and that it costs no MFMA pair)."""
import ctypes as C

import numpy as np

import sparta_amd as sa
from sparta_amd import _lib

lib = _lib.lib
_u8p, _i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)


def pack(masks):
    m = np.ascontiguousarray(masks, np.uint8)
    step, slot0 = np.full(len(m), -1, np.int32), np.full(len(m), -1, np.int32)
    n = C.c_int32(-1)
    assert lib.sparta_f32_pack_blocks(len(m), m.ctypes.data_as(_u8p), step.ctypes.data_as(_i32p), slot0.ctypes.data_as(_i32p), C.byref(n)) == _lib.OK
    return step, slot0, n.value


def popcount(m):
    return np.unpackbits(np.ascontiguousarray(m, np.uint8)[:, None], axis=1).sum(1).astype(np.int64)


def ffd_numpy(counts):
    """first-fit decreasing by count, ties in ascending index: (step of every block, steps)"""
    order = np.lexsort((np.arange(len(counts)), -np.asarray(counts)))
    used, step = [], np.zeros(len(counts), np.int64)
    for b in order:
        for s, u in enumerate(used):
            if u + counts[b] <= 8:
                break
        else:
            used.append(0)
            s = len(used) - 1
        used[s] += counts[b]
        step[b] = s
    return step, len(used)


def test_exported():
    assert hasattr(lib, "sparta_f32_pack_blocks") and hasattr(lib, "sparta_vbs_packed_info")
    assert "sparta_f32_pack_blocks" in _lib.SYMBOLS and "sparta_vbs_packed_info" in _lib.SYMBOLS
    assert lib.sparta_f32_pack_blocks(3, None, None, None, None) == _lib.ERR_INVALID


def test_hand_made_tiles():
    # eight blocks of one group each (every one a different group of its block): one step, slots 0..7 in block order
    step, slot0, n = pack([1 << m for m in range(8)])
    assert n == 1 and np.all(step == 0) and list(slot0) == list(range(8))
    # 4 + 4: one step; 5 + 4: two
    step, slot0, n = pack([0x0f, 0xf0])
    assert n == 1 and list(step) == [0, 0] and list(slot0) == [0, 4]
    step, slot0, n = pack([0x1f, 0xf0])
    assert n == 2 and list(step) == [0, 1] and list(slot0) == [0, 0]
    # decreasing: the block of five groups goes first although it comes second; the ties (two blocks of three) in block order
    step, slot0, n = pack([0x07, 0xf8, 0x70])
    assert n == 2 and list(step) == [0, 0, 1] and list(slot0) == [5, 0, 0]
    # a full block stays alone
    step, slot0, n = pack([0x03, 0xff, 0x0c])
    assert n == 2 and step[1] == 0 and slot0[1] == 0 and list(step[[0, 2]]) == [1, 1] and list(slot0[[0, 2]]) == [0, 2]
    # no block at all; a block without a group takes no slot
    assert pack([])[2] == 0
    step, slot0, n = pack([0x00])
    assert n == 1 and step[0] == 0 and slot0[0] == 0
    step, slot0, n = pack([0xff, 0x00])
    assert n == 1 and list(step) == [0, 0]


def test_invariants_on_random_tiles():
    rng = np.random.default_rng(11)
    for t in range(1000):
        nb = int(rng.integers(1, 40))
        fill = rng.random()
        masks = np.packbits(rng.random((nb, 8)) < fill, axis=1).reshape(-1)
        if t % 7 == 0:
            masks[rng.integers(nb)] = 0xff
        cnt = popcount(masks)
        step, slot0, n = pack(masks)
        assert step.min() >= 0 and step.max() == n - 1 and len(np.unique(step)) == n          # every block in exactly one step, no empty step
        for s in range(n):
            mine = np.flatnonzero(step == s)
            assert cnt[mine].sum() <= 8
            # the blocks of a step occupy disjoint runs of slots from 0 on
            iv = sorted((int(slot0[b]), int(slot0[b] + cnt[b])) for b in mine if cnt[b] > 0)
            assert all(a[1] == b[0] for a, b in zip(iv, iv[1:])) and (not iv or iv[0][0] == 0)
        ref_step, ref_n = ffd_numpy(cnt)
        assert n <= ref_n and np.array_equal(step, ref_step)
        step2, slot02, n2 = pack(masks)
        assert n2 == n and np.array_equal(step, step2) and np.array_equal(slot0, slot02)


def test_flagship_plan_arithmetic():
    """the plan of bench.py's default workload: 21 910 stored blocks in 1952 tiles become at most 17 300 steps, and the slots -- one MFMA pair
    each -- are exactly the non-empty 4-column groups (132 262: +0.3 % on the pairs of the one-block-per-step plan)"""
    m = sa.gen.cant_like(seed=2)
    eng = sa.BlockingEngine(blocking_algo=5, tau=0.6, col_block_size=32, row_block_size=32, force_fixed_size=True, sim_measure=1)
    vb = sa.VBR().fill_from_CSR_inplace(m, eng.GetGrouping(m), 32, 32, True)
    h = np.diff(vb.row_part)
    assert len(vb.jab) == 21910 and vb.block_rows == 1952 and h.max() <= 32
    steps = slots = groups = 0
    off = 0
    for ib in range(vb.block_rows):
        nb, hh = int(vb.nzcount[ib]), int(h[ib])
        blk = vb.mab[off:off + nb * 32 * hh].reshape(nb, 8, 4 * hh)       # block, group of four columns, (column, row)
        off += nb * 32 * hh
        bits = (blk != 0).any(axis=2)
        masks = (bits * (1 << np.arange(8))).sum(1).astype(np.uint8)
        step, slot0, n = pack(masks)
        cnt = popcount(masks)
        steps += n
        groups += int(cnt.sum())
        slots += sum(int((slot0[step == s] + cnt[step == s]).max()) for s in range(n))
    assert steps <= 17300, steps
    assert slots == groups == 132262, (slots, groups)
