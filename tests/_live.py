"""Shared by tests/test_live_host.py and tests/test_live_gpu.py: the geometries, the masks and a numpy restatement of the rule of the live-block set
(include/sparta_amd.h, sparta_vbs_set_live_blocks)."""
import functools

import numpy as np

import _util as U

TRAIN_KEYS = ("w3", "w13h1", "w48", "w100h200", "w200", "w13z")
MASKS = ("all", "none", "second", "one_per_row", "row_dead", "col_dead", "rand50", "rand90")


def _small():
    """3 x 5, w 4: heights 1 and 2, both block columns stored, the second ragged (one column) -- the geometry of tests/test_prune_gpu.py"""
    a = U._edge_arrays(3, 5, 4, [1, 2], [[0, 1], [0, 1]])
    return U.sa_vbr(a, U._edge_values(a, "real", 7290))


def _zrows():
    """10 x 40, w 16: heights 4, 0, 6, 0 with blocks IN the block-rows of height 0 -- the geometry of tests/test_prune_gpu.py"""
    a = U._edge_arrays(10, 40, 16, [4, 0, 6, 0], [[0, 2], [1, 2], [2], [0]])
    return U.sa_vbr(a, U._edge_values(a, "real", 7291))


@functools.lru_cache(maxsize=None)
def geometry(key):
    if key == "small":
        return _small()
    if key == "zrows":
        return _zrows()
    if key in U.TRAIN_F32 or key in U.TRAIN_H16:
        return U.train_geometries()[key]
    if key in U.POISON_F32:
        return U.poison_geometries()[key]
    return U.edge_geometries("real")[key]


F32_CASES = [(k, None) for k in U.EDGE_F32 + TRAIN_KEYS + ("small", "zrows")] + [("heights", (3, 9))]


def case_id(case):
    return case[0] + ("" if case[1] is None else "-range")


@functools.lru_cache(maxsize=None)
def table(key, br=None):
    T = geometry(key).block_table(br)
    T.setflags(write=False)
    return T


@functools.lru_cache(maxsize=None)
def mask(key, br, name):
    """keep[n_blocks] (uint8, read-only): the named mask on the blocks of the range, numbered as block_table numbers them"""
    T = table(key, br)
    n = len(T)
    brow, bcol = T[:, 3] >> 32, T[:, 3] & 0xffffffff
    keep = np.ones(n, np.uint8)
    if name == "none":
        keep[:] = 0
    elif name == "second":
        keep[1::2] = 0
    elif name == "one_per_row":                       # the first block of every block-row
        keep[:] = 0
        keep[np.unique(brow, return_index=True)[1]] = 1
    elif name == "row_dead" and n:                    # the block-row with most blocks
        keep[brow == np.bincount(brow).argmax()] = 0
    elif name == "col_dead" and n:                    # the block column with most blocks
        keep[bcol == np.bincount(bcol).argmax()] = 0
    elif name in ("rand50", "rand90"):
        rng = np.random.default_rng(9300 + n + int(name[4:]))
        keep[rng.random(n) < int(name[4:]) / 100.0] = 0
    keep.setflags(write=False)
    return keep


def rule(v, keep, br=None):
    """The rule, restated: (sd_groups, sd_count, t_blocks, t_count) for the block-rows br of v.
    SDDMM: block-row ib has nb * w stored columns in mab order; group g is columns 32 g .. 32 g + 31 of them and overlaps blocks 32 g // w ..
    min(32 g + 31, nb w - 1) // w; it is live iff one of those is.  A block-row of height 0 has no groups.  The block-row's slice holds the live group numbers,
    ascending, then -1.  spmm_t: the list of block column j is its blocks of height > 0 in block-row order; its slice holds the numbers of the live ones in
    that order, then -1."""
    b0, b1 = (0, v.block_rows) if br is None else br
    w, cols = int(v.block_col_size), int(v.cols)
    nz = [int(x) for x in v.nzcount[b0:b1]]
    hts = [int(v.row_part[ib + 1] - v.row_part[ib]) for ib in range(b0, b1)]
    jab = [int(x) for x in v.jab[int(np.sum(v.nzcount[:b0])):int(np.sum(v.nzcount[:b1]))]]
    sd_groups, sd_count, first = [], [], 0
    per_col = [[] for _ in range((cols - 1) // w + 1)]
    for nb, h in zip(nz, hts):
        ng = (nb * w + 31) // 32 if h > 0 else 0
        live = [g for g in range(ng) if any(keep[first + b] for b in range(32 * g // w, min(32 * g + 31, nb * w - 1) // w + 1))]
        sd_groups += live + [-1] * (ng - len(live))
        sd_count.append(len(live))
        if h > 0:
            for b in range(nb):
                per_col[jab[first + b]].append(first + b)
        first += nb
    t_blocks, t_count = [], []
    for lst in per_col:
        live = [b for b in lst if keep[b]]
        t_blocks += live + [-1] * (len(lst) - len(live))
        t_count.append(len(live))
    return tuple(np.array(a, np.int32) for a in (sd_groups, sd_count, t_blocks, t_count))


def element_keep(T, keep):
    """per element of the range's mab: 1 where its block is live (all n_all elements of a block)"""
    return np.repeat(np.asarray(keep, np.uint8), T[:, 2]).astype(bool)
