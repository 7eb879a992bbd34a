"""Shared by tests/test_live_forward_host.py and tests/test_live_forward_gpu.py: a Python restatement of the rule of the live forward product
(include/sparta_amd.h, sparta_vbs_set_live_forward), hand-written record arrays, and the invariants every output of the rule must satisfy."""
import numpy as np

from sparta_amd.host import STEP_DTYPE, STEP_FIRST, STEP_LAST, STEP_SPLIT, STEP_TAIL, STEP_LO_ABSENT, STEP_HI_ABSENT

EDGE = STEP_FIRST | STEP_LAST | STEP_SPLIT


def segments(steps, b, e):
    """the (first, last) positions of the segments of the range [b, e): a segment ends at a STEP_LAST record or at the end of the range"""
    out, q = [], b
    while q < e:
        sl = q
        while sl < e - 1 and not int(steps["mt_flags"][sl]) & STEP_LAST:
            sl += 1
        out.append((q, sl))
        q = sl + 1
    return out


def halves(steps, live, pair, s):
    """(rows 0..31 live, rows 32..63 live) of step s: a half counts where it is present"""
    f = int(steps["mt_flags"][s])
    if not pair:
        return bool(live[s][0]), False
    return bool(live[s][0]) and not f & STEP_LO_ABSENT, bool(live[s][1]) and not f & STEP_HI_ABSENT


def rule(steps, ranges, pair, live):
    """The rule, restated: (steps_out, ranges_out).  Per range the kept steps first and in order (every live step; the first step of a segment that has none),
    then the dropped steps unchanged and in order.  A kept record: STEP_FIRST / STEP_LAST say where it stands among the kept steps of its segment, the last
    one takes STEP_SPLIT, c_row, slot and the tile rows of the segment's last record, a half that is not live gets its absent flag (one-tile records: the
    lower flag for the whole step)."""
    steps = np.asarray(steps, STEP_DTYPE)
    live = np.asarray(live, np.uint8).reshape(-1, 2)
    ranges = np.asarray(ranges, np.int32).reshape(-1, 2)
    out, r_out = steps.copy(), np.zeros_like(ranges)
    for r, (b, e) in enumerate(ranges):
        kept, dropped = [], []
        for first, last in segments(steps, b, e):
            alive = [s for s in range(first, last + 1) if any(halves(steps, live, pair, s))]
            keepers = alive or [first]
            for s in range(first, last + 1):
                rec = steps[s].copy()
                if s not in keepers:
                    dropped.append(rec)
                    continue
                f = int(rec["mt_flags"]) & ~EDGE
                if s == keepers[0]:
                    f |= STEP_FIRST
                if s == keepers[-1]:
                    fl = int(steps["mt_flags"][last])
                    f = (f & ~0xffff) | (fl & 0xffff) | STEP_LAST | (fl & STEP_SPLIT)
                    rec["c_row"], rec["slot"] = steps["c_row"][last], steps["slot"][last]
                lo, hi = halves(steps, live, pair, s)
                if not lo:
                    f |= STEP_LO_ABSENT
                if pair and not hi:
                    f |= STEP_HI_ABSENT
                rec["mt_flags"] = f
                kept.append(rec)
        for i, rec in enumerate(kept + dropped):
            out[b + i] = rec
        r_out[r] = (b, b + len(kept))
    return out, r_out


def check_invariants(steps, ranges, pair, live, out, r_out):
    """what must hold of any output of the rule"""
    steps, out = np.asarray(steps, STEP_DTYPE), np.asarray(out, STEP_DTYPE)
    live = np.asarray(live, np.uint8).reshape(-1, 2)
    inside = np.zeros(len(steps), bool)
    for (b, e), (lb, le) in zip(np.asarray(ranges).reshape(-1, 2), np.asarray(r_out).reshape(-1, 2)):
        inside[b:e] = True
        assert lb == b and b <= le <= max(b, e)
        # a permutation of the input positions: a_off names the position (the test arrays give every step its own), the rest of a record may be edited
        assert sorted(out["a_off"][b:e].tolist()) == sorted(steps["a_off"][b:e].tolist())
        pos = {int(a): s for s, a in zip(range(b, e), steps["a_off"][b:e])}
        src = [pos[int(a)] for a in out["a_off"][b:e]]
        k = le - lb
        assert src[:k] == sorted(src[:k]) and src[k:] == sorted(src[k:]), "kept and dropped steps stay in order"
        assert all((out[b + i] == steps[s]) for i, s in enumerate(src) if i >= k), "dropped steps are unchanged"
        kept_of = {}
        for i in range(k):
            first = next(f for f, l in segments(steps, b, e) if f <= src[i] <= l)
            kept_of.setdefault(first, []).append(b + i)
        segs = segments(steps, b, e)
        assert sorted(kept_of) == [f for f, _ in segs], "every segment keeps at least one step"
        for first, last in segs:
            mine = kept_of[first]
            flags = [int(out["mt_flags"][i]) for i in mine]
            assert [bool(f & STEP_FIRST) for f in flags] == [True] + [False] * (len(mine) - 1)
            assert [bool(f & STEP_LAST) for f in flags] == [False] * (len(mine) - 1) + [True]
            end, fl = out[mine[-1]], int(steps["mt_flags"][last])
            assert (int(end["mt_flags"]) & (0xffff | STEP_SPLIT)) == (fl & (0xffff | STEP_SPLIT)) and end["c_row"] == steps["c_row"][last] and end["slot"] == steps["slot"][last]
            assert not any(f & STEP_SPLIT for f in flags[:-1])
            alive = [s for s in range(first, last + 1) if any(halves(steps, live, pair, s))]
            assert [src[i - b] for i in mine] == (alive or [first])
            for i in mine:
                s, f = src[i - b], int(out["mt_flags"][i])
                lo, hi = halves(steps, live, pair, s)
                assert bool(f & STEP_LO_ABSENT) == (not lo) and bool(f & STEP_HI_ABSENT) == (pair and not hi)
                assert (f & STEP_TAIL) == (int(steps["mt_flags"][s]) & STEP_TAIL)
                assert all(out[n][i] == steps[n][s] for n in ("a_off", "b_row", "h", "pad"))
    assert (out[~inside] == steps[~inside]).all(), "records outside the ranges are copied"


def make(tiles, pair=False, cuts=()):
    """Hand-written records.  tiles: per tile a list of steps, each "L" (live), "D" (dead), or for pair tiles two letters for rows 0..31 / 32..63 out of L, D
    and "-" (absent); cuts: positions where a range ends (a tile cut there is split: both pieces end in STEP_LAST | STEP_SPLIT with their own slot).
    Returns (steps, ranges, live)."""
    n = sum(len(t) for t in tiles)
    steps, live = np.zeros(n, STEP_DTYPE), np.zeros((n, 2), np.uint8)
    bounds = [0] + sorted(set(c for c in cuts if 0 <= c <= n)) + [n]
    ranges = np.array([(bounds[i], bounds[i + 1]) for i in range(len(bounds) - 1)], np.int32).reshape(-1, 2)
    q, slot = 0, 0
    for t, tile in enumerate(tiles):
        t0, t1 = q, q + len(tile)
        inner = [c for c in bounds if t0 < c < t1]
        for i, s in enumerate(tile):
            f = (40 if pair else 17 + t % 16)
            if q == t0 or q in inner:
                f |= STEP_FIRST
            if q == t1 - 1 or q + 1 in inner:
                f |= STEP_LAST
                if inner:
                    f |= STEP_SPLIT
            if i % 5 == 4:
                f |= STEP_TAIL
            lo, hi = (s[0], s[1]) if pair else (s, s)
            if pair and lo == "-":
                f |= STEP_LO_ABSENT
            if pair and hi == "-":
                f |= STEP_HI_ABSENT
            live[q] = (lo == "L", hi == "L")
            steps[q] = (2048 * q + 64, 32 * (7 * q % 11), 32 + t, 64 * t, f, slot if f & STEP_SPLIT else -1, 0)
            slot += 1 if f & STEP_SPLIT else 0
            q += 1
    return steps, ranges, live


def hand_cases():
    """name -> (steps, ranges, pair, live)"""
    rng = np.random.default_rng(20261020)
    word = lambda n, p: ["L" if x else "D" for x in rng.random(n) < p]  # noqa: E731
    pairs = ["LL", "LD", "DL", "DD", "L-", "-L", "D-", "-D"]
    out = {
        "all_live": make([list("LLL"), list("LL")]),
        "all_dead": make([list("DDD"), list("D"), list("DD")]),
        "dead_head": make([list("DDLL"), list("DL")]),
        "dead_tail": make([list("LLDD"), list("LD")]),
        "dead_middle": make([list("LDDL"), list("DLD")]),
        "split": make([list("LLDDLL"), list("DDDD"), list("LD")], cuts=(3, 8)),
        "split_dead_piece": make([list("LLDDDDLL")], cuts=(2, 6)),
        "ends_inside_tile": make([list("LDLD"), list("DDLL")], cuts=(6,)),
        "empty_range": make([list("LD")], cuts=(0, 2)),
        "pair_halves": make([["LL", "LD", "DL", "DD"], ["L-", "-L", "D-", "-D"], ["D-", "-D"], ["DD", "DL"]], pair=True),
        "pair_split": make([[pairs[i % 8] for i in range(11)], ["-D", "DD", "D-"]], pair=True, cuts=(4, 9)),
    }
    for n in (1, 63, 64, 65):
        for p in (0.0, 0.3, 1.0):
            out["one_segment_%d_%d" % (n, int(10 * p))] = make([word(n, p)])
        out["many_segments_%d" % n] = make([word(k, 0.4) for k in _cut(n, rng)])
    out["long_mixed"] = make([word(k, 0.25) for k in (130, 1, 2, 70, 64, 3)], cuts=(100, 200, 265))
    return {k: (v[0], v[1], k.startswith("pair"), v[2]) for k, v in out.items()}


def _cut(n, rng):
    """n steps in tiles of 1..9"""
    out = []
    while n > 0:
        k = min(n, int(rng.integers(1, 10)))
        out.append(k)
        n -= k
    return out
