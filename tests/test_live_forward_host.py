"""The rule of the live forward product on the host (no GPU): sparta_live_forward_compact against the Python restatement of tests/_live_forward.py on
hand-written record arrays -- segments that are all live, all dead, dead at the head, at the tail and in the middle, split tiles, a range that ends inside a
tile, pair tiles whose halves disagree or are absent, empty ranges, ranges of 1, 63, 64 and 65 steps -- and the invariants of its output."""
import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd.host import STEP_LAST, STEP_SPLIT, STEP_LO_ABSENT, STEP_HI_ABSENT

import _live_forward as LF

CASES = LF.hand_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_rule_equals_restatement(name):
    steps, ranges, pair, live = CASES[name]
    out, r_out, info = sa.live_forward_compact(steps, ranges, pair, live)
    want, r_want = LF.rule(steps, ranges, pair, live)
    assert np.array_equal(r_out, r_want)
    assert np.array_equal(out, want), np.flatnonzero(out != want)[:8]
    LF.check_invariants(steps, ranges, pair, live, out, r_out)
    kept = (r_out[:, 1] - r_out[:, 0])
    assert info["steps"] == len(steps) and info["kept"] == int(kept.sum())
    assert info["max_kept"] == int(kept.max()) and info["min_kept"] == int(kept.min())


def test_restatement_satisfies_invariants():
    for steps, ranges, pair, live in CASES.values():
        LF.check_invariants(steps, ranges, pair, live, *LF.rule(steps, ranges, pair, live))


def test_known_answers():
    """a few outputs written out by hand, so that the restatement and the library cannot be wrong in the same way"""
    steps, ranges, live = LF.make([list("DLDL"), list("DD")])
    out, r_out, info = sa.live_forward_compact(steps, ranges, False, live)
    assert r_out.tolist() == [[0, 3]] and info["segments"] == 2 and info["dead_segments"] == 1
    assert out["a_off"].tolist() == [steps["a_off"][i] for i in (1, 3, 4, 0, 2, 5)]
    f = out["mt_flags"]
    assert f[0] & sa.host.STEP_FIRST and not f[0] & STEP_LAST and f[1] & STEP_LAST and not f[1] & sa.host.STEP_FIRST
    assert f[2] & sa.host.STEP_FIRST and f[2] & STEP_LAST and f[2] & STEP_LO_ABSENT and not f[2] & STEP_HI_ABSENT
    assert (f[2] & 0xffff) == (steps["mt_flags"][5] & 0xffff) and not (f[0] | f[1]) & (STEP_LO_ABSENT | STEP_HI_ABSENT)
    assert (out[3:] == steps[[0, 2, 5]]).all()
    # pair tiles: the dead half of a kept step is marked absent, a step whose only present half is dead is dropped, an all-dead segment keeps its first step
    steps, ranges, live = LF.make([["LD", "D-", "-L"], ["DD", "-D"]], pair=True)
    out, r_out, _ = sa.live_forward_compact(steps, ranges, True, live)
    assert r_out.tolist() == [[0, 3]] and out["a_off"][:3].tolist() == [steps["a_off"][i] for i in (0, 2, 3)]
    both = STEP_LO_ABSENT | STEP_HI_ABSENT
    assert [int(x) & both for x in out["mt_flags"][:3]] == [STEP_HI_ABSENT, STEP_LO_ABSENT, both]


def test_segment_without_last_ends_at_the_range_end():
    steps, ranges, pair, live = CASES["ends_inside_tile"]
    steps = steps.copy()
    steps["mt_flags"][5] &= ~(STEP_LAST | STEP_SPLIT)
    out, r_out, _ = sa.live_forward_compact(steps, ranges, pair, live)
    want, r_want = LF.rule(steps, ranges, pair, live)
    assert np.array_equal(out, want) and np.array_equal(r_out, r_want)
    LF.check_invariants(steps, ranges, pair, live, out, r_out)


def test_bad_arguments():
    steps, ranges, pair, live = CASES["all_live"]
    with pytest.raises(ValueError):
        sa.live_forward_compact(steps, ranges, pair, live[:-1])
    with pytest.raises(sa.SpartaError):
        sa.live_forward_compact(steps, [[0, len(steps) + 1]], pair, live)
    with pytest.raises(sa.SpartaError):
        sa.live_forward_compact(steps, [[-1, 2]], pair, live)
    out, r_out, info = sa.live_forward_compact(steps[:0], np.zeros((0, 2), np.int32), pair, live[:0])
    assert len(out) == 0 and len(r_out) == 0 and info["kept"] == 0
