"""The case builder of the device-resident track manager (tests/resident_tracks_cases.py) against its own conditions: every rebuilt
quirk takes the restatement's branch in the frame meant for it, every baseline decision stays clear of its threshold, and the scripted
sequence, as a case, still takes every branch the restatement counts.  CPU only."""
import numpy as np
import pytest

import resident_tracks_cases as rc
import track_manager_cases as tc
from test_track_manager_np import MULTI, SINGLE

CASES = rc.all_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_builders_conditions_hold(name):
    rc.check_case(CASES[name])


def test_every_quirk_states_the_branch_it_is_about():
    for name, case in rc.quirk_cases().items():
        assert case["expect"], name


def test_the_sequence_as_a_case_takes_every_branch():
    single = rc.check_case(CASES["sequence_single"]).mgr
    assert [b for b in SINGLE if single.branches[b] == 0] == []
    multi = rc.check_case(CASES["sequence_multi_uav"]).mgr
    assert [b for b in MULTI + [b for b in SINGLE if not b.startswith("dead_short")] if multi.branches[b] == 0] == []
    ref = tc.run_sequence(False)
    assert dict(single.branches) == dict(ref.branches) and [t.id for t in single.opp] == [t.id for t in ref.opp]
    assert dict(multi.branches) == dict(tc.run_sequence(True).branches)


def test_the_duplicate_cases_contest_a_claim_on_both_sides():
    for (i, j) in ((0, 1), (63, 64), (64, 200)):
        case = CASES["duplicate_%d_%d" % (i, j)]
        second, fourth = case["frames"][1]["matches"], case["frames"][3]["matches"]
        assert (second[i][0].x, second[i][0].y) == (second[j][0].x, second[j][0].y)
        assert (fourth[i][0].x, fourth[i][0].y) == (fourth[j][0].x, fourth[j][0].y)
        r = rc.check_case(case)
        assert len(r.mgr.slam) == 257 and all(len(t) == 5 for t in r.mgr.slam)     # every track was continued: both duplicates found a partner


def test_the_ring_case_passes_the_ring():
    r = rc.check_case(CASES["ring_70_frames"])
    assert [len(t) for t in r.mgr.slam] == [70] and r.own_list(0)["obs"].shape == (1, 64, 4)
    assert r.own_list(0)["obs"][0, 0, 0] == r.mgr.slam[0][6].x


def test_the_bounded_tile_loops_equal_the_restatements_inside_the_image():
    grid = CASES["sequence_single"] and rc.Runner(CASES["sequence_single"]).grid
    rng = np.random.default_rng(3)
    for x, y in zip(rng.uniform(0, tc.WIDTH, 200), rng.uniform(0, tc.HEIGHT, 200)):
        f, g = rc.tm.Feat(x, y), rc.tm.Feat(x, y)
        grid.set_tile(f)
        rc.set_tile_bounded(grid, g)
        assert (f.row, f.col) == (g.row, g.col)


def test_the_edge_cases_keep_their_sizes():
    for n, o in ((0, 0), (1, 63), (65, 64), (257, 257), (63, 257)):
        r = rc.check_case(rc.edge_case(n, o))
        assert len(r.mgr.opp) == n and r.mgr.branches["opp_extended"] == min(n, o)
