"""The track manager's restatement (tests/track_manager_np.py) on hand-worked cases that fix the quirks of
TrackManager::manageTracks (track_manager.cpp:115-432) one by one, the scripted sequence's branch coverage, and the facet
search's definition.  CPU only: what the device and the C++ mirror are compared with in test_gpu_track_*.py."""
import itertools
import math
import os
import re
from fractions import Fraction

import pytest

import track_manager_cases as tc
import track_manager_np as tm

ROOT = os.path.join(os.path.dirname(__file__), "..")
IDENT = [[0.0, 0.0, 0.0, 1.0]] * 6           # no rotation: the baseline is the extent of the normalised pixels
N, MIN_LEN = 6, 3
B0, B1, B2, B3 = (100.0, 100.0), (500.0, 100.0), (100.0, 400.0), (500.0, 400.0)    # one point in each tile of a 2 x 2 grid


def track(tid, end, n, dx=0.0, dy=0.0):
    """A track of n observations ending at `end`, moving (dx, dy) pixels a frame."""
    t = tm.Trk(tm.Feat(end[0] - (n - 1 - i) * dx, end[1] - (n - 1 - i) * dy) for i in range(n))
    t.id = tid
    return t


def extend(trk, dx=0.0, dy=0.0, score=0.0):
    """The match that continues trk."""
    last = trk[-1]
    return [last.copy(), tm.Feat(last.x + dx, last.y + dy, score=score)]


def manager(slam=(), opp=(), multi_uav=False):
    m = tm.TrackManagerNp(tc.K, 0.05, 0.05, multi_uav)
    m.slam, m.opp = list(slam), list(opp)
    m.next_id = 100
    return m


def manage(m, matches, n_slam_max=4):
    m.manage(matches, IDENT, N, n_slam_max, MIN_LEN, tm.TileGridNp(tc.WIDTH, tc.HEIGHT, 2, 2))
    return m


def ids(tracks):
    return [t.id for t in tracks]


def test_nearly_equal_is_relative_at_machine_epsilon():
    a = 123.456
    assert tm.nearly_equal(a, a) and tm.nearly_equal(a, math.nextafter(a, math.inf)) and tm.nearly_equal(math.inf, math.inf)
    assert not tm.nearly_equal(a, a * (1 + 8 * tm.EPS)) and not tm.nearly_equal(0.0, 1e-300) and tm.nearly_equal(0.0, -0.0)


def test_tiles_of_the_four_points():
    g = tm.TileGridNp(tc.WIDTH, tc.HEIGHT, 2, 2)
    got = []
    for p in (B0, B1, B2, B3):
        f = tm.Feat(*p)
        g.set_tile(f)
        got.append(f.row * 2 + f.col)
    assert got == [0, 1, 2, 3]


def test_two_persistent_tracks_lost_in_one_frame_report_pre_deletion_indices():
    slam = [track(i + 1, B0, 4) for i in range(5)]
    for i, t in enumerate(slam):
        t[-1].x += 10.0 * i                                # distinct last observations
    m = manage(manager(slam), [extend(slam[0]), extend(slam[2]), extend(slam[4])], n_slam_max=5)
    assert m.lost == [1, 3] and ids(m.slam) == [1, 3, 5] and all(len(t) == 5 for t in m.slam)


def test_first_equal_match_wins_and_a_claimed_match_leaves_the_list():
    s = track(1, B0, 3)
    o = track(2, B0, 2)                                   # an opportunistic track ending at the same pixel
    first, second = extend(s, dx=1.0), extend(s, dx=2.0)
    m = manage(manager([s], [o]), [first, second], n_slam_max=1)
    assert m.slam[0][-1].x == B0[0] + 1.0                 # the persistent track took the first
    assert ids(m.opp) == [2] and m.opp[0][-1].x == B0[0] + 2.0 and len(m.opp[0]) == 3     # the second was left for the other


def test_eviction_of_an_existing_persistent_track():
    slam = [track(i + 1, (B0[0] + 10.0 * i, B0[1]), 4) for i in range(4)]
    cand = track(9, B3, 2)
    m = manage(manager(slam, [cand]), [extend(t) for t in slam] + [extend(cand)])
    # tile 0 holds 4, the candidate's tile 0: the youngest of tile 0 is persistent track 3, reported lost by its index
    assert m.lost == [3] and ids(m.slam) == [1, 2, 3] and ids(m.new_slam) == [9] and m.opp == []
    assert m.branches["evict_existing"] == 1 and m.branches["evict_new"] == 0


def test_eviction_of_a_new_persistent_track():
    slam = [track(i + 1, (B0[0] + 10.0 * i, B0[1]), 4) for i in range(2)]
    a, b, c = track(7, (B0[0] + 50.0, B0[1]), 3), track(8, (B0[0] + 60.0, B0[1]), 3), track(9, B3, 2)
    m = manage(manager(slam, [a, b, c]), [extend(t) for t in slam + [a, b, c]])
    # a and b (longer, so first) take the two free slots in tile 0, which then holds 4; c's tile holds none: b, the youngest of
    # tile 0, is a NEW persistent track and disappears altogether -- it is in no list afterwards
    assert m.lost == [] and ids(m.slam) == [1, 2] and sorted(ids(m.new_slam)) == [7, 9] and m.opp == []
    assert m.branches["evict_new"] == 1 and m.branches["evict_existing"] == 0


def test_index_shift_after_an_eviction():
    slam = [track(1, B0, 4), track(2, (B0[0] + 10.0, B0[1]), 4), track(3, (B0[0] + 20.0, B0[1]), 4), track(4, B1, 4)]
    c1, c2 = track(8, B3, 3), track(9, B2, 2)
    m = manage(manager(slam, [c1, c2]), [extend(t) for t in slam + [c1, c2]])
    # c1 evicts persistent track 2 (tile 0 holds 3 against 0); the indices above it move down.  Then tile 0 holds 2 against c2's
    # 0: track 1 (pre-deletion index 1) goes as well
    assert m.lost == [2, 1] and ids(m.slam) == [1, 4] and ids(m.new_slam) == [8, 9]


def test_no_eviction_at_a_tile_difference_of_exactly_one():
    slam = [track(1, B0, 4), track(2, (B0[0] + 10.0, B0[1]), 4), track(3, B1, 4), track(4, B2, 4)]
    cand = track(9, (B1[0] + 10.0, B1[1]), 2)
    m = manage(manager(slam, [cand]), [extend(t) for t in slam + [cand]])
    assert m.lost == [] and ids(m.slam) == [1, 2, 3, 4] and m.new_slam == [] and ids(m.opp) == [9]
    assert m.branches["no_evict_at_difference_one"] == 1 and m.branches["long_enough_waits"] == 1


@pytest.mark.parametrize("dx, kept", [(10.0, True), (1.0, False)])
def test_an_over_long_track_leaves_with_and_without_baseline(dx, kept):
    slam = [track(i + 1, p, 4) for i, p in enumerate((B0, B1, B2, B3))]
    long = track(9, (B0[0] + 60.0, B0[1]), 6, dx=dx)        # 7 observations after this frame, the window holds 6
    m = manage(manager(slam, [long]), [extend(t) for t in slam] + [extend(long, dx=dx)])
    assert m.opp == [] and m.new_slam == [] and m.lost == []
    if kept:                                               # 5 steps of 10 px over fx = 400: 0.125 > 0.05
        assert ids(m.msckf_n) == [9] and len(m.msckf_n[0]) == 6
        assert m.msckf_n[0][-1] == ((long[-1].x - tc.K[2]) / tc.K[0], (long[-1].y - tc.K[3]) / tc.K[1])
    else:                                                  # 5 px: 0.0125
        assert m.msckf_n == []


@pytest.mark.parametrize("dy, kept", [(30.0, True), (3.0, False)])
def test_a_dead_two_observation_track_against_the_short_list(dy, kept):
    dead = track(5, B0, 2, dy=dy)
    m = manage(manager([], [dead]), [])
    assert m.opp == [] and m.msckf_n == []
    assert ids(m.msckf_short_n) == ([5] if kept else []) and (not kept or len(m.msckf_short_n[0]) == 2)


def test_a_dead_track_longer_than_the_short_list_is_cropped_to_it():
    dead = track(5, B0, 7, dx=10.0)
    m = manage(manager([], [dead]), [])
    assert len(m.msckf_short_n[0]) == N - 1


def test_multi_uav_dead_tracks_by_id_without_baseline():
    a, b, c = track(5, B0, 3), track(6, B1, 2), track(7, B2, 4)          # none moves: no baseline would pass
    m = manager([], [a, b, c], multi_uav=True)
    m.opp_ids = [6, 5, 42]
    manage(m, [])
    assert ids(m.msckf_short_n) == [5] and m.opp_ids == []               # 6 is too short, 7 is not listed; the list is cleared
    assert m.branches["multi_dead_matched"] == 1 and m.branches["multi_dead_too_short"] == 1 and m.branches["multi_dead_unmatched"] == 1


def test_new_slam_tracks_msckf_slam_before_standard():
    still, moving = track(5, B0, 3), track(6, B1, 2, dx=15.0)
    m = manage(manager([], [still, moving]), [extend(still), extend(moving, dx=15.0)])
    assert ids(m.new_slam_std_n) == [5] and ids(m.new_slam_msckf_n) == [6]
    assert ids(m.new_slam) == [6, 5]                                     # promoted as 5, 6; reordered MSCKF-SLAM first
    assert m.branches["new_slam_reordered"] == 1
    manage(m, [extend(m.new_slam[0]), extend(m.new_slam[1])])
    assert ids(m.slam) == [6, 5] and [len(t) for t in m.normalize_slam_tracks(N)] == [4, 5]


def test_equal_lengths_keep_their_match_order():
    a, b, c, d = track(1, B0, 1), track(2, B1, 2), track(3, B2, 1), track(4, B3, 2)
    m = manage(manager([], [a, b, c, d]), [extend(t) for t in (a, b, c, d)], n_slam_max=0)
    assert [len(t) for t in m.opp] == [3, 3, 2, 2] and ids(m.opp) == [2, 4, 1, 3]


def test_an_unmatched_match_starts_a_two_observation_track_with_a_fresh_id():
    m = manage(manager(), [[tm.Feat(*B0), tm.Feat(B0[0] + 1, B0[1])], [tm.Feat(*B1), tm.Feat(B1[0] + 1, B1[1])]])
    assert ids(m.opp) == [100, 101] and [len(t) for t in m.opp] == [2, 2]


SINGLE = ["slam_extended", "slam_lost", "slam_lost_two_in_a_frame", "opp_extended", "opp_new", "dead_short_pass", "dead_short_fail",
          "sort_moved_past_equal_lengths", "promote_free_slot", "evict_new", "evict_existing", "no_evict_at_difference_one",
          "overlong_pass", "overlong_fail", "long_enough_waits", "too_short_waits", "new_slam_msckf", "new_slam_std", "new_slam_reordered"]
MULTI = ["multi_dead_matched", "multi_dead_too_short", "multi_dead_unmatched"]


def test_the_scripted_sequence_takes_every_branch():
    m = tc.run_sequence(False)
    assert [b for b in SINGLE if m.branches[b] == 0] == []
    mm = tc.run_sequence(True)
    assert [b for b in MULTI + [b for b in SINGLE if not b.startswith("dead_short")] if mm.branches[b] == 0] == []
    assert len(tc.sequence()) == tc.SEQ["n_frames"] - 1


def test_ids_are_unique_over_the_sequence():
    seen = set()

    def on_frame(i, fr, m):
        now = ids(m.slam) + ids(m.new_slam) + ids(m.opp)
        assert len(now) == len(set(now))
        seen.update(now)

    tc.run_sequence(False, on_frame=on_frame)
    assert min(seen) == 1 and max(seen) == len(seen)


def test_baseline_special_values():
    """A NaN observation takes no part (the extent stays finite), an infinite rotated coordinate does (the flag is set), a NaN
    last observation -- where the reference starts -- gives a NaN extent on that axis."""
    c = tc.baseline_cases()["special_values"]
    _, norm, delta, flag = tm.baseline_batch(c["tracks"], c["drop_last"], c["quats"], tc.K, *c["min_baseline"])
    assert math.isnan(norm[1][0]) and all(math.isfinite(v) for v in delta[0])
    assert delta[1][0] == math.inf and flag[1] == 1
    assert math.isnan(delta[3][1])


def test_min_and_max_equal_the_reference_chain():
    """The kernel's plain minimum and maximum against the restatement's literal `if ... else if`."""
    for c in tc.baseline_cases().values():
        for trk, drop in zip(c["tracks"], c["drop_last"]):
            ql = c["quats"][:len(c["quats"]) - drop]
            n = tm.normalize(tm.Trk(tm.Feat(u, v) for u, v in trk), tc.K, len(ql))
            if any(math.isnan(v) for p in n for v in p):
                continue
            cn = tm._qnorm(ql[-1])
            xs, ys = [n[-1][0]], [n[-1][1]]
            for j, (x, y) in enumerate(n):
                ci = tm._qnorm(ql[len(ql) - len(n) + j])
                q = tm._qmul((ci[0], -ci[1], -ci[2], -ci[3]), cn)
                r = tm._qmul(tm._qmul((q[0], -q[1], -q[2], -q[3]), (0.0, x, y, 1.0)), q)
                xs.append(tm._div(r[1], r[3]))
                ys.append(tm._div(r[2], r[3]))
            assert (max(xs) - min(xs), max(ys) - min(ys)) == tm.baseline_delta(n, ql)


# ---- the facet ------------------------------------------------------------------------------------------------------------------
FACETS = tc.facet_cases()


@pytest.mark.parametrize("name", sorted(FACETS))
def test_facet_cases(name):
    c = FACETS[name]
    assert tm.facet(c["points"], c["query"], tc.WIDTH, tc.HEIGHT) == c["expect"]


def test_facet_expectations_by_hand():
    assert FACETS["one_triangle"]["expect"] == [0, 1, 2]
    for name in ("outside_hull", "hull_triangle_outer_vertex", "outside_rectangle", "two_tracks"):
        assert FACETS[name]["expect"] == []


def test_twelve_points_against_the_exact_delaunay_property():
    c = FACETS["twelve_points"]
    pts = tm.facet_points(c["points"], tc.WIDTH, tc.HEIGHT)
    p = (Fraction(tm.f32(c["query"][0])), Fraction(tm.f32(c["query"][1])))
    i, j, k = c["expect"]
    a, b, cc = pts[i], pts[j], pts[k]
    if tm.orient(a, b, cc) < 0:
        b, cc = cc, b
    assert tm.orient(a, b, p) > 0 and tm.orient(b, cc, p) > 0 and tm.orient(cc, a, p) > 0           # strictly inside
    assert all(tm.in_circle(a, b, cc, pts[l]) < 0 for l in range(len(pts)) if l not in (i, j, k))   # an empty circumcircle
    # and it is the only such triangle: the triangulation of points in general position is unique
    others = [t for t in itertools.combinations(range(len(pts)), 3) if t != (i, j, k) and tm.orient(*(pts[v] for v in t)) != 0]
    for t in others:
        u, v, w = (pts[q] for q in t)
        if tm.orient(u, v, w) < 0:
            v, w = w, v
        inside = tm.orient(u, v, p) >= 0 and tm.orient(v, w, p) >= 0 and tm.orient(w, u, p) >= 0
        empty = all(tm.in_circle(u, v, w, pts[l]) <= 0 for l in range(len(pts)) if l not in t)
        assert not (inside and empty)


def test_outer_vertices_are_the_documented_ones():
    pts = tm.facet_points([], 640, 480)
    assert pts == [(1925, -1), (-1, 1925), (-1927, -1927)]


def test_the_new_symbols_are_declared_and_listed():
    from x_multi_agent_amd import engine
    header = open(os.path.join(ROOT, "include", "xk.h")).read()
    for s in ("xk_trk_baseline_setup", "xk_trk_baseline"):
        assert s in engine.SYMBOLS and re.search(r"\bint %s\(" % s, header)
