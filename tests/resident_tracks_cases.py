"""Cases of the device-resident track manager: scripted frame sequences that start from an empty store, the
restatement tests/track_manager_np.py::TrackManagerNp run beside them, and what of its state the device is compared with after every
frame.  The store has no entry that installs a track list, so every hand-worked quirk of tests/test_track_manager_np.py is REBUILT here
from frames: a few frames grow the tracks the quirk needs (a frame's n_slam_max and min_track_length decide who is promoted when), one
frame triggers it.  check_case asserts the builder's own conditions: the quirk's branch of the restatement was taken in the frame meant
for it, and every baseline decision is more than BASELINE_MARGIN from its threshold.

A case is a dict(multi_uav, tiles, max_tracks, frames, expect); a frame a dict(matches = [[previous Feat, current Feat]], cam_rots,
n_poses_max, n_slam_max, min_track_length, opp_ids or None) or dict(op = ("remove_persistent", idx) | ("remove_new_persistent", idxs) |
("clear",)).  Scores are whole numbers: the device holds them as the tracker's int."""
import math

import numpy as np

import track_manager_cases as tc
import track_manager_np as tm

RING = 64
N, MIN_LEN = 6, 3
B0, B1, B2, B3 = (100.0, 100.0), (500.0, 100.0), (100.0, 400.0), (500.0, 400.0)    # one point in each tile of a 2 x 2 grid


def ident(n):
    return [[0.0, 0.0, 0.0, 1.0] for _ in range(n)]


def set_tile_bounded(grid, f):
    """TiledImage::setTileForFeature with each loop bounded by its tile count, as the device runs it (the same tile for every feature
    inside the image; a NaN or infinite pixel ends where the kernel's loop does)."""
    c, col = f.xd - grid.tile_width - 0.5, 0
    for _ in range(grid.n_tiles_w + 1):
        if not c > 0:
            break
        col += 1
        c -= grid.tile_width
    r, row = grid.rows - f.yd - 0.5, grid.n_tiles_h - 1
    for _ in range(grid.n_tiles_h + 1):
        if not r > grid.tile_height:
            break
        row -= 1
        r -= grid.tile_height
    f.row, f.col = row, col


class Script:
    """Named features that move; a frame lists the ones matched, in match order."""

    def __init__(self, multi_uav=False, tiles=(2, 2), max_tracks=64):
        self.case = dict(multi_uav=multi_uav, tiles=tiles, max_tracks=max_tracks, frames=[], expect={})
        self.pos = {}

    def at(self, **named):
        self.pos.update(named)
        return self

    def frame(self, moves, n_slam_max, min_len=MIN_LEN, n_poses_max=N, rots=None, opp_ids=None, score=None):
        """moves: [(name, dx, dy)] or names (no motion)."""
        matches = []
        for i, mv in enumerate(moves):
            name, dx, dy = (mv, 0.0, 0.0) if isinstance(mv, str) else mv
            x, y = self.pos[name]
            s = float(score[i]) if score else 0.0
            matches.append([tm.Feat(x, y, score=s), tm.Feat(x + dx, y + dy, score=s)])
            self.pos[name] = (x + dx, y + dy)
        self.case["frames"].append(dict(matches=matches, cam_rots=ident(n_poses_max) if rots is None else rots, n_poses_max=n_poses_max,
                                        n_slam_max=n_slam_max, min_track_length=min_len, opp_ids=opp_ids))
        return self

    def op(self, *op):
        self.case["frames"].append(dict(op=op))
        return self

    def expect(self, **branches):
        """Branch counts of the restatement over the LAST frame added."""
        self.case["expect"][len(self.case["frames"]) - 1] = branches
        return self.case


# ---- the restatement beside the device ---------------------------------------------------------------------------------------------
class Runner:
    def __init__(self, case, K=tc.K, size=(tc.WIDTH, tc.HEIGHT), min_baseline=(0.05, 0.05)):
        self.case, self.K = case, K
        self.mgr = tm.TrackManagerNp(K, min_baseline[0], min_baseline[1], case["multi_uav"])
        self.grid = tm.TileGridNp(size[0], size[1], *case["tiles"])
        self.n_poses_max = N

    def step(self, frame):
        """One frame through the restatement -> claimed flags (None for an op)."""
        m = self.mgr
        if "op" in frame:
            op = frame["op"]
            if op[0] == "remove_persistent":
                del m.slam[op[1]]
            elif op[0] == "remove_new_persistent":
                for i in reversed(op[1]):
                    del m.new_slam[i]
            else:
                m.clear()
            return None
        pairs = [[p.copy(), c.copy()] for p, c in frame["matches"]]
        for p, _ in pairs:
            set_tile_bounded(self.grid, p)
        left = list(pairs)
        if self.case["multi_uav"]:
            m.opp_ids = list(frame["opp_ids"] or [])
        self.n_poses_max = frame["n_poses_max"]
        m.manage(left, frame["cam_rots"], frame["n_poses_max"], frame["n_slam_max"], frame["min_track_length"], self.grid)
        alive = {id(p) for p in left}
        return np.array([0 if id(p) in alive else 1 for p in pairs], np.uint8)

    def own_list(self, which):
        """What Klt.tracks_lists returns, from the restatement."""
        trks = (self.mgr.slam, self.mgr.new_slam, self.mgr.opp)[which]
        n = len(trks)
        out = dict(ids=np.array([t.id for t in trks], np.int64).reshape(n), lengths=np.array([len(t) for t in trks], np.int32).reshape(n),
                   obs=np.zeros((n, RING, 4)), score=np.zeros((n, RING), np.int32), tiles=np.zeros((n, RING, 2), np.int32))
        for i, t in enumerate(trks):
            for j, f in enumerate(t[-RING:]):
                out["obs"][i, j] = (f.x, f.y, f.xd, f.yd)
                out["score"][i, j] = int(f.score)
                out["tiles"][i, j] = (f.row, f.col)
        return out

    def measurement_lists(self):
        """The five lists in the order of XK_TRACKS_*: dicts of ids, off, xy."""
        m = self.mgr
        crop = min(self.n_poses_max, RING)
        lists = [m.msckf_n, m.msckf_short_n, m.new_slam_std_n, m.new_slam_msckf_n, [tm.normalize(t, self.K, crop) for t in m.slam]]
        out = []
        for lst in lists:
            off = np.zeros(len(lst) + 1, np.int32)
            off[1:] = np.cumsum([len(t) for t in lst])
            xy = np.array([p for t in lst for p in t], np.float64).reshape(-1, 2)
            out.append(dict(ids=np.array([t.id for t in lst], np.int64).reshape(len(lst)), off=off, xy=xy))
        return out


def same_bits(a, b):
    """Equal as bit patterns: NaN equals NaN, +0 differs from -0."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_case(case):
    """The builder's own conditions -> the restatement after the last frame."""
    r = Runner(case)
    for i, fr in enumerate(case["frames"]):
        before = dict(r.mgr.branches)
        r.step(fr)
        for b, count in case["expect"].get(i, {}).items():
            assert r.mgr.branches[b] - before.get(b, 0) == count, (i, b, r.mgr.branches[b] - before.get(b, 0))
    finite = [v for v in r.mgr.margins if math.isfinite(v)]
    assert not finite or min(finite) > tc.BASELINE_MARGIN, min(finite)
    return r


# ---- the hand-worked quirks, rebuilt ---------------------------------------------------------------------------------------------
def _grow_persistent(s, names, n_slam_max):
    """Three frames after which `names` are persistent tracks of 4 observations, in this order."""
    for _ in range(3):
        s.frame(names, n_slam_max)
    return s


def quirk_cases():
    c = {}
    # two persistent tracks lost in one frame report their indices before the deletions
    s = Script().at(**{"p%d" % i: (B0[0] + 10.0 * i, B0[1]) for i in range(5)})
    c["two_lost_in_one_frame"] = _grow_persistent(s, ["p%d" % i for i in range(5)], 5).frame(["p0", "p2", "p4"], 5).expect(
        slam_lost=2, slam_lost_two_in_a_frame=1, slam_extended=3)
    # the first equal match wins, and a claimed match leaves the list: the second goes to the opportunistic track ending at the same pixel
    s = _grow_persistent(Script().at(s=B0), ["s"], 1).at(o=(B0[0] - 1.0, B0[1])).frame(["s", ("o", 1.0, 0.0)], 1)
    s.pos["o"] = B0                                                   # (it is there already: the two matches below have one previous feature)
    c["first_equal_match_wins"] = s.frame([("s", 1.0, 0.0), ("o", 2.0, 0.0)], 1).expect(slam_extended=1, opp_extended=1, opp_new=0)
    # eviction of an existing persistent track: tile 0 holds 4, the candidate's tile none
    four = ["p%d" % i for i in range(4)]
    s = _grow_persistent(Script().at(**{"p%d" % i: (B0[0] + 10.0 * i, B0[1]) for i in range(4)}), four, 4).at(cand=B3)
    c["evict_existing"] = s.frame(four + ["cand"], 4).frame(four + ["cand"], 4).expect(evict_existing=1, evict_new=0)
    # eviction of a new persistent track: it is in no list afterwards
    s = _grow_persistent(Script().at(p0=B0, p1=(B0[0] + 10.0, B0[1])), ["p0", "p1"], 2)
    s.at(a=(B0[0] + 50.0, B0[1]), b=(B0[0] + 60.0, B0[1]), cc=B3)
    every = ["p0", "p1", "a", "b", "cc"]
    c["evict_new"] = s.frame(every, 2).frame(every, 4).expect(promote_free_slot=2, evict_new=1, evict_existing=0)
    # the index shift after an eviction: the second eviction reports the index before the frame's deletions
    s = Script().at(p0=B0, p1=(B0[0] + 10.0, B0[1]), p2=(B0[0] + 20.0, B0[1]), p3=B1)
    s = _grow_persistent(s, four, 4).at(c1=B3, c2=B2)
    s.frame(four + ["c1"], 4, min_len=6).frame(four + ["c1", "c2"], 4, min_len=6)
    c["index_shift"] = s.frame(four + ["c1", "c2"], 4).expect(evict_existing=2)
    # no eviction at a tile difference of exactly one
    s = _grow_persistent(Script().at(p0=B0, p1=(B0[0] + 10.0, B0[1]), p2=B1, p3=B2), four, 4).at(cand=(B1[0] + 10.0, B1[1]))
    c["no_eviction_at_difference_one"] = s.frame(four + ["cand"], 4).frame(four + ["cand"], 4).expect(
        no_evict_at_difference_one=1, long_enough_waits=1, evict_existing=0, evict_new=0)
    # an over-long track leaves, with and without baseline; 7 observations cropped to the window's 6
    for name, dx, branch in (("overlong_with_baseline", 10.0, "overlong_pass"), ("overlong_without_baseline", 1.0, "overlong_fail")):
        s = _grow_persistent(Script().at(p0=B0, p1=B1, p2=B2, p3=B3), four, 4).at(long=(B0[0] + 10.0, B0[1]))
        for _ in range(5):
            s.frame(four + [("long", dx, 0.0)], 4, min_len=8, n_poses_max=8)
        c[name] = s.frame(four + [("long", dx, 0.0)], 4).expect(**{branch: 1})
    # a dead two-observation track against the short list
    for name, dy, branch in (("dead_two_observations_pass", 30.0, "dead_short_pass"), ("dead_two_observations_fail", 3.0, "dead_short_fail")):
        c[name] = Script().at(d=(B0[0], B0[1] - dy)).frame([("d", 0.0, dy)], 0).frame([], 0).expect(**{branch: 1})
    # a dead track longer than the short list is cropped to it
    s = Script().at(d=B0)
    for _ in range(6):
        s.frame([("d", 10.0, 0.0)], 0, min_len=8, n_poses_max=8)
    c["dead_track_cropped"] = s.frame([], 0).expect(dead_short_pass=1)
    # multi_uav: dead tracks by id, no baseline check; ids 1, 2, 3 in the order the tracks start
    s = Script(multi_uav=True).at(c7=B2, a5=B0, b6=B1)
    s.frame(["c7"], 0, opp_ids=[]).frame(["c7", "a5"], 0, opp_ids=[]).frame(["c7", "a5", "b6"], 0, opp_ids=[])
    c["multi_uav_dead_by_id"] = s.frame([], 0, opp_ids=[3, 2, 42]).expect(multi_dead_matched=1, multi_dead_too_short=1, multi_dead_unmatched=1)
    # MSCKF-SLAM before standard, and the persistent list cropped in the frame after
    s = Script().at(still=B0, moving=B1).frame(["still"], 4).frame(["still", ("moving", 15.0, 0.0)], 4, min_len=6)
    s.frame(["still", ("moving", 15.0, 0.0)], 4).expect(new_slam_reordered=1, new_slam_msckf=1, new_slam_std=1)
    c["msckf_slam_before_standard"] = s.frame(["still", ("moving", 15.0, 0.0)], 4).expect(slam_extended=2)
    # equal lengths keep their match order
    s = Script().at(a=B0, b=B1, cc=B2, d=B3).frame(["b", "d"], 0)
    c["equal_lengths_keep_match_order"] = s.frame(["a", "cc", "b", "d"], 0).expect(sort_moved_past_equal_lengths=1)
    # an unmatched match starts a two-observation track with a fresh id
    c["unmatched_match_fresh_id"] = Script().at(a=B0, b=B1).frame([("a", 1.0, 0.0)], 4).frame([("a", 1.0, 0.0), ("b", 1.0, 0.0)], 4).expect(
        opp_new=1, opp_extended=1)
    return c


def sequence_case(multi_uav):
    """The scripted sequence of track_manager_cases (SEQ) as a case.  multi_uav: the caller upgrades, every frame, the six lowest ids
    among the opportunistic tracks of the frame before (run_sequence's rule)."""
    frames = []
    r = tm.TrackManagerNp(tc.K, tc.MIN_BASELINE[0], tc.MIN_BASELINE[1], multi_uav)
    grid = tm.TileGridNp(tc.WIDTH, tc.HEIGHT, *tc.SEQ["tiles"])
    for fr in tc.sequence(multi_uav):
        ids = sorted(t.id for t in r.opp)[:6] if multi_uav else None
        frames.append(dict(matches=fr["matches"], cam_rots=fr["cam_rots"], n_poses_max=tc.SEQ["n_poses_max"], n_slam_max=tc.SEQ["n_slam_max"],
                           min_track_length=tc.SEQ["min_track_length"], opp_ids=ids))
        r.opp_ids = list(ids or [])
        r.manage([[p.copy(), c.copy()] for p, c in fr["matches"]], fr["cam_rots"], tc.SEQ["n_poses_max"], tc.SEQ["n_slam_max"],
                 tc.SEQ["min_track_length"], grid)
    return dict(multi_uav=multi_uav, tiles=tc.SEQ["tiles"], max_tracks=64, frames=frames, expect={})


# ---- wavefront and workgroup edges ---------------------------------------------------------------------------------------------------
EDGE_SIZES = (0, 1, 63, 64, 65, 257)


def _spread(i):
    """Distinct pixels well inside the image, all tiles of a 2 x 2 grid."""
    return 20.0 + 2.25 * (i % 257), 30.0 + 1.5 * (i // 257) + 0.75 * (i % 200)


def edge_case(n_matches, n_opp):
    """n_opp opportunistic tracks, then a frame of n_matches matches: those that can continue a track do, in an order that is not the
    tracks', the rest start one.  Nothing is promoted (no slots), so both lists keep their sizes."""
    first = [[tm.Feat(*_spread(i), score=i % 7), tm.Feat(*_spread(10000 + i), score=i % 7)] for i in range(n_opp)]
    k = min(n_matches, n_opp)
    order = [(37 * j + 5) % n_opp for j in range(k)] if n_opp else []          # (37 is coprime to every size here)
    second = [[first[o][1].copy(), tm.Feat(*_spread(20000 + o), score=o % 7)] for o in order]
    second += [[tm.Feat(*_spread(30000 + j), score=1.0), tm.Feat(*_spread(40000 + j), score=1.0)] for j in range(n_matches - k)]
    fr = dict(cam_rots=ident(N), n_poses_max=N, n_slam_max=0, min_track_length=MIN_LEN, opp_ids=None)
    return dict(multi_uav=False, tiles=(2, 2), max_tracks=600, frames=[dict(fr, matches=first), dict(fr, matches=second)], expect={})


def duplicate_case(i, j, n=257):
    """n opportunistic tracks of which i and j end in the same feature, then n matches of which i and j have that previous feature:
    the contested claim.  Then the same with persistent tracks: the tracks are promoted and two matches continue tracks i and j."""
    shared = (333.25, 222.5)
    first = [[tm.Feat(*_spread(q)), tm.Feat(*(shared if q in (i, j) else _spread(10000 + q)))] for q in range(n)]
    second = [[first[q][1].copy(), tm.Feat(*_spread(20000 + q))] for q in range(n)]
    third = [[second[q][1].copy(), tm.Feat(*(shared if q in (i, j) else _spread(30000 + q)))] for q in range(n)]
    fourth = [[third[q][1].copy(), tm.Feat(*_spread(40000 + q))] for q in range(n)]
    fr = dict(cam_rots=ident(N), n_poses_max=N, min_track_length=MIN_LEN, opp_ids=None)
    # frames 1, 2: opportunistic (no slots); frame 3 promotes every track (n slots); frame 4: the persistent tracks claim
    return dict(multi_uav=False, tiles=(2, 2), max_tracks=600, expect={},
                frames=[dict(fr, matches=first, n_slam_max=0), dict(fr, matches=second, n_slam_max=0), dict(fr, matches=third, n_slam_max=n),
                        dict(fr, matches=fourth, n_slam_max=n)])


def special_value_cases():
    """NaN and +-inf x in a match's previous feature and in a track's last feature (the undistorted x: the tile comes from the
    distorted pixel, which stays inside the image), and an x of exactly 0 against 1e-320 (the denormal branch)."""
    c = {}
    fr = dict(cam_rots=ident(N), n_poses_max=N, n_slam_max=2, min_track_length=MIN_LEN, opp_ids=None)
    for name, v in (("nan", math.nan), ("plus_inf", math.inf), ("minus_inf", -math.inf)):
        # frame 1: three tracks; the second one's current (= last) feature has the special x
        a, b, d = (tm.Feat(*B0), tm.Feat(B0[0] + 1, B0[1])), (tm.Feat(*B1), tm.Feat(v, B1[1], B1[0] + 1, B1[1])), (tm.Feat(*B2), tm.Feat(B2[0] + 1, B2[1]))
        first = [list(a), list(b), list(d)]
        # frame 2: a continues; a match whose previous feature carries the same special x and b's y (NaN equals nothing, an infinity
        # only itself); one with the opposite infinity (or a NaN again); d continues
        other = -v if math.isinf(v) else v
        second = [[a[1].copy(), tm.Feat(B0[0] + 2, B0[1])], [tm.Feat(v, B1[1], B1[0] + 1, B1[1]), tm.Feat(B1[0] + 2, B1[1])],
                  [tm.Feat(other, B1[1], B1[0] + 1, B1[1]), tm.Feat(B1[0] + 3, B1[1])], [d[1].copy(), tm.Feat(B2[0] + 2, B2[1])]]
        third = [[p[1].copy(), tm.Feat(p[1].x + 1, p[1].y)] for p in second]
        c["special_" + name] = dict(multi_uav=False, tiles=(2, 2), max_tracks=16, expect={},
                                    frames=[dict(fr, matches=first), dict(fr, matches=second), dict(fr, matches=third)])
    zero = [[tm.Feat(5.0, B0[1], *B0), tm.Feat(0.0, B0[1], B0[0] + 1, B0[1])], [tm.Feat(6.0, B2[1], *B2), tm.Feat(1e-320, B2[1], B2[0] + 1, B2[1])]]
    second = [[tm.Feat(1e-320, B0[1], B0[0] + 1, B0[1]), tm.Feat(7.0, B0[1], B0[0] + 2, B0[1])],     # 1e-320 against the track's 0: not equal
              [tm.Feat(0.0, B2[1], B2[0] + 1, B2[1]), tm.Feat(8.0, B2[1], B2[0] + 2, B2[1])],          # 0 against 1e-320: not equal
              [tm.Feat(-0.0, B0[1], B0[0] + 1, B0[1]), tm.Feat(9.0, B0[1], B0[0] + 3, B0[1])]]         # -0 against 0: equal
    c["zero_against_denormal"] = dict(multi_uav=False, tiles=(2, 2), max_tracks=16, expect={1: dict(opp_new=2, opp_extended=1)},
                                      frames=[dict(fr, matches=zero), dict(fr, matches=second)])
    return c


def ring_case(n_frames=70):
    """One persistent track followed for 70 frames at N = 6: its true length passes the ring's 64."""
    s = Script().at(p=(40.0, 60.0))
    for _ in range(n_frames - 1):
        s.frame([("p", 3.0, 2.0)], 1)
    return s.case


def removal_case():
    """Persistent and new persistent tracks, the removal entries and clear between frames; the id counter survives clear."""
    names = ["p%d" % i for i in range(6)]
    s = Script().at(**{n: (B0[0] + 40.0 * i, B0[1] + 30.0 * i) for i, n in enumerate(names)}).at(q0=B3, q1=(B3[0] + 20.0, B3[1]), q2=(B3[0] + 40.0, B3[1]))
    _grow_persistent(s, names, 9)
    s.frame(names + ["q0", "q1", "q2"], 9).frame(names + ["q0", "q1", "q2"], 9)      # q0...q2 are new persistent tracks now
    s.op("remove_persistent", 2).op("remove_new_persistent", [0, 2]).frame([n for n in names if n != "p2"] + ["q1"], 9)
    s.op("remove_persistent", 0).op("clear").frame(["p1", "q1"], 9)
    return s.frame(["p1", "q1"], 9).case


def all_cases():
    c = dict(quirk_cases())
    c["sequence_single"] = sequence_case(False)
    c["sequence_multi_uav"] = sequence_case(True)
    c.update(special_value_cases())
    for i, j in ((0, 1), (63, 64), (64, 200)):
        c["duplicate_%d_%d" % (i, j)] = duplicate_case(i, j)
    c["ring_70_frames"] = ring_case()
    c["removals_and_clear"] = removal_case()
    return c
