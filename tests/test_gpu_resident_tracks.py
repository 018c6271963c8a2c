"""TrackManager::manageTracks on tracks that stay on the device (xk_trk_tracks_*) against the restatement
tests/track_manager_np.py::TrackManagerNp, after EVERY frame of every case of tests/resident_tracks_cases.py: the three own lists (ids,
order, true lengths, pixel observations bit for bit, scores, tiles), the five measurement lists (ids, offsets, normalised coordinates
bit for bit), the lost indices, `claimed` and the counts."""
import ctypes as C

import numpy as np
import pytest

import klt_cases as kc
import resident_tracks_cases as rc
import track_manager_cases as tmc
import tracker_frame_cases as tfc
from tracker_frame_chain import Rig

from x_multi_agent_amd import engine, tracker

pytestmark = pytest.mark.gpu
XK_EINVAL, XK_ECAPACITY = 1, 6
MAX_MATCHES = 300
CASES = rc.all_cases()


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(4, 0, 4)
    yield e
    e.close()


class Store:
    """A Klt with a track store on a 640 x 480 camera with the track manager's intrinsics."""

    def __init__(self, eng, case, max_matches=MAX_MATCHES):
        self.mf = tracker.MatchFilter(eng, max_matches, tmc.K, 0.0)
        self.k = tracker.Klt(eng, 0, tmc.WIDTH, tmc.HEIGHT, (15, 15), 0, match_filter=self.mf)
        self.setup(case)

    def setup(self, case):
        self.k.tracks_setup(case["max_tracks"], case["tiles"][0], case["tiles"][1], tmc.WIDTH, tmc.HEIGHT, 0.05, 0.05, case["multi_uav"])

    def close(self):
        self.k.close()
        self.mf.close()


def columns(matches):
    n = len(matches)
    prev = np.array([(p.x, p.y) for p, _ in matches], np.float64).reshape(n, 2)
    cur = np.array([(c.x, c.y) for _, c in matches], np.float64).reshape(n, 2)
    dprev = np.array([(p.xd, p.yd) for p, _ in matches], np.float64).reshape(n, 2)
    dcur = np.array([(c.xd, c.yd) for _, c in matches], np.float64).reshape(n, 2)
    score = np.array([int(c.score) for _, c in matches], np.int32).reshape(n)
    return prev, cur, dprev, dcur, score


def manage(k, frame, multi_uav):
    ids = list(frame["opp_ids"] or []) if multi_uav else None
    res = k.tracks_manage(*columns(frame["matches"]), frame["cam_rots"], frame["n_poses_max"], frame["n_slam_max"], frame["min_track_length"], ids)
    assert ids is None or ids == []                                # the caller's list is consumed
    return res


def apply_op(k, op):
    if op[0] == "remove_persistent":
        k.tracks_remove_persistent(op[1])
    elif op[0] == "remove_new_persistent":
        k.tracks_remove_new_persistent(op[1])
    else:
        k.tracks_clear()


def compare_lists(k, runner, label):
    for which in range(3):
        got, want = k.tracks_lists(which), runner.own_list(which)
        for key in ("ids", "lengths", "obs", "score", "tiles"):
            assert rc.same_bits(got[key], want[key]), (label, "list", which, key, got[key][:4], want[key][:4])


def compare(k, runner, res, claimed, label):
    m = runner.mgr
    compare_lists(k, runner, label)
    assert (res.status, res.n_persistent, res.n_new_persistent, res.n_opportunistic) == (0, len(m.slam), len(m.new_slam), len(m.opp)), label
    assert res.next_id == m.next_id and res.n_lost == len(m.lost) and res.n_claimed == int(claimed.sum()), label
    assert res.lost_slam_idxs.tolist() == list(m.lost), (label, res.lost_slam_idxs, m.lost)
    assert rc.same_bits(res.claimed, claimed), (label, "claimed")
    for l, (got, want) in enumerate(zip(res.lists, runner.measurement_lists())):
        for key in ("ids", "off", "xy"):
            assert rc.same_bits(got[key], want[key]), (label, "measurement list", l, key, got[key], want[key])


def run_case(eng, case, name):
    st, runner = Store(eng, case), rc.Runner(case)
    try:
        for i, fr in enumerate(case["frames"]):
            claimed = runner.step(fr)
            if "op" in fr:
                apply_op(st.k, fr["op"])
                compare_lists(st.k, runner, (name, i))
            else:
                compare(st.k, runner, manage(st.k, fr, case["multi_uav"]), claimed, (name, i))
    finally:
        st.close()
    return runner


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_against_the_restatement_after_every_frame(eng, name):
    run_case(eng, CASES[name], name)


@pytest.mark.parametrize("n_opp", rc.EDGE_SIZES)
def test_wavefront_and_workgroup_edges(eng, n_opp):
    """0, 1, 63, 64, 65 and 257 matches against n_opp opportunistic tracks: one store, set up anew per size."""
    st = Store(eng, rc.edge_case(0, 0))
    try:
        for n in rc.EDGE_SIZES:
            case = rc.edge_case(n, n_opp)
            st.setup(case)
            runner = rc.Runner(case)
            for i, fr in enumerate(case["frames"]):
                claimed = runner.step(fr)
                compare(st.k, runner, manage(st.k, fr, False), claimed, ("edge", n, n_opp, i))
    finally:
        st.close()


def test_the_ring_keeps_the_newest_64_and_the_true_length(eng):
    r = run_case(eng, CASES["ring_70_frames"], "ring")               # (every frame compared, the crop to n_poses_max included)
    assert [len(t) for t in r.mgr.slam] == [70]


def snapshot(k):
    return [k.tracks_lists(w) for w in range(3)]


def same_snapshot(a, b):
    return all(rc.same_bits(x[key], y[key]) for x, y in zip(a, b) for key in x)


def test_refusals_leave_the_store_as_it_was(eng):
    case = rc.quirk_cases()["evict_existing"]
    small = dict(case, max_tracks=6)                                  # 4 persistent tracks and the candidate: one slot is left
    st, runner = Store(eng, small), rc.Runner(small)
    try:
        frames = case["frames"]
        for fr in frames[:4]:
            runner.step(fr)
            res = manage(st.k, fr, False)
        before, next_id = snapshot(st.k), res.next_id
        last = frames[4]
        # a match outside the grid: the current feature right of the image
        outside = dict(last, matches=[[p.copy(), c.copy()] for p, c in last["matches"]])
        outside["matches"][2][1].xd = 5.0 * tmc.WIDTH
        with pytest.raises(engine.XkError) as e:
            manage(st.k, outside, False)
        assert e.value.status == XK_EINVAL and e.value.tracks_status == 1 and same_snapshot(before, snapshot(st.k))
        # a frame over max_tracks: two new tracks, one free slot
        extra = [[rc.tm.Feat(300.0 + 7 * j, 200.0), rc.tm.Feat(301.0 + 7 * j, 200.0)] for j in range(2)]
        with pytest.raises(engine.XkError) as e:
            manage(st.k, dict(last, matches=last["matches"] + extra), False)
        assert e.value.status == XK_ECAPACITY and e.value.tracks_status == 2 and same_snapshot(before, snapshot(st.k))
        # n_opp + n_matches > max_tracks with min_track_length <= 2
        with pytest.raises(engine.XkError) as e:
            manage(st.k, dict(last, matches=last["matches"] + extra[:1], min_track_length=2), False)
        assert e.value.status == XK_ECAPACITY and e.value.tracks_status == 2 and same_snapshot(before, snapshot(st.k))
        # the next valid frame gives the restatement's result, ids included
        claimed = runner.step(last)
        res = manage(st.k, last, False)
        compare(st.k, runner, res, claimed, "after the refusals")
        assert res.next_id == next_id
    finally:
        st.close()


def test_every_einval_leaves_the_object_usable(eng):
    case = rc.quirk_cases()["unmatched_match_fresh_id"]
    mf = tracker.MatchFilter(eng, 8, tmc.K, 0.0)
    k = tracker.Klt(eng, 0, tmc.WIDTH, tmc.HEIGHT, (15, 15), 0, match_filter=mf)
    fr = case["frames"][0]
    cols = columns(fr["matches"])

    def refused(call, rc_=XK_EINVAL):
        with pytest.raises(engine.XkError) as e:
            call()
        assert e.value.status == rc_, e.value

    try:
        raw = Raw(eng, k)                                              # before the setup: the library's own refusals
        idx0 = (C.c_uint * 1)(0)
        for got in (raw.manage(cols), raw.manage_frame(), eng.L.xk_trk_tracks_lists(k.p, C.c_int(0), None, None, None, None, None, C.byref(C.c_int(0))),
                    eng.L.xk_trk_tracks_remove_persistent(k.p, C.c_uint(0)), eng.L.xk_trk_tracks_remove_new_persistent(k.p, idx0, C.c_int(1)),
                    eng.L.xk_trk_tracks_clear(k.p)):
            assert got == XK_EINVAL
        for bad in (dict(max_tracks=0), dict(max_tracks=(1 << 20) + 1), dict(n_tiles_h=0), dict(n_tiles_w=65, n_tiles_h=64), dict(width=0),
                    dict(height=0), dict(min_baseline_x_n=float("nan"))):
            refused(lambda: k.tracks_setup(**dict(dict(max_tracks=8, n_tiles_h=2, n_tiles_w=2, width=tmc.WIDTH, height=tmc.HEIGHT), **bad)))
        k.tracks_setup(8, 2, 2, tmc.WIDTH, tmc.HEIGHT, 0.05, 0.05)
        runner = rc.Runner(case)
        claimed = runner.step(fr)
        compare(k, runner, manage(k, fr, False), claimed, "first")
        refused(lambda: k.tracks_setup(0))                             # a failed setup leaves the store as it was
        compare_lists(k, runner, "after a failed setup")
        nine = [np.zeros((9, 2))] * 4 + [np.zeros(9, np.int32)]
        for call in (lambda: k.tracks_manage(*nine, rc.ident(6), 6, 4, 3),                   # more matches than max_matches
                     lambda: k.tracks_manage(*cols, rc.ident(2), 6, 4, 3), lambda: k.tracks_manage(*cols, rc.ident(65), 6, 4, 3),
                     lambda: k.tracks_manage(*cols, rc.ident(6), 2, 4, 3), lambda: k.tracks_manage(*cols, rc.ident(6), 6, -1, 3),
                     lambda: k.tracks_manage(*cols, rc.ident(6), 6, 4, 0), lambda: k.tracks_manage(*cols, rc.ident(6), 6, 4, 7),
                     lambda: k.tracks_manage(*cols, rc.ident(6), 6, 4, 3, opp_ids=list(range(9))),
                     lambda: k.tracks_lists(3), lambda: k.tracks_lists(-1), lambda: k.tracks_remove_persistent(0),
                     lambda: k.tracks_remove_new_persistent([0]), lambda: k.tracks_manage_frame(rc.ident(6), 6, 4, 3)):   # no frame setup
            refused(call)
        compare_lists(k, runner, "after the refusals")
        fr = case["frames"][1]
        claimed = runner.step(fr)
        compare(k, runner, manage(k, fr, False), claimed, "second")
        # removal indices against the counts of the last result block: one new persistent track now
        assert len(runner.mgr.new_slam) == 1 and len(runner.mgr.slam) == 0
        for call in (lambda: k.tracks_remove_new_persistent([1]), lambda: k.tracks_remove_new_persistent([0, 0]),
                     lambda: k.tracks_remove_persistent(0)):
            refused(call)
        compare_lists(k, runner, "after refused removals")
        # multi_uav without an id list
        k.tracks_setup(8, 2, 2, tmc.WIDTH, tmc.HEIGHT, 0.05, 0.05, multi_uav=True)
        refused(lambda: k.tracks_manage(*cols, rc.ident(6), 6, 4, 3))
        assert k.tracks_manage(*cols, rc.ident(6), 6, 4, 3, opp_ids=[]).n_opportunistic == 1
    finally:
        k.close()
        mf.close()


class Raw:
    """The C entries through ctypes with every argument open to the caller: what the Python binding cannot get wrong."""

    def __init__(self, eng, k):
        self.L, self.p = eng.L, k.p
        self.lost, self.claimed = np.zeros(64, np.int32), np.zeros(64, np.uint8)
        self.ids, self.off, self.xy = np.zeros(256, np.int64), np.zeros(257, np.int32), np.zeros((4096, 2))

    def out(self, **over):
        o = tracker.TracksOut()
        o.cap_lost, o.cap_entries, o.cap_obs = 64, 256, 4096
        o.lost_slam_idxs, o.claimed = self.lost.ctypes.data_as(engine.c_ip), self.claimed.ctypes.data_as(tracker.c_ub)
        o.ids, o.off, o.xy = self.ids.ctypes.data_as(tracker.c_lp), self.off.ctypes.data_as(engine.c_ip), self.xy.ctypes.data_as(engine.c_dp)
        for key, v in over.items():
            setattr(o, key, v)
        return o

    def tail(self, quats, ids, n_ids, out, null_out, params):
        q = np.ascontiguousarray(rc.ident(6) if quats is None or quats is False else quats, np.float64)
        self.keep = (q, np.ascontiguousarray(list(ids or []) + [0], np.int64), C.c_int(0 if n_ids is None else n_ids), self.out() if out is None else out)
        return (None if quats is False else q.ctypes.data_as(engine.c_dp), C.c_int(len(q)), *(C.c_int(v) for v in params),
                None if ids is None else self.keep[1].ctypes.data_as(tracker.c_lp), None if n_ids is None else C.byref(self.keep[2]),
                None if null_out else C.byref(self.keep[3]))

    def manage(self, cols, null_col=None, quats=None, ids=None, n_ids=None, out=None, null_out=False, params=(6, 4, 3)):
        """quats False: a null C_q_G.  null_col: the index of the match column passed as NULL."""
        ptrs = [c.ctypes.data_as(engine.c_ip if i == 4 else engine.c_dp) for i, c in enumerate(cols)]
        if null_col is not None:
            ptrs[null_col] = None
        return self.L.xk_trk_tracks_manage(self.p, *ptrs, C.c_int(len(cols[4])), *self.tail(quats, ids, n_ids, out, null_out, params))

    def manage_frame(self, **kw):
        return self.L.xk_trk_tracks_manage_frame(self.p, *self.tail(kw.get("quats"), kw.get("ids"), kw.get("n_ids"), kw.get("out"), kw.get("null_out", False),
                                                                     kw.get("params", (6, 4, 3))))


def test_every_einval_of_the_c_entries_that_the_binding_cannot_reach(eng):
    """Null pointers, a negative id count, capacities below the bound, multi_uav outside 0 / 1, a null count, a negative n: each is
    XK_EINVAL, nothing changes, and the store goes on to give the restatement's result."""
    case = rc.quirk_cases()["unmatched_match_fresh_id"]
    mf = tracker.MatchFilter(eng, 8, tmc.K, 0.0)
    k = tracker.Klt(eng, 0, tmc.WIDTH, tmc.HEIGHT, (15, 15), 0, match_filter=mf)
    L = eng.L
    try:
        raw, runner = Raw(eng, k), rc.Runner(case)
        for multi_uav in (2, -1):
            assert L.xk_trk_tracks_setup(k.p, C.c_int(8), C.c_int(2), C.c_int(2), C.c_int(tmc.WIDTH), C.c_int(tmc.HEIGHT), C.c_double(0.05),
                                         C.c_double(0.05), C.c_int(multi_uav)) == XK_EINVAL
        k.tracks_setup(8, 2, 2, tmc.WIDTH, tmc.HEIGHT, 0.05, 0.05)
        for fr in case["frames"]:                                    # one new persistent track and one opportunistic track afterwards
            claimed = runner.step(fr)
            compare(k, runner, manage(k, fr, False), claimed, "set-up frames")
        assert len(runner.mgr.new_slam) == 1 and len(runner.mgr.opp) == 1
        nxt = dict(case["frames"][1], matches=[[c.copy(), rc.tm.Feat(c.x + 1.0, c.y)] for _, c in case["frames"][1]["matches"]])
        cols = columns(nxt["matches"])
        calls = [lambda i=i: raw.manage(cols, null_col=i) for i in range(5)]                      # a null match column with n > 0
        calls += [lambda: raw.manage(cols, quats=False),                                           # a null C_q_G
                  lambda: raw.manage(cols, ids=None, n_ids=2),                                     # null opp_ids with *n_opp_ids > 0
                  lambda: raw.manage(cols, ids=[1], n_ids=-1),                                     # a negative *n_opp_ids
                  lambda: raw.manage(cols, null_out=True)]                                         # a null out
        calls += [lambda f=f: raw.manage(cols, out=raw.out(**{f: None})) for f in ("lost_slam_idxs", "claimed", "ids", "off", "xy")]
        # the bounds with P = 1, O = 1, n = 2, six attitudes, n_poses_max 6: cap_lost >= 1, cap_entries >= 4, cap_obs >= 3 * 6 + 6 = 24
        calls += [lambda: raw.manage(cols, out=raw.out(cap_lost=0)), lambda: raw.manage(cols, out=raw.out(cap_entries=3)),
                  lambda: raw.manage(cols, out=raw.out(cap_obs=23)), lambda: raw.manage(cols, out=raw.out(cap_obs=-1))]
        calls += [lambda: L.xk_trk_tracks_lists(k.p, C.c_int(0), None, None, None, None, None, None),              # a null count
                  lambda: L.xk_trk_tracks_remove_new_persistent(k.p, (C.c_uint * 1)(0), C.c_int(-1)),                # n < 0
                  lambda: L.xk_trk_tracks_remove_new_persistent(k.p, None, C.c_int(1)),                              # null idxs with n > 0
                  lambda: raw.manage_frame()]                                                                        # no frame setup on this xk_trk
        for i, call in enumerate(calls):
            assert call() == XK_EINVAL, i
            compare_lists(k, runner, ("after refusal", i))
        # the capacities at the bound exactly are accepted, and the frame is the restatement's
        o = raw.out(cap_lost=1, cap_entries=4, cap_obs=24)
        claimed = runner.step(nxt)
        m = runner.mgr
        assert raw.manage(cols, out=o) == 0 and (o.n_persistent, o.n_new_persistent, o.n_opportunistic) == (len(m.slam), len(m.new_slam), len(m.opp))
        compare_lists(k, runner, "after the accepted frame")
        assert raw.claimed[:2].tolist() == claimed.tolist() and o.next_id == runner.mgr.next_id
    finally:
        k.close()
        mf.close()


def test_manage_frame_after_a_frame_that_returned_an_error(eng):
    """The scene `full` of tracker_frame_cases: a frame ends in XK_ECAPACITY.  Its block is not offered; the first frame behind it is."""
    sc = tfc.SCENES["full"]
    rig = Rig(eng, sc)
    params = (rc.ident(6), 6, 10, 3)
    try:
        rig.k.tracks_setup(256, 1, 1, tfc.W, tfc.H, 0.004, 0.004)
        failed = 0
        for i, img in enumerate(sc["sequences"][0]):
            try:
                f = rig.k.frame(img, seed=tfc.SEED + i)
            except engine.XkError as e:
                assert e.status == XK_ECAPACITY
                failed += 1
                before = snapshot(rig.k)
                with pytest.raises(engine.XkError) as e2:
                    rig.k.tracks_manage_frame(*params)
                assert e2.value.status == XK_EINVAL and same_snapshot(before, snapshot(rig.k))
                continue
            res = rig.k.tracks_manage_frame(*params, n_matches=f["n_matches"])
            assert res.status == 0
        assert failed >= 1
    finally:
        rig.close()


def test_the_id_counter_survives_clear_and_a_new_setup_restarts_it(eng):
    r = run_case(eng, CASES["removals_and_clear"], "removals")
    assert min(t.id for t in r.mgr.slam + r.mgr.new_slam + r.mgr.opp) > 9          # the tracks after the clear carry later ids


# ---- frame-fed: the matches never leave the device --------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["starved", "walk"])
def test_frame_fed_store_equals_the_store_fed_the_downloaded_frame(eng, scene):
    sc = tfc.SCENES[scene]
    rig = Rig(eng, sc)                                               # store A on the xk_trk that runs the frames
    mf = tracker.MatchFilter(eng, sc["max_matches"], kc.K_CHAIN, 0.0)   # store B on one of its own
    kb = tracker.Klt(eng, 0, tfc.W, tfc.H, (15, 15), 0, match_filter=mf)
    params = (rc.ident(6), 6, 10, 3)
    try:
        for k in (rig.k, kb):
            k.tracks_setup(1024, sc["n_tiles_h"], sc["n_tiles_w"], tfc.W, tfc.H, 0.004, 0.004)
        with pytest.raises(engine.XkError) as e:                     # before any frame
            rig.k.tracks_manage_frame(*params)
        assert e.value.status == XK_EINVAL
        n_frames = 0
        for si, seq in enumerate(sc["sequences"]):
            if si:
                rig.k.frame_reset()
                with pytest.raises(engine.XkError) as e:             # after a reset: the last frame's block is no longer offered
                    rig.k.tracks_manage_frame(*params)
                assert e.value.status == XK_EINVAL
            for i, img in enumerate(seq):
                f = rig.k.frame(img, seed=tfc.SEED + i)
                n = f["n_matches"]
                assert i > 0 or n == 0                               # a first frame: a valid empty match list
                a = rig.k.tracks_manage_frame(*params, n_matches=n)
                b = kb.tracks_manage(f["prev_xy"], f["cur_xy"], f["prev_dist_xy"], f["cur_dist_xy"], f["score"], *params)
                label = (scene, si, i)
                for key in tracker.TracksOut.COUNTS + ("next_id",):
                    assert getattr(a, key) == getattr(b, key), (label, key)
                assert rc.same_bits(a.claimed, b.claimed) and rc.same_bits(a.lost_slam_idxs, b.lost_slam_idxs), label
                for la, lb in zip(a.lists, b.lists):
                    assert all(rc.same_bits(la[key], lb[key]) for key in la), label
                assert same_snapshot(snapshot(rig.k), snapshot(kb)), label
                n_frames += 1
        assert n_frames >= 2
    finally:
        kb.close()
        mf.close()
        rig.close()
