"""xk_trk_frame -- Tracker::track in one call on a feature list that stays on the device (csrc/xk_frame.hip.h) --
on the scenes of tests/tracker_frame_cases.py:

  against TrackerNp (tests/tracker_frame_np.py, the composition of the existing restatements): counts, origins, kept sets, scores,
  tiles and descriptors equal; distorted and undistorted pixels within 1e-9 px, the bar tests/test_gpu_klt.py holds for the
  tracking's positions and for the chained filter's pixels (its docstring says why: the same integers on both sides, round-off of
  order 1e-13 px, and no discrete decision within its margin -- tests/test_tracker_frame_np.py asserts the margins);

  against the CHAIN of the stage entries driven through the host as host/examples/klt_main.cpp drives them (push, track, the
  overflow pass on the host, detect, describe, track, filter_matches), same library, same seeds: every output byte for byte.

Also: the same sequence twice and again after xk_trk_frame_reset, stage calls between frames, and the error paths."""
import numpy as np
import pytest

import klt_cases as kc
import tracker_frame_cases as tc
import tracker_frame_np as tnp
from tracker_frame_chain import ARRAYS, Rig, run_chain, run_frames

from x_multi_agent_amd import engine, tracker

pytestmark = pytest.mark.gpu
XK_EINVAL, XK_ECAPACITY = 1, 6
COUNTS = tracker.FrameOut.COUNTS
# a scene for the chain alone: three pyramid levels and an odd window.  (Against TrackerNp the scenes track with an even window on
# level 0, where no floor of the tracking sits on an integer: a detected feature's pixels are integers.)
PYRAMID = dict(tc.SCENES["walk"], name="pyramid", win=(15, 15), max_level=2)


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(4, 0, 4)
    yield e
    e.close()


_results = {}


def frames_of(eng, name):
    """The scene's sequences through xk_trk_frame, once per module."""
    if name not in _results:
        sc = PYRAMID if name == "pyramid" else tc.SCENES[name]
        rig = Rig(eng, sc)
        try:
            _results[name] = run_frames(rig, sc["sequences"])
        finally:
            rig.close()
    return _results[name]


def same_bytes(a, b, label):
    for si, (fa, fb) in enumerate(zip(a, b)):
        assert len(fa) == len(fb)
        for fi, (x, y) in enumerate(zip(fa, fb)):
            if isinstance(x, Exception) or isinstance(y, Exception):
                assert isinstance(x, engine.XkError) and isinstance(y, engine.XkError) and x.status == y.status, (label, si, fi)
                continue
            for key in COUNTS:
                assert x[key] == y[key], (label, si, fi, key)
            for key in ARRAYS:
                assert x[key].tobytes() == y[key].tobytes(), (label, si, fi, key)
            for key in x["features"]:
                assert x["features"][key].tobytes() == y["features"][key].tobytes(), (label, si, fi, key)


@pytest.mark.parametrize("name", list(tc.SCENES))
def test_scene_against_the_restatement(eng, name):
    got, ref = frames_of(eng, name), tc.restated(name)
    with_desc = tc.SCENES[name]["describe"] is not None
    worst = 0.0
    for si, (fg, fr) in enumerate(zip(got, ref)):
        assert len(fg) == len(fr)
        for fi, (g, r) in enumerate(zip(fg, fr)):
            at = (name, si, fi)
            if isinstance(r, tnp.CapacityError):
                assert isinstance(g, engine.XkError) and g.status == XK_ECAPACITY, at
                assert {k: g.counts[k] for k in COUNTS} == r.counts, at
                continue
            assert not isinstance(g, Exception), (at, g)
            print(at, {k: g[k] for k in COUNTS})
            for key in COUNTS:
                assert g[key] == r[key], (at, key)
            for key in ("score", "origin", "tiles"):
                assert np.array_equal(g[key], r[key]) and g[key].dtype == np.int32, (at, key)
            if with_desc:
                assert np.array_equal(g["desc"], r["desc"]), at
            for key in ("prev_xy", "cur_xy", "prev_dist_xy", "cur_dist_xy"):
                assert g[key].shape == r[key].shape, (at, key)
                if len(r[key]):
                    worst = max(worst, float(np.abs(g[key] - r[key]).max()))
            f, rf = g["features"], r["features"]
            assert len(f["dist_xy"]) == len(rf["dist_xy"]) and np.array_equal(f["score"], rf["score"]), at
            if len(rf["dist_xy"]):
                worst = max(worst, float(np.abs(f["dist_xy"] - rf["dist_xy"]).max()))
            if with_desc:
                assert np.array_equal(f["desc"], rf["desc"]), at
            if "n_total" in r:                                      # not a first frame: the resident list is the kept current features (tracker.cpp:299)
                assert f["dist_xy"].tobytes() == g["cur_dist_xy"].tobytes() and f["score"].tobytes() == g["score"].tobytes(), at
    print(name, "max |d pixel|", worst)
    assert worst <= 1e-9


@pytest.mark.parametrize("name", list(tc.SCENES) + ["pyramid"])
def test_scene_against_the_chain_of_stage_entries(eng, name):
    sc = PYRAMID if name == "pyramid" else tc.SCENES[name]
    got = frames_of(eng, name)
    rig = Rig(eng, sc, frame=False)
    try:
        ref = run_chain(rig, sc["sequences"])
    finally:
        rig.close()
    for si, (fg, fr) in enumerate(zip(got, ref)):
        assert len(fg) == len(fr)
        for fi, (g, r) in enumerate(zip(fg, fr)):
            at = (name, si, fi)
            if isinstance(r, Exception):
                assert isinstance(g, engine.XkError) and g.status == r.status == XK_ECAPACITY, at
                assert {k: g.counts[k] for k in r.counts} == r.counts, at
                continue
            assert not isinstance(g, Exception), (at, g)
            for key in r:
                if key in COUNTS:
                    assert g[key] == r[key], (at, key)
                elif key in ARRAYS and r[key] is not None:
                    assert g[key].tobytes() == r[key].tobytes(), (at, key)
            for key in ("dist_xy", "score", "desc"):
                assert g["features"][key].tobytes() == r["features"][key].tobytes(), (at, key)


def test_twice_and_after_a_reset(eng):
    sc = tc.SCENES["walk"]
    first = frames_of(eng, "walk")
    rig = Rig(eng, sc)
    try:
        same_bytes(run_frames(rig, sc["sequences"]), first, "a second tracker")
        rig.k.frame_reset()
        same_bytes(run_frames(rig, sc["sequences"]), first, "after a reset")
    finally:
        rig.close()


def test_stage_calls_between_frames(eng):
    """xk_trk_track and xk_trk_detect between two frames return what they return without a frame setup, and the frames go on as
    if nothing had been called.  xk_trk_describe of the PREVIOUS image after a frame that did not re-detect likewise."""
    sc = tc.SCENES["walk"]
    seq = sc["sequences"][0]
    first = frames_of(eng, "walk")[0]
    pts = np.array([[40.3, 50.2], [100.7, 60.1], [80.0, 40.0], [400.0, 3.0]], np.float32)
    rig, plain = Rig(eng, sc), Rig(eng, sc, frame=False)
    try:
        frames = []
        for i, img in enumerate(seq):
            r = rig.k.frame(img, seed=tc.SEED + i)
            r["features"] = rig.k.frame_features()
            frames.append(r)
            plain.k.push_image(img)
            if i in (1, 3):                                         # after a re-detecting frame, before one that does not
                a, b = rig.k.track(pts), plain.k.track(pts)
                for key in a:
                    assert a[key].tobytes() == b[key].tobytes(), (i, key)
                for which in (0, 1):
                    a, b = rig.k.detect(which, pts.astype(np.float64)), plain.k.detect(which, pts.astype(np.float64))
                    assert a["xy"].tobytes() == b["xy"].tobytes() and a["score"].tobytes() == b["score"].tobytes(), (i, which)
                    assert a["n_candidates"] == b["n_candidates"] and len(a["xy"]) > 0
                    sa, sb = rig.k.detect_stage(), plain.k.detect_stage()
                    assert sa[0].tobytes() == sb[0].tobytes() and sa[1].tobytes() == sb[1].tobytes()
                a, b = rig.k.describe(a["xy"], 1), plain.k.describe(b["xy"], 1)
                assert a["desc"].tobytes() == b["desc"].tobytes() and len(a["desc"]) > 0
        same_bytes([frames], [first], "with stage calls between the frames")
    finally:
        rig.close()
        plain.close()
    # describe(xy, 0) after a frame that did NOT re-detect: it queued the blur of the PREVIOUS slot under a predicate that was 0, and the
    # host may not count on a blur it queued there.  Above, the one such frame (4) finds that slot blurred by the describe(xy, 1) after
    # frame 3 and queues none; with n_feat_min = 1 no frame re-detects, and from frame 2 on the previous slot holds no earlier blur.
    sc = dict(sc, n_feat_min=1)
    rig, plain = Rig(eng, sc), Rig(eng, sc, frame=False)
    try:
        described_previous = 0
        for i, img in enumerate(seq):
            r = rig.k.frame(img, seed=tc.SEED + i)
            plain.k.push_image(img)
            if i > 1 and not r["redetected"]:
                a, b = rig.k.describe(pts.astype(np.int32), 0), plain.k.describe(pts.astype(np.int32), 0)
                assert all(a[key].tobytes() == b[key].tobytes() for key in ("desc", "keep_idx", "dir", "moments")) and len(a["desc"]) > 0, i
                described_previous += 1
        assert described_previous > 0
    finally:
        rig.close()
        plain.close()


def test_error_paths(eng):
    sc = tc.SCENES["walk"]
    seq = sc["sequences"][0]
    mf = tracker.MatchFilter(eng, 64, kc.K_CHAIN, 0.0)
    k = tracker.Klt(eng, 0, tc.W, tc.H, sc["win"], 0, match_filter=mf)
    try:
        def refused(call, status=XK_EINVAL):
            with pytest.raises(engine.XkError) as e:
                call()
            assert e.value.status == status
            return e.value

        refused(lambda: k.frame_setup())                            # before xk_trk_detect_setup
        k.detect_setup(9, 1, 6, 10, 8192)
        refused(lambda: k.frame(seq[0]))                            # before xk_trk_frame_setup
        refused(lambda: k.frame_reset())
        refused(lambda: k.frame_features())
        for bad in (dict(n_feat_min=-1), dict(n_tiles_h=0), dict(n_tiles_w=0), dict(n_tiles_h=100, n_tiles_w=100), dict(max_feat_per_tile=-1),
                    dict(threshold_px=-1.0), dict(n_hyp=0), dict(n_hyp=5000)):
            refused(lambda: k.frame_setup(**bad))
        k.describe_setup(1, -1.0, 25, None, 64)
        refused(lambda: k.frame_setup())                            # the detection's margin (10) is below the description's edge (25)
        k.detect_setup(9, 1, 6, 25, 8192)
        k.frame_setup(n_feat_min=20, n_hyp=64)
        assert len(k.frame_features()["score"]) == 0
        # more features accepted than max_matches (64 here): reported with the counts, and the next frame is a first frame
        k.detect_setup(9, 1, 2, 25, 8192)
        refused(lambda: k.frame(seq[0]))                            # (a new detection setup dropped the frame setup)
        k.frame_setup(n_feat_min=20, n_hyp=64)
        e = refused(lambda: k.frame(seq[0]), XK_ECAPACITY)
        assert e.counts["n_accepted"] > 64 and e.counts["n_matches"] == 0
        # more candidates than max_candidates
        k.detect_setup(9, 1, 6, 25, 16)
        k.frame_setup(n_feat_min=20, n_hyp=64)
        e = refused(lambda: k.frame(seq[0]), XK_ECAPACITY)
        assert e.counts["n_candidates"] > 16 and e.counts["n_accepted"] == 0
        # more keypoints than max_desc
        k.detect_setup(9, 1, 6, 25, 8192)
        k.describe_setup(1, -1.0, 25, None, 8)
        k.frame_setup(n_feat_min=20, n_hyp=64)
        e = refused(lambda: k.frame(seq[0]), XK_ECAPACITY)
        assert e.counts["n_accepted"] > 8
        # a frame, a direct push, and the next frame is a first frame again
        k.describe_setup(1, -1.0, 25, None, 64)
        k.frame_setup(n_feat_min=20, n_hyp=64)
        a = k.frame(seq[0])
        assert a["n_accepted"] > 7 and a["n_matches"] == 0
        b = k.frame(seq[1], seed=1)
        assert b["n_matches"] >= 7 and len(k.frame_features()["score"]) == b["n_matches"]
        k.push_image(seq[2])
        assert len(k.frame_features()["score"]) == 0
        c = k.frame(seq[0])
        assert c["n_matches"] == 0 and c["n_tracked"] == 0 and c["n_accepted"] == a["n_accepted"]
        # the photometric frame is not built
        k.photo_setup()
        refused(lambda: k.frame(seq[1]))
        # a new klt setup drops the frame setup
        k.setup(tc.W, tc.H, sc["win"], 0)
        refused(lambda: k.frame(seq[0]))
        with pytest.raises(ValueError):
            k.frame(seq[0][:10])
    finally:
        k.close()
        mf.close()
