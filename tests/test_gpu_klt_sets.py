"""The second Lucas-Kanade parameter set (xk_trk_klt_second, xk_trk_klt_select, _selected, _levels_of) through the C
ABI and tracker.Klt, on the cases of tests/klt_sets_np.py, whose conditions tests/test_klt_sets_np.py asserts without a GPU:

  xk_trk_track under either selection against klt_np.track with that set's parameters on the same images: status and the kept lists
  bit-equal, positions within 1e-9 px, min_eig within 1e-12 relative -- the bars of tests/test_gpu_klt.py, for the reason its header
  gives (A and b are the same integers on both sides);
  every pyramid level up to the deeper set's, both slots, bit-equal to klt_np;
  a tracker without a second set byte-equal to one built by the plain setup, and the error paths;
  Klt.photo_frame on the photometric sequence byte for byte against the chain of stage entries on a second tracker, which calls
  klt_select(1 if done else 0) between photo_calibrate and track, and against the two-set restatement with the bars of
  tests/test_gpu_photo_frame.py;
  Klt.frame under a selection switched in mid-sequence byte for byte against the chain;
  the C++ mirror (host/examples/photo_tracker_main.cpp --second) against Klt.photo_frame."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import klt_cases as kc
import klt_sets_np as ks
import photo_cases as phc
import photo_frame_cases as pc
import photo_np as pnp
import tracker_frame_cases as tc
import tracker_frame_chain as tfc
from photo_frame_chain import PhotoChain, PhotoRig, run_frames, state_of
from test_gpu_klt import compare
from test_gpu_photo_frame import same_frames
from test_gpu_photo_frame_host import checksum

from x_multi_agent_amd import engine, tracker

pytestmark = pytest.mark.gpu
XK_EINVAL = 1
COUNTS = tracker.FrameOut.COUNTS
PKG = os.path.join(os.path.dirname(__file__), "..", "x_multi_agent_amd")
W, H = ks.W, ks.H


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(4, 0, 4)
    yield e
    e.close()


def make_klt(eng, pair, second=True, **kw):
    s0, s1 = ks.PAIRS[pair]
    return tracker.Klt(eng, kc.MAX_FEATURES, W, H, s0["win"], s0["max_level"], ks.MAX_ITER, ks.EPS, s0["min_eig_thr"],
                       second=dict(s1) if second else None, **kw)


def refused(call, status=XK_EINVAL):
    with pytest.raises(engine.XkError) as e:
        call()
    assert e.value.status == status
    return e.value


def same_track(a, b, label):
    assert a.keys() == b.keys()
    for key in a:
        assert a[key].tobytes() == b[key].tobytes() and a[key].dtype == b[key].dtype, (label, key)


class SetsRig(PhotoRig):
    """photo_frame_chain.PhotoRig with the scene's second set declared right after the KLT setup; photo=False: a plain tracker."""

    def __init__(self, eng, sc, frame=True, photo=True):
        self.sc = sc
        self.mf = tracker.MatchFilter(eng, sc["max_matches"], kc.K_CHAIN, 0.0)
        try:
            self.k = k = tracker.Klt(eng, 0, W, H, sc["win"], sc["max_level"], sc["max_iter"], sc["eps"], sc["min_eig_thr"], match_filter=self.mf,
                                     second=sc.get("second"))
            k.detect_setup(sc["threshold"], sc["non_max_supp"], sc["block_half_length"], sc["margin"], sc["max_candidates"])
            d = sc["describe"]
            if d is not None:
                k.describe_setup(d["centroid"], d["angle_deg"], d["edge"], None, d["max_desc"])
            if photo:
                self.photo_setup()
            if frame:
                self.frame_setup()
                if photo:
                    k.photo_frame_setup(sc["n_hyp_photo"], sc["threshold_photo"])
        except Exception:
            self.close()
            raise


class Selecting:
    """A Klt whose photo_calibrate is followed by klt_select(1 if done else 0): what a caller of the stage entries does between
    xk_trk_photo_calibrate and xk_trk_track (tracker.cpp:641), done being the host's own record of an estimate so far."""

    def __init__(self, k):
        self._k, self.done = k, False

    def __getattr__(self, name):
        return getattr(self._k, name)

    def photo_calibrate(self, *a, **kw):
        c = self._k.photo_calibrate(*a, **kw)
        self.done = self.done or bool(c["estimated"])
        self._k.klt_select(1 if self.done else 0)
        return c

    def photo_reset(self):
        self._k.photo_reset()
        self.done = False


def chain_frames(rig, seq):
    """The sequence through the chain of stage entries with the selection made on the host -> per frame: the chain's dict with
    `features`, `state`, `done` and `selected` (the selection after the frame)."""
    view = types.SimpleNamespace(k=Selecting(rig.k), mf=rig.mf, sc=rig.sc)
    c = PhotoChain(view)
    frames = []
    for i, img in enumerate(seq):
        r = c.frame(img, pc.SEED + i, pc.SEED_PHOTO + i)
        r["features"], r["state"], r["done"], r["selected"] = c.features, state_of(view), view.k.done, rig.k.klt_selected
        frames.append(r)
    return frames


# ---- 1. xk_trk_track under either selection ----
@pytest.mark.parametrize("pair", ["A", "B", "C"])
def test_track_under_either_selection(eng, pair):
    a, b = ks.stage_images()
    pts = ks.stage_points()
    k = make_klt(eng, pair)
    try:
        assert k.klt_selected == 0 and [k.levels_of(0), k.levels_of(1)] == [ks.levels_of(s) for s in ks.PAIRS[pair]]
        k.push_image(a)
        k.push_image(b)
        compare(k.track(pts), ks.stage_restated(pair, 0), pair + " set 0")
        k.klt_select(1)
        assert k.klt_selected == 1
        got1 = k.track(pts)
        compare(got1, ks.stage_restated(pair, 1), pair + " set 1")
        same_track(k.track(pts), got1, pair + " set 1 twice")
        k.push_image(a)                                             # the selection is sticky across a push
        assert k.klt_selected == 1
        compare(k.track(pts), ks.stage_restated(pair, 1, True), pair + " set 1 after a push")
        k.klt_select(0)
        compare(k.track(pts), ks.stage_restated(pair, 0, True), pair + " set 0 after a push")
        # n around the features per workgroup, under the other set than the setup's
        k.klt_select(1)
        for n in (0, 1, kc.FEATURES_PER_WORKGROUP - 1, kc.FEATURES_PER_WORKGROUP + 1):
            got = k.track(pts[:n])
            ref = ks.stage_restated(pair, 1, True)
            assert np.array_equal(got["status"], ref["status"][:n]) and np.abs(got["cur_xy"] - ref["cur_xy"][:n]).max(initial=0.0) <= 1e-9
    finally:
        k.close()


def test_equal_sets_track_alike(eng):
    a, b = ks.stage_images()
    k = make_klt(eng, "D")
    try:
        k.push_image(a)
        k.push_image(b)
        got0 = k.track(ks.stage_points())
        k.klt_select(1)
        same_track(k.track(ks.stage_points()), got0, "D")
        compare(got0, ks.stage_restated("D", 0), "D")
    finally:
        k.close()


# ---- 2. the inspection path ----
@pytest.mark.parametrize("pair", ["A", "B"])
def test_every_level_up_to_the_deeper_set(eng, pair):
    imgs = ks.stage_images()
    deep = ks.deep_of(pair)
    k = make_klt(eng, pair)
    try:
        assert deep == 3 and k.levels() == ks.levels_of(ks.PAIRS[pair][0])
        assert [k.levels_of(0), k.levels_of(1)] == ([1, 3] if pair == "A" else [3, 1]) and k.levels_of(2) == -1
        k.push_image(imgs[0])
        k.push_image(imgs[1])
        for which in (0, 1):
            ref = ks.deep_pyramid(imgs[which], deep)
            for l in range(deep + 1):
                got = k.level(which, l)
                for g, r in zip(got, ref[l]):
                    assert g.shape == r.shape and g.dtype == r.dtype and g.tobytes() == r.tobytes(), (pair, which, l)
            refused(lambda: k.level(which, deep + 1))
    finally:
        k.close()


# ---- 3. no second set ----
def test_no_second_set_is_the_plain_tracker(eng):
    a, b = ks.stage_images()
    pts = ks.stage_points()
    s0 = ks.PAIRS["A"][0]
    plain, again, unused = make_klt(eng, "A", second=False), make_klt(eng, "A"), make_klt(eng, "A")
    try:
        # `again` declared a second set and then ran the plain setup again, which forgets it; `unused` keeps one and never selects it
        again.setup(W, H, s0["win"], s0["max_level"], ks.MAX_ITER, ks.EPS, s0["min_eig_thr"])
        assert plain.levels_of(1) == -1 and again.levels_of(1) == -1 and unused.levels_of(1) == 3
        refused(lambda: again.klt_select(1))
        ref = None
        for k in (plain, again, unused):
            k.push_image(a)
            k.push_image(b)
            got = k.track(pts)
            ref = ref or got
            same_track(got, ref, "track")
            refused(lambda: k.level(1, 2)) if k is not unused else k.level(1, 3)
    finally:
        for k in (plain, again, unused):
            k.close()
    sc = dict(tc.SCENES["walk"], win=s0["win"], max_level=s0["max_level"])
    seq = sc["sequences"][0][:4]
    rigs = [tfc.Rig(eng, sc), SetsRig(eng, sc, photo=False), SetsRig(eng, dict(sc, second=dict(ks.PAIRS["A"][1])), photo=False)]
    try:
        outs = [tfc.run_frames(r, [seq])[0] for r in rigs]
        assert outs[0][-1]["n_matches"] > 0 and outs[0][-1]["n_tracked"] > 0
        for o in outs[1:]:
            for fi, (x, y) in enumerate(zip(o, outs[0])):
                assert all(x[key] == y[key] for key in COUNTS), fi
                assert all(x[key].tobytes() == y[key].tobytes() for key in tfc.ARRAYS), fi
                assert all(x["features"][key].tobytes() == y["features"][key].tobytes() for key in x["features"]), fi
    finally:
        for r in rigs:
            r.close()


# ---- 4. error paths ----
def test_error_paths(eng):
    L = eng.L
    a, b = ks.stage_images()
    pts = ks.stage_points()
    k = make_klt(eng, "A", second=False)
    try:
        p = k.p
        second = lambda w, h, ml, thr=0.003: L.xk_trk_klt_second(p, C.c_int(w), C.c_int(h), C.c_int(ml), C.c_double(thr))
        assert L.xk_trk_klt_select(p, C.c_int(1)) == XK_EINVAL and b"xk_trk_klt_select" in L.xk_last_error(eng.h)
        assert k.klt_selected == 0
        for bad in (-1, 2):
            assert L.xk_trk_klt_select(p, C.c_int(bad)) == XK_EINVAL and k.klt_selected == 0
        assert L.xk_trk_klt_select(p, C.c_int(0)) == 0
        k.push_image(a)
        k.push_image(b)
        k.detect_setup(9, 1, 6, 25, 8192)
        before = k.track(pts)
        for bad in ((2, 9, 2), (9, 32, 2), (33, 33, 2), (9, 9, 5), (9, 9, -1)):       # a window outside 3...31, max_level 5
            assert second(*bad) == XK_EINVAL and b"xk_trk_klt_second" in L.xk_last_error(eng.h), bad
        assert second(9, 9, 2, -1.0) == XK_EINVAL and second(9, 9, 2, float("nan")) == XK_EINVAL
        assert k.levels_of(1) == -1 and k.klt_selected == 0
        # after the failures the two pushed images still track, and the detection setup is still there
        same_track(k.track(pts), before, "after failed calls")
        assert len(k.detect(1)["xy"]) > 0
        k.klt_second(**ks.PAIRS["A"][1])
        refused(lambda: k.track(pts))                               # a succeeding call forgets the images ...
        k.push_image(a)
        refused(lambda: k.track(pts))
        k.push_image(b)
        same_track(k.track(pts), before, "set 0 on the deeper slots")
        refused(lambda: k.detect(1))                                # ... and drops the dependent setups
        k.klt_select(1)
        k.klt_second(**ks.PAIRS["A"][1])                            # a setup-class call: the selection returns to 0
        assert k.klt_selected == 0
        refused(lambda: k.klt_select(2))
    finally:
        k.close()
    # a second window that does not fit the image: 16 x 16 pixels hold a 15 x 15 window, not a 16 x 16 one
    t = tracker.Klt(eng, 8, 16, 16, (9, 9), 2)
    try:
        img = np.ascontiguousarray(a[:16, :16])
        t.push_image(img)
        t.push_image(img)
        one = t.track(np.array([[8.0, 8.0]], np.float32))
        assert L.xk_trk_klt_second(t.p, C.c_int(16), C.c_int(9), C.c_int(0), C.c_double(0.003)) == XK_EINVAL
        assert b"does not fit" in L.xk_last_error(eng.h)
        same_track(t.track(np.array([[8.0, 8.0]], np.float32)), one, "16 x 16")
        assert L.xk_trk_klt_second(t.p, C.c_int(15), C.c_int(15), C.c_int(4), C.c_double(0.003)) == 0 and t.levels_of(1) == 0
    finally:
        t.close()
    assert L.xk_trk_klt_second(None, 9, 9, 2, C.c_double(0.003)) == XK_EINVAL and L.xk_trk_klt_selected(None) == -1


# ---- 5. the photometric frame ----
_photo = {}


def photo_frames(eng, pair):
    """The pair's photometric sequence through xk_trk_photo_frame twice on one tracker -- the second time after frame_reset and
    photo_reset and with the sticky selection on 1 -- once per module."""
    if pair not in _photo:
        sc = ks.scene(pair)
        rig = SetsRig(eng, sc)
        try:
            first = run_frames(rig, sc["sequences"])[0]
            assert rig.k.klt_selected == 0
            rig.k.frame_reset()
            rig.k.photo_reset()
            rig.k.klt_select(1)
            second = run_frames(rig, sc["sequences"])[0]
            assert rig.k.klt_selected == 1                          # the frame ignores the selection and leaves it unchanged
        finally:
            rig.close()
        _photo[pair] = (first, second)
    return _photo[pair]


@pytest.mark.parametrize("pair", ["A", "C"])
def test_photo_frame_against_the_chain_of_stage_entries(eng, pair):
    sc = ks.scene(pair)
    got, again = photo_frames(eng, pair)
    assert not any(isinstance(g, Exception) for g in got)
    rig = SetsRig(eng, sc, frame=False)
    try:
        ref = chain_frames(rig, sc["sequences"][0])
    finally:
        rig.close()
    for fi, (g, r) in enumerate(zip(got, ref)):
        print((pair, fi), {k: g[k] for k in COUNTS}, {k: g[k] for k in ("n_cal_kept", "estimated", "done", "support")}, "chain selected", r["selected"])
        assert g["done"] == r["done"], (pair, fi)
    done = [bool(g["done"]) for g in got]
    assert [r["selected"] for r in ref[1:]] == [int(d) for d in done[1:]] and 2 <= done.index(True) <= len(done) - 3
    same_frames([got], [ref], pair)
    # after photo_reset the next sequence starts on set 0 again with no further action, whatever the sticky selection says
    same_frames([again], [got], pair + " after a reset")


@pytest.mark.parametrize("pair", ["A", "C"])
def test_photo_frame_against_the_restatement(eng, pair):
    got, _ = photo_frames(eng, pair)
    pairs = [[g["state"]["ring"][-1] for g in got]]
    ref = ks.run_np(pair, pairs)[0]
    worst = 0.0
    for fi, (g, r) in enumerate(zip(got, ref)):
        at = (pair, fi)
        for key in ("n_cal_kept", "estimated", "done", "support"):
            assert g[key] == r[key], (at, key)
        assert phc.close([g["a_rel"], g["b_rel"]], [r["a_rel"], r["b_rel"]]) and phc.close(g["frame_ab"], r["frame_ab"]), at
        assert phc.close(g["state"]["ring"][-1], r["restated_pair"]), at
        assert np.array_equal(g["state"]["raw"], r["raw"]) and np.array_equal(g["state"]["working"], r["working"]), at
        if g["done"] and "n_total" in r:
            assert np.array_equal(g["state"]["working"], pnp.correct(g["state"]["raw"], *g["state"]["ring"][-1])), at
        for key in COUNTS:
            assert g[key] == r[key], (at, key)
        for key in ("score", "origin", "tiles"):
            assert np.array_equal(g[key], r[key]) and g[key].dtype == np.int32, (at, key)
        assert np.array_equal(g["desc"], r["desc"]), at
        for key in ("prev_intensity", "cur_intensity"):
            assert g[key].tobytes() == r[key].tobytes(), (at, key)
        for key in ("prev_xy", "cur_xy", "prev_dist_xy", "cur_dist_xy"):
            assert g[key].shape == r[key].shape, (at, key)
            if len(r[key]):
                worst = max(worst, float(np.abs(g[key] - r[key]).max()))
        f, rf = g["features"], r["features"]
        assert len(f["dist_xy"]) == len(rf["dist_xy"]) and np.array_equal(f["score"], rf["score"]) and np.array_equal(f["desc"], rf["desc"]), at
        assert f["intensity"].tobytes() == rf["intensity"].tobytes(), at
        if len(rf["dist_xy"]):
            worst = max(worst, float(np.abs(f["dist_xy"] - rf["dist_xy"]).max()))
    print(pair, "max |d pixel|", worst)
    assert worst <= 1e-9


# ---- 6. the plain frame under a selection switched in mid-sequence ----
def test_frame_follows_the_selection(eng):
    s0, s1 = ks.PAIRS["A"]
    sc = dict(tc.SCENES["walk"], win=s0["win"], max_level=s0["max_level"], second=dict(s1))
    seq = sc["sequences"][0]
    rig, plain = SetsRig(eng, sc, photo=False), SetsRig(eng, sc, frame=False, photo=False)
    try:
        chain = tfc.Chain(plain)
        tracked = {0: 0, 1: 0}
        for i, img in enumerate(seq):
            which = 1 if i < 3 else 0
            rig.k.klt_select(which)
            plain.k.klt_select(which)
            g, r = rig.k.frame(img, seed=tc.SEED + i), chain.frame(img, tc.SEED + i)
            assert rig.k.klt_selected == which
            for key in r:
                if key in COUNTS:
                    assert g[key] == r[key], (i, key)
                elif r[key] is not None:
                    assert g[key].tobytes() == r[key].tobytes(), (i, key)
            feats = rig.k.frame_features()
            assert all(feats[key].tobytes() == chain.features[key].tobytes() for key in feats), i
            tracked[which] += g["n_tracked"] + g["n_new_tracked"]
        assert tracked[0] > 0 and tracked[1] > 0
    finally:
        rig.close()
        plain.close()


# ---- 7. the host mirror ----
def test_cpp_photo_tracker_with_a_second_set(eng, tmp_path):
    exe = os.path.join(PKG, "xk_photo_tracker_example")
    if not os.path.exists(exe):
        from x_multi_agent_amd import build
        build.build_host()
    sc = ks.scene("A")
    seq, d, s1 = sc["sequences"][0], sc["describe"], sc["second"]
    frac = (kc.K_CHAIN[0] / W, kc.K_CHAIN[1] / H, kc.K_CHAIN[2] / W, kc.K_CHAIN[3] / H)
    Kc = (W * frac[0], H * frac[1], W * frac[2], H * frac[3])
    seed, seed_photo, threshold_photo = 11, 23, 12
    mf = tracker.MatchFilter(eng, sc["max_matches"], Kc, 0.0)
    k = tracker.Klt(eng, 0, W, H, sc["win"], sc["max_level"], 30, 0.01, sc["min_eig_thr"], match_filter=mf, second=s1)
    try:
        k.detect_setup(sc["threshold"], sc["non_max_supp"], sc["block_half_length"], max(sc["margin"], d["edge"]), 32768)
        k.describe_setup(d["centroid"], -1.0, d["edge"], None, sc["max_matches"])
        k.frame_setup(sc["n_feat_min"], sc["n_tiles_h"], sc["n_tiles_w"], sc["max_feat_per_tile"], sc["threshold_px"], sc["n_hyp"])
        k.photo_setup(sc["kernel_size"], sc["eps_gap"], sc["eps_base"], sc["n_hyp_photo"])
        k.photo_frame_setup(sc["n_hyp_photo"], threshold_photo)
        frames = [k.photo_frame(img, seed=seed + i, seed_photo=seed_photo + i) for i, img in enumerate(seq)]
    finally:
        k.close()
        mf.close()
    assert any(f["done"] and f["n_matches"] >= 7 for f in frames) and not frames[2]["done"] and frames[2]["n_matches"] >= 7

    case = tmp_path / "case.txt"
    case.write_text(f"{frac[0]!r} {frac[1]!r} {frac[2]!r} {frac[3]!r} 0.0 {W} {H} {W} {sc['win'][0]} {sc['win'][1]} {sc['max_level']} "
                    f"{sc['min_eig_thr']!r} {sc['threshold']} {sc['non_max_supp']} {sc['block_half_length']} {sc['margin']} {sc['n_feat_min']} "
                    f"{sc['n_tiles_h']} {sc['n_tiles_w']} {sc['max_feat_per_tile']} {sc['threshold_px']!r} {sc['n_hyp']} {seed} "
                    f"{sc['max_matches']} 1 {d['centroid']} {d['edge']} {sc['kernel_size']} {sc['eps_gap']!r} {sc['eps_base']!r} "
                    f"{sc['n_hyp_photo']} {threshold_photo} {seed_photo}\n")
    paths = []
    for i, img in enumerate(seq):
        p = tmp_path / f"image{i}.raw"
        p.write_bytes(np.ascontiguousarray(img).tobytes())
        paths.append(str(p))
    env = dict(os.environ, LD_LIBRARY_PATH=PKG + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    opt = ["--second", str(s1["win"][0]), str(s1["win"][1]), str(s1["max_level"]), repr(s1["min_eig_thr"])]
    r = subprocess.run([exe] + opt + [str(case)] + paths, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 6 * len(seq)
    for i, f in enumerate(frames):
        out = {line.split()[0]: line.split()[1:] for line in lines[6 * i:6 * i + 6]}
        assert [int(v) for v in out["F"]] == [i] + [f[key] for key in COUNTS], i
        g = out["G"]
        assert [int(v) for v in g[:4]] == [f["n_cal_kept"], int(f["estimated"]), int(f["done"]), f["support"]], i
        gains = np.array([float(v) for v in g[4:]])
        assert gains.tobytes() == np.concatenate([[f["a_rel"], f["b_rel"]], f["frame_ab"]]).tobytes(), i
        assert [int(v) for v in out["O"]] == f["origin"].tolist(), i
        v = np.array([float(x) for x in out["I"]]).reshape(-1, 2)
        assert v[:, 0].tobytes() == f["prev_intensity"].tobytes() and v[:, 1].tobytes() == f["cur_intensity"].tobytes(), i
        assert int(out["K"][0]) == int(f["done"]), i
        assert int(out["X"][0], 16) == checksum(f), i
