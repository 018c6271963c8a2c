"""xk_trk_describe_setup / xk_trk_describe / xk_trk_describe_stage (csrc/xk_orb.hip.h) through tracker.Klt and the C ABI, against
the NumPy restatement tests/orb_np.py on every scene of tests/orb_cases.py: the blurred image with its borders, the pattern, the
kept indices, the moments, the directions and the descriptors, all bit for bit -- there is no tolerance.  Then the two slots and
the blur flag across pushes, a repeated call, the tracking and the detection before and after a description on the same xk_trk,
the chain detection -> description -> place.Database.knn_match on a shifted pair, every status code, and what a setup survives.
tests/test_orb_np.py verifies the restatement and the scenes without a GPU."""
import ctypes as C

import numpy as np
import pytest

import fast_cases as fc
import klt_cases as kc
import orb_cases as oc
import orb_np as onp

from x_multi_agent_amd import engine, place, tracker

pytestmark = pytest.mark.gpu
c_ub, c_sb = tracker.c_ub, tracker.c_sb
c_ip = engine.c_ip
KEYS = ("keep_idx", "moments", "dir", "desc")


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(4, 0, 4)
    yield e
    e.close()


def check(got, ref, label):
    for key in KEYS:
        assert got[key].dtype == ref[key].dtype and got[key].shape == ref[key].shape, (label, key)
        assert np.array_equal(got[key], ref[key]), (label, key)


@pytest.mark.parametrize("name", oc.GPU_SCENES)
def test_scene_against_the_restatement(eng, name):
    sc, im, pts, ref = oc.SCENES[name], oc.image(name), oc.points(name), oc.restated(name)
    passed, used = oc.pattern(name)
    k = tracker.Klt(eng, 8, sc["width"], im.shape[0], (3, 3), 0)
    try:
        k.describe_setup(sc["centroid"], sc["angle"], sc["edge"], passed, len(pts))      # (max_desc = n exactly: the block's end)
        k.push_image(im)                                                                # (the row stride of the array goes through)
        got = k.describe(pts, 1)
        print(name, "keypoints", len(pts), "kept", len(got["keep_idx"]), "mean bit", np.unpackbits(got["desc"]).mean())
        G, pat = k.describe_stage(1)
        assert np.array_equal(pat, used) and pat.dtype == np.int8
        assert G.dtype == np.uint8 and np.array_equal(G, ref["G"]), name
        check(got, ref, name)
        again = k.describe(pts, 1)                                                      # a repeated call is byte-equal
        for key in KEYS:
            assert got[key].tobytes() == again[key].tobytes(), key
    finally:
        k.close()


def test_slots_pushes_and_the_calls_around_a_description(eng):
    """which = 0 / 1 give the two images' results; after a further push the description is the new image's and the other slot's is
    unchanged (the blur flag stays with its slot across the swap); xk_trk_track and xk_trk_detect return the same bytes before and
    after a description on the same xk_trk."""
    name = kc.CHAIN
    sc = kc.SCENES[name]
    W, H = sc["size"]
    im1, im2 = kc.images(name)
    im3 = np.ascontiguousarray(fc.boxes_image(W, H, 55, 80))
    feats = kc.points(name)
    pat = onp.default_pattern()
    pts = oc.keypoints(W, H, 31, 65, 99)
    ref = [onp.describe(np.ascontiguousarray(im[:, :W]), pts, pat, 31, 1) for im in (im1, im2, im3)]
    assert not np.array_equal(ref[0]["desc"], ref[1]["desc"]) and not np.array_equal(ref[1]["desc"], ref[2]["desc"])
    k = tracker.Klt(eng, kc.MAX_FEATURES, W, H, sc["win"], sc["max_level"], sc["max_iter"], sc["eps"], sc["thr"])
    try:
        k.detect_setup(9, True, 4, 4, 2048)
        k.describe_setup(1, -1.0, 31, None, 128)
        k.push_image(im1)
        check(k.describe(pts, 1), ref[0], "first image, current")     # blurs slot A
        k.push_image(im2)
        track0, det0 = k.track(feats), [k.detect(w) for w in (0, 1)]
        check(k.describe(pts, 0), ref[0], "first image, previous")    # slot A's blur was carried across the swap
        check(k.describe(pts, 1), ref[1], "second image, current")
        for w in (0, 1, 0):
            check(k.describe(pts, w), ref[w], w)
        track1, det1 = k.track(feats), [k.detect(w) for w in (0, 1)]
        for key in track0:
            assert track0[key].tobytes() == track1[key].tobytes(), key
        for a, b in zip(det0, det1):
            assert a["xy"].tobytes() == b["xy"].tobytes() and a["score"].tobytes() == b["score"].tobytes() and a["n_candidates"] == b["n_candidates"]
        k.push_image(im3)                                              # overwrites slot A, whose flag was set: it must be cleared
        check(k.describe(pts, 1), ref[2], "third image, current")
        check(k.describe(pts, 0), ref[1], "second image, previous")
        assert np.array_equal(k.describe_stage(0)[0], ref[1]["G"]) and np.array_equal(k.describe_stage(1)[0], ref[2]["G"])
        k.push_image(im1)                                              # a push with no description in between, then the stage alone blurs
        assert np.array_equal(k.describe_stage(1)[0], ref[0]["G"]) and np.array_equal(k.describe_stage(0)[0], ref[2]["G"])
        check(k.describe(pts, 1), ref[0], "fourth push, current")
        check(k.describe(pts, 0), ref[2], "fourth push, previous")
    finally:
        k.close()


def test_chain_detect_describe_match(eng):
    """detect -> describe of the accepted pixels with margin >= edge keeps all of them; a scene and its copy shifted by (5, 3),
    described at correspondingly shifted keypoints, give equal descriptors, which place.Database.knn_match pairs at distance 0."""
    hp = oc.HOST
    a, b = oc.shifted_pair()
    H, W = a.shape
    dx, dy = oc.SHIFT
    k = tracker.Klt(eng, hp["max_features"], W, H, (3, 3), 0)
    db = place.Database(eng, place.load_vocabulary(), 0.0, max_desc=hp["max_features"])
    try:
        k.detect_setup(hp["threshold"], hp["nms"], hp["b"], max(hp["m"], hp["edge"]), hp["max_candidates"])
        k.describe_setup(hp["orientation"], hp["angle"], hp["edge"], None, hp["max_desc"])
        k.push_image(a)
        det = k.detect(1)
        assert len(det["xy"]) > 20
        da = k.describe(det["xy"], 1)
        assert np.array_equal(da["keep_idx"], np.arange(len(det["xy"])))
        ref = onp.describe(a, det["xy"], onp.default_pattern(), hp["edge"], hp["orientation"])
        check(da, ref, "detected")
        k.push_image(b)
        moved = det["xy"] + np.array([dx, dy], np.int32)
        d_b = k.describe(moved, 1)
        inside = d_b["keep_idx"]                                        # the shifted keypoints the second image's border keeps
        assert len(inside) > 20 and len(inside) < len(moved)
        assert np.array_equal(d_b["desc"], da["desc"][inside]) and np.array_equal(d_b["moments"], da["moments"][inside])
        assert len({d.tobytes() for d in da["desc"]}) == len(da["desc"])          # no two features share a descriptor
        idx, dist = db.knn_match(d_b["desc"], da["desc"])
        assert np.array_equal(idx[:, 0], inside) and not dist[:, 0].any() and np.all(dist[:, 1] > 0)
    finally:
        db.close()
        k.close()


def test_status_codes_and_what_a_setup_survives(eng):
    L = eng.L
    EINVAL, ECAP = 1, 6
    t = C.c_void_p()
    assert L.xk_trk_create(eng.h, C.c_int(8), C.c_double(1.0), C.c_double(1.0), C.c_double(0.0), C.c_double(0.0), C.c_double(0.0), C.byref(t)) == 0
    im = np.ascontiguousarray(oc.rects_image())
    H, W = im.shape
    MAXD = 16
    pts = np.ascontiguousarray(oc.keypoints(W, H, 25, 5, 7)[:MAXD])
    n = len(pts)
    ref = onp.describe(im, pts, onp.default_pattern(), 25, 1)
    assert 0 < len(ref["keep_idx"]) < n
    desc, keep, dirs, mom, nk = np.full((MAXD + 1, 32), 7, np.uint8), np.full(MAXD + 1, -7, np.int32), np.full((MAXD + 1, 2), -7, np.int32), \
        np.full((MAXD + 1, 2), -7, np.int32), C.c_int(-1)
    many = np.full((MAXD + 1, 2), 40, np.int32)
    good = np.ascontiguousarray(oc.corner_pattern())
    ptr = lambda a, ty: None if a is None else a.ctypes.data_as(ty)
    klt = lambda w=W, h=H: L.xk_trk_klt_setup(t, C.c_int(w), C.c_int(h), C.c_int(3), C.c_int(3), C.c_int(0), C.c_int(30), C.c_double(0.01), C.c_double(0.003))
    setup = lambda o=1, ang=-1.0, e=25, p=None, cap=MAXD, tt=t: L.xk_trk_describe_setup(tt, C.c_int(o), C.c_double(ang), C.c_int(e), ptr(p, c_sb), C.c_int(cap))
    push = lambda a=im: L.xk_trk_push_image(t, ptr(a, c_ub), C.c_int(a.shape[1]))

    def describe(which=1, p=pts, m=n, d=desc, ki=keep, di=dirs, mo=mom, c=nk, tt=t):
        return L.xk_trk_describe(tt, C.c_int(which), ptr(p, c_ip), C.c_int(m), ptr(d, c_ub), ptr(ki, c_ip), ptr(di, c_ip), ptr(mo, c_ip),
                                 None if c is None else C.byref(c))

    stage = lambda which=1, tt=t: L.xk_trk_describe_stage(tt, C.c_int(which), None, None)
    untouched = lambda: bool(np.all(desc == 7) and np.all(keep == -7) and np.all(dirs == -7) and np.all(mom == -7))

    def works(r=ref):
        desc[:], keep[:], dirs[:], mom[:] = 7, -7, -7, -7
        assert describe() == 0 and nk.value == len(r["keep_idx"])
        m = nk.value
        assert np.array_equal(desc[:m], r["desc"]) and np.array_equal(keep[:m], r["keep_idx"]) and np.array_equal(dirs[:m], r["dir"])
        assert np.array_equal(mom[:m], r["moments"])
        assert np.all(desc[m:] == 7) and np.all(keep[m:] == -7)                          # nothing past the kept rows
        return True

    try:
        assert setup() == EINVAL and b"xk_trk_describe_setup" in L.xk_last_error(eng.h)     # before xk_trk_klt_setup
        assert describe() == EINVAL and stage() == EINVAL
        assert klt() == 0
        assert describe() == EINVAL and stage() == EINVAL                                   # no description setup
        bad_coord, bad_pair = good.copy(), good.copy()
        bad_coord[200, 3] = 16
        bad_pair[255] = (3, -4, 3, -4)
        low = good.copy()
        low[17, 0] = -16
        for kw in (dict(o=2), dict(o=-1), dict(ang=float("nan")), dict(ang=float("inf")), dict(e=24), dict(e=4097), dict(cap=0), dict(cap=32769),
                   dict(p=bad_coord), dict(p=low), dict(p=bad_pair), dict(tt=None)):
            assert setup(**kw) == EINVAL, kw
        assert describe() == EINVAL
        assert setup() == 0
        assert describe() == EINVAL and b"pushed" in L.xk_last_error(eng.h)                 # no image yet
        assert stage() == EINVAL
        assert push() == 0
        assert describe(which=0) == EINVAL and stage(which=0) == EINVAL                     # the previous slot is still empty
        for kw in (dict(which=2), dict(which=-1), dict(d=None), dict(ki=None), dict(di=None), dict(mo=None), dict(c=None), dict(m=-1), dict(p=None),
                   dict(tt=None)):
            assert describe(**kw) == EINVAL, kw
        assert stage(which=2) == EINVAL
        assert untouched()
        assert describe(p=many, m=MAXD + 1) == ECAP and untouched() and nk.value == -1      # more keypoints than max_desc
        assert b"max_desc" in L.xk_last_error(eng.h)
        assert works() and stage() == 0
        assert describe(p=None, m=0) == 0 and nk.value == 0                                 # n = 0
        assert describe(p=np.ascontiguousarray(pts[[i for i in range(n) if i not in ref["keep_idx"]]]), m=n - len(ref["keep_idx"])) == 0 and nk.value == 0
        # a setup that is refused leaves the earlier one in place
        assert setup(e=24) == EINVAL and setup(p=bad_pair) == EINVAL and setup(cap=0) == EINVAL
        assert works()
        # a new setup takes effect: the fixed angle, a caller's pattern, the extremes of edge and max_desc
        assert setup(o=0, ang=37.0, p=good) == 0
        assert works(onp.describe(im, pts, good, 25, 0, 37.0))
        assert setup(e=4096, cap=32768) == 0 and describe() == 0 and nk.value == 0
        # a new xk_trk_klt_setup drops the description setup; one that is refused does not
        assert setup() == 0 and klt(w=15) == EINVAL and works()
        assert klt() == 0
        assert describe() == EINVAL and b"xk_trk_describe_setup" in L.xk_last_error(eng.h)
        assert stage() == EINVAL
        assert setup() == 0 and push() == 0 and works()
        # an image smaller than 2 edge + 1 keeps nothing, with XK_OK
        small = np.ascontiguousarray(im[:50, :50])
        assert klt(w=50, h=50) == 0 and setup() == 0 and push(small) == 0
        inside = np.array([[25, 25], [24, 25], [10, 10], [49, 49]], np.int32)
        assert describe(p=inside, m=4) == 0 and nk.value == 0
        assert klt(w=51, h=51) == 0 and setup() == 0 and push(np.ascontiguousarray(im[:51, :51])) == 0
        assert describe(p=inside, m=4) == 0 and nk.value == 1 and keep[0] == 0               # 2 edge + 1 keeps its centre
        assert np.array_equal(desc[0], onp.describe(im[:51, :51], inside, onp.default_pattern(), 25, 1)["desc"][0])
    finally:
        L.xk_trk_destroy(t)
