"""xk_trk_detect_setup / xk_trk_detect / xk_trk_detect_stage (csrc/xk_fast.hip.h) through tracker.Klt and the C ABI, against
the NumPy restatement tests/fast_np.py on every scene of tests/fast_cases.py: the score image, the sorted keys, the counts,
the accepted pixels and their scores, all bit for bit -- every quantity is an integer, there is no tolerance.  Then the two
slots, a repeated call, the tracking before and after a detection on the same xk_trk, every status code, and what a setup
survives.  tests/test_fast_np.py verifies the restatement and the scenes without a GPU."""
import ctypes as C

import numpy as np
import pytest

import fast_cases as fc
import fast_np as fnp
import klt_cases as kc

from x_multi_agent_amd import engine, tracker

pytestmark = pytest.mark.gpu
c_ub, c_fp = tracker.c_ub, tracker.c_fp
c_dp, c_ip = engine.c_dp, engine.c_ip
c_up = C.POINTER(C.c_uint)


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(4, 0, 4)
    yield e
    e.close()


def make(eng, name):
    sc = fc.SCENES[name]
    im = fc.image(name)
    k = tracker.Klt(eng, sc["max_features"], sc["width"], im.shape[0], (3, 3), 0)
    k.detect_setup(sc["threshold"], sc["nms"], sc["b"], sc["m"], sc["max_candidates"])
    return k, sc, im


def check(k, ref, got, label):
    S, keys = k.detect_stage()
    assert S.dtype == np.uint8 and np.array_equal(S, ref["S"]), label
    assert keys.dtype == np.uint32 and np.array_equal(keys, ref["keys"]), label
    assert got["n_candidates"] == ref["n_candidates"], label
    assert got["xy"].dtype == np.int32 and got["xy"].shape == ref["xy"].shape and np.array_equal(got["xy"], ref["xy"]), label
    assert np.array_equal(got["score"], ref["score"]), label


@pytest.mark.parametrize("name", fc.GPU_SCENES)
def test_scene_against_the_restatement(eng, name):
    k, sc, im = make(eng, name)
    try:
        k.push_image(im)                                     # (the row stride of the array goes through)
        ref = fc.restated(name)
        got = k.detect(1, sc["old"])
        print(name, "candidates", got["n_candidates"], "accepted", len(got["xy"]))
        check(k, ref, got, name)
        again = k.detect(1, sc["old"])                       # a repeated call is bit-equal
        for key in ("xy", "score"):
            assert got[key].tobytes() == again[key].tobytes(), key
        assert again["n_candidates"] == got["n_candidates"]
        check(k, ref, again, name)
    finally:
        k.close()


def test_both_slots_and_the_tracking_around_a_detection(eng):
    """which = 0 / 1 give the two images' results; xk_trk_track returns the same bytes before and after a detection on the same
    xk_trk (they share the handle's buffers and stream)."""
    name = kc.CHAIN
    sc = kc.SCENES[name]
    W, H = sc["size"]
    im1, im2 = kc.images(name)
    pts = kc.points(name)
    k = tracker.Klt(eng, kc.MAX_FEATURES, W, H, sc["win"], sc["max_level"], sc["max_iter"], sc["eps"], sc["thr"])
    try:
        k.detect_setup(9, True, 4, 4, 2048)
        k.push_image(im1)
        k.push_image(im2)
        before = k.track(pts)
        r = [fnp.detect(np.ascontiguousarray(im[:, :W]), 9, 1, 4, 4) for im in (im1, im2)]
        assert not np.array_equal(r[0]["xy"], r[1]["xy"])
        for which in (0, 1, 0):
            check(k, r[which], k.detect(which), which)
        after = k.track(pts)
        for key in before:
            assert before[key].tobytes() == after[key].tobytes(), key
        # the detected pixels are features the tracker can follow
        got = k.track(k.detect(0)["xy"].astype(np.float32))
        assert len(got["keep_idx"]) > 0
    finally:
        k.close()


def test_status_codes_and_what_a_setup_survives(eng):
    L = eng.L
    EINVAL, ECAP = 1, 6
    t = C.c_void_p()
    MAXM = 8
    assert L.xk_trk_create(eng.h, C.c_int(MAXM), C.c_double(1.0), C.c_double(1.0), C.c_double(0.0), C.c_double(0.0), C.c_double(0.0), C.byref(t)) == 0
    dots = np.ascontiguousarray(fc.dots_image())                                 # 96 x 48: 34 candidates; b = 5 accepts 18, b = 200 one
    H, W = dots.shape
    xy, score, nf, nc = np.full((MAXM, 2), -7, np.int32), np.full(MAXM, -7, np.int32), C.c_int(-1), C.c_int(-1)
    old = np.zeros((MAXM + 1, 2))
    ptr = lambda a, ty: None if a is None else a.ctypes.data_as(ty)
    klt = lambda w=W, h=H: L.xk_trk_klt_setup(t, C.c_int(w), C.c_int(h), C.c_int(3), C.c_int(3), C.c_int(0), C.c_int(30), C.c_double(0.01), C.c_double(0.003))
    setup = lambda thr=9, nms=1, b=200, m=4, cap=64, tt=t: L.xk_trk_detect_setup(tt, C.c_int(thr), C.c_int(nms), C.c_int(b), C.c_int(m), C.c_int(cap))
    push = lambda a=dots: L.xk_trk_push_image(t, ptr(a, c_ub), C.c_int(a.shape[1]))

    def detect(which=1, o=None, n_old=0, p=xy, s=score, f=nf, c=nc, tt=t):
        return L.xk_trk_detect(tt, C.c_int(which), ptr(o, c_dp), C.c_int(n_old), ptr(p, c_ip), ptr(s, c_ip),
                               None if f is None else C.byref(f), None if c is None else C.byref(c))

    stage = lambda tt=t: L.xk_trk_detect_stage(tt, None, None, None)
    untouched = lambda: bool(np.all(xy == -7) and np.all(score == -7))
    try:
        assert setup() == EINVAL and b"xk_trk_detect_setup" in L.xk_last_error(eng.h)      # before xk_trk_klt_setup
        assert detect() == EINVAL and stage() == EINVAL
        assert klt() == 0
        assert detect() == EINVAL and stage() == EINVAL                                     # no detection setup
        for kw in (dict(thr=0), dict(thr=255), dict(nms=2), dict(nms=-1), dict(b=-1), dict(b=4097), dict(m=-1), dict(m=4097), dict(cap=0),
                   dict(cap=32769), dict(tt=None)):
            assert setup(**kw) == EINVAL, kw
        assert detect() == EINVAL
        assert setup() == 0
        assert detect() == EINVAL and b"pushed" in L.xk_last_error(eng.h)                   # no image yet
        assert push() == 0
        assert detect(which=0) == EINVAL and stage() == EINVAL                              # the previous slot is still empty
        for kw in (dict(which=2), dict(which=-1), dict(p=None), dict(s=None), dict(f=None), dict(c=None), dict(n_old=-1), dict(o=None, n_old=1),
                   dict(tt=None)):
            assert detect(**kw) == EINVAL, kw
        assert untouched()
        assert detect(o=old, n_old=MAXM + 1) == ECAP and untouched()                        # more old features than max_matches
        assert detect() == 0 and (nf.value, nc.value) == (1, 34) and xy[0].tolist() == [fc.DOT_X0, fc.DOT_Y] and score[0] == 229
        assert stage() == 0
        # a setup that is refused leaves the earlier one in place
        assert setup(thr=0) == EINVAL and setup(cap=0) == EINVAL
        xy[:], score[:] = -7, -7
        assert detect() == 0 and (nf.value, nc.value) == (1, 34)
        # more accepted than max_matches: both counts true, the lists untouched
        assert setup(b=5) == 0
        assert stage() == EINVAL                                                            # a new setup: no detection yet
        xy[:], score[:] = -7, -7
        assert detect() == ECAP and (nf.value, nc.value) == (18, 34) and untouched()
        assert b"max_matches" in L.xk_last_error(eng.h)
        # more candidates than max_candidates: the true count, nothing selected, the lists untouched
        assert setup(cap=33) == 0
        assert detect() == ECAP and (nf.value, nc.value) == (0, 34) and untouched()
        assert b"max_candidates" in L.xk_last_error(eng.h)
        n = C.c_int(-1)
        assert L.xk_trk_detect_stage(t, None, None, C.byref(n)) == 0 and n.value == 34
        assert setup(cap=34, b=200) == 0 and detect() == 0 and (nf.value, nc.value) == (1, 34)
        # nothing found is XK_OK
        assert setup(thr=254) == 0 and detect() == 0 and (nf.value, nc.value) == (0, 0)
        assert push() == 0 and detect(which=0) == 0
        # a new xk_trk_klt_setup drops the detection setup; one that is refused does not
        assert setup() == 0 and klt(w=15) == EINVAL and detect() == 0 and nf.value == 1
        assert klt() == 0
        assert detect() == EINVAL and b"xk_trk_detect_setup" in L.xk_last_error(eng.h)
        assert stage() == EINVAL
        assert setup() == 0 and push() == 0 and detect() == 0 and nf.value == 1
    finally:
        L.xk_trk_destroy(t)
