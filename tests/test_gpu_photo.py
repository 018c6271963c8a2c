"""xk_trk_photo_* (csrc/xk_photo.hip.h) through tracker.Klt and the C ABI, against the NumPy restatement tests/photo_np.py on the
cases of tests/photo_cases.py: intensities (sums, counts and the fp64 quotient exact), the gain RANSAC (per-hypothesis inlier
counts, winner and support exact; the gains within the tolerance measured on the restatement), the parameter ring, the
correction (bit for bit, with the rebuilt pyramid and the blur of a later description), the per-frame call against the
composition of the restated steps, every status code and what a setup survives.  tests/test_photo_np.py verifies the
restatement and the cases without a GPU."""
import ctypes as C

import numpy as np
import pytest

import fast_cases as fc
import klt_cases as kc
import klt_np as knp
import orb_np as onp
import photo_cases as pc
import photo_np as pnp

from x_multi_agent_amd import engine, tracker

pytestmark = pytest.mark.gpu
c_ub, c_fp = tracker.c_ub, tracker.c_fp
c_ip, c_dp = engine.c_ip, engine.c_dp
XK_EINVAL, XK_ECAPACITY = 1, 6


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(4, 0, 4)
    yield e
    e.close()


def make(eng, size, max_features=512, win=(5, 5), max_level=1, **kw):
    return tracker.Klt(eng, max_features, size[0], size[1], win, max_level, **kw)


# ---- intensity ----
@pytest.mark.parametrize("kernel_size", pc.INT_KERNELS)
def test_intensity_on_both_planes(eng, kernel_size):
    im, pts = pc.int_image(), pc.int_points()
    other = np.ascontiguousarray(255 - im)
    k = make(eng, pc.INT_SIZE, 16)
    try:
        k.photo_setup(kernel_size, 0.0, 0.0, 8)
        k.push_image(other)
        k.push_image(im)
        for which, img in ((1, im), (0, other)):
            ref = pnp.intensity(img, pts, kernel_size)
            for plane in (0, 1):
                got = k.photo_intensity(pts, which, plane)
                print(kernel_size, which, plane, got[1], got[2])
                assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
                assert got[0].tobytes() == ref[0].tobytes()                      # the fp64 quotient, exactly
        assert k.photo_intensity(pts, 1, 0)[2][7] == 0                           # 40 pixels outside: count 0, value 0
        k.photo_correct(1)                                                      # the working plane differs from the raw one now
        w = pnp.intensity(pnp.correct(im, 1.0, 0.0), pts, kernel_size)
        got = k.photo_intensity(pts, 1, 1)
        assert np.array_equal(got[1], w[1]) and got[0].tobytes() == w[0].tobytes()
        assert np.array_equal(k.photo_intensity(pts, 1, 0)[1], pnp.intensity(im, pts, kernel_size)[1])
    finally:
        k.close()


# ---- gains ----
@pytest.fixture(scope="module")
def gk(eng):
    k = make(eng, (32, 32), 320)
    k.photo_setup(30, 0.02, 0.01, 256)
    yield k
    k.close()


def check_gains(got, ref, compare_ab):
    assert np.array_equal(got["support"], ref["support"])
    if compare_ab:
        assert pc.close(got["a_rel"], ref["a_rel"]) and pc.close(got["b_rel"], ref["b_rel"]), (got, ref)
        assert pc.close(got["frame_ab"], ref["frame_ab"]), (got["frame_ab"], ref["frame_ab"])


@pytest.mark.parametrize("n", pc.GAIN_N)
@pytest.mark.parametrize("n_hyp", pc.GAIN_HYP)
def test_gains_against_the_restatement(gk, n, n_hyp):
    o, p, r = pc.gain_case(n, n_hyp)
    gk.photo_reset()
    ring = [(1.0, 0.0)]
    ref = pnp.process_frame(ring, [(o, p)], [1], n_hyp, pc.RANSAC_SEED, 0.02, 0.01)
    got = gk.photo_gains(o, p, (1,), n_hyp, pc.RANSAC_SEED)
    ab, inl = gk.photo_hypotheses(0, 0, n_hyp)
    print(n, n_hyp, "support", got["support"], "winner", r["winner"], "a, b", got["a_rel"], got["b_rel"], "restated", r["a"], r["b"],
          "deviation", abs(got["a_rel"][0] - r["a"]) / abs(r["a"]), abs(got["b_rel"][0] - r["b"]) / abs(r["b"]))
    assert np.array_equal(inl, r["inliers"])                                     # per hypothesis, exactly
    assert ab.tobytes() == r["ab"].tobytes()                                     # four terms in the picks' order: the same operations
    best = int(np.argmax(inl))
    assert best == r["winner"] and got["support"][0] == r["support"] == inl[best]
    check_gains(got, ref, pc.strict(n, n_hyp))
    params = gk.photo_params()
    assert params.shape == (2, 2) and tuple(params[0]) == (1.0, 0.0)
    if pc.strict(n, n_hyp):
        assert pc.close(params[1], ring[1]) and params[1].tobytes() == got["frame_ab"][2:].tobytes()
    again = gk.photo_gains(o, p, (1,), n_hyp, pc.RANSAC_SEED)                    # the same seed: identical bytes (the ring has moved
    for key in ("a_rel", "b_rel", "support"):                                    # on, so only what does not depend on it)
        assert again[key].tobytes() == got[key].tobytes(), key
    ab2, inl2 = gk.photo_hypotheses(0, 0, n_hyp)
    assert ab2.tobytes() == ab.tobytes() and inl2.tobytes() == inl.tobytes()
    gk.photo_reset()
    third = gk.photo_gains(o, p, (1,), n_hyp, pc.RANSAC_SEED)
    assert third["frame_ab"].tobytes() == got["frame_ab"].tobytes() and gk.photo_params().tobytes() == params.tobytes()


def test_gains_small_group_all_outliers_and_the_ring(gk):
    gk.photo_reset()
    o, p, _ = pc.gain_data(4, 1)
    got = gk.photo_gains(o, p, (1,), 4, 0)                                       # n = 4: identity, support 0, the ring still advances
    assert (got["a_rel"][0], got["b_rel"][0], got["support"][0]) == (1.0, 0.0, 0)
    ref = pnp.process_frame([(1.0, 0.0)], [(o, p)], [1], 4, 0, 0.02, 0.01)
    assert got["frame_ab"].tobytes() == ref["frame_ab"].tobytes()                # no sum involved: the chain alone, exactly
    assert len(gk.photo_params()) == 2
    with pytest.raises(tracker.XkError) as e:
        gk.photo_hypotheses(0, 0, 1)                                             # a group of <= 4 has no hypotheses
    assert e.value.status == XK_EINVAL
    rng = np.random.default_rng(3)                                               # all outliers: no hypothesis has an inlier ...
    p = rng.uniform(0.1, 0.9, 40)
    o = p + rng.choice([-1.0, 1.0], 40) * rng.uniform(20.0, 30.0, 40) * np.arange(1, 41)
    r = pnp.gains_ransac(o, p, 16, 5)
    assert r["support"] == 0                                                     # (... in the restatement either)
    gk.photo_reset()
    got = gk.photo_gains(o, p, (1,), 16, 5)
    assert (got["a_rel"][0], got["b_rel"][0], got["support"][0]) == (1.0, 0.0, 0)
    assert np.array_equal(gk.photo_hypotheses(0, 0, 16)[1], np.zeros(16, np.int32))


def test_gains_three_groups_and_sixteen_calls(gk):
    gk.photo_reset()
    ring = [(1.0, 0.0)]
    cases = [pc.gain_case(n, 63) for n in (63, 64, 65)]
    for o, p, _ in cases:                                                        # three advancing calls
        pnp.process_frame(ring, [(o, p)], [1], 63, pc.RANSAC_SEED, 0.02, 0.01)
        gk.photo_gains(o, p, (1,), 63, pc.RANSAC_SEED)
    assert len(gk.photo_params()) == 4 and pc.close(gk.photo_params(), np.array(ring))
    groups = [(o, p) for o, p, _ in cases]
    ref = pnp.process_frame(ring, groups, [1, 2, 3], 63, pc.RANSAC_SEED, 0.02, 0.01)
    got = gk.photo_gains([g[0] for g in groups], [g[1] for g in groups], (1, 2, 3), 63, pc.RANSAC_SEED)
    print("three groups", got, ref["frame_ab"])
    check_gains(got, ref, True)
    for g in range(3):                                                           # group g drew from seed + g
        assert np.array_equal(gk.photo_hypotheses(g, 0, 63)[1], ref["ransac"][g]["inliers"])
    before = gk.photo_params()
    with pytest.raises(tracker.XkError) as e:                                    # beyond the ring: refused, the ring untouched
        gk.photo_gains(groups[0][0], groups[0][1], (len(before) + 1,), 63, 0)
    assert e.value.status == XK_EINVAL and gk.photo_params().tobytes() == before.tobytes()
    with pytest.raises(tracker.XkError):
        gk.photo_gains(groups[0][0], groups[0][1], (0,), 63, 0)
    gk.photo_reset()
    o, p, _ = pc.gain_data(5, 77, noise=5.0e-4, outliers=0.0)                    # five inliers: enough support to move the ring
    ring = [(1.0, 0.0)]
    for i in range(16):
        if i == 15:
            before = gk.photo_params()
        gk.photo_gains(o, p, (1,), 1, pc.RANSAC_SEED)
        pnp.process_frame(ring, [(o, p)], [1], 1, pc.RANSAC_SEED, 0.02, 0.01)
    after = gk.photo_params()
    assert before.shape == (15, 2) and after.shape == (15, 2)                    # stays at 15; the first entry is the second of before
    assert after[:14].tobytes() == before[1:].tobytes()
    print("ring after 16 calls, largest deviation from the restated ring", np.abs(after - np.array(ring)).max())
    assert len({tuple(r) for r in after}) == 15                                  # (the entries differ: the shift is visible)
    got = gk.photo_gains(o, p, (15,), 1, pc.RANSAC_SEED)                         # the oldest entry is still addressable
    assert got["support"][0] == 5


# ---- correction ----
@pytest.mark.parametrize("a,b,spatial", pc.COR_PAIRS)
def test_correction_bit_for_bit(eng, a, b, spatial):
    im = pc.cor_image()
    W, H = pc.COR_SIZE
    ps = pc.cor_spatial() if spatial else None
    k = make(eng, pc.COR_SIZE, 320, (3, 3), 2)
    try:
        k.photo_setup(4, 0.0, 0.0, 64)
        k.describe_setup(0, -1.0, 25, None, 16)
        k.push_image(im)
        k.describe_stage(1)                                                      # blurs the uncorrected image: the flag is set
        if (a, b) != (1.0, 0.0):
            # put (a, b) into the ring through the estimate itself: exact data of the pair o = p (a - b) + b, no drift terms
            p = np.linspace(0.1, 0.9, 64)
            got = k.photo_gains(p * (a - b) + b, p, (1,), 8, 1)
            assert got["support"][0] == 64
            a, b = k.photo_params()[-1]
        if spatial:
            k.photo_set_spatial(ps)
        ref = pnp.correct(im, float(a), float(b), ps)
        if (a, b) == (1.0, 0.0):
            assert np.array_equal(ref, pnp.LUT[im])                              # the table of the input
        elif not spatial:                                                        # negative and above-255 values: sign rule and wrap
            c = ((im.astype(np.float32) / np.float32(255)) * np.float32(a - b) + np.float32(b)) * np.float32(255)
            assert (c <= -1).any() and (c >= 256).any()
        k.photo_correct(1)
        pyr = knp.build_pyramid(ref, (3, 3), 2)
        assert k.levels() == len(pyr) - 1 == 2
        for l, (I, dx, dy) in enumerate(pyr):
            g = k.level(1, l)
            assert np.array_equal(g[0], I), ("image", l)                         # level 0: the corrected image, bit for bit
            assert np.array_equal(g[1], dx) and np.array_equal(g[2], dy), ("derivatives", l)
        assert np.array_equal(k.photo_raw(1), im)                                # the raw plane still holds the pushed bytes
        G, _ = k.describe_stage(1)
        assert np.array_equal(G, onp.blur(ref))                                  # the blur was redone on the corrected image
        k.photo_correct(1)                                                       # idempotent
        assert np.array_equal(k.level(1, 0)[0], ref) and np.array_equal(k.photo_raw(1), im)
        if spatial:
            k.photo_set_spatial(None)
            k.photo_correct(1)
            assert np.array_equal(k.level(1, 0)[0], pnp.correct(im, float(a), float(b)))
    finally:
        k.close()


def test_correction_of_an_odd_width(eng):
    """Width 41: the last group of a row is written byte by byte and the padding columns stay out of every load."""
    rng = np.random.default_rng(12)
    im = rng.integers(0, 256, (17, 41), dtype=np.uint8)
    ps = rng.uniform(-0.1, 0.1, (17, 41)).astype(np.float32)
    k = make(eng, (41, 17), 16, (5, 5), 1)
    try:
        k.photo_setup(4, 0.0, 0.0, 8)
        k.push_image(im)
        k.photo_set_spatial(ps)
        k.photo_correct(1)
        ref = pnp.correct(im, 1.0, 0.0, ps)
        for l, (I, dx, dy) in enumerate(knp.build_pyramid(ref, (5, 5), 1)):
            g = k.level(1, l)
            assert np.array_equal(g[0], I) and np.array_equal(g[1], dx) and np.array_equal(g[2], dy), l
    finally:
        k.close()


# ---- the per-frame chain ----
def test_calibrate_against_the_composed_restatement(eng):
    q = pc.FRAME
    im1, im2 = pc.frame_images()
    xy, val = pc.frame_features()
    (r0, ring0), (r1, ring1), (r2, ring2) = pc.frame_restated()
    k = make(eng, q["size"], 64, q["win"], q["max_level"], max_iter=q["max_iter"], eps=q["eps"], min_eig_thr=q["min_eig_thr"])
    try:
        k.photo_setup(q["kernel_size"], q["eps_gap"], q["eps_base"], 64)
        k.push_image(im1)
        k.push_image(im2)
        g0 = k.photo_calibrate(xy[:3], val[:3], q["n_hyp"], q["ransac_seed"])    # 3 features, no estimate yet: nothing happens
        assert not g0["estimated"] and len(g0["keep_idx"]) == 0
        assert k.photo_params().tobytes() == np.array(ring0).tobytes() and np.array_equal(k.level(1, 0)[0], im2)
        g1 = k.photo_calibrate(xy, val, q["n_hyp"], q["ransac_seed"])
        print("kept", len(g1["keep_idx"]), "of", len(xy), "support", g1["support"], "a, b", g1["a_rel"], g1["b_rel"], "restated", r1["a_rel"],
              r1["b_rel"], "frame", g1["frame_ab"], r1["frame_ab"])
        assert g1["estimated"]
        assert np.array_equal(g1["keep_idx"], r1["keep_idx"])
        assert np.array_equal(g1["sum"], r1["sum"]) and np.array_equal(g1["count"], r1["count"])
        assert g1["intensity"].tobytes() == r1["intensity"].tobytes()
        assert g1["support"] == r1["support"]
        assert np.array_equal(k.photo_hypotheses(0, 0, q["n_hyp"])[1], r1["ransac"]["inliers"])
        assert pc.close(g1["a_rel"], r1["a_rel"]) and pc.close(g1["b_rel"], r1["b_rel"]) and pc.close(g1["frame_ab"], r1["frame_ab"])
        params = k.photo_params()
        assert params.shape == (2, 2) and pc.close(params, np.array(ring1))
        # the image: corrected with the DEVICE's pair (the restated pair differs from it within the tolerance, and float32 hides it
        # or not); with the restated pair wherever the two give the same float32 gain and base
        img = k.level(1, 0)[0]
        assert np.array_equal(img, pnp.correct(im2, *params[-1]))
        if np.float32(params[-1][0] - params[-1][1]) == np.float32(ring1[-1][0] - ring1[-1][1]) and np.float32(params[-1][1]) == np.float32(ring1[-1][1]):
            assert np.array_equal(img, r1["image"])
        for l, (I, dx, dy) in enumerate(knp.build_pyramid(img, q["win"], q["max_level"])):
            g = k.level(1, l)
            assert np.array_equal(g[0], I) and np.array_equal(g[1], dx) and np.array_equal(g[2], dy), l
        assert np.array_equal(k.photo_raw(1), im2) and np.array_equal(k.photo_raw(0), im1)
        assert np.array_equal(k.level(0, 0)[0], im1)                             # the previous image's working plane is untouched
        g2 = k.photo_calibrate(xy[:3], val[:3], q["n_hyp"], q["ransac_seed"])    # 3 features after an estimate: the old pair corrects
        assert not g2["estimated"] and k.photo_params().tobytes() == params.tobytes()
        assert np.array_equal(k.level(1, 0)[0], img)
        k.push_image(im2)                                                        # a fresh image, 3 features: corrected with the old pair
        assert np.array_equal(k.level(1, 0)[0], im2)
        g3 = k.photo_calibrate(xy[:3], val[:3], q["n_hyp"], q["ransac_seed"])
        assert not g3["estimated"] and np.array_equal(k.level(1, 0)[0], img) and np.array_equal(k.photo_raw(1), im2)
        # the tracking that follows reads the working planes
        tr = k.track(xy)
        p_prev = knp.build_pyramid(img, q["win"], q["max_level"])
        ref = knp.track(p_prev, p_prev, xy, q["win"], q["max_iter"], q["eps"], q["min_eig_thr"])
        assert np.array_equal(tr["keep_idx"], ref["keep_idx"])
    finally:
        k.close()


# ---- arguments and lifetime ----
def test_arguments_and_lifetime(eng):
    L = eng.L
    im = pc.int_image()
    k = make(eng, pc.INT_SIZE, 8)
    try:
        p = k.p
        d, i4 = np.zeros(64), np.zeros(64, np.int32)
        dp, ip = d.ctypes.data_as(c_dp), i4.ctypes.data_as(c_ip)
        f = np.zeros(64, np.float32).ctypes.data_as(c_fp)
        buf = np.zeros(im.shape, np.uint8).ctypes.data_as(c_ub)
        n1 = C.c_int(0)
        one = np.ones(1, np.int32).ctypes.data_as(c_ip)                           # frame_back of one group
        zero = np.zeros(4, np.int32).ctypes.data_as(c_ip)                         # inputs (ip, dp take the outputs): a pixel, off
        k.push_image(im)
        k.push_image(im)
        before = [
            lambda: L.xk_trk_photo_intensity(p, 1, 0, zero, 1, dp, ip, ip),
            lambda: L.xk_trk_photo_gains(p, 1, zero, dp, dp, one, 1, C.c_ulong(0), dp, dp, ip, dp),
            lambda: L.xk_trk_photo_hypotheses(p, 0, 0, 0, dp, ip),
            lambda: L.xk_trk_photo_params(p, dp, dp, C.byref(n1)),
            lambda: L.xk_trk_photo_reset(p),
            lambda: L.xk_trk_photo_set_spatial(p, None),
            lambda: L.xk_trk_photo_correct(p, 1),
            lambda: L.xk_trk_photo_raw(p, 1, buf),
            lambda: L.xk_trk_photo_calibrate(p, f, dp, 4, 1, C.c_ulong(0), ip, dp, ip, ip, C.byref(n1), dp, dp, ip, dp, C.byref(n1)),
        ]
        for call in before:                                                      # every entry before the setup
            assert call() == XK_EINVAL
        for args in ((1, 0.0, 0.0, 8), (65, 0.0, 0.0, 8), (30, -0.1, 0.0, 8), (30, 0.0, 1.5, 8), (30, float("nan"), 0.0, 8), (30, 0.0, 0.0, 0),
                     (30, 0.0, 0.0, 4097)):
            assert L.xk_trk_photo_setup(p, C.c_int(args[0]), C.c_double(args[1]), C.c_double(args[2]), C.c_int(args[3])) == XK_EINVAL, args
        k.photo_setup(30, 0.0, 0.0, 8)
        assert np.array_equal(k.photo_raw(1), im) and np.array_equal(k.photo_raw(0), im)     # images pushed before the setup are raw too
        for call in before:
            assert call() == 0
        assert L.xk_trk_photo_intensity(p, 1, 0, zero, 9, dp, ip, ip) == XK_ECAPACITY          # n > max_matches
        assert L.xk_trk_photo_calibrate(p, f, dp, 9, 1, C.c_ulong(0), ip, dp, ip, ip, C.byref(n1), dp, dp, ip, dp, C.byref(n1)) == XK_ECAPACITY
        off = np.array([0, 9], np.int32)
        assert L.xk_trk_photo_gains(p, 1, off.ctypes.data_as(c_ip), dp, dp, one, 1, C.c_ulong(0), dp, dp, ip, dp) == XK_ECAPACITY
        assert L.xk_trk_photo_intensity(p, 2, 0, zero, 1, dp, ip, ip) == XK_EINVAL and L.xk_trk_photo_intensity(p, 1, 2, zero, 1, dp, ip, ip) == XK_EINVAL
        assert L.xk_trk_photo_gains(p, 15, zero, dp, dp, one, 1, C.c_ulong(0), dp, dp, ip, dp) == XK_EINVAL
        assert L.xk_trk_photo_gains(p, 1, zero, dp, dp, one, 9, C.c_ulong(0), dp, dp, ip, dp) == XK_EINVAL      # n_hyp > max_hyp
        assert L.xk_trk_photo_gains(p, 1, zero, dp, dp, zero, 1, C.c_ulong(0), dp, dp, ip, dp) == XK_EINVAL     # frame_back 0
        assert L.xk_trk_photo_correct(p, 2) == XK_EINVAL and L.xk_trk_photo_raw(p, 1, None) == XK_EINVAL
        k.photo_gains(np.zeros(4), np.zeros(4), (1,), 1, 0)                                  # the ring advances
        ring = k.photo_params()
        assert len(ring) >= 2
        assert L.xk_trk_photo_setup(p, C.c_int(1), C.c_double(0), C.c_double(0), C.c_int(8)) == XK_EINVAL   # a failed setup ...
        assert np.array_equal(k.photo_raw(1), im) and k.photo_params().tobytes() == ring.tobytes()   # ... leaves the old one, ring and all
        k.setup(pc.INT_SIZE[0], pc.INT_SIZE[1], (5, 5), 1)                                   # xk_trk_klt_setup drops the photo setup
        k.push_image(im)
        assert L.xk_trk_photo_raw(p, 1, buf) == XK_EINVAL and L.xk_trk_photo_correct(p, 1) == XK_EINVAL
    finally:
        k.close()


def test_without_a_photo_setup_nothing_changes(eng):
    """Two xk_trk on the chained scene of the tracking tests, one with a photo setup (and no correction): the same tracking and
    detection, byte for byte."""
    name = kc.CHAIN
    sc = kc.SCENES[name]
    W, H = sc["size"]
    im1, im2 = kc.images(name)
    feats = kc.points(name)
    out = []
    for photo in (False, True):
        k = tracker.Klt(eng, kc.MAX_FEATURES, W, H, sc["win"], sc["max_level"], sc["max_iter"], sc["eps"], sc["thr"])
        try:
            k.detect_setup(9, True, 4, 4, 2048)
            if photo:
                k.photo_setup(30, 0.0, 0.0, 64)
            k.push_image(im1)
            k.push_image(im2)
            out.append((k.track(feats), k.detect(1), [k.level(w, l) for w in (0, 1) for l in range(k.levels() + 1)]))
        finally:
            k.close()
    (t0, d0, l0), (t1, d1, l1) = out
    for key in t0:
        assert t0[key].tobytes() == t1[key].tobytes(), key
    assert d0["xy"].tobytes() == d1["xy"].tobytes() and d0["score"].tobytes() == d1["score"].tobytes()
    for a, b in zip(l0, l1):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


def test_replacing_each_setup_leaves_the_others_working(eng):
    """The detection, description and photo setups alive on one xk_trk while each is replaced by one of the same parameters: every
    entry returns the bytes it returned before.  By design one thing changes: a new photo setup starts its ring over at (1, 0).
    A new xk_trk_klt_setup then drops all three."""
    im = fc.dots_image()
    k = make(eng, (96, 48), 32, (5, 5), 0)
    setups = dict(detect=lambda: k.detect_setup(9, True, 5, 4, 2048), describe=lambda: k.describe_setup(0, -1.0, 25, None, 64),
                  photo=lambda: k.photo_setup(30, 0.0, 0.0, 8))

    def blobs(v):
        if isinstance(v, dict):
            return [blobs(v[key]) for key in sorted(v)]
        if isinstance(v, (tuple, list)):
            return [blobs(x) for x in v]
        return np.asarray(v).tobytes()

    def calls():
        det = k.detect(1)
        xy = det["xy"]
        return xy, blobs([det, k.describe(xy, 0), k.describe(xy, 1), k.track(xy.astype(np.float32)), k.photo_intensity(xy, 1, 0),
                          k.photo_intensity(xy, 1, 1), k.photo_raw(1), k.describe_stage(0), k.describe_stage(1)])

    try:
        for f in setups.values():
            f()
        k.push_image(im)
        k.push_image(im)
        o, p, _ = pc.gain_data(4, 1)
        k.photo_gains(o, p, (1,), 4, 0)                                          # the ring advances: two entries
        assert len(k.photo_params()) == 2
        xy, record = calls()
        assert len(xy) == len(fc.restated("dots")["xy"]) > 0                     # (the calls had something to return)
        for name, f in setups.items():
            f()
            assert calls()[1] == record, name
            assert len(k.photo_params()) == (1 if name == "photo" else 2), name
        assert k.photo_params().tobytes() == np.array([[1.0, 0.0]]).tobytes()   # the exception: the new photo setup's ring
        k.setup(96, 48, (5, 5), 0)
        for entry in (lambda: k.detect(1), lambda: k.describe(xy, 1), lambda: k.photo_raw(1)):
            with pytest.raises(tracker.XkError) as e:
                entry()
            assert e.value.status == XK_EINVAL
    finally:
        k.close()
