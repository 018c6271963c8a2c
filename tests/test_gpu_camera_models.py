"""The radial-tangential and the equidistant camera model of the tracker on the device (xk_trk_camera_model, xk_trk_distort,
xk_trk_undistort_status; csrc/xk_camera.h) against their NumPy restatement (tests/camera_models_np.py) on the
coefficient sets and scenes of tests/camera_models_cases.py, whose conditions tests/test_camera_models_np.py asserts without a GPU.

The bar on a pixel is the project's 1e-12, relative to the point's distance from the pixel origin as in
test_gpu_fundamental.test_undistort_agrees_with_the_restatement, times max(1, 1 / min det J): Newton's fixed point amplifies the
round-off of the residual by the inverse Jacobian.  min det J is the restatement's, at its solutions (the equidistant model's
d theta_d / d theta stands in for it)."""
import ctypes as C

import numpy as np
import pytest

import camera_models_cases as cc
import camera_models_np as cnp
import fundamental_cases as fc
import fundamental_np as fnp

from x_multi_agent_amd import engine, tracker

pytestmark = pytest.mark.gpu
XK_EINVAL, XK_ECAPACITY = 1, 6
K = cc.K


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(4, 0, 4)
    yield e
    e.close()


@pytest.fixture(scope="module")
def filters(eng):
    made = {name: tracker.MatchFilter(eng, cc.MAX_MATCHES, K, model=model, coeffs=k) for name, (model, k) in cc.SETS.items()}
    yield made
    for mf in made.values():
        mf.close()


def rel_err(got, ref):
    return np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)


def bar_of(detj):
    return 1e-12 * max(1.0, 1.0 / float(np.nanmin(detj)))


@pytest.mark.parametrize("name", cc.REGULAR)
def test_undistort_and_distort_agree_with_the_restatement(filters, name):
    """500 random pixels, the principal point, a point on each axis and the four corners.  Measured on an MI355X, worst relative error
    of undistort / distort: EUROC 3.7e-15 / 4.1e-16 (bar 2.6e-12), BARREL 8.0e-16 / 3.2e-15, TUMVI 1.3e-15 / 5.0e-16 (bar 1e-12), KB
    1.5e-15 / 1.0e-15 (bar 1.16e-12); the device's largest step count equals the restatement's (6, 5, 3, 4)."""
    model, k = cc.SETS[name]
    mf = filters[name]
    p = cc.gpu_points()
    ref, state, steps, detj = cc.restated_undistort(name)
    bar = bar_of(detj)
    got = mf.undistort(p)
    n_invalid, max_steps = mf.undistort_status()
    worst_u = float(rel_err(got, ref).max())
    fwd_ref = cnp.distort(p, K, model, k)
    worst_d = float(rel_err(mf.distort(p), fwd_ref).max())
    print(name, "bar", bar, "undistort: worst relative error", worst_u, "distort:", worst_d, "steps", max_steps, "restated", int(steps.max()))
    assert worst_u <= bar and worst_d <= bar
    assert n_invalid == 0 and 1 <= max_steps <= int(steps.max()) + 1
    assert np.abs(got - p).max() > 5.0


def test_folding_set(filters):
    """Where the model folds inside the image.  Measured on an MI355X: worst relative error over the compared points 4.0e-15
    (bar 8.3e-12, min det J 0.12 among them); 6 of the 507 points invalid on the device and in the restatement; at most 7 steps."""
    mf = filters["FOLDING"]
    p = cc.gpu_points()
    ref, state, steps, detj = cc.restated_undistort("FOLDING")
    sure = (state == cnp.CONVERGED) & (detj >= cc.FOLD_DETJ)
    unsure = int((~sure).sum())
    assert unsure <= 0.03 * len(p)
    got = mf.undistort(p)
    n_invalid, max_steps = mf.undistort_status()
    bar = bar_of(detj[sure])
    worst = float(rel_err(got[sure], ref[sure]).max())
    print("FOLDING: bar", bar, "worst relative error", worst, "invalid", n_invalid, "restated", int((state == cnp.INVALID).sum()), "steps", max_steps)
    assert worst <= bar
    assert np.isfinite(got).all()
    # a point is either moved or, invalid, bit-equal to its input; the device's invalid points are among the latter
    same = (got.view(np.uint64) == p.view(np.uint64)).all(axis=1)
    centre = (p == np.array([K[2], K[3]])).all(axis=1)       # (the principal point maps to itself and is valid)
    assert int((same & ~centre).sum()) == n_invalid
    assert not (same & sure & ~centre).any()
    assert abs(n_invalid - int((state == cnp.INVALID).sum())) <= unsure
    assert n_invalid > 0 and 1 <= max_steps <= cnp.MAX_STEPS


@pytest.mark.parametrize("name", ["EUROC", "KB"])
def test_block_edges(filters, name):
    model, k = cc.SETS[name]
    mf = filters[name]
    p = cc.gpu_points()
    ref, _, steps, detj = cc.restated_undistort(name)
    bar = bar_of(detj)
    whole_u, whole_d = mf.undistort(p), mf.distort(p)
    for n in (0, 1, 255, 256, 257):
        u, st = mf.undistort(p[:n]), mf.undistort_status()
        d = mf.distort(p[:n])
        assert u.shape == d.shape == (n, 2)
        assert u.tobytes() == whole_u[:n].tobytes() and d.tobytes() == whole_d[:n].tobytes(), n
        if n:
            assert float(rel_err(u, ref[:n]).max()) <= bar
            assert st == (0, int(steps[:n].max())) or st == (0, int(steps[:n].max()) + 1), (n, st)
    # the two-list layout of xk_trk_filter_matches, 2 n points with n = 257: the kept pairs carry the device's own undistortion
    n = 257
    dp, dc = p[:n], p[-n:]
    mask, keep, pxy, cxy = mf.filter_matches(dp, dc, fc.THR, 16, 1)
    assert mf.undistort_status()[0] == 0
    und_p, und_c = mf.undistort(dp), mf.undistort(dc)
    assert pxy.tobytes() == und_p[keep].tobytes() and cxy.tobytes() == und_c[keep].tobytes()
    assert np.array_equal(keep, np.flatnonzero(mask))


def test_status_codes(eng, filters):
    L = eng.L
    p = cc.gpu_points()[:64]
    mf = tracker.MatchFilter(eng, 64, K, 0.0)
    try:
        mf.camera_model(*cc.SETS["EUROC"])
        before = mf.undistort(p)
        assert before.tobytes() == filters["EUROC"].undistort(p).tobytes()
        k5 = (C.c_double * 5)(*cc.SETS["EUROC"][1])
        nan5 = (C.c_double * 5)(0.1, float("nan"), 0.0, 0.0, 0.0)
        inf4 = (C.c_double * 4)(0.1, 0.0, float("inf"), 0.0)
        for model, coeffs, count in ((3, k5, 4), (-1, k5, 1), (0, k5, 0), (0, k5, 2), (1, k5, 3), (1, k5, 6), (2, k5, 5), (2, k5, 3),
                                     (1, nan5, 5), (2, inf4, 4), (0, (C.c_double * 1)(float("nan")), 1),
                                     (1, None, 4), (2, None, 4), (0, None, 1)):
            assert L.xk_trk_camera_model(mf.p, C.c_int(model), coeffs, C.c_int(count)) == XK_EINVAL, (model, count)
            assert b"xk_trk_camera_model" in L.xk_last_error(eng.h)
            assert mf.undistort(p).tobytes() == before.tobytes(), (model, count)      # the camera is what it was
        assert L.xk_trk_camera_model(None, C.c_int(1), k5, C.c_int(5)) == XK_EINVAL
        # xk_trk_distort: capacity and status rules of xk_trk_undistort
        out = np.zeros((80, 2))
        big = np.ascontiguousarray(cc.gpu_points()[:65])
        ptr = lambda a: a.ctypes.data_as(engine.c_dp)
        assert L.xk_trk_distort(mf.p, ptr(big), C.c_int(65), ptr(out)) == XK_ECAPACITY
        assert b"xk_trk_distort" in L.xk_last_error(eng.h)
        assert L.xk_trk_distort(mf.p, ptr(big), C.c_int(-1), ptr(out)) == XK_EINVAL
        assert L.xk_trk_distort(mf.p, None, C.c_int(4), ptr(out)) == XK_EINVAL
        assert L.xk_trk_distort(mf.p, ptr(big), C.c_int(4), None) == XK_EINVAL
        assert L.xk_trk_distort(None, ptr(big), C.c_int(4), ptr(out)) == XK_EINVAL
        assert L.xk_trk_distort(mf.p, None, C.c_int(0), None) == 0
        assert L.xk_trk_undistort_status(None, None, None) == XK_EINVAL
        assert L.xk_trk_undistort_status(mf.p, None, None) == 0                      # any output may be NULL
        steps = C.c_int(-1)
        assert L.xk_trk_undistort_status(mf.p, None, C.byref(steps)) == 0 and steps.value >= 1
        # the four-coefficient form is the five-coefficient one with k3 = 0
        mf.camera_model(*cc.SETS["BARREL"])
        four = mf.undistort(p)
        mf.camera_model(cnp.RADTAN, tuple(cc.SETS["BARREL"][1]) + (0.0,))
        assert mf.undistort(p).tobytes() == four.tobytes()
        assert mf.undistort_status()[0] == 0
        # XK_CAM_FOV through the new entry is the create-time camera, bit for bit, and reports zeros
        fov = tracker.MatchFilter(eng, 64, K, fc.S_FOV)
        try:
            mf.camera_model(tracker.CAM_FOV, (fc.S_FOV,))
            assert mf.undistort(p).tobytes() == fov.undistort(p).tobytes()
            assert mf.undistort_status() == (0, 0) and fov.undistort_status() == (0, 0)
            assert mf.distort(p).tobytes() == fov.distort(p).tobytes()
            back = fov.distort(fov.undistort(p))
            assert float(rel_err(back, p).max()) <= 1e-12
            dp, dc, _ = fc.pair(*fc.DISTORTED_CASE[:3], fc.DISTORTED_CASE[4], "general", fc.S_FOV)
            a, b = mf.filter_matches(dp[:64], dc[:64], fc.THR, 32, 2), fov.filter_matches(dp[:64], dc[:64], fc.THR, 32, 2)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a[1]) >= 7
        finally:
            fov.close()
    finally:
        mf.close()


@pytest.mark.parametrize("case", cc.FILTER_CASES)
def test_filter_on_distorted_pixels(filters, case):
    """xk_trk_filter_matches under the model against fundamental_np's filter fed the restatement's undistortion: under the
    restatement's conditions (margin >= 1e-6, every hypothesis kept; asserted in tests/test_camera_models_np.py) the mask bit for bit."""
    name, n, share, noise, n_hyp, scene_seed = case
    mf = filters[name]
    dp, dc = cc.filter_scene(name, n, share, noise, scene_seed)
    ref = cc.restated_filter(*case)
    assert ref["margin"] >= 1e-6 and ref["kept"].all()
    mask, keep, pxy, cxy = mf.filter_matches(dp, dc, fc.THR, n_hyp, cc.FILTER_SEED)
    assert mf.undistort_status()[0] == 0
    assert mask.tobytes() == ref["mask"].tobytes()
    assert np.array_equal(keep, ref["keep_idx"]) and 7 <= len(keep) < n
    und_p, und_c = mf.undistort(dp), mf.undistort(dc)
    assert pxy.tobytes() == und_p[keep].tobytes() and cxy.tobytes() == und_c[keep].tobytes()
    detj = np.concatenate([cnp.undistort(d, K, *cc.SETS[name])[3] for d in (dp, dc)])
    assert float(max(rel_err(pxy, ref["prev_xy"]).max(), rel_err(cxy, ref["cur_xy"]).max())) <= bar_of(detj)
