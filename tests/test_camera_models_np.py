"""The NumPy restatement of the tracker's camera models (tests/camera_models_np.py) checked on its own, the conditions
of every coefficient set and scene the GPU tests use (tests/camera_models_cases.py), and the three new entry points in the header and
in the cross-compiled library.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import camera_models_cases as cc
import camera_models_np as cnp
import fundamental_np as fnp

from x_multi_agent_amd import engine

ROOT = os.path.join(os.path.dirname(__file__), "..")
CAM_SYMBOLS = ("xk_trk_camera_model", "xk_trk_distort", "xk_trk_undistort_status")
# the prototype's step bounds (radial-tangential, equidistant) over the regular sets
STEP_BOUND = {cnp.RADTAN: 6, cnp.EQUIDISTANT: 4}


@pytest.mark.parametrize("name", cc.REGULAR)
def test_every_pixel_converges_and_round_trips(name):
    """20 000 uniform pixels.  The round trip's bar, 1e-12 px: a pixel is at most 900 from the origin, so an ulp of it is 1.1e-13 and
    the conditioning and the trip back to pixels round a handful of times."""
    model, k = cc.SETS[name]
    p = cc.draw(cc.N_DRAW)
    u, state, steps, detj = cc.restated_undistort(name, "draw")
    assert (state == cnp.CONVERGED).all()
    assert 1 <= steps.max() <= STEP_BOUND[model]
    assert np.isfinite(u).all() and (detj > 0.0).all()
    back = cnp.distort(u, cc.K, model, k)
    worst = float(np.abs(back - p).max())
    print(name, "steps", int(steps.max()), "min det J", float(detj.min()), "round trip [px]", worst, "bend [px]", float(np.abs(u - p).max()))
    assert worst <= 1e-12
    assert np.abs(u - p).max() > 5.0                          # the case is not trivial


def test_folding_set_leaves_a_few_pixels_invalid():
    model, k = cc.SETS["FOLDING"]
    p = cc.draw(cc.N_DRAW)
    u, state, steps, detj = cc.restated_undistort("FOLDING", "draw")
    bad = state == cnp.INVALID
    share = float(bad.mean())
    print("FOLDING: invalid share", share, "steps", int(steps.max()))
    assert 0.001 <= share <= 0.02
    assert u[bad].tobytes() == p[bad].tobytes()               # an invalid point keeps its distorted pixel
    assert np.isfinite(u).all() and np.isnan(detj[bad]).all() and (detj[~bad] > 0.0).all()
    back = cnp.distort(u[~bad], cc.K, model, k)
    assert np.abs(back - p[~bad]).max() <= 1e-12
    assert np.abs(u - p).max() > 5.0
    # the device test's points: few enough of them are invalid or near the fold
    state_g, detj_g = cc.restated_undistort("FOLDING")[1], cc.restated_undistort("FOLDING")[3]
    unsure = int(((state_g == cnp.INVALID) | (detj_g < cc.FOLD_DETJ)).sum())
    assert 0 < unsure <= 0.03 * len(state_g)


def test_forward_maps_against_their_formulas():
    """The forward maps once more, point by point in plain Python, on a few pixels."""
    fx, fy, cx, cy = cc.K
    pts = cc.gpu_points()[-9:]
    for name, (model, k) in cc.SETS.items():
        got = cnp.distort(pts, cc.K, model, k)
        for (u, v), g in zip(pts, got):
            x, y = (u - cx) / fx, (v - cy) / fy
            if model == cnp.RADTAN:
                k1, k2, p1, p2, k3 = tuple(k) + (0.0,) * (5 - len(k))
                r2 = x * x + y * y
                gain = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
                xd, yd = x * gain + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * gain + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
            else:
                r = np.hypot(x, y)
                th = np.arctan(r)
                s = th * (1 + k[0] * th ** 2 + k[1] * th ** 4 + k[2] * th ** 6 + k[3] * th ** 8) / r if r > 1e-8 else 1.0
                xd, yd = x * s, y * s
            assert abs(xd * fx + cx - g[0]) <= 1e-10 and abs(yd * fy + cy - g[1]) <= 1e-10, name
    # the Jacobian against central differences
    x, y = np.array([0.3, -0.5, 0.7]), np.array([0.2, 0.4, -0.1])
    k = cnp._coeffs(*cc.EUROC)
    a, b, c, d = cnp.radtan_jacobian(k, x, y)
    h = 1e-6
    fpx, fmx = cnp.radtan_forward(k, x + h, y), cnp.radtan_forward(k, x - h, y)
    fpy, fmy = cnp.radtan_forward(k, x, y + h), cnp.radtan_forward(k, x, y - h)
    for ana, num in ((a, (fpx[0] - fmx[0]) / (2 * h)), (b, (fpy[0] - fmy[0]) / (2 * h)), (c, (fpx[1] - fmx[1]) / (2 * h)), (d, (fpy[1] - fmy[1]) / (2 * h))):
        assert np.abs(ana - num).max() <= 1e-8


def test_edge_points():
    for name, (model, k) in cc.SETS.items():
        centre = np.array([[cc.K[2], cc.K[3]]])
        u, state, steps, _ = cnp.undistort(centre, cc.K, model, k)
        assert state[0] == cnp.CONVERGED and u.tobytes() == centre.tobytes(), name
        assert cnp.distort(centre, cc.K, model, k).tobytes() == centre.tobytes(), name
        assert steps[0] == (0 if model == cnp.EQUIDISTANT else 1)
        bad = np.array([[np.nan, 3.0], [np.inf, 1.0]])
        u, state, _, _ = cnp.undistort(bad, cc.K, model, k)
        assert (state == cnp.INVALID).all() and u.tobytes() == bad.tobytes(), name
        assert len(cnp.undistort(np.zeros((0, 2)), cc.K, model, k)[0]) == 0


@pytest.mark.parametrize("case", cc.FILTER_CASES)
def test_filter_scenes_meet_their_conditions(case):
    r = cc.restated_filter(*case)
    assert (r["states"] == cnp.CONVERGED).all()
    assert r["margin"] >= 1e-6 and r["kept"].all()
    assert 7 <= r["n_inliers"] < case[1]                      # something was kept and something removed
    dp, _ = cc.filter_scene(*case[:4], case[5])
    assert np.abs(dp - cnp.undistort(dp, cc.K, *cc.SETS[case[0]])[0]).max() > 5.0      # the lens matters on this scene


def test_entry_points_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "xk.h")).read()
    for name in CAM_SYMBOLS:
        assert re.search(r"^(?:int|void) " + name + r"\(", hdr, flags=re.M), name
        assert name in engine.SYMBOLS
    for macro, value in (("XK_CAM_FOV", 0), ("XK_CAM_RADTAN", 1), ("XK_CAM_EQUIDISTANT", 2)):
        assert re.search(r"^#define %s %d$" % (macro, value), hdr, flags=re.M), macro
    for path in (engine.LIB_PATH, engine.LAB_LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        for name in CAM_SYMBOLS:
            assert f" {name}\n" in syms, (path, name)
    # both kernels are in the gfx950 code object of the library
    blob = open(engine.LIB_PATH, "rb").read()
    for k in (b"xk_fund_undistort", b"xk_cam_distort"):
        assert k in blob
