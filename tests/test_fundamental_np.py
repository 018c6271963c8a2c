"""The NumPy restatement of the fundamental-matrix RANSAC filter of the tracker's matches (tests/fundamental_np.py)
checked on its own, the conditions of every scene the GPU tests use, and the six new entry points in the header and in
the cross-compiled library.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import fundamental_cases as fc
import fundamental_np as fnp

from x_multi_agent_amd import engine, synth

ROOT = os.path.join(os.path.dirname(__file__), "..")
K = fc.K
TRK_SYMBOLS = ("xk_trk_create", "xk_trk_destroy", "xk_trk_undistort", "xk_trk_fundamental_ransac",
               "xk_trk_fundamental_hypotheses", "xk_trk_filter_matches")


def test_sampler_on_the_projects_stream():
    # the same stream as synth.SplitMix: hypothesis h consumes values 7h ... 7h+6
    for seed, h, n in ((0, 0, 10), (1, 2, 300), (12345, 7, 7), (9, 4095, 512)):
        z = synth.SplitMix(seed).u64(7 * h + 7)[7 * h:]
        picks = []
        for k in range(7):
            r = ((int(z[k]) >> 32) * (n - k)) >> 32
            for p in sorted(picks):
                if r >= p:
                    r += 1
            picks.append(r)
        assert picks == fnp.sample(seed, h, n)
        assert len(set(picks)) == 7 and all(0 <= p < n for p in picks)
    assert sorted(fnp.sample(3, 5, 7)) == list(range(7))


def test_candidates_satisfy_their_seven_points_and_are_singular():
    """200 hypotheses of a noisy scene with outliers.  Bounds, unit-norm F on conditioned coordinates of order one:
    the seven points are met through the SVD null space alone -- nine products of round-off 1.1e-16 each, and the
    trip to pixel coordinates and back rescales entries without cancelling more than cx/fx -- so 1e-15 is typical and
    1e-12 is asserted; det F = 0 passes through the cubic's root, whose condition reaches 1e5 on near-double roots, so
    eps * 1e5 with a decade to spare: 1e-10 (a unit-norm matrix that is not singular misses by order 0.1)."""
    n, share, noise, _, scene_seed = fc.CANDIDATE_CASE
    p, c, _ = fc.pair(n, share, noise, scene_seed)
    P1, P2 = fnp.through_float(p), fnp.through_float(c)
    total = 0
    for h in range(200):
        s = fnp.sample(0, h, n)
        sol = fnp.solve7(fnp.condition(P1[s], K), fnp.condition(P2[s], K), K)
        assert 1 <= len(sol["cands"]) <= 3 and sol["general"]
        for F in sol["cands"]:
            total += 1
            assert abs(np.linalg.norm(F) - 1.0) < 1e-12
            assert fnp.sample_residual(F, P1, P2, K, s) < 1e-12
            assert abs(np.linalg.det(fnp.to_conditioned(F, K))) < 1e-10
    assert total >= 200 * 1.5        # (a real cubic has one or three real roots)


def test_ransac_recovers_planted_masks():
    n, share, noise, n_hyp, scene_seed = fc.PLANTED_CASE
    p, c, planted = fc.pair(n, share, noise, scene_seed)
    for seed in (0, 1, 2, 3):
        r = fc.restated(n, share, noise, n_hyp, scene_seed, seed)
        assert np.array_equal(r["mask"].astype(bool), planted) and r["n_inliers"] == int(planted.sum())
        assert np.array_equal((fnp.error(r["F"], fnp.through_float(p), fnp.through_float(c)) <= fc.THR ** 2), planted)
    assert fnp.ransac(p[:6], c[:6], K)["n_inliers"] == 0 and not fnp.ransac(p[:6], c[:6], K)["mask"].any()


def test_still_camera_keeps_every_pair():
    """Equal lists: the seven constraints are symmetric, every member of the null space is skew-symmetric, and p^T F p = 0."""
    p, c, _ = fc.pair(40, 0.0, 0.0, 5, "still")
    assert np.array_equal(p, c)
    r = fnp.ransac(p, c, K, fc.THR, 64, 0)
    assert r["n_inliers"] == 40 and r["mask"].all() and not r["kept"].any()      # (the all-singular rule: never `kept`)
    for cands in r["cands"]:
        assert len(cands) == 2


def test_rotation_only_and_collinear_scenes_stay_finite():
    p, c, _ = fc.pair(40, 0.0, 0.0, 5, "rotation")
    for a, b in ((p, c), fc.collinear_pair()):
        r = fnp.ransac(a, b, K, fc.THR, 64, 0)
        assert r["n_inliers"] == int(r["mask"].sum()) and np.isfinite(r["F"]).all()
        assert all(np.isfinite(cands).all() for cands in r["cands"])


def test_undistortion_inverts_the_generators_distortion():
    """atan then tan at arguments <= 0.9 (d tan <= 2.5), about ten operations of one ulp of a value <= 752 (1.1e-13) each:
    < 3e-12 px; 1e-11 asserted.  s = 0 is the identity on pixels; r <= 0.01 is left alone as the reference does."""
    rng = np.random.default_rng(3)
    xy = np.stack([rng.uniform(0, fnp.WIDTH, 500), rng.uniform(0, fnp.HEIGHT, 500)], axis=1)
    back = fnp.undistort(fnp.distort(xy, K, fc.S_FOV), K, fc.S_FOV)
    r = np.hypot((fnp.distort(xy, K, fc.S_FOV)[:, 0] - K[2]) / K[0], (fnp.distort(xy, K, fc.S_FOV)[:, 1] - K[3]) / K[1])
    assert np.abs(back - xy)[r > 0.01].max() < 1e-11
    assert np.abs(fnp.distort(xy, K, fc.S_FOV) - xy).max() > 5.0          # (the distortion is not a no-op: tens of pixels)
    assert np.abs(fnp.undistort(xy, K, 0.0) - xy).max() <= 1e-13          # ((u - cx)/fx fx + cx: one ulp of 752)
    centre = np.array([[K[2] + 1.0, K[3] - 2.0]])
    assert np.abs(fnp.undistort(centre, K, fc.S_FOV) - centre).max() <= 1e-13


@pytest.mark.parametrize("n,share,noise,n_hyp,scene_seed", fc.MASK_CASES)
def test_gpu_mask_scenes_meet_their_conditions(n, share, noise, n_hyp, scene_seed):
    r = fc.restated(n, share, noise, n_hyp, scene_seed)
    assert r["margin"] >= 1e-6 and r["kept"].all()
    assert r["winner"] >= 0 and r["n_inliers"] >= 7


def test_gpu_candidate_planted_and_distorted_scenes_meet_their_conditions():
    n, share, noise, n_hyp, scene_seed = fc.CANDIDATE_CASE
    assert fc.restated(n, share, noise, n_hyp, scene_seed)["kept"].mean() >= 0.95
    n, share, noise, n_hyp, scene_seed = fc.PLANTED_CASE
    for seed in (1, 2, 3):
        assert fc.restated(n, share, noise, n_hyp, scene_seed, seed)["margin"] >= 1e-6
    for case in fc.DISTORTED_CASES:
        r = fc.restated_filter(*case)
        assert r["margin"] >= 1e-6 and r["kept"].all()
        assert np.array_equal(r["keep_idx"], np.flatnonzero(r["mask"])) and len(r["prev_xy"]) == r["n_inliers"]
    r = fc.restated_filter(*fc.DISTORTED_CASE)
    assert np.array_equal(r["mask"].astype(bool), fc.pair(*fc.DISTORTED_CASE[:3], fc.DISTORTED_CASE[4], "general", fc.S_FOV)[2])


def test_entry_points_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "xk.h")).read()
    for name in TRK_SYMBOLS:
        assert re.search(r"^(?:int|void) " + name + r"\(", hdr, flags=re.M), name
        assert name in engine.SYMBOLS
    for path in (engine.LIB_PATH, engine.LAB_LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        for name in TRK_SYMBOLS:
            assert f" {name}\n" in syms, (path, name)
    # the four kernels are in the gfx950 code object of the library
    blob = open(engine.LIB_PATH, "rb").read()
    for k in (b"xk_fund_undistort", b"xk_fund_solve", b"xk_fund_score", b"xk_fund_mask"):
        assert k in blob
