"""The NumPy restatement of the essential-matrix RANSAC filter (tests/essential_np.py) checked on its own, and the
two new entry points in the header and in the cross-compiled library.  No GPU."""
import os
import re
import subprocess

import numpy as np

import essential_np as enp

from x_multi_agent_amd import engine, synth

ROOT = os.path.join(os.path.dirname(__file__), "..")


def test_sampler_pinned_and_on_the_projects_stream():
    assert enp.sample(0, 0, 10) == [8, 3, 0, 9, 1]
    assert enp.sample(1, 2, 300) == [121, 182, 136, 159, 130]
    # the same stream as synth.SplitMix: hypothesis h consumes values 5h ... 5h+4
    for seed, h, n in ((0, 0, 10), (1, 2, 300), (12345, 7, 5)):
        z = synth.SplitMix(seed).u64(5 * h + 5)[5 * h:]
        picks = []
        for k in range(5):
            r = ((int(z[k]) >> 32) * (n - k)) >> 32
            for p in sorted(picks):
                if r >= p:
                    r += 1
            picks.append(r)
        assert picks == enp.sample(seed, h, n)
        assert len(set(picks)) == 5 and all(0 <= p < n for p in picks)


def test_candidates_satisfy_the_constraints_and_their_five_points():
    """200 hypotheses of a noisy scene.  Bounds: the five points are met through the SVD null space alone, so at
    round-off (1e-12 on coordinates of order one); the cubic constraints pass through a 10 x 10 elimination and an
    eigen-decomposition whose condition numbers reach 1e5...1e6 on such samples, so eps * 1e6 with a decade to spare:
    1e-8 would be typical, 1e-6 is asserted (a unit-norm matrix that is not essential misses them by order one)."""
    cur_xy, rec_xy, _, _, K = enp.make_scene(120, 0.5, 0.25, 2)
    cur, rec = enp.normalise(cur_xy, *K), enp.normalise(rec_xy, *K)
    total = 0
    for h in range(200):
        s = enp.sample(0, h, len(cur))
        cands, lam = enp.solve5(cur[s], rec[s])
        assert len(cands) <= 10 and len(lam) == 10
        for E in cands:
            total += 1
            assert abs(np.linalg.norm(E) - 1.0) < 1e-12
            assert enp.constraint_residual(E) < 1e-6
            assert np.abs(np.einsum("pi,ij,pj->p", rec[s], E, cur[s])).max() < 1e-12
    assert total >= 200 * 2      # (the five-point problem has 2 to 10 real solutions, about 4.5 on average)


def test_planted_essential_matrix_is_among_the_candidates():
    """Exact fp64 projections of a planted motion: the planted E is one of the real solutions.  Bound: the solver's own
    accuracy on a well-separated root, eps * condition <= 1e-16 * 1e7."""
    rng = np.random.default_rng(5)
    for _ in range(10):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        ang = rng.uniform(0.05, 0.2)
        Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
        t = rng.normal(size=3)
        t *= rng.uniform(0.3, 0.9) / np.linalg.norm(t)
        X = np.stack([rng.uniform(-3, 3, 5), rng.uniform(-2, 2, 5), rng.uniform(4, 12, 5)], axis=1)
        Xr = X @ R.T + t
        cur, rec = X / X[:, 2:], Xr / Xr[:, 2:]
        E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
        E /= np.linalg.norm(E)
        cands, _ = enp.solve5(cur, rec)
        assert len(cands) >= 1
        assert min(enp.efro(E, c) for c in cands) < 1e-9


def test_ransac_recovers_a_planted_inlier_set():
    cur_xy, rec_xy, inl, E_true, K = enp.make_scene(40, 0.3, 0.0, 103)
    r = enp.ransac(cur_xy, rec_xy, *K, 1.0, 64, 0)
    assert np.array_equal(r["mask"].astype(bool), inl) and r["n_inliers"] == int(inl.sum())
    assert enp.efro(r["E"], E_true) < 1e-3       # (float32 pixels: 3e-5 px of rounding through a five-point sample)
    assert enp.ransac(cur_xy[:4], rec_xy[:4], *K)["n_inliers"] == 0


def test_entry_points_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "xk.h")).read()
    for name in ("xk_pr_essential_ransac", "xk_pr_essential_hypotheses"):
        assert re.search(r"^int " + name + r"\(xk_pr \*p,", hdr, flags=re.M), name
        assert name in engine.SYMBOLS
    assert hdr.count("place_recognition.cpp:269-281") >= 2
    syms = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True).stdout
    assert " xk_pr_essential_ransac\n" in syms and " xk_pr_essential_hypotheses\n" in syms
    # the three kernels are in the gfx950 code object of the library
    blob = open(engine.LIB_PATH, "rb").read()
    for k in (b"xk_ess_solve", b"xk_ess_score", b"xk_ess_mask"):
        assert k in blob
