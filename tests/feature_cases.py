"""The geometries the per-feature kernel (csrc/xk_feature.hip.h: DLT triangulation by one-sided Jacobi, Gauss-Newton with the reference's
lagging termination rule, Jacobians, observability constraint, null-space projection, Cholesky gate) is tested on besides the circle of
synth.true_poses (not a test): built once, shared by the CPU file (test_feature_cases.py: what each case must be, by the two CPU references
alone) and the GPU file (test_gpu_feature_geometry.py).

A case is synth.make_scenario with its landmarks=, track_len= and err_scale= arguments; the pose generator goes in by substituting
synth.true_poses for the duration of the call, so make_scenario's own random stream -- the golden vectors and bench.py depend on it -- is
the one it always was.  Generators keep true_poses' signature.

The tolerances of the triangulated point in CASES are not free parameters: `pt_spread` is the C oracle's own largest per-track change of the
point, |d gpf| / |gpf - p_last|, when obs_xy and G_p_C are perturbed by a relative 4e-16 (measured by test_feature_cases.py, which also
checks the number recorded here), and `pt_tol` = max(1000 pt_spread, 1e-12): a Jacobi null vector and LAPACK's differ by more than one
input ulp moves either of them."""
import contextlib
import functools

import numpy as np

from x_multi_agent_amd import synth

FPS = 30.0
PERTURB_REL = 4e-16          # relative size of the input perturbation the spreads are measured with
PERTURB_DRAWS = 4            # independent sign patterns; the spread is the largest over them
GAMMA_TOL = 1e-8             # the project's gamma bar, applied per track


def _wobble(t):
    """The small attitude motion synth.true_poses rides on its circle."""
    return synth._small_rot(np.array([0.02 * np.sin(3.0 * t), 0.015 * np.cos(2.5 * t), 0.01 * np.sin(1.7 * t)]))


def _axes_at(th):
    """Camera axes of synth.true_poses at angle th: optical axis radially outward."""
    zc = np.array([np.cos(th), np.sin(th), 0.0])
    xc = np.array([np.sin(th), -np.cos(th), 0.0])
    return np.column_stack([xc, np.cross(zc, xc), zc])


def forward(n_frames, phase0=0.3, agent_offset=0.0):
    """1 m/s ALONG the optical axis (the epipole in the middle of the image: landmarks near the axis have almost no parallax)."""
    th = phase0 + agent_offset
    R0 = _axes_at(th)
    Rs, ps = [], []
    for i in range(n_frames):
        t = i / FPS
        Rs.append(R0 @ _wobble(t))
        ps.append(np.array([5.0 * np.cos(th), 5.0 * np.sin(th), 1.5]) + 1.0 * t * R0[:, 2])
    return Rs, ps


def hover(amp):
    """A near-stationary camera: translation of size `amp` metres, rotation of +-0.2 rad (a vehicle holding position and looking around)."""
    def gen(n_frames, phase0=0.3, agent_offset=0.0):
        th = phase0 + agent_offset
        R0 = _axes_at(th)
        Rs, ps = [], []
        for i in range(n_frames):
            Rs.append(R0 @ synth._small_rot(0.2 * np.array([np.sin(1.1 * i), np.cos(0.9 * i), np.sin(0.5 * i + 1.0)])))
            ps.append(np.array([5.0 * np.cos(th), 5.0 * np.sin(th), 1.5]) + amp * np.array([np.sin(2.1 * i), np.cos(1.3 * i), np.sin(0.7 * i)]))
        return Rs, ps
    return gen


def stopped(n_frames, phase0=0.3, agent_offset=0.0):
    """The circle of synth.true_poses with a vehicle that stops: the last pose repeats the one before it."""
    Rs, ps = _CIRCLE(n_frames, phase0, agent_offset)
    Rs[-1], ps[-1] = Rs[-2].copy(), ps[-2].copy()
    return Rs, ps


def collapsed(n_frames, phase0=0.3, agent_offset=0.0):
    """Every pose of the window is the first one."""
    Rs, ps = _CIRCLE(1, phase0, agent_offset)
    return [Rs[0].copy() for _ in range(n_frames)], [ps[0].copy() for _ in range(n_frames)]


_CIRCLE = synth.true_poses
GENERATORS = {"circle": _CIRCLE, "forward": forward, "hover_1mm": hover(1e-3), "hover_1um": hover(1e-6), "stopped": stopped,
              "collapsed": collapsed}


@contextlib.contextmanager
def poses_from(gen):
    keep = synth.true_poses
    synth.true_poses = gen
    try:
        yield
    finally:
        synth.true_poses = keep


def landmarks_at_depth(gen, n_frames, count, lo, hi, seed):
    """`count` landmarks in the field of view of the middle camera of gen(n_frames), lo .. hi metres deep, laid out as make_scenario lays
    out its own (4 .. 20 m) but from a generator of their own."""
    Rs, ps = gen(n_frames)
    mid = n_frames // 2
    u = synth.SplitMix(0xD0000 + seed).uniform(3 * count).reshape(count, 3)
    depth = lo + (hi - lo) * u[:, 2]
    pc = np.column_stack([(u[:, 0] - 0.5) * depth, (u[:, 1] - 0.5) * 0.8 * depth, depth])
    return (Rs[mid] @ pc.T).T + ps[mid]


# kind "well": a well-conditioned family (every condition of test_feature_cases.test_well_conditioned holds, no track left out);
#      "micro": the deliberately near-degenerate one; "stopped": tracks of length 2 cannot be triangulated; "collapsed": no track can.
# pt_spread: measured by test_feature_cases.py (see the module docstring); pt_tol = max(1000 pt_spread, 1e-12).
# gamma_ref / pt_ref (micro only): the larger of the two reference disagreements of the family per track, on gamma and on the point --
#      C oracle against ref_np 9.8e-9 / 4.5e-8, spread 4.9e-8 / 2.6e-7 (measured and checked by test_feature_cases.py); the GPU bound is 100 x that.
CASES = {
    "circle":              dict(kind="well", gen="circle", N=10, K=40, seed=77, pt_spread=3.1e-14, pt_tol=3.1e-11),
    "forward":             dict(kind="well", gen="forward", N=10, K=40, seed=77, pt_spread=2.6e-13, pt_tol=2.6e-10),
    "forward_ragged_n30":  dict(kind="well", gen="forward", N=30, K=60, seed=77, track_len=(2, 30), pt_spread=1.4e-12, pt_tol=1.4e-9),
    "forward_ragged_n10":  dict(kind="well", gen="forward", N=10, K=40, seed=77, track_len=(2, 10), pt_spread=1.6e-12, pt_tol=1.6e-9),
    "forward_gate4_n40":   dict(kind="well", gen="forward", N=40, K=40, seed=77, track_len=(2, 40), pt_spread=3.7e-12, pt_tol=3.7e-9),
    "forward_gate4_n58":   dict(kind="well", gen="forward", N=58, K=40, seed=77, pt_spread=7.4e-15, pt_tol=7.4e-12),
    "hover_1mm_exact":     dict(kind="well", gen="hover_1mm", N=10, K=40, seed=77, err_scale=0.0, pt_spread=7.9e-9, pt_tol=7.9e-6),
    "hover_1mm_err":       dict(kind="well", gen="hover_1mm", N=10, K=40, seed=77, err_scale=0.01, pt_spread=2.3e-10, pt_tol=2.3e-7),
    "far_200_1000m":       dict(kind="well", gen="circle", N=10, K=40, seed=77, depth=(200.0, 1000.0), pt_spread=9.9e-13, pt_tol=9.9e-10),
    "near_0p3_1m":         dict(kind="well", gen="circle", N=10, K=40, seed=77, depth=(0.3, 1.0), pt_spread=1.1e-14, pt_tol=1.1e-11),
    "len2_circle":         dict(kind="well", gen="circle", N=10, K=40, seed=77, track_len=2, pt_spread=1.7e-12, pt_tol=1.7e-9),
    "len2_forward":        dict(kind="well", gen="forward", N=10, K=40, seed=77, track_len=2, pt_spread=2.2e-11, pt_tol=2.2e-8),
    "hover_1um":           dict(kind="micro", gen="hover_1um", N=10, K=40, seed=77, err_scale=0.0, gamma_ref=5.0e-8, pt_ref=2.7e-7),
    # failed triangulation, one case per compression schedule (test_gpu_feature_geometry.SCHEDULES)
    "stopped":             dict(kind="stopped", gen="stopped", N=10, K=40, seed=77, track_len=(2, 10), err_scale=0.0),
    "stopped_tall_n40":    dict(kind="stopped", gen="stopped", N=40, K=60, seed=79, track_len=(2, 40), err_scale=0.0),
    "stopped_small_k6":    dict(kind="stopped", gen="stopped", N=10, K=6, seed=92, track_len=(2, 10), err_scale=0.0, len2=2),
    "stopped_slam_n30":    dict(kind="stopped", gen="stopped", N=30, K=40, M=6, seed=78, track_len=(2, 30), err_scale=0.0),
    "collapsed":           dict(kind="collapsed", gen="collapsed", N=10, K=40, seed=77, track_len=(2, 10), err_scale=0.0),
}
WELL = [c for c, v in CASES.items() if v["kind"] == "well"]
STOPPED = [c for c, v in CASES.items() if v["kind"] == "stopped"]


@functools.lru_cache(maxsize=None)
def scenario(name):
    """The scenario dict of a case (built once; callers do not write into it)."""
    c = CASES[name]
    gen, N, K, M = GENERATORS[c["gen"]], c["N"], c["K"], c.get("M", 0)
    lm = None
    if "depth" in c:
        lm = landmarks_at_depth(gen, N, K + M, c["depth"][0], c["depth"][1], c["seed"])
    with poses_from(gen):
        sc = synth.make_scenario(N, K, M, seed=c["seed"], landmarks=lm, track_len=c.get("track_len"), err_scale=c.get("err_scale", 1.0))
    if c["kind"] == "stopped":       # (the estimate of a stopped vehicle: one pose twice, whatever the window error was)
        sc["C_q_G"][-1], sc["G_p_C"][-1] = sc["C_q_G"][-2], sc["G_p_C"][-2]
    elif c["kind"] == "collapsed":
        sc["C_q_G"][:], sc["G_p_C"][:] = sc["C_q_G"][0], sc["G_p_C"][0]
    return sc


def track_lengths(sc):
    return np.diff(sc["trk_off"]).astype(int)


def perturbed(sc, draw):
    """sc with obs_xy and G_p_C moved by a relative PERTURB_REL, signs from generator `draw`."""
    rng = np.random.default_rng(1000 + draw)
    out = dict(sc)
    for key in ("obs_xy", "G_p_C"):
        s = rng.integers(0, 2, size=sc[key].shape) * 2.0 - 1.0
        out[key] = sc[key] * (1.0 + PERTURB_REL * s)
    return out


def point_error(gpf, gpf_ref, sc):
    """Per track |gpf - gpf_ref| / |gpf_ref - p_last|: the error of the triangulated point against its distance from the anchor camera."""
    return np.linalg.norm(gpf - gpf_ref, axis=1) / np.linalg.norm(gpf_ref - sc["G_p_C"][-1], axis=1)


def per_track_rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)) / np.abs(b)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The C oracle on a case, computed once: -> (info of msckf_update: inlier, gamma, feats, gn_iters; visual_update's dict; the stacked
    rows H and residual of the accepted tracks and SLAM features, whose Gram products the compressed system must keep)."""
    from oracle import c_oracle
    sc = scenario(name)
    jac, res, _, info = c_oracle.msckf_update(sc)
    if "slam_anchor_idxs" in sc:
        js, rs, _, _ = c_oracle.slam_update(sc["C_q_G"], sc["G_p_C"], sc["slam_feat"], sc["slam_anchor_idxs"], sc["slam_track_sizes"],
                                            sc["slam_z_last"], sc["P"], sc["n_poses_max"], sc["sigma_img"])
        jac, res = np.vstack([jac, js]), np.concatenate([res, rs])
    return info, c_oracle.visual_update(sc), (jac, res)


def spreads(name):
    """The C oracle against itself under the input perturbation: -> (largest per-track relative change of gamma, of the point as
    point_error measures it, whether any verdict or Gauss-Newton iteration count moved)."""
    from oracle import c_oracle
    sc, info = scenario(name), oracle(name)[0]
    sg = sp = 0.0
    moved = False
    for d in range(PERTURB_DRAWS):
        _, _, _, pi = c_oracle.msckf_update(perturbed(sc, d))
        sg = max(sg, float(per_track_rel(pi["gamma"], info["gamma"]).max()))
        sp = max(sp, float(point_error(pi["feats"], info["feats"], sc).max()))
        moved |= not (np.array_equal(pi["inlier"], info["inlier"]) and np.array_equal(pi["gn_iters"], info["gn_iters"]))
    return sg, sp, moved
