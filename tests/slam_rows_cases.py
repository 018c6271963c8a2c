"""The cases the two kernels that put a persistent feature's rows into the visual update are tested on (not a test): xk_slam_rows_body
(csrc/xk_feature.hip.h; slam_update.cpp:49-214: two rows per feature already in the state, gated at the 0.9 quantile of dof = 2 * track
size) and xk_msckf_slam_init (csrc/xk_slaminit.hip.h; msckf_slam_update.cpp:64-267: the projected rows of a track whose feature joins the
state this frame, and the column-space rows that initialise it).  Built once, shared by the CPU file (test_slam_rows_cases.py: what each
case must be, by the CPU references alone) and the GPU file (test_gpu_slam_rows.py: the kernels FEATURE BY FEATURE).

A SLAM case is synth.make_scenario with what it never produces put in afterwards: track sizes other than n_poses (a persistent feature's
track grows every frame without limit), features anchored in the newest pose (the `an == pos` branch, slam_update.cpp:120-131) and in
pose 0, gross outliers (0.6 added to z_last of every third feature), a feature behind the newest camera.  An MSCKF-SLAM case takes
make_scenario's full-window tracks and keeps the last L observations of each.

`row_spread` is not a free parameter: it is the largest element-wise disagreement of the two CPU references (the C oracle and
oracle/ref_np.py) on a feature's two rows [h | res], relative to the largest entry of h in that row -- measured by
test_slam_rows_cases.py, which also checks the number recorded here -- and the GPU is held to row_tol = max(1000 row_spread, 1e-12), the
rule of pt_spread / pt_tol in feature_cases.py."""
import functools
import warnings

import numpy as np

import feature_cases as fc
from x_multi_agent_amd import synth

GAMMA_TOL = fc.GAMMA_TOL
REF_TOL = 1e-10              # the two references (or one reference's spread) per feature on gamma
MARGIN = 1e-5                # no gamma this close (relative) to its threshold
SIZES = (1, 2, "n", 256, 257, 1000)          # "n": n_poses, what make_scenario gives every feature


def row_tol(c):
    return max(1000.0 * c["row_spread"], 1e-12)


# sizes: the track sizes, dealt out so that every size meets outliers and inliers (size of feature j: sizes[(j + j // len) % len]).
# outliers: z_last[j] += 0.6 for j % 3 == outliers (None: none); "gate": both verdicts must be well represented.
# newest / oldest: features re-anchored in the newest pose / in pose 0 (their inverse-depth state restated in that pose).
# behind: features whose estimated inverse depth is negated -- the estimated landmark lies behind the newest camera (c[2] < 0).  The
#   reference has no guard: the residual and the rows are finite and the gate decides.  behind_inlier: what both CPU references decide.
# row_spread: measured by test_slam_rows_cases.py (module docstring).
SLAM_CASES = {
    # the three launch forms of the mixed-size case: alone (K = 0), fused into xk_build_rows (K > 0, window <= 33), next to the packed
    # per-track kernel (K > 0, window > 33: 128-row slots)
    "sizes_alone":   dict(N=12, K=0, M=40, seed=7412, sizes=SIZES, outliers=0, gate=True, row_spread=5.7e-15),
    "sizes_fused":   dict(N=12, K=6, M=40, seed=7413, sizes=SIZES, outliers=0, gate=True, row_spread=3.8e-15),
    "sizes_packed":  dict(N=34, K=5, M=40, seed=7414, sizes=SIZES, outliers=0, gate=True, row_spread=3.6e-15),
    # the same features with the outliers on other slots: the second update of test_a_rejected_slot_keeps_nothing
    "sizes_moved":   dict(N=12, K=0, M=40, seed=7412, sizes=SIZES, outliers=1, gate=True, row_spread=2.8e-15),
    "anchors_short_window": dict(N=20, n_poses=14, K=0, M=45, seed=7421, sizes=("n",), outliers=0, gate=True,
                                 newest=(0, 1, 7, 20, 33, 44), oldest=(2, 3, 11, 30, 43), row_spread=4.3e-15),
    "tiles_m70_n33": dict(N=33, K=0, M=70, seed=7431, sizes=("n", 300), outliers=0, gate=True, newest=(31, 32, 63, 64, 69),
                          row_spread=2.4e-15),                                    # 2 M = 140: rows 63 | 64 and 127 | 128 are tile boundaries
    "tall_window_n34": dict(N=34, K=0, M=66, seed=7441, sizes=("n", 2), outliers=0, gate=True, oldest=(63, 64), row_spread=3.5e-15),   # 128-row slots
    "behind_camera": dict(N=12, K=0, M=40, seed=7451, sizes=("n",), outliers=None, gate=False, behind=(4, 17, 30),
                          behind_inlier=(0, 1, 0), row_spread=2.5e-15),
}
SLAM_GATE = [c for c, v in SLAM_CASES.items() if v["gate"]]


def _true_ivd(sc, j, a, K):
    c = sc["R_true"][a].T @ (sc["landmarks_true"][K + j] - sc["p_true"][a])
    return np.array([c[0] / c[2], c[1] / c[2], 1.0 / c[2]])


@functools.lru_cache(maxsize=None)
def slam_scenario(name):
    """The scenario dict of a SLAM case (built once; callers do not write into it)."""
    c = SLAM_CASES[name]
    N, K, M = c["N"], c["K"], c["M"]
    sc = synth.make_scenario(N, K, M, seed=c["seed"], n_poses=c.get("n_poses"))
    npz = len(sc["G_p_C"])
    feat, anchors, z = sc["slam_feat"].copy(), sc["slam_anchor_idxs"].copy(), sc["slam_z_last"].copy()
    for idxs, a_new in ((c.get("newest", ()), npz - 1), (c.get("oldest", ()), 0)):
        for j in idxs:                   # the estimate keeps its error: state = truth in the new anchor - (truth in the old one - state)
            err = _true_ivd(sc, j, int(anchors[j]), K) - feat[3 * j:3 * j + 3]
            feat[3 * j:3 * j + 3] = _true_ivd(sc, j, a_new, K) - err
            anchors[j] = a_new
    for j in c.get("behind", ()):
        assert anchors[j] != npz - 1
        feat[3 * j + 2] = -feat[3 * j + 2]
    if c["outliers"] is not None:
        z[c["outliers"]::3] += 0.6
    ns = len(c["sizes"])
    sizes = np.array([npz if s == "n" else s for s in (c["sizes"][(j + j // ns) % ns] for j in range(M))], dtype=np.int32)
    return dict(sc, slam_feat=feat, slam_anchor_idxs=anchors, slam_z_last=z, slam_track_sizes=sizes)


def slam_perturbed(sc, draw):
    """sc with slam_z_last, slam_feat and G_p_C moved by a relative fc.PERTURB_REL, signs from generator `draw`."""
    rng = np.random.default_rng(2000 + draw)
    out = dict(sc)
    for key in ("slam_z_last", "slam_feat", "G_p_C"):
        s = rng.integers(0, 2, size=sc[key].shape) * 2.0 - 1.0
        out[key] = sc[key] * (1.0 + fc.PERTURB_REL * s)
    return out


def _slam_args(sc):
    return (sc["C_q_G"], sc["G_p_C"], sc["slam_feat"], sc["slam_anchor_idxs"], sc["slam_track_sizes"], sc["slam_z_last"], sc["P"],
            sc["n_poses_max"], sc["sigma_img"])


def rows_per_feature(jac, res, inlier):
    """The references stack the ACCEPTED features' rows without gaps (slam_update.cpp:36-44); -> [M, 2, n + 1] = [h | res] of feature
    j at [j], NaN where it was rejected."""
    M, n = len(inlier), jac.shape[1]
    out = np.full((M, 2, n + 1), np.nan)
    r = 0
    for j in range(M):
        if inlier[j]:
            out[j, :, :n], out[j, :, n] = jac[r:r + 2], res[r:r + 2]
            r += 2
    return out


def row_error(got, ref):
    """Per feature: the largest element-wise |got - ref| over its two rows [h | res], each relative to the largest |h| of that row of
    ref (NaN where ref has no rows).  got, ref: [M, 2, n + 1]."""
    scale = np.abs(ref[:, :, :-1]).max(axis=2, keepdims=True)
    return (np.abs(got - ref) / scale).max(axis=(1, 2))


@functools.lru_cache(maxsize=None)
def slam_oracle(name):
    """The C oracle on a SLAM case, computed once: -> dict(inlier, gamma, rows [M, 2, n + 1] (NaN: rejected), chi [M] the thresholds)."""
    from oracle import c_oracle
    sc = slam_scenario(name)
    jac, res, _, info = c_oracle.slam_update(*_slam_args(sc))
    chi = np.array([c_oracle.chi2inv(0.9, 2 * int(s)) for s in sc["slam_track_sizes"]])
    return dict(inlier=info["inlier"], gamma=info["gamma"], rows=rows_per_feature(jac, res, info["inlier"]), chi=chi)


@functools.lru_cache(maxsize=None)
def slam_ref_np(name):
    """oracle/ref_np.py on a SLAM case, feature by feature -- the rows of the rejected ones too."""
    from oracle import ref_np
    sc = slam_scenario(name)
    M, n = len(sc["slam_anchor_idxs"]), sc["P"].shape[0]
    rows, gam, inl = np.zeros((M, 2, n + 1)), np.zeros(M), np.zeros(M, np.int32)
    for j in range(M):
        h, r, g, ok = ref_np.slam_process_one_track(sc["slam_track_sizes"][j], sc["slam_z_last"][j], j, sc["C_q_G"], sc["G_p_C"],
                                                    sc["slam_feat"], sc["slam_anchor_idxs"], sc["P"], sc["n_poses_max"],
                                                    sc["sigma_img"] ** 2)
        rows[j, :, :n], rows[j, :, n], gam[j], inl[j] = h, r, g, ok
    return dict(inlier=inl, gamma=gam, rows=rows)


def slam_verdicts_move(name):
    """Does any verdict of the C oracle move when the inputs move by a relative fc.PERTURB_REL?"""
    from oracle import c_oracle
    sc, ref = slam_scenario(name), slam_oracle(name)
    return any(not np.array_equal(c_oracle.slam_update(*_slam_args(slam_perturbed(sc, d)))[3]["inlier"], ref["inlier"])
               for d in range(fc.PERTURB_DRAWS))


def depth_in_newest_camera(sc):
    """c[2] of every feature's estimated landmark in the newest camera."""
    from oracle import ref_np
    Rn, pn = ref_np.quat_to_rot(sc["C_q_G"][-1]), sc["G_p_C"][-1]
    out = []
    for j, a in enumerate(sc["slam_anchor_idxs"]):
        al, be, rho = sc["slam_feat"][3 * j:3 * j + 3]
        gpf = ref_np.quat_to_rot(sc["C_q_G"][a]) @ np.array([al, be, 1.0]) / rho + sc["G_p_C"][a]
        out.append((Rn.T @ (gpf - pn))[2])
    return np.array(out)


# ---------------------------------------------------------------------------------------------------------------------------------
# MSCKF-SLAM tracks.  L: the tracks' lengths (each keeps the LAST L observations of a full-window track); the engine's n_feat_max
# is K2 = len(L).  outlier: (track, its second half moved by 30 sigma).  kind "stopped": the last two poses of the window are one pose
# (fc.STOPPED): the Gauss-Newton system of a 2-observation track is exactly singular.
# ---------------------------------------------------------------------------------------------------------------------------------
MS_CASES = {
    "short_n8":         dict(kind="well", N=8, L=(2, 3, 5), seed=7501),                     # L = 2: ONE projected row
    "second_pass_n34":  dict(kind="well", N=34, L=(32, 33, 34), seed=7502),                 # 2 L = 64, 66, 68: the wave's strided loops go round twice
    "slot128_n40":      dict(kind="well", N=40, L=(40, 40, 40), seed=7503),                 # 2 L - 3 = 77 rows: a 128-row slot
    "mixed_n12":        dict(kind="well", N=12, L=(2, 7, 12, 4, 9), seed=7504),
    "partial_full_n12": dict(kind="well", N=12, n_poses=9, L=(9, 9, 9), seed=7505),
    "partial_short_n12": dict(kind="well", N=12, n_poses=9, L=(3, 5, 8, 2), seed=7506),
    "outlier_n10":      dict(kind="well", N=10, L=(10, 8, 6), seed=7507, outlier=1),
    "stopped_n10":      dict(kind="stopped", N=10, L=(2, 6, 10), seed=7508),
}
MS_WELL = [c for c, v in MS_CASES.items() if v["kind"] == "well"]


@functools.lru_cache(maxsize=None)
def ms_scenario(name):
    """-> (scenario dict without tracks or SLAM features -- the window, and a prior with K2 free feature slots --, the MSCKF-SLAM tracks)."""
    c = MS_CASES[name]
    K2 = len(c["L"])
    gen = fc.stopped if c["kind"] == "stopped" else fc._CIRCLE
    with fc.poses_from(gen):
        sc = synth.make_scenario(c["N"], K2, K2, seed=c["seed"], n_poses=c.get("n_poses"), outlier_frac=0.0,
                                 err_scale=0.0 if c["kind"] == "stopped" else 1.0)
    if c["kind"] == "stopped":
        sc["C_q_G"][-1], sc["G_p_C"][-1] = sc["C_q_G"][-2], sc["G_p_C"][-2]
    tracks = [t[len(t) - L:].copy() for t, L in zip(synth.tracks_as_list(sc), c["L"])]
    if "outlier" in c:
        t = tracks[c["outlier"]]
        t[len(t) // 2:] += 30.0 * sc["sigma_img"]
    base = {k: sc[k] for k in ("C_q_G", "G_p_C", "P", "n_poses_max", "sigma_img")}
    base.update(trk_off=np.zeros(1, np.int32), obs_xy=np.zeros((0, 2)))
    return base, tracks


def _ms_one(sc, trk):
    from oracle import ref_np
    return ref_np.msckf_slam_process_one_track(trk, sc["C_q_G"], sc["G_p_C"], sc["P"], sc["n_poses_max"], sc["sigma_img"] ** 2)


@functools.lru_cache(maxsize=None)
def ms_oracle(name):
    """ref_np on an MSCKF-SLAM case, computed once: -> (per track: msckf_slam_process_one_track's dict, or None where it raises
    LinAlgError -- the exactly singular track of the stopped window --, ref_np.visual_update's dict on the tracks it serves)."""
    from oracle import ref_np
    sc, tracks = ms_scenario(name)
    per = []
    for t in tracks:
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                per.append(_ms_one(sc, t))
        except np.linalg.LinAlgError:
            per.append(None)
    served = [t for t, o in zip(tracks, per) if o is not None]
    upd = ref_np.visual_update([], sc["C_q_G"], sc["G_p_C"], sc["P"], sc["n_poses_max"], sc["sigma_img"], msckf_slam_tracks=served)
    return per, upd


def ms_spread(name):
    """ref_np against itself when obs and G_p_C move by a relative fc.PERTURB_REL (the stand-in for a second reference): -> (largest
    per-track relative change of gamma, whether any verdict or Gauss-Newton iteration count moved)."""
    sc, tracks = ms_scenario(name)
    per = ms_oracle(name)[0]
    sg, moved = 0.0, False
    for d in range(fc.PERTURB_DRAWS):
        rng = np.random.default_rng(3000 + d)
        psc = dict(sc, G_p_C=sc["G_p_C"] * (1.0 + fc.PERTURB_REL * (rng.integers(0, 2, size=sc["G_p_C"].shape) * 2.0 - 1.0)))
        for t, o in zip(tracks, per):
            po = _ms_one(psc, t * (1.0 + fc.PERTURB_REL * (rng.integers(0, 2, size=t.shape) * 2.0 - 1.0)))
            sg = max(sg, abs(po["gamma"] - o["gamma"]) / abs(o["gamma"]))
            moved |= po["inlier"] != o["inlier"] or po["gn_iters"] != o["gn_iters"]
    return sg, moved
