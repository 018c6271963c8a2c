"""The fleets and matches the covariance-intersection entries are tested on ENTRY BY ENTRY (not a test): the MSCKF-MSCKF block
(csrc/xk_ci.hip.h, csrc/xk_ci_api.hip.h: xk_triangulate_multi, xk_ci_gather, xk_msckf_feature in batch mode, xk_ci_project, xk_ci_hph,
xk_ci_combine, xk_small_gamma, xk_scale_blocks; msckf_update.cpp:96-279) on both of its routes -- the host-ABI entry xk_msckf_ci_track
and the device-resident round xk_ci_round_device -- and the SLAM-SLAM match (xk_slam_match; multi_slam_update.cpp:61-246).  Built once,
shared by the CPU file (test_ci_entry_cases.py: what each case must be, by the two CPU references alone) and the GPU file
(test_gpu_ci_entries.py).

A fleet is built the way ci_round_cases.fleet_case builds it -- agent r is synth.make_scenario(N, 8, M, seed=S + r,
agent_offset=0.03 r, landmarks=<agent 0's>, outlier_frac=0), the own agent is rank 1 % world, all 8 staged tracks are shared (8 is the
round's limit) -- with what those fleets never have: track lengths that differ per agent (down to L = 2), windows that are not full on
the own and on a matched side, SLAM features behind the pose columns (M > 0), a matched agent whose observations belong to another
landmark (the JOINT gate rejects what the own gate accepted), and 8 x 34 poses (a joint gate past the chi-square table).

Contract of a match dict (ref_np.msckf_ci_track, c_oracle.msckf_ci_track, engine.msckf_ci_track): q_list / p_list hold the agent's
VALID poses, n_poses_max is what its covariance is laid out for.

`prod_spread` and `pt_spread` are not free parameters: the largest disagreement of the two CPU references (the C oracle and
oracle/ref_np.py) over a case's tracks -- on the joint gamma and the basis-independent products H^T S^-1 H, H^T S^-1 res (prod_spread),
on the jointly triangulated point as feature_cases.point_error measures it (pt_spread) -- measured by test_ci_entry_cases.py, which also
checks the numbers recorded here.  The GPU is held to prod_tol = max(1000 prod_spread, 1e-12), never above the cap of
test_gpu_dense_ci.py (1e-7); pt_tol = max(1000 pt_spread, 1e-12) is what the wrong concatenation order must exceed on the CPU."""
import functools

import numpy as np

import feature_cases as fc
from x_multi_agent_amd import synth

K_TRACKS = 8                 # staged = shared: the round's limit
W = 0.04                     # the fixed weight of every other agent (searched weights have files of their own)
GAMMA_TOL = fc.GAMMA_TOL     # own gamma
REF_TOL = 1e-10              # the two references on a gamma
MARGIN = 1e-5                # no gamma this close (relative) to its threshold
# caps: what test_gpu_dense_ci.py asserts on the full, even fleets
PROD_CAP, PJ_TOL = 1e-7, 1e-14
HOST_P_TOL, HOST_CORR_TOL = 1e-8, 1e-7
ROUND_P_TOL, ROUND_CORR_TOL = 1e-8, 1e-6
SLAM_TOL = dict(gamma=1e-9, H=1e-12, res=1e-10, S=1e-10, P_j=1e-14, post=1e-9, corr=1e-8)

# windows: {rank: valid poses} (absent: full).  track_len: make_scenario's argument per agent -- "window": (3, n_poses of that agent);
# other_len: the length of every OTHER agent's tracks.  shift: added to the x coordinate of the other agents' observations of the ODD
# tracks (another landmark's observations under this track's id).  prod_spread / pt_spread: module docstring.
MS_CASES = {
    # n = 81 = 2 * 32 + 17; L_i differ per agent, L = 2 (d = 1) on matched sides and on the own side; feature columns and the 4 Mmax
    # payload offset
    "ragged_w3_N10_M2":         dict(world=3, N=10, M=2, seed=5212, track_len=(2, 10), prod_spread=2.1e-13, pt_spread=2.8e-15),
    # a matched agent AND the own agent with n_poses < N
    "short_windows_w2_N12":     dict(world=2, N=12, M=0, seed=5200, windows={1: 7, 0: 9}, track_len="window", prod_spread=7.8e-14,
                                     pt_spread=2.8e-15),
    # k = 7, m = 21: the 24-row stack of xk_ci_project; n = 54
    "limits_w8_N6_M1":          dict(world=8, N=6, M=1, seed=5200, track_len=(2, 6), prod_spread=3.3e-13, pt_spread=4.5e-16),
    # the joint gate rejects while the own gate passes, on the odd tracks: fused and rejected entries interleave
    "wrong_association_w2_N10": dict(world=2, N=10, M=0, seed=5300, other_len=3, shift=0.06, prod_spread=1.4e-13, pt_spread=3.8e-15),
    # n = 255: 8 chunks of xk_ci_hph, the last one 31 columns wide; its dynamic LDS at m n
    "wide_w2_N30_M20":          dict(world=2, N=30, M=20, seed=5200, track_len=(2, 30), prod_spread=4.0e-14, pt_spread=2.6e-15),
    # dof = 2 * 272 - 3 = 541: past the chi-square table (513 entries)
    "far_dof_w8_N34":           dict(world=8, N=34, M=0, seed=5200, prod_spread=2.9e-14, pt_spread=3.5e-16),
}
SENSITIVE = [c for c in MS_CASES if c != "far_dof_w8_N34"]


def prod_tol(c):
    return min(PROD_CAP, max(1000.0 * c["prod_spread"], 1e-12))


def pt_tol(c):
    return max(1000.0 * c["pt_spread"], 1e-12)


@functools.lru_cache(maxsize=None)
def fleet(name):
    """-> dict(world, N, M, K, rank, scs [the agents' scenario dicts], sc [the own one], tracks [per agent the list of its tracks]).
    Built once; callers do not write into it."""
    c = MS_CASES[name]
    world, N, M = c["world"], c["N"], c["M"]
    rank = 1 % world
    scs, lm = [], None
    for r in range(world):
        npz = c.get("windows", {}).get(r)
        tl = c.get("track_len")
        if tl == "window":
            tl = (3, N if npz is None else npz)
        if "other_len" in c and r != rank:
            tl = c["other_len"]
        sc = synth.make_scenario(N, K_TRACKS, M, seed=c["seed"] + r, agent_offset=0.03 * r, landmarks=lm, outlier_frac=0.0,
                                 n_poses=npz, track_len=tl)
        lm = sc["landmarks_true"] if lm is None else lm
        if "shift" in c and r != rank:
            off = sc["trk_off"]
            for j in range(1, K_TRACKS, 2):
                sc["obs_xy"][off[j]:off[j + 1], 0] += c["shift"]
        scs.append(sc)
    return dict(world=world, N=N, M=M, K=K_TRACKS, rank=rank, scs=scs, sc=scs[rank], tracks=[synth.tracks_as_list(s) for s in scs])


def matches_of(fl, j, n_poses_max=None):
    """The match dicts of shared track j, the other agents by rank.  n_poses_max: None = the contract (N); "list" = the wrong variant,
    the length of the agent's pose list."""
    return [dict(obs=fl["tracks"][r][j], q_list=fl["scs"][r]["C_q_G"], p_list=fl["scs"][r]["G_p_C"], P=fl["scs"][r]["P"],
                 n_poses_max=len(fl["scs"][r]["G_p_C"]) if n_poses_max == "list" else fl["N"])
            for r in range(fl["world"]) if r != fl["rank"]]


def lengths(fl, j):
    """-> (own L, sum of L over all agents) of shared track j."""
    return len(fl["tracks"][fl["rank"]][j]), sum(len(t[j]) for t in fl["tracks"])


def products(ci):
    """The basis-independent products of an entry dict(S, H, res): -> (H^T S^-1 H, H^T S^-1 res)."""
    Si = np.linalg.inv(ci["S"])
    return ci["H"].T @ Si @ ci["H"], ci["H"].T @ Si @ ci["res"]


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


def _entries(name, mod, n_poses_max=None):
    fl, sc = fleet(name), fleet(name)["sc"]
    return [mod.msckf_ci_track(fl["tracks"][fl["rank"]][j], sc["C_q_G"], sc["G_p_C"], sc["P"], fl["N"], sc["sigma_img"],
                               matches_of(fl, j, n_poses_max), W) for j in range(K_TRACKS)]


def _flat(name, outs, numpy_ref):
    """Both references' results in one form, per track: dict(own_inlier, own_gamma, own_chi, ci_gamma (None: own gate rejected),
    ci_chi, ci (None | dict(S, P_j, H, res)), gpf, verdict in {"own_rejected", "joint_rejected", "fused"})."""
    from oracle import ref_np
    fl, per = fleet(name), []
    for j, o in enumerate(outs):
        L, Ltot = lengths(fl, j)
        own_inl = bool(o["self"]["inlier"]) if numpy_ref else bool(o["self_inlier"])
        d = dict(own_inlier=own_inl, own_gamma=float(o["self"]["gamma"] if numpy_ref else o["self_gamma"]),
                 own_chi=ref_np.chi2inv(0.95, 2 * L - 3), ci_gamma=float(o["ci_gamma"]) if own_inl else None,
                 ci_chi=ref_np.chi2inv(0.95, 2 * Ltot - 3), ci=o["ci"], gpf=np.asarray(o["gpf"], float))
        d["verdict"] = "own_rejected" if not own_inl else ("fused" if o["ci"] is not None else "joint_rejected")
        per.append(d)
    return per


@functools.lru_cache(maxsize=None)
def ms_ref_np(name):
    """oracle/ref_np.py on the 8 shared tracks of a case, computed once (-> _flat's list)."""
    from oracle import ref_np
    return _flat(name, _entries(name, ref_np), True)


@functools.lru_cache(maxsize=None)
def ms_oracle(name):
    """The C oracle on the same tracks."""
    from oracle import c_oracle
    return _flat(name, _entries(name, c_oracle), False)


@functools.lru_cache(maxsize=None)
def ms_applied(name):
    """ref_np.apply_ci on every fused entry of ms_ref_np: -> per track None | (posterior, correction)."""
    from oracle import ref_np
    return [None if t["ci"] is None else ref_np.apply_ci(t["ci"]["P_j"], t["ci"]["H"], t["ci"]["res"], t["ci"]["S"])
            for t in ms_ref_np(name)]


def ms_list_length_variant(name):
    """The wrong contract restated on the CPU: the matched agents' attitude columns at 15 + 3 len(q_list) + 3 pos."""
    from oracle import ref_np
    return _flat(name, _entries(name, ref_np, "list"), True)


def point_error(fl, gpf, gpf_ref):
    """|gpf - gpf_ref| / |gpf_ref - p_last| (feature_cases.point_error for one point; p_last: the own agent's newest pose)."""
    return float(np.linalg.norm(gpf - gpf_ref) / np.linalg.norm(gpf_ref - fl["sc"]["G_p_C"][-1]))


def self_first_point(fl, j):
    """The wrong concatenation order restated on the CPU: the own observations FIRST, then the matched agents' (the reference puts the
    matched agents first and the own agent last, msckf_update.cpp:113-149).  -> the jointly triangulated point."""
    from oracle import ref_np
    q, p, o = [], [], []
    for r in [fl["rank"]] + [r for r in range(fl["world"]) if r != fl["rank"]]:
        t, s = fl["tracks"][r][j], fl["scs"][r]
        q += list(s["C_q_G"][len(s["C_q_G"]) - len(t):])
        p += list(s["G_p_C"][len(s["G_p_C"]) - len(t):])
        o += list(t)
    ivd, _ = ref_np.triangulate_gn(q, p, o)
    return ref_np.global_feature_position(ivd, q[-1], p[-1])


def unweighted_product(fl, j, ci):
    """The wrong S_ci restated on the CPU: H^T S^-1 H with the gate's unweighted S = sum_i H_i P_i H_i^T + sigma^2 I for the entry's S.
    The other agents' Jacobians are not part of an entry; what is needed of them is S_ci itself:
    S_ci - sigma^2 I = H P H^T / w0 + (sum_other H_i P_i H_i^T) / w."""
    k, sc = fl["world"] - 1, fl["sc"]
    w0 = 1.0 - k * W
    var, own = sc["sigma_img"] ** 2, ci["H"] @ sc["P"] @ ci["H"].T
    others = W * (ci["S"] - var * np.eye(len(own)) - own / w0)
    return products(dict(S=own + others + var * np.eye(len(own)), H=ci["H"], res=ci["res"]))[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# SLAM-SLAM matches (xk_multi_slam_match).  Own side N = 10, M = 6 (n = 93); other side N = 8, M = 3 (no = 72), 6 of its 8 window
# poses valid, its landmarks a reordered slice of the own ones: its feature 0 is the own feature 5, 1 is 2, 2 is 0 -- the ids differ
# across every match.  Anchors forced on each side into pose 0 and into the newest pose (the estimate keeps its error, as
# slam_rows_cases does it).
# ---------------------------------------------------------------------------------------------------------------------------------
SLAM_OWN = dict(N=10, M=6, seed=5400)
SLAM_OTHER = dict(N=8, M=3, n_poses=6, seed=5401, agent_offset=0.03, slice=(5, 2, 0))
SLAM_ANCHORS_OWN = {5: "oldest", 2: "newest"}      # own feature -> forced anchor
SLAM_ANCHORS_OTHER = {0: "newest", 1: "oldest"}
SIGMA_LANDMARK = 0.1
ASYM = 1e-9                  # added to ONE off-diagonal entry of the own prior inside a gathered block, not to its mirror image
# (own feature, other feature, ci_slam_w, asymmetric prior)
SLAM_MATCHES = [(5, 0, 0.02, False), (5, 0, 0.5, False), (5, 0, 0.98, False), (2, 1, 0.5, False), (0, 2, 0.02, False),
                (0, 2, 0.98, True), (2, 1, 0.5, True),
                (1, 0, 0.5, False), (3, 2, 0.5, False)]              # different landmarks
SLAM_TRUE = [m for m in SLAM_MATCHES if SLAM_OTHER["slice"][m[1]] == m[0]]


def _reanchor(sc, forced):
    feat, anchors = sc["slam_feat"].copy(), sc["slam_anchor_idxs"].copy()
    npz = len(sc["G_p_C"])
    for j, where in forced.items():
        a_new = npz - 1 if where == "newest" else 0

        def true_ivd(a):
            c = sc["R_true"][a].T @ (sc["landmarks_true"][j] - sc["p_true"][a])      # (K = 0: landmark j is SLAM feature j)
            return np.array([c[0] / c[2], c[1] / c[2], 1.0 / c[2]])
        err = true_ivd(int(anchors[j])) - feat[3 * j:3 * j + 3]
        feat[3 * j:3 * j + 3] = true_ivd(a_new) - err
        anchors[j] = a_new
    return dict(sc, slam_feat=feat, slam_anchor_idxs=anchors)


@functools.lru_cache(maxsize=None)
def slam_sides():
    """-> (own scenario, other scenario).  Built once; callers do not write into them."""
    own = synth.make_scenario(SLAM_OWN["N"], 0, SLAM_OWN["M"], seed=SLAM_OWN["seed"])
    lm = own["landmarks_true"][list(SLAM_OTHER["slice"])]
    oth = synth.make_scenario(SLAM_OTHER["N"], 0, SLAM_OTHER["M"], seed=SLAM_OTHER["seed"], n_poses=SLAM_OTHER["n_poses"],
                              agent_offset=SLAM_OTHER["agent_offset"], landmarks=lm)
    return _reanchor(own, SLAM_ANCHORS_OWN), _reanchor(oth, SLAM_ANCHORS_OTHER)


def slam_prior(own, fid, asym):
    """The own prior of a match; asym: ASYM added at (anchor position block row 1, feature block column 2) only."""
    if not asym:
        return own["P"]
    P = own["P"].copy()
    P[15 + 3 * int(own["slam_anchor_idxs"][fid]) + 1, 15 + 6 * own["n_poses_max"] + 3 * fid + 2] += ASYM
    return P


def slam_args(match, swap=False):
    """The argument list of multi_slam_match (ref_np, c_oracle and the engine take the same one) of a SLAM_MATCHES entry.
    swap: the roles exchanged -- the small agent matches against the large one (no > n)."""
    own, oth = slam_sides()
    fid, ofid, w, asym = match
    a = [own["C_q_G"], own["G_p_C"], own["slam_feat"], int(own["slam_anchor_idxs"][fid]), fid, slam_prior(own, fid, asym),
         own["n_poses_max"]]
    b = [oth["C_q_G"], oth["G_p_C"], oth["slam_feat"], int(oth["slam_anchor_idxs"][ofid]), ofid, oth["P"], oth["n_poses_max"]]
    return (b + a if swap else a + b) + [SIGMA_LANDMARK, w]


@functools.lru_cache(maxsize=None)
def slam_refs():
    """-> (ref_np's, the C oracle's) multi_slam_match dicts of SLAM_MATCHES, computed once."""
    from oracle import c_oracle, ref_np
    return [ref_np.multi_slam_match(*slam_args(m)) for m in SLAM_MATCHES], [c_oracle.multi_slam_match(*slam_args(m)) for m in SLAM_MATCHES]
