"""The inputs and the CPU yardstick of the searched device CI round (not a test): built once, shared by the CPU and the GPU file.

A fleet is built the way test_gpu_dense_ci.test_device_ci_round_matches_host_abi_round builds it: agent r is
synth.make_scenario(N, 12, 0, seed=4100 + r, agent_offset=0.03 r, landmarks=<agent 0's>, outlier_frac=0), the own agent is rank
1 % world, three shared tracks, M = 0.  Optionally one track is corrupted on the own side (obs += 0.05 N(0, 1), generator seed 5) so
that its own chi-square gate rejects it.

The yardstick is oracle/ref_np.msckf_ci_track + ref_np.apply_ci in the reference's loop (every entry from the same prior, applyCI
overwrites), with ref_np.fuse_ci_msckf replaced by the formula at weights that are either given or searched by
tests/ci_weights_ref.py (info per agent, then solve)."""
import functools

import numpy as np

import ci_weights_ref as cw
from oracle import ref_np
from x_multi_agent_amd import synth

K_TRACKS_STAGED, M_SLAM, N_TRACKS = 12, 0, 3
# (world, N, corrupted track or None): the smallest shapes at which the batched projection can go wrong
SHAPES = [(2, 10, None),      # k1 = 2, m = 3; one factor launch, n = 75 is no multiple of 16
          (4, 10, 1),         # m = 9, rank-deficient M_i; a rejected track between two fused ones
          (8, 10, None),      # m = 21 and k1 = 8, the limits; 63 right-hand sides
          (2, 30, None),      # n = 195: two 192-row slabs with the Schur product, batched
          (3, 30, 2)]         # the same with three agents; the last track rejected
SHAPE_IDS = [f"w{w}_N{N}_c{c}" for w, N, c in SHAPES]


def info_solve(P, H):
    """The second CPU route to M = H P^-1 H^T: LAPACK's general solve instead of the Cholesky factor."""
    return H @ np.linalg.solve(P, H.T)


@functools.lru_cache(maxsize=None)
def fleet_case(world, N, corrupt):
    scs, lm = [], None
    for r in range(world):
        sc = synth.make_scenario(N, K_TRACKS_STAGED, M_SLAM, seed=4100 + r, agent_offset=0.03 * r, landmarks=lm, outlier_frac=0.0)
        lm = sc["landmarks_true"] if lm is None else lm
        scs.append(sc)
    rank = 1 % world
    if corrupt is not None:
        sc = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in scs[rank].items()}
        off = sc["trk_off"]
        rng = np.random.default_rng(5)
        sc["obs_xy"][off[corrupt]:off[corrupt + 1]] += 0.05 * rng.standard_normal((off[corrupt + 1] - off[corrupt], 2))
        scs[rank] = sc
    return dict(world=world, N=N, K=K_TRACKS_STAGED, M=M_SLAM, n_tracks=N_TRACKS, rank=rank, scs=scs, sc=scs[rank], corrupt=corrupt)


def packed(case):
    """-> (payloads [world, payload_doubles], tracks [world, n_tracks (1 + 2N)]) as the all-gather would leave them (host arrays)."""
    from x_multi_agent_amd import fleet
    dyn = np.zeros(16)
    dyn[9] = 1.0
    scs, N, M = case["scs"], case["N"], case["M"]
    pays = np.stack([fleet.pack_payload_host(r, 0.0, dyn, scs[r]["C_q_G"], scs[r]["G_p_C"], None, None, scs[r]["P"], N, M)
                     for r in range(case["world"])])
    trks = np.stack([fleet.pack_tracks(scs[r], case["n_tracks"], N).ravel() for r in range(case["world"])])
    return pays, trks


def others_of(case, pays=None, trks=None):
    """The received snapshots as fleet.ci_round takes them (host-ABI route)."""
    from x_multi_agent_amd import fleet
    if pays is None:
        pays, trks = packed(case)
    out = []
    for r in range(case["world"]):
        if r == case["rank"]:
            continue
        u = fleet.unpack_payload(pays[r], case["N"], case["M"])
        u["tracks"] = fleet.unpack_tracks(trks[r], case["N"])
        out.append(u)
    return out


def yardstick(case, weights=None, info=cw.info, start=None):
    """The reference's loop over the shared tracks on the CPU.
    weights: None = searched by ci_weights_ref (M_i through `info`, start point `start` or uniform); else per track the weight
    vector to use (own agent first, then the others by rank; the entry of a track that gives no entry is not looked at).
    -> dict(n_fused, rejected (set of track indices without an entry), P (the last fused posterior), corrections,
            tracks: {j: dict(Ps, Hs, M (through cw.info), w, iters)} for the fused tracks)"""
    scs, rank, sc, N = case["scs"], case["rank"], case["sc"], case["N"]
    tr = [synth.tracks_as_list(s) for s in scs]
    rec = {}
    state = {"j": None}

    def fuse(Pa, Ha, Pbs, Hbs, _w):
        j = state["j"]
        Ps, Hs = [Pa] + list(Pbs), [Ha] + list(Hbs)
        if weights is not None:
            w, it = np.asarray(weights[j], dtype=float), None
        else:
            w, it = cw.solve(np.array([info(P, H) for P, H in zip(Ps, Hs)]), start)
        assert len(w) == len(Ps), (j, w)
        rec[j] = dict(Ps=Ps, Hs=Hs, M=np.array([cw.info(P, H) for P, H in zip(Ps, Hs)]), w=w, iters=it)
        S = sum(H @ P @ H.T / wi for P, H, wi in zip(Ps, Hs, w))
        return S, 1.0 / w[0]

    keep = ref_np.fuse_ci_msckf
    ref_np.fuse_ci_msckf = fuse
    try:
        P_last, corrs, rejected = None, [], set()
        for j in range(case["n_tracks"]):
            state["j"] = j
            matches = [dict(obs=tr[r][j], q_list=scs[r]["C_q_G"], p_list=scs[r]["G_p_C"], P=scs[r]["P"], n_poses_max=N)
                       for r in range(case["world"]) if r != rank]
            o = ref_np.msckf_ci_track(tr[rank][j], sc["C_q_G"], sc["G_p_C"], sc["P"], N, sc["sigma_img"], matches, -1.0)
            if o["ci"] is None:
                rejected.add(j)
                continue
            c = o["ci"]
            P_last, corr = ref_np.apply_ci(c["P_j"], c["H"], c["res"], c["S"])
            corrs.append(corr)
    finally:
        ref_np.fuse_ci_msckf = keep
    return dict(n_fused=len(corrs), rejected=rejected, P=P_last, corrections=corrs, tracks=rec)


@functools.lru_cache(maxsize=None)
def searched(world, N, corrupt):
    """The yardstick with its own searched weights, through both CPU routes to M_i: -> (cw.info route, np.linalg.solve route)."""
    case = fleet_case(world, N, corrupt)
    return yardstick(case), yardstick(case, info=info_solve)
