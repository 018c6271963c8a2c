"""Parity of the HIP path (through the C ABI, libxk.so) with the CPU oracle and the
golden vectors.  Tolerance: north_star asks <= 1e-6 relative Frobenius on P; the
tests hold the GPU path to 1e-9 (TOL_TIGHT) on the small cases and 1e-8 at full size."""
import numpy as np
import pytest

from helpers import TOL_NORTH_STAR, TOL_TIGHT, VISUAL_CASES, check_gamma_per_track, check_visual, load_case, rel
from x_multi_agent_amd import synth

pytestmark = pytest.mark.gpu


def _engine(xk, sc):
    N = sc["n_poses_max"]
    K = len(sc["trk_off"]) - 1
    M = len(sc["slam_anchor_idxs"]) if "slam_anchor_idxs" in sc else 0
    return xk.Engine(N, M, max(K, 1))


@pytest.mark.parametrize("name", VISUAL_CASES)
def test_golden_vectors(xk, name):
    sc, exp = load_case(name)
    eng = _engine(xk, sc)
    got = eng.visual_update(sc)
    rp, rc = check_visual(got, exp, tol=TOL_TIGHT)
    assert rp <= TOL_NORTH_STAR
    eng.close()


@pytest.mark.parametrize("name", VISUAL_CASES[:4])
def test_stage_by_stage_matches_golden(xk, name):
    """xk_msckf_build -> xk_qr_compress -> xk_apply_update, checking the basis-independent
    products T^T T, T^T z of the compressed system."""
    sc, exp = load_case(name)
    eng = _engine(xk, sc)
    eng.stage(sc)
    b = eng.msckf_build(sc["sigma_img"])
    assert np.array_equal(b["inlier"], exp["inlier"])
    T, z = eng.qr_compress()
    assert np.abs(np.tril(T[:, 15:], -1)).max() == 0.0 and np.abs(T[:, :15]).max() == 0.0
    assert rel(T.T @ T, exp["HtH"]) <= 1e-10
    assert rel(T.T @ z, exp["Htr"]) <= 1e-10
    corr = eng.apply_update()
    P = eng.download_P()
    assert rel(P, exp["P"]) <= TOL_TIGHT and rel(corr, exp["correction"]) <= 1e-8
    eng.close()


@pytest.mark.parametrize("cfg", [2, 4, 3])
def test_compression_keeps_the_gram_matrix_to_rounding(xk, oracle_c, cfg):
    """the reflector scalar chain runs ONE Newton step after v_rsq_f64 / v_rcp_f64 (~4e-15 per reflector, not
    1 ulp).  What that may cost is orthogonality of the accumulated Q, i.e. R^T R drifting from A^T A over the several hundred
    reflectors a column sees in three tree levels.  Pinned on the widest systems -- config 2 (331 columns, single launch, wide
    geometry), the headline (narrow geometry), config 3 (316 columns, 39 launches): ||T^T T - H^T H|| / ||H^T H|| with H the
    C oracle's stacked rows (its own rounding included) stays at a few 1e-14."""
    sc = synth.make_config(cfg)
    N, K = sc["n_poses_max"], len(sc["trk_off"]) - 1
    M = len(sc["slam_anchor_idxs"]) if "slam_anchor_idxs" in sc else 0
    eng = xk.Engine(N, M, K)
    eng.stage(sc)
    b = eng.msckf_build(sc["sigma_img"])
    T, z = eng.qr_compress()
    eng.close()
    jac, res, _, info = oracle_c.msckf_update(sc)
    assert np.array_equal(b["inlier"], info["inlier"])
    if M:
        js, rs, _, _ = oracle_c.slam_update(sc["C_q_G"], sc["G_p_C"], sc["slam_feat"], sc["slam_anchor_idxs"], sc["slam_track_sizes"],
                                            sc["slam_z_last"], sc["P"], N, sc["sigma_img"])
        jac, res = np.vstack([jac, js]), np.concatenate([res, rs])
    G = jac.T @ jac
    eg, ez = rel(T.T @ T, G), rel(T.T @ z, jac.T @ res)
    print(f"config {cfg}: rel |T^T T - H^T H| = {eg:.2e}, rel |T^T z - H^T r| = {ez:.2e}")
    assert eg <= 5e-13 and ez <= 5e-12, (eg, ez)


CASES_VS_ORACLE = {
    "cfg1": lambda: synth.make_config(1),
    "cfg2_msckf_slam": lambda: synth.make_config(2),
    "cfg4_headline": lambda: synth.make_config(4),
    "cfg4_agent3": lambda: synth.make_config(4, agent_id=3),
    "ragged_n30": lambda: synth.make_scenario(30, 150, 0, seed=901, track_len=(2, 30)),
    "len2_tracks": lambda: synth.make_scenario(10, 20, 0, seed=902, track_len=2),
    "window_not_full": lambda: synth.make_scenario(30, 100, 10, seed=903, n_poses=17),
    "large_prior": lambda: synth.make_scenario(30, 200, 0, seed=904, prior_scale=100.0),
    "max_window_n64": lambda: synth.make_scenario(64, 40, 0, seed=905),
    # CAQR tree shapes: one tile, exactly one / one-and-a-bit merge groups, the 40-way first level (> 400 tiles),
    # and a stack where most tiles are rejected (all-zero tiles inside the merge groups)
    "caqr_1_tile": lambda: synth.make_scenario(8, 1, 0, seed=906, outlier_frac=0.0),
    "caqr_20_tiles": lambda: synth.make_scenario(8, 20, 0, seed=907),
    "caqr_21_tiles": lambda: synth.make_scenario(8, 21, 0, seed=908),
    "caqr_401_tiles": lambda: synth.make_scenario(8, 401, 0, seed=909),
    "caqr_450_tiles_40way": lambda: synth.make_scenario(10, 450, 0, seed=910),
    "caqr_1700_tiles_three_levels": lambda: synth.make_scenario(3, 1700, 0, seed=71),
    "caqr_mostly_rejected": lambda: synth.make_scenario(12, 120, 0, seed=911, outlier_frac=0.7),
    # SLAM rows only / SLAM-dominated stacks, and the two tile heights either side of the 64-row boundary
    "slam_only_m5": lambda: synth.make_scenario(8, 0, 5, seed=1201),
    "slam_heavy_m40": lambda: synth.make_scenario(6, 2, 40, seed=1203),
    "tile64_last_n33": lambda: synth.make_scenario(33, 30, 0, seed=1204),
    "tile128_first_n34": lambda: synth.make_scenario(34, 30, 0, seed=1205),
    # windows above 33 poses: packed gate matrix, the gate's Cholesky on four waves (two / three tile columns per wave either
    # side of d = 111) next to the one-wave gate of the short tracks, 26 / 32 rows per lane either side of 104-row tiles,
    # rejected tracks skipped by the tile step, the 40-way first merge level in the 32-lane layout with its pending strip
    "gate4_n40_ragged": lambda: synth.make_scenario(40, 60, 0, seed=1301, track_len=(2, 40)),
    "gate4_two_columns_n57": lambda: synth.make_scenario(57, 40, 0, seed=1302),
    "gate4_three_columns_n58": lambda: synth.make_scenario(58, 40, 0, seed=1303),
    "tile26_last_n53": lambda: synth.make_scenario(53, 45, 0, seed=1304, outlier_frac=0.3),
    "tile32_first_n54": lambda: synth.make_scenario(54, 45, 0, seed=1305, outlier_frac=0.3),
    "merge32_n50_420_tiles": lambda: synth.make_scenario(50, 420, 0, seed=1306, outlier_frac=0.25),
    "wide_window_with_slam_n40": lambda: synth.make_scenario(40, 50, 10, seed=1307),
}


@pytest.mark.parametrize("name", list(CASES_VS_ORACLE))
def test_against_c_oracle(xk, oracle_c, name):
    sc = CASES_VS_ORACLE[name]()
    ref = oracle_c.visual_update(sc)
    eng = _engine(xk, sc)
    got = eng.visual_update(sc)
    eng.close()
    assert np.array_equal(got["inlier"], ref["inlier"]), "MSCKF inlier masks differ"
    assert np.array_equal(got["inlier_slam"], ref["inlier_slam"])
    fin = np.isfinite(ref["gamma"])
    assert rel(got["gamma"][fin], ref["gamma"][fin]) <= 1e-8
    check_gamma_per_track(got["gamma"], got["inlier"], ref["gamma"])     # 1e-8 on every finite track; non-finite ones rejected
    rp, rc = rel(got["P"], ref["P"]), rel(got["correction"], ref["correction"])
    assert rp <= 1e-8 and rp <= TOL_NORTH_STAR, rp
    assert rc <= 1e-7, rc
    assert np.abs(got["P"] - got["P"].T).max() == 0.0


def test_config3_full_size_properties(xk, oracle_c):
    """window 50, 800 tracks: the oracle's dense QR is slow but still finishes; beyond the direct
    comparison, check the size-independent properties."""
    sc = synth.make_config(3)
    eng = _engine(xk, sc)
    got = eng.visual_update(sc)
    P0, P1 = sc["P"], got["P"]
    assert np.abs(P1 - P1.T).max() == 0.0
    assert np.linalg.eigvalsh(P1).min() >= -1e-10 * np.linalg.norm(P1)
    assert np.linalg.eigvalsh(P0 - P1).min() >= -1e-9 * np.linalg.norm(P0)          # P+ <= P-
    # permuting the tracks changes nothing (row-order invariance of the compression)
    K = len(sc["trk_off"]) - 1
    perm = np.random.default_rng(0).permutation(K)
    L = sc["trk_off"][1] - sc["trk_off"][0]
    obs = sc["obs_xy"].reshape(K, L, 2)[perm].reshape(-1, 2)
    sc2 = dict(sc, obs_xy=obs)
    got2 = eng.visual_update(sc2)
    assert np.array_equal(got2["inlier"], got["inlier"][perm])
    assert rel(got2["P"], P1) <= 1e-9 and rel(got2["correction"], got["correction"]) <= 1e-8
    eng.close()
    ref = oracle_c.visual_update(sc)
    assert np.array_equal(got["inlier"], ref["inlier"])
    assert rel(P1, ref["P"]) <= 1e-8


def test_no_measurements_and_all_outliers(xk):
    sc = synth.make_scenario(10, 5, 0, seed=11)
    eng = xk.Engine(10, 0, 8)
    empty = dict(sc, trk_off=np.zeros(1, dtype=np.int32), obs_xy=np.zeros((0, 2)))
    got = eng.visual_update(empty)     # h.size() == 0 -> no update (updater.cpp:106)
    assert np.array_equal(got["P"], sc["P"]) and not got["correction"].any()
    noise = 0.05 * np.random.default_rng(1).standard_normal(sc["obs_xy"].shape)
    bad = dict(sc, obs_xy=sc["obs_xy"] + noise)   # every track fails the gate -> zero rows (Q1)
    got = eng.visual_update(bad)
    assert got["inlier"].sum() == 0
    assert rel(got["P"], 0.5 * (sc["P"] + sc["P"].T)) <= 1e-14 and np.abs(got["correction"]).max() <= 1e-14
    eng.close()


def test_staged_equals_convenience_and_is_repeatable(xk):
    sc = synth.make_config(1)
    eng = _engine(xk, sc)
    eng.visual_update(sc)          # (a handle's first update does not know the acceptance ratio yet: it may take the 184-tile geometry
    a = eng.visual_update(sc)      #  and the following ones the 152-tile one -- equal to rounding; bit for bit from the second on)
    eng.stage(sc)
    b = eng.visual_update_staged(sc["sigma_img"])
    Pb = eng.download_P()
    assert np.array_equal(a["P"], Pb) and np.array_equal(a["correction"], b["correction"])
    eng.stage(sc)
    eng.run_steps(sc["sigma_img"], 3)           # bench path: same prior, posterior of last step
    tm = eng.bench_staged(sc["sigma_img"], 1, 2)
    assert tm["total_ms"] > 0 and tm["rows_stacked"] == int(a["inlier"].sum()) * 17
    eng.close()


def test_capacity_and_argument_errors(xk):
    sc = synth.make_config(1)
    eng = xk.Engine(10, 0, 10)                  # k_max = 10 < 50 tracks
    with pytest.raises(xk.XkError) as e:
        eng.visual_update(sc)
    assert e.value.status == 6                  # XK_ECAPACITY
    eng.close()
    eng = xk.Engine(8, 0, 60)                   # window shorter than the tracks
    with pytest.raises(xk.XkError):
        eng.visual_update(sc)
    eng.close()


def test_repeated_updates_are_bit_identical(xk):
    """The compression runs redundant / unsynchronised workgroups (column splits of the merges, the replicated
    block factorisations of the Cholesky): any race between them would make the posterior vary between runs."""
    sc = synth.make_config(4)
    eng = _engine(xk, sc)
    eng.stage(sc)
    first, zero = None, None
    for i in range(13):
        eng.upload_P(sc["P"])
        r = eng.visual_update_staged(sc["sigma_img"])
        P = eng.download_P()
        if i == 0:                 # (the first update of a handle may take another geometry: equal to rounding, checked below)
            zero = P.copy()
            continue
        if first is None:
            first = (P.copy(), r["correction"].copy())
        assert np.array_equal(P, first[0]) and np.array_equal(r["correction"], first[1])
    assert np.linalg.norm(zero - first[0]) <= 1e-11 * np.linalg.norm(first[0])
    eng.close()
