"""The two kernels that put a persistent feature's rows into the visual update, FEATURE BY FEATURE: xk_slam_rows_body
(csrc/xk_feature.hip.h, launched alone or inside xk_build_rows) against the C oracle, xk_msckf_slam_init (csrc/xk_slaminit.hip.h) against
oracle/ref_np.py.  The cases and what the CPU references say about them are tests/slam_rows_cases.py and tests/test_slam_rows_cases.py.

Per feature: the verdict, the gate statistic (1e-8 on every feature -- one norm over all features hides an inlier's error behind an
outlier's gamma) and the rows AS BUILT (xk_debug_stack_rows of the lab build: xk_qr_compress always compresses the whole stack, so the
rows themselves leave the device nowhere else) within the bound the case table derives from the two CPU references' own disagreement.

Track sizes: a persistent feature's track grows every frame, and the gate is the 0.9 quantile at dof = 2 * size for EVERY size
(slam_update.cpp:196-199).  With the threshold read from a table that ends at dof 512 and nothing behind it, every feature of size >= 257
that the reference rejects is accepted: the sizes_* cases fail on the verdicts then."""
import numpy as np
import pytest

import slam_rows_cases as sr
from helpers import check_gamma_per_track, rel
from oracle import c_oracle

pytestmark = pytest.mark.gpu


def _dims(sc):
    return sc["n_poses_max"], len(sc["slam_anchor_idxs"]), len(sc["trk_off"]) - 1


def _check_slam_features(eng, name, label):
    """Build the staged case and compare verdict, gamma and the two rows [h | res] of every feature with the C oracle."""
    c, sc, o = sr.SLAM_CASES[name], sr.slam_scenario(name), sr.slam_oracle(name)
    N, M, K = _dims(sc)
    eng.stage(sc)
    b = eng.msckf_build(sc["sigma_img"])
    got = eng.debug_stack_rows(K, 2 * M).reshape(M, 2, -1)
    got = np.concatenate([np.zeros((M, 2, 15)), got], axis=2)                  # (the tiles hold the active columns: the core's are zero)
    acc = o["inlier"].astype(bool)
    assert not o["rows"][acc][:, :, :15].any()
    assert np.array_equal(b["inlier_slam"], o["inlier"]), (label, np.where(b["inlier_slam"] != o["inlier"])[0],
                                                           sc["slam_track_sizes"][b["inlier_slam"] != o["inlier"]])
    dg = np.abs(b["gamma_slam"] - o["gamma"]) / np.abs(o["gamma"])
    de = sr.row_error(got[acc], o["rows"][acc])
    print(f"{label}: per-feature gamma {dg.max():.2e} (bound {sr.GAMMA_TOL:.0e}), rows {de.max():.2e} (bound {sr.row_tol(c):.1e})")
    assert dg.max() <= sr.GAMMA_TOL, (label, int(np.argmax(dg)), dg.max())
    assert de.max() <= sr.row_tol(c), (label, int(np.argmax(de)), de.max())
    assert not got[~acc].any(), (label, "a rejected feature has rows", np.where(got[~acc].any(axis=(1, 2)))[0])
    return b


def _check_update(eng, name, label):
    """The whole update of the case against the C oracle: verdicts, gammas per track and per feature, P, correction."""
    sc = sr.slam_scenario(name)
    ref = c_oracle.visual_update(sc)
    eng.stage(sc)
    r = eng.visual_update_staged(sc["sigma_img"])
    P = eng.download_P()
    assert np.array_equal(r["inlier_slam"], ref["inlier_slam"]) and np.array_equal(r["inlier"], ref["inlier"]), label
    check_gamma_per_track(r["gamma_slam"], r["inlier_slam"], ref["gamma_slam"])
    check_gamma_per_track(r["gamma"], r["inlier"], ref["gamma"])
    rp, rc = rel(P, ref["P"]), rel(r["correction"], ref["correction"])
    print(f"{label}: P {rp:.2e}, correction {rc:.2e}")
    assert rp <= 1e-8 and rc <= 1e-6, (label, rp, rc)
    return r


@pytest.mark.parametrize("name", [n for n, c in sr.SLAM_CASES.items() if c["K"] == 0])
def test_slam_rows_alone_feature_by_feature(xk, name):
    c, sc = sr.SLAM_CASES[name], sr.slam_scenario(name)
    N, M, K = _dims(sc)
    eng = xk.LabEngine(N, M, 1)
    _check_update(eng, name, name)
    assert eng.caqr_status()["schedule"] == 4           # 2 M rows against n > 3 M columns: not compressed, the rows go to the update as built
    b = _check_slam_features(eng, name, name)
    if "behind" in c:                                  # no guard in the reference: the gate decides, as both CPU references have it
        assert tuple(b["inlier_slam"][list(c["behind"])]) == c["behind_inlier"]
    eng.close()


@pytest.mark.parametrize("name,packed", [("sizes_fused", False), ("sizes_packed", True)])
def test_slam_rows_next_to_tracks(xk, name, packed):
    """The mixed-size case with tracks present: inside xk_build_rows (windows of at most 33 poses), and as a launch of its own next to
    the packed per-track kernel (longer windows, 128-row slots)."""
    sc = sr.slam_scenario(name)
    N, M, K = _dims(sc)
    assert K > 0 and (len(sc["G_p_C"]) > 33) == packed
    eng = xk.LabEngine(N, M, K)
    _check_update(eng, name, name)
    _check_slam_features(eng, name, name)
    eng.close()


def test_a_rejected_slot_keeps_nothing_from_the_update_before(xk):
    """Two updates on ONE handle with the outliers moved from features 0, 3, 6 .. to 1, 4, 7 ..: every slot that carried rows in the
    first update and is rejected in the second is zero, and the second update is a fresh handle's."""
    first, second = sr.slam_oracle("sizes_alone"), sr.slam_oracle("sizes_moved")
    assert ((first["inlier"] == 1) & (second["inlier"] == 0)).sum() >= 8
    sc = sr.slam_scenario("sizes_moved")
    N, M, K = _dims(sc)
    eng = xk.LabEngine(N, M, 1)
    _check_update(eng, "sizes_alone", "first")
    _check_slam_features(eng, "sizes_alone", "first")
    _check_slam_features(eng, "sizes_moved", "second")
    _check_update(eng, "sizes_moved", "second")
    eng.close()


def test_more_long_track_sizes_than_the_handle_remembers(xk):
    """xk_stage_slam keeps the last eight thresholds it computed past the table: 20 different sizes past it in one call, staged twice,
    every verdict the C oracle's both times; a size whose dof does not fit an int is refused."""
    sc = dict(sr.slam_scenario("sizes_alone"))
    sizes = sc["slam_track_sizes"].copy()
    sizes[::2] = 257 + 37 * np.arange(20)
    sc["slam_track_sizes"] = sizes
    info = c_oracle.slam_update(*sr._slam_args(sc))[3]
    assert info["inlier"][::2].any() and not info["inlier"][::2].all()
    N, M, K = _dims(sc)
    eng = xk.LabEngine(N, M, 1)
    for rep in range(2):
        eng.stage(sc)
        b = eng.msckf_build(sc["sigma_img"])
        assert np.array_equal(b["inlier_slam"], info["inlier"]), (rep, np.where(b["inlier_slam"] != info["inlier"])[0])
        check_gamma_per_track(b["gamma_slam"], b["inlier_slam"], info["gamma"])
    with pytest.raises(xk.XkError) as e:
        eng.stage(dict(sc, slam_track_sizes=np.where(np.arange(M) == 3, 2 ** 30, sizes).astype(np.int32)))
    assert e.value.status == 1
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# MSCKF-SLAM tracks
# ---------------------------------------------------------------------------------------------------------------------------------
def _ms_run(xk, name):
    """-> (engine with the case built last, update result, posterior, msckf_slam_results)"""
    sc, tracks = sr.ms_scenario(name)
    eng = xk.LabEngine(sc["n_poses_max"], len(tracks), 1)
    eng.stage(sc)
    eng.stage_msckf_slam(tracks)
    r = eng.visual_update_staged(sc["sigma_img"])
    ms, P = eng.msckf_slam_results(), eng.download_P()
    eng.stage(sc)
    eng.stage_msckf_slam(tracks)
    eng.msckf_build(sc["sigma_img"])
    return eng, r, P, ms


def _check_ms_track(eng, name, k, ms, o, L):
    """Track k against ref_np's dict o: verdict, gamma, the feature, what initMsckfSlamFeatures consumes (independent of the column-space
    basis), H2's shape, and for an accepted track the Gram products of its projected rows as built."""
    blk = slice(3 * k, 3 * k + 3)
    assert ms["inlier"][k] == int(o["inlier"]), (name, k)
    dg = abs(ms["gamma"][k] - o["gamma"]) / abs(o["gamma"])
    df = rel(ms["features"][blk], o["feature"])
    H2 = ms["H2"][blk, blk]
    assert np.all(np.tril(H2, -1) == 0) and np.abs(np.diag(H2)).min() > 0, (name, k)
    H2i, rH2i = np.linalg.inv(H2), np.linalg.inv(o["H2"])
    dG, dHH = rel(H2i @ ms["H1"][blk], rH2i @ o["H1"]), rel(H2i @ H2i.T, rH2i @ rH2i.T)
    dr = np.abs(H2i @ ms["r1"][blk] - rH2i @ o["r1"]).max()
    line = f"{name}[{k}] L={L}: gamma {dg:.2e}, feature {df:.2e}, H2^-1 H1 {dG:.2e}, H2^-1 H2^-T {dHH:.2e}, H2^-1 r1 {dr:.2e}"
    d = 2 * L - 3
    if o["inlier"]:
        rows = eng.debug_stack_rows(k, d)                # (no track is staged: the MSCKF-SLAM tracks' slots K .. K + K2 - 1 start at 0)
        H0, r0 = np.concatenate([np.zeros((d, 15)), rows[:, :-1]], axis=1), rows[:, -1]
        eg, ez = rel(H0.T @ H0, o["jac0"].T @ o["jac0"]), rel(H0.T @ r0, o["jac0"].T @ o["res0"])
        line += f", H0^T H0 {eg:.2e}, H0^T r0 {ez:.2e}"
    print(line)
    assert dg <= sr.GAMMA_TOL and df <= 1e-9, (name, k, dg, df)
    assert dG <= 1e-9 and dHH <= 1e-9 and dr <= 1e-10, (name, k, dG, dHH, dr)
    if o["inlier"]:
        assert eg <= 1e-10 and ez <= 1e-10, (name, k, eg, ez)


def _check_ms_system(eng, upd, P, r, name):
    """The compressed system holds the accepted tracks' rows and nothing of a rejected one; posterior and correction are ref_np's."""
    T, z = eng.qr_compress()
    H, res = upd["h_stack"], upd["res_stack"]
    eg, ez = rel(T.T @ T, H.T @ H), rel(T.T @ z, H.T @ res)
    rp, rc = rel(P, upd["P"]), rel(r["correction"], upd["correction"])
    print(f"{name}: T^T T {eg:.2e}, T^T z {ez:.2e}, P {rp:.2e}, correction {rc:.2e}")
    assert eg <= 1e-10 and ez <= 1e-10, (name, eg, ez)
    assert rp <= 1e-9 and rc <= 1e-8, (name, rp, rc)


@pytest.mark.parametrize("name", sr.MS_WELL)
def test_msckf_slam_tracks_track_by_track(xk, name):
    sc, tracks = sr.ms_scenario(name)
    per, upd = sr.ms_oracle(name)
    eng, r, P, ms = _ms_run(xk, name)
    assert np.all(ms["H2"][np.kron(np.eye(len(tracks)), np.ones((3, 3))) == 0] == 0)      # block diagonal
    for k, (o, t) in enumerate(zip(per, tracks)):
        _check_ms_track(eng, name, k, ms, o, len(t))
    _check_ms_system(eng, upd, P, r, name)
    eng.close()


def test_msckf_slam_stopped_window(xk):
    """The last two poses are one pose: the 2-observation track cannot be triangulated.  It is rejected with a gamma that is not
    finite, and the update is the reference's update of the two other tracks.  (The feature initialisation is not called on it.)"""
    name = "stopped_n10"
    sc, tracks = sr.ms_scenario(name)
    per, upd = sr.ms_oracle(name)
    assert per[0] is None
    eng, r, P, ms = _ms_run(xk, name)
    assert ms["inlier"][0] == 0 and not np.isfinite(ms["gamma"][0])
    assert np.isfinite(P).all() and np.isfinite(r["correction"]).all()
    for k in (1, 2):
        _check_ms_track(eng, name, k, ms, per[k], len(tracks[k]))
    _check_ms_system(eng, upd, P, r, name)
    eng.close()
