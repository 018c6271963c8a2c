"""The per-feature kernel (csrc/xk_feature.hip.h) on motion other than the circle of synth.true_poses, and on tracks whose triangulation
fails.  The cases and what the CPU references say about them are tests/feature_cases.py and tests/test_feature_cases.py; here the GPU is
compared with the C oracle TRACK BY TRACK: the gate statistic (1e-8 on every track -- one norm over all tracks hides an inlier's error behind
an outlier's gamma), the Gauss-Newton iteration count and the triangulated point (xk_debug_feature_points of the lab build: neither leaves
the device otherwise), besides the verdicts, the posterior and the Gram products of the compressed system.

Failed triangulation: a vehicle that stops has one pose twice at the end of its window, the Gauss-Newton system of every 2-observation
track is exactly singular, its landmark is NaN and the track is rejected (msckf_update.cpp:349-357).  The kernel writes such a track's tile
or factor record anyway -- NaN -- and every consumer has to leave the slot out by tile_rows = 0, by a select and not by a product: asserted
on every compression schedule (xk_caqr_status says which one ran) and across updates on one handle, where a slot keeps what the update
before left in it."""
import numpy as np
import pytest

import feature_cases as fc
from helpers import TOL_NORTH_STAR, rel
from x_multi_agent_amd import synth

pytestmark = pytest.mark.gpu


def _dims(sc):
    return sc["n_poses_max"], len(sc.get("slam_anchor_idxs", ())), len(sc["trk_off"]) - 1


def _update(eng, sc):
    """-> (flags and correction, posterior, triangulated points, Gauss-Newton iteration counts)"""
    eng.stage(sc)
    r = eng.visual_update_staged(sc["sigma_img"])
    P = eng.download_P()
    gpf, it = eng.debug_feature_points()
    return r, P, gpf, it


def _check_tracks(r, info, label):
    """Verdicts equal; gamma NaN exactly where the oracle's is, rejected there; every other track within the per-track bar."""
    nf = ~np.isfinite(info["gamma"])
    assert np.array_equal(np.isnan(r["gamma"]), nf), (label, np.where(np.isnan(r["gamma"]))[0], np.where(nf)[0])
    assert not r["inlier"][nf].any(), label
    assert np.array_equal(r["inlier"], info["inlier"]), (label, np.where(r["inlier"] != info["inlier"])[0])
    dg = fc.per_track_rel(r["gamma"][~nf], info["gamma"][~nf])
    if dg.size:
        print(f"{label}: per-track gamma {dg.max():.2e}")
        assert dg.max() <= fc.GAMMA_TOL, (label, int(np.argmax(dg)), dg.max())


@pytest.mark.parametrize("name", fc.WELL)
def test_well_conditioned_families_track_by_track(xk, name):
    c, sc = fc.CASES[name], fc.scenario(name)
    info, ref, (H, res) = fc.oracle(name)
    N, M, K = _dims(sc)
    eng = xk.LabEngine(N, M, K)
    r, P, gpf, it = _update(eng, sc)
    _check_tracks(r, info, name)
    assert np.array_equal(it, info["gn_iters"]), (name, np.where(it != info["gn_iters"])[0], it, info["gn_iters"])
    dp = fc.point_error(gpf, info["feats"], sc)
    rp, rc = rel(P, ref["P"]), rel(r["correction"], ref["correction"])
    print(f"{name}: point {dp.max():.2e} (bound {c['pt_tol']:.1e}), P {rp:.2e}, correction {rc:.2e}, iterations {it.min()}-{it.max()}")
    assert dp.max() <= c["pt_tol"], (name, int(np.argmax(dp)), dp.max())
    assert rp <= 1e-8 and rc <= 1e-7, (rp, rc)
    assert np.abs(P - P.T).max() == 0.0
    # the compressed system keeps the Gram products of the oracle's stacked rows
    eng.stage(sc)
    b = eng.msckf_build(sc["sigma_img"])
    assert np.array_equal(b["inlier"], info["inlier"])
    T, z = eng.qr_compress()
    eng.close()
    eg, ez = rel(T.T @ T, H.T @ H), rel(T.T @ z, H.T @ res)
    print(f"{name}: T^T T {eg:.2e}, T^T z {ez:.2e}")
    assert eg <= 1e-10 and ez <= 1e-10, (eg, ez)


def test_micro_translation(xk):
    """hover_1um: 1 um of translation under +-0.2 rad of rotation, the DLT matrix has two close small singular values and the references
    themselves agree to ~5e-8 per track.  Verdicts and finiteness are exact requirements; gamma and the point are held to 100 x the
    references' own disagreement, on the tracks whose iteration count agrees (at most 10 % may differ; the references differ on none)."""
    name = "hover_1um"
    c, sc = fc.CASES[name], fc.scenario(name)
    info, ref, _ = fc.oracle(name)
    N, M, K = _dims(sc)
    eng = xk.LabEngine(N, M, K)
    r, P, gpf, it = _update(eng, sc)
    eng.close()
    assert np.array_equal(r["inlier"], info["inlier"])
    assert np.isfinite(r["gamma"]).all() and np.isfinite(gpf).all() and np.isfinite(P).all() and np.isfinite(r["correction"]).all()
    assert rel(P, ref["P"]) <= TOL_NORTH_STAR
    same = it == info["gn_iters"]
    dg = fc.per_track_rel(r["gamma"], info["gamma"])[same]
    dp = fc.point_error(gpf, info["feats"], sc)[same]
    print(f"{name}: {int((~same).sum())} tracks left out, per-track gamma {dg.max():.2e} (bound {100 * c['gamma_ref']:.1e}), "
          f"point {dp.max():.2e} (bound {100 * c['pt_ref']:.1e}), P {rel(P, ref['P']):.2e}")
    assert (~same).sum() <= K // 10, (it, info["gn_iters"])
    assert dg.max() <= 100 * c["gamma_ref"] and dp.max() <= 100 * c["pt_ref"], (dg.max(), dp.max())


# (case, options set on the handle, updates on it, the schedule xk_caqr_status must report)
SCHEDULES = {
    "single_launch": ("stopped", {}, 3, 2),                      # three updates: the first-update geometry and the adaptive one
    "multi_launch": ("stopped", {"caqr_resident": 0}, 2, 0),
    "tall_window_tail": ("stopped_tall_n40", {}, 2, 3),
    "small_stack": ("stopped_small_k6", {}, 2, 4),
    "slam_split": ("stopped_slam_n30", {"slam_split": 1}, 3, 2),
    "slam_whole_stack": ("stopped_slam_n30", {"slam_split": 0}, 2, 2),
    "separate_kalman": ("stopped", {"pipe_kalman": 0}, 3, 2),
}


@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_failed_triangulation_on_every_schedule(xk, sched):
    name, opts, reps, want = SCHEDULES[sched]
    sc = fc.scenario(name)
    info, ref, _ = fc.oracle(name)
    N, M, K = _dims(sc)
    if sched.startswith("slam"):
        assert sc["P"].shape[0] > 206                # where the split form exists (xk_compress.hip.h: split_plan)
    eng = xk.LabEngine(N, M, K)
    for k, v in opts.items():
        eng.set_option(k, v)
    for rep in range(reps):
        r, P, gpf, it = _update(eng, sc)
        st = eng.caqr_status()
        label = f"{sched}[{rep}]"
        assert st["schedule"] == want and st["giveups"] == 0, (label, st)
        _check_tracks(r, info, label)
        assert np.isnan(gpf[~np.isfinite(info["gamma"])]).any(axis=1).all()
        assert np.array_equal(r["inlier_slam"], ref["inlier_slam"])
        assert np.isfinite(P).all() and np.isfinite(r["correction"]).all(), label
        rp = rel(P, ref["P"])
        print(f"{label}: P {rp:.2e}, correction {rel(r['correction'], ref['correction']):.2e}")
        assert rp <= 1e-8, (label, rp)
    eng.close()


@pytest.mark.parametrize("resident", [1, 0])
def test_collapsed_window_moves_nothing(xk, resident):
    """Every pose one pose: no track can be triangulated, every slot is NaN, and the update is the one of no inlier at all."""
    sc = fc.scenario("collapsed")
    N, M, K = _dims(sc)
    eng = xk.LabEngine(N, M, K)
    eng.set_option("caqr_resident", resident)
    for rep in range(2):
        r, P, gpf, it = _update(eng, sc)
        assert r["inlier"].sum() == 0 and np.isnan(r["gamma"]).all()
        assert rel(P, 0.5 * (sc["P"] + sc["P"].T)) <= 1e-14 and np.abs(r["correction"]).max() <= 1e-14, rep
    assert eng.caqr_status()["giveups"] == 0
    eng.close()


@pytest.mark.parametrize("resident", [1, 0])
def test_nan_slots_do_not_outlive_their_update(xk, resident):
    """A rejected track's slot is not cleared between updates.  stopped, an ordinary scenario with fewer tracks, one with more, collapsed
    (every slot NaN), the first ordinary one again, on ONE handle: each ordinary posterior is a fresh handle's."""
    few = synth.make_scenario(10, 24, 0, seed=7701)
    more = synth.make_scenario(10, 56, 0, seed=7702, track_len=(2, 10))
    seq = [fc.scenario("stopped"), few, more, fc.scenario("collapsed"), few]
    eng = xk.LabEngine(10, 0, 56)
    eng.set_option("caqr_resident", resident)
    for i, sc in enumerate(seq):
        r, P, _, _ = _update(eng, sc)
        assert np.isfinite(P).all() and np.isfinite(r["correction"]).all(), i
        if sc is few or sc is more:
            fresh = xk.LabEngine(10, 0, 56)
            fresh.set_option("caqr_resident", resident)
            r0, P0, _, _ = _update(fresh, sc)
            fresh.close()
            assert np.array_equal(r["inlier"], r0["inlier"]), i
            assert rel(P, P0) <= 1e-11, (i, rel(P, P0))
    assert eng.caqr_status()["giveups"] == 0
    eng.close()
