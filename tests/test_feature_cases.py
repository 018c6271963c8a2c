"""What the cases of tests/feature_cases.py must be, asserted with the two CPU references alone (the C oracle and oracle/ref_np.py), so that
a disagreement of the GPU on one of them (test_gpu_feature_geometry.py) is a finding about the kernel and not about the case.

A well-conditioned case: the references agree per track on gamma to 1e-10, the C oracle moves by no more than 1e-10 per track when its
inputs move by a relative 4e-16, no verdict and no Gauss-Newton iteration count moves with them, no gamma is within 1e-5 of its
chi-square threshold, no track is non-finite -- and no track is left out of any of this.  A case that misses a condition gets another
seed, never another condition.  The spread of the triangulated point measured here is what the table's point tolerance is derived from."""
import warnings

import numpy as np
import pytest

import feature_cases as fc
from oracle import c_oracle, ref_np
from x_multi_agent_amd import synth


def _ref_np(name):
    sc = fc.scenario(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return ref_np.msckf_update(synth.tracks_as_list(sc), sc["C_q_G"], sc["G_p_C"], sc["P"], sc["n_poses_max"], sc["sigma_img"])[3]


def test_the_generators_leave_make_scenario_alone():
    """The substitution lasts for the call: the default stream -- golden vectors, bench.py -- is what it was."""
    before = synth.make_scenario(10, 8, 0, seed=77)
    fc.scenario("forward")
    assert synth.true_poses is fc._CIRCLE
    after = synth.make_scenario(10, 8, 0, seed=77)
    assert all(np.array_equal(before[k], after[k]) for k in ("C_q_G", "G_p_C", "obs_xy", "P", "landmarks_true"))
    # a case with given landmarks draws the same window error and the same noise as one without
    a, b = fc.scenario("circle"), fc.scenario("far_200_1000m")
    assert np.array_equal(a["G_p_C"], b["G_p_C"]) and np.array_equal(a["P"], b["P"]) and not np.array_equal(a["obs_xy"], b["obs_xy"])


@pytest.mark.parametrize("name", fc.WELL)
def test_well_conditioned(name):
    c, sc = fc.CASES[name], fc.scenario(name)
    info = fc.oracle(name)[0]
    L = fc.track_lengths(sc)
    assert np.isfinite(info["gamma"]).all() and np.isfinite(info["feats"]).all()
    rinfo = _ref_np(name)
    assert np.array_equal(info["inlier"], rinfo["inlier"]) and np.array_equal(info["gn_iters"], rinfo["gn_iters"])
    dg = fc.per_track_rel(info["gamma"], rinfo["gamma"]).max()
    sg, sp, moved = fc.spreads(name)
    chi = np.array([c_oracle.chi2inv(0.95, 2 * l - 3) for l in L])
    margin = (np.abs(info["gamma"] - chi) / chi).min()
    print(f"{name}: C oracle vs ref_np {dg:.2e}, spread gamma {sg:.2e} point {sp:.2e}, iterations {info['gn_iters'].min()}-"
          f"{info['gn_iters'].max()}, margin {margin:.2e}")
    assert dg <= 1e-10 and sg <= 1e-10, (dg, sg)
    assert not moved
    assert margin >= 1e-5, margin
    # the table's point tolerance: the recorded spread is the measured one (rounded up), the bound follows from it
    assert 0.5 * c["pt_spread"] <= sp <= c["pt_spread"], (sp, c["pt_spread"])
    assert c["pt_tol"] == pytest.approx(max(1000.0 * c["pt_spread"], 1e-12), rel=1e-12)


def test_the_families_take_the_iteration_counts_they_are_there_for():
    """The circle takes 3 Gauss-Newton iterations on every track; the other motions are what moves the lagging termination rule."""
    its = {n: fc.oracle(n)[0]["gn_iters"] for n in fc.WELL + ["hover_1um"]}
    assert set(its["circle"]) == {3}
    assert max(i.max() for i in its.values()) >= 7 and min(i.min() for i in its.values()) == 2
    assert its["forward"].max() > 3 and its["hover_1mm_exact"].max() > 3


def test_micro_translation_is_near_degenerate_and_recorded():
    """hover_1um: the references themselves agree to ~1e-8 only; what the GPU is held to is 100 x their larger disagreement."""
    name = "hover_1um"
    c, sc, info = fc.CASES[name], fc.scenario(name), fc.oracle(name)[0]
    rinfo = _ref_np(name)
    assert np.isfinite(info["gamma"]).all() and np.isfinite(info["feats"]).all()
    assert np.array_equal(info["inlier"], rinfo["inlier"]) and np.array_equal(info["gn_iters"], rinfo["gn_iters"])   # the references leave out none
    sg, sp, moved = fc.spreads(name)
    assert not moved
    dg = max(fc.per_track_rel(info["gamma"], rinfo["gamma"]).max(), sg)
    dp = max(fc.point_error(info["feats"], rinfo["feats"], sc).max(), sp)
    print(f"{name}: gamma {dg:.2e} point {dp:.2e}")
    assert 0.5 * c["gamma_ref"] <= dg <= c["gamma_ref"] and 0.5 * c["pt_ref"] <= dp <= c["pt_ref"], (dg, dp)
    assert dg > 1e-10                               # (it is not one of the well-conditioned ones)


@pytest.mark.parametrize("name", fc.STOPPED)
def test_stopped_rejects_exactly_the_two_observation_tracks(name):
    c, sc = fc.CASES[name], fc.scenario(name)
    info, ref, _ = fc.oracle(name)
    L, K = fc.track_lengths(sc), c["K"]
    assert np.array_equal(sc["G_p_C"][-1], sc["G_p_C"][-2]) and np.array_equal(sc["C_q_G"][-1], sc["C_q_G"][-2])
    nf = ~np.isfinite(info["gamma"])
    assert np.array_equal(nf, L == 2) and np.array_equal(nf, ~np.isfinite(ref["gamma"]))
    if "len2" in c:                                 # (the small stack: the count is part of the case)
        assert nf.sum() == c["len2"]
    else:
        assert 3 <= nf.sum() <= K // 4
    assert not info["inlier"][nf].any() and info["inlier"].sum() >= K // 2
    assert np.isfinite(ref["P"]).all() and np.isfinite(ref["correction"]).all()
    assert np.linalg.norm(ref["P"] - sc["P"]) > 1e-3 * np.linalg.norm(sc["P"])      # the update does something
    with pytest.raises(np.linalg.LinAlgError):      # only the C oracle serves the exactly singular cases
        _ref_np(name)


def test_collapsed_rejects_every_track():
    sc = fc.scenario("collapsed")
    info, ref, _ = fc.oracle("collapsed")
    assert not np.isfinite(info["gamma"]).any() and not info["inlier"].any()
    assert np.array_equal(ref["P"], sc["P"]) and not ref["correction"].any()


def test_per_track_bar_sees_what_the_norm_hides():
    """A relative error of 1e-6 on one inlier's gate statistic passes the norm over all tracks behind a single outlier and fails the
    per-track bar; a track without a finite reference must be a rejected one."""
    from helpers import check_gamma_per_track, rel
    info = fc.oracle("circle")[0]
    ref, inl = info["gamma"], info["inlier"]
    k = int(np.argmin(ref))
    assert inl[k] and ref.max() > 100 * ref[k]
    got = ref.copy()
    got[k] *= 1.0 + 1e-6
    assert rel(got, ref) <= 1e-8                    # the existing assertion does not notice
    check_gamma_per_track(ref, inl, ref)
    with pytest.raises(AssertionError, match="per-track gamma"):
        check_gamma_per_track(got, inl, ref)
    sinfo = fc.oracle("stopped")[0]
    check_gamma_per_track(sinfo["gamma"], sinfo["inlier"], sinfo["gamma"])
    with pytest.raises(AssertionError, match="finite reference"):
        check_gamma_per_track(sinfo["gamma"], np.ones_like(sinfo["inlier"]), sinfo["gamma"])
