"""What the cases of tests/slam_rows_cases.py must be, asserted with the CPU references alone, so that a disagreement of the GPU on one of
them (test_gpu_slam_rows.py) is a finding about a kernel and not about the case.

SLAM rows have two references, the C oracle and oracle/ref_np.py.  MSCKF-SLAM tracks have ref_np alone; what stands in for the second
one is its own spread when every input moves by a relative 4e-16.  A well-conditioned case: every gamma finite, nothing left out; the
references (or the spread) agree per feature to 1e-10 on gamma; no verdict moves under the perturbation; no gamma within 1e-5 of its
threshold; in a gate case the reference accepts at least a quarter of the features and rejects at least a quarter.  A case that misses a
condition gets another seed, never another condition.  The disagreement of the two references on the built rows measured here is what
the table's row bound is derived from."""
import numpy as np
import pytest

import feature_cases as fc
import slam_rows_cases as sr
from oracle import c_oracle, ref_np


@pytest.mark.parametrize("name", list(sr.SLAM_CASES))
def test_slam_case_is_well_conditioned(name):
    c, sc = sr.SLAM_CASES[name], sr.slam_scenario(name)
    o, r = sr.slam_oracle(name), sr.slam_ref_np(name)
    M = c["M"]
    assert o["gamma"].shape == r["gamma"].shape == (M,) and np.isfinite(o["gamma"]).all() and np.isfinite(r["gamma"]).all()
    assert np.array_equal(o["inlier"], r["inlier"])
    dg = fc.per_track_rel(o["gamma"], r["gamma"]).max()
    margin = (np.abs(o["gamma"] - o["chi"]) / o["chi"]).min()
    acc = o["inlier"].astype(bool)
    assert np.isfinite(r["rows"]).all() and np.isfinite(o["rows"][acc]).all() and np.isnan(o["rows"][~acc]).all()
    spread = sr.row_error(r["rows"][acc], o["rows"][acc]).max()
    print(f"{name}: C oracle vs ref_np gamma {dg:.2e}, rows {spread:.2e}, margin {margin:.2e}, accepted {acc.sum()} of {M}")
    assert dg <= sr.REF_TOL, dg
    assert not sr.slam_verdicts_move(name)
    assert margin >= sr.MARGIN, margin
    if c["gate"]:
        assert 4 * acc.sum() >= M and 4 * (~acc).sum() >= M, acc.sum()
    # the table's row bound: the recorded spread is the measured one (rounded up)
    assert 0.5 * c["row_spread"] <= spread <= c["row_spread"], (spread, c["row_spread"])


@pytest.mark.parametrize("name", ["sizes_alone", "sizes_fused", "sizes_packed", "sizes_moved"])
def test_every_track_size_has_features_on_both_sides_of_its_threshold(name):
    """{1, 2, n_poses, 256, 257, 1000} in one call: 2 * 256 = 512 is the table's last dof, 257 the first size past it."""
    sc, o = sr.slam_scenario(name), sr.slam_oracle(name)
    sizes = sc["slam_track_sizes"]
    assert set(sizes) == {1, 2, len(sc["G_p_C"]), 256, 257, 1000}
    for s in set(sizes):
        inl = o["inlier"][sizes == s]
        assert inl.any() and not inl.all(), (s, inl)
    # what a gate that is switched off past the table would accept: features the reference rejects
    far = (sizes > 256) & (o["inlier"] == 0)
    assert far.sum() >= 4 and np.isfinite(o["chi"][far]).all()
    assert ref_np.chi2inv(0.9, 514) == pytest.approx(555.49, abs=5e-3) and ref_np.chi2inv(0.9, 2000) == pytest.approx(2081.47, abs=5e-3)


def test_the_issue_s_check_of_the_long_track_gate():
    """make_scenario(12, 0, 40, seed=7412) with 0.6 on every third z_last: at size 257 and at size 1000 the reference rejects 14 of 40."""
    sc = dict(sr.slam_scenario("sizes_alone"))
    for size in (257, 1000):
        sc["slam_track_sizes"] = np.full(40, size, np.int32)
        info = ref_np.slam_update(sc["slam_track_sizes"], sc["slam_z_last"], sc["C_q_G"], sc["G_p_C"], sc["slam_feat"],
                                  sc["slam_anchor_idxs"], sc["P"], sc["n_poses_max"], sc["sigma_img"])[3]
        assert (info["inlier"] == 0).sum() == 14 and info["gamma"][::3].min() >= 7.5e3


def test_forced_anchors_and_the_short_window():
    for name in ("anchors_short_window", "tiles_m70_n33", "tall_window_n34"):
        c, sc, o = sr.SLAM_CASES[name], sr.slam_scenario(name), sr.slam_oracle(name)
        npz = len(sc["G_p_C"])
        newest, oldest = list(c.get("newest", ())), list(c.get("oldest", ()))
        assert (sc["slam_anchor_idxs"][newest] == npz - 1).all() and (sc["slam_anchor_idxs"][oldest] == 0).all()
        for idx in (newest, oldest):                # re-anchoring keeps an inlier an inlier: both verdicts among the forced ones
            if len(idx) >= 5:
                assert o["inlier"][idx].any() and not o["inlier"][idx].all()
        # the newest-pose branch: two unit entries in the feature's own columns and nothing else (slam_update.cpp:120-131)
        for j in newest:
            if o["inlier"][j]:
                h = o["rows"][j][:, :-1]
                fcol = 15 + 6 * c["N"] + 3 * j
                assert h[0, fcol] == 1.0 and h[1, fcol + 1] == 1.0 and np.count_nonzero(h) == 2
    assert len(sr.slam_scenario("anchors_short_window")["G_p_C"]) == 14 < sr.SLAM_CASES["anchors_short_window"]["N"]
    assert 2 * sr.SLAM_CASES["tiles_m70_n33"]["M"] > 128 and sr.SLAM_CASES["tiles_m70_n33"]["N"] <= 33 < sr.SLAM_CASES["tall_window_n34"]["N"]


def test_feature_behind_the_newest_camera_is_pinned():
    """The reference has no guard on c[2] < 0 (slam_update.cpp:100-113): residual and rows are finite and the gate decides.  Both CPU
    references decide alike; the table records it."""
    c, sc = sr.SLAM_CASES["behind_camera"], sr.slam_scenario("behind_camera")
    o, r = sr.slam_oracle("behind_camera"), sr.slam_ref_np("behind_camera")
    idx = list(c["behind"])
    depth = sr.depth_in_newest_camera(sc)
    assert (depth[idx] < 0).all() and (np.delete(depth, idx) > 0).all()
    assert tuple(o["inlier"][idx]) == tuple(r["inlier"][idx]) == c["behind_inlier"]
    assert 0 in c["behind_inlier"] and 1 in c["behind_inlier"]
    assert np.isfinite(r["rows"][idx]).all()


@pytest.mark.parametrize("name", sr.MS_WELL)
def test_msckf_slam_case_is_well_conditioned(name):
    c = sr.MS_CASES[name]
    sc, tracks = sr.ms_scenario(name)
    per, upd = sr.ms_oracle(name)
    assert [len(t) for t in tracks] == list(c["L"]) and len(per) == len(tracks) and None not in per
    assert len(sc["G_p_C"]) == c.get("n_poses", c["N"]) and sc["P"].shape[0] == 15 + 6 * c["N"] + 3 * len(tracks)
    gam = np.array([o["gamma"] for o in per])
    assert np.isfinite(gam).all()
    sg, moved = sr.ms_spread(name)
    chi = np.array([ref_np.chi2inv(0.95, 2 * len(t) - 3) for t in tracks])
    margin = (np.abs(gam - chi) / chi).min()
    print(f"{name}: spread gamma {sg:.2e}, margin {margin:.2e}, verdicts {[int(o['inlier']) for o in per]}")
    assert sg <= sr.REF_TOL and not moved
    assert margin >= sr.MARGIN
    assert np.array_equal(upd["msckf_slam"]["inlier"], [int(o["inlier"]) for o in per])
    assert np.linalg.norm(upd["P"] - sc["P"]) > 1e-4 * np.linalg.norm(sc["P"])      # the update does something (a handful of rows)
    if "outlier" in c:
        k = c["outlier"]
        assert [int(o["inlier"]) for o in per] == [int(i != k) for i in range(len(per))] and gam[k] > 10 * chi[k]
        assert np.isfinite(per[k]["H1"]).all() and np.isfinite(per[k]["H2"]).all()    # its column-space rows are still produced


def test_msckf_slam_cases_cover_the_shapes_they_are_there_for():
    L = {n: c["L"] for n, c in sr.MS_CASES.items()}
    assert {2, 3, 5} <= set(L["short_n8"]) and {32, 33} <= set(L["second_pass_n34"]) and sr.MS_CASES["second_pass_n34"]["N"] == 34
    assert set(L["slot128_n40"]) == {40} and 2 * 40 - 3 > 64
    assert len(set(L["mixed_n12"])) >= 4
    for n in ("partial_full_n12", "partial_short_n12"):
        assert sr.MS_CASES[n]["n_poses"] < sr.MS_CASES[n]["N"]
    assert set(L["partial_full_n12"]) == {sr.MS_CASES["partial_full_n12"]["n_poses"]}
    assert max(L["partial_short_n12"]) < sr.MS_CASES["partial_short_n12"]["n_poses"]
    assert all(3 <= len(v) <= 6 for v in L.values())


def test_stopped_window_what_ref_np_does_with_the_singular_track():
    """The last two poses are one pose: the Gauss-Newton system of the 2-observation track is exactly singular and ref_np raises
    (numpy.linalg.inv; the reference's Eigen inverse returns non-finite numbers instead and the gate rejects the track).  The expected
    update is the reference's update of the two other tracks."""
    sc, tracks = sr.ms_scenario("stopped_n10")
    assert np.array_equal(sc["G_p_C"][-1], sc["G_p_C"][-2]) and np.array_equal(sc["C_q_G"][-1], sc["C_q_G"][-2])
    assert [len(t) for t in tracks] == [2, 6, 10]
    with pytest.raises(np.linalg.LinAlgError):
        sr._ms_one(sc, tracks[0])
    per, upd = sr.ms_oracle("stopped_n10")
    assert per[0] is None and all(o is not None and o["inlier"] for o in per[1:])
    assert list(upd["msckf_slam"]["inlier"]) == [1, 1]
    assert np.isfinite(upd["P"]).all() and np.isfinite(upd["correction"]).all()
    assert np.linalg.norm(upd["P"] - sc["P"]) > 1e-3 * np.linalg.norm(sc["P"])
    with pytest.raises(RuntimeError, match="status 2"):      # the C oracle's triangulation of the same two observations: XO_ESINGULAR
        c_oracle.triangulate_gn(sc["C_q_G"][-2:], sc["G_p_C"][-2:], tracks[0])


def test_per_feature_bar_sees_what_the_norm_over_all_features_hides():
    """helpers.check_visual holds gamma_slam to the per-feature bar as well: 1e-6 on one inlier behind the outliers' thousands."""
    from helpers import check_gamma_per_track, rel
    o = sr.slam_oracle("sizes_alone")
    k = int(np.argmin(o["gamma"]))
    got = o["gamma"].copy()
    got[k] *= 1.0 + 1e-6
    assert o["inlier"][k] and rel(got, o["gamma"]) <= 1e-8
    with pytest.raises(AssertionError, match="per-track gamma"):
        check_gamma_per_track(got, o["inlier"], o["gamma"])
