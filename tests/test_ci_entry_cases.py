"""What the cases of tests/ci_entry_cases.py must be, asserted with the two CPU references alone (the C oracle and oracle/ref_np.py), so
that a disagreement of the GPU on one of them (test_gpu_ci_entries.py) is a finding about a kernel or a route and not about the case.

Per MSCKF-MSCKF case: the references agree on every verdict (own gate, joint gate), on both gammas to 1e-10, on the basis-independent
products and on P_j; no gamma within 1e-5 of its threshold; the verdict classes the case is there for are present; the disagreement
of the references measured here is the one recorded in the table (the GPU's bound is derived from it).  And the wrong variants restated
on the CPU -- own observations first in the joint triangulation, the gate's unweighted S for the entry's S, a matched agent's attitude
columns placed by the length of its pose list -- move the case's numbers by far more than the GPU's tolerance: a kernel or a route that
did any of it would fail the GPU file.  A case that misses a condition gets another seed, never another condition."""
import numpy as np
import pytest

import ci_entry_cases as ce
from oracle import c_oracle, ref_np


def _spreads(name):
    """-> (largest disagreement of the references on the joint gamma and the two products, on the triangulated point)."""
    fl, sp, ps = ce.fleet(name), 0.0, 0.0
    for a, b in zip(ce.ms_ref_np(name), ce.ms_oracle(name)):
        ps = max(ps, ce.point_error(fl, b["gpf"], a["gpf"]))
        if a["ci_gamma"] is not None:
            sp = max(sp, abs(b["ci_gamma"] - a["ci_gamma"]) / abs(a["ci_gamma"]))
        if a["ci"] is not None:
            A, B = ce.products(a["ci"]), ce.products(b["ci"])
            sp = max(sp, ce.rel(B[0], A[0]), ce.rel(B[1], A[1]))
    return sp, ps


@pytest.mark.parametrize("name", list(ce.MS_CASES))
def test_references_agree_and_no_gamma_sits_on_its_threshold(name):
    c, fl = ce.MS_CASES[name], ce.fleet(name)
    r, o = ce.ms_ref_np(name), ce.ms_oracle(name)
    assert len(r) == len(o) == ce.K_TRACKS == len(fl["sc"]["trk_off"]) - 1
    margin = np.inf
    for j, (a, b) in enumerate(zip(r, o)):
        assert a["verdict"] == b["verdict"], j
        assert np.isfinite(a["own_gamma"]) and abs(b["own_gamma"] - a["own_gamma"]) <= ce.REF_TOL * abs(a["own_gamma"]), j
        margin = min(margin, abs(a["own_gamma"] - a["own_chi"]) / a["own_chi"])
        if a["own_inlier"]:
            assert np.isfinite(a["ci_gamma"]) and abs(b["ci_gamma"] - a["ci_gamma"]) <= ce.REF_TOL * abs(a["ci_gamma"]), j
            margin = min(margin, abs(a["ci_gamma"] - a["ci_chi"]) / a["ci_chi"])
            assert (a["ci_gamma"] < a["ci_chi"]) == (a["verdict"] == "fused")
        if a["ci"] is not None:
            A, B = ce.products(a["ci"]), ce.products(b["ci"])
            assert ce.rel(B[0], A[0]) <= ce.REF_TOL and ce.rel(B[1], A[1]) <= ce.REF_TOL, j
            assert ce.rel(b["ci"]["P_j"], a["ci"]["P_j"]) <= ce.PJ_TOL, j
    sp, ps = _spreads(name)
    print(f"{name}: verdicts {[t['verdict'] for t in r]}, margin {margin:.2e}, prod_spread {sp:.2e}, pt_spread {ps:.2e}")
    assert margin >= ce.MARGIN, margin
    # the table's bounds: the recorded spreads are the measured ones (rounded up)
    assert 0.5 * c["prod_spread"] <= sp <= c["prod_spread"], (sp, c["prod_spread"])
    assert 0.5 * c["pt_spread"] <= ps <= c["pt_spread"], (ps, c["pt_spread"])
    assert ce.prod_tol(c) <= ce.PROD_CAP


def test_verdict_classes_every_case_is_there_for():
    count = {n: {v: [t["verdict"] for t in ce.ms_ref_np(n)].count(v) for v in ("fused", "own_rejected", "joint_rejected")}
             for n in ce.MS_CASES}
    for n, k in count.items():
        assert k["fused"] >= 3, (n, k)
        assert sum(k.values()) == ce.K_TRACKS
    assert count["short_windows_w2_N12"]["own_rejected"] >= 1 and count["limits_w8_N6_M1"]["own_rejected"] >= 1
    assert count["wrong_association_w2_N10"]["joint_rejected"] >= 3
    # fused and rejected entries interleave: the joint gate rejects the odd tracks alone
    v = [t["verdict"] for t in ce.ms_ref_np("wrong_association_w2_N10")]
    assert all(x == "joint_rejected" for x in v[1::2]) and "joint_rejected" not in v[0::2]
    # the reference's own applyCI of the fused entries: finite, and it moves the covariance
    for n in ce.MS_CASES:
        for t, ap in zip(ce.ms_ref_np(n), ce.ms_applied(n)):
            assert (ap is None) == (t["ci"] is None)
            if ap is not None:
                assert np.isfinite(ap[0]).all() and np.isfinite(ap[1]).all() and ce.rel(ap[0], ce.fleet(n)["sc"]["P"]) > 1e-4


def test_cases_cover_the_shapes_they_are_there_for():
    fl = {n: ce.fleet(n) for n in ce.MS_CASES}
    n_of = lambda f: f["sc"]["P"].shape[0]
    lens = lambda f: np.array([[len(f["tracks"][r][j]) for r in range(f["world"])] for j in range(ce.K_TRACKS)])
    f = fl["ragged_w3_N10_M2"]
    others = np.delete(lens(f), f["rank"], axis=1)
    assert n_of(f) == 81 == 2 * 32 + 17 and (others == 2).sum() >= 2 and (lens(f)[:, f["rank"]] == 2).any()
    assert all(len(set(row)) > 1 for row in lens(f))            # no track has one length on all three agents
    f = fl["short_windows_w2_N12"]
    assert [len(s["G_p_C"]) for s in f["scs"]] == [9, 7] and f["rank"] == 1 and f["N"] == 12
    assert all(s["P"].shape[0] == 15 + 6 * 12 for s in f["scs"])
    assert lens(f)[:, 0].max() <= 9 and lens(f)[:, 1].max() <= 7 and lens(f).min() == 3
    f = fl["limits_w8_N6_M1"]
    assert f["world"] - 1 == 7 and n_of(f) == 54 and lens(f).min() == 2
    f = fl["wrong_association_w2_N10"]
    assert (lens(f)[:, 0] == 3).all() and (lens(f)[:, 1] == 10).all()
    f = fl["wide_w2_N30_M20"]
    assert n_of(f) == 255 and 255 % 32 == 31 and (255 + 31) // 32 == 8 and len(set(lens(f).ravel())) >= 8
    f = fl["far_dof_w8_N34"]
    dof = 2 * lens(f).sum(axis=1) - 3
    assert (dof == 541).all() and 541 >= 513
    assert ref_np.chi2inv(0.95, 541) == pytest.approx(596.22, abs=5e-3)
    assert c_oracle.chi2inv(0.95, 541) == pytest.approx(ref_np.chi2inv(0.95, 541), rel=1e-12)
    for f in fl.values():                                  # nothing here is larger than n = 255, and 8 tracks are the round's limit
        assert n_of(f) <= 255 and len(f["sc"]["trk_off"]) - 1 == 8


@pytest.mark.parametrize("name", ce.SENSITIVE)
def test_wrong_variants_are_far_outside_the_gpu_tolerance(name):
    c, fl, r = ce.MS_CASES[name], ce.fleet(name), ce.ms_ref_np(name)
    fused = [j for j, t in enumerate(r) if t["ci"] is not None]
    # own observations first in the joint triangulation: same landmark, another DLT start and anchor pose, so the Gauss-Newton
    # iteration stops elsewhere.  It is the weakest of the three (the point alone moves): asserted on the case's worst track
    moved = [ce.point_error(fl, ce.self_first_point(fl, j), r[j]["gpf"]) for j in range(ce.K_TRACKS)]
    # the gate's unweighted S in place of the CI-weighted one
    unw = [ce.rel(ce.unweighted_product(fl, j, r[j]["ci"]), ce.products(r[j]["ci"])[0]) for j in fused]
    print(f"{name}: self-first moves the point by {min(moved):.1e} .. {max(moved):.1e} (pt_tol {ce.pt_tol(c):.1e}), "
          f"unweighted S moves H^T S^-1 H by {min(unw):.1e} .. {max(unw):.1e} (tolerance {ce.prod_tol(c):.1e})")
    assert max(moved) > ce.pt_tol(c)
    assert min(unw) > 1000.0 * ce.prod_tol(c)


def test_list_length_for_the_matched_window_size_is_far_outside_the_gpu_tolerance():
    """short_windows_w2_N12: the matched agent sends 9 valid poses of a window of 12.  Its attitude columns are at 15 + 3 * 12 + 3 pos;
    placing them by the list length (15 + 3 * 9 + 3 pos) moves H^T S^-1 H of every fused entry."""
    name = "short_windows_w2_N12"
    c, r, v = ce.MS_CASES[name], ce.ms_ref_np(name), ce.ms_list_length_variant(name)
    moved = [ce.rel(ce.products(b["ci"])[0], ce.products(a["ci"])[0]) for a, b in zip(r, v) if a["ci"] is not None and b["ci"] is not None]
    print(f"list length for n_poses_max moves H^T S^-1 H by {min(moved):.1e} .. {max(moved):.1e}")
    assert len(moved) >= 3 and min(moved) > 1000.0 * ce.prod_tol(c)
    # the own side is not touched by it: same own gamma
    assert all(a["own_gamma"] == b["own_gamma"] for a, b in zip(r, v))


# ---------------------------------------------------------------------------------------------------------------------------------
# SLAM-SLAM matches
# ---------------------------------------------------------------------------------------------------------------------------------
def test_slam_match_cases():
    own, oth = ce.slam_sides()
    R, O = ce.slam_refs()
    chi = ref_np.chi2inv(0.9, 3)
    assert own["P"].shape[0] == 93 and oth["P"].shape[0] == 72 and len(oth["G_p_C"]) == 6 < oth["n_poses_max"] == 8
    # anchors in pose 0 and in the newest pose on each side; the ids differ across every match
    assert own["slam_anchor_idxs"][5] == 0 and own["slam_anchor_idxs"][2] == 9
    assert oth["slam_anchor_idxs"][0] == 5 and oth["slam_anchor_idxs"][1] == 0
    assert all(m[0] != m[1] for m in ce.SLAM_MATCHES) and {m[2] for m in ce.SLAM_MATCHES} == {0.02, 0.5, 0.98}
    margin = np.inf
    for m, a, b in zip(ce.SLAM_MATCHES, R, O):
        assert a["inlier"] == b["inlier"] == (m in ce.SLAM_TRUE), m
        assert abs(b["gamma"] - a["gamma"]) <= ce.REF_TOL * a["gamma"], m
        assert ce.rel(b["H"], a["H"]) <= ce.SLAM_TOL["H"] and ce.rel(b["res"], a["res"]) <= ce.SLAM_TOL["res"], m
        margin = min(margin, abs(a["gamma"] - chi) / chi)
        if a["inlier"]:
            assert ce.rel(b["S"], a["S"]) <= ce.SLAM_TOL["S"] and ce.rel(b["P_j"], a["P_j"]) <= ce.SLAM_TOL["P_j"], m
        # the three gathered blocks of either side: anchor position, anchor attitude (behind n_poses_MAX position blocks), feature
        for h, sc, fid, npm in ((a["H"], own, m[0], 10), (None, oth, m[1], 8)):
            an = int(sc["slam_anchor_idxs"][fid])
            cols = sorted(15 + 3 * an + np.arange(3)) + sorted(15 + 3 * npm + 3 * an + np.arange(3)) + sorted(15 + 6 * npm + 3 * fid + np.arange(3))
            if h is not None:
                assert sorted(np.nonzero(np.abs(h).sum(axis=0))[0]) == cols, m
    assert sum(a["inlier"] for a in R) >= 4 and sum(not a["inlier"] for a in R) >= 1
    assert margin >= ce.MARGIN, margin


def test_slam_match_asymmetric_prior_is_seen_by_s_not_by_gamma():
    """1e-9 on ONE side of the diagonal inside a gathered block.  The reference multiplies H P H^T out as written, so S takes P_iv and
    P_vi apart: the prior's transpose gives another S (by more than 100 x the tolerance on S).  gamma = res^T S^-1 res sees the symmetric
    part of S^-1 alone and the antisymmetric part of S enters it in second order: an inverse that assumed symmetry would show in S, and
    in gamma only if it dropped more than the antisymmetric part."""
    asym = [m for m in ce.SLAM_MATCHES if m[3]]
    assert len(asym) >= 2
    for m in asym:
        args = ce.slam_args(m)
        assert np.abs(args[5] - args[5].T).max() == pytest.approx(ce.ASYM, rel=1e-3)
        a = ref_np.multi_slam_match(*args)
        args[5] = args[5].T.copy()
        t = ref_np.multi_slam_match(*args)
        assert a["inlier"] and ce.rel(t["S"], a["S"]) > 100.0 * ce.SLAM_TOL["S"]
        assert np.abs(a["S"] - a["S"].T).max() > 100.0 * ce.SLAM_TOL["S"] * np.abs(a["S"]).max()
        assert abs(t["gamma"] - a["gamma"]) <= ce.SLAM_TOL["gamma"] * a["gamma"]
        # why these two entries are not fed to xk_apply_ci: applyCI by Cholesky reads ONE triangle of S (include/xk.h), the reference
        # inverts the whole matrix, and on this S that is 1e-7 .. 4e-7 on the posterior -- the input's asymmetry, amplified, not rounding
        Pr, cr = ref_np.apply_ci(a["P_j"], a["H"], a["res"], a["S"])
        for tri in (np.tril(a["S"]) + np.tril(a["S"], -1).T, np.triu(a["S"]) + np.triu(a["S"], 1).T):
            Pt, ct = ref_np.apply_ci(a["P_j"], a["H"], a["res"], tri)
            assert 5e-8 < ce.rel(Pt, Pr) < 1e-6 and ce.rel(ct, cr) > 10.0 * ce.SLAM_TOL["corr"]
    sym = [m for m in ce.SLAM_TRUE if not m[3]]
    assert len(sym) >= 4 and {m[2] for m in sym} == {0.02, 0.5, 0.98}        # what goes through xk_apply_ci
