"""The covariance-intersection kernels ENTRY BY ENTRY against oracle/ref_np.py, on the fleets and matches of tests/ci_entry_cases.py
(what each case is, and that the two CPU references agree on it, is asserted by test_ci_entry_cases.py without a GPU): uneven track
lengths down to L = 2, windows that are not full on the own and on a matched side, SLAM feature columns, tracks the JOINT gate rejects
after the own gate accepted them, a joint gate past the chi-square table; SLAM-SLAM matches whose two sides differ in N, M, feature id
and anchor.

Per MSCKF-MSCKF case and shared track, both routes: the host-ABI entry xk_msckf_ci_track (+ xk_apply_ci), the device-resident round
xk_ci_round_device with that one track, and one round with all 8 tracks.  Every figure is printed before it is asserted.  Bounds: the
caps of test_gpu_dense_ci.py, and below them ci_entry_cases.prod_tol for the joint gamma and the two basis-independent products."""
import numpy as np
import pytest

import ci_entry_cases as ce
from helpers import rel
from oracle import ref_np

pytestmark = pytest.mark.gpu


def _check(errs, bounds, what):
    """errs: {quantity: worst value}; printed whole, then every one held to its bound."""
    print(f"{what}: " + ", ".join(f"{k} {v:.2e} (bound {bounds[k]:.1e})" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= bounds[k], (what, k, v, bounds[k])


def _worse(errs, key, value):
    errs[key] = max(errs.get(key, 0.0), float(value))


def _payloads(fl):
    """The agents' payloads as the all-gather leaves them: -> host array [world, payload_doubles]."""
    from x_multi_agent_amd import fleet
    dyn = np.zeros(16)
    dyn[9] = 1.0
    return np.stack([fleet.pack_payload_host(r, 0.0, dyn, s["C_q_G"], s["G_p_C"], s.get("slam_feat"), s.get("slam_anchor_idxs"), s["P"],
                                             fl["N"], fl["M"]) for r, s in enumerate(fl["scs"])])


def _track_rows(fl, js):
    """The tracks buffer of a round whose shared tracks are the staged tracks js: -> host array [world, len(js), 1 + 2 N]."""
    out = np.zeros((fl["world"], len(js), 1 + 2 * fl["N"]))
    for r in range(fl["world"]):
        for i, j in enumerate(js):
            o = fl["tracks"][r][j]
            out[r, i, 0] = len(o)
            out[r, i, 1:1 + 2 * len(o)] = o.ravel()
    return out


@pytest.mark.parametrize("name", list(ce.MS_CASES))
def test_host_abi_route_entry_by_entry(xk, name):
    """xk_msckf_ci_track per shared track: both verdicts and gammas, the products, P_j; then xk_apply_ci's posterior and correction."""
    c, fl, ref, applied = ce.MS_CASES[name], ce.fleet(name), ce.ms_ref_np(name), ce.ms_applied(name)
    sc = fl["sc"]
    bounds = dict(own_gamma=ce.GAMMA_TOL, joint_gamma=ce.prod_tol(c), HtSiH=ce.prod_tol(c), HtSires=ce.prod_tol(c), P_j=ce.PJ_TOL,
                  posterior=ce.HOST_P_TOL, correction=ce.HOST_CORR_TOL)
    errs = {}
    eng = xk.Engine(fl["N"], fl["M"], ce.K_TRACKS)
    for j, t in enumerate(ref):
        g = eng.msckf_ci_track(fl["tracks"][fl["rank"]][j], sc["C_q_G"], sc["G_p_C"], sc["P"], fl["N"], sc["sigma_img"],
                               ce.matches_of(fl, j), ce.W)
        assert g["self_inlier"] == t["own_inlier"], (j, g["self_gamma"], t["own_gamma"])
        _worse(errs, "own_gamma", abs(g["self_gamma"] - t["own_gamma"]) / abs(t["own_gamma"]))
        if t["own_inlier"]:
            _worse(errs, "joint_gamma", abs(g["ci_gamma"] - t["ci_gamma"]) / abs(t["ci_gamma"]))
        assert (g["ci"] is not None) == (t["ci"] is not None), (j, t["verdict"], g["ci_gamma"], t["ci_chi"])
        if t["ci"] is None:
            continue
        (A, b), (Ar, br) = ce.products(g["ci"]), ce.products(t["ci"])
        _worse(errs, "HtSiH", rel(A, Ar))
        _worse(errs, "HtSires", rel(b, br))
        _worse(errs, "P_j", rel(g["ci"]["P_j"], t["ci"]["P_j"]))
        P, corr = eng.apply_ci(g["ci"]["P_j"], g["ci"]["H"], g["ci"]["res"], g["ci"]["S"])
        _worse(errs, "posterior", rel(P, applied[j][0]))
        _worse(errs, "correction", rel(corr, applied[j][1]))
    eng.close()
    _check(errs, bounds, f"{name} host-ABI route")


@pytest.mark.parametrize("name", list(ce.MS_CASES))
def test_device_round_one_track_at_a_time(xk, name):
    """xk_ci_round_device with ONE shared track, self_track = [j]: n_fused is the reference's verdict; fused: the correction and the
    resident posterior are the reference's; not fused: the resident covariance is byte-equal to the prior."""
    import torch
    fl, ref, applied = ce.fleet(name), ce.ms_ref_np(name), ce.ms_applied(name)
    sc, world, rank = fl["sc"], fl["world"], fl["rank"]
    pays = _payloads(fl)
    nv = pays[:, 5].astype(np.int32)                         # the header's n_poses: what the round takes as n_poses_valid
    assert list(nv) == [len(s["G_p_C"]) for s in fl["scs"]]
    dp = torch.from_numpy(pays).cuda()
    rows = [_track_rows(fl, [j]) for j in range(ce.K_TRACKS)]
    dts = torch.from_numpy(np.stack(rows)).cuda()
    torch.cuda.synchronize()                                 # the engine works on its own stream
    bounds = dict(posterior=ce.ROUND_P_TOL, correction=ce.ROUND_CORR_TOL)
    errs = {}
    eng = xk.Engine(fl["N"], fl["M"], ce.K_TRACKS)
    prior = None
    for j, t in enumerate(ref):
        eng.stage(sc)                                        # resident P = the staged prior again
        if prior is None:
            prior = eng.download_P()
            assert np.array_equal(prior, sc["P"])
        n_fused, corr = eng.ci_round_device(dp.data_ptr(), pays.shape[1], world, rank, dts[j].data_ptr(), 1, rows[j][:, :, 0], nv,
                                            [j], sc["sigma_img"], ce.W, want_corrections=True)
        P = eng.download_P()
        assert n_fused == int(t["ci"] is not None), (j, t["verdict"])
        if t["ci"] is None:
            assert corr.shape == (0, eng.n) and P.tobytes() == prior.tobytes(), (j, t["verdict"])
            continue
        _worse(errs, "posterior", rel(P, applied[j][0]))
        _worse(errs, "correction", rel(corr[0], applied[j][1]))
    eng.close()
    _check(errs, bounds, f"{name} device round, one track at a time")


@pytest.mark.parametrize("name", list(ce.MS_CASES))
def test_device_round_with_all_eight_tracks(xk, name):
    """One round with all 8 shared tracks (fleet.ci_round_device: lengths and window sizes from the device buffers): n_fused is the
    reference's count, the corrections arrive in track order entry by entry, the posterior is the LAST fused entry's alone."""
    import torch
    from x_multi_agent_amd import fleet
    fl, ref, applied = ce.fleet(name), ce.ms_ref_np(name), ce.ms_applied(name)
    sc, world = fl["sc"], fl["world"]
    dp = torch.from_numpy(_payloads(fl)).cuda()
    dt = torch.from_numpy(_track_rows(fl, list(range(ce.K_TRACKS))).reshape(world, -1)).cuda()
    torch.cuda.synchronize()
    eng = xk.Engine(fl["N"], fl["M"], ce.K_TRACKS)
    eng.stage(sc)
    n_fused, corr = fleet.ci_round_device(eng, sc, fl["rank"], world, dp, dt, ce.K_TRACKS, ce.W, want_corrections=True)
    P = eng.download_P()
    eng.close()
    fused = [j for j, t in enumerate(ref) if t["ci"] is not None]
    assert n_fused == len(fused) >= 3 and corr.shape == (n_fused, sc["P"].shape[0])
    errs = {}
    for i, j in enumerate(fused):                            # a rejected track in between shifts nothing
        _worse(errs, "correction", rel(corr[i], applied[j][1]))
    _worse(errs, "posterior", rel(P, applied[fused[-1]][0]))
    _check(errs, dict(posterior=ce.ROUND_P_TOL, correction=ce.ROUND_CORR_TOL), f"{name} device round, 8 tracks")
    # Q6: every entry starts from the prior; an earlier fused entry leaves no trace in the posterior
    assert all(rel(applied[j][0], applied[fused[-1]][0]) > 1e-4 for j in fused[:-1])


def test_matched_window_size_is_validated(xk):
    """xk_msckf_ci_track: a matched agent's list is no longer than its window (m_nposes <= m_nposes_max) and its covariance holds that
    window (m_n >= 15 + 6 m_nposes_max): XK_EINVAL before anything is queued."""
    name = "short_windows_w2_N12"
    fl = ce.fleet(name)
    sc = fl["sc"]
    eng = xk.Engine(fl["N"], fl["M"], ce.K_TRACKS)
    for bad in (8, 13):                                      # 9 valid poses in a window of 8; a window of 13 in 15 + 6 * 12 columns
        matches = [dict(m, n_poses_max=bad) for m in ce.matches_of(fl, 1)]
        with pytest.raises(xk.XkError) as e:
            eng.msckf_ci_track(fl["tracks"][fl["rank"]][1], sc["C_q_G"], sc["G_p_C"], sc["P"], fl["N"], sc["sigma_img"], matches, ce.W)
        assert e.value.status == 1, bad
    g = eng.msckf_ci_track(fl["tracks"][fl["rank"]][1], sc["C_q_G"], sc["G_p_C"], sc["P"], fl["N"], sc["sigma_img"], ce.matches_of(fl, 1), ce.W)
    assert g["ci"] is not None                               # the handle stays usable
    eng.close()


def test_slam_matches_field_by_field(xk):
    """xk_multi_slam_match on sides that differ in N, M, n_poses, feature id and anchor, at three weights, and on a prior with an
    asymmetric entry inside a gathered block: every field against ref_np.  The entries built from the symmetric prior then go through
    xk_apply_ci.  The two built from the asymmetric prior do not: their S is asymmetric by 4e-8 (relative), applyCI's Cholesky reads
    one triangle of S where the reference inverts the whole matrix (include/xk.h), and the difference is the input's, not rounding:
    measured on an MI355X 3.9e-7 on the posterior and 4.4e-6 on the correction, which ref_np.apply_ci on one triangle of the same S
    reproduces on the CPU (test_ci_entry_cases.test_slam_match_asymmetric_prior_is_seen_by_s_not_by_gamma)."""
    own, _ = ce.slam_sides()
    R, _ = ce.slam_refs()
    eng = xk.Engine(own["n_poses_max"], len(own["slam_anchor_idxs"]), 4)
    errs, n_applied = {}, 0
    for m, t in zip(ce.SLAM_MATCHES, R):
        g = eng.multi_slam_match(*ce.slam_args(m))
        assert g["inlier"] == t["inlier"], (m, g["gamma"], t["gamma"])
        _worse(errs, "gamma", abs(g["gamma"] - t["gamma"]) / t["gamma"])
        _worse(errs, "H", rel(g["H"], t["H"]))
        _worse(errs, "res", rel(g["res"], t["res"]))
        if not t["inlier"]:
            continue
        _worse(errs, "S", rel(g["S"], t["S"]))
        _worse(errs, "P_j", rel(g["P_j"], t["P_j"]))
        if m[3]:
            continue
        n_applied += 1
        P, corr = eng.apply_ci(g["P_j"], g["H"], g["res"], g["S"])
        Pr, cr = ref_np.apply_ci(t["P_j"], t["H"], t["res"], t["S"])
        _worse(errs, "post", rel(P, Pr))
        _worse(errs, "corr", rel(corr, cr))
    eng.close()
    assert n_applied >= 4
    _check(errs, ce.SLAM_TOL, "SLAM-SLAM matches")


def test_slam_match_against_a_larger_agent_is_a_capacity_error(xk):
    """The roles swapped: an engine sized for the small agent (n = 72) matches against the large one (no = 93 > n).  Pinned: status 6."""
    _, oth = ce.slam_sides()
    eng = xk.Engine(oth["n_poses_max"], len(oth["slam_anchor_idxs"]), 4)
    with pytest.raises(xk.XkError) as e:
        eng.multi_slam_match(*ce.slam_args(ce.SLAM_MATCHES[0], swap=True))
    assert e.value.status == 6
    g = eng.multi_slam_match(*(ce.slam_args(ce.SLAM_MATCHES[0], swap=True)[:7] * 2 + [ce.SIGMA_LANDMARK, 0.5]))   # the handle stays usable
    assert np.isfinite(g["gamma"])
    eng.close()
