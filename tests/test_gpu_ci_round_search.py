"""Searched CI weights inside the device-resident CI round (xk_ci_round_device with -1 <= ci_msckf_w < 0 and the option
"ci_weight_search" on): the batched information projection (one factorisation per agent and round), the search per shared track,
and the weights' way into S_ci and the block scaling -- against the CPU yardstick of tests/ci_round_cases.py."""
import numpy as np
import pytest

import ci_weights_ref as cw
from ci_round_cases import SHAPE_IDS, SHAPES, fleet_case, others_of, packed, searched, yardstick
from ci_weights_cases import weight_tolerance
from helpers import rel

pytestmark = pytest.mark.gpu


class Fleet:
    """One engine with the own agent's problem staged and the other agents' payloads in device memory."""

    def __init__(self, xk, case, search=1):
        import torch
        self.case, self.torch = case, torch
        self.eng = xk.Engine(case["N"], case["M"], case["K"])
        self.eng.set_option("ci_weight_search", search)
        self.pays, self.trks = packed(case)
        self.dp, self.dt = torch.from_numpy(self.pays).cuda(), torch.from_numpy(self.trks).cuda()
        torch.cuda.synchronize()

    def set_payloads(self, pays):
        self.dp = self.torch.from_numpy(np.ascontiguousarray(pays)).cuda()
        self.torch.cuda.synchronize()

    def round(self, w, corrections=True):
        """Re-stage the prior, run the device round: -> (n_fused, corrections, posterior, [(weights, steps) per track])."""
        from x_multi_agent_amd import fleet
        c = self.case
        self.eng.stage(c["sc"])
        fused, corr = fleet.ci_round_device(self.eng, c["sc"], c["rank"], c["world"], self.dp, self.dt, c["n_tracks"], w,
                                            want_corrections=corrections)
        P = self.eng.download_P()
        ws = [self.eng.ci_round_weights(j) for j in range(c["n_tracks"])] if w < 0 else None
        return fused, corr, P, ws

    def close(self):
        self.eng.close()


def check_against_yardstick_at_reported_weights(case, fused, corr, P, ws):
    """Given the weights, the arithmetic is the fixed-weight round's: the bars are those of test_gpu_dense_ci against the oracle."""
    y = yardstick(case, weights=[w for w, _ in ws])
    assert fused == y["n_fused"]
    assert {j for j, (w, _) in enumerate(ws) if len(w) == 0} == y["rejected"]
    dP = rel(P, y["P"])
    dc = [rel(a, b) for a, b in zip(corr, y["corrections"])]
    print(f"world {case['world']}, n = {P.shape[0]}: {fused} fused, weights {[np.round(w, 4).tolist() for w, _ in ws]}, steps "
          f"{[it for _, it in ws]}; posterior rel {dP:.2e}, corrections rel {['%.1e' % d for d in dc]}")
    assert dP <= 1e-8, dP
    assert len(corr) == len(y["corrections"]) and all(d <= 1e-6 for d in dc), dc
    return y


# ---- 1: the round's posterior at the weights it reports ------------------------------------------------------------------------------
@pytest.mark.parametrize("world,N,corrupt", SHAPES, ids=SHAPE_IDS)
def test_posterior_at_the_reported_weights(xk, world, N, corrupt):
    case = fleet_case(world, N, corrupt)
    f = Fleet(xk, case)
    fused, corr, P, ws = f.round(-1.0)
    last_w, last_it = f.eng.ci_last_weights()
    f.close()
    check_against_yardstick_at_reported_weights(case, fused, corr, P, ws)
    w_lf, it_lf = [x for x in ws if len(x[0])][-1]
    assert np.array_equal(last_w, w_lf) and last_it == it_lf          # xk_ci_last_weights: the last fused track's


# ---- 2: the weights are the minimiser ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,N,corrupt", SHAPES, ids=SHAPE_IDS)
def test_weights_are_the_minimiser(xk, world, N, corrupt):
    case = fleet_case(world, N, corrupt)
    cpu, _ = searched(world, N, corrupt)
    f = Fleet(xk, case)
    _, _, _, ws = f.round(-1.0, corrections=False)
    f.close()
    assert len(cpu["tracks"]) >= 2
    for j, t in cpu["tracks"].items():
        w, it = ws[j]
        assert len(w) == world, (j, w)
        gap = cw.logdet(t["M"], w) - cw.logdet(t["M"], t["w"])
        print(f"track {j}: w = {w}, {it} steps (CPU {t['w']}, {t['iters']}); |dw| = {np.abs(w - t['w']).max():.2e}, log det gap {gap:.2e}")
        assert abs(w.sum() - 1.0) <= 1e-15
        assert w.min() >= cw.LB
        assert abs(gap) <= 1e-8, gap
        assert it <= 12


# ---- 3: end to end against the CPU route with its own weights ------------------------------------------------------------------------
def end_to_end_tolerance(world, N, corrupt):
    """Ten times the relative difference between the yardstick's two CPU routes to M_i on this shape, floor 1e-8."""
    a, b = searched(world, N, corrupt)
    measured = rel(a["P"], b["P"])
    return max(10.0 * measured, 1e-8), measured


@pytest.mark.parametrize("world,N,corrupt", SHAPES, ids=SHAPE_IDS)
def test_end_to_end_against_the_cpu_search(xk, world, N, corrupt):
    case = fleet_case(world, N, corrupt)
    cpu, _ = searched(world, N, corrupt)
    tol, measured = end_to_end_tolerance(world, N, corrupt)
    f = Fleet(xk, case)
    fused, _, P, _ = f.round(-1.0, corrections=False)
    f.close()
    d = rel(P, cpu["P"])
    print(f"world {world}, n = {P.shape[0]}: device vs CPU search rel {d:.2e}; two CPU routes {measured:.2e}, tolerance {tol:.2e}")
    assert fused == cpu["n_fused"]
    assert d <= tol, (d, tol)


# ---- 4: the gates do not see the weights ---------------------------------------------------------------------------------------------
def test_gates_do_not_see_the_weights(xk):
    case = fleet_case(4, 10, 1)
    f = Fleet(xk, case)
    fused_f, _, P_f, _ = f.round(0.04)
    fused_s, _, P_s, ws = f.round(-1.0)
    f.close()
    y_f = yardstick(case, weights=[[1.0 - 3 * 0.04] + [0.04] * 3] * case["n_tracks"])
    assert fused_f == fused_s == y_f["n_fused"]
    assert {j for j, (w, _) in enumerate(ws) if len(w) == 0} == y_f["rejected"] == {1}
    assert rel(P_f, y_f["P"]) <= 1e-8                                 # (the fixed round is what it was)
    d = rel(P_s, P_f)
    print(f"searched vs fixed (w = 0.04) posterior: rel {d:.3f}")
    assert d > 1e-2                                                   # the searched weights reached S_ci and the block scaling


# ---- 5: the start does not matter, and the bits repeat -------------------------------------------------------------------------------
def test_start_does_not_matter_and_bits_repeat(xk):
    case = fleet_case(4, 10, 1)
    tol, _ = weight_tolerance()
    f = Fleet(xk, case)
    _, _, P1, a = f.round(-1.0)
    _, _, _, b = f.round(-0.04)
    _, _, P2, c = f.round(-1.0)
    f.close()
    g = Fleet(xk, case)
    _, _, P3, d = g.round(-1.0)
    g.close()
    for j in range(case["n_tracks"]):
        assert len(a[j][0]) == len(b[j][0])
        if len(a[j][0]):
            print(f"track {j}: |w(-1) - w(-0.04)| = {np.abs(a[j][0] - b[j][0]).max():.2e} (tolerance {tol:.1e})")
            assert np.abs(a[j][0] - b[j][0]).max() <= tol
        assert np.array_equal(a[j][0], c[j][0]) and a[j][1] == c[j][1]
        assert np.array_equal(a[j][0], d[j][0]) and a[j][1] == d[j][1]
    assert np.array_equal(P1, P2) and np.array_equal(P1, P3)


# ---- 6: the switch and the errors ----------------------------------------------------------------------------------------------------
def test_switch_and_errors(xk):
    from x_multi_agent_amd import fleet
    case = fleet_case(2, 10, None)
    f = Fleet(xk, case, search=0)
    with pytest.raises(xk.XkError) as err:                            # option at 0
        f.round(-0.5)
    assert err.value.status == 1
    f.eng.set_option("ci_weight_search", 1)
    with pytest.raises(xk.XkError) as err:                            # no searched round yet
        f.eng.ci_round_weights(0)
    assert err.value.status == 1
    for bad in (-2.0, 0.0, 1.5):
        with pytest.raises(xk.XkError) as err:
            f.round(bad)
        assert err.value.status == 1, bad
    # the other agent's covariance with one negative direction: a numerical exit code, nothing applied, the handle goes on working
    n = 15 + 6 * case["N"]
    other = 1 - case["rank"]
    Pg = case["scs"][other]["P"]
    rng = np.random.default_rng(17)
    u = rng.standard_normal(n)
    Pbad = Pg - 40.0 * np.abs(Pg).max() * np.outer(u, u) / (u @ u)
    assert np.linalg.eigvalsh(Pbad).min() < 0
    pays = f.pays.copy()
    assert np.array_equal(pays[other, -n * n:].reshape(n, n), Pg)     # (the covariance is the tail of the payload)
    pays[other, -n * n:] = Pbad.ravel()
    f.set_payloads(pays)
    with pytest.raises(xk.XkError) as err:
        f.round(-1.0)
    assert err.value.status == 2 and f"rank {other}" in str(err.value), str(err.value)
    assert np.array_equal(f.eng.download_P(), case["sc"]["P"])
    # the same engine then runs the good round
    f.set_payloads(f.pays)
    fused, corr, P, ws = f.round(-1.0)
    check_against_yardstick_at_reported_weights(case, fused, corr, P, ws)
    with pytest.raises(xk.XkError) as err:
        f.eng.ci_round_weights(case["n_tracks"])
    assert err.value.status == 1
    # ... and a fixed-weight round afterwards matches the host-ABI route, as before
    f.eng.set_option("ci_weight_search", 0)
    fused_d, _, P_d, _ = f.round(0.04)
    f.eng.stage(case["sc"])
    fused_h, P_h = fleet.ci_round(f.eng, case["sc"], others_of(case, f.pays, f.trks), case["n_tracks"], 0.04)
    f.close()
    assert fused_d == fused_h >= 1 and rel(P_d, P_h) <= 1e-9


# ---- 7: against the host-ABI searched route ------------------------------------------------------------------------------------------
def test_against_the_host_abi_searched_route(xk):
    from x_multi_agent_amd import fleet
    case = fleet_case(4, 10, 1)
    tol, measured = end_to_end_tolerance(4, 10, 1)
    f = Fleet(xk, case)
    fused_d, _, P_d, _ = f.round(-1.0, corrections=False)
    f.eng.stage(case["sc"])
    fused_h, P_h = fleet.ci_round(f.eng, case["sc"], others_of(case, f.pays, f.trks), case["n_tracks"], -1.0)
    f.close()
    d = rel(P_d, P_h)
    print(f"device searched round vs xk_msckf_ci_track + xk_apply_ci: rel {d:.2e} (tolerance {tol:.2e}, two CPU routes {measured:.2e})")
    assert fused_d == fused_h >= 2
    assert d <= tol, (d, tol)
