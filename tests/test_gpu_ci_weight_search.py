"""Searched covariance-intersection weights (negative ci_*_w with xk_set_option "ci_weight_search" = 1): the solver kernel on its
own against the CPU yardstick (tests/ci_weights_ref.py), the information projection behind it, and the four CI entries that use it.

One deviation from the issue's wording of the optimality check: it compares g_i = tr(A^-1 M_i) on the free coordinates with m.
sum_i w_i g_i = m holds at every w, so the multiplier of sum w = 1 is m only while no bound is active; in the case that ends on
w_b = 1e-4 the CPU yardstick itself has g = (3.0000096, 2.9039), i.e. |g_a - m| = 3.2e-6 m at the true optimum.  ci_weights_cases.kkt
therefore tests against the multiplier lam = (m - sum_active w_i g_i) / sum_free w_i, which IS m in the four interior cases -- the
same bound 1e-8 there, and the correct condition at the bound."""
import os

import numpy as np
import pytest

import ci_weights_ref as cw
from ci_weights_cases import CASES, case, covariances, draw_H, kkt, weight_tolerance
from helpers import GOLDEN_DIR, rel
from oracle import ref_np

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(xk):
    e = xk.Engine(8, 2, 4)
    e.set_option("ci_weight_search", 1)
    yield e
    e.close()


def _hph(Ps, Hs):
    return [H @ P @ H.T for P, H in zip(Ps, Hs)]


# ---- 1-3: the solver alone, on identical inputs -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_solver_alone_against_the_cpu_newton(eng, name):
    c = case(name)
    Ms, m = c["M"], c["M"].shape[1]
    tol, _ = weight_tolerance()
    w, it = eng.ci_solve_weights(Ms)
    ok, free, g, lam = kkt(Ms, w, 1e-8)
    print(f"{name}: w = {w}, {it} steps (CPU {c['iters']}); max |g - lam| / lam on free = {np.abs(g[free] - lam).max() / lam:.2e}, "
          f"lam - m = {lam - m:.2e}, |w - w_cpu| = {np.abs(w - c['w']).max():.2e} (tolerance {tol:.1e}), "
          f"log det gap = {cw.logdet(Ms, w) - cw.logdet(Ms, c['w']):.2e}")
    assert ok, (g, lam)
    assert abs(w.sum() - 1.0) <= 1e-15 and w.min() >= cw.LB
    assert cw.logdet(Ms, w) >= cw.logdet(Ms, c["w"]) - 1e-10
    assert np.array_equal(w <= cw.LB, c["w"] <= cw.LB)
    assert np.abs(w - c["w"]).max() <= tol
    assert it <= 12
    if name == "3x1_bound":
        assert w[1] == cw.LB
    else:
        assert free.all() and abs(lam - m) <= 1e-12 * m      # interior: the multiplier is m, the issue's form of the check


def test_flat_objective_returns_the_start_untouched(eng):
    Ma = case("3x1_shaped")["M"][0]
    w, it = eng.ci_solve_weights([Ma, Ma], [0.7, 0.3])
    assert it == 0 and np.array_equal(w, [0.7, 0.3])


def test_same_inputs_same_bits(xk, eng):
    Ms = case("21x7")["M"]
    w1, it1 = eng.ci_solve_weights(Ms)
    w2, it2 = eng.ci_solve_weights(Ms)
    fresh = xk.Engine(8, 2, 4)
    w3, it3 = fresh.ci_solve_weights(Ms)     # (the solver itself needs no option: the option guards the negative-weight entries)
    fresh.close()
    assert np.array_equal(w1, w2) and np.array_equal(w1, w3) and it1 == it2 == it3


# ---- 4: information projection M_i = H_i P_i^-1 H_i^T --------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8, 30])
def test_information_projection_through_a_searched_entry(xk, N):
    """Well-conditioned covariances (cond ~ 6e3) at n = 69 (one xk_chol_whole launch) and n = 195 (two 192-row slabs with the Schur
    GEMM between them): the weights of a searched fuse_ci_slam satisfy the optimality condition for NumPy's M_i."""
    rng = np.random.default_rng(17 + N)
    e = xk.Engine(N, 2 if N == 8 else 0, 4)
    e.set_option("ci_weight_search", 1)
    n, m = e.n, 6
    Ps = []
    for _ in range(2):
        B = rng.standard_normal((n, n)) * 0.2
        Ps.append(B @ B.T + 1e-3 * np.eye(n))
    Hs = [np.diag(10 ** np.roll(np.linspace(-0.7, 0.7, m), 3 * i)) @ rng.standard_normal((m, n)) for i in range(2)]
    e.fuse_ci_slam(Ps[0], Hs[0], Ps[1], Hs[1], -1.0)
    w, it = e.ci_last_weights()
    e.close()
    Ms = [cw.info(P, H) for P, H in zip(Ps, Hs)]
    ok, free, g, lam = kkt(Ms, w, 1e-8)
    print(f"n = {n}: w = {w}, {it} steps, max |g - lam| / lam = {np.abs(g[free] - lam).max() / lam:.2e}")
    assert len(w) == 2 and ok and free.all(), (w, g, lam)


def test_information_projection_of_filter_covariances(eng):
    """synth's covariances (cond ~ 4e9): two CPU routes to M_i already differ by 2e-8 and in w by 3e-9, so only the objective is
    compared here (and the consistency of the fused output below)."""
    a, b = covariances()
    c = case("3x1_shaped")
    eng.fuse_ci_slam(a, c["H"][0], b, c["H"][1], -1.0)
    w, _ = eng.ci_last_weights()
    print(f"w = {w} (CPU {c['w']}), log det gap = {cw.logdet(c['M'], w) - cw.logdet(c['M'], c['w']):.2e}")
    assert abs(cw.logdet(c["M"], w) - cw.logdet(c["M"], c["w"])) <= 1e-8


# ---- 5: the fused output is the fixed-weight formula at the returned weights -----------------------------------------------------
def test_fused_output_is_consistent_with_the_returned_weights(eng):
    a, b = covariances()
    tol, _ = weight_tolerance()
    c = case("3x1_shaped")
    Ta, Tb = _hph([a, b], c["H"])
    got = {}
    for w_in in (-0.3, -1.0):
        S, wr = eng.fuse_ci_slam(a, c["H"][0], b, c["H"][1], w_in)
        w, it = eng.ci_last_weights()
        got[w_in] = w
        assert len(w) == 2 and w.min() >= cw.LB
        assert rel(S, Ta / (1.0 - w[1]) + Tb / w[1]) <= 1e-12
        assert wr == 1.0 / (1.0 - w[1])
        print(f"fuse_ci_slam({w_in}): w = {w}, {it} steps")
    assert np.abs(got[-0.3] - got[-1.0]).max() <= tol          # the start does not matter
    rng = np.random.default_rng(11)
    for k in (1, 3, 7):
        Hs = draw_H(rng, 3 * k, k, True)
        Ps = [a] + [b] * k
        S, wr = eng.fuse_ci_msckf(a, Hs[0], Ps[1:], Hs[1:], -0.1)
        w, it = eng.ci_last_weights()
        assert len(w) == k + 1 and w.min() >= cw.LB and abs(w.sum() - 1.0) <= 1e-15
        assert rel(S, sum(T / wi for T, wi in zip(_hph(Ps, Hs), w))) <= 1e-12
        assert wr == 1.0 / w[0]
        Ms = [cw.info(P, H) for P, H in zip(Ps, Hs)]
        wc, _ = cw.solve(Ms)
        print(f"fuse_ci_msckf(-0.1, k = {k}): w = {w}, {it} steps, log det gap to the CPU = {cw.logdet(Ms, w) - cw.logdet(Ms, wc):.2e}")
        assert abs(cw.logdet(Ms, w) - cw.logdet(Ms, wc)) <= 1e-8


# ---- 6: the per-track forms ----------------------------------------------------------------------------------------------------------
def test_multi_slam_match_searched_keeps_the_gate_and_weights_its_s(xk):
    z = np.load(os.path.join(GOLDEN_DIR, "ci_two_agents.npz"))
    a = {k[2:]: z[k] for k in z.files if k.startswith("a_")}
    b = {k[2:]: z[k] for k in z.files if k.startswith("b_")}
    N, w_fix, var_l = int(z["n_poses_max"]), float(z["ci_slam_w"]), float(z["sigma_landmark"]) ** 2
    e = xk.Engine(N, 4, 12)
    n_in = 0
    for j in range(4):
        args = (a["C_q_G"], a["G_p_C"], a["slam_feat"], int(a["slam_anchor_idxs"][j]), j, a["P"], N,
                b["C_q_G"], b["G_p_C"], b["slam_feat"], int(b["slam_anchor_idxs"][j]), j, b["P"], N, float(z["sigma_landmark"]))
        e.set_option("ci_weight_search", 0)
        f = e.multi_slam_match(*args, w_fix)
        e.set_option("ci_weight_search", 1)
        s = e.multi_slam_match(*args, -w_fix)
        assert s["inlier"] == f["inlier"] and s["gamma"] == f["gamma"]
        assert np.array_equal(s["H"], f["H"]) and np.array_equal(s["res"], f["res"])
        if not s["inlier"]:
            continue
        n_in += 1
        w, _ = e.ci_last_weights()
        assert len(w) == 2 and w.min() >= cw.LB
        Ta = f["H"] @ a["P"] @ f["H"].T
        Tb = w_fix * (f["S"] - var_l * np.eye(3) - Ta / (1.0 - w_fix))          # the other side's 3 x 3 block, from the fixed-weight S
        assert rel(s["S"], Ta / (1.0 - w[1]) + Tb / w[1] + var_l * np.eye(3)) <= 1e-10
        Pj = a["P"].copy()
        cols = np.flatnonzero(np.abs(f["H"]).sum(axis=0))
        assert len(cols) == 9
        for c0 in cols[::3]:
            Pj[c0:c0 + 3, c0:c0 + 3] *= 1.0 / (1.0 - w[1])
        assert rel(s["P_j"], Pj) <= 1e-14
        Pn, _ = e.apply_ci(s["P_j"], s["H"], s["res"], s["S"])
        assert np.isfinite(Pn).all() and np.array_equal(Pn, Pn.T)
    e.close()
    assert n_in >= 1


def test_msckf_ci_track_searched_keeps_the_gates_and_weights_its_s(xk, monkeypatch):
    g = np.load(os.path.join(GOLDEN_DIR, "multi_uav_n8_k20.npz"))
    N, sig, w_fix = int(g["n_poses_max"]), float(g["sigma_img"]), float(g["ci_msckf_w"])
    off, obs = g["own_trk_off"], g["own_obs"]
    q0, p0, P0 = g["a0_C_q_G"], g["a0_G_p_C"], g["a0_P"]
    table = {}
    for i, (t, ag) in enumerate(zip(g["match_track"], g["match_agent"])):
        table.setdefault(int(t), []).append(dict(obs=g[f"recv{i}"], q_list=g[f"a{ag}_C_q_G"], p_list=g[f"a{ag}_G_p_C"], P=g[f"a{ag}_P"],
                                                 n_poses_max=N))
    e = xk.Engine(N, 0, 20)
    n_ci = 0
    for t, matches in table.items():
        trk = obs[off[t]:off[t + 1]]
        k = len(matches)
        w_in = min(w_fix, 0.9 / k)
        e.set_option("ci_weight_search", 0)
        f = e.msckf_ci_track(trk, q0, p0, P0, N, sig, matches, w_in)
        e.set_option("ci_weight_search", 1)
        s = e.msckf_ci_track(trk, q0, p0, P0, N, sig, matches, -w_in)
        assert s["self_inlier"] == f["self_inlier"] and s["self_gamma"] == f["self_gamma"]
        assert (s["ci"] is None) == (f["ci"] is None)
        if f["self_inlier"]:
            assert s["ci_gamma"] == f["ci_gamma"]
        if s["ci"] is None:
            continue
        n_ci += 1
        sc, fc = s["ci"], f["ci"]
        assert np.array_equal(sc["H"], fc["H"]) and np.array_equal(sc["res"], fc["res"])
        w, it = e.ci_last_weights()
        assert len(w) == k + 1 and w.min() >= cw.LB and abs(w.sum() - 1.0) <= 1e-15
        print(f"track {t}, {k} other agent(s): w = {w}, {it} steps")
        L, Pj = len(trk), P0.copy()
        for i in range(L):
            for c0 in (15 + 3 * (len(p0) - L + i), 15 + 3 * (len(p0) - L + i) + 3 * N):
                Pj[c0:c0 + 3, c0:c0 + 3] *= 1.0 / w[0]
        assert rel(sc["P_j"], Pj) <= 1e-14
        T0 = fc["H"] @ P0 @ fc["H"].T
        m = 3 * k
        if k == 1:      # two terms: the other agent's follows from the fixed-weight S of the same call
            T1 = w_in * (fc["S"] - sig ** 2 * np.eye(m) - T0 / (1.0 - w_in))
            assert rel(sc["S"], T0 / w[0] + T1 / w[1] + sig ** 2 * np.eye(m)) <= 1e-10
        # any k: the NumPy restatement of the block with its fixed-weight fuseCI replaced by the formula at the returned weights,
        # compared through the basis-independent products (as test_msckf_ci_track_golden_and_oracle does)
        monkeypatch.setattr(ref_np, "fuse_ci_msckf", lambda Pa, Ha, Pbs, Hbs, _w: (
            Ha @ Pa @ Ha.T / w[0] + sum(Hb @ Pb @ Hb.T / wi for Pb, Hb, wi in zip(Pbs, Hbs, w[1:])), 1.0 / w[0]))
        o = ref_np.msckf_ci_track(trk, q0, p0, P0, N, sig, matches, w_in)["ci"]
        monkeypatch.undo()
        Sg, So = np.linalg.inv(sc["S"]), np.linalg.inv(o["S"])
        assert rel(sc["H"].T @ Sg @ sc["H"], o["H"].T @ So @ o["H"]) <= 1e-7
        assert rel(sc["H"].T @ Sg @ sc["res"], o["H"].T @ So @ o["res"]) <= 1e-7
        Pn, _ = e.apply_ci(sc["P_j"], sc["H"], sc["res"], sc["S"])
        assert np.isfinite(Pn).all() and np.array_equal(Pn, Pn.T)
    e.close()
    assert n_ci >= 2


# ---- 7: the switch and the errors ------------------------------------------------------------------------------------------------
def test_switch_and_error_codes(xk):
    a, b = covariances()
    c = case("3x1_shaped")
    Ha, Hb = c["H"]
    e = xk.Engine(8, 2, 4)
    with pytest.raises(xk.XkError) as err:          # option at its default 0: as before
        e.fuse_ci_slam(a, Ha, b, Hb, -0.5)
    assert err.value.status == 1
    e.set_option("ci_weight_search", 1)
    for bad in (-2.0, 0.0, 1.5):
        with pytest.raises(xk.XkError) as err:
            e.fuse_ci_slam(a, Ha, b, Hb, bad)
        assert err.value.status == 1, bad
    # a covariance with one negative direction: a numerical exit code, and the handle goes on working
    rng = np.random.default_rng(17)
    u = rng.standard_normal(a.shape[0])
    Pbad = a - 40.0 * np.abs(a).max() * np.outer(u, u) / (u @ u)
    assert np.linalg.eigvalsh(Pbad).min() < 0
    with pytest.raises(xk.XkError) as err:
        e.fuse_ci_slam(Pbad, Ha, b, Hb, -0.5)
    assert err.value.status == 2
    S, wr = e.fuse_ci_slam(a, Ha, b, Hb, -0.5)
    w, _ = e.ci_last_weights()
    assert np.isfinite(S).all() and wr == 1.0 / (1.0 - w[1])
    S, wr = e.fuse_ci_slam(a, Ha, b, Hb, 0.25)      # and fixed weights are what they were
    assert rel(S, Ha @ a @ Ha.T / 0.75 + Hb @ b @ Hb.T / 0.25) <= 1e-12 and wr == 1.0 / 0.75
    e.close()
