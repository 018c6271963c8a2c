"""The CPU yardstick of the CI weight search (tests/ci_weights_ref.py) is itself checked: against a brute-force grid for
two agents and against a general-purpose constrained optimiser for more."""
import numpy as np
import pytest

import ci_weights_ref as cw
from ci_weights_cases import CASES, matrices


@pytest.mark.parametrize("name", [c for c in CASES if CASES[c][1] == 1])
def test_two_agent_newton_result_sits_at_the_grid_optimum(name):
    """k1 = 2: log det(M_a (1 - t) + M_b t) = log det M_a + sum_j log(1 - t + t lam_j), lam_j the eigenvalues of M_a^-1 M_b.
    A 200 001-point grid over t = w_b in [1e-4, 1 - 1e-4]; the Newton result lies within one cell of the grid's argmax."""
    Ma, Mb = matrices(name)
    lam = np.linalg.eigvals(np.linalg.solve(Ma, Mb)).real
    t = np.linspace(cw.LB, 1 - cw.LB, 200001)
    f = np.log(1 - t[:, None] + t[:, None] * lam[None, :]).sum(axis=1)
    w, it = cw.solve([Ma, Mb])
    assert abs(w[1] - t[np.argmax(f)]) <= t[1] - t[0], (w, t[np.argmax(f)])
    assert abs(w.sum() - 1) <= 1e-15 and w.min() >= cw.LB and it <= 6


@pytest.mark.parametrize("name", list(CASES))
def test_newton_reaches_the_objective_of_slsqp(name):
    """SLSQP (ftol = 1e-15) on the same problem: the objective gap is <= 1e-12.  The WEIGHTS of two different methods agree only to
    ~1e-7 (the objective is flat at its optimum), which is why no test compares weights across methods at a tight tolerance."""
    opt = pytest.importorskip("scipy.optimize")
    Ms = matrices(name)
    k1 = len(Ms)
    w, _ = cw.solve(Ms)
    r = opt.minimize(lambda x: -cw.logdet(Ms, x), np.full(k1, 1.0 / k1), jac=lambda x: -cw.grad(Ms, x), method="SLSQP",
                     bounds=[(cw.LB, 1.0)] * k1, constraints=[dict(type="eq", fun=lambda x: x.sum() - 1, jac=lambda x: np.ones(k1))],
                     options=dict(ftol=1e-15, maxiter=500))
    ws = np.maximum(r.x, cw.LB)
    ws /= ws.sum()
    assert abs(cw.logdet(Ms, w) - cw.logdet(Ms, ws)) <= 1e-12, (w, ws)


def test_extended_precision_run_moves_the_weights_by_rounding_only():
    """The same solver in np.longdouble: what float64 rounding does to the weights.  The GPU test's weight tolerance is ten times the
    largest difference here (floor 1e-12, tests/ci_weights_cases.weight_tolerance)."""
    from ci_weights_cases import weight_tolerance
    tol, worst = weight_tolerance()
    print(f"float64 vs longdouble Newton: largest weight difference {worst:.2e} -> tolerance {tol:.2e}")
    assert worst <= 1e-13 and tol == max(10 * worst, 1e-12)


def test_flat_objective_returns_the_start():
    Ma = matrices("3x1_shaped")[0]
    w, it = cw.solve([Ma, Ma], [0.7, 0.3])
    assert it == 0 and np.array_equal(w, [0.7, 0.3])
