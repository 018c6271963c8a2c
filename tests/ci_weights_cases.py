"""The inputs of the CI weight-search tests (not a test): built once, shared by the CPU and the GPU file."""
import functools

import numpy as np

import ci_weights_ref as cw
from x_multi_agent_amd import synth

# name -> (m, k other agents, shaped rows?); the first five draw from ONE generator in this order, the last from its own
CASES = {"3x1_shaped": (3, 1, True), "6x2_shaped": (6, 2, True), "9x3": (9, 3, False), "21x7": (21, 7, False),
         "9x3_shaped": (9, 3, True), "3x1_bound": (3, 1, False)}


@functools.lru_cache(maxsize=None)
def covariances():
    """synth's filter covariances (cond ~ 4e9): own agent n = 69, every other agent n = 54."""
    return synth.make_scenario(8, 24, 2, seed=321)["P"], synth.make_scenario(6, 5, 1, seed=322)["P"]


def draw_H(rng, m, k, shaped):
    a, b = covariances()
    Hs = []
    for i in range(k + 1):
        H = rng.standard_normal((m, (a if i == 0 else b).shape[0]))
        if shaped:   # rows of very different scale, rolled per agent: pulls the optimum away from the uniform point
            H = np.diag(10 ** np.roll(np.linspace(-0.7, 0.7, m), i * max(1, m // (k + 1)))) @ H
        Hs.append(H)
    return Hs


@functools.lru_cache(maxsize=None)
def _all():
    a, b = covariances()
    rng = np.random.default_rng(7)
    out = {}
    for name, (m, k, shaped) in CASES.items():
        Hs = draw_H(np.random.default_rng(5) if name == "3x1_bound" else rng, m, k, shaped)
        Ms = np.array([cw.info(a if i == 0 else b, H) for i, H in enumerate(Hs)])
        w, it = cw.solve(Ms)
        out[name] = dict(H=Hs, M=Ms, w=w, iters=it)
    return out


def case(name):
    """dict(H per agent, M (k1 x m x m), w = CPU Newton result from the uniform start, iters)."""
    return _all()[name]


def matrices(name):
    return case(name)["M"]


@functools.lru_cache(maxsize=None)
def weight_tolerance():
    """-> (tolerance, measured): the CPU Newton in float64 against the same in np.longdouble over all cases; the tolerance for the same
    method on the same numbers on another machine is ten times the largest difference, floor 1e-12."""
    worst = 0.0
    for name in CASES:
        c = case(name)
        wl, _ = cw.solve(c["M"], dtype=np.longdouble)
        worst = max(worst, float(np.abs(c["w"] - wl.astype(np.float64)).max()))
    return max(10 * worst, 1e-12), worst


def kkt(Ms, w, tol):
    """The optimality conditions at w, evaluated in NumPy: on the free coordinates g_i = tr(A^-1 M_i) equals the multiplier lam of
    sum w = 1 to tol * lam, on the ones at the bound g_i <= lam (1 + tol).  sum_i w_i g_i = m at every w, so lam = m when no bound is
    active and lam = (m - sum_active w_i g_i) / sum_free w_i otherwise.  -> (ok, free mask, g, lam)"""
    Ms = np.asarray(Ms)
    m = Ms.shape[1]
    g = cw.grad(Ms, w)
    free = np.asarray(w) > cw.LB
    lam = (m - np.dot(w[~free], g[~free])) / np.sum(w[free])
    ok = np.abs(g[free] - lam).max() <= tol * lam and (g[~free] <= lam * (1 + tol)).all()
    return bool(ok), free, g, lam
