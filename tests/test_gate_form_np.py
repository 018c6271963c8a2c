"""The gate statistic without the projection (csrc/xk_feature.hip.h: xk_chol_gate_gls), by NumPy alone.

A spans the complement of range(Hf), so gamma = (A^T res)^T (A^T M A)^-1 (A^T res) is the minimum of a generalised least-squares problem,

    gamma = min_x (res - Hf x)^T M^-1 (res - Hf x) = |y - Y z|^2,   [y | Y] = L^-1 [res | Hf],  M = L L^T,  z = (Y^T Y)^-1 Y^T y,

which the kernel evaluates for tracks of at most 32 observations.  Here, on every family of tests/feature_cases.py that triangulates: the
two forms agree per track within the project's gamma bar and give the same verdicts; the smallest pivot of C = Y^T Y scaled to unit
diagonal, computed as the kernel computes it, stays above the kernel's threshold XK_GLS_PIVOT_MIN (read from the header), and falls below
it on a window of constant attitude, where Hf has exactly rank 2 and the kernel must take the projected form."""
import os
import re

import numpy as np
import pytest

import feature_cases as fc
from oracle import ref_np
from x_multi_agent_amd import synth

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "x_multi_agent_amd", "csrc", "xk_feature.hip.h")
TRIANGULATING = [c for c, v in fc.CASES.items() if v["kind"] in ("well", "micro", "stopped")]   # stopped: the tracks that have a point


def pivot_min():
    m = re.search(r"^#define XK_GLS_PIVOT_MIN\s+(\S+)", open(HEADER).read(), re.M)
    assert m, "XK_GLS_PIVOT_MIN not found in xk_feature.hip.h"
    return float(m.group(1))


def constant_attitude():
    """`forward` with every attitude set to the first one: all R g coincide, the observability constraint removes the same direction from
    every block of Hf."""
    sc = dict(fc.scenario("forward"))
    sc["C_q_G"] = np.tile(np.asarray(sc["C_q_G"])[0], (len(sc["C_q_G"]), 1))
    return sc


def both_forms(sc):
    """Per track with a finite triangulated point: -> (gamma projected, gamma GLS by the residual form, smallest unit-diagonal pivot of C,
    |y|^2 / gamma, verdicts of the two forms)."""
    P, var = sc["P"], sc["sigma_img"] ** 2
    out = []
    for trk in synth.tracks_as_list(sc):
        L = len(trk)
        q_l, p_l = sc["C_q_G"][len(sc["C_q_G"]) - L:], sc["G_p_C"][len(sc["G_p_C"]) - L:]
        try:
            ivd, _ = ref_np.triangulate_gn(q_l, p_l, trk)
        except np.linalg.LinAlgError:        # (a stopped vehicle's 2-observation tracks: exactly singular normal equations, no point)
            continue
        gpf = ref_np.global_feature_position(ivd, q_l[-1], p_l[-1])
        if not np.all(np.isfinite(gpf)):
            continue
        o = ref_np.msckf_track_jacobians(trk, sc["C_q_G"], sc["G_p_C"], sc["n_poses_max"], gpf, P.shape[1])
        if o is None:
            continue
        jac, hf, res = o
        M = jac @ P @ jac.T + var * np.eye(2 * L)
        _, a = ref_np.left_nullspace(hf)
        r0 = a.T @ res
        g_proj = float(r0 @ np.linalg.solve(a.T @ M @ a, r0))
        yY = np.linalg.solve(np.linalg.cholesky(M), np.column_stack([res, hf]))
        y, Y = yY[:, 0], yY[:, 1:]
        C, b = Y.T @ Y, Y.T @ y
        # as the kernel: D = diag(C)^-1/2, Cholesky of D C D with a unit diagonal, pivots p2 and p3
        with np.errstate(all="ignore"):
            s = 1.0 / np.sqrt(np.diag(C))
            l21, l31, h23 = C[0, 1] * s[0] * s[1], C[0, 2] * s[0] * s[2], C[1, 2] * s[1] * s[2]
            p2 = 1.0 - l21 * l21
            l32 = (h23 - l31 * l21) / np.sqrt(p2)
            p3 = 1.0 - l31 * l31 - l32 * l32
            w1 = b[0] * s[0]
            w2 = (b[1] * s[1] - l21 * w1) / np.sqrt(p2)
            w3 = (b[2] * s[2] - l31 * w1 - l32 * w2) / np.sqrt(p3)
            u3 = w3 / np.sqrt(p3)
            u2 = (w2 - l32 * u3) / np.sqrt(p2)
            u1 = w1 - l21 * u2 - l31 * u3
            z = np.array([u1, u2, u3]) * s
            e = y - Y @ z
            g_gls = float(e @ e)
        pmin = min(p2, p3) if p2 == p2 and p3 == p3 else -np.inf
        chi = ref_np.chi2inv(0.95, 2 * L - 3)
        out.append((g_proj, g_gls, pmin, float(y @ y) / g_proj, g_proj < chi, g_gls < chi))
    return out


@pytest.fixture(scope="module")
def forms():
    return {name: both_forms(fc.scenario(name)) for name in TRIANGULATING}


def test_residual_form_agrees_with_the_projected_form(forms):
    for name, rows in forms.items():
        assert rows, name
        gp, gg = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
        dg = fc.per_track_rel(gg, gp)
        print(f"{name}: {len(rows)} tracks, per-track gamma {dg.max():.2e}, |y|^2 / gamma <= {max(r[3] for r in rows):.3g}")
        assert dg.max() <= fc.GAMMA_TOL, (name, int(np.argmax(dg)), dg.max())
        assert [r[4] for r in rows] == [r[5] for r in rows], name


def test_pivot_threshold_separates_triangulating_tracks_from_constant_attitude(forms):
    thr = pivot_min()
    lo = {name: min(r[2] for r in rows) for name, rows in forms.items()}
    worst = min(lo, key=lo.get)
    const = both_forms(constant_attitude())
    hi = max(r[2] for r in const)
    print(f"smallest unit-diagonal pivot of C over the triangulating families: {lo[worst]:.2e} ({worst}); "
          f"largest on the constant-attitude window: {hi:.2e} ({len(const)} tracks); threshold {thr:.1e}")
    assert len(const) == len(fc.scenario("forward")["trk_off"]) - 1
    assert lo[worst] > thr, (worst, lo[worst])
    assert hi < thr, hi
    # the threshold sits well inside the gap, in both directions
    assert lo[worst] > 1e2 * thr and abs(hi) < 1e-2 * thr
