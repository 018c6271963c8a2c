"""The two forms of the per-feature gate (csrc/xk_feature.hip.h) against each other on the device: lab option "feat_gate_form" 1 (default;
generalised least squares on M itself, xk_chol_gate_gls, for tracks of at most 32 observations) and 0 (the projected form S = A^T M A
everywhere).  One update each on fresh handles: gamma agrees per track within the project's bar, between the two and against the C
oracle; everything else -- verdicts, Gauss-Newton iteration counts, triangulated points, posterior, correction -- is bit for bit the
same, because the reflectors and the record / tile write are moved, not changed.  Where the new form does not run (33 observations) or
hands the track back to the projected form (constant attitude: Hf of rank 2), gamma is bit for bit the same too."""
import numpy as np
import pytest

import feature_cases as fc
from test_gate_form_np import constant_attitude
from x_multi_agent_amd import synth

pytestmark = pytest.mark.gpu

# name -> (scenario, how gamma of the two settings must compare: "tol" = fc.GAMMA_TOL per track, "equal" = bit for bit)
SHAPES = {
    "circle": (lambda: fc.scenario("circle"), "tol"),
    "forward_ragged_n10": (lambda: fc.scenario("forward_ragged_n10"), "tol"),        # 2 .. 10 observations: a 4 x 4 M with a 4 x 3 Hf, one block
    "forward_ragged_n30": (lambda: fc.scenario("forward_ragged_n30"), "tol"),        # every block count 1 .. 4
    "full_n32": (lambda: synth.make_scenario(32, 8, 0, seed=3208), "tol"),           # 64 rows exactly: the last shape the four-block gate holds
    "full_n33": (lambda: synth.make_scenario(33, 8, 0, seed=3308), "equal"),         # 66 rows: keeps the projected path
    "stopped_slam_n30": (lambda: fc.scenario("stopped_slam_n30"), "tol"),            # the xk_build_rows body, NaN tracks
    "constant_attitude": (constant_attitude, "equal"),                               # the fallback ran: nothing else makes gamma equal
}


def _dims(sc):
    return sc["n_poses_max"], len(sc.get("slam_anchor_idxs", ())), len(sc["trk_off"]) - 1


def _update(eng, sc):
    eng.stage(sc)
    r = eng.visual_update_staged(sc["sigma_img"])
    gpf, it = eng.debug_feature_points()
    return dict(gamma=r["gamma"].copy(), inlier=r["inlier"].copy(), correction=r["correction"].copy(), P=eng.download_P(), gpf=gpf, it=it)


def _same_but_gamma(a, b, label):
    for key in ("inlier", "it", "gpf", "P", "correction"):
        assert np.array_equal(a[key], b[key], equal_nan=(key == "gpf")), (label, key)


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_two_forms_agree(xk, oracle_c, name):
    make, how = SHAPES[name]
    sc = make()
    N, M, K = _dims(sc)
    if name == "full_n32" or name == "full_n33":
        assert (fc.track_lengths(sc) == N).all()
    info = oracle_c.msckf_update(sc)[3]
    got = {}
    for form in (1, 0):
        eng = xk.LabEngine(N, M, K)
        eng.set_option("feat_gate_form", form)
        got[form] = _update(eng, sc)
        eng.close()
    new, old = got[1], got[0]
    _same_but_gamma(new, old, name)
    fin = np.isfinite(info["gamma"])
    for form in (1, 0):
        g = got[form]["gamma"]
        assert np.isfinite(g[fin]).all(), (name, form)
        if name != "constant_attitude":
            assert np.array_equal(np.isnan(g), np.isnan(info["gamma"])), (name, form)
    if how == "equal":
        assert np.array_equal(new["gamma"], old["gamma"], equal_nan=True), (name, np.where(new["gamma"] != old["gamma"])[0])
    else:
        dg = fc.per_track_rel(new["gamma"][fin], old["gamma"][fin])
        print(f"{name}: gamma, new form against projected form {dg.max():.2e} per track")
        assert dg.max() <= fc.GAMMA_TOL, (name, int(np.argmax(dg)), dg.max())
        assert (new["gamma"][fin] != old["gamma"][fin]).any(), name        # (the new form did run)
    if name != "constant_attitude":      # (there the oracle's own third direction is implementation-defined: finiteness only, above)
        for form in (1, 0):
            do = fc.per_track_rel(got[form]["gamma"][fin], info["gamma"][fin])
            print(f"{name}: gamma, form {form} against the C oracle {do.max():.2e} per track")
            assert do.max() <= fc.GAMMA_TOL, (name, form, int(np.argmax(do)), do.max())
            assert np.array_equal(got[form]["inlier"], info["inlier"]), (name, form)


def test_a_repeated_update_is_bit_for_bit(xk):
    """Three updates on one handle with the new form: the third repeats the second (the first runs the first-update geometry)."""
    sc = fc.scenario("forward_ragged_n30")
    N, M, K = _dims(sc)
    eng = xk.LabEngine(N, M, K)
    eng.set_option("feat_gate_form", 1)
    runs = [_update(eng, sc) for _ in range(3)]
    eng.close()
    _same_but_gamma(runs[2], runs[1], "repeat")
    assert np.array_equal(runs[2]["gamma"], runs[1]["gamma"], equal_nan=True)
    assert np.array_equal(runs[1]["gamma"], runs[0]["gamma"], equal_nan=True) and np.array_equal(runs[1]["inlier"], runs[0]["inlier"])
