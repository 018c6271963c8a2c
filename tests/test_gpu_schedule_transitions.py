"""Schedule transitions on one handle.  launch_compress forms the measurement system afresh for every frame, from that frame's stack
(xk_caqr_status schedule): the whole stack compressed into d_R (0 / 2 / 3), the split compression of the tracks' rows into d_R2 (2, n > 206 with
SLAM features), the SLAM rows alone or a small stack as built in d_R2 (4), or no rows at all (4).  A filter moves between these from one frame
to the next, and what one frame leaves behind -- the contents of d_R2, the record of the last compression that compressed_spec follows (xk_handle::last), the
plan the rows were built for --
must never reach the next one's posterior.

Each family of frames shares one handle shape; a de Bruijn sequence over its kinds takes every ordered pair of kinds (repeats included) once,
through each entry point: xk_visual_update_staged, the queued pass, the two-call form of the MULTI_UAV order (which defers the compression
behind xk_apply_update where n <= 206), the reference-shaped xk_msckf_build + xk_qr_compress + xk_apply_update, and the IEKF pass with
correction_total != 0.  Every kind has its own inputs and prior, so a leftover value can never pass for a fresh one.  Every frame is checked
against the C oracle (the NumPy composition of tests/aux_rows_np.py for the sun rows and for the pass)."""
import ctypes as C

import numpy as np
import pytest

import aux_rows_np as A
from helpers import rel
from x_multi_agent_amd import synth

pytestmark = pytest.mark.gpu


def _empty(sc):
    """The same window, prior and n with no measurement row at all: no track, no SLAM feature."""
    e = {k: v for k, v in sc.items() if not k.startswith("slam_")}
    e["trk_off"] = np.zeros(1, dtype=np.int32)
    e["obs_xy"] = np.zeros((0, 2))
    return e


def _sun_only(sc):
    return dict(_empty(sc), sun=synth.make_sun(61, err_deg=2.0))


# family: (N, Mmax, Kmax, entry points, {kind: scenario}).
FAMILIES = {
    # config 2's shape (n = 345): the split compression (d_R2, mode 1) next to the small stack and the SLAM rows alone
    "S": (30, 50, 200, ("staged", "queued", "two_call", "reference", "pass"), {
        "full": lambda: synth.make_config(2),
        "rejected": lambda: synth.make_scenario(30, 200, 50, seed=8102, outlier_frac=0.4),
        "slam_only": lambda: synth.make_scenario(30, 0, 50, seed=8103),
        "small": lambda: synth.make_scenario(30, 6, 50, seed=8104, track_len=(4, 14)),
        "empty": lambda: _empty(synth.make_scenario(30, 0, 50, seed=8105)),
        "sun_only": lambda: _sun_only(synth.make_scenario(30, 0, 50, seed=8106)),
    }),
    # the split compression in the wide geometry: 6 N + 1 = 199 > 192 columns (n = 396)
    "W": (33, 61, 120, ("staged", "reference"), {
        "full": lambda: synth.make_scenario(33, 120, 61, seed=8201),
        "small": lambda: synth.make_scenario(33, 6, 61, seed=8202, track_len=(4, 14)),
        "slam_only": lambda: synth.make_scenario(33, 0, 61, seed=8203),
    }),
    # n = 177 <= 206 with SLAM rows: the two-call form defers the compression behind xk_apply_update
    "D": (12, 30, 120, ("staged", "queued", "two_call", "reference", "pass"), {
        "tracks+slam": lambda: synth.make_scenario(12, 120, 30, seed=8301),
        "slam_only": lambda: synth.make_scenario(12, 0, 30, seed=8302),
        "small": lambda: synth.make_scenario(12, 3, 30, seed=8303, track_len=(3, 8)),
        "empty": lambda: _empty(synth.make_scenario(12, 0, 30, seed=8304)),
        "sun_only": lambda: _sun_only(synth.make_scenario(12, 0, 30, seed=8305)),
    }),
    # the headline shape (N = 30, no SLAM feature, n = 195)
    "H": (30, 0, 400, ("staged", "queued", "two_call", "reference"), {
        "full": lambda: synth.make_config(4),
        "mid": lambda: synth.make_scenario(30, 20, 0, seed=8401, track_len=(4, 20)),
        "small": lambda: synth.make_scenario(30, 3, 0, seed=8402),
        "empty": lambda: _empty(synth.make_scenario(30, 3, 0, seed=8403)),
    }),
    # tall windows (128-row slots, config 3): the multi-launch schedule and its tail launch
    "T": (50, 0, 800, ("staged", "reference"), {
        "full": lambda: synth.make_config(3),
        "small": lambda: synth.make_scenario(50, 3, 0, seed=8501, track_len=(10, 40)),
        "empty": lambda: _empty(synth.make_scenario(50, 3, 0, seed=8502)),
    }),
}
# xk_caqr_status schedule word per family, kind and entry point, as the library reported it before launch_compress was split into one
# function per schedule (recorded on an MI355X from that build, every frame of the de Bruijn sequences below; not derived from the code):
# 0 multi-launch, 2 single launch, 3 multi-launch + tail, 4 nothing compressed.  "*": every entry point but the ones named beside it.
SCHEDULE = {
    "D": {
        "empty": {"*": 4},
        "slam_only": {"*": 4, "reference": 2},
        "small": {"*": 4, "reference": 2},
        "sun_only": {"*": 4},
        "tracks+slam": {"*": 2},
    },
    "H": {
        "empty": {"*": 4},
        "full": {"*": 2},
        "mid": {"*": 2},
        "small": {"*": 4, "reference": 2},
    },
    "S": {
        "empty": {"*": 4},
        "full": {"*": 2},
        "rejected": {"*": 2},
        "slam_only": {"*": 4, "reference": 2},
        "small": {"*": 4, "reference": 2},
        "sun_only": {"*": 4},
    },
    "T": {
        "empty": {"*": 4},
        "full": {"*": 3},
        "small": {"*": 0, "staged": 4},
    },
    "W": {
        "full": {"*": 2},
        "slam_only": {"*": 2, "staged": 4},
        "small": {"*": 2, "staged": 4},
    },
}
NO_ROWS = {"empty", "sun_only"}


def de_bruijn(m):
    """B(m, 2) as a path: m^2 + 1 symbols in which every ordered pair (a, b) of 0..m-1 follows once."""
    a, seq = [0] * 3, []

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, m):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return seq + seq[:1]


def _dims(sc):
    return len(sc["trk_off"]) - 1, len(sc["slam_anchor_idxs"]) if "slam_anchor_idxs" in sc else 0


def _corr_total(n, seed):
    return 1e-3 * np.random.default_rng(seed).standard_normal(n)


_EXP = {}


def _expect(oracle_c, fam, kind, sc, ct):
    """-> dict(P, correction, inlier, inlier_slam) of this kind's frame; with ct: the pass with correction_total = ct."""
    key = (fam, kind, ct is not None)
    if key in _EXP:
        return _EXP[key]
    K, M = _dims(sc)
    if ct is None and kind not in NO_ROWS:
        e = oracle_c.visual_update(sc)
        e = dict(P=e["P"], correction=e["correction"], inlier=e["inlier"], inlier_slam=e["inlier_slam"] if M else np.zeros(0, int))
    else:
        o = A.stacked_update(sc, sun=sc.get("sun"))
        if ct is None:
            P, corr = o["P"], o["correction"]
        elif o["h"].shape[0] == 0:                 # (no row at all: K = 0 in applyUpdate, the correction is -correction_total)
            P, corr = sc["P"].copy(), -ct
        else:
            P, corr = A.R.apply_update(sc["P"], o["h"], o["res"], o["r_diag"], ct, True)
        e = dict(P=P, correction=corr, inlier=np.asarray(o["msckf"]["inlier"]),
                 inlier_slam=np.asarray(o["slam"]["inlier"]) if M else np.zeros(0, int))
    _EXP[key] = e
    return e


def _fetch_flags(eng):
    K, M = max(eng._K, 1), max(eng._M, 1)
    inl, inls = np.zeros(K, np.int32), np.zeros(M, np.int32)
    rc = eng.L.xk_fetch_flags(eng.h, inl.ctypes.data_as(C.POINTER(C.c_int)), None, inls.ctypes.data_as(C.POINTER(C.c_int)), None)
    assert rc == 0, (rc, eng.L.xk_last_error(eng.h))
    return inl[:eng._K], inls[:eng._M]


def _stage(eng, sc):
    eng.stage(sc)                                  # window, tracks, SLAM features, prior
    eng.stage_msckf_slam([])                       # (MSCKF-SLAM tracks persist until restaged)
    if "sun" in sc:
        s = sc["sun"]
        eng.stage_sun_angle(s["q"], s["x"], s["y"], s.get("calib"))


def _run(eng, entry, sc, ct):
    """One frame through one entry point -> (correction, inlier, inlier_slam)."""
    sig = sc["sigma_img"]
    if entry == "staged":
        r = eng.visual_update_staged(sig)
        return r["correction"], r["inlier"], r["inlier_slam"]
    if entry == "reference":
        f = eng.msckf_build(sig)
        eng.qr_compress(want=False)
        return eng.apply_update(None, True), f["inlier"], f["inlier_slam"]
    if entry == "queued":
        eng._chk(eng.L.xk_build_compress_update_async(eng.h, C.c_double(sig)), "xk_build_compress_update_async")
        corr = eng.apply_update(None, True)
    elif entry == "two_call":
        eng._chk(eng.L.xk_build_compress_async(eng.h, C.c_double(sig)), "xk_build_compress_async")
        corr = eng.apply_update(None, True)
    else:
        assert entry == "pass"
        eng.build_compress_update_pass_async(sig, ct, True)
        corr = eng.apply_update(ct, True)
    return (corr,) + _fetch_flags(eng)


def _check_frame(eng, entry, kind, got, exp, what):
    corr, inl, inls = got
    P = eng.download_P()
    assert np.array_equal(np.asarray(inl).astype(int), np.asarray(exp["inlier"]).astype(int)), (what, "MSCKF inlier mask")
    assert np.array_equal(np.asarray(inls).astype(int), np.asarray(exp["inlier_slam"]).astype(int)), (what, "SLAM inlier mask")
    rp, rc = rel(P, exp["P"]), rel(corr, exp["correction"])
    assert rp <= 1e-8 and rc <= 1e-6, (what, rp, rc)
    sched = eng.caqr_status()["schedule"]
    want = SCHEDULE[what[0]][kind]
    assert sched == want.get(entry, want["*"]), (what, sched, want)


CASES = [(f, e) for f in sorted(FAMILIES) for e in FAMILIES[f][3]]


@pytest.mark.parametrize("fam,entry", CASES, ids=[f"{f}-{e}" for f, e in CASES])
def test_every_transition_of_a_family(xk, oracle_c, fam, entry):
    N, Mmax, Kmax, _, kinds = FAMILIES[fam]
    names = sorted(kinds)
    scs = {k: kinds[k]() for k in names}
    n = 15 + 6 * N + 3 * Mmax
    assert all(s["P"].shape == (n, n) for s in scs.values())
    m = len(names)
    seq = de_bruijn(m)
    assert len(seq) == m * m + 1 and {(a, b) for a, b in zip(seq, seq[1:])} == {(a, b) for a in range(m) for b in range(m)}
    ct = _corr_total(n, 8600 + n) if entry == "pass" else None
    exps = {k: _expect(oracle_c, fam, k, scs[k], ct) for k in names}
    eng = xk.Engine(N, Mmax, Kmax)
    try:
        for i, j in enumerate(seq):
            kind = names[j]
            sc = scs[kind]
            _stage(eng, sc)
            got = _run(eng, entry, sc, ct)
            prev = names[seq[i - 1]] if i else None
            _check_frame(eng, entry, kind, got, exps[kind], (fam, entry, i, prev, kind))
    finally:
        eng.close()


@pytest.mark.parametrize("fam,kind", [("D", "small"), ("S", "full")])
@pytest.mark.parametrize("built,applied", [(0, 1), (1, 0)])
def test_slam_split_changed_between_build_and_apply(xk, oracle_c, fam, kind, built, applied):
    """The compression follows what the rows were built for, not the option as it stands when xk_apply_update runs it."""
    N, Mmax, Kmax, _, kinds = FAMILIES[fam]
    sc = kinds[kind]()
    exp = _expect(oracle_c, fam, kind, sc, None)
    eng = xk.Engine(N, Mmax, Kmax)
    try:
        eng.set_option("slam_split", built)
        _stage(eng, sc)
        eng._chk(eng.L.xk_build_compress_async(eng.h, C.c_double(sc["sigma_img"])), "xk_build_compress_async")
        eng.set_option("slam_split", applied)
        corr = eng.apply_update(None, True)
        inl, inls = _fetch_flags(eng)
        assert np.array_equal(inl, exp["inlier"]) and np.array_equal(inls, exp["inlier_slam"])
        P = eng.download_P()
        assert rel(P, exp["P"]) <= 1e-8 and rel(corr, exp["correction"]) <= 1e-6, (rel(P, exp["P"]), rel(corr, exp["correction"]))
    finally:
        eng.close()


@pytest.mark.parametrize("entry", ["reference", "two_call"])
def test_empty_update_reports_nothing_compressed(xk, entry):
    """A frame without a measurement row after one the split compression served: P and the correction untouched, schedule 4."""
    N, Mmax, Kmax, _, kinds = FAMILIES["S"]
    full, empty = kinds["full"](), kinds["empty"]()
    eng = xk.Engine(N, Mmax, Kmax)
    try:
        _stage(eng, full)
        _run(eng, entry, full, None)
        assert eng.caqr_status()["schedule"] != 4
        _stage(eng, empty)
        corr, _, _ = _run(eng, entry, empty, None)
        assert eng.caqr_status()["schedule"] == 4
        assert rel(eng.download_P(), empty["P"]) <= 1e-12 and not np.any(corr)
    finally:
        eng.close()
