"""The update entries of csrc/xk_update_api.hip.h share one queued pass, one redo after a single launch that gave up and one record of how
far the staged update has got (xk_handle::upd).  Two things no other file runs:

1. The redo through the entries test_gpu_fused_kalman.py does not take it through: the two-call form, the reference-shaped
   xk_msckf_build + xk_qr_compress + xk_apply_update, the pass with correction_total != 0, xk_run_steps and xk_bench_staged -- on a shape
   where the two-call form defers the compression behind xk_apply_update (n = 177) and on one the split compression serves (n = 345).  The
   lab option "caqr_poison" raises the abort word before the launch: it leaves at once, nothing stalls.
2. A pass that is queued and never collected: the inputs are staged again and another frame runs.  Restaging drops the whole record, so the
   new frame owes nothing to the abandoned one.

Same frames, expectations and bounds as test_gpu_schedule_transitions.py: inlier masks equal, rel |dP| <= 1e-8, correction <= 1e-6, against the
C oracle (the NumPy composition of tests/aux_rows_np.py for the pass)."""
import ctypes as C

import numpy as np
import pytest

from helpers import rel
from test_gpu_schedule_transitions import FAMILIES, SCHEDULE, _check_frame, _corr_total, _expect, _run, _stage

pytestmark = pytest.mark.gpu

# family -> (kind of the frame whose single launch gives up, kind of the frame after it)
RETRY_SHAPES = {"D": ("tracks+slam", "small"), "S": ("rejected", "full")}
RETRY_ENTRIES = ("two_call", "reference", "pass", "run_steps", "bench_staged")


def _check(eng, got, exp, what, sched):
    """_check_frame with the schedule word given: after a give-up the single launch is off for the next `caqr_rearm` (64) updates, so the
    recorded SCHEDULE table does not apply."""
    corr, inl, inls = got
    P = eng.download_P()
    assert np.array_equal(np.asarray(inl).astype(int), np.asarray(exp["inlier"]).astype(int)), (what, "MSCKF inlier mask")
    assert np.array_equal(np.asarray(inls).astype(int), np.asarray(exp["inlier_slam"]).astype(int)), (what, "SLAM inlier mask")
    rp, rc = rel(P, exp["P"]), rel(corr, exp["correction"])
    print(what, "rel dP", rp, "rel dcorr", rc)
    assert rp <= 1e-8 and rc <= 1e-6, (what, rp, rc)
    assert eng.caqr_status()["schedule"] == sched, (what, eng.caqr_status(), sched)


def _after_giveup(fam, kind, entry):
    """Schedule word of a frame once the single launch has stepped aside: the multi-launch schedule (0) wherever SCHEDULE records a single
    launch (2); frames that are not compressed (4) stay so."""
    want = SCHEDULE[fam][kind]
    s = want.get(entry, want["*"])
    return 0 if s == 2 else s


@pytest.mark.parametrize("fam", sorted(RETRY_SHAPES))
@pytest.mark.parametrize("entry", RETRY_ENTRIES)
def test_single_launch_that_gives_up_is_redone_through_every_entry(xk, oracle_c, fam, entry):
    N, Mmax, Kmax, _, kinds = FAMILIES[fam]
    k1, k2 = RETRY_SHAPES[fam]
    sc1, sc2 = kinds[k1](), kinds[k2]()
    n = 15 + 6 * N + 3 * Mmax
    ct = _corr_total(n, 8600 + n) if entry == "pass" else None
    eng = xk.LabEngine(N, Mmax, Kmax)
    try:
        eng.set_option("caqr_poison", 1)
        _stage(eng, sc1)
        if entry in ("run_steps", "bench_staged"):
            # (both leave the prior resident: the entries raise on a status other than XK_OK)
            if entry == "run_steps":
                eng.run_steps(sc1["sigma_img"], 2)
            else:
                eng.bench_staged(sc1["sigma_img"], 0, 2)
            assert eng.caqr_status()["giveups"] == 1, eng.caqr_status()
            assert rel(eng.download_P(), sc1["P"]) == 0.0
            entry2 = "staged"
            got = _run(eng, entry2, sc1, None)      # the same staged frame right after
        else:
            entry2 = entry
            got = _run(eng, entry, sc1, ct)
        _check(eng, got, _expect(oracle_c, fam, k1, sc1, ct), (fam, entry, k1), 0)
        assert eng.caqr_status()["giveups"] == 1, eng.caqr_status()
        # nothing of the redo reaches the next frame
        eng.set_option("caqr_poison", 0)
        _stage(eng, sc2)
        got = _run(eng, entry2, sc2, ct)
        _check(eng, got, _expect(oracle_c, fam, k2, sc2, ct), (fam, entry, k1, k2), _after_giveup(fam, k2, entry2))
        assert eng.caqr_status()["giveups"] == 1, eng.caqr_status()
    finally:
        eng.close()


# (family, how the abandoned frame was queued, its kind, the kind of the frame that runs instead)
ABANDONED = [
    ("D", "queued", "slam_only", "tracks+slam"),    # B's two-call form defers its compression
    ("D", "two_call", "tracks+slam", "small"),      # A's compression was deferred and never ran
    ("S", "queued", "full", "rejected"),
]


@pytest.mark.parametrize("entry", ["two_call", "reference", "queued"])
@pytest.mark.parametrize("fam,start,ka,kb", ABANDONED, ids=[f"{f}-{s}" for f, s, _, _ in ABANDONED])
def test_abandoned_pass_does_not_reach_the_next_frame(xk, oracle_c, fam, start, ka, kb, entry):
    """Frame A is queued (xk_build_compress_update_async, or xk_build_compress_async whose xk_apply_update never comes) and not collected;
    frame B, staged over it, must come out as B."""
    N, Mmax, Kmax, _, kinds = FAMILIES[fam]
    sa, sb = kinds[ka](), kinds[kb]()
    eng = xk.Engine(N, Mmax, Kmax)
    try:
        _stage(eng, sa)
        fn = eng.L.xk_build_compress_update_async if start == "queued" else eng.L.xk_build_compress_async
        eng._chk(fn(eng.h, C.c_double(sa["sigma_img"])), start)
        _stage(eng, sb)
        got = _run(eng, entry, sb, None)
        _check_frame(eng, entry, kb, got, _expect(oracle_c, fam, kb, sb, None), (fam, entry, start, ka, kb))
    finally:
        eng.close()
