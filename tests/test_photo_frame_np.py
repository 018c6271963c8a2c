"""The scenes of tests/photo_frame_cases.py verified from the restatement alone (photo_frame_np.PhotoTrackerNp), without a GPU: every
frame's margins (the tracking's, the RANSAC's, the gain RANSAC's, the float cast of the resident positions, the distance of every
truncated coordinate from an integer, the size of every gain component the relative bound is applied to), the events each scene is
there for, and the intensity bookkeeping of a frame -- the gathers of photo_frame_np.bookkeeping -- against a literal list walk of
tracker.cpp:658-686 and :222-227."""
import numpy as np
import pytest

import klt_np as knp
import photo_cases as phc
import photo_frame_cases as pc
import photo_frame_np as pfn
import photo_np as pnp
from test_tracker_frame_np import float_boundary_margin


def frames(name):
    """(sequence, frame, result) of every frame that returned."""
    return [(si, fi, r) for si, seq in enumerate(pc.restated(name)) for fi, r in enumerate(seq) if not isinstance(r, Exception)]


@pytest.mark.parametrize("name", list(pc.SCENES))
def test_every_margin_of_every_frame(name):
    sc = pc.SCENES[name]
    assert all(len(seq) <= 8 and all(im.shape == (pc.H, pc.W) and im.dtype == np.uint8 for im in seq) for seq in sc["sequences"])
    assert sc["max_matches"] <= 320
    for si, fi, r in frames(name):
        at = (name, si, fi)
        klt, which = knp.worst_margin(list(r["klt_margins"]) + list(r["cal_margins"]))
        cast, _ = float_boundary_margin(r["features"]["dist_xy"])
        tr = np.concatenate(r["truncated"] + [np.zeros(0)])
        trunc = float(np.abs(tr - np.rint(tr)).min()) if len(tr) else np.inf
        print(at, "KLT margin", klt, which, "RANSAC margin", r["ransac_margin"], "float boundary", cast, "truncation", trunc)
        assert klt >= 1e-9, (at, which)
        assert r["ransac_margin"] >= 1e-6, at
        assert cast >= 1e-9, at
        assert trunc >= 1e-9, at                                     # (a tracked coordinate within 1e-9 of an integer could truncate differently)
        assert len(r["features"]["dist_xy"]) <= sc["max_matches"]
        if r["estimated"]:
            # what the relative bound photo_cases.close is applied to: no component so small that its round-off alone exceeds the bound
            v = np.concatenate([[r["a_rel"], r["b_rel"]], r["frame_ab"], r["ring"][-1]])
            assert np.abs(v).min() >= 1e-2, (at, v)
            if r["cal_ransac"] is not None:
                assert r["cal_ransac"]["margin"] >= phc.MARGIN, at


def test_gain_walk_estimates_redetects_overflows_and_corrects():
    fr = [r for _, _, r in frames("gain_walk")]
    assert len(fr) == 6 and fr[0]["n_matches"] == 0 and not fr[0]["estimated"] and not fr[0]["done"]
    assert np.array_equal(fr[0]["raw"], fr[0]["working"])                        # no calibration on a first frame
    later = fr[1:]
    assert all(r["estimated"] and r["done"] and r["support"] >= 5 for r in later)
    assert [len(r["ring"]) for r in fr] == [1, 2, 3, 4, 5, 6]
    assert any(r["redetected"] and r["n_new_tracked"] > 0 for r in later[1:])     # a re-detection after done
    assert any(r["n_left"] < r["n_tracked"] for r in later)                      # the overflow pass removed a pair
    assert all((r["raw"] != r["working"]).any() for r in later)
    assert all(r["desc"].any() and r["n_matches"] >= 7 for r in later)
    # every match carries both intensities, and the resident list the current ones
    for r in later:
        assert len(r["prev_intensity"]) == len(r["cur_intensity"]) == r["n_matches"]
        assert np.array_equal(r["features"]["intensity"], r["cur_intensity"]) and (r["cur_intensity"] > 0).all()
    # a re-detected pair's previous intensity was taken on the previous WORKING plane, a tracked pair's on an earlier raw plane
    r = later[2]
    assert (r["origin"] < 0).any() and (r["origin"] >= 0).any()


def test_switch_redetects_with_the_new_threshold_on_the_frame_of_the_first_estimate():
    a, b = [r for _, _, r in frames("gain_walk")], [r for _, _, r in frames("switch")]
    assert pc.SCENES["switch"]["threshold_photo"] != pc.SCENES["switch"]["threshold"]
    assert a[0]["n_candidates"] == b[0]["n_candidates"]                           # the first frame: the first threshold in both
    assert not b[0]["done"] and b[1]["estimated"] and b[1]["redetected"] and a[1]["redetected"]
    assert b[1]["n_candidates"] != a[1]["n_candidates"] and b[1]["n_candidates"] > 0


def test_dense_calibrates_more_than_257_features():
    fr = [r for _, _, r in frames("dense")]
    assert fr[0]["n_accepted"] > 257
    # the refit workgroup and the compaction's 256-wide chunk see more than one pass, the last tracking workgroup is not full
    assert fr[1]["estimated"] and fr[1]["n_cal_kept"] > 257 and fr[0]["n_accepted"] % 4 != 0 and fr[1]["n_tracked"] > 0


def test_starved_edges():
    s = pc.restated("starved")
    one, two = s[0][1], s[1][1]
    assert (one["n_tracked"], one["n_left"]) == (1, 1) and (two["n_tracked"], two["n_left"]) == (2, 1)
    # three resident features before done: no calibration tracking, no estimate, nothing corrected; then an empty resident list
    a = s[2]
    assert a[0]["n_accepted"] == 3 and (a[1]["n_cal_kept"], a[1]["estimated"], a[1]["done"]) == (0, False, False)
    assert np.array_equal(a[1]["raw"], a[1]["working"]) and a[1]["n_tracked"] == 3 and a[1]["n_matches"] == 0
    assert len(a[1]["features"]["dist_xy"]) == 0 and (a[2]["n_tracked"], a[2]["redetected"]) == (0, 1) and a[2]["n_accepted"] > 0
    # four resident features of which the calibration keeps three, before done: the ring does not advance, nothing is corrected
    b = s[3]
    assert b[0]["n_accepted"] == 4 and (b[1]["n_cal_kept"], b[1]["estimated"], b[1]["done"]) == (3, False, False)
    assert len(b[1]["ring"]) == 1 and np.array_equal(b[1]["raw"], b[1]["working"])
    # the long sequence: done from its frame 1; lists of 6 and 7 pairs into the RANSAC; an empty list after the six
    c = s[4]
    assert c[0]["n_accepted"] == 7 and c[1]["estimated"] and c[1]["done"] and c[1]["n_cal_kept"] == 7
    assert (c[2]["n_total"], c[2]["n_matches"], c[2]["winner"]) == (6, 0, -1)
    assert (c[3]["n_total"], c[3]["n_matches"]) == (7, 7) and c[3]["winner"] >= 0
    assert (c[4]["n_left"], c[4]["n_total"], c[4]["n_matches"], c[4]["winner"]) == (6, 6, 0, -1) and c[4]["estimated"]
    assert (c[5]["n_tracked"], c[5]["redetected"]) == (0, 1) and not c[5]["estimated"]
    ring = c[5]["ring"]
    # after done: three resident features are corrected with the ring as it stands
    d = s[5]
    assert (d[1]["n_cal_kept"], d[1]["estimated"], d[1]["done"]) == (0, False, True) and d[1]["ring"] == ring
    assert np.array_equal(d[1]["working"], pnp.correct(d[1]["raw"], *ring[-1])) and (d[1]["working"] != d[1]["raw"]).any()
    assert np.array_equal(d[0]["working"], d[0]["raw"])                           # (a first frame is never corrected)
    # ... and so are four of which the calibration keeps three: the ring does not advance
    e = s[6]
    assert (e[1]["n_cal_kept"], e[1]["estimated"], e[1]["done"]) == (3, False, True) and e[1]["ring"] == ring
    assert np.array_equal(e[1]["working"], pnp.correct(e[1]["raw"], *ring[-1]))


def test_blank_detects_nothing():
    for _, _, r in frames("blank"):
        assert all(r[k] == 0 for k in ("n_tracked", "n_left", "redetected", "n_candidates", "n_accepted", "n_new_tracked", "n_matches"))
        assert not r["estimated"] and not r["done"] and len(r["features"]["dist_xy"]) == 0


def test_full_runs_out_of_room_after_its_calibration_and_starts_again():
    seq = pc.restated("full")[0]
    assert not isinstance(seq[1], Exception) and seq[1]["n_matches"] > 0 and len(seq[1]["ring"]) == 2
    e = seq[2]
    assert isinstance(e, pfn.CapacityError) and e.counts["redetected"] == 1
    assert e.calibration["estimated"] and len(e.ring) == 3                        # the calibration before the error advanced the ring
    fresh = pc.tracker_np("full")
    fresh.state = dict(ring=list(e.ring), done=True)
    first = fresh.track(pc.SCENES["full"]["sequences"][0][3], seed=pc.SEED + 3)
    assert seq[3]["n_matches"] == 0 and seq[3]["n_accepted"] == first["n_accepted"] > 0 and not seq[3]["estimated"]
    for k, v in fresh.features.items():
        assert np.array_equal(seq[3]["features"][k], v)


def test_spatial_accumulates_rows_on_every_estimating_frame():
    fr = [r for _, _, r in frames("spatial")]
    rows = [r["sp_rows"] for r in fr]
    assert rows[0] == 0 and all(r["estimated"] for r in fr[1:])
    assert all(b > a for a, b in zip(rows, rows[1:])), rows
    plain = [r for _, _, r in frames("gain_walk")]
    for a, b in zip(fr, plain):                                                   # accumulating changes nothing else
        assert a["n_matches"] == b["n_matches"] and np.array_equal(a["working"], b["working"])


# ---- the intensity bookkeeping against a literal list walk ----
class _Feat:
    def __init__(self, ident, intensity):
        self.ident, self.intensity = ident, intensity


def _list_walk(res_int, status1, cur_int1, erase, new_int, status2, cur_int2, mask):
    """tracker.cpp:658-686 (features1 erased where the status is 0, features2 built beside it with its own intensity), the overflow
    pass's erases from the back, the same post-filter on the new features, :222-227 (insert at the end of both lists), and the
    mask of the outlier removal (:286-293), on lists of objects."""
    def post_filter(features1, status, cur_int):
        features2, it = [], 0
        cur_int = list(cur_int)
        for i in range(len(status)):
            if not status[i]:
                del features1[it]
                continue
            features2.append(_Feat(features1[it].ident, cur_int.pop(0)))      # computeIntensity(img2, ...), :666
            it += 1
        return features2

    f1 = [_Feat(i, v) for i, v in enumerate(res_int)]
    f2 = post_filter(f1, status1, cur_int1)
    for i in range(len(f2) - 1, -1, -1):
        if erase[i]:
            del f1[i], f2[i]
    n1 = [_Feat(-(k + 1), v) for k, v in enumerate(new_int)]
    n2 = post_filter(n1, status2, cur_int2)
    f1.extend(n1), f2.extend(n2)                                               # :224-225
    out = [(a, b) for a, b, m in zip(f1, f2, mask) if m]
    return [a.intensity for a, _ in out], [b.intensity for _, b in out], [a.ident for a, _ in out]


def test_bookkeeping_equals_the_list_walk():
    rng = np.random.default_rng(11)
    for trial in range(300):
        n = trial if trial < 3 else int(rng.integers(0, 40))
        n_new = (0, 1, 2)[trial % 3] if trial < 9 else int(rng.integers(0, 20))
        res_int = rng.uniform(0, 1, n)
        status1 = rng.uniform(size=n) < 0.8
        keep1 = np.flatnonzero(status1)
        cur_int1 = rng.uniform(0, 1, len(keep1))
        erase = rng.uniform(size=len(keep1)) < 0.3
        stay = np.flatnonzero(~erase)
        new_int = rng.uniform(0, 1, n_new)
        status2 = rng.uniform(size=n_new) < 0.7
        keep2 = np.flatnonzero(status2)
        cur_int2 = rng.uniform(0, 1, len(keep2))
        mask = rng.uniform(size=len(stay) + len(keep2)) < 0.6
        kept3 = np.flatnonzero(mask)
        ip, ic = pfn.bookkeeping(res_int, keep1, cur_int1, stay, new_int, keep2, cur_int2, kept3)
        wp, wc, ident = _list_walk(res_int, status1, cur_int1, erase, new_int, status2, cur_int2, mask)
        assert ip.tolist() == wp and ic.tolist() == wc, (trial, n, n_new)
        origin = np.concatenate([keep1[stay], -(keep2 + 1)])[kept3]
        assert origin.tolist() == ident, trial
