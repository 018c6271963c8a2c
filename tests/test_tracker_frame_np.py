"""The scenes of tests/tracker_frame_cases.py verified from the restatement alone (tracker_frame_np.TrackerNp), without a GPU:
every frame's margins, the events each scene is there for on the frames named, and the overflow pass as a mask against the
reference's sequential erase loop."""
import numpy as np
import pytest

import fast_np as fastnp
import klt_np as knp
import tracker_frame_cases as tc
import tracker_frame_np as tnp


def frames(name):
    """(sequence, frame, result) of every frame that returned."""
    return [(si, fi, r) for si, seq in enumerate(tc.restated(name)) for fi, r in enumerate(seq) if not isinstance(r, Exception)]


def float_boundary_margin(xy):
    """-> (px, rel): the smallest distance of a coordinate from the nearest boundary between two float32 roundings (the midpoint of
    two adjacent floats), in pixels and relative to the coordinate.

    The device's own positions feed the next frame through a float cast (tracker.cpp:629-633), and tests/test_gpu_tracker_frame.py
    holds them within 1e-9 px of the restatement's: a position at least 1e-9 px from every boundary casts to the same float on both
    sides.  That is the margin asserted, in the unit of the bar it protects.  The same 1e-9 taken relative to the coordinate (1e-7 px
    at 100 px, where two boundaries are 7.6e-6 px apart) would exclude 2.6 % of all positions: no scene of some hundred coordinates
    meets it for any seed (0.974^400 = 3e-5 for the walk, 1e-11 for the dense scene), so it is printed, not asserted."""
    v = np.asarray(xy, np.float64).ravel()
    v = v[v != 0.0]
    if not len(v):
        return np.inf, np.inf
    f = v.astype(np.float32)
    lo = (f.astype(np.float64) + np.nextafter(f, np.float32(-np.inf)).astype(np.float64)) / 2.0
    hi = (f.astype(np.float64) + np.nextafter(f, np.float32(np.inf)).astype(np.float64)) / 2.0
    d = np.minimum(np.abs(v - lo), np.abs(v - hi))
    return float(d.min()), float((d / np.abs(v)).min())


@pytest.mark.parametrize("name", list(tc.SCENES))
def test_every_margin_of_every_frame(name):
    sc = tc.SCENES[name]
    assert all(len(seq) <= 8 and all(im.shape == (tc.H, tc.W) for im in seq) for seq in sc["sequences"]) and sc["max_matches"] <= 320
    for si, fi, r in frames(name):
        klt, which = knp.worst_margin(r["klt_margins"])
        cast, cast_rel = float_boundary_margin(r["features"]["dist_xy"])
        print(name, si, fi, "KLT margin", klt, which, "RANSAC margin", r["ransac_margin"], "float boundary", cast, "px", cast_rel, "relative")
        assert klt >= 1e-9, (name, si, fi, which)
        assert r["ransac_margin"] >= 1e-6, (name, si, fi)
        assert cast >= 1e-9, (name, si, fi)
        assert len(r["features"]["dist_xy"]) <= sc["max_matches"]


def test_walk_redetects_does_not_and_overflows():
    fr = [r for _, _, r in frames("walk")]
    assert len(fr) == 6 and fr[0]["n_accepted"] >= 30 and fr[0]["n_matches"] == 0
    later = fr[1:]
    assert [r["redetected"] for r in later] == [1, 1, 1, 0, 1]
    assert all(r["n_left"] < r["n_tracked"] for r in later)                       # the overflow pass removed a pair
    assert all(r["n_new_tracked"] > 0 and (r["origin"] < 0).sum() > 0 for r in later if r["redetected"])
    assert all(r["n_accepted"] == 0 and (r["origin"] >= 0).all() for r in later if not r["redetected"])
    assert all(r["n_matches"] >= 7 and r["desc"].any() for r in later)
    # a re-detected pair carries the detection's tile for its previous feature and a new Feature's for its current one
    r = later[0]
    new = r["origin"] < 0
    assert (r["tiles"][new, 2:] == -1).all() and (r["tiles"][~new] >= 0).all()


def test_dense_straddles_the_chunk_and_the_workgroup():
    fr = [r for _, _, r in frames("dense")]
    assert fr[0]["n_accepted"] > 257
    for r in fr[1:]:
        assert r["n_tracked"] > 256 and r["n_tracked"] % 4 != 0 and r["n_matches"] > 256 and not r["redetected"]


def test_starved_edges():
    seqs = tc.restated("starved")
    a = seqs[0]
    assert a[0]["n_accepted"] == 7
    assert (a[1]["n_left"], a[1]["n_matches"]) == (7, 7) and a[1]["winner"] >= 0          # seven pairs: the RANSAC's smallest sample
    assert (a[3]["n_left"], a[3]["n_matches"], a[3]["winner"]) == (6, 0, -1)              # six pairs keep nothing
    assert len(a[3]["features"]["dist_xy"]) == 0
    assert (a[4]["n_tracked"], a[4]["n_left"], a[4]["redetected"]) == (0, 0, 1)           # zero pairs: the re-detection starts from nothing
    assert a[4]["n_accepted"] > 0 and a[4]["n_new_tracked"] == a[4]["n_total"] < 7 and a[4]["n_matches"] == 0
    one, two = seqs[1][1], seqs[2][1]
    assert (one["n_tracked"], one["n_left"]) == (1, 1)                                     # the only pair is the last pair
    assert (two["n_tracked"], two["n_left"]) == (2, 1)                                     # both in one tile over its cap: the first goes


def test_blank_detects_nothing():
    for _, _, r in frames("blank"):
        assert all(r[k] == 0 for k in ("n_tracked", "n_left", "redetected", "n_candidates", "n_accepted", "n_new_tracked", "n_matches"))
        assert len(r["features"]["dist_xy"]) == 0


def test_full_runs_out_of_room_and_starts_again():
    seq = tc.restated("full")[0]
    assert isinstance(seq[2], tnp.CapacityError) and seq[2].counts["n_left"] + seq[2].counts["n_new_tracked"] > tc.SCENES["full"]["max_matches"]
    assert not isinstance(seq[1], Exception) and seq[1]["n_matches"] > 0
    # the frame after it is a first frame, and equals a fresh tracker's first frame on that image
    fresh = tc.tracker_np("full")
    first = fresh.track(tc.SCENES["full"]["sequences"][0][3], seed=tc.SEED + 3)
    assert seq[3]["n_matches"] == 0 and seq[3]["n_accepted"] == first["n_accepted"] > 0
    for k, v in fresh.features.items():
        assert np.array_equal(seq[3]["features"][k], v)


def test_overflow_mask_equals_the_sequential_erase_loop():
    rng = np.random.default_rng(5)
    for trial in range(300):
        n = trial if trial < 3 else int(rng.integers(0, 60))
        grid = fastnp.TileGrid(160, 120, int(rng.integers(1, 5)), int(rng.integers(1, 6)), int(rng.integers(0, 4)))
        cur = np.stack([rng.uniform(-0.5, 159.5, n), rng.uniform(-0.5, 119.5, n)], axis=1)
        prev = np.stack([rng.uniform(-0.5, 159.5, n), rng.uniform(-0.5, 119.5, n)], axis=1)
        keep, _, tiles_cur = fastnp.remove_overflow(grid, prev.tolist(), cur.tolist())
        mask, tiles = tnp.overflow_mask(grid, cur.tolist())
        assert np.flatnonzero(mask).tolist() == keep and tiles == tiles_cur, (trial, n)
