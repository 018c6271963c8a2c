"""The second Lucas-Kanade parameter set of a PHOTOMETRIC_CALI build (Tracker::featureTracking, tracker.cpp:641-651; DESIGN 3.11 and
3.19) restated, and the cases of tests/test_klt_sets_np.py and tests/test_gpu_klt_sets.py.  No arithmetic of its own: klt_np's
pyramid and tracking, photo_frame_np's frame.

    deep_pyramid      an image's pyramid to a given level -- every image is built to the deeper of the two sets' levels, and each
                      tracking is handed its own first levels + 1 images
    TwoSetTrackerNp   PhotoTrackerNp with two sets: the feature trackings of a frame use set 1 once state["done"] is true at that
                      point of the frame (calibrateImage has run by then, tracker.cpp:849 before :193), set 0 before; the
                      calibration's own tracking between the raw images always gets set 0 (:784-787)

The window pairs (160 x 120 images):

    A   set 0: 31 x 31, max_level 2 -> levels 1;  set 1: 9 x 9, max_level 3 -> levels 3: the second set is deeper, the slots grow
    B   A's sets swapped: the second set is shallower
    C   set 1 an even, non-square window (12 x 7) with min_eig_thr raised to C_THR, under which some feature fails that set 0 keeps
    D   set 1 equal to set 0

The photometric sequence is photo_frame_cases' gain_walk behind one uniform image: the first frame detects nothing, frame 1 has an
empty resident list and re-detects on the uniform image, frame 2 re-detects on the first walk image and tracks what it found with
set 0, frame 3 is the first whose calibration has features to estimate from -- done becomes true there -- and frames 4 ... 6 follow."""
import contextlib
import functools
import math

import numpy as np

import klt_cases as kc
import klt_np as knp
import photo_frame_cases as pc
import photo_frame_np as pfn
import tracker_frame_cases as tc

W, H = pc.W, pc.H
C_THR = 0.01                               # min_eig_thr of C's set 1 (set 0 keeps the reference's 0.003)
SET_31 = dict(win=(31, 31), max_level=2, min_eig_thr=0.003)
SET_9 = dict(win=(9, 9), max_level=3, min_eig_thr=0.003)
PAIRS = {
    "A": (SET_31, SET_9),
    "B": (SET_9, SET_31),
    "C": (dict(win=(16, 16), max_level=1, min_eig_thr=0.003), dict(win=(12, 7), max_level=2, min_eig_thr=C_THR)),
    "D": (dict(win=(15, 15), max_level=2, min_eig_thr=0.003), dict(win=(15, 15), max_level=2, min_eig_thr=0.003)),
}
MAX_ITER, EPS = 30, 0.01                   # shared: the reference passes one term_crit_ to both calls

# the stage entry's case: two images of klt_cases and the first points of that scene, the edge points among them
STAGE_SCENE, STAGE_N = "w31_n257", 72


def levels_of(s):
    return knp.n_levels(W, H, s["win"], s["max_level"])


def deep_of(pair):
    return max(levels_of(PAIRS[pair][0]), levels_of(PAIRS[pair][1]))


def deep_pyramid(img, levels):
    """-> list of (image uint8, dIx int16, dIy int16) for levels 0 ... levels, whatever window asks for them."""
    img = np.ascontiguousarray(img, np.uint8)
    out = []
    for l in range(levels + 1):
        if l:
            img = knp.pyr_down(img)
        out.append((img,) + knp.scharr(img))
    return out


def _floor_apart(v, m):
    """klt_np._floor, with the floor of a whole number noted under a name of its own.  A detected feature sits on an integer pixel, and
    under an odd window (31, 9 and 7 here; klt_np's frame scenes all take even ones) its window's corner px 2^-l - (win - 1) / 2 is a
    whole or a half number that fp64 holds EXACTLY: the same bits on both sides, so that floor has nothing to decide although its
    distance to the next integer is 0.  Every other floor keeps the name "floor" and its 1e-9 bar."""
    f = math.floor(v)
    m.note("floor_whole" if v == f else "floor", min(v - f, f + 1.0 - v))
    return f


@contextlib.contextmanager
def _whole_floors_apart():
    keep, knp._floor = knp._floor, _floor_apart
    try:
        yield
    finally:
        knp._floor = keep


def track_set(pyr_prev, pyr_cur, prev_xy, s):
    """klt_np.track under set s on deep pyramids: the set's own first levels + 1 images."""
    n = levels_of(s) + 1
    with _whole_floors_apart():
        return knp.track(pyr_prev[:n], pyr_cur[:n], prev_xy, s["win"], MAX_ITER, EPS, s["min_eig_thr"])


def worst_margin(margins):
    """klt_np.worst_margin over every decision but the floors of whole numbers (see _floor_apart)."""
    return knp.worst_margin([{k: v for k, v in m.items() if k != "floor_whole"} for m in margins])


@functools.lru_cache(maxsize=None)
def stage_images():
    return tuple(np.ascontiguousarray(im[:, :W]) for im in kc.images(STAGE_SCENE))


def stage_points():
    return kc.points(STAGE_SCENE)[:STAGE_N]


@functools.lru_cache(maxsize=None)
def stage_restated(pair, which, reverse=False):
    """The stage case under set `which` of the pair; reverse: from the second image to the first (after a third push)."""
    a, b = stage_images()
    if reverse:
        a, b = b, a
    deep = deep_of(pair)
    return track_set(deep_pyramid(a, deep), deep_pyramid(b, deep), stage_points(), PAIRS[pair][which])


class TwoSetTrackerNp(pfn.PhotoTrackerNp):
    def __init__(self, *args, sets, force=None, **kw):
        """sets: (set 0, set 1); force: None -- the switch on state["done"] -- or the one set every feature tracking uses."""
        s0 = sets[0]
        super().__init__(*args, win=s0["win"], max_level=s0["max_level"], min_eig_thr=s0["min_eig_thr"], max_iter=MAX_ITER, eps=EPS, **kw)
        self.sets, self.force = sets, force
        self.deep = max(levels_of(sets[0]), levels_of(sets[1]))
        self.used = []                     # the set of every feature tracking, in call order
        self._deep = {}

    def _deep_pyr(self, pyr):
        """The deep pyramid of the image whose set-0 pyramid is `pyr` (kept for the two frames an image lives)."""
        key = id(pyr[0][0])
        if key not in self._deep:
            if len(self._deep) > 4:
                self._deep.pop(next(iter(self._deep)))
            self._deep[key] = (pyr[0][0], deep_pyramid(pyr[0][0], self.deep))
        return self._deep[key][1]

    def _track(self, pyr_prev, pyr_cur, dist_xy):
        which = self.force if self.force is not None else (1 if self.state["done"] else 0)
        self.used.append(which)
        r = track_set(self._deep_pyr(pyr_prev), self._deep_pyr(pyr_cur), np.asarray(dist_xy, np.float64).reshape(-1, 2).astype(np.float32),
                      self.sets[which])
        self.margins.extend(r["margins"])
        return r


def _sequence():
    return [np.full((H, W), 128, np.uint8)] + list(pc.SCENES["gain_walk"]["sequences"][0])


@functools.lru_cache(maxsize=None)
def scene(pair):
    """gain_walk's setups with the pair's sets (`second` is what Klt(..., second=) takes) on the sequence above."""
    s0, s1 = PAIRS[pair]
    return dict(pc.SCENES["gain_walk"], name="sets_" + pair, sequences=[_sequence()], win=s0["win"], max_level=s0["max_level"],
                min_eig_thr=s0["min_eig_thr"], max_iter=MAX_ITER, eps=EPS, second=dict(s1))


def tracker_np(pair, force=None, sets=None):
    sc = scene(pair)
    kw = {k: sc[k] for k in ("max_matches", "threshold", "non_max_supp", "block_half_length", "margin", "max_candidates", "n_feat_min",
                             "n_tiles_h", "n_tiles_w", "max_feat_per_tile", "threshold_px", "n_hyp", "kernel_size", "eps_gap", "eps_base",
                             "n_hyp_photo", "threshold_photo")}
    d = sc["describe"]
    return TwoSetTrackerNp(W, H, kc.K_CHAIN, 0.0, describe=None if d is None else dict(d, pattern=tc.pattern()),
                           sets=sets or PAIRS[pair], force=force, **kw)


def run_np(pair, pairs=None, force=None, sequences=1):
    """The scene's sequence through TwoSetTrackerNp, `sequences` times with reset() and photo_reset() between -> per sequence, per
    frame: the frame's dict with `features`, `ring` and `used` (the set of each of its feature trackings).  pairs: per sequence, per
    frame, the ring pair to take as given."""
    t = tracker_np(pair, force)
    out = []
    for si in range(sequences):
        if si:
            t.photo_reset()
        t.reset()
        frames = []
        for i, img in enumerate(scene(pair)["sequences"][0]):
            t.used = []
            r = t.track(img, seed=pc.SEED + i, seed_photo=pc.SEED_PHOTO + i, ring_pair=None if pairs is None else pairs[si][i])
            r["features"] = {k: v.copy() for k, v in t.features.items()}
            r["ring"] = list(t.state["ring"])
            r["used"] = list(t.used)
            frames.append(r)
        out.append(frames)
    return out


@functools.lru_cache(maxsize=None)
def restated(pair, force=None):
    return run_np(pair, force=force)[0]
