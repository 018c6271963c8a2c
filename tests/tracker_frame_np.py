"""TrackerNp: the control flow of `Tracker::track` (src/x/vision/tracker.cpp:134-306, a build without PHOTOMETRIC_CALI, pyramid
level 0) composed from the restatements that already exist.  No arithmetic of its own:

    pyramid and tracking   klt_np.build_pyramid / track / post_filter
    overflow pass          fast_np.remove_overflow + TileGrid
    detection              fast_np.detect
    description            orb_np.describe
    outlier removal        fundamental_np.filter_matches

It is what xk_trk_frame is compared against (tests/test_gpu_tracker_frame.py).  `overflow_mask` is the overflow pass as the device
states it -- a pure function of the tile histogram -- and tests/test_tracker_frame_np.py holds it against the sequential loop."""
import numpy as np

import fast_np as fastnp
import fundamental_np as fnp
import klt_np as knp
import orb_np as onp

NEW_TILE = (-1, -1)      # a new Feature's tile (feature.h:161-166): what the current feature of a re-detected pair carries


class CapacityError(Exception):
    """What xk_trk_frame reports as XK_ECAPACITY; counts: those reached."""

    def __init__(self, what, counts):
        super().__init__(what)
        self.counts = counts


def overflow_mask(grid, cur_xy):
    """Tracker::removeOverflowFeatures as one mask: pair i stays iff it is the last one or its current tile holds at most
    max_feat_per_tile of the current features.  -> (bool [n], tiles of the current list)."""
    n = len(cur_xy)
    tiles = [grid.tile(*p) for p in cur_xy]
    grid.reset()
    for t in tiles:
        grid.increment(*t)
    return np.array([i == n - 1 or grid.count(*tiles[i]) <= grid.max_feat_per_tile for i in range(n)], bool), tiles


class TrackerNp:
    def __init__(self, width, height, K, s=0.0, max_matches=320, win=(21, 21), max_level=2, max_iter=30, eps=0.01, min_eig_thr=0.003,
                 threshold=9, non_max_supp=1, block_half_length=20, margin=20, max_candidates=8192,
                 describe=None, n_feat_min=40, n_tiles_h=1, n_tiles_w=1, max_feat_per_tile=10000, threshold_px=0.3, n_hyp=128):
        """describe: None, or dict(pattern, edge, centroid, angle_deg, max_desc)."""
        self.W, self.H, self.K, self.s, self.max_matches = width, height, K, s, max_matches
        self.klt = dict(win=win, max_iter=max_iter, eps=eps, min_eig_thr=min_eig_thr)
        self.max_level = max_level
        self.det = dict(threshold=threshold, non_max_supp=non_max_supp, block_half_length=block_half_length, margin=margin)
        self.max_candidates = max_candidates
        self.desc = describe
        self.n_feat_min = n_feat_min
        self.grid = fastnp.TileGrid(width, height, n_tiles_h, n_tiles_w, max_feat_per_tile)
        self.ransac = dict(threshold_px=threshold_px, n_hyp=n_hyp)
        self.reset()
        self.prev_img = self.prev_pyr = None

    def reset(self):
        """The next frame is a first frame; the images stay."""
        self.features = None                 # dict(dist_xy fp64 [n, 2], score int32 [n], desc uint8 [n, 32])

    def _detect(self, img, old_xy, counts):
        d = fastnp.detect(img, old_xy=old_xy, **self.det)
        counts["n_candidates"], counts["n_accepted"] = int(d["n_candidates"]), len(d["xy"])
        if d["n_candidates"] > self.max_candidates:
            counts["n_accepted"] = 0         # (reported, nothing selected)
            raise CapacityError("more candidates than max_candidates", counts)
        if len(d["xy"]) > self.max_matches:
            raise CapacityError("more features accepted than max_matches", counts)
        desc = np.zeros((len(d["xy"]), 32), np.uint8)
        if self.desc is not None:
            if len(d["xy"]) > self.desc["max_desc"]:
                raise CapacityError("more keypoints than max_desc", counts)
            o = onp.describe(img, d["xy"], self.desc["pattern"], self.desc["edge"], self.desc["centroid"], self.desc["angle_deg"])
            assert len(o["keep_idx"]) == len(d["xy"])        # margin >= edge: every detected feature is described
            desc = o["desc"]
        return d["xy"].astype(np.float64), d["score"].astype(np.int32), desc

    def _track(self, pyr_prev, pyr_cur, dist_xy):
        """featureTracking: the float cast of the distorted pixels (tracker.cpp:629-633) -> the tracking's dict."""
        r = knp.track(pyr_prev, pyr_cur, np.asarray(dist_xy, np.float64).reshape(-1, 2).astype(np.float32), **self.klt)
        self.margins.extend(r["margins"])
        return r

    def track(self, img, seed=0):
        """One image -> the frame's dict, as tracker.Klt.frame returns it, plus `ransac_margin` and `klt_margins`."""
        img = np.ascontiguousarray(np.asarray(img)[:, :self.W])
        pyr = knp.build_pyramid(img, self.klt["win"], self.max_level)
        counts = dict(n_tracked=0, n_left=0, redetected=0, n_candidates=0, n_accepted=0, n_new_tracked=0, n_matches=0, winner=-1)
        self.margins = []
        prev_img, prev_pyr, feats = self.prev_img, self.prev_pyr, self.features
        self.prev_img, self.prev_pyr, self.features = img, pyr, None      # (whatever fails below: the next frame is a first frame)
        empty = dict(prev_xy=np.zeros((0, 2)), cur_xy=np.zeros((0, 2)), prev_dist_xy=np.zeros((0, 2)), cur_dist_xy=np.zeros((0, 2)),
                     score=np.zeros(0, np.int32), origin=np.zeros(0, np.int32), tiles=np.zeros((0, 4), np.int32),
                     desc=np.zeros((0, 32), np.uint8), ransac_margin=np.inf, klt_margins=self.margins)
        if feats is None:
            xy, score, desc = self._detect(img, (), counts)
            self.features = dict(dist_xy=xy, score=score, desc=desc)
            return dict(counts, **empty)
        # featureTracking and its post-filter: score and descriptor follow their feature (:670-679)
        r = self._track(prev_pyr, pyr, feats["dist_xy"])
        keep = r["keep_idx"]
        prev, cur = feats["dist_xy"][keep], r["kept_cur"]
        score, desc, origin = feats["score"][keep], feats["desc"][keep], keep.astype(np.int32)
        counts["n_tracked"] = len(keep)
        # removeOverflowFeatures
        stay, tiles_prev, tiles_cur = fastnp.remove_overflow(self.grid, prev.tolist(), cur.tolist())
        stay = np.asarray(stay, np.int64)
        tiles = np.array([tiles_prev[i] + tiles_cur[i] for i in stay], np.int32).reshape(-1, 4)
        prev, cur, score, desc, origin = prev[stay], cur[stay], score[stay], desc[stay], origin[stay]
        counts["n_left"] = len(stay)
        if len(stay) < self.n_feat_min:                               # tracker.cpp:204-228
            counts["redetected"] = 1
            nxy, nscore, ndesc = self._detect(prev_img, prev, counts)
            r2 = self._track(prev_pyr, pyr, nxy)
            k2 = r2["keep_idx"]
            counts["n_new_tracked"] = len(k2)
            if len(stay) + len(k2) > self.max_matches:
                raise CapacityError("old plus new features exceed max_matches", counts)
            ntiles = np.array([self.grid.tile(*nxy[k]) + NEW_TILE for k in k2], np.int32).reshape(-1, 4)
            prev, cur = np.concatenate([prev, nxy[k2]]), np.concatenate([cur, r2["kept_cur"]])
            score, desc = np.concatenate([score, nscore[k2]]), np.concatenate([desc, ndesc[k2]])
            origin, tiles = np.concatenate([origin, -(k2.astype(np.int32) + 1)]), np.concatenate([tiles, ntiles])
        # undistortion and outlier removal (:233-293)
        f = fnp.filter_matches(prev, cur, self.K, self.s, seed=seed, **self.ransac)
        m = f["keep_idx"]
        counts["n_matches"], counts["winner"] = len(m), int(f["winner"])
        self.features = dict(dist_xy=cur[m], score=score[m], desc=desc[m])       # :299
        return dict(counts, prev_xy=f["prev_xy"], cur_xy=f["cur_xy"], prev_dist_xy=prev[m], cur_dist_xy=cur[m], score=score[m],
                    origin=origin[m], tiles=tiles[m], desc=desc[m], ransac_margin=f["margin"], klt_margins=self.margins,
                    n_total=len(prev))
