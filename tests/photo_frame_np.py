"""PhotoTrackerNp: the control flow of `Tracker::track` of a PHOTOMETRIC_CALI build (src/x/vision/tracker.cpp:134-306 with
calibrateImage at :186-190, pyramid level 0) composed from the restatements that already exist.  No arithmetic of its own:

    the frame               tracker_frame_np.TrackerNp's pieces (pyramid, tracking, overflow pass, detection, description, RANSAC)
    calibrateImage          photo_np.calibrate (tracking between the RAW images, intensities, gain RANSAC, ring, correction)
    computeIntensity        photo_np.intensity
    the spatial rows        photo_spatial_np.add

It is what xk_trk_photo_frame is compared against (tests/test_gpu_photo_frame.py).  Which plane each step reads:

    detection, description, featureTracking      the WORKING (corrected) planes
    intensity of a detected feature (:461)       the working plane it was detected on, at its integer pixel
    intensity of a tracked feature (:666)        the RAW current plane, at the truncated pixel
    calibrateImage's own tracking                the RAW planes

The device's refit sums run in a fixed order of their own, so its ring pair agrees with NumPy's only within
photo_cases.GAINS_RTOL; a float32 gain that differs in its last bit changes the corrected image and everything behind it.  `track`
therefore takes the frame's ring pair as given (ring_pair): the restated pair is returned for the comparison, the given one enters
the ring, as tests/test_gpu_photo.py corrects "with the DEVICE's pair".

`bookkeeping` is the list handling of a frame on indices alone -- which intensity travels with which pair through the post-filter,
the overflow pass, the concatenation and the RANSAC -- as the device states it with gathers; tests/test_photo_frame_np.py holds it
against a literal list walk of tracker.cpp:658-686 and :222-227."""
import numpy as np

import fast_np as fastnp
import fundamental_np as fnp
import klt_np as knp
import photo_np as pnp
import photo_spatial_np as snp
import tracker_frame_np as tnp

CapacityError = tnp.CapacityError


def bookkeeping(res_int, keep1, cur_int1, stay, new_int, keep2, cur_int2, kept3):
    """The intensities of a frame's matches as gathers.  res_int: the resident intensities; keep1: the resident positions the
    post-filter kept, cur_int1 the intensities of their current features (by kept position); stay: the kept positions the overflow
    pass left; new_int: the intensities of the re-detection's accepted features, keep2 the accepted positions the second post-filter
    kept, cur_int2 the intensities of their current features; kept3: the positions of the concatenated list the RANSAC kept.
    -> (previous intensities, current intensities) of the matches."""
    res_int, cur_int1, new_int, cur_int2 = (np.asarray(v, np.float64) for v in (res_int, cur_int1, new_int, cur_int2))
    keep1, stay, keep2, kept3 = (np.asarray(v, np.int64) for v in (keep1, stay, keep2, kept3))
    prev = np.concatenate([res_int[keep1][stay], new_int[keep2]])
    cur = np.concatenate([cur_int1[stay], cur_int2])
    return prev[kept3], cur[kept3]


class PhotoTrackerNp(tnp.TrackerNp):
    def __init__(self, *args, kernel_size=30, eps_gap=0.0, eps_base=0.0, n_hyp_photo=64, threshold_photo=-1, spatial=None, **kw):
        """spatial: None, or dict(div, max_count, max_rows) -- the rows a frame's calibration accumulates (no estimate here)."""
        super().__init__(*args, **kw)
        self.kernel_size, self.eps_gap, self.eps_base = kernel_size, eps_gap, eps_base
        self.n_hyp_photo, self.threshold_photo = n_hyp_photo, threshold_photo
        self.spatial = spatial
        self.prev_raw = None
        self.photo_reset()

    def photo_reset(self):
        self.state = dict(ring=[(1.0, 0.0)], done=False)
        if self.spatial is not None:
            self.grid_sp = snp.grid(self.W, self.H, self.spatial["div"])
            self.sp_state = snp.new_state(self.grid_sp)

    def _detect(self, img, old_xy, counts):
        """featureDetection with the threshold in force (tracker.cpp:848) and the accepted features' intensities on `img` (:461)."""
        base = self.det["threshold"]
        if self.state["done"] and self.threshold_photo >= 0:
            self.det["threshold"] = self.threshold_photo
        try:
            xy, score, desc = super()._detect(img, old_xy, counts)
        finally:
            self.det["threshold"] = base
        value, _, _ = pnp.intensity(img, xy.astype(np.int64), self.kernel_size)
        return xy, score, desc, value

    def _cur_intensity(self, raw, kept_cur):
        self.truncated.append(np.asarray(kept_cur, np.float64).ravel())
        return pnp.intensity(raw, np.trunc(kept_cur).astype(np.int64), self.kernel_size)[0]       # static_cast<int>, tracker.cpp:666

    def track(self, img, seed=0, seed_photo=0, ring_pair=None):
        """One image -> TrackerNp.track's dict, plus prev_intensity, cur_intensity, the calibration's outcome (n_cal_kept, estimated,
        done, support, a_rel, b_rel, frame_ab), `raw` and `working` (the two planes of the current image after the frame) and
        `restated_pair` (the ring's last pair as restated, before ring_pair replaced it), `cal_margins` and `cal_ransac` (of the
        calibration's tracking and gain RANSAC) and `truncated` (every coordinate the frame truncated to a pixel)."""
        raw = np.ascontiguousarray(np.asarray(img)[:, :self.W])
        counts = dict(n_tracked=0, n_left=0, redetected=0, n_candidates=0, n_accepted=0, n_new_tracked=0, n_matches=0, winner=-1)
        self.margins, self.truncated = [], []
        prev_raw, prev_img, prev_pyr, feats = self.prev_raw, self.prev_img, self.prev_pyr, self.features
        self.prev_raw, self.features = raw, None                      # (whatever fails below: the next frame is a first frame)
        cal = dict(n_cal_kept=0, estimated=False, done=self.state["done"], support=0, a_rel=1.0, b_rel=0.0, frame_ab=np.zeros(4),
                   restated_pair=self.state["ring"][-1], cal_margins=[], cal_ransac=None, truncated=self.truncated)
        empty = dict(prev_xy=np.zeros((0, 2)), cur_xy=np.zeros((0, 2)), prev_dist_xy=np.zeros((0, 2)), cur_dist_xy=np.zeros((0, 2)),
                     score=np.zeros(0, np.int32), origin=np.zeros(0, np.int32), tiles=np.zeros((0, 4), np.int32),
                     desc=np.zeros((0, 32), np.uint8), prev_intensity=np.zeros(0), cur_intensity=np.zeros(0), ransac_margin=np.inf,
                     klt_margins=self.margins)
        if feats is None:                                             # tracker.cpp:160-168: no calibration on a first frame
            work = raw.copy()
            self.prev_img, self.prev_pyr = work, knp.build_pyramid(work, self.klt["win"], self.max_level)
            xy, score, desc, value = self._detect(work, (), counts)
            self.features = dict(dist_xy=xy, score=score, desc=desc, intensity=value)
            return dict(counts, **empty, **cal, raw=raw, working=work)
        # calibrateImage (:186-190, :761-858) from the previous features and their intensities
        R = len(feats["dist_xy"])
        n_hyp = max(1, min(R, self.n_hyp_photo))
        c = pnp.calibrate(self.state, prev_raw, raw, feats["dist_xy"].astype(np.float32), feats["intensity"], n_hyp, seed_photo, self.kernel_size,
                          self.eps_gap, self.eps_base, dict(self.klt, max_level=self.max_level))
        cal.update(n_cal_kept=len(c["keep_idx"]), estimated=bool(c["estimated"]), done=self.state["done"], support=int(c["support"]),
                   a_rel=float(c["a_rel"]), b_rel=float(c["b_rel"]), frame_ab=np.asarray(c["frame_ab"], np.float64),
                   restated_pair=self.state["ring"][-1], cal_margins=[] if c["track"] is None else c["track"]["margins"],
                   cal_ransac=c["ransac"])
        if c["track"] is not None:
            self.truncated.append(np.asarray(c["track"]["kept_cur"], np.float64).ravel())
        work = c["image"]
        if c["estimated"] and ring_pair is not None:
            self.state["ring"][-1] = (float(ring_pair[0]), float(ring_pair[1]))
            work = pnp.correct(raw, *self.state["ring"][-1])
        if c["estimated"] and self.spatial is not None:
            keep = c["keep_idx"]
            lists = (np.trunc(feats["dist_xy"].astype(np.float32)[keep]).astype(np.int32), np.trunc(c["track"]["kept_cur"]).astype(np.int32),
                     feats["intensity"][keep], c["intensity"])
            snp.add(self.sp_state, self.grid_sp, self.state["ring"], [lists], [1], self.spatial["max_count"], self.spatial["max_rows"])
        pyr = knp.build_pyramid(work, self.klt["win"], self.max_level)
        self.prev_img, self.prev_pyr = work, pyr
        planes = dict(raw=raw, working=work)
        # featureTracking on the working planes and its post-filter; the kept current features' intensities on the raw plane (:666)
        r = self._track(prev_pyr, pyr, feats["dist_xy"])
        keep = r["keep_idx"]
        prev, cur = feats["dist_xy"][keep], r["kept_cur"]
        score, desc, origin = feats["score"][keep], feats["desc"][keep], keep.astype(np.int32)
        cur_int1 = self._cur_intensity(raw, cur)
        counts["n_tracked"] = len(keep)
        stay, tiles_prev, tiles_cur = fastnp.remove_overflow(self.grid, prev.tolist(), cur.tolist())
        stay = np.asarray(stay, np.int64)
        tiles = np.array([tiles_prev[i] + tiles_cur[i] for i in stay], np.int32).reshape(-1, 4)
        prev, cur, score, desc, origin = prev[stay], cur[stay], score[stay], desc[stay], origin[stay]
        counts["n_left"] = len(stay)
        new_int, k2, cur_int2 = np.zeros(0), np.zeros(0, np.int64), np.zeros(0)
        try:
            if len(stay) < self.n_feat_min:                           # tracker.cpp:204-228, on the previous working plane
                counts["redetected"] = 1
                nxy, nscore, ndesc, new_int = self._detect(prev_img, prev, counts)
                r2 = self._track(prev_pyr, pyr, nxy)
                k2 = r2["keep_idx"]
                counts["n_new_tracked"] = len(k2)
                if len(stay) + len(k2) > self.max_matches:
                    raise CapacityError("old plus new features exceed max_matches", counts)
                cur_int2 = self._cur_intensity(raw, r2["kept_cur"])
                ntiles = np.array([self.grid.tile(*nxy[k]) + tnp.NEW_TILE for k in k2], np.int32).reshape(-1, 4)
                prev, cur = np.concatenate([prev, nxy[k2]]), np.concatenate([cur, r2["kept_cur"]])
                score, desc = np.concatenate([score, nscore[k2]]), np.concatenate([desc, ndesc[k2]])
                origin, tiles = np.concatenate([origin, -(k2.astype(np.int32) + 1)]), np.concatenate([tiles, ntiles])
        except CapacityError as e:
            e.calibration, e.planes = cal, planes
            raise
        f = fnp.filter_matches(prev, cur, self.K, self.s, seed=seed, **self.ransac)
        m = f["keep_idx"]
        counts["n_matches"], counts["winner"] = len(m), int(f["winner"])
        ip, ic = bookkeeping(feats["intensity"], keep, cur_int1, stay, new_int, k2, cur_int2, m)
        self.features = dict(dist_xy=cur[m], score=score[m], desc=desc[m], intensity=ic)             # :299
        return dict(counts, prev_xy=f["prev_xy"], cur_xy=f["cur_xy"], prev_dist_xy=prev[m], cur_dist_xy=cur[m], score=score[m],
                    origin=origin[m], tiles=tiles[m], desc=desc[m], prev_intensity=ip, cur_intensity=ic, ransac_margin=f["margin"],
                    klt_margins=self.margins, n_total=len(prev), **cal, **planes)
