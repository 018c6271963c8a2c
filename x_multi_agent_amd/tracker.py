"""Outlier removal of the tracker's matches on the device -- ctypes binding of the xk_trk_* entry points
(include/xk.h).  Mirrors the undistortion and the fundamental-matrix filter (RANSAC, or LMedS under `outlier_method(4)`) of `Tracker::track`
(src/x/vision/tracker.cpp:233-293, camera.cpp:62-87): what every frame's match list passes through before the track
manager sees it.

`Klt` is the step in front of it: the pyramidal Lucas-Kanade tracking of `Tracker::featureTracking` (tracker.cpp:623-690),
from two images and the previous features to the pairs that filter takes.  `Klt.detect` produces those features:
`Tracker::featureDetection` (tracker.cpp:390-590), FAST and the neighbourhood selection on a pushed image, and
`Klt.describe` their rotated-BRIEF descriptors (`PlaceRecognition::compute`, place_recognition.cpp:72-94), which is what
place.Database takes.  `Klt.photo_*` is the photometric calibration a PHOTOMETRIC_CALI build runs in front of all of them
(`Tracker::calibrateImage`, tracker.cpp:761-877, and IRPhotoCalib): photo_calibrate between push_image and track.
`Klt.frame` is `Tracker::track` itself (tracker.cpp:134-306, without the photometric step): one call per image on a feature list
that stays on the device (csrc/xk_frame.hip.h); `Klt.photo_frame` is the same call of a PHOTOMETRIC_CALI build, with the
calibration between the push and the tracking and the features' intensities resident beside them.

`MatchFilter.baseline` is what the track manager behind them asks every frame (`TrackManager::checkBaseline`,
track_manager.cpp:576-636, and `Camera::normalize`): the normalisation, crop and baseline check of all candidate tracks at once.

`Klt.tracks_*` is `TrackManager::manageTracks` itself (track_manager.cpp:115-436) on tracks that stay on the device: `tracks_manage` takes
a match list from the host, `tracks_manage_frame` the block the last `frame` / `photo_frame` left there (csrc/xk_track_store.hip.h).

No fallback: everything numeric runs in libxk.so's HIP kernels (csrc/xk_fundamental.hip.h, csrc/xk_klt.hip.h, csrc/xk_fast.hip.h,
csrc/xk_orb.hip.h, csrc/xk_photo.hip.h, csrc/xk_tracks.hip.h, csrc/xk_track_store.hip.h)."""
import ctypes as C

import numpy as np

from .engine import XkError, c_dp, c_ip

c_ub = C.POINTER(C.c_ubyte)
c_fp = C.POINTER(C.c_float)
c_sp = C.POINTER(C.c_short)
c_sb = C.POINTER(C.c_byte)
c_lp = C.POINTER(C.c_longlong)
CAM_FOV, CAM_RADTAN, CAM_EQUIDISTANT = 0, 1, 2      # XK_CAM_*: MatchFilter(model=...), MatchFilter.camera_model


class _Trk:
    """What MatchFilter and Klt share: an xk_trk (its own, or its owner's), the status check and the release."""
    owner = None

    def _create(self, eng, max_matches, K=(1.0, 1.0, 0.0, 0.0), s=0.0):
        self.eng, self.L, self.p = eng, eng.L, C.c_void_p()
        self._chk(self.L.xk_trk_create(eng.h, C.c_int(max_matches), *(C.c_double(v) for v in K), C.c_double(s), C.byref(self.p)), "xk_trk_create")

    def _error(self, rc, what):
        return XkError(rc, what, (self.L.xk_last_error(self.eng.h) or b"").decode())

    def _chk(self, rc, what):
        if rc != 0:
            raise self._error(rc, what)

    def outlier_method(self, method):
        """Tracker's outlier_method_ (tracker.h:256): 8 = cv::RANSAC (the default), 4 = cv::LMEDS.  Sticky on the xk_trk: filter_matches,
        Klt.frame and Klt.photo_frame follow it from the next call on."""
        self._chk(self.L.xk_trk_outlier_method(self.p, C.c_int(method)), "xk_trk_outlier_method")

    def close(self):
        if self.owner is None and self.p:
            self.L.xk_trk_destroy(self.p)
        self.p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MatchFilter(_Trk):
    """The camera model and the RANSAC of x::Tracker on one agent's GPU.  K = (fx, fy, cx, cy) in pixels or a 3 x 3 camera
    matrix, s = the FOV distortion parameter (0: none)."""

    def __init__(self, eng, max_matches, K, s=0.0, model=None, coeffs=None):
        K = np.asarray(K, np.float64)
        self.K = tuple(float(v) for v in ((K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.shape == (3, 3) else K.ravel()))
        self.s = float(s)
        self.max_matches = int(max_matches)
        self._create(eng, self.max_matches, self.K, self.s)
        if model is not None:
            try:
                self.camera_model(model, coeffs)
            except Exception:
                self.close()
                raise

    def camera_model(self, model, coeffs):
        """xk_trk_camera_model: CAM_FOV (s), CAM_RADTAN (k1 k2 p1 p2 [k3]) or CAM_EQUIDISTANT (k1 ... k4), DESIGN 3.10.2.  Sticky:
        undistort, distort, filter_matches, Klt.frame and Klt.photo_frame follow it from the next call on."""
        k = np.ascontiguousarray(() if coeffs is None else coeffs, np.float64).ravel()
        self._chk(self.L.xk_trk_camera_model(self.p, C.c_int(model), k.ctypes.data_as(c_dp) if len(k) else None, C.c_int(len(k))),
                  "xk_trk_camera_model")

    def undistort(self, dist_xy):
        """Camera::undistort (camera.cpp:62-87): distorted pixels [n, 2] -> undistorted pixels [n, 2], fp64."""
        d = np.ascontiguousarray(dist_xy, np.float64).reshape(-1, 2)
        out = np.zeros((max(len(d), 1), 2))
        self._chk(self.L.xk_trk_undistort(self.p, d.ctypes.data_as(c_dp), C.c_int(len(d)), out.ctypes.data_as(c_dp)), "xk_trk_undistort")
        return out[:len(d)]

    def distort(self, xy):
        """The forward map of the camera model: undistorted pixels [n, 2] -> distorted pixels [n, 2], fp64."""
        u = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
        out = np.zeros((max(len(u), 1), 2))
        self._chk(self.L.xk_trk_distort(self.p, u.ctypes.data_as(c_dp), C.c_int(len(u)), out.ctypes.data_as(c_dp)), "xk_trk_distort")
        return out[:len(u)]

    def undistort_status(self):
        """-> (invalid points, most Newton steps) of the last undistortion: undistort, filter_matches or a frame.  (0, 0) under the FOV model."""
        bad, steps = C.c_int(0), C.c_int(0)
        self._chk(self.L.xk_trk_undistort_status(self.p, C.byref(bad), C.byref(steps)), "xk_trk_undistort_status")
        return bad.value, steps.value

    def fundamental_ransac(self, prev_xy, cur_xy, threshold_px=0.3, n_hyp=1024, seed=0):
        """cv::findFundamentalMat(pts1, pts2, RANSAC, threshold_px, 0.99, mask) (tracker.cpp:243-260) on undistorted
        pixels [n, 2] (cast to float32 as the reference does) -> (mask uint8 [n], F [3, 3] in pixel coordinates with
        cur^T F prev = 0, n_inliers).  All n_hyp hypotheses are evaluated."""
        prev = np.ascontiguousarray(prev_xy, np.float32).reshape(-1, 2)
        cur = np.ascontiguousarray(cur_xy, np.float32).reshape(-1, 2)
        if len(prev) != len(cur):
            raise ValueError("prev_xy and cur_xy differ in length")
        n = len(prev)
        mask, F, ninl = np.zeros(max(n, 1), np.uint8), np.zeros(9), C.c_int(0)
        self._chk(self.L.xk_trk_fundamental_ransac(self.p, prev.ctypes.data_as(c_fp), cur.ctypes.data_as(c_fp), C.c_int(n),
                                                   C.c_double(threshold_px), C.c_int(n_hyp), C.c_ulong(seed), mask.ctypes.data_as(c_ub),
                                                   F.ctypes.data_as(c_dp), C.byref(ninl)), "xk_trk_fundamental_ransac")
        return mask[:n], F.reshape(3, 3), ninl.value

    def fundamental_hypotheses(self, first, count):
        """What the last RANSAC left for hypotheses first ... first+count-1 -> (n_cand [count], F [count, 3, 3, 3] in pixel
        coordinates and of unit Frobenius norm, inliers [count, 3])."""
        nc = np.zeros(max(count, 1), np.int32)
        F = np.zeros((max(count, 1), 3, 3, 3))
        inl = np.zeros((max(count, 1), 3), np.int32)
        self._chk(self.L.xk_trk_fundamental_hypotheses(self.p, C.c_int(first), C.c_int(count), nc.ctypes.data_as(c_ip), F.ctypes.data_as(c_dp),
                                                       inl.ctypes.data_as(c_ip)), "xk_trk_fundamental_hypotheses")
        return nc[:count], F[:count], inl[:count]

    def fundamental_lmeds(self, prev_xy, cur_xy, n_hyp=1024, seed=0):
        """cv::findFundamentalMat(pts1, pts2, LMEDS, ., 0.99, mask) on undistorted pixels [n, 2] (cast to float32) -> (mask uint8 [n],
        F [3, 3], n_inliers, median, sigma): the winner has the smallest median of the pairs' errors, an inlier has error <= sigma^2 with
        sigma = 2.5 * 1.4826 * (1 + 5 / (n - 7)) * sqrt(median), at least 0.001.  All n_hyp hypotheses are evaluated."""
        prev = np.ascontiguousarray(prev_xy, np.float32).reshape(-1, 2)
        cur = np.ascontiguousarray(cur_xy, np.float32).reshape(-1, 2)
        if len(prev) != len(cur):
            raise ValueError("prev_xy and cur_xy differ in length")
        n = len(prev)
        mask, F, ninl, med, sig = np.zeros(max(n, 1), np.uint8), np.zeros(9), C.c_int(0), C.c_double(0.0), C.c_double(0.0)
        self._chk(self.L.xk_trk_fundamental_lmeds(self.p, prev.ctypes.data_as(c_fp), cur.ctypes.data_as(c_fp), C.c_int(n), C.c_int(n_hyp),
                                                  C.c_ulong(seed), mask.ctypes.data_as(c_ub), F.ctypes.data_as(c_dp), C.byref(ninl),
                                                  C.byref(med), C.byref(sig)), "xk_trk_fundamental_lmeds")
        return mask[:n], F.reshape(3, 3), ninl.value, med.value, sig.value

    def fundamental_medians(self, first, count):
        """What the last call left if it ran LMedS -> (median [count, 3] of hypotheses first ... first+count-1, +inf where there is no
        candidate, and (median, sigma) of its winner)."""
        med, last = np.zeros((max(count, 1), 3)), np.zeros(2)
        self._chk(self.L.xk_trk_fundamental_medians(self.p, C.c_int(first), C.c_int(count), med.ctypes.data_as(c_dp), last.ctypes.data_as(c_dp)),
                  "xk_trk_fundamental_medians")
        return med[:count], (float(last[0]), float(last[1]))

    def fundamental_score(self, prev_xy, cur_xy, F, threshold_px=0.3):
        """The models F [m, 3, 3] (pixel coordinates, used as given) on the pairs [n, 2] -> (inliers int32 [m]: errors <= threshold_px^2,
        median fp64 [m]: 0.5 (e[(n-1)/2] + e[n/2]) of the ascending errors, +inf where that is not finite)."""
        prev = np.ascontiguousarray(prev_xy, np.float32).reshape(-1, 2)
        cur = np.ascontiguousarray(cur_xy, np.float32).reshape(-1, 2)
        if len(prev) != len(cur):
            raise ValueError("prev_xy and cur_xy differ in length")
        Fm = np.ascontiguousarray(F, np.float64).reshape(-1, 9)
        m = len(Fm)
        inl, med = np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1))
        self._chk(self.L.xk_trk_fundamental_score(self.p, prev.ctypes.data_as(c_fp), cur.ctypes.data_as(c_fp), C.c_int(len(prev)),
                                                  Fm.ctypes.data_as(c_dp), C.c_int(m), C.c_double(threshold_px), inl.ctypes.data_as(c_ip),
                                                  med.ctypes.data_as(c_dp)), "xk_trk_fundamental_score")
        return inl[:m], med[:m]

    def filter_matches(self, prev_dist_xy, cur_dist_xy, threshold_px=0.3, n_hyp=1024, seed=0):
        """tracker.cpp:233-293: distorted pixels [n, 2] of the tracked pairs -> (mask uint8 [n], keep_idx [m] ascending,
        prev_xy [m, 2], cur_xy [m, 2] undistorted fp64 pixels of the kept pairs in input order)."""
        prev = np.ascontiguousarray(prev_dist_xy, np.float64).reshape(-1, 2)
        cur = np.ascontiguousarray(cur_dist_xy, np.float64).reshape(-1, 2)
        if len(prev) != len(cur):
            raise ValueError("prev_dist_xy and cur_dist_xy differ in length")
        n = len(prev)
        mask, keep = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.int32)
        pxy, cxy, ninl = np.zeros((max(n, 1), 2)), np.zeros((max(n, 1), 2)), C.c_int(0)
        self._chk(self.L.xk_trk_filter_matches(self.p, prev.ctypes.data_as(c_dp), cur.ctypes.data_as(c_dp), C.c_int(n),
                                               C.c_double(threshold_px), C.c_int(n_hyp), C.c_ulong(seed), mask.ctypes.data_as(c_ub),
                                               keep.ctypes.data_as(c_ip), pxy.ctypes.data_as(c_dp), cxy.ctypes.data_as(c_dp),
                                               C.byref(ninl)), "xk_trk_filter_matches")
        m = ninl.value
        return mask[:n], keep[:m], pxy[:m], cxy[:m]

    def baseline_setup(self, max_tracks, max_obs):
        """xk_trk_baseline_setup: the capacities of one baseline() call."""
        self._chk(self.L.xk_trk_baseline_setup(self.p, C.c_int(max_tracks), C.c_int(max_obs)), "xk_trk_baseline_setup")

    def baseline(self, tracks, drop_last, C_q_G, min_baseline_x_n, min_baseline_y_n):
        """Camera::normalize(track, list size) and TrackManager::checkBaseline (track_manager.cpp:576-636) of a frame's
        candidate tracks: tracks = a list of fp64 [L_k, 2] arrays of undistorted pixels (oldest first), drop_last uint8 [K],
        C_q_G fp64 [n_quats, 4] (x, y, z, w) -> dict of norm_off int32 [K + 1], norm_xy fp64 [norm_off[K], 2], delta_xy fp64
        [K, 2], flag uint8 [K]."""
        trk = [np.ascontiguousarray(t, np.float64).reshape(-1, 2) for t in tracks]
        K = len(trk)
        off = np.zeros(K + 1, np.int32)
        off[1:] = np.cumsum([len(t) for t in trk])
        obs = np.concatenate(trk + [np.zeros((1, 2))])
        drop = np.ascontiguousarray(drop_last, np.uint8).ravel()
        if len(drop) != K:
            raise ValueError("baseline: one drop_last per track")
        q = np.ascontiguousarray(C_q_G, np.float64).reshape(-1, 4)
        norm_off, norm = np.zeros(K + 1, np.int32), np.zeros((len(obs), 2))
        delta, flag = np.zeros((max(K, 1), 2)), np.zeros(max(K, 1), np.uint8)
        self._chk(self.L.xk_trk_baseline(self.p, off.ctypes.data_as(c_ip), obs.ctypes.data_as(c_dp), drop.ctypes.data_as(c_ub), C.c_int(K),
                                         q.ctypes.data_as(c_dp), C.c_int(len(q)), C.c_double(min_baseline_x_n), C.c_double(min_baseline_y_n),
                                         norm_off.ctypes.data_as(c_ip), norm.ctypes.data_as(c_dp), delta.ctypes.data_as(c_dp),
                                         flag.ctypes.data_as(c_ub)), "xk_trk_baseline")
        return dict(norm_off=norm_off, norm_xy=norm[:norm_off[K]].copy(), delta_xy=delta[:K], flag=flag[:K])


class Klt(_Trk):
    """cv::calcOpticalFlowPyrLK as x::Tracker calls it (tracker.cpp:642-651, parameters tracker.h:234-261) and the post-filter
    behind it (:658-686) on one agent's GPU: push_image per frame, track per frame.  match_filter: an existing MatchFilter
    whose xk_trk this object shares, so that one device object serves both steps of a frame (max_features is then its
    max_matches); without one the object owns an xk_trk with placeholder intrinsics, which the tracking never reads.  second: None,
    or dict(win=(w, h), max_level=, min_eig_thr=) -- the second parameter set of a PHOTOMETRIC_CALI build (tracker.cpp:641-651), declared
    right after the KLT setup (klt_second); klt_select chooses between the two for track and frame, photo_frame chooses on the device."""

    def __init__(self, eng, max_features, width, height, win=(31, 31), max_level=2, max_iter=30, eps=0.01, min_eig_thr=0.003,
                 match_filter=None, second=None):
        self.owner = match_filter
        if match_filter is not None:
            self.eng, self.L, self.p, self.max_features = eng, eng.L, match_filter.p, match_filter.max_matches
        else:
            self.max_features = int(max_features)
            self._create(eng, self.max_features)
        try:
            self.setup(width, height, win, max_level, max_iter, eps, min_eig_thr)
            if second is not None:
                self.klt_second(**second)
        except XkError:
            self.close()
            raise

    def setup(self, width, height, win=(31, 31), max_level=2, max_iter=30, eps=0.01, min_eig_thr=0.003):
        """xk_trk_klt_setup: new sizes and parameters; the pushed images are forgotten."""
        self._chk(self.L.xk_trk_klt_setup(self.p, C.c_int(width), C.c_int(height), C.c_int(win[0]), C.c_int(win[1]), C.c_int(max_level),
                                          C.c_int(max_iter), C.c_double(eps), C.c_double(min_eig_thr)), "xk_trk_klt_setup")
        self.width, self.height, self.win = int(width), int(height), (int(win[0]), int(win[1]))

    def klt_second(self, win=(31, 31), max_level=2, min_eig_thr=0.003):
        """xk_trk_klt_second: the second parameter set (win_size_photo_, max_level_photo_, min_eig_thr_photo_), which photo_frame
        switches to on the device once its calibration is done.  A setup-class call: the pushed images are forgotten and every
        setup made after the KLT setup is dropped."""
        self._chk(self.L.xk_trk_klt_second(self.p, C.c_int(win[0]), C.c_int(win[1]), C.c_int(max_level), C.c_double(min_eig_thr)),
                  "xk_trk_klt_second")

    def klt_select(self, which):
        """xk_trk_klt_select: the set (0 or 1) that track and frame use from now on.  Sticky; photo_frame ignores it."""
        self._chk(self.L.xk_trk_klt_select(self.p, C.c_int(which)), "xk_trk_klt_select")

    @property
    def klt_selected(self):
        return int(self.L.xk_trk_klt_selected(self.p))

    def levels(self):
        """The highest pyramid level the first set uses (rule 1 of DESIGN 3.11)."""
        return int(self.L.xk_trk_klt_levels(self.p))

    def levels_of(self, which):
        """The highest pyramid level set `which` uses; -1 for a second set that was not declared."""
        return int(self.L.xk_trk_klt_levels_of(self.p, C.c_int(which)))

    def push_image(self, img):
        """The next frame, uint8 [height, >= width]; a row stride beyond the width (a view of a wider array) is passed on."""
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim != 2 or img.shape[0] != self.height or img.shape[1] < self.width:
            raise ValueError("push_image: a uint8 image of the set-up height and at least the set-up width")
        if img.strides[1] != 1:
            img = np.ascontiguousarray(img)
        self._chk(self.L.xk_trk_push_image(self.p, img.ctypes.data_as(c_ub), C.c_int(img.strides[0])), "xk_trk_push_image")

    def track(self, prev_xy):
        """Tracker::featureTracking: float32 pixels [n, 2] in the previous image -> dict of cur_xy fp64 [n, 2], status uint8
        [n], min_eig [n], keep_idx [m] ascending, kept_prev [m, 2], kept_cur [m, 2] (input order)."""
        prev = np.ascontiguousarray(prev_xy, np.float32).reshape(-1, 2)
        n, m = len(prev), max(len(prev), 1)
        cur, status, eig = np.zeros((m, 2)), np.zeros(m, np.uint8), np.zeros(m)
        keep, kp, kc, nk = np.zeros(m, np.int32), np.zeros((m, 2)), np.zeros((m, 2)), C.c_int(0)
        self._chk(self.L.xk_trk_track(self.p, prev.ctypes.data_as(c_fp), C.c_int(n), cur.ctypes.data_as(c_dp), status.ctypes.data_as(c_ub),
                                      eig.ctypes.data_as(c_dp), keep.ctypes.data_as(c_ip), kp.ctypes.data_as(c_dp), kc.ctypes.data_as(c_dp),
                                      C.byref(nk)), "xk_trk_track")
        k = nk.value
        return dict(cur_xy=cur[:n], status=status[:n], min_eig=eig[:n], keep_idx=keep[:k], kept_prev=kp[:k], kept_cur=kc[:k])

    def level(self, which, level):
        """Pyramid level `level` of the previous (which = 0) or current (1) image -> (image uint8, dIx int16, dIy int16)."""
        w, h = C.c_int(0), C.c_int(0)
        self._chk(self.L.xk_trk_klt_level(self.p, C.c_int(which), C.c_int(level), None, None, None, C.byref(w), C.byref(h)), "xk_trk_klt_level")
        img, dx, dy = np.zeros((h.value, w.value), np.uint8), np.zeros((h.value, w.value), np.int16), np.zeros((h.value, w.value), np.int16)
        self._chk(self.L.xk_trk_klt_level(self.p, C.c_int(which), C.c_int(level), img.ctypes.data_as(c_ub), dx.ctypes.data_as(c_sp),
                                          dy.ctypes.data_as(c_sp), None, None), "xk_trk_klt_level")
        return img, dx, dy

    def detect_setup(self, threshold=9, non_max_supp=True, block_half_length=20, margin=20, max_candidates=8192):
        """xk_trk_detect_setup: the parameters of Tracker::featureDetection (tracker.h:245-255) for the set-up image size.  A
        later setup() drops it."""
        self._chk(self.L.xk_trk_detect_setup(self.p, C.c_int(threshold), C.c_int(int(non_max_supp)), C.c_int(block_half_length),
                                             C.c_int(margin), C.c_int(max_candidates)), "xk_trk_detect_setup")
        self.max_candidates = int(max_candidates)

    def detect(self, which=1, old_xy=None):
        """Tracker::featureDetection (tracker.cpp:390-590) on the previous (which = 0) or current (1) image: FAST, the border,
        the order by score and the selection outside the neighbourhood of old_xy (fp64 pixels [n_old, 2]) and of one another
        -> dict of xy int32 [n, 2], score int32 [n] (ascending key), n_candidates."""
        old = np.zeros((0, 2)) if old_xy is None else np.ascontiguousarray(old_xy, np.float64).reshape(-1, 2)
        xy, score = np.zeros((self.max_features, 2), np.int32), np.zeros(self.max_features, np.int32)
        nf, nc = C.c_int(0), C.c_int(0)
        rc = self.L.xk_trk_detect(self.p, C.c_int(which), old.ctypes.data_as(c_dp) if len(old) else None, C.c_int(len(old)),
                                  xy.ctypes.data_as(c_ip), score.ctypes.data_as(c_ip), C.byref(nf), C.byref(nc))
        if rc != 0:
            err = self._error(rc, "xk_trk_detect")
            err.n_found, err.n_candidates = nf.value, nc.value
            raise err
        return dict(xy=xy[:nf.value].copy(), score=score[:nf.value].copy(), n_candidates=nc.value)

    def detect_stage(self):
        """What the last detect left -> (score image uint8 [height, width], the candidates' keys uint32, ascending)."""
        n = C.c_int(0)
        self._chk(self.L.xk_trk_detect_stage(self.p, None, None, C.byref(n)), "xk_trk_detect_stage")
        S, keys = np.zeros((self.height, self.width), np.uint8), np.zeros(max(self.max_candidates, 1), np.uint32)
        self._chk(self.L.xk_trk_detect_stage(self.p, S.ctypes.data_as(c_ub), keys.ctypes.data_as(C.POINTER(C.c_uint)), None),
                  "xk_trk_detect_stage")
        return S, keys[:min(n.value, self.max_candidates)].copy()

    def describe_setup(self, orientation=0, angle_deg=-1.0, edge=31, pattern=None, max_desc=8192):
        """xk_trk_describe_setup: orientation 0 = the fixed angle angle_deg (what cv::ORB::compute sees on cv::FAST keypoints:
        -1), 1 = the intensity centroid; edge = OpenCV's edgeThreshold; pattern int8 [256, 4] (x1 y1 x2 y2 within -15...15;
        OpenCV's is the first 256 rows of its bit_pattern_31_), None: the project's default.  A later setup()
        drops it."""
        pp = None
        if pattern is not None:
            pat = np.ascontiguousarray(pattern, np.int8)
            if pat.shape != (256, 4):
                raise ValueError("describe_setup: the pattern is int8 [256, 4]")
            pp = pat.ctypes.data_as(c_sb)
        self._chk(self.L.xk_trk_describe_setup(self.p, C.c_int(int(orientation)), C.c_double(angle_deg), C.c_int(edge), pp, C.c_int(max_desc)),
                  "xk_trk_describe_setup")

    def describe(self, xy, which=1):
        """cv::ORB::compute (place_recognition.cpp:83-88) of the keypoints xy (int32 pixels [n, 2]) on the previous (which = 0)
        or current (1) image -> dict of desc uint8 [m, 32], keep_idx int32 [m] (the keypoints at least `edge` inside the image,
        input order), dir int32 [m, 2] (16384 cos, 16384 sin), moments int32 [m, 2] (m10, m01; zeros with a fixed angle)."""
        pts = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
        n, m = len(pts), max(len(pts), 1)
        desc, keep, dirs, mom, nk = np.zeros((m, 32), np.uint8), np.zeros(m, np.int32), np.zeros((m, 2), np.int32), np.zeros((m, 2), np.int32), C.c_int(0)
        self._chk(self.L.xk_trk_describe(self.p, C.c_int(which), pts.ctypes.data_as(c_ip), C.c_int(n), desc.ctypes.data_as(c_ub),
                                         keep.ctypes.data_as(c_ip), dirs.ctypes.data_as(c_ip), mom.ctypes.data_as(c_ip), C.byref(nk)),
                  "xk_trk_describe")
        k = nk.value
        return dict(desc=desc[:k].copy(), keep_idx=keep[:k].copy(), dir=dirs[:k].copy(), moments=mom[:k].copy())

    def describe_stage(self, which=1):
        """-> (the blurred image uint8 [height, width] of the previous (which = 0) or current (1) image, the pattern in use
        int8 [256, 4])."""
        G, pat = np.zeros((self.height, self.width), np.uint8), np.zeros((256, 4), np.int8)
        self._chk(self.L.xk_trk_describe_stage(self.p, C.c_int(which), G.ctypes.data_as(c_ub), pat.ctypes.data_as(c_sb)), "xk_trk_describe_stage")
        return G, pat

    # ---- Tracker::track in one call (tracker.cpp:134-306) on a feature list that stays on the device, csrc/xk_frame.hip.h ----
    _frame_buf = None

    def frame_setup(self, n_feat_min=40, n_tiles_h=1, n_tiles_w=1, max_feat_per_tile=10000, threshold_px=0.3, n_hyp=1024):
        """xk_trk_frame_setup, after detect_setup (and describe_setup, if the features carry descriptors): n_feat_min of
        tracker.cpp:204, the tile grid and cap of removeOverflowFeatures, threshold and hypotheses of the outlier removal.  A
        later setup(), detect_setup() or describe_setup() drops it."""
        self._chk(self.L.xk_trk_frame_setup(self.p, C.c_int(n_feat_min), C.c_int(n_tiles_h), C.c_int(n_tiles_w), C.c_int(max_feat_per_tile),
                                            C.c_double(threshold_px), C.c_int(n_hyp)), "xk_trk_frame_setup")

    def _frame_arrays(self):
        """What xk_trk_frame_out points at: max_features rows each, allocated once."""
        m = self.max_features
        if self._frame_buf is None or len(self._frame_buf["score"]) != m:
            self._frame_buf = dict(prev_xy=np.zeros((m, 2)), cur_xy=np.zeros((m, 2)), prev_dist_xy=np.zeros((m, 2)), cur_dist_xy=np.zeros((m, 2)),
                                   score=np.zeros(m, np.int32), origin=np.zeros(m, np.int32), tiles=np.zeros((m, 4), np.int32),
                                   desc=np.zeros((m, 32), np.uint8))
        return self._frame_buf

    def _frame_call(self, entry, img, o, arrays, seeds, calibration=None):
        """What frame() and photo_frame() share: the image check, `arrays` wired into the struct o by field name, the call of `entry`
        with `seeds`, the counts, and on a failure the XkError with `counts` (and with `calibration`, a function of o, its result as
        `calibration`) -> the counts, the calibration's outcome and the first n_matches rows of every array."""
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim != 2 or img.shape[0] != self.height or img.shape[1] < self.width:
            raise ValueError(entry[len("xk_trk_"):] + ": a uint8 image of the set-up height and at least the set-up width")
        if img.strides[1] != 1:
            img = np.ascontiguousarray(img)
        types = dict(o._fields_)
        for name, v in arrays.items():
            setattr(o, name, v.ctypes.data_as(types[name]))
        rc = getattr(self.L, entry)(self.p, img.ctypes.data_as(c_ub), C.c_int(img.strides[0]), *(C.c_ulong(s) for s in seeds), C.byref(o))
        counts = {k: int(getattr(o, k)) for k in FrameOut.COUNTS}
        cal = calibration(o) if calibration else {}
        if rc != 0:
            err = self._error(rc, entry)
            err.counts = counts
            if calibration:
                err.calibration = cal
            raise err
        m = counts["n_matches"]
        out = dict(counts, **cal)
        out.update({k: v[:m].copy() for k, v in arrays.items()})
        return out

    def frame(self, img, seed=0):
        """xk_trk_frame, Tracker::track of one image (uint8 [height, >= width]) -> dict of the counts n_tracked, n_left, redetected,
        n_candidates, n_accepted, n_new_tracked, n_matches, winner, and per match prev_xy, cur_xy (undistorted fp64 pixels),
        prev_dist_xy, cur_dist_xy, score, origin, tiles int32 [m, 4] (previous row, column, current row, column), desc uint8
        [m, 32].  A first frame returns no matches.  On XK_ECAPACITY the XkError carries the counts reached as `counts`."""
        return self._frame_call("xk_trk_frame", img, FrameOut(), self._frame_arrays(), (seed,))

    def frame_features(self):
        """The resident list as the device holds it -> dict of dist_xy fp64 [n, 2], score int32 [n], desc uint8 [n, 32] (zeros
        without a description)."""
        m = self.max_features
        xy, score, desc, n = np.zeros((m, 2)), np.zeros(m, np.int32), np.zeros((m, 32), np.uint8), C.c_int(0)
        self._chk(self.L.xk_trk_frame_features(self.p, xy.ctypes.data_as(c_dp), score.ctypes.data_as(c_ip), desc.ctypes.data_as(c_ub),
                                               C.byref(n)), "xk_trk_frame_features")
        return dict(dist_xy=xy[:n.value].copy(), score=score[:n.value].copy(), desc=desc[:n.value].copy())

    def frame_reset(self):
        """The next frame is a first frame; the pushed images stay."""
        self._chk(self.L.xk_trk_frame_reset(self.p), "xk_trk_frame_reset")

    # ---- Tracker::track in one call, a PHOTOMETRIC_CALI build (calibrateImage at tracker.cpp:186-190) ----
    _photo_frame_buf = None

    def photo_frame_setup(self, n_hyp_photo=None, threshold_photo=-1):
        """xk_trk_photo_frame_setup, after frame_setup and photo_setup: the cap of a frame's gain RANSAC (None: max_hyp of the
        photo setup) and fast_detection_delta_photo_, the FAST threshold once a frame has estimated gains (< 0: no switch).  Whatever
        drops the frame setup drops it, and so does a later photo_setup()."""
        self._chk(self.L.xk_trk_photo_frame_setup(self.p, C.c_int(self.photo_max_hyp if n_hyp_photo is None else n_hyp_photo),
                                                  C.c_int(threshold_photo)), "xk_trk_photo_frame_setup")

    def photo_frame(self, img, seed=0, seed_photo=0):
        """xk_trk_photo_frame, Tracker::track of one image with the photometric calibration -> frame()'s dict, and prev_intensity,
        cur_intensity fp64 [m] (getIntensity of both features of each match), n_cal_kept, estimated (bool), done (bool), support,
        a_rel, b_rel, frame_ab fp64 [4] (the calibration's outcome, as photo_calibrate's).  On XK_ECAPACITY the XkError carries the
        counts reached as `counts` and the calibration's outcome as `calibration`."""
        m = self.max_features
        if self._photo_frame_buf is None or len(self._photo_frame_buf["prev_intensity"]) != m:
            self._photo_frame_buf = dict(prev_intensity=np.zeros(m), cur_intensity=np.zeros(m))

        def calibration(o):
            return dict(n_cal_kept=int(o.n_cal_kept), estimated=bool(o.estimated), done=bool(o.done), support=int(o.support),
                        a_rel=float(o.a_rel), b_rel=float(o.b_rel), frame_ab=np.array(o.frame_ab[:], np.float64))
        return self._frame_call("xk_trk_photo_frame", img, PhotoFrameOut(), dict(self._frame_arrays(), **self._photo_frame_buf),
                                (seed, seed_photo), calibration)

    def photo_frame_intensities(self):
        """The resident intensities beside frame_features() -> fp64 [n]."""
        v, n = np.zeros(self.max_features), C.c_int(0)
        self._chk(self.L.xk_trk_photo_frame_intensities(self.p, v.ctypes.data_as(c_dp), C.byref(n)), "xk_trk_photo_frame_intensities")
        return v[:n.value].copy()

    # ---- photometric calibration (Tracker::calibrateImage, tracker.cpp:761-877; irPhotoCalib.cpp), csrc/xk_photo.hip.h ----
    def photo_setup(self, kernel_size=30, epsilon_gap=0.0, epsilon_base=0.0, max_hyp=512):
        """xk_trk_photo_setup: the raw plane of both image slots, the spatial map (zeros), the parameter ring (one entry (1, 0))
        and the scratch of a gain estimate of up to max_hyp hypotheses.  A later setup() drops it."""
        self._chk(self.L.xk_trk_photo_setup(self.p, C.c_int(kernel_size), C.c_double(epsilon_gap), C.c_double(epsilon_base), C.c_int(max_hyp)),
                  "xk_trk_photo_setup")
        self.photo_max_hyp = int(max_hyp)

    def photo_intensity(self, xy, which=1, plane=1):
        """Tracker::computeIntensity (tracker.cpp:860-877) at the pixels xy (int32 [n, 2]) of the previous (which = 0) or current
        (1) image, its raw (plane = 0) or working (1) plane -> (value fp64 [n], sum int32 [n], count int32 [n])."""
        pts = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
        n, m = len(pts), max(len(pts), 1)
        value, s, c = np.zeros(m), np.zeros(m, np.int32), np.zeros(m, np.int32)
        self._chk(self.L.xk_trk_photo_intensity(self.p, C.c_int(which), C.c_int(plane), pts.ctypes.data_as(c_ip), C.c_int(n),
                                                value.ctypes.data_as(c_dp), s.ctypes.data_as(c_ip), c.ctypes.data_as(c_ip)),
                  "xk_trk_photo_intensity")
        return value[:n], s[:n], c[:n]

    def photo_gains(self, o_hist, o_cur, frame_back=(1,), n_hyp=None, seed=0):
        """IRPhotoCalib::ProcessCurrentFrame (irPhotoCalib.cpp:95-160, :212-218): o_hist, o_cur are lists of G arrays (or one
        array: one group), frame_back one int per group; n_hyp None: min(the largest group, max_hyp), at least 1 -> dict of
        a_rel, b_rel fp64 [G], support int32 [G], frame_ab fp64 [4]."""
        if not isinstance(o_hist, (list, tuple)):
            o_hist, o_cur = [o_hist], [o_cur]
        oh = [np.ascontiguousarray(v, np.float64).ravel() for v in o_hist]
        oc = [np.ascontiguousarray(v, np.float64).ravel() for v in o_cur]
        if len(oh) != len(oc) or len(oh) != len(frame_back) or any(len(a) != len(b) for a, b in zip(oh, oc)):
            raise ValueError("photo_gains: o_hist, o_cur and frame_back differ in length")
        G = len(oh)
        off = np.zeros(G + 1, np.int32)
        off[1:] = np.cumsum([len(v) for v in oh])
        H = np.concatenate(oh + [np.zeros(1)])
        Cu = np.concatenate(oc + [np.zeros(1)])
        fb = np.ascontiguousarray(frame_back, np.int32)
        if n_hyp is None:
            n_hyp = max(1, min(max(len(v) for v in oh), self.photo_max_hyp))
        a, b, sup, fab = np.zeros(max(G, 1)), np.zeros(max(G, 1)), np.zeros(max(G, 1), np.int32), np.zeros(4)
        self._chk(self.L.xk_trk_photo_gains(self.p, C.c_int(G), off.ctypes.data_as(c_ip), H.ctypes.data_as(c_dp), Cu.ctypes.data_as(c_dp),
                                            fb.ctypes.data_as(c_ip), C.c_int(n_hyp), C.c_ulong(seed), a.ctypes.data_as(c_dp),
                                            b.ctypes.data_as(c_dp), sup.ctypes.data_as(c_ip), fab.ctypes.data_as(c_dp)), "xk_trk_photo_gains")
        return dict(a_rel=a[:G], b_rel=b[:G], support=sup[:G], frame_ab=fab)

    def photo_hypotheses(self, g, first, count):
        """What the last gain estimate left for hypotheses first ... first+count-1 of group g -> (ab fp64 [count, 2], inliers
        int32 [count])."""
        ab, inl = np.zeros((max(count, 1), 2)), np.zeros(max(count, 1), np.int32)
        self._chk(self.L.xk_trk_photo_hypotheses(self.p, C.c_int(g), C.c_int(first), C.c_int(count), ab.ctypes.data_as(c_dp),
                                                 inl.ctypes.data_as(c_ip)), "xk_trk_photo_hypotheses")
        return ab[:count], inl[:count]

    def photo_params(self):
        """The parameter ring, oldest first -> fp64 [count, 2] of (a, b)."""
        a, b, n = np.zeros(15), np.zeros(15), C.c_int(0)
        self._chk(self.L.xk_trk_photo_params(self.p, a.ctypes.data_as(c_dp), b.ctypes.data_as(c_dp), C.byref(n)), "xk_trk_photo_params")
        return np.stack([a[:n.value], b[:n.value]], axis=1)

    def photo_reset(self):
        """The ring back to (1, 0)."""
        self._chk(self.L.xk_trk_photo_reset(self.p), "xk_trk_photo_reset")

    def photo_set_spatial(self, ps=None):
        """The spatial map params_PS_: float32 [height, width], None: zeros."""
        pp = None
        if ps is not None:
            ps = np.ascontiguousarray(ps, np.float32)
            if ps.shape != (self.height, self.width):
                raise ValueError("photo_set_spatial: the map is float32 [height, width]")
            pp = ps.ctypes.data_as(c_fp)
        self._chk(self.L.xk_trk_photo_set_spatial(self.p, pp), "xk_trk_photo_set_spatial")

    def photo_correct(self, which=1):
        """IRPhotoCalib::getCorrectedImage of the previous (which = 0) or current (1) image with the ring's last pair."""
        self._chk(self.L.xk_trk_photo_correct(self.p, C.c_int(which)), "xk_trk_photo_correct")

    def photo_raw(self, which=1):
        """Level 0 of the raw plane -> uint8 [height, width], the image as pushed."""
        img = np.zeros((self.height, self.width), np.uint8)
        self._chk(self.L.xk_trk_photo_raw(self.p, C.c_int(which), img.ctypes.data_as(c_ub)), "xk_trk_photo_raw")
        return img

    def photo_calibrate(self, prev_xy, prev_intensity, n_hyp=None, seed=0):
        """Tracker::calibrateImage (tracker.cpp:761-858), between push_image and track: float32 pixels [n, 2] of the previous
        features and their intensities fp64 [n] -> dict of keep_idx int32 [m], intensity fp64 [m], sum, count int32 [m] (the
        kept features in the raw current image), a_rel, b_rel, support, frame_ab fp64 [4], estimated (bool).  n_hyp None:
        min(n, max_hyp), at least 1."""
        prev = np.ascontiguousarray(prev_xy, np.float32).reshape(-1, 2)
        pin = np.ascontiguousarray(prev_intensity, np.float64).ravel()
        if len(prev) != len(pin):
            raise ValueError("photo_calibrate: prev_xy and prev_intensity differ in length")
        n, m = len(prev), max(len(prev), 1)
        if n_hyp is None:
            n_hyp = max(1, min(n, self.photo_max_hyp))
        keep, val, s, c = np.zeros(m, np.int32), np.zeros(m), np.zeros(m, np.int32), np.zeros(m, np.int32)
        nk, a, b, sup, est, fab = C.c_int(0), C.c_double(0), C.c_double(0), C.c_int(0), C.c_int(0), np.zeros(4)
        self._chk(self.L.xk_trk_photo_calibrate(self.p, prev.ctypes.data_as(c_fp), pin.ctypes.data_as(c_dp), C.c_int(n), C.c_int(n_hyp),
                                                C.c_ulong(seed), keep.ctypes.data_as(c_ip), val.ctypes.data_as(c_dp), s.ctypes.data_as(c_ip),
                                                c.ctypes.data_as(c_ip), C.byref(nk), C.byref(a), C.byref(b), C.byref(sup),
                                                fab.ctypes.data_as(c_dp), C.byref(est)), "xk_trk_photo_calibrate")
        k = nk.value
        return dict(keep_idx=keep[:k].copy(), intensity=val[:k].copy(), sum=s[:k].copy(), count=c[:k].copy(), a_rel=a.value, b_rel=b.value,
                    support=sup.value, frame_ab=fab, estimated=bool(est.value))

    # ---- the spatial photometric map (irPhotoCalib.cpp:162-210, :314-420), csrc/xk_photo_spatial.hip.h ----
    SPATIAL_STATES = ("accumulating", "estimated", "failed-and-accumulating")
    spatial_n = 0                    # unknowns of the last estimate: what photo_spatial_stage sizes its arrays by

    def photo_spatial_setup(self, div=16, coverage_thr=0.9, max_count=500, max_rows=65536, gp_length=5.0, gp_sigma_f=0.01, gp_sigma_n=0.01):
        """xk_trk_photo_spatial_setup, after photo_setup: the grid of div x div cells, the coverage threshold, the per-cell cap
        (SP_max_correscount_), the row list's capacity and the GP's hyperparameters.  A later setup() or photo_setup() drops it."""
        self._chk(self.L.xk_trk_photo_spatial_setup(self.p, C.c_int(div), C.c_double(coverage_thr), C.c_int(max_count), C.c_int(max_rows),
                                                    C.c_double(gp_length), C.c_double(gp_sigma_f), C.c_double(gp_sigma_n)),
                  "xk_trk_photo_spatial_setup")
        self.spatial_grid = (self.width // div, self.height // div)

    def photo_spatial_add(self, pix_hist, pix_cur, o_hist, o_cur, frame_back=(1,)):
        """One ProcessCurrentFrame worth of rows (irPhotoCalib.cpp:162-198), after photo_gains: lists of G arrays (or one array each:
        one group) of int32 pixels [n, 2] and fp64 intensities [n], frame_back one int per group."""
        if not isinstance(pix_hist, (list, tuple)):
            pix_hist, pix_cur, o_hist, o_cur = [pix_hist], [pix_cur], [o_hist], [o_cur]
        ph = [np.ascontiguousarray(v, np.int32).reshape(-1, 2) for v in pix_hist]
        pc = [np.ascontiguousarray(v, np.int32).reshape(-1, 2) for v in pix_cur]
        oh = [np.ascontiguousarray(v, np.float64).ravel() for v in o_hist]
        oc = [np.ascontiguousarray(v, np.float64).ravel() for v in o_cur]
        G = len(ph)
        if not (len(pc) == len(oh) == len(oc) == len(frame_back) == G) or any(not (len(a) == len(b) == len(c) == len(d))
                                                                               for a, b, c, d in zip(ph, pc, oh, oc)):
            raise ValueError("photo_spatial_add: the lists differ in length")
        off = np.zeros(G + 1, np.int32)
        off[1:] = np.cumsum([len(v) for v in ph])
        PH, PC = np.concatenate(ph + [np.zeros((1, 2), np.int32)]), np.concatenate(pc + [np.zeros((1, 2), np.int32)])
        OH, OC = np.concatenate(oh + [np.zeros(1)]), np.concatenate(oc + [np.zeros(1)])
        fb = np.ascontiguousarray(frame_back, np.int32)
        self._chk(self.L.xk_trk_photo_spatial_add(self.p, C.c_int(G), off.ctypes.data_as(c_ip), PH.ctypes.data_as(c_ip), PC.ctypes.data_as(c_ip),
                                                  OH.ctypes.data_as(c_dp), OC.ctypes.data_as(c_dp), fb.ctypes.data_as(c_ip)),
                  "xk_trk_photo_spatial_add")

    def photo_spatial_status(self):
        """-> dict of rows, covered, cells, ready (bool), dropped, state (one of SPATIAL_STATES)."""
        v = [C.c_int(0) for _ in range(6)]
        self._chk(self.L.xk_trk_photo_spatial_status(self.p, *[C.byref(x) for x in v]), "xk_trk_photo_spatial_status")
        return dict(rows=v[0].value, covered=v[1].value, cells=v[2].value, ready=bool(v[3].value), dropped=v[4].value,
                    state=self.SPATIAL_STATES[v[5].value])

    def photo_spatial_rows(self, first=0, count=None):
        """Rows first ... first+count-1 (count None: to the last one) -> dict of sid_hist, sid_cur int32 [count], b fp64 [count],
        counts int32 [cells], coverage uint8 [cells]."""
        if count is None:
            count = self.photo_spatial_status()["rows"] - first
        m, cells = max(count, 1), self.spatial_grid[0] * self.spatial_grid[1]
        sh, sc, b = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m)
        cnt, cov = np.zeros(cells, np.int32), np.zeros(cells, np.uint8)
        self._chk(self.L.xk_trk_photo_spatial_rows(self.p, C.c_int(first), C.c_int(count), sh.ctypes.data_as(c_ip), sc.ctypes.data_as(c_ip),
                                                   b.ctypes.data_as(c_dp), cnt.ctypes.data_as(c_ip), cov.ctypes.data_as(c_ub)),
                  "xk_trk_photo_spatial_rows")
        return dict(sid_hist=sh[:count], sid_cur=sc[:count], b=b[:count], counts=cnt, coverage=cov)

    def photo_spatial_estimate(self, install=True):
        """EstimateSpatialParameters (irPhotoCalib.cpp:314-420) on the accumulated rows -> dict of n, converged (bool), ls_iterations,
        gp_iterations, ls_residual, gp_residual.  install: a converged map goes into the PS plane and accumulation stops."""
        o = SpatialOutcome()
        self._chk(self.L.xk_trk_photo_spatial_estimate(self.p, C.c_int(int(bool(install))), C.byref(o)), "xk_trk_photo_spatial_estimate")
        self.spatial_n = o.n
        return dict(n=o.n, converged=bool(o.converged), ls_iterations=o.ls_iterations, gp_iterations=o.gp_iterations,
                    ls_residual=o.ls_residual, gp_residual=o.gp_residual)

    def photo_spatial_stage(self):
        """The last estimate's intermediates -> dict of var_of_cell int32 [cells], L fp64 [n, n], c, x, alpha fp64 [n], coarse float32
        [ch, cw], ps float32 [height, width]."""
        n, (cw, ch) = max(self.spatial_n, 1), self.spatial_grid
        voc, L = np.zeros(cw * ch, np.int32), np.zeros((n, n))
        c, x, al = np.zeros(n), np.zeros(n), np.zeros(n)
        coarse, ps = np.zeros((ch, cw), np.float32), np.zeros((self.height, self.width), np.float32)
        self._chk(self.L.xk_trk_photo_spatial_stage(self.p, voc.ctypes.data_as(c_ip), L.ctypes.data_as(c_dp), c.ctypes.data_as(c_dp),
                                                    x.ctypes.data_as(c_dp), al.ctypes.data_as(c_dp), coarse.ctypes.data_as(c_fp),
                                                    ps.ctypes.data_as(c_fp)), "xk_trk_photo_spatial_stage")
        return dict(var_of_cell=voc, L=L, c=c, x=x, alpha=al, coarse=coarse, ps=ps)

    def photo_spatial_reset(self):
        """Counts, coverage and rows back to empty, the state back to accumulating; the PS plane keeps what it holds."""
        self._chk(self.L.xk_trk_photo_spatial_reset(self.p), "xk_trk_photo_spatial_reset")


    # ---- TrackManager::manageTracks on tracks that stay on the device (track_manager.cpp:115-436), csrc/xk_track_store.hip.h ----
    _tracks = None

    def tracks_setup(self, max_tracks, n_tiles_h=1, n_tiles_w=1, width=None, height=None, min_baseline_x_n=0.0, min_baseline_y_n=0.0,
                     multi_uav=False):
        """xk_trk_tracks_setup: the store of max_tracks tracks, empty, ids from 1.  The tile grid is TiledImage's of a width x height
        image (default: the set-up size); the intrinsics are the xk_trk's (match_filter=...)."""
        width, height = self.width if width is None else width, self.height if height is None else height
        self._chk(self.L.xk_trk_tracks_setup(self.p, C.c_int(max_tracks), C.c_int(n_tiles_h), C.c_int(n_tiles_w), C.c_int(width), C.c_int(height),
                                             C.c_double(min_baseline_x_n), C.c_double(min_baseline_y_n), C.c_int(1 if multi_uav else 0)),
                  "xk_trk_tracks_setup")
        self._tracks = dict(max_tracks=int(max_tracks), n=[0, 0, 0])

    def _tracks_call(self, entry, head, n, C_q_G, n_poses_max, n_slam_features_max, min_track_length, opp_ids):
        if self._tracks is None:
            raise self._error(1, entry + ": before tracks_setup")
        q = np.ascontiguousarray(C_q_G, np.float64).reshape(-1, 4)
        slam, new, opp = self._tracks["n"]
        per = slam + new
        cap_lost, cap_entries = max(per, 1), max(opp + n + per, 1)
        cap_obs = max((opp + n) * max(len(q), 1) + per * min(max(int(n_poses_max), 1), 64), 1)
        o = TracksOut()
        lost, claimed = np.zeros(cap_lost, np.int32), np.zeros(max(n, 1), np.uint8)
        ids, off, xy = np.zeros(cap_entries, np.int64), np.zeros(cap_entries + 1, np.int32), np.zeros((cap_obs, 2))
        o.cap_lost, o.cap_entries, o.cap_obs = cap_lost, cap_entries, cap_obs
        o.lost_slam_idxs, o.claimed = lost.ctypes.data_as(c_ip), claimed.ctypes.data_as(c_ub)
        o.ids, o.off, o.xy = ids.ctypes.data_as(c_lp), off.ctypes.data_as(c_ip), xy.ctypes.data_as(c_dp)
        id_list = None if opp_ids is None else np.ascontiguousarray(list(opp_ids) + [0], np.int64)
        n_ids = C.c_int(0 if opp_ids is None else len(opp_ids))
        rc = getattr(self.L, entry)(self.p, *head, q.ctypes.data_as(c_dp), C.c_int(len(q)), C.c_int(n_poses_max), C.c_int(n_slam_features_max),
                                    C.c_int(min_track_length), None if id_list is None else id_list.ctypes.data_as(c_lp),
                                    None if opp_ids is None else C.byref(n_ids), C.byref(o))
        if rc != 0:
            err = self._error(rc, entry)
            err.tracks_status = int(o.status)
            raise err
        if opp_ids is not None:
            del opp_ids[:]                                        # the caller's list is consumed (track_manager.cpp:355)
        self._tracks["n"] = [int(o.n_persistent), int(o.n_new_persistent), int(o.n_opportunistic)]
        return TracksResult(o, lost, claimed[:n], ids, off, xy)

    def tracks_manage(self, prev_xy, cur_xy, prev_dist_xy, cur_dist_xy, score, C_q_G, n_poses_max, n_slam_features_max, min_track_length,
                      opp_ids=None):
        """xk_trk_tracks_manage: manageTracks of a match list in the columns Klt.frame returns -> TracksResult.  opp_ids: a Python list
        (setOppUpgradesMSCKF), required with multi_uav; it is emptied on success.  On a refusal the XkError carries the device's `tracks_status` (XK_TRACKS_OUTSIDE_GRID, XK_TRACKS_CAPACITY; 0 otherwise)."""
        cols = [np.ascontiguousarray(v, np.float64).reshape(-1, 2) for v in (prev_xy, cur_xy, prev_dist_xy, cur_dist_xy)]
        sc = np.ascontiguousarray(score, np.int32).ravel()
        n = len(sc)
        if any(len(c) != n for c in cols):
            raise ValueError("tracks_manage: columns of one length")
        head = [c.ctypes.data_as(c_dp) for c in cols] + [sc.ctypes.data_as(c_ip), C.c_int(n)]
        return self._tracks_call("xk_trk_tracks_manage", head, n, C_q_G, n_poses_max, n_slam_features_max, min_track_length, opp_ids)

    def tracks_manage_frame(self, C_q_G, n_poses_max, n_slam_features_max, min_track_length, opp_ids=None, n_matches=None):
        """xk_trk_tracks_manage_frame: the same on the matches the last frame() / photo_frame() left on the device; only the attitudes
        and the ids go up.  n_matches: that frame's count, for the output capacities (default: max_features)."""
        n = self.max_features if n_matches is None else int(n_matches)
        return self._tracks_call("xk_trk_tracks_manage_frame", [], n, C_q_G, n_poses_max, n_slam_features_max, min_track_length, opp_ids)

    def tracks_lists(self, which):
        """xk_trk_tracks_lists: which = 0 persistent, 1 new persistent, 2 opportunistic -> dict of ids int64 [n], lengths int32 [n] (true
        lengths), obs fp64 [n, 64, 4] (undistorted x, y, distorted x, y; the newest min(length, 64) oldest first), score int32 [n, 64],
        tiles int32 [n, 64, 2]."""
        n = C.c_int(0)
        self._chk(self.L.xk_trk_tracks_lists(self.p, C.c_int(which), None, None, None, None, None, C.byref(n)), "xk_trk_tracks_lists")
        m = max(n.value, 1)
        ids, lengths, obs = np.zeros(m, np.int64), np.zeros(m, np.int32), np.zeros((m, 64, 4))
        score, tiles = np.zeros((m, 64), np.int32), np.zeros((m, 64, 2), np.int32)
        self._chk(self.L.xk_trk_tracks_lists(self.p, C.c_int(which), ids.ctypes.data_as(c_lp), lengths.ctypes.data_as(c_ip), obs.ctypes.data_as(c_dp),
                                             score.ctypes.data_as(c_ip), tiles.ctypes.data_as(c_ip), C.byref(n)), "xk_trk_tracks_lists")
        k = n.value
        return dict(ids=ids[:k], lengths=lengths[:k], obs=obs[:k], score=score[:k], tiles=tiles[:k])

    def tracks_remove_persistent(self, idx):
        """TrackManager::removePersistentTracksAtIndex."""
        if idx < 0:
            raise self._error(1, "xk_trk_tracks_remove_persistent: a negative index")
        self._chk(self.L.xk_trk_tracks_remove_persistent(self.p, C.c_uint(idx)), "xk_trk_tracks_remove_persistent")
        self._tracks["n"][0] -= 1

    def tracks_remove_new_persistent(self, idxs):
        """TrackManager::removeNewPersistentTracksAtIndexes: indices in increasing order."""
        if any(i < 0 for i in idxs):
            raise self._error(1, "xk_trk_tracks_remove_new_persistent: a negative index")
        v = np.ascontiguousarray(list(idxs) + [0], np.uint32)
        self._chk(self.L.xk_trk_tracks_remove_new_persistent(self.p, v.ctypes.data_as(C.POINTER(C.c_uint)), C.c_int(len(idxs))),
                  "xk_trk_tracks_remove_new_persistent")
        self._tracks["n"][1] -= len(idxs)

    def tracks_clear(self):
        """TrackManager::clear: the lists empty, the id counter as it was."""
        self._chk(self.L.xk_trk_tracks_clear(self.p), "xk_trk_tracks_clear")
        self._tracks["n"] = [0, 0, 0]


class FrameOut(C.Structure):
    """xk_trk_frame_out (include/xk.h)"""
    COUNTS = ("n_tracked", "n_left", "redetected", "n_candidates", "n_accepted", "n_new_tracked", "n_matches", "winner")
    _fields_ = [(k, C.c_int) for k in COUNTS] + [(k, c_dp) for k in ("prev_xy", "cur_xy", "prev_dist_xy", "cur_dist_xy")] + \
               [(k, c_ip) for k in ("score", "origin", "tiles")] + [("desc", c_ub)]


class PhotoFrameOut(C.Structure):
    """xk_trk_photo_frame_out (include/xk.h)"""
    _fields_ = FrameOut._fields_ + [(k, c_dp) for k in ("prev_intensity", "cur_intensity")] + \
               [(k, C.c_int) for k in ("n_cal_kept", "estimated", "done", "support")] + \
               [("a_rel", C.c_double), ("b_rel", C.c_double), ("frame_ab", C.c_double * 4)]


class SpatialOutcome(C.Structure):
    """xk_photo_spatial_outcome (include/xk.h)"""
    _fields_ = [("n", C.c_int), ("converged", C.c_int), ("ls_iterations", C.c_int), ("gp_iterations", C.c_int),
                ("ls_residual", C.c_double), ("gp_residual", C.c_double)]


class TracksOut(C.Structure):
    """xk_trk_tracks_out (include/xk.h)"""
    COUNTS = ("status", "n_persistent", "n_new_persistent", "n_opportunistic", "n_lost", "n_claimed", "n_candidates", "n_candidate_obs")
    _fields_ = [(k, C.c_int) for k in COUNTS] + [("next_id", C.c_longlong), ("n_list", C.c_int * 5)] + \
               [(k, C.c_int) for k in ("cap_lost", "cap_entries", "cap_obs")] + \
               [("lost_slam_idxs", c_ip), ("claimed", c_ub), ("ids", c_lp), ("off", c_ip), ("xy", c_dp)]


class TracksResult:
    """What Klt.tracks_manage and tracks_manage_frame return, as NumPy arrays: the counts of xk_trk_tracks_out as attributes, next_id,
    lost_slam_idxs int32 [n_lost], claimed uint8 [n], and `lists`: per measurement list (XK_TRACKS_MSCKF, _MSCKF_SHORT, _NEW_SLAM_STD,
    _NEW_MSCKF_SLAM, _PERSISTENT) a dict of ids int64 [k], off int32 [k + 1] and xy fp64 [off[k], 2], the normalised coordinates."""
    NAMES = ("msckf", "msckf_short", "new_slam_std", "new_msckf_slam", "persistent")

    def __init__(self, o, lost, claimed, ids, off, xy):
        for k in TracksOut.COUNTS:
            setattr(self, k, int(getattr(o, k)))
        self.next_id = int(o.next_id)
        self.lost_slam_idxs = lost[:self.n_lost].copy()
        self.claimed = claimed.copy()
        self.lists, e = [], 0
        for l in range(5):
            k = int(o.n_list[l])
            first, last = int(off[e]), int(off[e + k])
            self.lists.append(dict(ids=ids[e:e + k].copy(), off=(off[e:e + k + 1] - first).astype(np.int32), xy=xy[first:last].copy()))
            e += k
        for name, lst in zip(self.NAMES, self.lists):
            setattr(self, name, lst)
