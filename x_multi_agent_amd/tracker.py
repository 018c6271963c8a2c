"""Outlier removal of the tracker's matches on the device -- ctypes binding of the xk_trk_* entry points
(include/xk.h).  Mirrors the undistortion and the fundamental-matrix RANSAC of `Tracker::track`
(src/x/vision/tracker.cpp:233-293, camera.cpp:62-87): what every frame's match list passes through before the track
manager sees it.

No fallback: everything numeric runs in libxk.so's HIP kernels (csrc/xk_fundamental.hip.h)."""
import ctypes as C

import numpy as np

from .engine import XkError, c_dp, c_ip

c_ub = C.POINTER(C.c_ubyte)
c_fp = C.POINTER(C.c_float)


class MatchFilter:
    """The camera model and the RANSAC of x::Tracker on one agent's GPU.  K = (fx, fy, cx, cy) in pixels or a 3 x 3 camera
    matrix, s = the FOV distortion parameter (0: none)."""

    def __init__(self, eng, max_matches, K, s=0.0):
        self.eng, self.L = eng, eng.L
        K = np.asarray(K, np.float64)
        self.K = tuple(float(v) for v in ((K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.shape == (3, 3) else K.ravel()))
        self.s = float(s)
        self.max_matches = int(max_matches)
        self.p = C.c_void_p()
        rc = self.L.xk_trk_create(eng.h, C.c_int(self.max_matches), *(C.c_double(v) for v in self.K), C.c_double(self.s),
                                  C.byref(self.p))
        if rc != 0:
            raise XkError(rc, "xk_trk_create", (self.L.xk_last_error(eng.h) or b"").decode())

    def close(self):
        if self.p:
            self.L.xk_trk_destroy(self.p)
            self.p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise XkError(rc, what, (self.L.xk_last_error(self.eng.h) or b"").decode())

    def undistort(self, dist_xy):
        """Camera::undistort (camera.cpp:62-87): distorted pixels [n, 2] -> undistorted pixels [n, 2], fp64."""
        d = np.ascontiguousarray(dist_xy, np.float64).reshape(-1, 2)
        out = np.zeros((max(len(d), 1), 2))
        self._chk(self.L.xk_trk_undistort(self.p, d.ctypes.data_as(c_dp), C.c_int(len(d)), out.ctypes.data_as(c_dp)), "xk_trk_undistort")
        return out[:len(d)]

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
