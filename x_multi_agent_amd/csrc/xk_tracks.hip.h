// xk_tracks.hip.h -- normalisation and baseline check of a batch of feature tracks (gfx950): the numerical part of
// TrackManager::manageTracks (track_manager.cpp:115-436).
//
//   Camera::normalize(track, max_size): the newest min(length, max_size) observations, (u - cx) / fx, (v - cy) / fy   (camera.cpp)
//   TrackManager::checkBaseline: every normalised ray (x, y, 1) rotated into the last camera of the attitude list, the extent of
//                                the rotated coordinates per axis against two thresholds                     (track_manager.cpp:576-636)
//
// Neither depends on where the manager's list walk stands when it asks, so one launch per frame serves every candidate track
// (DESIGN 3.16).  tests/track_manager_np.py restates both in Python floats, operation by operation.
//
//   xk_tracks_baseline  one WAVEFRONT per track, one lane per kept observation (a window holds at most 64 poses), XK_TRACKS_WAVES
//                       tracks per workgroup.  The attitude list is normalised into the LDS once per workgroup (one lane per
//                       quaternion), one barrier; after it no wavefront waits for another.  The minimum and maximum per axis are
//                       butterflies over the wavefront.  fp64 throughout, no atomics, no inline assembly.
// The normalisation has no multiply-add to contract: norm_xy is the host mirror's x::Camera::normalize bit for bit.  The rotation
// is written without contraction, so that the restatement follows it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define XK_TRACKS_MAX_QUATS 64     // one lane per pose of the window
#define XK_TRACKS_WAVES 4          // tracks per workgroup

struct XkTracksArgs {
  const double *quat;              // [n_quats][4] xyzw, C_q_G oldest first
  const int *trk_off;              // [K + 1] into obs_xy, in observations
  const int *norm_off;             // [K + 1] into norm_xy: the prefix sum of the cropped lengths (the host has it from the validation)
  const unsigned char *drop_last;  // [K] 1: the track's list is the first n_quats - 1 attitudes (cam_rots_short)
  const double *obs_xy;            // undistorted pixels
  int K, n_quats;
  double fx, fy, cx, cy;
  double min_x, min_y;             // min_baseline_x_n, min_baseline_y_n
  double *norm_xy;
  double *delta_xy;                // [K][2]
  unsigned char *flag;             // [K]
};

// min and max of the values that are numbers: a NaN on either side gives the other side (NaN only if both are)
__device__ __forceinline__ double xk_tracks_min(double a, double b) { return b != b ? a : a != a ? b : b < a ? b : a; }
__device__ __forceinline__ double xk_tracks_max(double a, double b) { return b != b ? a : a != a ? b : b > a ? b : a; }

// Hamilton product r = a b of quaternions held as (w, x, y, z), the order Eigen::Quaterniond multiplies in
__device__ __forceinline__ void xk_tracks_qmul(const double *a, const double *b, double *r) {
#pragma clang fp contract(off)
  r[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  r[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  r[2] = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3];
  r[3] = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
}

// The body of the launch for the first K tracks of a batch: xk_tracks_baseline takes K from its arguments, the track store's kernel
// (xk_track_store.hip.h) from the count an earlier launch left on the device.  Every thread of the workgroup calls it (one barrier).
__device__ __forceinline__ void xk_tracks_baseline_body(const XkTracksArgs &a, int K) {
#pragma clang fp contract(off)
  __shared__ double q_n[XK_TRACKS_MAX_QUATS][4];                 // the normalised attitudes as (w, x, y, z)
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < a.n_quats) {                                 // (n_quats <= 64: the first wavefront)
    const double x = a.quat[4 * threadIdx.x], y = a.quat[4 * threadIdx.x + 1], z = a.quat[4 * threadIdx.x + 2], w = a.quat[4 * threadIdx.x + 3];
    const double n2 = x * x + y * y + z * z + w * w;
    const double n = n2 > 0.0 ? sqrt(n2) : 1.0;                  // Eigen's normalized(): a zero quaternion stays as it is
    q_n[threadIdx.x][0] = w / n; q_n[threadIdx.x][1] = x / n; q_n[threadIdx.x][2] = y / n; q_n[threadIdx.x][3] = z / n;
  }
  __syncthreads();
  const int k = blockIdx.x * XK_TRACKS_WAVES + (threadIdx.x >> 6);
  if (k >= K) return;                                             // (a whole wavefront, after the only barrier)
  const int o0 = a.trk_off[k], len_all = a.trk_off[k + 1] - o0;
  const int nq = a.n_quats - (int)a.drop_last[k];
  const int len = len_all < nq ? len_all : nq;                   // Camera::normalize(track, nq): the newest len observations
  const int i_last = nq - 1, i_first = i_last - len + 1;         // track_manager.cpp:588-589
  const double *obs = a.obs_xy + 2 * (size_t)(o0 + len_all - len);
  const double NaN = __longlong_as_double(0x7ff8000000000000ll);
  double rx = NaN, ry = NaN;                                     // lanes without an observation take no part
  if (lane < len) {
    const double x = (obs[2 * lane] - a.cx) / a.fx, y = (obs[2 * lane + 1] - a.cy) / a.fy;
    double *out = a.norm_xy + 2 * ((size_t)a.norm_off[k] + lane);
    out[0] = x; out[1] = y;
    // Cn_q_Ci = conj(Ci_q_G) Cn_q_G, the ray conj(Cn_q_Ci) (0, x, y, 1) Cn_q_Ci (track_manager.cpp:606-610)
    const double *ci = q_n[i_first + lane], *cn = q_n[i_last];
    const double ci_c[4] = {ci[0], -ci[1], -ci[2], -ci[3]};
    double q[4], t[4], r[4];
    xk_tracks_qmul(ci_c, cn, q);
    const double q_c[4] = {q[0], -q[1], -q[2], -q[3]}, ray[4] = {0.0, x, y, 1.0};
    xk_tracks_qmul(q_c, ray, t);
    xk_tracks_qmul(t, q, r);
    rx = r[1] / r[3]; ry = r[2] / r[3];                          // (a zero z: an infinity takes part, 0 / 0 does not)
  }
  double mnx = rx, mxx = rx, mny = ry, mxy = ry;
  for (int o = 32; o > 0; o >>= 1) {
    mnx = xk_tracks_min(mnx, __shfl_xor(mnx, o, 64)); mxx = xk_tracks_max(mxx, __shfl_xor(mxx, o, 64));
    mny = xk_tracks_min(mny, __shfl_xor(mny, o, 64)); mxy = xk_tracks_max(mxy, __shfl_xor(mxy, o, 64));
  }
  if (lane == 0) {
    // The reference starts its minimum and maximum at the UNROTATED last observation (:592-595) and updates them with
    // `if (v < min) min = v; else if (v > max) max = v;`.  With the starting value in the set min <= max always holds, so no v is
    // below the one and above the other: the chain equals a plain minimum and maximum over the rotated coordinates and that value.
    // A NaN coordinate fails both comparisons and takes no part; a NaN starting value stays (every comparison with it fails).
    const double x0 = (obs[2 * (len - 1)] - a.cx) / a.fx, y0 = (obs[2 * (len - 1) + 1] - a.cy) / a.fy;
    const double dx = x0 != x0 ? x0 : xk_tracks_max(x0, mxx) - xk_tracks_min(x0, mnx);
    const double dy = y0 != y0 ? y0 : xk_tracks_max(y0, mxy) - xk_tracks_min(y0, mny);
    a.delta_xy[2 * k] = dx; a.delta_xy[2 * k + 1] = dy;
    a.flag[k] = (dx > a.min_x || dy > a.min_y) ? 1 : 0;          // :632
  }
}

__global__ __launch_bounds__(64 * XK_TRACKS_WAVES) void xk_tracks_baseline(XkTracksArgs a) { xk_tracks_baseline_body(a, a.K); }
