// xk_fundamental.hip.h -- fundamental-matrix RANSAC / LMedS filter of the tracker's matches, Tracker::track (gfx950).
//
//   camera_.undistort(current_features); camera_.undistort(previous_features_);           (tracker.cpp:233-237, camera.cpp:62-87)
//   cv::findFundamentalMat(pts1, pts2, cv::RANSAC, 0.3, 0.99, mask); keep the masked pairs (tracker.cpp:243-293)
//
// Four launches on the handle's stream, no host round trip between them:
//   xk_fund_undistort  one thread per point, both lists: the FOV model's inverse (camera.cpp:69-87) -- or, after xk_trk_camera_model,
//                      the Newton inverse of the radial-tangential or the equidistant model (xk_camera.h), one branch per thread,
//                      invalid points and the largest step count into two counters -- the fp64 undistorted
//                      pixels (what the matches carry) and their float cast widened back to fp64 (what the RANSAC sees: the
//                      reference casts to cv::Point2f, tracker.cpp:251-256)
//   xk_fund_solve      one thread per hypothesis: seven distinct pairs from the counter-based splitmix64 sampler, the
//                      seven-point minimal solver, up to three unit-norm candidates in PIXEL coordinates
//   xk_fund_score      one workgroup per hypothesis, lanes over points: max(d1^2, d2^2) of the two point-to-epipolar-line
//                      distances of every pair under every candidate, inlier count and summed inlier error per candidate, the
//                      hypothesis' best candidate, and a packed 64-bit atomicMax key (count << 32 | ~hypothesis)
//   xk_fund_mask       one workgroup: the winner's mask, F and count (counted here, with the mask), and the ORDERED
//                      compaction (workgroup scan) of the kept indices and of the kept pairs' undistorted fp64 pixels
//                      (tracker.cpp:262-271 pushes them in order)
//
// Under outlier_method = cv::LMEDS (xk_trk_outlier_method, xk_trk_fundamental_lmeds) the last two launches are instead
//   xk_fund_median     the same grid as xk_fund_score: per candidate the median 0.5 (e[(n-1)/2] + e[n/2]) of the pairs' errors by
//                      radix select in LDS (xk_ransac_median), the hypothesis' candidate of smallest median
//   xk_fund_mask_lmeds one workgroup: the argmin over the hypotheses (smallest median, lowest hypothesis, lowest candidate),
//                      sigma = 2.5 * 1.4826 * (1 + 5 / (n - 7)) * sqrt(median), at least 0.001, the mask error <= sigma^2 and the
//                      same compaction; the winner's median and sigma go behind the result block
// n < 8 keeps nothing there.  For 8 <= n <= 13 both middle errors belong to the seven sample points, which every candidate fits
// exactly: the medians are round-off and the selection is arbitrary (in OpenCV too); the formula is kept.
//
// All n_hyp hypotheses are evaluated, so there is no `prob` (xk_essential.hip.h says why).  No refit.
//
// fp64 throughout.  Convention: p1 = previous, p2 = current, p2^T F p1 = 0, F row-major.  The solve runs on conditioned
// coordinates x = (u - cx)/fx, y = (v - cy)/fy; the score runs on pixels.
//
// The minimal solver, every step stated so that a CPU restatement can follow it:
//   1. null space of the 7 x 9 epipolar system (row p: p2_i p1_j at 3i + j): seven Householder reflectors on its
//      transpose; the last two columns of Q are F1, F2 (unit norm, orthogonal)
//   2. det(l F1 + (1 - l) F2) = det(F2 + l D), D = F1 - F2: c0 = [a0 a1 a2], c1 = [d0 a1 a2] + [a0 d1 a2] + [a0 a1 d2],
//      c2 = [d0 d1 a2] + [d0 a1 d2] + [a0 d1 d2], c3 = [d0 d1 d2] in triple products of the rows a of F2 and d of D
//   3. degenerate cubics, with m = max |c_k| and f = XK_FUND_COEF_FLOOR:
//        m <= f                    every member of the pencil is singular (F1, F2 have unit norm, so the floor is relative to
//                                  them): the candidates are F1 and F2 themselves
//        |c3| <= f m               a root at infinity: the candidate F1 - F2, and the roots of the polynomial deflated to its
//                                  highest coefficient above f m
//   4. real roots by xk_ransac_real_roots: the roots of each derivative bracket the roots of the next, safeguarded Newton
//      inside each bracket (no trigonometric closed form)
//   5. per root F = l F1 + (1 - l) F2, unit Frobenius norm, K^-T F K^-1, unit norm again; ascending l, special candidates
//      last; a non-finite candidate is dropped
// There is NO collinearity or other degeneracy test of the sample: a degenerate sample yields candidates that score badly.
//
// Mapping: the 63 doubles of the system stay in registers (every loop of the solver with constant bounds is unrolled), one
// thread per hypothesis, no LDS workspace.  Sampler, null space, root finder, score body, winner and compaction: xk_ransac.hip.h.  The solver functions are __host__ __device__ so that the same text can be
// exercised on a CPU.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "xk_camera.h"
#include "xk_ransac.hip.h"

#define XK_FUND_MAXC 3             // candidates per hypothesis
#define XK_FUND_MAX_HYP 4096
#define XK_FUND_COEF_FLOOR 1e-12   // relative: to max |c_k| for the leading coefficient, to the unit-norm pencil for all of them
#define XK_FUND_SOLVE_T 64         // hypotheses per workgroup of the solve kernel: one wavefront

XK_RANSAC_HD double xk_fund_triple(const double *x, const double *y, const double *z) {
  return x[0] * (y[1] * z[2] - y[2] * z[1]) - x[1] * (y[0] * z[2] - y[2] * z[0]) + x[2] * (y[0] * z[1] - y[1] * z[0]);
}

// Fn (conditioned coordinates, any scale) -> unit norm, K^-T Fn K^-1, unit norm again, into out[9]; false if not finite.
XK_RANSAC_HD bool xk_fund_to_pixels(const double *Fn, double fx, double fy, double cx, double cy, double *out) {
  double nn = 0.0, F[9], G[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) nn += Fn[e] * Fn[e];
  double inv = 1.0 / sqrt(nn);
#pragma unroll
  for (int e = 0; e < 9; ++e) F[e] = Fn[e] * inv;
#pragma unroll
  for (int i = 0; i < 3; ++i) {                // G = F K^-1
    G[3 * i] = F[3 * i] / fx;
    G[3 * i + 1] = F[3 * i + 1] / fy;
    G[3 * i + 2] = F[3 * i + 2] - F[3 * i] * cx / fx - F[3 * i + 1] * cy / fy;
  }
  nn = 0.0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {                // K^-T G
    F[j] = G[j] / fx;
    F[3 + j] = G[3 + j] / fy;
    F[6 + j] = G[6 + j] - G[j] * cx / fx - G[3 + j] * cy / fy;
    nn += F[j] * F[j] + F[3 + j] * F[3 + j] + F[6 + j] * F[6 + j];
  }
  inv = 1.0 / sqrt(nn);
  bool ok = true;
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    out[e] = F[e] * inv;
    ok = ok && (fabs(out[e]) <= 2.0);          // (false for a NaN too)
  }
  return ok;
}

// Seven conditioned pairs -> candidates Fout[<= 3][9] (row-major, pixel coordinates, unit Frobenius norm); returns their number.
XK_RANSAC_HD int xk_fund_solve7(const double (*p1)[2], const double (*p2)[2], double fx, double fy, double cx, double cy,
                             double *Fout) {
  // 1. null space
  double Nt[9][2], F1[9], F2[9];
  xk_ransac_null_space<7>(p1, p2, Nt);
#pragma unroll
  for (int t = 0; t < 9; ++t) { F1[t] = Nt[t][0]; F2[t] = Nt[t][1]; }
  // 2. the cubic
  double D[9], c[4];
#pragma unroll
  for (int e = 0; e < 9; ++e) D[e] = F1[e] - F2[e];
  c[0] = xk_fund_triple(F2, F2 + 3, F2 + 6);
  c[1] = xk_fund_triple(D, F2 + 3, F2 + 6) + xk_fund_triple(F2, D + 3, F2 + 6) + xk_fund_triple(F2, F2 + 3, D + 6);
  c[2] = xk_fund_triple(D, D + 3, F2 + 6) + xk_fund_triple(D, F2 + 3, D + 6) + xk_fund_triple(F2, D + 3, D + 6);
  c[3] = xk_fund_triple(D, D + 3, D + 6);
  const double cmax = fmax(fmax(fabs(c[0]), fabs(c[1])), fmax(fabs(c[2]), fabs(c[3])));
  if (!(cmax < 1e300)) return 0;               // (non-finite input)
  int nc = 0;
  // 3. degenerate cubics
  if (cmax <= XK_FUND_COEF_FLOOR) {
    if (xk_fund_to_pixels(F1, fx, fy, cx, cy, Fout + 9 * nc)) ++nc;
    if (xk_fund_to_pixels(F2, fx, fy, cx, cy, Fout + 9 * nc)) ++nc;
    return nc;
  }
  const double flo = XK_FUND_COEF_FLOOR * cmax;
  const int deg = fabs(c[3]) > flo ? 3 : (fabs(c[2]) > flo ? 2 : (fabs(c[1]) > flo ? 1 : 0));
  // 4. real roots
  double roots[3] = {0.0, 0.0, 0.0};
  int nr = 0;
  if (deg == 3) nr = xk_ransac_real_roots<3>(c, roots);
  else if (deg == 2) nr = xk_ransac_real_roots<2>(c, roots);
  else if (deg == 1) nr = xk_ransac_real_roots<1>(c, roots);
  if (nr < 0) nr = 0;
  // 5. candidates
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    if (s < nr && nc < XK_FUND_MAXC) {
      double Fn[9];
#pragma unroll
      for (int e = 0; e < 9; ++e) Fn[e] = F2[e] + roots[s] * D[e];
      if (xk_fund_to_pixels(Fn, fx, fy, cx, cy, Fout + 9 * nc)) ++nc;
    }
  }
  if (deg < 3 && nc < XK_FUND_MAXC && xk_fund_to_pixels(D, fx, fy, cx, cy, Fout + 9 * nc)) ++nc;
  return nc;
}

// OpenCV's fundamental-matrix error of the pair (p1, p2) in pixels: the larger of the two squared point-to-epipolar-line
// distances (not Sampson's).
XK_RANSAC_HD double xk_fund_error(const double *F, double x1, double y1, double x2, double y2) {
  double a = F[0] * x1 + F[1] * y1 + F[2], b = F[3] * x1 + F[4] * y1 + F[5], c = F[6] * x1 + F[7] * y1 + F[8];
  const double e2 = x2 * a + y2 * b + c, s2 = a * a + b * b;
  a = F[0] * x2 + F[3] * y2 + F[6]; b = F[1] * x2 + F[4] * y2 + F[7]; c = F[2] * x2 + F[5] * y2 + F[8];
  const double e1 = x1 * a + y1 * b + c, s1 = a * a + b * b;
  return fmax(e1 * e1 / s1, e2 * e2 / s2);     // (fmax drops one NaN; two, 0/0 under F = 0, compare false against t2)
}

// camera.cpp:69-87 on one distorted pixel; s_term = 1 / (2 tan(s/2)) (camera.cpp:39), unused where s = 0.
XK_RANSAC_HD void xk_fund_undistort1(double ud, double vd, double fx, double fy, double cx, double cy, double s, double s_term,
                                  double *u, double *v) {
  const double x = (ud - cx) / fx, y = (vd - cy) / fy;
  const double r = sqrt(x * x + y * y);
  double f = 1.0;
  if (r > 0.01 && s != 0.0) f = tan(r * s) * s_term / r;
  *u = f * x * fx + cx;
  *v = f * y * fy + cy;
}

// The camera models of xk_trk_camera_model: the FOV model above, or one of xk_camera.h's two, between the pinhole
// arithmetic of xk_fund_undistort1.  k[5]: the model's coefficients (unused under the FOV model).
// One distorted pixel through the inverse of `model`: false where the point is INVALID (xk_cam_inverse says when); an invalid point
// keeps its distorted pixel, bit for bit.  *steps: Newton steps taken (0 under the FOV model, which has a closed form).
XK_RANSAC_HD bool xk_cam_undistort1(int model, const double *k, double ud, double vd, double fx, double fy, double cx, double cy, double s,
                                 double s_term, double *u, double *v, int *steps) {
  if (model == XK_CAM_MODEL_FOV) {
    *steps = 0;
    xk_fund_undistort1(ud, vd, fx, fy, cx, cy, s, s_term, u, v);
    return true;
  }
  double x, y;
  const bool ok = xk_cam_inverse(model, k, (ud - cx) / fx, (vd - cy) / fy, &x, &y, steps);
  *u = ok ? x * fx + cx : ud;
  *v = ok ? y * fy + cy : vd;
  return ok;
}

// One undistorted pixel through the forward map of `model`.  FOV: r_d = atan(2 r tan(s/2)) / s = atan(r / s_term) / s, and the identity
// where that r_d is not above the 0.01 below which xk_fund_undistort1 is the identity too.
XK_RANSAC_HD void xk_cam_distort1(int model, const double *k, double u, double v, double fx, double fy, double cx, double cy, double s,
                               double s_term, double *ud, double *vd) {
  const double x = (u - cx) / fx, y = (v - cy) / fy;
  double xd = x, yd = y;
  if (model != XK_CAM_MODEL_FOV) {
    xk_cam_forward(model, k, x, y, &xd, &yd);
  } else if (s != 0.0) {
    const double r = sqrt(x * x + y * y);
    const double rd = atan(r / s_term) / s;
    if (rd > 0.01) { xd = x * (rd / r); yd = y * (rd / r); }
  }
  *ud = xd * fx + cx;
  *vd = yd * fy + cy;
}


struct XkFundArgs {
  const double *dist;               // [n_pts][2] distorted pixels (xk_fund_undistort only)
  double *und;                      // [n_pts][2] undistorted pixels, fp64: previous list, then the current one behind it
  double *pts;                      // [n_pts][2] the same through float
  int n_pts;                        // points of xk_fund_undistort (2 n for a frame)
  int n, n_hyp;
  double fx, fy, cx, cy, s, s_term, t2;
  unsigned long long seed;
  XkRansacScratch sc;               // XK_FUND_MAX_HYP hypotheses of XK_FUND_MAXC candidates
  // result
  double *F;                        // [9]
  XkKeptPairs kept;                 // res: n_inliers, winner hypothesis
  unsigned char *mask;              // [n]
  double *lmeds;                    // [2] the winner's median and sigma (xk_fund_mask_lmeds only)
  int min_n;                        // fewer pairs than this leave no candidate: 7, least median of squares 8
  const int *n_dev;                 // NULL: n pairs.  Else n is the bound every list is laid out by (the current list starts 2 n doubles behind
                                    //   the previous one), *n_dev the count (xk_dev_count); xk_fund_undistort then takes n_pts = 2 n
  int model;                        // XK_CAM_MODEL_*: what xk_fund_undistort and xk_cam_distort apply (xk_trk_camera_model)
  double cam_k[5];                  // its coefficients; unused under the FOV model, which has s and s_term
  int *cam_cnt;                     // [2] invalid points, largest step count: cleared in front of xk_fund_undistort.  NULL under the FOV model
};

__global__ __launch_bounds__(256) void xk_fund_undistort(XkFundArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_pts) return;
  if (a.n_dev && (i >= a.n ? i - a.n : i) >= xk_dev_count(a.n_dev, a.n)) return;   // (past the count of its list)
  double u, v;
  if (a.model == XK_CAM_MODEL_FOV) {
    xk_fund_undistort1(a.dist[2 * i], a.dist[2 * i + 1], a.fx, a.fy, a.cx, a.cy, a.s, a.s_term, &u, &v);
  } else {
    int steps;
    const bool ok = xk_cam_undistort1(a.model, a.cam_k, a.dist[2 * i], a.dist[2 * i + 1], a.fx, a.fy, a.cx, a.cy, a.s, a.s_term, &u, &v, &steps);
    if (!ok) atomicAdd(a.cam_cnt, 1);
    if (steps > 0) atomicMax(a.cam_cnt + 1, steps);
  }
  a.und[2 * i] = u; a.und[2 * i + 1] = v;
  a.pts[2 * i] = (double)(float)u; a.pts[2 * i + 1] = (double)(float)v;
}

// The forward map of a list: und [n_pts][2] undistorted pixels -> pts [n_pts][2] distorted pixels, one thread per point.
__global__ __launch_bounds__(256) void xk_cam_distort(XkFundArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_pts) return;
  double ud, vd;
  xk_cam_distort1(a.model, a.cam_k, a.und[2 * i], a.und[2 * i + 1], a.fx, a.fy, a.cx, a.cy, a.s, a.s_term, &ud, &vd);
  a.pts[2 * i] = ud; a.pts[2 * i + 1] = vd;
}

__global__ __launch_bounds__(XK_FUND_SOLVE_T) void xk_fund_solve(XkFundArgs a) {
  const int h = blockIdx.x * XK_FUND_SOLVE_T + threadIdx.x;
  if (h == 0) *a.sc.key = 0ull;
  if (h >= a.n_hyp) return;
  const int n = xk_dev_count(a.n_dev, a.n);
  if (n < a.min_n) {                            // (only with a device count: the stage entries return before the launch.  No candidate, so
    a.sc.ncand[h] = 0;                          //  the key stays zero and xk_fund_mask keeps nothing)
    return;
  }
  int pick[7];
  xk_ransac_sample<7>(a.seed, h, n, pick);
  const double *P1 = a.pts, *P2 = a.pts + 2 * (size_t)a.n;
  double p1[7][2], p2[7][2];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    p1[k][0] = (P1[2 * pick[k]] - a.cx) / a.fx; p1[k][1] = (P1[2 * pick[k] + 1] - a.cy) / a.fy;
    p2[k][0] = (P2[2 * pick[k]] - a.cx) / a.fx; p2[k][1] = (P2[2 * pick[k] + 1] - a.cy) / a.fy;
  }
  double *F = a.sc.cand + (size_t)h * (XK_FUND_MAXC * 9);   // (written in place: a slot index in registers would be a runtime one)
  const int nc = xk_fund_solve7(p1, p2, a.fx, a.fy, a.cx, a.cy, F);
  for (int i = nc * 9; i < XK_FUND_MAXC * 9; ++i) F[i] = 0.0;
  a.sc.ncand[h] = nc;
}

__global__ __launch_bounds__(256) void xk_fund_score(XkFundArgs a) {
  const double *P1 = a.pts, *P2 = a.pts + 2 * (size_t)a.n;
  xk_ransac_score<XK_FUND_MAXC>(a.sc, xk_dev_count(a.n_dev, a.n), a.t2, [&](const double *F, int i) {
    return xk_fund_error(F, P1[2 * i], P1[2 * i + 1], P2[2 * i], P2[2 * i + 1]);
  });
}

// The winner's mask, F and count, and the ordered compaction of the kept pairs: valid = false keeps nothing.  Fp: the winner's candidate.
__device__ __forceinline__ void xk_fund_keep(const XkFundArgs &a, bool valid, int h, const double *Fp, double t2) {
  const double F[9] = {Fp[0], Fp[1], Fp[2], Fp[3], Fp[4], Fp[5], Fp[6], Fp[7], Fp[8]};
  const double *P1 = a.pts, *P2 = a.pts + 2 * (size_t)a.n;
  const double *U1 = a.und, *U2 = a.und + 2 * (size_t)a.n;
  const int kept = xk_ransac_compact(
      xk_dev_count(a.n_dev, a.n),
      [&](int i) {
        const bool keep = valid && xk_fund_error(F, P1[2 * i], P1[2 * i + 1], P2[2 * i], P2[2 * i + 1]) <= t2;
        a.mask[i] = keep ? 1 : 0;
        return keep;
      },
      [&](int i, int pos) {
        a.kept.keep_idx[pos] = i;
        a.kept.kept_prev[2 * pos] = U1[2 * i]; a.kept.kept_prev[2 * pos + 1] = U1[2 * i + 1];
        a.kept.kept_cur[2 * pos] = U2[2 * i]; a.kept.kept_cur[2 * pos + 1] = U2[2 * i + 1];
      });
  if (threadIdx.x < 9) a.F[threadIdx.x] = valid ? Fp[threadIdx.x] : 0.0;
  // (the count is this kernel's own: the length of what it compacted, whatever the scoring kernel's rounding made of the same pairs)
  if (threadIdx.x == 0) { a.kept.res[0] = kept; a.kept.res[1] = valid ? h : -1; }
}

__global__ __launch_bounds__(256) void xk_fund_mask(XkFundArgs a) {
  const XkRansacWinner w = xk_ransac_winner(*a.sc.key);
  const int h = w.valid ? w.h : 0;
  xk_fund_keep(a, w.valid, h, a.sc.cand + ((size_t)h * XK_FUND_MAXC + (w.valid ? a.sc.bestc[h] : 0)) * 9, a.t2);
}

// Least median of squares (cv::LMEDS): xk_fund_median takes the place of xk_fund_score, xk_fund_mask_lmeds that of xk_fund_mask.
// A count below a.min_n = 8 leaves no candidate (the scale needs n - 7 > 0; xk_fund_solve has left ncand = 0 then).
__global__ __launch_bounds__(256) void xk_fund_median(XkFundArgs a) {
  const double *P1 = a.pts, *P2 = a.pts + 2 * (size_t)a.n;
  xk_ransac_median<XK_FUND_MAXC>(a.sc, max(xk_dev_count(a.n_dev, a.n), 1), [&](const double *F, int i) {
    return xk_fund_error(F, P1[2 * i], P1[2 * i + 1], P2[2 * i], P2[2 * i + 1]);
  });
}

// sigma = 2.5 * 1.4826 * (1 + 5 / (n - 7)) * sqrt(med), at least 0.001, evaluated in this order (OpenCV's LMeDSPointSetRegistrator);
// there is no multiply-add in it to contract.  An inlier has error <= sigma^2.
__global__ __launch_bounds__(256) void xk_fund_mask_lmeds(XkFundArgs a) {
  const int n = xk_dev_count(a.n_dev, a.n);
  const XkMedianWinner w = xk_ransac_median_winner(a.sc, a.n_hyp, XK_FUND_MAXC);
  const bool valid = w.valid && n >= a.min_n;
  double sigma = 0.0;
  if (valid) {
    sigma = 2.5 * 1.4826 * (1.0 + 5.0 / (double)(n - 7)) * sqrt(w.med);
    sigma = fmax(sigma, 0.001);
  }
  xk_fund_keep(a, valid, w.h, a.sc.cand + ((size_t)w.h * XK_FUND_MAXC + (valid ? a.sc.bestc[w.h] : 0)) * 9, sigma * sigma);
  if (threadIdx.x == 0) { a.lmeds[0] = valid ? w.med : 0.0; a.lmeds[1] = sigma; }
}
