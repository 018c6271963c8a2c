// xk_camera.h -- the radial-tangential and the equidistant camera model on conditioned coordinates x = (u - cx)/fx, y = (v - cy)/fy:
// the forward map and its Newton inverse, one point at a time (DESIGN 3.10.2 defines both).  Plain C++ with no HIP in it, so that
// the device (xk_fundamental.hip.h: xk_cam_undistort1, xk_cam_distort1) and the host mirror (host/src/camera.cpp) compile the SAME
// text; the FOV model stays where it was (xk_fund_undistort1, Camera::radialGain).
//
// k[5] are the coefficients: radial-tangential k1 k2 p1 p2 k3, equidistant k1 k2 k3 k4 (k[4] unused).
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define XK_CAM_HD __host__ __device__ inline
#else
#define XK_CAM_HD inline
#endif

#define XK_CAM_MODEL_FOV 0
#define XK_CAM_MODEL_RADTAN 1
#define XK_CAM_MODEL_EQUIDISTANT 2
#define XK_CAM_MAX_STEPS 20        // of either Newton iteration
#define XK_CAM_RADTAN_TOL 1e-28    // converged: dx^2 + dy^2 <= tol (1 + x^2 + y^2), the point after the step
#define XK_CAM_EQUI_TOL 1e-14      // converged: |dtheta| <= tol (1 + |theta|), the angle after the step
#define XK_CAM_EQUI_RMIN 1e-8      // at or below this radius the equidistant scale is 1
#define XK_CAM_HALF_PI 1.5707963267948966

// The radial-tangential forward map at (x, y) and, with J, its Jacobian [dxd/dx dxd/dy; dyd/dx dyd/dy] as J[0..3].
XK_CAM_HD void xk_cam_radtan(const double *k, double x, double y, double *xd, double *yd, double *J) {
  const double r2 = x * x + y * y;
  const double g = 1.0 + r2 * (k[0] + r2 * (k[1] + r2 * k[4]));
  *xd = x * g + 2.0 * k[2] * x * y + k[3] * (r2 + 2.0 * x * x);
  *yd = y * g + k[2] * (r2 + 2.0 * y * y) + 2.0 * k[3] * x * y;
  if (J) {
    const double gp = k[0] + r2 * (2.0 * k[1] + 3.0 * k[4] * r2);      // dg / d(r^2)
    const double off = 2.0 * x * y * gp + 2.0 * k[2] * x + 2.0 * k[3] * y;
    J[0] = g + 2.0 * x * x * gp + 2.0 * k[2] * y + 6.0 * k[3] * x;
    J[1] = off;
    J[2] = off;
    J[3] = g + 2.0 * y * y * gp + 6.0 * k[2] * y + 2.0 * k[3] * x;
  }
}

// theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8) and, with d, its derivative.
XK_CAM_HD double xk_cam_equi_theta(const double *k, double th, double *d) {
  const double t2 = th * th;
  if (d) *d = 1.0 + t2 * (3.0 * k[0] + t2 * (5.0 * k[1] + t2 * (7.0 * k[2] + t2 * 9.0 * k[3])));
  return th * (1.0 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))));
}

// The forward map of `model` (radial-tangential or equidistant) at the undistorted point (x, y).
XK_CAM_HD void xk_cam_forward(int model, const double *k, double x, double y, double *xd, double *yd) {
  if (model == XK_CAM_MODEL_RADTAN) {
    xk_cam_radtan(k, x, y, xd, yd, nullptr);
    return;
  }
  const double r = sqrt(x * x + y * y);
  double scale = 1.0;
  if (r > XK_CAM_EQUI_RMIN) scale = xk_cam_equi_theta(k, atan(r), nullptr) / r;
  *xd = x * scale; *yd = y * scale;
}

// The inverse of `model` (radial-tangential or equidistant) at the distorted point (xd, yd): true and (*x, *y) where the iteration
// converged; false where the point is INVALID -- the model folds there (the derivative is not > 0; a NaN lands here too), the
// equidistant angle leaves (0, pi/2), or XK_CAM_MAX_STEPS steps have passed -- and then (*x, *y) means nothing.  *steps: Newton
// steps taken (0 where the equidistant radius is not above its floor).
XK_CAM_HD bool xk_cam_inverse(int model, const double *k, double xd, double yd, double *x_out, double *y_out, int *steps) {
  double x = xd, y = yd;
  bool done = false;
  *steps = 0;
  if (model == XK_CAM_MODEL_RADTAN) {
    for (int it = 0; it < XK_CAM_MAX_STEPS; ++it) {
      double fx, fy, J[4];
      xk_cam_radtan(k, x, y, &fx, &fy, J);
      const double det = J[0] * J[3] - J[1] * J[2];
      if (!(det > 0.0)) break;
      const double ex = fx - xd, ey = fy - yd;
      const double dx = -(J[3] * ex - J[1] * ey) / det, dy = -(J[0] * ey - J[2] * ex) / det;
      x += dx; y += dy;
      *steps = it + 1;
      if (dx * dx + dy * dy <= XK_CAM_RADTAN_TOL * (1.0 + x * x + y * y)) { done = true; break; }
    }
  } else {
    const double rd = sqrt(xd * xd + yd * yd);
    if (rd <= XK_CAM_EQUI_RMIN) {
      done = true;                               // (scale 1)
    } else {
      double th = rd;
      for (int it = 0; it < XK_CAM_MAX_STEPS; ++it) {
        double d;
        const double f = xk_cam_equi_theta(k, th, &d) - rd;
        if (!(d > 0.0)) break;
        const double dth = -f / d;
        th += dth;
        *steps = it + 1;
        if (!(th > 0.0 && th < XK_CAM_HALF_PI)) break;
        if (fabs(dth) <= XK_CAM_EQUI_TOL * (1.0 + fabs(th))) { done = true; break; }
      }
      const double scale = tan(th) / rd;
      x = xd * scale; y = yd * scale;
    }
  }
  *x_out = x; *y_out = y;
  return done && fabs(x) < 1e300 && fabs(y) < 1e300;
}
