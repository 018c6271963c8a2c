// xk_aux.hip.h -- the non-visual rows of the visual update: the laser-range-finder facet row (RangeUpdate::processRangedFacet,
// src/x/vio/range_update.cpp:61-270) and the two sun-sensor rows (SolarUpdate::processSunAngle, src/x/vio/solar_update.cpp:36-94),
// stacked by VioUpdater::constructUpdate under the MSCKF, MSCKF-SLAM and SLAM rows (vio_updater.cpp:352-423).
//
// One workgroup builds both from the staged window, SLAM features and measurement, evaluates the range row's chi2_1(0.9) gate against
// the RESIDENT prior (h has at most 33 non-zeros: h P h^T gathers a 33 x 33 block of P) and writes [rows | residual] (row-major,
// n + 1 doubles per row), the chosen variances and the gate result into a small device block.  The rows never go through the QR: the
// update appends them to whatever system the compression left (xk_api.hip, launch_update).
#pragma once
#include <hip/hip_runtime.h>

#define XK_AUX_THREADS 256
#define XK_AUX_NMAX 528      // n <= 15 + 511 (C1P <= 512, xk_create)

// The staged measurement as the kernel reads it (a kernel argument: no copy of its own).
struct XkAuxIn {
  double range, img_x, img_y, var_range;   // RangeMeasurement (types.h:224-238), sigma_range^2
  double q_imu[4];                         // state.getOrientation(), xyzw
  double ang[2];                           // SunAngleMeasurement x_angle, y_angle (deg)
  double s_q_i[4];                         // sun sensor -> IMU, xyzw (the reference writes it (w, x, y, z), solar_update.cpp:51)
  double g_sun[3];                         // sun vector in the world frame (normalised here, :55)
  double var_sun;                          // deg^2 (:47)
  double var_comp;                         // sigma_img^2: every row's variance when the reference compresses the stack (vio_updater.cpp:507-509)
  double chi1;                             // chi2_1(0.9), range_update.cpp:250-251
  int facet[3];                            // tr_feat_ids
  int has_range, has_sun, compressed;
};

struct XkAuxArgs {
  const double *q, *p;      // window lists (xyzw / xyz per pose)
  int n_poses, N;           // poses in the window, n_poses_max
  const double *feat;       // SLAM inverse-depth states [3M]
  const int *anchor;        // SLAM anchors [M]
  const double *P;          // prior, n x n column-major
  int n;
  XkAuxIn in;
  double *rows;             // [naux][n + 1]: range row first (if staged), then the two sun rows; column n = residual
  double *rdiag;            // [naux]
  double *flags;            // [0] range gamma, [1] range inlier (1 / 0)
};

__device__ __forceinline__ void xk_aux_rot(const double *q, double *r /*row-major*/) {
  // q.normalized().toRotationMatrix(), q stored xyzw
  const double nn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double x = q[0] / nn, y = q[1] / nn, z = q[2] / nn, w = q[3] / nn;
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  r[0] = 1 - (tyy + tzz); r[1] = txy - twz;       r[2] = txz + twy;
  r[3] = txy + twz;       r[4] = 1 - (txx + tzz); r[5] = tyz - twx;
  r[6] = txz - twy;       r[7] = tyz + twx;       r[8] = 1 - (txx + tyy);
}
__device__ __forceinline__ void xk_aux_cross(const double *a, const double *b, double *c) {
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
// row vector v^T times [u]x (x::Skew, tools.h:57-65): v^T [u]x w = v . (u x w) = w . (v x u)
__device__ __forceinline__ void xk_aux_vskew(const double *v, const double *u, double *o) { xk_aux_cross(v, u, o); }
// row vector v^T R (R row-major)
__device__ __forceinline__ void xk_aux_vR(const double *v, const double *R, double *o) {
  for (int k = 0; k < 3; ++k) o[k] = v[0] * R[k] + v[1] * R[3 + k] + v[2] * R[6 + k];
}

__global__ __launch_bounds__(XK_AUX_THREADS) void xk_aux_rows(XkAuxArgs a) {
  __shared__ double row[3][XK_AUX_NMAX + 1];
  __shared__ int ecol[33];
  __shared__ double eval_[33];
  __shared__ double red[XK_AUX_THREADS];
  __shared__ double sres;
  const XkAuxIn &in = a.in;
  const int n = a.n, tid = threadIdx.x;
  const int naux = (in.has_range ? 1 : 0) + (in.has_sun ? 2 : 0);
  for (int e = tid; e < 3 * (XK_AUX_NMAX + 1); e += blockDim.x) (&row[0][0])[e] = 0.0;
  __syncthreads();
  if (tid == 0 && in.has_range) {
    // ---- range_update.cpp:76-230 ----
    double f[3][3], Ra[3][9], al[3], be[3], rh[3];
    int an[3];
    for (int j = 0; j < 3; ++j) {
      const int id = in.facet[j];
      al[j] = a.feat[3 * id]; be[j] = a.feat[3 * id + 1]; rh[j] = a.feat[3 * id + 2];
      an[j] = a.anchor[id];
      xk_aux_rot(a.q + 4 * an[j], Ra[j]);
      const double u[3] = {al[j], be[j], 1.0};
      for (int r = 0; r < 3; ++r)
        f[j][r] = 1.0 / rh[j] * (Ra[j][3 * r] * u[0] + Ra[j][3 * r + 1] * u[1] + Ra[j][3 * r + 2] * u[2]) + a.p[3 * an[j] + r];
    }
    const int pos = a.n_poses - 1;             // current camera: the last window entry (C_q_G.back())
    double Rn[9];
    xk_aux_rot(a.q + 4 * pos, Rn);
    const double *pn = a.p + 3 * pos;
    double d01[3], d21[3], Gn[3];
    for (int r = 0; r < 3; ++r) { d01[r] = f[0][r] - f[1][r]; d21[r] = f[2][r] - f[1][r]; }
    xk_aux_cross(d01, d21, Gn);
    const double l[3] = {in.img_x, in.img_y, 1.0};
    double RtG[3];
    for (int k = 0; k < 3; ++k) RtG[k] = Rn[k] * Gn[0] + Rn[3 + k] * Gn[1] + Rn[6 + k] * Gn[2];
    const double A = (f[1][0] - pn[0]) * Gn[0] + (f[1][1] - pn[1]) * Gn[1] + (f[1][2] - pn[2]) * Gn[2];
    const double B = l[0] * RtG[0] + l[1] * RtG[1] + l[2] * RtG[2];
    const double range_hat = A / B;
    sres = in.range - range_hat;
    // blocks: current position / attitude, per feature anchor position / attitude and the feature itself (:160-230)
    double blk[11][3];
    int bcol[11];
    for (int k = 0; k < 3; ++k) blk[0][k] = -1.0 / B * Gn[k];
    {
      double t[3];
      xk_aux_vR(Gn, Rn, t);
      xk_aux_vskew(t, l, blk[1]);
      for (int k = 0; k < 3; ++k) blk[1][k] *= A / (B * B);
    }
    bcol[0] = XK_CORE + 3 * pos;
    bcol[1] = XK_CORE + 3 * (a.N + pos);
    double Gpr[3], bary[3];
    for (int r = 0; r < 3; ++r) {
      Gpr[r] = A / B * (Rn[3 * r] * l[0] + Rn[3 * r + 1] * l[1] + Rn[3 * r + 2] * l[2]) + pn[r];
      bary[r] = 1.0 / 3.0 * (f[0][r] + f[1][r] + f[2][r]);
    }
    double bmr[3];
    for (int r = 0; r < 3; ++r) bmr[r] = bary[r] - Gpr[r];
    for (int j = 0; j < 3; ++j) {
      const int j1 = (j + 2) % 3, j2 = (j + 1) % 3;   // J_f0: f2 - f1, J_f1: f0 - f2, J_f2: f1 - f0
      double e[3], c[3], Jf[3];
      for (int r = 0; r < 3; ++r) e[r] = f[j1][r] - f[j2][r];
      xk_aux_cross(e, bmr, c);
      for (int k = 0; k < 3; ++k) Jf[k] = 1.0 / B * (1.0 / 3.0 * Gn[k] + c[k]);
      double *Jp = blk[2 + 3 * j], *Jq = blk[3 + 3 * j], *Ji = blk[4 + 3 * j];
      for (int k = 0; k < 3; ++k) Jp[k] = Jf[k];
      double t[3];
      xk_aux_vR(Jf, Ra[j], t);
      const double u[3] = {al[j], be[j], 1.0};
      xk_aux_vskew(t, u, Jq);
      for (int k = 0; k < 3; ++k) Jq[k] *= -1.0 / rh[j];
      // mat = I, column 2 = (-alpha / rho, -beta / rho, -1 / rho)
      Ji[0] = 1.0 / rh[j] * t[0];
      Ji[1] = 1.0 / rh[j] * t[1];
      Ji[2] = 1.0 / rh[j] * (t[0] * (-al[j] / rh[j]) + t[1] * (-be[j] / rh[j]) + t[2] * (-1.0 / rh[j]));
      bcol[2 + 3 * j] = XK_CORE + 3 * an[j];
      bcol[3 + 3 * j] = XK_CORE + 3 * (a.N + an[j]);
      bcol[4 + 3 * j] = XK_CORE + 3 * (2 * a.N + in.facet[j]);
    }
    // accumulated in the reference's order: current pose first, then per feature anchor position, anchor attitude, feature
    for (int b = 0; b < 11; ++b)
      for (int k = 0; k < 3; ++k) {
        row[0][bcol[b] + k] += blk[b][k];
        ecol[3 * b + k] = bcol[b] + k;
        eval_[3 * b + k] = blk[b][k];
      }
  }
  if (tid == 0 && in.has_sun) {
    // ---- solar_update.cpp:36-94 ----
    const int r0 = in.has_range ? 1 : 0;
    double Rq[9], Rs[9];
    xk_aux_rot(in.q_imu, Rq);
    xk_aux_rot(in.s_q_i, Rs);
    const double gn = sqrt(in.g_sun[0] * in.g_sun[0] + in.g_sun[1] * in.g_sun[1] + in.g_sun[2] * in.g_sun[2]);
    const double g[3] = {in.g_sun[0] / gn, in.g_sun[1] / gn, in.g_sun[2] / gn};
    double v[3], s[3];
    for (int k = 0; k < 3; ++k) v[k] = Rq[k] * g[0] + Rq[3 + k] * g[1] + Rq[6 + k] * g[2];      // R_q^T G_sun
    for (int k = 0; k < 3; ++k) s[k] = Rs[k] * v[0] + Rs[3 + k] * v[1] + Rs[6 + k] * v[2];      // R_s^T R_q^T G_sun
    const double sn = sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    for (int k = 0; k < 3; ++k) s[k] /= sn;
    const double R2D = 57.2957795130;
    const double h0 = R2D * atan2(s[0], s[2]), h1 = R2D * atan2(s[1], s[2]);
    row[r0][n] = in.ang[0] - h0;
    row[r0 + 1][n] = in.ang[1] - h1;
    const double d0 = s[0] * s[0] + s[2] * s[2], d1 = s[1] * s[1] + s[2] * s[2];
    const double m[2][3] = {{s[2] / d0, 0.0, -s[0] / d0}, {0.0, s[2] / d1, -s[1] / d1}};
    for (int i = 0; i < 2; ++i) {
      double t[3], o[3];
      // mat R_s^T: (m R_s^T)_k = sum_r m_r Rs[k][r]
      for (int k = 0; k < 3; ++k) t[k] = m[i][0] * Rs[3 * k] + m[i][1] * Rs[3 * k + 1] + m[i][2] * Rs[3 * k + 2];
      xk_aux_vskew(t, v, o);
      for (int k = 0; k < 3; ++k) row[r0 + i][6 + k] = R2D * o[k];   // kIdxQ = 6
    }
  }
  __syncthreads();
  // ---- range gate (range_update.cpp:235-262): gamma = r^2 / (h P h^T + sigma_range^2) against the prior ----
  if (in.has_range) {
    double acc = 0.0;
    for (int e = tid; e < 33 * 33; e += blockDim.x) {
      const int i = e / 33, j = e % 33;
      acc += eval_[i] * eval_[j] * a.P[(size_t)ecol[i] + (size_t)ecol[j] * n];
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = XK_AUX_THREADS / 2; s > 0; s >>= 1) {
      if (tid < s) red[tid] += red[tid + s];
      __syncthreads();
    }
    const double S = red[0] + in.var_range;
    const double r = sres;
    const double gamma = r * (1.0 / S) * r;
    const bool inl = gamma < in.chi1;
    if (!inl)                                  // rejected: a zero row, residual 0, variance 1 (RangeUpdate's initial state, :26-30)
      for (int e = tid; e < n; e += blockDim.x) row[0][e] = 0.0;
    if (tid == 0) {
      row[0][n] = inl ? r : 0.0;
      a.flags[0] = gamma;
      a.flags[1] = inl ? 1.0 : 0.0;
      a.rdiag[0] = in.compressed ? in.var_comp : (inl ? in.var_range : 1.0);
    }
    __syncthreads();
  }
  if (tid == 0 && in.has_sun) {
    const int r0 = in.has_range ? 1 : 0;
    a.rdiag[r0] = a.rdiag[r0 + 1] = in.compressed ? in.var_comp : in.var_sun;
  }
  for (int e = tid; e < naux * (n + 1); e += blockDim.x) a.rows[e] = row[e / (n + 1)][e % (n + 1)];
}

// [base system | aux rows] -> one dense system over all n columns (row-major, row stride ld = n + 1, residual in column n) with its
// variance vector: the base rows (c of them, columns [col0, col0 + kdim) of T, residual z) carry rscalar, the aux rows their own.
struct XkAuxStackArgs {
  const double *T; long str, stc; int c, kdim, col0;
  const double *z; long sz;
  const double *rdiag; double rscalar;
  const double *aux; const double *aux_rdiag; int naux;
  int n; double *out; double *out_rdiag;
};
__global__ __launch_bounds__(256) void xk_aux_stack(XkAuxStackArgs a) {
  const int r = blockIdx.x, ld = a.n + 1;
  double *dst = a.out + (size_t)r * ld;
  if (r < a.c) {
    for (int j = threadIdx.x; j <= a.n; j += blockDim.x) {
      double v = 0.0;
      if (j == a.n) v = a.z[(size_t)r * a.sz];
      else if (j >= a.col0 && j < a.col0 + a.kdim) v = a.T[(size_t)r * a.str + (size_t)(j - a.col0) * a.stc];
      dst[j] = v;
    }
    if (threadIdx.x == 0) a.out_rdiag[r] = a.rdiag ? a.rdiag[r] : a.rscalar;
  } else {
    const double *src = a.aux + (size_t)(r - a.c) * ld;
    for (int j = threadIdx.x; j <= a.n; j += blockDim.x) dst[j] = src[j];
    if (threadIdx.x == 0) a.out_rdiag[r] = a.aux_rdiag[r - a.c];
  }
}
