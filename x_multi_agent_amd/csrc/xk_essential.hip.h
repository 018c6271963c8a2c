// xk_essential.hip.h -- essential-matrix RANSAC filter of PlaceRecognition::findCorrespondences (gfx950).
//
//   cv::findEssentialMat(current_points, received_points, K, cv::RANSAC, 0.99, 1.0, mask)   (place_recognition.cpp:269-281)
//
// Three launches on the handle's stream, no host round trip between them:
//   xk_ess_solve    one thread per hypothesis: five distinct pairs from the counter-based splitmix64 sampler, the
//                   five-point minimal solver, up to ten unit-norm candidates into the device scratch block
//   xk_ess_score    one workgroup per hypothesis, lanes over points: squared Sampson distance of every pair under every
//                   candidate, inlier count and summed inlier distance per candidate, the hypothesis' best candidate,
//                   and a packed 64-bit atomicMax key (count << 32 | ~hypothesis) -- order-independent
//   xk_ess_mask     the winner's inlier set, its E and count
//
// The pair count is a value (the stage entry, xk_pr_essential_ransac) or, with XkEssArgs::n_dev, what an earlier launch on the
// stream left in device memory (xk_pr_find_correspondences, xk_correspond.hip.h): then n only bounds grids and buffers.
//
// All n_hyp hypotheses are evaluated.  The CPU estimator's adaptive stop (prob = 0.99) only truncates a sequential loop,
// and the best of all hypotheses is at least the best of any prefix: `prob` is therefore not a parameter.
//
// fp64 throughout.  Convention: rec^T E cur = 0 on x = (u - cx)/fx, y = (v - cy)/fy; threshold t = threshold_px/((fx+fy)/2).
//
// The minimal solver (Nister's five-point route, every step stated so that a CPU restatement can follow it):
//   1. null space of the 5 x 9 epipolar system: five Householder reflectors on its transpose, the last four columns of Q
//   2. det E = 0 and 2 E E^T E - tr(E E^T) E = 0 on E = x X + y Y + z Z + W: a 10 x 20 system in the monomials of degree <= 3
//   3. Gauss-Jordan with row pivoting on the ten columns x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy
//   4. the 3 x 3 polynomial matrix B(z) from the rows <x^2z> - z <x^2>, <y^2z> - z <y^2>, <xyz> - z <xy>; det B(z) has degree 10
//   5. its real roots: the roots of each derivative bracket the roots of the next, safeguarded Newton inside each bracket
//   6. (x, y) from the null vector of B(z), then three Gauss-Newton steps on the ten constraints themselves
//   7. unit Frobenius norm; a pivot below XK_ESS_PIVOT_FLOOR (relative) or a non-finite candidate drops the sample
// The solver functions are __host__ __device__ so that the same text can be exercised on a CPU.  Sampler, null space (1.),
// root finder (5.), the score kernel's body and the winner's decoding are shared with xk_fundamental.hip.h: xk_ransac.hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "xk_ransac.hip.h"

#define XK_ESS_MAXC 10            // candidates per hypothesis
#define XK_ESS_MAX_HYP 4096
#define XK_ESS_PIVOT_FLOOR 1e-13  // relative to the largest entry of the 10 x 20 system
#define XK_ESS_WS 201             // doubles of workspace per hypothesis: the 10 x 20 system, odd stride (LDS banks)
#define XK_ESS_SOLVE_T 32         // hypotheses per workgroup of the solve kernel (32 x 201 doubles of LDS)

// ---- polynomials in (x, y, z, w = 1): monomials as sorted index tuples in lexicographic order ----
// quadratic (a <= b): 10;  cubic (a <= b <= c): 20
XK_RANSAC_HD int xk_ess_c3(int a, int b, int c) {
  const int off[4] = {0, 10, 16, 19};
  const int m = 4 - a, bb = b - a, cc = c - a;
  return off[a] + bb * m - bb * (bb - 1) / 2 + (cc - bb);
}
// o[10] += s * p[4] * q[4]
XK_RANSAC_HD void xk_ess_ll(const double *p, const double *q, double s, double *o) {
  int idx = 0;
  for (int a = 0; a < 4; ++a)
    for (int b = a; b < 4; ++b, ++idx) o[idx] += s * (a == b ? p[a] * q[a] : p[a] * q[b] + p[b] * q[a]);
}
// o[20] += Q[10] * l[4]
XK_RANSAC_HD void xk_ess_ql(const double *Q, const double *l, double *o) {
  int idx = 0;
  for (int a = 0; a < 4; ++a)
    for (int b = a; b < 4; ++b, ++idx)
      for (int c = 0; c < 4; ++c) {
        const int m = c < a ? xk_ess_c3(c, a, b) : (c < b ? xk_ess_c3(a, c, b) : xk_ess_c3(a, b, c));
        o[m] += Q[idx] * l[c];
      }
}

XK_RANSAC_HD void xk_ess_mat3(const double *A, const double *B, double *C, bool ta, bool tb) {   // C = op(A) op(B)
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += (ta ? A[3 * k + i] : A[3 * i + k]) * (tb ? B[3 * j + k] : B[3 * k + j]);
      C[3 * i + j] = s;
    }
}

// f[10] = (det E, 2 E E^T E - tr(E E^T) E)
XK_RANSAC_HD void xk_ess_constraints(const double *E, double *f) {
  double T[9], TE[9];
  xk_ess_mat3(E, E, T, false, true);
  xk_ess_mat3(T, E, TE, false, false);
  const double tr = T[0] + T[4] + T[8];
  f[0] = E[0] * (E[4] * E[8] - E[5] * E[7]) - E[1] * (E[3] * E[8] - E[5] * E[6]) + E[2] * (E[3] * E[7] - E[4] * E[6]);
  for (int i = 0; i < 9; ++i) f[1 + i] = 2.0 * TE[i] - tr * E[i];
}

// One Gauss-Newton step on the ten constraints in (x, y, z); Nt[9][4] holds (X, Y, Z, W) entry by entry.
XK_RANSAC_HD void xk_ess_polish(const double (*Nt)[4], double *xyz) {
  double E[9], f[10], J[3][10], T[9], S[9];
  for (int e = 0; e < 9; ++e) E[e] = xyz[0] * Nt[e][0] + xyz[1] * Nt[e][1] + xyz[2] * Nt[e][2] + Nt[e][3];
  xk_ess_constraints(E, f);
  xk_ess_mat3(E, E, T, false, true);    // E E^T
  xk_ess_mat3(E, E, S, true, false);    // E^T E
  const double tr = T[0] + T[4] + T[8];
  const double cof[9] = {E[4] * E[8] - E[5] * E[7], E[5] * E[6] - E[3] * E[8], E[3] * E[7] - E[4] * E[6],
                         E[2] * E[7] - E[1] * E[8], E[0] * E[8] - E[2] * E[6], E[1] * E[6] - E[0] * E[7],
                         E[1] * E[5] - E[2] * E[4], E[2] * E[3] - E[0] * E[5], E[0] * E[4] - E[1] * E[3]};
  for (int v = 0; v < 3; ++v) {
    double D[9], a[9], b[9], c[9], t1[9];
    double dd = 0.0, trd = 0.0;
    for (int e = 0; e < 9; ++e) { D[e] = Nt[e][v]; dd += cof[e] * D[e]; trd += E[e] * D[e]; }
    xk_ess_mat3(D, S, a, false, false);       // dE E^T E
    xk_ess_mat3(E, D, t1, false, true);       // E dE^T
    xk_ess_mat3(t1, E, b, false, false);      // E dE^T E
    xk_ess_mat3(T, D, c, false, false);       // E E^T dE
    J[v][0] = dd;
    for (int e = 0; e < 9; ++e) J[v][1 + e] = 2.0 * (a[e] + b[e] + c[e]) - 2.0 * trd * E[e] - tr * D[e];
  }
  double A[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};   // J^T J (00 01 02 11 12 22), J^T f
  for (int r = 0; r < 10; ++r) {
    A[0] += J[0][r] * J[0][r]; A[1] += J[0][r] * J[1][r]; A[2] += J[0][r] * J[2][r];
    A[3] += J[1][r] * J[1][r]; A[4] += J[1][r] * J[2][r]; A[5] += J[2][r] * J[2][r];
    g[0] += J[0][r] * f[r]; g[1] += J[1][r] * f[r]; g[2] += J[2][r] * f[r];
  }
  const double c00 = A[3] * A[5] - A[4] * A[4], c01 = A[2] * A[4] - A[1] * A[5], c02 = A[1] * A[4] - A[2] * A[3];
  const double c11 = A[0] * A[5] - A[2] * A[2], c12 = A[1] * A[2] - A[0] * A[4], c22 = A[0] * A[3] - A[1] * A[1];
  const double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
  if (!(fabs(det) > 0.0)) return;
  const double d0 = (c00 * g[0] + c01 * g[1] + c02 * g[2]) / det, d1 = (c01 * g[0] + c11 * g[1] + c12 * g[2]) / det,
               d2 = (c02 * g[0] + c12 * g[1] + c22 * g[2]) / det;
  if (d0 == d0 && d1 == d1 && d2 == d2) { xyz[0] -= d0; xyz[1] -= d1; xyz[2] -= d2; }
}

// Five normalised pairs -> candidates Eout[<= 10][9] (row-major, unit Frobenius norm, ascending z); returns their number.
// ws: XK_ESS_WS doubles of workspace (LDS on the device).
XK_RANSAC_HD int xk_ess_solve5(const double (*cur)[2], const double (*rec)[2], double *ws, double *Eout) {
  // 1. null space
  double Nt[9][4];
  xk_ransac_null_space<5>(cur, rec, Nt);
  // 2. the ten cubics, columns in elimination order
  const int col_of[20] = {0, 2, 4, 5, 3, 8, 9, 10, 11, 12, 1, 6, 7, 13, 14, 15, 16, 17, 18, 19};   // lexicographic -> column
  {
    double G[6][10], row[20];
    const int sym[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
    for (int s = 0; s < 6; ++s)
      for (int m = 0; m < 10; ++m) G[s][m] = 0.0;
    for (int i = 0; i < 3; ++i)
      for (int k = i; k < 3; ++k)
        for (int m = 0; m < 3; ++m) xk_ess_ll(Nt[3 * i + m], Nt[3 * k + m], 2.0, G[sym[i][k]]);   // 2 E E^T
    for (int m = 0; m < 10; ++m) {
      const double tr = 0.5 * (G[0][m] + G[3][m] + G[5][m]);
      G[0][m] -= tr; G[3][m] -= tr; G[5][m] -= tr;
    }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        for (int m = 0; m < 20; ++m) row[m] = 0.0;
        for (int k = 0; k < 3; ++k) xk_ess_ql(G[sym[i][k]], Nt[3 * k + j], row);
        for (int m = 0; m < 20; ++m) ws[(1 + 3 * i + j) * 20 + col_of[m]] = row[m];
      }
    // det E = sum_j E_0j cof_j
    for (int m = 0; m < 20; ++m) row[m] = 0.0;
    for (int j = 0; j < 3; ++j) {
      const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      double cof[10];
      for (int m = 0; m < 10; ++m) cof[m] = 0.0;
      xk_ess_ll(Nt[3 + j1], Nt[6 + j2], 1.0, cof);
      xk_ess_ll(Nt[3 + j2], Nt[6 + j1], -1.0, cof);
      xk_ess_ql(cof, Nt[j], row);
    }
    for (int m = 0; m < 20; ++m) ws[col_of[m]] = row[m];
  }
  // 3. Gauss-Jordan, row pivoting
  double big = 0.0;
  for (int i = 0; i < 200; ++i) big = fmax(big, fabs(ws[i]));
  if (!(big > 0.0) || !(big < 1e300)) return 0;
  for (int p = 0; p < 10; ++p) {
    int pr = p;
    double pv = fabs(ws[p * 20 + p]);
    for (int r = p + 1; r < 10; ++r)
      if (fabs(ws[r * 20 + p]) > pv) { pv = fabs(ws[r * 20 + p]); pr = r; }
    if (!(pv > XK_ESS_PIVOT_FLOOR * big)) return 0;
    if (pr != p)
      for (int c = p; c < 20; ++c) { const double t = ws[p * 20 + c]; ws[p * 20 + c] = ws[pr * 20 + c]; ws[pr * 20 + c] = t; }
    const double inv = 1.0 / ws[p * 20 + p];
    for (int c = p; c < 20; ++c) ws[p * 20 + c] *= inv;
    for (int r = 0; r < 10; ++r) {
      if (r == p) continue;
      const double m = ws[r * 20 + p];
      for (int c = p; c < 20; ++c) ws[r * 20 + c] -= m * ws[p * 20 + c];
    }
  }
  // 4. B(z): rows (4,5), (6,7), (8,9); columns x, y, 1; ascending powers of z
  double bz[3][3][5], poly[11];
  for (int r = 0; r < 3; ++r) {
    const double *e = ws + (4 + 2 * r) * 20 + 10, *f = ws + (5 + 2 * r) * 20 + 10;
    for (int q = 0; q < 2; ++q) {
      bz[r][q][0] = e[3 * q + 2]; bz[r][q][1] = e[3 * q + 1] - f[3 * q + 2]; bz[r][q][2] = e[3 * q] - f[3 * q + 1];
      bz[r][q][3] = -f[3 * q]; bz[r][q][4] = 0.0;
    }
    bz[r][2][0] = e[9]; bz[r][2][1] = e[8] - f[9]; bz[r][2][2] = e[7] - f[8]; bz[r][2][3] = e[6] - f[7]; bz[r][2][4] = -f[6];
  }
  for (int m = 0; m < 11; ++m) poly[m] = 0.0;
  for (int r = 0; r < 3; ++r) {
    const int r1 = (r + 1) % 3, r2 = (r + 2) % 3;     // cyclic: the cofactor sign is +
    double minor[7];
    for (int m = 0; m < 7; ++m) minor[m] = 0.0;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) minor[i + j] += bz[r1][0][i] * bz[r2][1][j] - bz[r1][1][i] * bz[r2][0][j];
    for (int i = 0; i < 5; ++i)
      for (int j = 0; j < 7; ++j) poly[i + j] += bz[r][2][i] * minor[j];
  }
  // 5. real roots
  double pmax = 0.0;
  for (int m = 0; m < 11; ++m) pmax = fmax(pmax, fabs(poly[m]));
  if (!(pmax > 0.0) || !(pmax < 1e300)) return 0;
  for (int m = 0; m < 11; ++m) poly[m] /= pmax;
  double roots[10];
  const int nr = fabs(poly[10]) > 0.0 ? xk_ransac_real_roots<10>(poly, roots) : -1;   // (no usable leading coefficient)
  if (nr <= 0) return 0;
  // 6., 7.
  for (int s = 0; s < nr; ++s) {
    const double z = roots[s];
    double b[3][3];
    for (int r = 0; r < 3; ++r)
      for (int q = 0; q < 3; ++q) b[r][q] = xk_ransac_horner(bz[r][q], 4, z);
    double best[3] = {0, 0, 0}, bn = -1.0;
    for (int r = 0; r < 3; ++r) {
      const int r1 = (r + 1) % 3, r2 = (r + 2) % 3;
      const double v[3] = {b[r1][1] * b[r2][2] - b[r1][2] * b[r2][1], b[r1][2] * b[r2][0] - b[r1][0] * b[r2][2],
                           b[r1][0] * b[r2][1] - b[r1][1] * b[r2][0]};
      const double nn = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
      if (nn > bn) { bn = nn; best[0] = v[0]; best[1] = v[1]; best[2] = v[2]; }
    }
    double xyz[3] = {best[0] / best[2], best[1] / best[2], z};
    for (int it = 0; it < 3; ++it) xk_ess_polish(Nt, xyz);
    double E[9], nn = 0.0;
    for (int e = 0; e < 9; ++e) {
      E[e] = xyz[0] * Nt[e][0] + xyz[1] * Nt[e][1] + xyz[2] * Nt[e][2] + Nt[e][3];
      nn += E[e] * E[e];
    }
    const double inv = 1.0 / sqrt(nn);
    for (int e = 0; e < 9; ++e) {
      E[e] *= inv;
      if (!(fabs(E[e]) <= 2.0)) return 0;      // non-finite
      Eout[9 * s + e] = E[e];
    }
  }
  return nr;
}

// Squared Sampson distance of the pair (cur, rec) under rec^T E cur = 0.
XK_RANSAC_HD double xk_ess_sampson(const double *E, double cx, double cy, double rx, double ry) {
  const double c0 = E[0] * cx + E[1] * cy + E[2], c1 = E[3] * cx + E[4] * cy + E[5], c2 = E[6] * cx + E[7] * cy + E[8];
  const double t0 = E[0] * rx + E[3] * ry + E[6], t1 = E[1] * rx + E[4] * ry + E[7];
  const double num = rx * c0 + ry * c1 + c2;
  return num * num / (c0 * c0 + c1 * c1 + t0 * t0 + t1 * t1);
}

struct XkEssArgs {
  const float *cur_xy, *rec_xy;     // [n][2] pixels
  int n, n_hyp;
  const int *n_dev;                 // NULL: n pairs.  Else n is the bound the grids are sized by, *n_dev the count (xk_dev_count)
  double fx, fy, cx, cy, t2;
  unsigned long long seed;
  XkRansacScratch s;                // XK_ESS_MAX_HYP hypotheses of XK_ESS_MAXC candidates
  // result
  unsigned char *mask;              // [n]
  double *E;                        // [9]
  int *res;                         // n_inliers, winner hypothesis
};

__global__ __launch_bounds__(XK_ESS_SOLVE_T) void xk_ess_solve(XkEssArgs a) {
  __shared__ double ws[XK_ESS_SOLVE_T * XK_ESS_WS];
  const int h = blockIdx.x * XK_ESS_SOLVE_T + threadIdx.x;
  if (h == 0) *a.s.key = 0ull;
  if (h >= a.n_hyp) return;
  const int n = xk_dev_count(a.n_dev, a.n);
  double *E = a.s.cand + (size_t)h * (XK_ESS_MAXC * 9);
  if (n < 5) {                      // (the sampler has no rejection loop: below five pairs its indices leave the list)
    for (int i = 0; i < XK_ESS_MAXC * 9; ++i) E[i] = 0.0;
    a.s.ncand[h] = 0;
    return;
  }
  int pick[5];
  xk_ransac_sample<5>(a.seed, h, n, pick);
  double cur[5][2], rec[5][2];
  for (int k = 0; k < 5; ++k) {
    cur[k][0] = ((double)a.cur_xy[2 * pick[k]] - a.cx) / a.fx; cur[k][1] = ((double)a.cur_xy[2 * pick[k] + 1] - a.cy) / a.fy;
    rec[k][0] = ((double)a.rec_xy[2 * pick[k]] - a.cx) / a.fx; rec[k][1] = ((double)a.rec_xy[2 * pick[k] + 1] - a.cy) / a.fy;
  }
  const int nc = xk_ess_solve5(cur, rec, ws + threadIdx.x * XK_ESS_WS, E);
  for (int i = nc * 9; i < XK_ESS_MAXC * 9; ++i) E[i] = 0.0;
  a.s.ncand[h] = nc;
}

// The squared Sampson distance of pair i, pixels normalised on the way.
__device__ __forceinline__ double xk_ess_error_at(const XkEssArgs &a, const double *E, int i) {
  return xk_ess_sampson(E, ((double)a.cur_xy[2 * i] - a.cx) / a.fx, ((double)a.cur_xy[2 * i + 1] - a.cy) / a.fy,
                        ((double)a.rec_xy[2 * i] - a.cx) / a.fx, ((double)a.rec_xy[2 * i + 1] - a.cy) / a.fy);
}

__global__ __launch_bounds__(256) void xk_ess_score(XkEssArgs a) {
  xk_ransac_score<XK_ESS_MAXC>(a.s, xk_dev_count(a.n_dev, a.n), a.t2, [&](const double *E, int i) { return xk_ess_error_at(a, E, i); });
}

__global__ __launch_bounds__(256) void xk_ess_mask(XkEssArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x, n = xk_dev_count(a.n_dev, a.n);
  const XkRansacWinner w = xk_ransac_winner(*a.s.key);
  if (!w.valid) {
    if (i < n) a.mask[i] = 0;
    if (i < 9) a.E[i] = 0.0;
    if (i == 0) { a.res[0] = 0; a.res[1] = -1; }
    return;
  }
  const double *Ep = a.s.cand + ((size_t)w.h * XK_ESS_MAXC + a.s.bestc[w.h]) * 9;
  const double E[9] = {Ep[0], Ep[1], Ep[2], Ep[3], Ep[4], Ep[5], Ep[6], Ep[7], Ep[8]};
  if (i < n) a.mask[i] = xk_ess_error_at(a, E, i) <= a.t2 ? 1 : 0;
  if (i < 9) a.E[i] = Ep[i];
  if (i == 0) { a.res[0] = w.count; a.res[1] = w.h; }
}
