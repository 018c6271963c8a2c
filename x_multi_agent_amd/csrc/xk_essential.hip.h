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
// The solver functions are __host__ __device__ so that the same text can be exercised on a CPU.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define XK_ESS_HD __host__ __device__ inline
#define XK_ESS_MAXC 10            // candidates per hypothesis
#define XK_ESS_MAX_HYP 4096
#define XK_ESS_PIVOT_FLOOR 1e-13  // relative to the largest entry of the 10 x 20 system
#define XK_ESS_WS 201             // doubles of workspace per hypothesis: the 10 x 20 system, odd stride (LDS banks)
#define XK_ESS_SOLVE_T 32         // hypotheses per workgroup of the solve kernel (32 x 201 doubles of LDS)

XK_ESS_HD unsigned long long xk_ess_mix(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// Hypothesis h draws values 5h .. 5h+4 of the stream (value i = mix(seed + (i+1) golden)); draw k lands in [0, n-k) and
// is shifted past the earlier picks in ascending order: five distinct indices, no rejection loop.
XK_ESS_HD void xk_ess_sample(unsigned long long seed, int h, int n, int pick[5]) {
  unsigned int sorted[5];
  for (int k = 0; k < 5; ++k) {
    const unsigned long long z = xk_ess_mix(seed + (unsigned long long)(5ll * h + k + 1) * 0x9E3779B97F4A7C15ull);
    unsigned int r = (unsigned int)(((z >> 32) * (unsigned long long)(n - k)) >> 32);
    int m = 0;
    while (m < k && r >= sorted[m]) { ++r; ++m; }
    for (int j = k; j > m; --j) sorted[j] = sorted[j - 1];
    sorted[m] = r;
    pick[k] = (int)r;
  }
}

// ---- polynomials in (x, y, z, w = 1): monomials as sorted index tuples in lexicographic order ----
// quadratic (a <= b): 10;  cubic (a <= b <= c): 20
XK_ESS_HD int xk_ess_c3(int a, int b, int c) {
  const int off[4] = {0, 10, 16, 19};
  const int m = 4 - a, bb = b - a, cc = c - a;
  return off[a] + bb * m - bb * (bb - 1) / 2 + (cc - bb);
}
// o[10] += s * p[4] * q[4]
XK_ESS_HD void xk_ess_ll(const double *p, const double *q, double s, double *o) {
  int idx = 0;
  for (int a = 0; a < 4; ++a)
    for (int b = a; b < 4; ++b, ++idx) o[idx] += s * (a == b ? p[a] * q[a] : p[a] * q[b] + p[b] * q[a]);
}
// o[20] += Q[10] * l[4]
XK_ESS_HD void xk_ess_ql(const double *Q, const double *l, double *o) {
  int idx = 0;
  for (int a = 0; a < 4; ++a)
    for (int b = a; b < 4; ++b, ++idx)
      for (int c = 0; c < 4; ++c) {
        const int m = c < a ? xk_ess_c3(c, a, b) : (c < b ? xk_ess_c3(a, c, b) : xk_ess_c3(a, b, c));
        o[m] += Q[idx] * l[c];
      }
}

XK_ESS_HD double xk_ess_horner(const double *c, int d, double x) {
  double f = c[d];
  for (int k = d - 1; k >= 0; --k) f = f * x + c[k];
  return f;
}

// The root of the degree-d polynomial c in (lo, hi), f(lo) and f(hi) of opposite sign: Newton, bisection where it leaves
// the bracket or stalls.
XK_ESS_HD double xk_ess_bracket_root(const double *c, int d, double lo, double hi, double flo) {
  double xl = flo < 0 ? lo : hi, xh = flo < 0 ? hi : lo;
  double x = 0.5 * (lo + hi), dxold = fabs(hi - lo), dx = dxold;
  for (int it = 0; it < 200; ++it) {
    double f = c[d], df = 0.0;
    for (int k = d - 1; k >= 0; --k) { df = df * x + f; f = f * x + c[k]; }
    if (f < 0) xl = x; else xh = x;
    if (f == 0.0) return x;
    double xn = x - f / df;
    if (xn > fmin(xl, xh) && xn < fmax(xl, xh) && fabs(2.0 * f) <= fabs(dxold * df)) {
      dxold = dx; dx = xn - x;
    } else {                                   // (a non-finite Newton step lands here too)
      dxold = dx; dx = 0.5 * (xh - xl); xn = xl + dx;
    }
    if (xn == x || fabs(dx) <= 1e-15 * fabs(xn)) return xn;
    x = xn;
  }
  return x;
}

// Real roots of c[0..10] (ascending), ascending; -1 where the polynomial has no usable leading coefficient.
XK_ESS_HD int xk_ess_real_roots(const double *c, double *roots) {
  double prev[10], cur[10], pd[11];
  int nprev = 0;
  if (!(fabs(c[10]) > 0.0)) return -1;
  for (int d = 1; d <= 10; ++d) {
    const int m = 10 - d;                      // pd = m-th derivative of c
    double big = 0.0;
    for (int k = 0; k <= d; ++k) {
      double f = c[k + m];
      for (int j = k + 1; j <= k + m; ++j) f *= (double)j;
      pd[k] = f;
    }
    for (int k = 0; k < d; ++k) big = fmax(big, fabs(pd[k] / pd[d]));
    const double R = 1.0 + big;                // Cauchy's bound
    if (!(R < 1e300)) return -1;
    int nc = 0;
    double lo = -R, flo = xk_ess_horner(pd, d, lo);
    for (int s = 0; s <= nprev; ++s) {
      const double hi = s < nprev ? prev[s] : R;
      const double fhi = xk_ess_horner(pd, d, hi);
      if ((flo < 0) != (fhi < 0) && nc < 10) cur[nc++] = xk_ess_bracket_root(pd, d, lo, hi, flo);
      lo = hi; flo = fhi;
    }
    for (int s = 0; s < nc; ++s) prev[s] = cur[s];
    nprev = nc;
  }
  for (int s = 0; s < nprev; ++s) roots[s] = prev[s];
  return nprev;
}

XK_ESS_HD void xk_ess_mat3(const double *A, const double *B, double *C, bool ta, bool tb) {   // C = op(A) op(B)
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += (ta ? A[3 * k + i] : A[3 * i + k]) * (tb ? B[3 * j + k] : B[3 * k + j]);
      C[3 * i + j] = s;
    }
}

// f[10] = (det E, 2 E E^T E - tr(E E^T) E)
XK_ESS_HD void xk_ess_constraints(const double *E, double *f) {
  double T[9], TE[9];
  xk_ess_mat3(E, E, T, false, true);
  xk_ess_mat3(T, E, TE, false, false);
  const double tr = T[0] + T[4] + T[8];
  f[0] = E[0] * (E[4] * E[8] - E[5] * E[7]) - E[1] * (E[3] * E[8] - E[5] * E[6]) + E[2] * (E[3] * E[7] - E[4] * E[6]);
  for (int i = 0; i < 9; ++i) f[1 + i] = 2.0 * TE[i] - tr * E[i];
}

// One Gauss-Newton step on the ten constraints in (x, y, z); Nt[9][4] holds (X, Y, Z, W) entry by entry.
XK_ESS_HD void xk_ess_polish(const double (*Nt)[4], double *xyz) {
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
XK_ESS_HD int xk_ess_solve5(const double (*cur)[2], const double (*rec)[2], double *ws, double *Eout) {
  // 1. null space
  double a[5][9], beta[5], Nt[9][4];
  for (int p = 0; p < 5; ++p) {
    const double r3[3] = {rec[p][0], rec[p][1], 1.0}, c3[3] = {cur[p][0], cur[p][1], 1.0};
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) a[p][3 * i + j] = r3[i] * c3[j];
  }
  for (int k = 0; k < 5; ++k) {
    double s = 0.0;
    for (int t = k; t < 9; ++t) s += a[k][t] * a[k][t];
    const double nrm = sqrt(s);
    beta[k] = 0.0;
    if (!(nrm > 0.0)) continue;
    const double alpha = a[k][k] > 0 ? -nrm : nrm;
    a[k][k] -= alpha;
    double vv = 0.0;
    for (int t = k; t < 9; ++t) vv += a[k][t] * a[k][t];
    beta[k] = 2.0 / vv;
    for (int j = k + 1; j < 5; ++j) {
      double d = 0.0;
      for (int t = k; t < 9; ++t) d += a[k][t] * a[j][t];
      d *= beta[k];
      for (int t = k; t < 9; ++t) a[j][t] -= d * a[k][t];
    }
  }
  for (int v = 0; v < 4; ++v) {
    double q[9];
    for (int t = 0; t < 9; ++t) q[t] = (t == 5 + v) ? 1.0 : 0.0;
    for (int k = 4; k >= 0; --k) {
      double d = 0.0;
      for (int t = k; t < 9; ++t) d += a[k][t] * q[t];
      d *= beta[k];
      for (int t = k; t < 9; ++t) q[t] -= d * a[k][t];
    }
    for (int t = 0; t < 9; ++t) Nt[t][v] = q[t];
  }
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
  const int nr = xk_ess_real_roots(poly, roots);
  if (nr <= 0) return 0;
  // 6., 7.
  for (int s = 0; s < nr; ++s) {
    const double z = roots[s];
    double b[3][3];
    for (int r = 0; r < 3; ++r)
      for (int q = 0; q < 3; ++q) b[r][q] = xk_ess_horner(bz[r][q], 4, z);
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
XK_ESS_HD double xk_ess_sampson(const double *E, double cx, double cy, double rx, double ry) {
  const double c0 = E[0] * cx + E[1] * cy + E[2], c1 = E[3] * cx + E[4] * cy + E[5], c2 = E[6] * cx + E[7] * cy + E[8];
  const double t0 = E[0] * rx + E[3] * ry + E[6], t1 = E[1] * rx + E[4] * ry + E[7];
  const double num = rx * c0 + ry * c1 + c2;
  return num * num / (c0 * c0 + c1 * c1 + t0 * t0 + t1 * t1);
}

struct XkEssArgs {
  const float *cur_xy, *rec_xy;     // [n][2] pixels
  int n, n_hyp;
  double fx, fy, cx, cy, t2;
  unsigned long long seed;
  // scratch block
  double *cand;                     // [XK_ESS_MAX_HYP][10][9]
  double *sum;                      // [XK_ESS_MAX_HYP][10]
  int *cnt;                         // [XK_ESS_MAX_HYP][10]
  int *ncand, *bestc;               // [XK_ESS_MAX_HYP]
  unsigned long long *key;
  // result
  unsigned char *mask;              // [n]
  double *E;                        // [9]
  int *res;                         // n_inliers, winner hypothesis
};

__global__ __launch_bounds__(XK_ESS_SOLVE_T) void xk_ess_solve(XkEssArgs a) {
  __shared__ double ws[XK_ESS_SOLVE_T * XK_ESS_WS];
  const int h = blockIdx.x * XK_ESS_SOLVE_T + threadIdx.x;
  if (h == 0) *a.key = 0ull;
  if (h >= a.n_hyp) return;
  int pick[5];
  xk_ess_sample(a.seed, h, a.n, pick);
  double cur[5][2], rec[5][2];
  for (int k = 0; k < 5; ++k) {
    cur[k][0] = ((double)a.cur_xy[2 * pick[k]] - a.cx) / a.fx; cur[k][1] = ((double)a.cur_xy[2 * pick[k] + 1] - a.cy) / a.fy;
    rec[k][0] = ((double)a.rec_xy[2 * pick[k]] - a.cx) / a.fx; rec[k][1] = ((double)a.rec_xy[2 * pick[k] + 1] - a.cy) / a.fy;
  }
  double *E = a.cand + (size_t)h * (XK_ESS_MAXC * 9);
  const int nc = xk_ess_solve5(cur, rec, ws + threadIdx.x * XK_ESS_WS, E);
  for (int i = nc * 9; i < XK_ESS_MAXC * 9; ++i) E[i] = 0.0;
  a.ncand[h] = nc;
}

__global__ __launch_bounds__(256) void xk_ess_score(XkEssArgs a) {
  __shared__ int s_cnt[4];
  __shared__ double s_sum[4];
  const int h = blockIdx.x, nc = a.ncand[h];
  int best_c = -1, best_cnt = -1;
  double best_sum = 0.0;
  for (int c = 0; c < XK_ESS_MAXC; ++c) {
    int cnt = 0;
    double sum = 0.0;
    if (c < nc) {
      const double *Ep = a.cand + ((size_t)h * XK_ESS_MAXC + c) * 9;
      const double E[9] = {Ep[0], Ep[1], Ep[2], Ep[3], Ep[4], Ep[5], Ep[6], Ep[7], Ep[8]};
      for (int i = threadIdx.x; i < a.n; i += 256) {
        const double d = xk_ess_sampson(E, ((double)a.cur_xy[2 * i] - a.cx) / a.fx, ((double)a.cur_xy[2 * i + 1] - a.cy) / a.fy,
                                        ((double)a.rec_xy[2 * i] - a.cx) / a.fx, ((double)a.rec_xy[2 * i + 1] - a.cy) / a.fy);
        if (d <= a.t2) { ++cnt; sum += d; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { cnt += __shfl_down(cnt, o, 64); sum += __shfl_down(sum, o, 64); }
      if ((threadIdx.x & 63) == 0) { s_cnt[threadIdx.x >> 6] = cnt; s_sum[threadIdx.x >> 6] = sum; }
      __syncthreads();
      cnt = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
      sum = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
      __syncthreads();
      if (cnt > best_cnt || (cnt == best_cnt && sum < best_sum)) { best_cnt = cnt; best_sum = sum; best_c = c; }
    }
    if (threadIdx.x == 0) { a.cnt[h * XK_ESS_MAXC + c] = cnt; a.sum[h * XK_ESS_MAXC + c] = sum; }
  }
  if (threadIdx.x == 0) {
    a.bestc[h] = best_c;
    // count in the high word, inverted hypothesis index in the low word: the maximum is the highest count, then the lowest h
    if (best_c >= 0) atomicMax(a.key, ((unsigned long long)best_cnt << 32) | (unsigned long long)(0xffffffffu - (unsigned int)h));
  }
}

__global__ __launch_bounds__(256) void xk_ess_mask(XkEssArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const unsigned long long key = *a.key;
  if (key == 0ull) {                       // no hypothesis produced a candidate
    if (i < a.n) a.mask[i] = 0;
    if (i < 9) a.E[i] = 0.0;
    if (i == 0) { a.res[0] = 0; a.res[1] = -1; }
    return;
  }
  const int h = (int)(0xffffffffu - (unsigned int)(key & 0xffffffffull));
  const double *Ep = a.cand + ((size_t)h * XK_ESS_MAXC + a.bestc[h]) * 9;
  const double E[9] = {Ep[0], Ep[1], Ep[2], Ep[3], Ep[4], Ep[5], Ep[6], Ep[7], Ep[8]};
  if (i < a.n) {
    const double d = xk_ess_sampson(E, ((double)a.cur_xy[2 * i] - a.cx) / a.fx, ((double)a.cur_xy[2 * i + 1] - a.cy) / a.fy,
                                    ((double)a.rec_xy[2 * i] - a.cx) / a.fx, ((double)a.rec_xy[2 * i + 1] - a.cy) / a.fy);
    a.mask[i] = d <= a.t2 ? 1 : 0;
  }
  if (i < 9) a.E[i] = Ep[i];
  if (i == 0) { a.res[0] = (int)(key >> 32); a.res[1] = h; }
}
