// xk_ciw.hip.h -- the covariance-intersection weight search (gfx950).
//   CovarianceIntersection::solveW   src/x/ekf/ci.cpp:143-190 (called from :65-73 and :105-119 for negative weights)
// The reference hands  det((sum_i w_i M_i)^-1),  M_i = H_i P_i^-1 H_i^T,  1e-4 <= w_i <= 1,  sum w = 1  to NLopt's COBYLA
// with a wall-time limit.  f(w) = -log det A(w), A = sum w_i M_i, has the same minimiser and is convex, so it is found here
// by an active-set Newton iteration: a handful of steps, no time limit, the same bits on every call.
//   g_i  = tr(A^-1 M_i)            = tr Y_i,         Y_i = L^-1 M_i L^-T,  A = L L^T
//   H_ij = tr(A^-1 M_i A^-1 M_j)   = <Y_i, Y_j>_F
// sum_i w_i g_i = m at every w, so with no bound active the multiplier of sum w = 1 is m.  The upper bound never binds
// (k1 >= 2 weights of at least 1e-4 that sum to one).  det itself is never formed: it leaves the fp64 range for small
// covariances; only the Cholesky pivots of A are looked at.
#pragma once
#include <hip/hip_runtime.h>

#define XK_CIW_MAXK1 8
#define XK_CIW_MAXM 21
#define XK_CIW_MM (XK_CIW_MAXM * XK_CIW_MAXM)
#define XK_CIW_LB 1e-4
#define XK_CIW_TOL 1e-10
#define XK_CIW_MAXIT 50
#define XK_CIW_THREADS 256
#define XK_CIW_WS (24 + 2 * XK_CIW_MAXK1 * 576)   // doubles: weights, start, info words, then M_i and H_i P_i H_i^T (24 x 24 slots)

struct XkCiwArgs {
  const double *M;    // [problem][k1] symmetric m x m matrices (ld = m)
  long pstride;       // doubles between two problems
  int mstride;        // doubles between two matrices of a problem
  int m, k1;
  const double *w0;   // [problem][8] feasible start (device), or null = uniform
  double *w;          // out [problem][8]
  int *info;          // out [problem][2]: Newton steps taken, status (0, or 2 = A not positive definite / no convergence)
  int *status;        // optional status word of the handle: set to 2 when a problem fails, never cleared here
  // precise != 0 (the device CI round): the result must not depend on the start beyond rounding, also for M_i that are rank-deficient
  // inside the m x m block (sum_i M_i with a condition number of 1e7).  Two things, both exact in exact arithmetic:
  //   - the problem is whitened first, M_i <- L0^-1 M_i L0^-T with sum_i M_i / k1 = L0 L0^T: the objective changes by a constant, the
  //     iteration then works on matrices whose uniform sum is the identity (the gradient's rounding error scales with cond(A));
  //   - once the convergence test passes after at least one step, ONE more Newton step is taken: the test allows a gradient residual
  //     of 1e-10 lam, i.e. weights a few 1e-11 from the minimiser depending on where the iteration came from; the step squares that.
  int precise;
};

// One workgroup per problem.  Every sum runs in a fixed order (no atomics, no order that depends on timing).
__global__ __launch_bounds__(XK_CIW_THREADS) void xk_ci_weights(XkCiwArgs a) {
  __shared__ double Ms[XK_CIW_MAXK1 * XK_CIW_MM], Ys[XK_CIW_MAXK1 * XK_CIW_MM];
  __shared__ double As[XK_CIW_MAXM][XK_CIW_MAXM + 1];
  __shared__ double part[44 * 4];                                  // 36 pairs i <= j, then 8 traces; four partial sums each
  __shared__ double Hs[XK_CIW_MAXK1][XK_CIW_MAXK1], gs[XK_CIW_MAXK1], ws[XK_CIW_MAXK1], ds[XK_CIW_MAXK1];
  __shared__ int act[XK_CIW_MAXK1], ctl[2];                        // ctl[0]: 0 go on, 1 converged, 2 failed; ctl[1]: steps taken
  const int tid = threadIdx.x, m = a.m, k1 = a.k1, mm = m * m;
  const double *Mp = a.M + (long)blockIdx.x * a.pstride;
  for (int e = tid; e < k1 * mm; e += XK_CIW_THREADS) Ms[(e / mm) * XK_CIW_MM + e % mm] = Mp[(long)(e / mm) * a.mstride + e % mm];
  if (tid == 0) {
    double rest = 0.0;
    for (int i = k1 - 1; i >= 0; --i) {
      ws[i] = a.w0 ? a.w0[8 * (long)blockIdx.x + i] : (i ? 1.0 / k1 : 1.0 - rest);
      rest += ws[i];
      act[i] = ws[i] <= XK_CIW_LB;
    }
    ctl[0] = ctl[1] = 0;
  }
  __syncthreads();
  bool whiten = a.precise != 0, polished = false;   // (whiten: uniform over the workgroup; polished: thread 0's)
  for (;;) {
    // A = sum_i w_i M_i  (whitening pass: the uniform sum)
    for (int e = tid; e < mm; e += XK_CIW_THREADS) {
      double s = 0.0;
      for (int i = 0; i < k1; ++i) s = fma(whiten ? 1.0 / k1 : ws[i], Ms[i * XK_CIW_MM + e], s);
      As[e % m][e / m] = s;
    }
    __syncthreads();
    // A = L L^T, right-looking, lane r of wave 0 owns row r (L in the lower triangle of As)
    if (tid < 64) {
      auto wsync = [] { __builtin_amdgcn_s_waitcnt(0xc07f); __builtin_amdgcn_wave_barrier(); };
      bool bad = false;
      for (int k = 0; k < m; ++k) {
        const double p = As[k][k];
        if (!(p > 0.0)) bad = true;
        const double d = sqrt(p);
        wsync();
        if (tid == k) As[k][k] = d;
        if (tid > k && tid < m) As[tid][k] = As[tid][k] / d;
        wsync();
        if (tid > k && tid < m)
          for (int j = k + 1; j <= tid; ++j) As[tid][j] = fma(-As[tid][k], As[j][k], As[tid][j]);
        wsync();
      }
      if (bad && tid == 0) ctl[0] = 2;
    }
    __syncthreads();
    if (ctl[0]) break;
    // Z_i = L^-1 M_i: one thread per column (i, c)
    for (int t = tid; t < k1 * m; t += XK_CIW_THREADS) {
      const int i = t / m, c = t % m;
      const double *Mi = Ms + i * XK_CIW_MM + m * c;
      double *Y = Ys + i * XK_CIW_MM + m * c;
      for (int r = 0; r < m; ++r) {
        double s = Mi[r];
        for (int q = 0; q < r; ++q) s = fma(-As[r][q], Y[q], s);
        Y[r] = s / As[r][r];
      }
    }
    __syncthreads();
    // Y_i = Z_i L^-T: one thread per row (i, r)
    for (int t = tid; t < k1 * m; t += XK_CIW_THREADS) {
      const int i = t / m, r = t % m;
      double *Y = Ys + i * XK_CIW_MM + r;
      for (int c = 0; c < m; ++c) {
        double s = Y[m * c];
        for (int q = 0; q < c; ++q) s = fma(-As[c][q], Y[m * q], s);
        Y[m * c] = s / As[c][c];
      }
    }
    __syncthreads();
    if (whiten) {                                                   // M_i <- L0^-1 M_i L0^-T (symmetric part), then the iteration proper
      for (int t = tid; t < k1 * mm; t += XK_CIW_THREADS) {
        const int i = t / mm, e = t % mm, r = e % m, c = e / m;
        Ms[i * XK_CIW_MM + e] = 0.5 * (Ys[i * XK_CIW_MM + r + m * c] + Ys[i * XK_CIW_MM + c + m * r]);
      }
      whiten = false;
      __syncthreads();
      continue;
    }
    // H_ij = <Y_i, Y_j>, g_i = tr Y_i: four interleaved partial sums per value, added in their order below
    if (tid < 44 * 4) {
      const int p = tid >> 2, q = tid & 3;
      double s = 0.0;
      if (p < 36) {
        int i = 0, rest = p;
        while (rest >= XK_CIW_MAXK1 - i) { rest -= XK_CIW_MAXK1 - i; ++i; }
        const int j = i + rest;
        if (j < k1) {
          const double *Yi = Ys + i * XK_CIW_MM, *Yj = Ys + j * XK_CIW_MM;
          for (int e = q; e < mm; e += 4) s = fma(Yi[e], Yj[e], s);
        }
      } else if (p - 36 < k1) {
        const double *Yi = Ys + (p - 36) * XK_CIW_MM;
        for (int r = q; r < m; r += 4) s += Yi[r + m * r];
      }
      part[tid] = s;
    }
    __syncthreads();
    if (tid < 44) {
      const double v = ((part[4 * tid] + part[4 * tid + 1]) + part[4 * tid + 2]) + part[4 * tid + 3];
      if (tid < 36) {
        int i = 0, rest = tid;
        while (rest >= XK_CIW_MAXK1 - i) { rest -= XK_CIW_MAXK1 - i; ++i; }
        Hs[i][i + rest] = v;
        Hs[i + rest][i] = v;
      } else gs[tid - 36] = v;
    }
    __syncthreads();
    if (tid == 0) {
      // lam: the multiplier of sum w = 1 on the free coordinates (= m while no bound is active)
      auto multiplier = [&] {
        double sw = 0.0, sg = 0.0;
        for (int i = 0; i < k1; ++i)
          if (!act[i]) { sw += ws[i]; sg = fma(ws[i], gs[i], sg); }
        return sg / sw;
      };
      double lam = multiplier();
      bool released = false;
      for (int i = 0; i < k1; ++i)
        if (act[i] && gs[i] > lam * (1.0 + XK_CIW_TOL)) { act[i] = 0; released = true; }
      if (released) lam = multiplier();
      double worst = 0.0;
      for (int i = 0; i < k1; ++i)
        if (!act[i]) worst = fmax(worst, fabs(gs[i] - lam));
      const bool conv = worst <= XK_CIW_TOL * lam;
      const bool polish = conv && a.precise && !polished && ctl[1] > 0 && ctl[1] < XK_CIW_MAXIT;
      if (conv && !polish) ctl[0] = 1;                             // (tested BEFORE the step: a flat objective returns its start)
      else if (ctl[1] >= XK_CIW_MAXIT) ctl[0] = 2;
      else {
        if (polish) polished = true;
        // Newton step on the free coordinates with sum d = 0: the constraint is eliminated through the largest free weight r
        // (d_r = -sum of the others), the reduced system <Y_i - Y_r, Y_j - Y_r> d = g_i - g_r is solved by Cholesky.  A free
        // coordinate that sits on the bound and would leave the feasible set goes back into the active set, and the step is redone.
        for (int again = 1; again;) {
          again = 0;
          int r = -1, idx[XK_CIW_MAXK1], nf = 0;
          for (int i = 0; i < k1; ++i)
            if (!act[i] && (r < 0 || ws[i] > ws[r])) r = i;
          if (r < 0) { ctl[0] = 2; break; }                        // (cannot happen for a feasible start: the largest weight is free)
          for (int i = 0; i < k1; ++i) {
            ds[i] = 0.0;
            if (!act[i] && i != r) idx[nf++] = i;
          }
          double R[XK_CIW_MAXK1][XK_CIW_MAXK1], y[XK_CIW_MAXK1], scale = 0.0;
          for (int x = 0; x < nf; ++x) {
            for (int z = 0; z <= x; ++z) R[x][z] = (Hs[idx[x]][idx[z]] - Hs[idx[x]][r]) - (Hs[r][idx[z]] - Hs[r][r]);
            y[x] = gs[idx[x]] - gs[r];
            scale = fmax(scale, R[x][x]);
          }
          bool skip[XK_CIW_MAXK1];
          for (int x = 0; x < nf; ++x) {                           // R = C C^T; a direction the objective is flat along gets no step
            for (int z = 0; z <= x; ++z) {
              double s = R[x][z];
              for (int q = 0; q < z; ++q) s -= R[x][q] * R[z][q];
              if (z < x) R[x][z] = skip[z] ? 0.0 : s / R[z][z];
              else { skip[x] = !(s > 1e-14 * scale); R[x][x] = skip[x] ? 1.0 : sqrt(s); }
            }
          }
          for (int x = 0; x < nf; ++x) {
            double s = y[x];
            for (int q = 0; q < x; ++q) s -= R[x][q] * y[q];
            y[x] = skip[x] ? 0.0 : s / R[x][x];
          }
          double dr = 0.0;
          for (int x = nf - 1; x >= 0; --x) {
            double s = y[x];
            for (int q = x + 1; q < nf; ++q) s -= R[q][x] * y[q];
            y[x] = skip[x] ? 0.0 : s / R[x][x];
          }
          for (int x = 0; x < nf; ++x) { ds[idx[x]] = y[x]; dr -= y[x]; }
          ds[r] = dr;
          for (int i = 0; i < k1; ++i)
            if (!act[i] && ws[i] <= XK_CIW_LB && ds[i] < 0.0) { act[i] = 1; again = 1; }
        }
        // the step, cut at the nearest bound; whoever reaches it joins the active set
        double alpha = 1.0;
        for (int i = 0; i < k1; ++i)
          if (!act[i] && ds[i] < 0.0) alpha = fmin(alpha, (ws[i] - XK_CIW_LB) / -ds[i]);
        int r = -1;
        for (int i = 0; i < k1 && ctl[0] == 0; ++i) {
          if (act[i]) continue;
          ws[i] = fmax(fma(alpha, ds[i], ws[i]), XK_CIW_LB);
          if (ws[i] <= XK_CIW_LB) act[i] = 1;
          if (r < 0 || ws[i] > ws[r]) r = i;
        }
        if (r >= 0) {
          double rest = 0.0;                                       // sum w = 1 is restored on the largest free weight
          for (int i = 0; i < k1; ++i)
            if (i != r) rest += ws[i];
          ws[r] = 1.0 - rest;
          ctl[1]++;
        }
      }
    }
    __syncthreads();
    if (ctl[0]) break;
  }
  if (tid == 0) {
    for (int i = 0; i < 8; ++i) a.w[8 * (long)blockIdx.x + i] = i < k1 ? ws[i] : 0.0;
    a.info[2 * blockIdx.x] = ctl[1];
    a.info[2 * blockIdx.x + 1] = ctl[0] == 1 ? 0 : 2;
    if (ctl[0] != 1 && a.status) *a.status = 2;
  }
}

// The consumers of the weights.  A CI entry keeps its weights in eight device doubles -- written from the host's constants
// (fixed weights) or by xk_ci_weights (searched) -- and everything after that reads them from there.
struct XkCiwSetArgs {
  double *w;
  double v[XK_CIW_MAXK1];
};
__global__ void xk_ciw_set(XkCiwSetArgs a) {
  if (threadIdx.x < XK_CIW_MAXK1) a.w[threadIdx.x] = a.v[threadIdx.x];
}

// S (+)= T / w[i]  (+ diag on the diagonal): the weighted sums of ci.cpp:78-85 and :120-122, one agent per launch in the
// caller's order.  Each product and each sum is rounded on its own (what the GEMM epilogue with a host-side alpha did).
// pair != 0: the pairwise form, whose own weight is 1 - w[1].  w_result (optional) receives the factor of agent 0.
struct XkCiwSumArgs {
  const double *T;
  double *S;
  int m, first, i, pair, add_diag;
  double diag;
  const double *w;
  double *w_result;
};
__global__ void xk_ciw_sum(XkCiwSumArgs a) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const double wi = (a.pair && a.i == 0) ? 1.0 - a.w[1] : a.w[a.i];
  if (e == 0 && a.w_result) *a.w_result = 1.0 / ((a.pair) ? 1.0 - a.w[1] : a.w[0]);
  if (e >= a.m * a.m) return;
  double v = __dmul_rn(1.0 / wi, a.T[e]);
  if (!a.first) v = __dadd_rn(v, a.S[e]);
  if (a.add_diag && e % a.m == e / a.m) v = __dadd_rn(v, a.diag);
  a.S[e] = v;
}
