// xk_ciw_round.hip.h -- the searched CI weights of the device-resident CI round (gfx950).
// The round (xk_ci_round_device) needs  M_i^(j) = H_ij P_i^-1 H_ij^T  for every agent i and every shared track j before
// xk_ci_weights can run.  An agent's covariance is the same for all tracks, so it is factored ONCE per round with the rows of
// all tracks as right-hand sides (at most 21 x 8 = 168 columns), and all agents go through the same launches: blockIdx.y (or .z)
// is the agent, the pointers come from a descriptor table in the kernel arguments.
//   xk_ciwr_assemble   [P_i | H_i1^T ... H_iT^T]  per agent, row-major, from the payloads where they lie  (+ the start points)
//   xk_ciwr_chol       xk_chol_whole's schedule (16 x 16 pivot chain, v_mfma_f64_16x16x4_f64 tiles) per 192-row slab, batched
//   xk_ciwr_schur      the Schur complement between two slabs (only for n > 192), batched
//   xk_ciwr_xtx        M_i^(j) = X_ij^T X_ij  for every (track, agent), in the layout xk_ci_weights reads
//   (xk_ci_weights, xk_ciw.hip.h: one workgroup per track)
//   xk_ciwr_finish     S_ci = sum_i T_i / w_i + sigma^2 I  per track with the searched weights, 1 / w_0 for the block scaling, and
//                      the round's results in pinned host memory behind one marker
// fp64 throughout; every element is summed in a fixed order, nothing is accumulated with atomics: the same inputs give the same
// weights bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include "xk_chol16.hip.h"
#include "xk_feature.hip.h"
#include "xk_linalg.hip.h"
#include "xk_ci.hip.h"
#include "xk_ciw.hip.h"

#define XK_CIWR_MAXT 8                                   // shared tracks of a round
#define XK_CIWR_MAXRHS (XK_CIW_MAXM * XK_CIWR_MAXT)      // 168 right-hand sides

// The round's pinned words (xk_handle::h_ci_w, XK_CIP_DOUBLES doubles of host memory the kernels write and the host polls), defined
// here once for xk_ciwr_finish and for the host (xk_ci_api.hip.h: xk_ci_combine's host_gate / host_marker, the waits, the readers).
//   gate words of track j   [0] the own chi-square verdict, [1] the joint gamma, [2] the marker (unsigned long long): xk_ci_combine
//                           with fixed weights, xk_ciwr_finish with searched ones
//   weights of track j      eight doubles, searched rounds only
//   info words              ints, per track [2 j] Newton steps, [2 j + 1] the solver's failure word
//   status words            ints, per agent the pivot status of its factorisation
#define XK_CIP_DOUBLES 128
__host__ __device__ __forceinline__ double *xk_cip_gate(double *w, int j) { return w + 16 + 4 * j; }
__host__ __device__ __forceinline__ unsigned long long *xk_cip_marker(double *w, int j) { return reinterpret_cast<unsigned long long *>(xk_cip_gate(w, j) + 2); }
__host__ __device__ __forceinline__ double *xk_cip_weights(double *w, int j) { return w + 48 + 8 * j; }
__host__ __device__ __forceinline__ int *xk_cip_info(double *w) { return reinterpret_cast<int *>(w + 112); }
__host__ __device__ __forceinline__ int *xk_cip_status(double *w) { return reinterpret_cast<int *>(w + 120); }

// per-agent workspace: Maug_i and X_i, n x ld row-major each, ld = n + 168
struct XkCiwrAgents {
  double *Maug[XK_CIW_MAXK1], *X[XK_CIW_MAXK1];
  int ld;
};

struct XkCiwrAssembleArgs {
  XkCiwrAgents ag;
  const double *P[XK_CIW_MAXK1];      // n x n covariances (column-major, symmetric)
  const double *H[XK_CIWR_MAXT];      // per track: [agent] m x n column-major (ld = m), agents m * n doubles apart
  int n, m, k1, nt;
  double *start;                      // [nt][8] start points of the search, or null (uniform)
  double st[XK_CIW_MAXK1];
  int *status;                        // [8] per-agent pivot status of the round, cleared here
};
// grid (blocks over n * ncols, agents)
__global__ __launch_bounds__(256) void xk_ciwr_assemble(XkCiwrAssembleArgs a) {
  const int i = blockIdx.y, n = a.n, m = a.m, ncols = n + a.nt * m;
  if (blockIdx.x == 0 && i == 0) {
    if (a.start && threadIdx.x < 8 * a.nt) a.start[threadIdx.x] = a.st[threadIdx.x & 7];
    if (threadIdx.x >= 64 && threadIdx.x < 64 + XK_CIW_MAXK1) a.status[threadIdx.x - 64] = 0;
  }
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)n * ncols) return;
  const int r = (int)(idx / ncols), c = (int)(idx % ncols);
  double v;
  if (c < n) v = a.P[i][(size_t)r + (size_t)c * n];
  else {
    const int j = (c - n) / m, q = (c - n) % m;                       // row r of the right-hand sides = column r of H_ij
    v = a.H[j][(size_t)i * m * n + q + (size_t)m * r];
  }
  a.ag.Maug[i][(size_t)r * a.ag.ld + c] = v;
}

// One 192-row slab of every agent's factorisation and solve: workgroup (chunk, agent) runs xk_chol_whole's schedule on
// Maug_i + off * ld + off.  (xk_chol_whole itself is on the measured path of the Kalman stage and stays as it is; this is its
// schedule with the operands taken from the agent table and the status word per agent.)
struct XkCiwrCholArgs {
  XkCiwrAgents ag;
  int off, c, ncols;    // the slab starts at row / column off, is c <= 192 rows deep, and the system has ncols columns behind off
  int *status;          // [agent]: set to 2 if a pivot is not positive
  XkCholWholeTab tab;
};
__global__ __launch_bounds__(64 * XK_CHOLW_WAVES) void xk_ciwr_chol(XkCiwrCholArgs a) {
  constexpr int NW = XK_CHOLW_NW, NS = XK_CHOLW_NS, NT = NS + 2, XR = XK_CHOLW_MAXB;
  __shared__ __attribute__((aligned(16))) double Xs[2][XK_CHOLW_MAXB + 1][256];
  __shared__ __attribute__((aligned(16))) double Ls[2][16 * 17];
  __shared__ __attribute__((aligned(16))) double dbuf[256];
  const int lane = threadIdx.x & 63, hw = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  if (hw == 7) return;
  const int wave = (hw & 3) == 3 ? NW : (hw >> 2) * 3 + (hw & 3);
  const int ag = blockIdx.y, ld = a.ag.ld;
  const double *Maug = a.ag.Maug[ag] + (size_t)a.off * ld + a.off;
  double *X = a.ag.X[ag] + (size_t)a.off * ld + a.off;
  const int nbk = (a.c + 15) / 16;
  if (wave == NW) {
    bool bad = false;
    __syncthreads();
    for (int j = 0; j < nbk; ++j) {
      if (xk_chol16_bcast(dbuf, Ls[j & 1], lane)) bad = true;
      __syncthreads();                                             // barrier 1
      if (j + 1 == nbk) break;
      __syncthreads();                                             // barrier 2
    }
    if (bad && lane == 0) a.status[ag] = 2;                        // (every chunk of the agent finds the same: same value)
    return;
  }
  const int li = lane & 15, lk = lane >> 4;
  int si[NT], sk[NT];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int i = a.tab.i[wave][s], k = a.tab.k[wave][s];
    si[s] = (i == 255) ? -1 : i;
    sk[s] = (i == 255) ? -1 : k;
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    si[NS + u] = (wave + NW * u < nbk) ? wave + NW * u : -1;
    sk[NS + u] = XR;
  }
  const int rcol = a.c + 16 * (int)blockIdx.x + li;
  const bool rc_ok = rcol < a.ncols;
  xk_d4 T[NT];
#pragma unroll
  for (int s = 0; s < NT; ++s) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * si[s] + lk + 4 * r, col = (s < NS) ? 16 * sk[s] + li : rcol;
      double v = 0.0;
      if (si[s] >= 0) {
        if (s < NS) v = (row < a.c && col < a.c) ? Maug[(size_t)row * ld + col] : (row == col ? 1.0 : 0.0);
        else v = (rc_ok && row < a.c) ? Maug[(size_t)row * ld + col] : 0.0;
      }
      T[s][r] = v;
    }
  }
  if (wave == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) dbuf[64 * r + lane] = T[0][r];
  }
  __syncthreads();
  for (int j = 0; j < nbk; ++j) {
    const int par = j & 1;
    __syncthreads();                                               // barrier 1: Ls[par] = L_jj^-1
    double lv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) lv[q] = Ls[par][li * 17 + 4 * q + lk];
#pragma unroll
    for (int s = 2; s < NT; ++s) {
      if (si[s] == j) {
        xk_d4 x = {0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < 4; ++q) x = __builtin_amdgcn_mfma_f64_16x16x4f64(lv[q], T[s][q], x, 0, 0, 0);
        if (s == 2 || s == 3) {
#pragma unroll
          for (int q = 0; q < 4; ++q) T[s - 2] = __builtin_amdgcn_mfma_f64_16x16x4f64(-x[q], x[q], T[s - 2], 0, 0, 0);
#pragma unroll
          for (int r = 0; r < 4; ++r) dbuf[64 * r + lane] = T[s - 2][r];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) Xs[par][sk[s]][64 * r + lane] = x[r];
        if (s >= NS) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 16 * j + lk + 4 * r;
            if (rc_ok && row < a.c) X[(size_t)row * ld + rcol] = x[r];
          }
        }
      }
    }
    if (j + 1 == nbk) break;
    __syncthreads();                                               // barrier 2: Xs[par], dbuf
#pragma unroll
    for (int s = 0; s < NT; ++s) {
      if (si[s] > j && !(si[s] == j + 1 && sk[s] == j + 1)) {
        const double *xi = &Xs[par][si[s]][lane], *xk = &Xs[par][sk[s]][lane];
#pragma unroll
        for (int q = 0; q < 4; ++q) T[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(-xi[64 * q], xk[64 * q], T[s], 0, 0, 0);
      }
    }
  }
}

// acc += Xa^T Xb over rows [k0, k1) of a row-major X (ld), Xa / Xb = 16 columns from ca / cb on; columns at or beyond ncol read as
// zero.  One wave; the result is in the MFMA C/D layout: acc[r] = element (lk + 4 r, li).  Rows are taken four at a time in
// ascending order: the order of every sum is fixed.
__device__ __forceinline__ xk_d4 xk_ciwr_xtx_tile(const double *X, int ld, int k0, int k1, int ca, int cb, int ncol, int lane, xk_d4 acc) {
  const int li = lane & 15, lk = lane >> 4;
  const bool a_ok = ca + li < ncol, b_ok = cb + li < ncol;
  const double *pa = X + ca + li, *pb = X + cb + li;
  for (int k = k0; k < k1; k += 16) {
    double va[4], vb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {                                   // four steps' operands in flight
      const int row = k + 4 * u + lk;
      va[u] = (a_ok && row < k1) ? pa[(size_t)row * ld] : 0.0;
      vb[u] = (b_ok && row < k1) ? pb[(size_t)row * ld] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(va[u], vb[u], acc, 0, 0, 0);
  }
  return acc;
}

// Schur complement between two slabs: Maug[off + r][off + c] -= sum_k X[off - cb + k][off + r] X[off - cb + k][off + c] for the
// tiles at or right of the diagonal tile (the factorisation reads whole diagonal tiles and nothing left of them).
// grid (column tiles, row tiles, agents), one wave per 16 x 16 tile.
struct XkCiwrSchurArgs {
  XkCiwrAgents ag;
  int off, cb;          // the slab just solved: rows [off - cb, off)
  int M, N;             // rows and columns of the trailing system behind off
};
__global__ __launch_bounds__(64) void xk_ciwr_schur(XkCiwrSchurArgs a) {
  const int tj = blockIdx.x, ti = blockIdx.y, ag = blockIdx.z, lane = threadIdx.x, ld = a.ag.ld;
  if (tj < ti) return;
  const double *Xs = a.ag.X[ag] + (size_t)(a.off - a.cb) * ld + a.off;
  double *C = a.ag.Maug[ag] + (size_t)a.off * ld + a.off;
  xk_d4 acc = {0, 0, 0, 0};
  acc = xk_ciwr_xtx_tile(Xs, ld, 0, a.cb, 16 * ti, 16 * tj, a.N, lane, acc);
  const int li = lane & 15, lk = lane >> 4, col = 16 * tj + li;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 16 * ti + lk + 4 * r;
    if (row < a.M && col < a.N) C[(size_t)row * ld + col] -= acc[r];
  }
}

// M_i^(j) = X_ij^T X_ij, X_ij = columns [n + j m, n + (j + 1) m) of X_i (n rows).  grid (tracks, agents), four waves: each takes a
// quarter of the rows for every 16 x 16 tile of the m x m result; the four partial sums are added in wave order.
struct XkCiwrXtxArgs {
  XkCiwrAgents ag;
  int n, m;
  double *M;            // out [track][8 agents][576], m x m (ld = m)
};
__global__ __launch_bounds__(256) void xk_ciwr_xtx(XkCiwrXtxArgs a) {
  __shared__ double part[4][4][256];     // [wave][tile][C/D layout]
  const int j = blockIdx.x, ag = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = a.n, m = a.m, ld = a.ag.ld, c0 = n + j * m, nt = (m + 15) / 16;
  const int kq = (((n + 3) / 4 + 3) / 4) * 4;                        // rows per wave, a multiple of four
  const int k0 = min(wave * kq, n), k1 = min(k0 + kq, n);
  for (int t = 0; t < nt * nt; ++t) {
    xk_d4 acc = {0, 0, 0, 0};
    acc = xk_ciwr_xtx_tile(a.ag.X[ag], ld, k0, k1, c0 + 16 * (t / nt), c0 + 16 * (t % nt), c0 + m, lane, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) part[wave][t][64 * r + lane] = acc[r];
  }
  __syncthreads();
  double *Mo = a.M + ((size_t)j * XK_CIW_MAXK1 + ag) * 576;
  for (int e = threadIdx.x; e < nt * nt * 256; e += 256) {
    const int t = e >> 8, x = e & 255, r = x >> 6, ln = x & 63;
    const int row = 16 * (t / nt) + (ln >> 4) + 4 * r, col = 16 * (t % nt) + (ln & 15);
    if (row < m && col < m) Mo[row + m * col] = ((part[0][t][x] + part[1][t][x]) + part[2][t][x]) + part[3][t][x];
  }
}

// The end of the searched chain, one workgroup: per track the CI-weighted innovation covariance with the searched weights
//   S_ci = sum_i T_i / w_i + sigma^2 I,   T_i = H_i P_i H_i^T (the chunk partials of xk_ci_hph, added as xk_ci_combine adds them)
// and 1 / w_0 for the scaling of the own pose blocks; then everything the host decides on goes to pinned memory -- gate words,
// weights, the solver's info words, the per-agent pivot status -- and the markers behind it (system-scope release).
struct XkCiwrFinishArgs {
  int nt, k1, m, nchunk;
  double var_img;
  const double *Si[XK_CIWR_MAXT];       // per track: [k1][XK_CI_MAXCHUNK][576]
  double *S_ci[XK_CIWR_MAXT];           // per track: m x m
  const int *own_inlier[XK_CIWR_MAXT];  // per track: the own chi-square verdict
  const double *gamma[XK_CIWR_MAXT];    // per track: the joint gamma
  const double *w;                      // [track][8] searched weights
  const int *info;                      // [track][2]
  const int *status;                    // [8] per-agent pivot status
  double *winv;                         // out [track]: 1 / w_0
  double *host;                         // pinned: h_ci_w, the XK_CIP words above
  unsigned long long seq;
};
__global__ __launch_bounds__(512) void xk_ciwr_finish(XkCiwrFinishArgs a) {
  const int m = a.m, t = threadIdx.x;
  for (int j = 0; j < a.nt; ++j) {
    const double *w = a.w + 8 * j;
    for (int e = t; e < m * m; e += 512) {
      double c = 0.0;
      for (int i = 0; i < a.k1; ++i) {
        double part[XK_CI_MAXCHUNK];
#pragma unroll
        for (int cb = 0; cb < XK_CI_MAXCHUNK; ++cb) part[cb] = (cb < a.nchunk) ? a.Si[j][((size_t)i * XK_CI_MAXCHUNK + cb) * 576 + e] : 0.0;
        double v = 0.0;
#pragma unroll
        for (int cb = 0; cb < XK_CI_MAXCHUNK; ++cb)
          if (cb < a.nchunk) v += part[cb];
        c = __dadd_rn(c, __dmul_rn(1.0 / w[i], v));
      }
      if (e % m == e / m) c = __dadd_rn(c, a.var_img);
      a.S_ci[j][e] = c;
    }
  }
  if (t < a.nt) a.winv[t] = 1.0 / a.w[8 * t];
  if (t < 8 * a.nt) __hip_atomic_store(xk_cip_weights(a.host, 0) + t, a.w[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (t < 2 * a.nt) __hip_atomic_store(xk_cip_info(a.host) + t, a.info[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (t < 8) __hip_atomic_store(xk_cip_status(a.host) + t, a.status[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (t < a.nt) {
    __hip_atomic_store(xk_cip_gate(a.host, t), (double)*a.own_inlier[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(xk_cip_gate(a.host, t) + 1, *a.gamma[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  __threadfence_system();
  __syncthreads();
  if (t < a.nt) __hip_atomic_store(xk_cip_marker(a.host, t), a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
