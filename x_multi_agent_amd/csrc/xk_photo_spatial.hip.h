// xk_photo_spatial.hip.h -- the spatial photometric map params_PS_ estimated on the device (gfx950).
//
//   IRPhotoCalib::ProcessCurrentFrame, the spatial part: correspondences between grid cells, per frame   (irPhotoCalib.cpp:162-210)
//   IRPhotoCalib::EstimateSpatialParameters: sparse least squares, Gaussian-process smoothing, upsample   (irPhotoCalib.cpp:314-420)
//
// The algorithm is this project's own statement of those calls (the comment in include/xk.h), restated in NumPy by
// tests/photo_spatial_np.py.  What is bit-defined: the row list (sid_hist, sid_cur, b) in point order, the counts, the coverage,
// the numbering (covered cells in ascending cell id), L = A^T A (exact integers) and c = A^T b (every entry summed in ascending
// row order).  Both solves are the same Jacobi-preconditioned conjugate gradients in fp64 with sums in an order fixed by n alone:
// two runs on the same rows give the same bytes.  No floating-point atomics, no inline assembly.
//
//   xk_photo_sp_accumulate  ONE wavefront per call, the counts in LDS (up to XK_PSP_LDS_CELLS cells; in global memory beyond): points
//                           64 at a time.  If no lane's count[sh] + 128 exceeds max_count (a chunk adds at most 64 to a cell) the chunk
//                           is decided in parallel and the counts move by LDS integer atomics; otherwise the chunk is walked point by
//                           point, uniformly by all lanes, with the sequential rule.  Row slots come from a ballot prefix either way
//   xk_photo_sp_number      one workgroup: an ordered scan of the coverage bytes -> var_of_cell, cell_of_var, n
//   xk_photo_sp_clear       the int32 multiplicities and degrees back to zero (n x n of them)
//   xk_photo_sp_count       one thread per row: integer atomicAdd of the two off-diagonal multiplicities and the two degrees
//   xk_photo_sp_normal      one wavefront per variable: row v of L in fp64 (degree on the diagonal, -multiplicity beside it) and
//                           c[v], its terms picked from the row list in ascending row order (ballot, then the set lanes in order)
//   xk_photo_sp_kernel      K_ij = sf^2 exp(-d^2 / (2 l^2)) + sn^2 [i = j] from cell_of_var
//   xk_photo_sp_pcg_init    one workgroup: x = 0, r = rhs, p = z = r / diag, r.z, |rhs|^2, the cap, the done flag
//   xk_photo_sp_matvec      one matrix row per wavefront, XK_PSP_MV_ROWS rows per workgroup: q = A p and one partial p.q per workgroup
//   xk_photo_sp_step        one workgroup: the partials in slot order, x, r, z, p, r.z, the iteration count, the done flag
//   xk_photo_sp_predict     one wavefront per grid cell: the GP mean (float), then that cell's pixels of the upsampled map
// Every launch behind xk_photo_sp_number reads n from the device; every solver kernel looks at the done flag first.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "xk_photo.hip.h"

#define XK_PSP_NMAX 2048           // unknowns a setup holds at most: two dense n x n fp64 matrices
#define XK_PSP_LDS_CELLS 8192      // counts kept in LDS up to here (32 KB)
#define XK_PSP_MV_ROWS 4           // rows per workgroup of xk_photo_sp_matvec: one per wavefront
#define XK_PSP_T 256
#define XK_PSP_TOL 1.0e-13

enum { XK_PSP_ACCUMULATING = 0, XK_PSP_ESTIMATED = 1, XK_PSP_FAILED = 2 };

// One solve's record on the device
struct XkPspSolve {
  double rz, bb, rr, thr;          // r.z, |rhs|^2, |r|^2 of the last iteration, tol^2 |rhs|^2
  int it, done, converged, cap;
};

// What lives on the device between calls and is copied to the pinned block whole
struct XkPspState {
  XkPspSolve ls, gp;
  int rows, dropped, covered, ready;
  int n, pad[3];
};

struct XkPspGrid {
  int w, h, div, cw, ch, cells;
};

struct XkPspAccArgs {
  XkPspGrid g;
  int max_count, max_rows;
  double thr;                      // (double)(float)coverage_thr
  // the points: pixels as ints [n][2], or (per-frame call) the previous points as floats indexed through keep_idx
  const int *pix_hist, *pix_cur;
  const float *prev_f;             // NULL, or [.][2]: the history pixel of point j is the truncation of prev_f[keep_idx[j]]
  const int *keep_idx;
  const double *o_hist, *o_cur;
  const int *off, *frame_back;     // [G + 1], [G]
  int G;
  const XkPhotoState *ring;
  int per_frame;                   // 1: nothing happens unless the state says the frame estimated gains
  int *count;                      // [cells]
  unsigned char *coverage;         // [cells], padded to a multiple of 4 zero bytes
  int *sid_hist, *sid_cur;         // [max_rows]
  double *b;
  XkPspState *st;
};

__device__ __forceinline__ int xk_psp_cell(const XkPspGrid &g, int x, int y) {
  // -1: outside the image, or in the remainder column / row that the reference aliases into a neighbour's id
  if (x < 0 || y < 0 || x >= g.w || y >= g.h) return -1;
  const int cx = x / g.div, cy = y / g.div;
  if (cx >= g.cw || cy >= g.ch) return -1;
  return cy * g.cw + cx;
}

__global__ __launch_bounds__(64) void xk_photo_sp_accumulate(XkPspAccArgs a) {
#pragma clang fp contract(off)
  __shared__ int s_cnt[XK_PSP_LDS_CELLS];
  const int lane = threadIdx.x;
  if (a.per_frame && !a.ring->estimated) return;
  const int cells = a.g.cells;
  const bool lds = cells <= XK_PSP_LDS_CELLS;
  int *cnt = lds ? s_cnt : a.count;
  if (lds) {
    for (int i = lane; i < cells; i += 64) s_cnt[i] = a.count[i];
  }
  __syncthreads();
  int rows = a.st->rows, dropped = a.st->dropped;
  const int last = a.ring->ring_n - 1;
  for (int g = 0; g < a.G; ++g) {
    const int first = a.off[g], m = a.off[g + 1] - first;
    const int at = last - a.frame_back[g];
    double a_hc = 1.0, b_hc = 0.0;
    if (at >= 0)   // (the host checked; a per-frame call always has at >= 0: the ring has just grown)
      xk_photo_relative(a.ring->ring[2 * at], a.ring->ring[2 * at + 1], a.ring->ring[2 * last], a.ring->ring[2 * last + 1], &a_hc, &b_hc);
    const double gain = a_hc - b_hc;
    for (int c0 = 0; c0 < m; c0 += 64) {
      const int j = first + c0 + lane;
      const bool in = c0 + lane < m;
      int sh = -1, sc = -1;
      double bv = 0.0;
      if (in) {
        int hx, hy;
        if (a.prev_f) {
          const int k = a.keep_idx[j];
          hx = (int)a.prev_f[2 * k]; hy = (int)a.prev_f[2 * k + 1];
        } else {
          hx = a.pix_hist[2 * j]; hy = a.pix_hist[2 * j + 1];
        }
        sh = xk_psp_cell(a.g, hx, hy);
        sc = xk_psp_cell(a.g, a.pix_cur[2 * j], a.pix_cur[2 * j + 1]);
        bv = (a.o_cur[j] * gain - a.o_hist[j]) + b_hc;
      }
      const bool cand = sh >= 0 && sc >= 0 && sh != sc;
      const bool near_cap = cand && cnt[sh] + 128 > a.max_count;
      bool take = cand;
      if (__ballot(near_cap) == 0ull) {
        if (cand) { atomicAdd(&cnt[sh], 1); atomicAdd(&cnt[sc], 1); }
      } else {
        // the sequential rule, point by point; every lane does the same reads and the same stores
        const unsigned long long cm = __ballot(cand);
        unsigned long long tm = 0ull;
        for (int l = 0; l < 64; ++l) {
          const int h = __shfl(sh, l, 64), c = __shfl(sc, l, 64);
          if (!((cm >> l) & 1ull)) continue;
          const int ch = cnt[h];
          if (ch > a.max_count) continue;
          tm |= 1ull << l;
          cnt[h] = ch + 1;
          cnt[c] = cnt[c] + 1;
        }
        take = (tm >> lane) & 1ull;
      }
      const unsigned long long tk = __ballot(take);
      if (take) {
        a.coverage[sh] = 1; a.coverage[sc] = 1;
        const int slot = rows + __popcll(tk & ((1ull << lane) - 1ull));
        if (slot < a.max_rows) { a.sid_hist[slot] = sh; a.sid_cur[slot] = sc; a.b[slot] = bv; }
      }
      const int taken = __popcll(tk), room = max(a.max_rows - rows, 0);
      rows += min(taken, room);
      dropped += taken - min(taken, room);
      __syncthreads();
    }
  }
  if (lds) {
    for (int i = lane; i < cells; i += 64) a.count[i] = s_cnt[i];
  }
  __syncthreads();                                               // (this wavefront's coverage bytes are written)
  int cov = 0;
  const unsigned int *cw4 = reinterpret_cast<const unsigned int *>(a.coverage);
  for (int i = lane; i < (cells + 3) / 4; i += 64) cov += __popc(cw4[i] & 0x01010101u);
  const int covered = (int)xk_klt_wave_sum(cov);
  if (lane == 0) {
    a.st->rows = rows; a.st->dropped = dropped; a.st->covered = covered;
    a.st->ready = ((double)covered / (double)cells > a.thr) ? 1 : 0;
  }
}

// ---- numbering ----
struct XkPspNumArgs {
  const unsigned char *coverage;
  int cells, n_max;
  int *var_of_cell, *cell_of_var;
  XkPspState *st;
};

__global__ __launch_bounds__(XK_PSP_T) void xk_photo_sp_number(XkPspNumArgs a) {
  __shared__ int s_w[XK_PSP_T / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int base = 0;
  for (int c0 = 0; c0 < a.cells; c0 += XK_PSP_T) {
    const int cell = c0 + threadIdx.x;
    const bool on = cell < a.cells && a.coverage[cell] != 0;
    const unsigned long long m = __ballot(on);
    if (lane == 0) s_w[wv] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < XK_PSP_T / 64; ++k) { before += k < wv ? s_w[k] : 0; total += s_w[k]; }
    const int v = base + before + __popcll(m & ((1ull << lane) - 1ull));
    if (cell < a.cells) a.var_of_cell[cell] = on ? v : -1;
    if (on && v < a.n_max) a.cell_of_var[v] = cell;
    base += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) a.st->n = base;                          // (may exceed n_max: the host refuses, the launches behind clamp)
}

// ---- the normal equations ----
struct XkPspNormArgs {
  const int *sid_hist, *sid_cur;
  const double *b;
  const int *var_of_cell;
  int *mult;                       // [n][ld] int32, aliased with the second fp64 matrix (it is filled after these are read)
  int *deg;                        // [n]
  double *L, *c, *diag;            // [n][ld], [n], [n]
  int ld, n_max, max_rows;
  const XkPspState *st;
};

__device__ __forceinline__ int xk_psp_n(const XkPspState *st, int n_max) { return min(st->n, n_max); }

__global__ __launch_bounds__(XK_PSP_T) void xk_photo_sp_clear(XkPspNormArgs a) {
  const int n = xk_psp_n(a.st, a.n_max), i = blockIdx.x;
  if (i >= n) return;
  for (int j = threadIdx.x; j < n; j += XK_PSP_T) a.mult[(size_t)i * a.ld + j] = 0;
  if (threadIdx.x == 0) a.deg[i] = 0;
}

__global__ __launch_bounds__(XK_PSP_T) void xk_photo_sp_count(XkPspNormArgs a) {
  const int rows = min(a.st->rows, a.max_rows), n = xk_psp_n(a.st, a.n_max);
  const int r = blockIdx.x * XK_PSP_T + threadIdx.x;
  if (r >= rows) return;
  const int vh = a.var_of_cell[a.sid_hist[r]], vc = a.var_of_cell[a.sid_cur[r]];
  if (vh < 0 || vc < 0 || vh >= n || vc >= n) return;            // (n > n_max: the host refuses the estimate)
  atomicAdd(&a.mult[(size_t)vh * a.ld + vc], 1);
  atomicAdd(&a.mult[(size_t)vc * a.ld + vh], 1);
  atomicAdd(&a.deg[vh], 1);
  atomicAdd(&a.deg[vc], 1);
}

// Row v of L, and c[v] = sum over the rows r that touch variable v, r ascending, of +b_r (v is the row's current cell) or -b_r (its
// history cell): the wavefront passes over the row list 64 rows at a time and adds the set lanes' terms in lane order.
__global__ __launch_bounds__(XK_PSP_T) void xk_photo_sp_normal(XkPspNormArgs a) {
#pragma clang fp contract(off)
  const int n = xk_psp_n(a.st, a.n_max), rows = min(a.st->rows, a.max_rows);
  const int lane = threadIdx.x & 63, v = blockIdx.x * (XK_PSP_T / 64) + (threadIdx.x >> 6);
  if (v >= n) return;                                            // (a whole wavefront; no barrier below)
  const int d = a.deg[v];
  for (int j = lane; j < n; j += 64) a.L[(size_t)v * a.ld + j] = j == v ? (double)d : -(double)a.mult[(size_t)v * a.ld + j];
  double s = 0.0;
  for (int r0 = 0; r0 < rows; r0 += 64) {
    const int r = r0 + lane;
    double t = 0.0;
    bool on = false;
    if (r < rows) {
      const int vh = a.var_of_cell[a.sid_hist[r]], vc = a.var_of_cell[a.sid_cur[r]];
      if (vc == v) { t = a.b[r]; on = true; }
      else if (vh == v) { t = -a.b[r]; on = true; }
    }
    unsigned long long m = __ballot(on);
    while (m) {
      const int l = __ffsll((long long)m) - 1;
      s = s + __shfl(t, l, 64);
      m &= m - 1ull;
    }
  }
  if (lane == 0) { a.c[v] = s; a.diag[v] = (double)d; }
}

// ---- the Gaussian process ----
struct XkPspGpArgs {
  const int *cell_of_var;
  double *K, *diag;                // [n][ld], [n]
  int ld, n_max;
  XkPspGrid g;
  double sf2, sn2, inv2l2;         // sf^2, sn^2, 1 / (2 l^2) from the float hyperparameters
  const double *alpha;
  float *coarse;                   // [cells]
  float *ps;                       // [h][pitch]
  int pitch;
  const XkPspState *st;
};

__device__ __forceinline__ double xk_psp_cov(const XkPspGpArgs &a, int cell_i, int cell_j) {
  const int dx = cell_i % a.g.cw - cell_j % a.g.cw, dy = cell_i / a.g.cw - cell_j / a.g.cw;
  return a.sf2 * exp(-(double)(dx * dx + dy * dy) * a.inv2l2);
}

__global__ __launch_bounds__(XK_PSP_T) void xk_photo_sp_kernel(XkPspGpArgs a) {
  const int n = xk_psp_n(a.st, a.n_max), i = blockIdx.x;
  if (i >= n) return;
  const int ci = a.cell_of_var[i];
  for (int j = threadIdx.x; j < n; j += XK_PSP_T) {
    const double k = xk_psp_cov(a, ci, a.cell_of_var[j]);
    a.K[(size_t)i * a.ld + j] = j == i ? k + a.sn2 : k;
  }
  if (threadIdx.x == 0) a.diag[i] = a.sf2 + a.sn2;
}

__device__ __forceinline__ double xk_psp_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(64) void xk_photo_sp_predict(XkPspGpArgs a) {
  const int n = xk_psp_n(a.st, a.n_max), cell = blockIdx.x, lane = threadIdx.x;
  if (cell >= a.g.cells || !a.st->gp.converged) return;
  double s = 0.0;
  for (int i = lane; i < n; i += 64) s += xk_psp_cov(a, cell, a.cell_of_var[i]) * a.alpha[i];
  const float v = (float)xk_psp_wave_sum(s);
  if (lane == 0) a.coarse[cell] = v;
  // this cell's pixels; the last column / row of cells also takes the remainder (the clamp of the statement)
  const int cx = cell % a.g.cw, cy = cell / a.g.cw;
  const int x0 = cx * a.g.div, x1 = cx == a.g.cw - 1 ? a.g.w : x0 + a.g.div;
  const int y0 = cy * a.g.div, y1 = cy == a.g.ch - 1 ? a.g.h : y0 + a.g.div;
  const int bw = x1 - x0, total = bw * (y1 - y0);
  for (int k = lane; k < total; k += 64) {
    const int r = k / bw, c = k - r * bw;
    a.ps[(size_t)(y0 + r) * a.pitch + x0 + c] = v;               // x0 + c < w <= pitch, y0 + r < h
  }
}

// ---- preconditioned conjugate gradients on a dense symmetric matrix ----
struct XkPspPcgArgs {
  const double *A;                 // [n][ld]
  const double *rhs, *diag;
  double *x, *r, *p, *q, *partial; // [n] each; partial: one slot per workgroup of the matvec
  int ld, n_max, cap;              // cap > 0: the iteration cap (lab); 0: 2 n
  XkPspSolve *s;
  const XkPspSolve *after;         // NULL, or a solve that must have converged for this one to start
  const XkPspState *st;
};

// z = M^-1 r with M = diag.  A variable of degree 0 (every row that touched it was dropped) has a zero row and a zero right-hand
// side: it keeps x = 0.
__device__ __forceinline__ double xk_psp_prec(double r, double d) { return d > 0.0 ? r / d : 0.0; }

// The sum of one value per thread of a 256-thread workgroup, in a fixed order; every thread gets it.
__device__ __forceinline__ double xk_psp_block_sum(double v, double *s_w) {
  v = xk_psp_wave_sum(v);
  __syncthreads();                                               // (s_w is free again)
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

__global__ __launch_bounds__(XK_PSP_T) void xk_photo_sp_pcg_init(XkPspPcgArgs a) {
  __shared__ double s_w[XK_PSP_T / 64];
  const int n = xk_psp_n(a.st, a.n_max);
  const bool skip = a.after && !a.after->converged;
  double bb = 0.0, rz = 0.0;
  for (int i = threadIdx.x; i < n; i += XK_PSP_T) {
    const double r = a.rhs[i], z = xk_psp_prec(r, a.diag[i]);
    a.x[i] = 0.0; a.r[i] = r; a.p[i] = z;
    bb += r * r; rz += r * z;
  }
  bb = xk_psp_block_sum(bb, s_w);
  rz = xk_psp_block_sum(rz, s_w);
  if (threadIdx.x == 0) {
    XkPspSolve s;
    s.bb = bb; s.rr = bb; s.rz = rz; s.thr = XK_PSP_TOL * XK_PSP_TOL * bb;
    s.it = 0; s.cap = a.cap > 0 ? a.cap : 2 * n;
    s.converged = (!skip && bb == 0.0) ? 1 : 0;                   // a zero right-hand side: x = 0 is the solution
    s.done = (skip || bb == 0.0 || !(bb == bb)) ? 1 : 0;
    *a.s = s;
  }
}

__global__ __launch_bounds__(64 * XK_PSP_MV_ROWS) void xk_photo_sp_matvec(XkPspPcgArgs a) {
  __shared__ double s_pq[XK_PSP_MV_ROWS];
  if (a.s->done) return;                                         // (the whole grid)
  const int n = xk_psp_n(a.st, a.n_max);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, row = blockIdx.x * XK_PSP_MV_ROWS + wv;
  double pq = 0.0;
  if (row < n) {
    const double *Ar = a.A + (size_t)row * a.ld;
    double s = 0.0;
    for (int j = lane; j < n; j += 64) s += Ar[j] * a.p[j];
    s = xk_psp_wave_sum(s);
    if (lane == 0) a.q[row] = s;
    pq = a.p[row] * s;
  }
  if (lane == 0) s_pq[wv] = pq;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < XK_PSP_MV_ROWS; ++k) t += s_pq[k];
    a.partial[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(XK_PSP_T) void xk_photo_sp_step(XkPspPcgArgs a) {
  __shared__ double s_w[XK_PSP_T / 64];
  if (a.s->done) return;
  const int n = xk_psp_n(a.st, a.n_max), slots = (n + XK_PSP_MV_ROWS - 1) / XK_PSP_MV_ROWS;
  double t = 0.0;
  for (int k = threadIdx.x; k < slots; k += XK_PSP_T) t += a.partial[k];
  const double pq = xk_psp_block_sum(t, s_w);
  const double rz = a.s->rz, alpha = rz / pq;
  double rr = 0.0, rz1 = 0.0;
  for (int i = threadIdx.x; i < n; i += XK_PSP_T) {
    const double r = a.r[i] - alpha * a.q[i];
    a.x[i] += alpha * a.p[i];
    a.r[i] = r;
    rr += r * r; rz1 += r * xk_psp_prec(r, a.diag[i]);
  }
  rr = xk_psp_block_sum(rr, s_w);
  rz1 = xk_psp_block_sum(rz1, s_w);
  const double beta = rz1 / rz;
  for (int i = threadIdx.x; i < n; i += XK_PSP_T) a.p[i] = xk_psp_prec(a.r[i], a.diag[i]) + beta * a.p[i];
  __syncthreads();                                               // (every thread has read the record)
  if (threadIdx.x == 0) {
    const int it = a.s->it + 1;
    const bool conv = rr < a.s->thr, bad = !(rr == rr) || !(pq == pq);
    a.s->it = it; a.s->rr = rr; a.s->rz = rz1;
    a.s->converged = (conv && !bad) ? 1 : 0;
    a.s->done = (conv || bad || it >= a.s->cap) ? 1 : 0;
  }
}
