// xk_ransac.hip.h -- what the RANSAC filters share (gfx950): xk_essential.hip.h, xk_fundamental.hip.h and the ordered
// compaction of xk_klt.hip.h.  One copy of each piece, so that the sampler's stream, the tie-break rule, the key packing and
// the chunked scan cannot drift apart between the filters.
//
//   stream, sampler     splitmix64, M distinct indices per hypothesis without a rejection loop
//   null space          of the M x 9 epipolar system, Householder on its transpose
//   polynomials         Horner, the safeguarded bracket root, real roots by derivative bracketing
//   score               per candidate inlier count + summed error, the hypothesis' best candidate, the packed atomicMax key
//   winner              the key decoded
//   median              per candidate the median of the errors by radix select in LDS (least median of squares), the argmin
//   ordered compaction  ballot + popcount per wavefront, wave totals through LDS, a running base over chunks of 256
//   XkRansacScratch     the per-hypothesis scratch block; XkKeptPairs, the "kept pairs" tail of a result block
//
// What a model keeps to itself: its minimal solver past the null space, its error function, its kernels.  The solver pieces
// are __host__ __device__ so that the same text can be exercised on a CPU.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define XK_RANSAC_HD __host__ __device__ inline

// The count of a launch.  n_dev == NULL: n, by value, as the stage entries pass it.  Otherwise the host knows only the bound n (it sized
// the grid and the buffers by it) and the count is what an earlier launch on the same stream left at n_dev: a plain load, held
// within the bound.  The frame entry (xk_frame.hip.h) launches this way.
__device__ __forceinline__ int xk_dev_count(const int *n_dev, int n) { return n_dev ? min(max(*n_dev, 0), n) : n; }

XK_RANSAC_HD unsigned long long xk_ransac_mix(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// Hypothesis h draws values M h .. M h + M - 1 of the stream (value i = mix(seed + (i+1) golden)); draw k lands in [0, n-k)
// and is shifted past the earlier picks in ascending order: M distinct indices, no rejection loop.
template <int M>
XK_RANSAC_HD void xk_ransac_sample(unsigned long long seed, int h, int n, int pick[M]) {
  unsigned int sorted[M];
#pragma unroll
  for (int k = 0; k < M; ++k) {
    const unsigned long long z = xk_ransac_mix(seed + (unsigned long long)((long long)M * h + k + 1) * 0x9E3779B97F4A7C15ull);
    unsigned int r = (unsigned int)(((z >> 32) * (unsigned long long)(n - k)) >> 32);
#pragma unroll
    for (int m = 0; m < k; ++m)
      if (r >= sorted[m]) ++r;
    pick[k] = (int)r;
    sorted[k] = r;
#pragma unroll
    for (int j = k; j > 0; --j)
      if (sorted[j] < sorted[j - 1]) { const unsigned int t = sorted[j]; sorted[j] = sorted[j - 1]; sorted[j - 1] = t; }
  }
}

// Null space of the M x 9 epipolar system of the pairs (p1, p2), row p: p2_i p1_j at 3i + j.  M Householder reflectors on its
// transpose (beta = 0 for a zero column), applied backwards to e_M .. e_8: the last 9 - M columns of Q, orthonormal, entry by
// entry in Nt[9][9 - M].
template <int M>
XK_RANSAC_HD void xk_ransac_null_space(const double (*p1)[2], const double (*p2)[2], double (*Nt)[9 - M]) {
  double a[M][9], beta[M];
#pragma unroll
  for (int p = 0; p < M; ++p) {
    const double u[3] = {p2[p][0], p2[p][1], 1.0}, v[3] = {p1[p][0], p1[p][1], 1.0};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) a[p][3 * i + j] = u[i] * v[j];
  }
#pragma unroll
  for (int k = 0; k < M; ++k) {
    double s = 0.0;
#pragma unroll
    for (int t = k; t < 9; ++t) s += a[k][t] * a[k][t];
    const double nrm = sqrt(s);
    beta[k] = 0.0;
    if (nrm > 0.0) {
      const double alpha = a[k][k] > 0 ? -nrm : nrm;
      a[k][k] -= alpha;
      double vv = 0.0;
#pragma unroll
      for (int t = k; t < 9; ++t) vv += a[k][t] * a[k][t];
      beta[k] = 2.0 / vv;
#pragma unroll
      for (int j = k + 1; j < M; ++j) {
        double d = 0.0;
#pragma unroll
        for (int t = k; t < 9; ++t) d += a[k][t] * a[j][t];
        d *= beta[k];
#pragma unroll
        for (int t = k; t < 9; ++t) a[j][t] -= d * a[k][t];
      }
    }
  }
#pragma unroll
  for (int v = 0; v < 9 - M; ++v) {
    double q[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) q[t] = (t == M + v) ? 1.0 : 0.0;
#pragma unroll
    for (int k = M - 1; k >= 0; --k) {
      double d = 0.0;
#pragma unroll
      for (int t = k; t < 9; ++t) d += a[k][t] * q[t];
      d *= beta[k];
#pragma unroll
      for (int t = k; t < 9; ++t) q[t] -= d * a[k][t];
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) Nt[t][v] = q[t];
  }
}

XK_RANSAC_HD double xk_ransac_horner(const double *c, int d, double x) {
  double f = c[d];
  for (int k = d - 1; k >= 0; --k) f = f * x + c[k];
  return f;
}

// The root of the degree-d polynomial c in (lo, hi), f(lo) and f(hi) of opposite sign: Newton, bisection where it leaves
// the bracket or stalls.
XK_RANSAC_HD double xk_ransac_bracket_root(const double *c, int d, double lo, double hi, double flo) {
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

// Real roots of c[0..D] (ascending powers, |c[D]| > 0), ascending: the roots of each derivative bracket the roots of the next.
// -1 where the bound on the roots is not finite.  Plain loops on purpose: unrolled into select chains this is 1.7x the code
// at D = 10 (LAB).
template <int D>
XK_RANSAC_HD int xk_ransac_real_roots(const double *c, double *roots) {
  double prev[D], cur[D], pd[D + 1];
  int nprev = 0;
  for (int d = 1; d <= D; ++d) {
    const int m = D - d;                       // pd = m-th derivative of c
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
    double lo = -R, flo = xk_ransac_horner(pd, d, lo);
    for (int s = 0; s <= nprev; ++s) {
      const double hi = s < nprev ? prev[s] : R;
      const double fhi = xk_ransac_horner(pd, d, hi);
      if ((flo < 0) != (fhi < 0) && nc < D) cur[nc++] = xk_ransac_bracket_root(pd, d, lo, hi, flo);
      lo = hi; flo = fhi;
    }
    for (int s = 0; s < nc; ++s) prev[s] = cur[s];
    nprev = nc;
  }
  for (int s = 0; s < nprev; ++s) roots[s] = prev[s];
  return nprev;
}

// The scratch block of a filter with at most MAXC candidates per hypothesis and max_hyp hypotheses.
struct XkRansacScratch {
  double *cand;                     // [max_hyp][MAXC][9]
  double *sum;                      // [max_hyp][MAXC]
  int *cnt;                         // [max_hyp][MAXC]
  int *ncand, *bestc;               // [max_hyp]
  unsigned long long *key;
};

template <int MAXC>
inline size_t xk_ransac_scratch_bytes(size_t max_hyp) {
  return sizeof(double) * (max_hyp * MAXC * 10 + 1) + sizeof(int) * max_hyp * (MAXC + 2);
}

// base: 8-byte aligned; the doubles first, so everything stays aligned
template <int MAXC>
inline XkRansacScratch xk_ransac_scratch(void *base, size_t max_hyp) {
  XkRansacScratch s;
  s.cand = (double *)base;
  s.sum = s.cand + max_hyp * MAXC * 9;
  s.key = (unsigned long long *)(s.sum + max_hyp * MAXC);
  s.cnt = (int *)(s.key + 1);
  s.ncand = s.cnt + max_hyp * MAXC;
  s.bestc = s.ncand + max_hyp;
  return s;
}

// The body of a score kernel: workgroup blockIdx.x of 256 takes hypothesis blockIdx.x, lanes over the n points.  err(C, i) is
// the squared error of point i under the candidate C[9].  Per candidate the inlier count (err <= t2) and the summed inlier
// error; the hypothesis' best candidate (most inliers, then the smaller sum, then the lower index); and the filter's key.
template <int MAXC, class Err>
__device__ __forceinline__ void xk_ransac_score(const XkRansacScratch &s, int n, double t2, Err err) {
  __shared__ int s_cnt[4];
  __shared__ double s_sum[4];
  const int h = blockIdx.x, nc = s.ncand[h];
  int best_c = -1, best_cnt = -1;
  double best_sum = 0.0;
  for (int c = 0; c < MAXC; ++c) {
    int cnt = 0;
    double sum = 0.0;
    if (c < nc) {
      const double *Cp = s.cand + ((size_t)h * MAXC + c) * 9;
      const double C[9] = {Cp[0], Cp[1], Cp[2], Cp[3], Cp[4], Cp[5], Cp[6], Cp[7], Cp[8]};
      for (int i = threadIdx.x; i < n; i += 256) {
        const double d = err(C, i);
        if (d <= t2) { ++cnt; sum += d; }
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
    if (threadIdx.x == 0) { s.cnt[h * MAXC + c] = cnt; s.sum[h * MAXC + c] = sum; }
  }
  if (threadIdx.x == 0) {
    s.bestc[h] = best_c;
    // count in the high word, inverted hypothesis index in the low word: the maximum is the highest count, then the lowest h
    if (best_c >= 0) atomicMax(s.key, ((unsigned long long)best_cnt << 32) | (unsigned long long)(0xffffffffu - (unsigned int)h));
  }
}

// Errors of a candidate that the median body keeps in LDS: n at most this many are computed once and staged, more are recomputed in
// every pass.  4096 keys are 32 KiB; with the histogram a workgroup holds 33 KiB, so four of them (one per SIMD) still fit the 160 KiB
// of a CU.  Both paths see the same keys, so they give the same bits.
#define XK_RANSAC_MED_STAGE 4096

// The order key of a squared error d >= +0: its bit pattern, which orders as the value does; a NaN counts as +inf.
__device__ __forceinline__ unsigned long long xk_ransac_med_key(double d) {
  return d != d ? 0x7ff0000000000000ull : (unsigned long long)__double_as_longlong(d);
}

// The body of a median kernel (least median of squares): the same grid as xk_ransac_score, workgroup blockIdx.x of 256 takes hypothesis
// blockIdx.x, lanes over the n >= 1 points, candidates in turn.  Per candidate med = 0.5 (e[(n-1)/2] + e[n/2]) of the ascending errors
// e, to s.sum; a candidate whose median is not finite is not a candidate (s.sum = +inf, as for the slots past ncand).  s.cnt = 0.
// The hypothesis' best candidate (smallest median, then the lower index; -1: none) to s.bestc.  No key: the medians are doubles, the
// winner is an argmin over s.sum (xk_ransac_median_winner).
//
// e[(n-1)/2] by radix select on the keys, most significant byte first: per pass a 256-bin histogram in LDS by integer atomics (counts
// do not depend on the order of the adds), scanned by wavefront 0 (four bins per lane, named scalars), the rank narrowed into the bin
// that holds it.  After eight passes the key is known, and with it the number of keys below it and equal to it.  e[n/2] is the same key
// if more than n/2 keys are <= it, else the smallest key above it: one min-reduction pass.
template <int MAXC, class Err>
__device__ __forceinline__ void xk_ransac_median(const XkRansacScratch &s, int n, Err err) {
  __shared__ unsigned long long s_key[XK_RANSAC_MED_STAGE];
  __shared__ unsigned long long s_min[4];
  __shared__ int s_hist[256];
  __shared__ int s_sel[4];                     // the chosen bin, the rank inside it, the pass' keys below it, the keys in it
  const int h = blockIdx.x, nc = s.ncand[h];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bool staged = n <= XK_RANSAC_MED_STAGE;
  int best_c = -1;
  double best_med = 0.0;
  for (int c = 0; c < MAXC; ++c) {
    double med = INFINITY;
    if (c < nc) {
      const double *Cp = s.cand + ((size_t)h * MAXC + c) * 9;
      const double C[9] = {Cp[0], Cp[1], Cp[2], Cp[3], Cp[4], Cp[5], Cp[6], Cp[7], Cp[8]};
      auto key_at = [&](int i) { return staged ? s_key[i] : xk_ransac_med_key(err(C, i)); };
      if (staged)
        for (int i = threadIdx.x; i < n; i += 256) s_key[i] = xk_ransac_med_key(err(C, i));
      unsigned long long pre = 0ull;           // the bytes chosen so far, in place
      int rank = (n - 1) / 2, below = 0, equal = 0;
      for (int p = 0; p < 8; ++p) {
        const int shift = 56 - 8 * p;
        s_hist[threadIdx.x] = 0;
        __syncthreads();                       // (also: s_key is written, and s_sel of the pass before has been read)
        for (int i = threadIdx.x; i < n; i += 256) {
          const unsigned long long k = key_at(i);
          if (p == 0 || ((k ^ pre) >> (shift + 8)) == 0ull) atomicAdd(&s_hist[(int)((k >> shift) & 255ull)], 1);
        }
        __syncthreads();
        if (w == 0) {
          const int a0 = s_hist[4 * lane], a1 = s_hist[4 * lane + 1], a2 = s_hist[4 * lane + 2], a3 = s_hist[4 * lane + 3];
          const int tot = a0 + a1 + a2 + a3;
          int inc = tot;
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
          }
          const int exc = inc - tot;           // keys of this pass in the bins below this lane's four
          if (exc <= rank && rank < inc) {     // exactly one lane: the counts of a pass sum to more than the rank
            int r = rank - exc, b = 0, in_bin = a0;
            if (r >= a0) { r -= a0; b = 1; in_bin = a1;
              if (r >= a1) { r -= a1; b = 2; in_bin = a2;
                if (r >= a2) { r -= a2; b = 3; in_bin = a3; } } }
            s_sel[0] = 4 * lane + b;
            s_sel[1] = r;
            s_sel[2] = rank - r;
            s_sel[3] = in_bin;
          }
        }
        __syncthreads();
        const int bin = s_sel[0];
        below += s_sel[2];
        rank = s_sel[1];
        equal = s_sel[3];                      // (not s_hist[bin]: the next pass is already zeroing it)
        pre |= (unsigned long long)bin << shift;
      }
      // pre = e[(n-1)/2]; `below` keys are smaller, `equal` keys equal it
      unsigned long long hi = pre;
      if (below + equal <= n / 2) {            // (uniform: every thread holds the same counts)
        unsigned long long m = ~0ull;
        for (int i = threadIdx.x; i < n; i += 256) {
          const unsigned long long k = key_at(i);
          if (k > pre && k < m) m = k;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const unsigned long long v = __shfl_down(m, o, 64);
          if (v < m) m = v;
        }
        if (lane == 0) s_min[w] = m;
        __syncthreads();
        hi = s_min[0];
        if (s_min[1] < hi) hi = s_min[1];
        if (s_min[2] < hi) hi = s_min[2];
        if (s_min[3] < hi) hi = s_min[3];
      }
      __syncthreads();                         // (s_key, s_hist and s_min are free for the next candidate)
      med = 0.5 * (__longlong_as_double((long long)pre) + __longlong_as_double((long long)hi));
      if (!(med < INFINITY)) med = INFINITY;
      else if (best_c < 0 || med < best_med) { best_med = med; best_c = c; }
    }
    if (threadIdx.x == 0) { s.cnt[h * MAXC + c] = 0; s.sum[h * MAXC + c] = med; }
  }
  if (threadIdx.x == 0) s.bestc[h] = best_c;
}

// The winner of the medians by ONE workgroup of 256: smallest median, then the lowest hypothesis (its candidate is s.bestc: the
// smallest median, then the lowest candidate).  (median, hypothesis) is a total order, so the reduction's shape does not matter.
struct XkMedianWinner { bool valid; int h; double med; };
__device__ __forceinline__ XkMedianWinner xk_ransac_median_winner(const XkRansacScratch &s, int n_hyp, int maxc) {
  __shared__ double s_med[4];
  __shared__ int s_h[4];
  double med = INFINITY;
  int hb = 0x7fffffff;
  for (int h = threadIdx.x; h < n_hyp; h += 256) {
    const int c = s.bestc[h];
    if (c < 0) continue;
    const double m = s.sum[(size_t)h * maxc + c];
    if (m < med) { med = m; hb = h; }          // (ascending h per thread: a tie keeps the lower one)
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double m = __shfl_down(med, o, 64);
    const int h = __shfl_down(hb, o, 64);
    if (m < med || (m == med && h < hb)) { med = m; hb = h; }
  }
  if ((threadIdx.x & 63) == 0) { s_med[threadIdx.x >> 6] = med; s_h[threadIdx.x >> 6] = hb; }
  __syncthreads();
  med = s_med[0]; hb = s_h[0];
#pragma unroll
  for (int j = 1; j < 4; ++j)
    if (s_med[j] < med || (s_med[j] == med && s_h[j] < hb)) { med = s_med[j]; hb = s_h[j]; }
  __syncthreads();
  XkMedianWinner wn;
  wn.valid = hb != 0x7fffffff;
  wn.h = wn.valid ? hb : 0;
  wn.med = wn.valid ? med : 0.0;
  return wn;
}

// The key decoded.  valid = false: no hypothesis produced a candidate (the solve kernel's thread 0 zeroes the key).
struct XkRansacWinner { bool valid; int h, count; };
__device__ __forceinline__ XkRansacWinner xk_ransac_winner(unsigned long long key) {
  XkRansacWinner w;
  w.valid = key != 0ull;
  w.h = (int)(0xffffffffu - (unsigned int)(key & 0xffffffffull));
  w.count = (int)(key >> 32);
  return w;
}

// The "kept pairs" tail of a result block for n pairs: the doubles kept_prev [n][2], kept_cur [n][2], then the ints res [2],
// keep_idx [n].  The first res[0] rows of each list are written.  The block's byte plane [n] follows at xk_kept_pairs_end.
struct XkKeptPairs {
  double *kept_prev, *kept_cur;
  int *res, *keep_idx;
};
inline size_t xk_kept_pairs_bytes(size_t n) { return sizeof(double) * 4 * n + sizeof(int) * (2 + n); }
inline XkKeptPairs xk_kept_pairs(double *at, size_t n) {
  XkKeptPairs k;
  k.kept_prev = at; k.kept_cur = at + 2 * n;
  k.res = (int *)(at + 4 * n);
  k.keep_idx = k.res + 2;
  return k;
}
inline unsigned char *xk_kept_pairs_end(const XkKeptPairs &k, size_t n) { return (unsigned char *)(k.keep_idx + n); }

// ORDERED compaction by ONE workgroup of 256: keep(i) is asked once for every i < n, put(i, pos) called for every kept i with
// the number pos of kept indices below i; returns the total.  A thread's put(i, .) directly follows its keep(i), so the two
// may share what keep loaded through the caller's locals.
template <class Keep, class Put>
__device__ __forceinline__ int xk_ransac_compact(int n, Keep keep, Put put) {
  __shared__ int s_w[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int base = 0;                                // kept before this chunk of 256
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + threadIdx.x;
    const bool k = i < n && keep(i);
    const unsigned long long b = __ballot(k);
    const int before = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) s_w[w] = __popcll(b);
    __syncthreads();
    int off = base;
    for (int j = 0; j < w; ++j) off += s_w[j];
    base += s_w[0] + s_w[1] + s_w[2] + s_w[3];
    if (k) put(i, off + before);               // (off + before < n: it counts kept indices below i)
    __syncthreads();
  }
  return base;
}
