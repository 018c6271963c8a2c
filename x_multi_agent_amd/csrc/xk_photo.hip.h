// xk_photo.hip.h -- photometric calibration of the tracker's images, Tracker::calibrateImage (gfx950).
//
//   computeIntensity(img, x, y): the box mean around a feature                                      (tracker.cpp:860-877)
//   IRPhotoCalib::EstimateGainsRansac: the affine gain between two lists of intensities             (irPhotoCalib.cpp:221-312)
//   IRPhotoCalib::ProcessCurrentFrame: the gains chained into a history of 15 frames                (irPhotoCalib.cpp:95-160, :212-218)
//   IRPhotoCalib::getCorrectedImage: every pixel of the current image rewritten                     (irPhotoCalib.cpp:442-472)
//
// The algorithm is this project's own statement of those calls, restated in NumPy by tests/photo_np.py.  What
// the reference keeps as an integer stays an EXACT integer (the window sums, which it accumulates in float); the gain fit is
// the closed-form minimum of the cost Ceres iterates on (photoetricOptimization.h:57-100), not Ceres' last iterate; the
// RANSAC draws from the counter-based sampler of xk_ransac.hip.h, not from std::random_device.  fp64 and fp32 arithmetic is
// written without contraction, so that a restatement in IEEE arithmetic follows it operation by operation.
//
//   xk_photo_intensity  one WAVEFRONT per point, XK_PHOTO_WAVES points per workgroup, no barrier: lanes stride over the clipped
//                       window's pixels, int32 per lane (<= 64 terms of <= 255), the butterfly of xk_klt_wave_sum for the total
//   xk_photo_gather     (per-frame call only) the kept points' truncated pixels, their previous intensities, the group's bounds
//   xk_photo_solve      one thread per hypothesis: four distinct points from the sampler, the 2 x 2 normal equations by Cramer
//   xk_photo_score      one workgroup per hypothesis: xk_ransac_score<1>, C[0] = a, C[1] = b, the packed atomicMax key
//   xk_photo_refit      one workgroup: the winner's inliers, fp64 partial sums in a fixed order, the same closed form
//   xk_photo_chain      one thread: chainGains / getRelativeGains per group, the weighted mean, the drift adjustments, the ring
//   xk_photo_correct    16 pixels per lane where they lie inside the row (one 16-byte load of the raw image, four of PS, one
//                       16-byte store), single bytes at the row's end; fp32 with every operation rounded once
// The sizes of a group, the kept count of the per-frame call and the ring live on the device: a frame's launches need no host
// round trip between them.  No atomics beyond the skeleton's key, no inline assembly.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "xk_klt.hip.h"
#include "xk_ransac.hip.h"

#define XK_PHOTO_RING 15           // frames of history (irPhotoCalib.cpp:215)
#define XK_PHOTO_MAX_GROUPS 14     // groups of one call: one per history frame behind the current one
#define XK_PHOTO_MAX_HYP 4096
#define XK_PHOTO_WAVES 4           // points per workgroup of xk_photo_intensity
#define XK_PHOTO_SOLVE_T 64
#define XK_PHOTO_INLIER 8.0e-3     // irPhotoCalib.cpp:270, strict
#define XK_PHOTO_PRIOR_W 0.1       // photoetricOptimization.h:66

// What lives on the device between calls and comes back whole after each: the ring (pair k at 2k), the last call's results.
struct XkPhotoState {
  double ring[2 * XK_PHOTO_RING];
  double a_rel[XK_PHOTO_MAX_GROUPS], b_rel[XK_PHOTO_MAX_GROUPS];   // per group: the refit's gain, (1, 0) for a group of <= 4
  double frame_ab[4];              // the weighted relative pair after the adjustments, the frame's origin pair
  int support[XK_PHOTO_MAX_GROUPS];
  int ring_n;                      // 1 ... 15
  int done;                        // a per-frame call has estimated gains (CALIBRATION_DONE)
  int estimated;                   // the last per-frame call did
  int pad;
};

struct XkPhotoIntArgs {
  const unsigned char *img;        // level 0 of a plane
  int w, h, pitch, hk;
  const int *xy;                   // [n][2]
  const int *n_dev;                // NULL, or where the device holds the count (<= n)
  int n;
  double *value;
  int *sum, *count;
};

struct XkPhotoGainArgs {
  XkRansacScratch sc;
  const double *o_hist, *o_cur;
  const int *off;                  // [G + 1]
  const int *frame_back;           // [G]
  int g, G, n_hyp, per_frame;
  unsigned long long seed;
  double eps_gap, eps_base;
  XkPhotoState *st;
};

struct XkPhotoGatherArgs {
  XkKeptPairs kept;
  const double *prev_intensity;    // [n]
  int *ixy;                        // [n][2]
  double *o_hist;                  // [n]
  int *off, *frame_back;
};

struct XkPhotoCorrectArgs {
  const unsigned char *raw;
  unsigned char *out;
  const float *PS;                 // [h][pitch] floats
  int w, h, pitch;
  int per_frame;                   // 1: correct iff the state says done, else copy
  const XkPhotoState *st;
};

__global__ __launch_bounds__(64 * XK_PHOTO_WAVES) void xk_photo_intensity(XkPhotoIntArgs a) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * XK_PHOTO_WAVES + (threadIdx.x >> 6);
  const int n = a.n_dev ? min(*a.n_dev, a.n) : a.n;
  if (i >= n) return;                                            // (a whole wavefront; the kernel has no barrier)
  const long long x = a.xy[2 * i], y = a.xy[2 * i + 1];
  const long long x0 = x - a.hk > 0 ? x - a.hk : 0, x1 = x + a.hk < a.w ? x + a.hk : a.w;      // (64 bits: any int32 point)
  const long long y0 = y - a.hk > 0 ? y - a.hk : 0, y1 = y + a.hk < a.h ? y + a.hk : a.h;
  int s = 0, cnt = 0;
  if (x1 > x0 && y1 > y0) {
    const int ww = (int)(x1 - x0), wh = (int)(y1 - y0);
    cnt = ww * wh;
    const unsigned char *p = a.img + (size_t)y0 * a.pitch + (size_t)x0;      // columns x0 ... x1 - 1 < w only: never the padding
    for (int k = lane; k < cnt; k += 64) {
      const int r = k / ww, c = k - r * ww;
      s += p[r * a.pitch + c];
    }
  }
  const int total = (int)xk_klt_wave_sum(s);
  if (lane == 0) {
    a.sum[i] = total;
    a.count[i] = cnt;
    a.value[i] = cnt > 0 ? (double)total / (255.0 * (double)cnt) : 0.0;
  }
}

__global__ __launch_bounds__(256) void xk_photo_gather(XkPhotoGatherArgs a) {
  const int kept = a.kept.res[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) { a.off[0] = 0; a.off[1] = kept; a.frame_back[0] = 1; }
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= kept) return;
  a.ixy[2 * j] = (int)a.kept.kept_cur[2 * j];                    // static_cast<int> (tracker.cpp:807-808); within [-0.5, W - 0.5]
  a.ixy[2 * j + 1] = (int)a.kept.kept_cur[2 * j + 1];
  a.o_hist[j] = a.prev_intensity[a.kept.keep_idx[j]];
}

// The minimum of sum (o - p a - (1 - p) b)^2 + w^2 (a - 1)^2 + w^2 b^2 from its sums: u = p, v = 1 - p.
struct XkPhotoSums { double uu, uv, vv, uo, vo; };

XK_RANSAC_HD void xk_photo_fit(const XkPhotoSums &s, double *a, double *b) {
#pragma clang fp contract(off)
  const double w2 = XK_PHOTO_PRIOR_W * XK_PHOTO_PRIOR_W;
  const double m00 = s.uu + w2, m11 = s.vv + w2, r0 = s.uo + w2;
  const double det = m00 * m11 - s.uv * s.uv;
  *a = (r0 * m11 - s.uv * s.vo) / det;
  *b = (m00 * s.vo - s.uv * r0) / det;
}

__global__ __launch_bounds__(XK_PHOTO_SOLVE_T) void xk_photo_solve(XkPhotoGainArgs a) {
#pragma clang fp contract(off)
  const int h = blockIdx.x * XK_PHOTO_SOLVE_T + threadIdx.x;
  if (h == 0) *a.sc.key = 0ull;
  const int first = a.off[a.g], n = a.off[a.g + 1] - first;
  if (h >= a.n_hyp || n <= 4) return;
  int pick[4];
  xk_ransac_sample<4>(a.seed + (unsigned long long)a.g, h, n, pick);
  XkPhotoSums s = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double o = a.o_hist[first + pick[k]], u = a.o_cur[first + pick[k]], v = 1.0 - u;
    s.uu += u * u; s.uv += u * v; s.vv += v * v; s.uo += u * o; s.vo += v * o;
  }
  double ga, gb;
  xk_photo_fit(s, &ga, &gb);
  double *C = a.sc.cand + (size_t)h * 9;
  C[0] = ga; C[1] = gb;
#pragma unroll
  for (int k = 2; k < 9; ++k) C[k] = 0.0;
  a.sc.ncand[h] = (isfinite(ga) && isfinite(gb)) ? 1 : 0;
}

__device__ __forceinline__ bool xk_photo_inlier(double o, double p, double ga, double gb) {
#pragma clang fp contract(off)
  return fabs(o - (p * (ga - gb) + gb)) < XK_PHOTO_INLIER;
}

__global__ __launch_bounds__(256) void xk_photo_score(XkPhotoGainArgs a) {
  const int first = a.off[a.g], n = a.off[a.g + 1] - first;
  if (n <= 4) return;                                            // (the whole workgroup)
  const double *O = a.o_hist + first, *P = a.o_cur + first;
  // the skeleton counts err <= t2: 0 for an inlier of the strict bound, 2 for everything else against t2 = 1
  xk_ransac_score<1>(a.sc, n, 1.0, [&](const double *C, int i) { return xk_photo_inlier(O[i], P[i], C[0], C[1]) ? 0.0 : 2.0; });
}

__global__ __launch_bounds__(256) void xk_photo_refit(XkPhotoGainArgs a) {
#pragma clang fp contract(off)
  __shared__ double s_p[4][5];
  __shared__ int s_c[4];
  const int first = a.off[a.g], n = a.off[a.g + 1] - first;
  if (n <= 4) {
    if (threadIdx.x == 0) { a.st->a_rel[a.g] = 1.0; a.st->b_rel[a.g] = 0.0; a.st->support[a.g] = 0; }
    return;
  }
  const XkRansacWinner w = xk_ransac_winner(*a.sc.key);
  const bool valid = w.valid && w.count > 0;
  const double ga = valid ? a.sc.cand[(size_t)w.h * 9] : 1.0, gb = valid ? a.sc.cand[(size_t)w.h * 9 + 1] : 0.0;
  double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  int cnt = 0;
  if (valid)
    for (int i = threadIdx.x; i < n; i += 256) {
      const double o = a.o_hist[first + i], u = a.o_cur[first + i], q = 1.0 - u;
      if (xk_photo_inlier(o, u, ga, gb)) {
        ++cnt;
        v[0] += u * u; v[1] += u * q; v[2] += q * q; v[3] += u * o; v[4] += q * o;
      }
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_down(cnt, o, 64);
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] += __shfl_down(v[k], o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_c[threadIdx.x >> 6] = cnt;
#pragma unroll
    for (int k = 0; k < 5; ++k) s_p[threadIdx.x >> 6][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int support = s_c[0] + s_c[1] + s_c[2] + s_c[3];
    double t[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) t[k] = (s_p[0][k] + s_p[1][k]) + (s_p[2][k] + s_p[3][k]);
    double ra = 1.0, rb = 0.0;
    if (support > 0) {
      const XkPhotoSums s = {t[0], t[1], t[2], t[3], t[4]};
      xk_photo_fit(s, &ra, &rb);
    }
    a.st->a_rel[a.g] = ra; a.st->b_rel[a.g] = rb; a.st->support[a.g] = support;
  }
}

// irPhotoCalib.cpp:68-82, operation by operation
XK_RANSAC_HD void xk_photo_relative(double a1, double b1, double a2, double b2, double *a12, double *b12) {
#pragma clang fp contract(off)
  const double e12 = (a2 - b2) / (a1 - b1);
  *b12 = (b2 - b1) / (a1 - b1);
  *a12 = e12 + *b12;
}
XK_RANSAC_HD void xk_photo_chain_gains(double a01, double b01, double a12, double b12, double *a02, double *b02) {
#pragma clang fp contract(off)
  const double e02 = (a01 - b01) * (a12 - b12);
  *b02 = b01 + (a01 - b01) * b12;
  *a02 = e02 + *b02;
}

__global__ __launch_bounds__(64) void xk_photo_chain(XkPhotoGainArgs a) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  XkPhotoState *st = a.st;
  if (a.per_frame) {
    st->estimated = 0;
    if (a.off[1] - a.off[0] < 4) return;                         // tracker.cpp:826: the ring does not advance
  }
  const int size = st->ring_n;
  const double ap = st->ring[2 * (size - 1)], bp = st->ring[2 * (size - 1) + 1];
  double w_a = 0.0, w_b = 0.0;
  int w_count = 0;
  for (int g = 0; g < a.G; ++g) {
    if (a.off[g + 1] - a.off[g] <= 4) continue;                  // irPhotoCalib.cpp:116 (xk_photo_refit left (1, 0), support 0)
    const int at = size - a.frame_back[g];                       // (1 <= frame_back <= size: the host checked)
    double aoc, boc, apc, bpc;
    xk_photo_chain_gains(st->ring[2 * at], st->ring[2 * at + 1], st->a_rel[g], st->b_rel[g], &aoc, &boc);
    xk_photo_relative(ap, bp, aoc, boc, &apc, &bpc);
    const int sup = st->support[g];
    w_a += apc * (double)sup; w_b += bpc * (double)sup; w_count += sup;
  }
  double wa = 1.0, wb = 0.0;
  if (w_count >= 5) { wa = w_a / (double)w_count; wb = w_b / (double)w_count; }
  const double delta = (1.0 - (wa - wb)) * a.eps_gap;
  wa = wa + delta;
  wb = wb - delta;
  wa = wa - (wa - 1.0) * a.eps_base;
  wb = wb - wb * a.eps_base;
  double ao, bo;
  xk_photo_chain_gains(ap, bp, wa, wb, &ao, &bo);
  st->frame_ab[0] = wa; st->frame_ab[1] = wb; st->frame_ab[2] = ao; st->frame_ab[3] = bo;
  if (size == XK_PHOTO_RING) {
    for (int k = 0; k < 2 * (XK_PHOTO_RING - 1); ++k) st->ring[k] = st->ring[k + 2];
    st->ring[2 * (XK_PHOTO_RING - 1)] = ao; st->ring[2 * (XK_PHOTO_RING - 1) + 1] = bo;
  } else {
    st->ring[2 * size] = ao; st->ring[2 * size + 1] = bo;
    st->ring_n = size + 1;
  }
  if (a.per_frame) { st->estimated = 1; st->done = 1; }
}

// One pixel of getCorrectedImage: every fp32 operation rounded once, then the remainder's sign rule and the table of :42-51.
__device__ __forceinline__ unsigned int xk_photo_pixel(unsigned int v, float gain, float base, float ps) {
  const float f = __fmul_rn((float)v, 1.f / 255.f);
  const float c = __fmul_rn(__fsub_rn(__fadd_rn(__fmul_rn(f, gain), base), ps), 255.f);
  const int x = (isfinite(c) && fabsf(c) < 2147483648.f) ? (int)c : 0;
  const int u = max(x % 256, 0);
  return (unsigned int)(u < 128 ? 2 * u : (u == 128 ? 255 : 512 - 2 * u));
}

__device__ __forceinline__ unsigned int xk_photo_four(unsigned int v, float gain, float base, const float4 &ps) {
  return xk_photo_pixel(v & 255u, gain, base, ps.x) | (xk_photo_pixel((v >> 8) & 255u, gain, base, ps.y) << 8) |
         (xk_photo_pixel((v >> 16) & 255u, gain, base, ps.z) << 16) | (xk_photo_pixel(v >> 24, gain, base, ps.w) << 24);
}

__global__ __launch_bounds__(256) void xk_photo_correct(XkPhotoCorrectArgs a) {
  const int gpr = a.pitch >> 4;                                  // groups of 16 columns per row
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= gpr * a.h) return;
  const int y = t / gpr, x0 = (t - y * gpr) << 4;
  if (x0 >= a.w) return;
  const bool apply = !a.per_frame || a.st->done != 0;
  const int size = a.st->ring_n;
  const double ga = a.st->ring[2 * (size - 1)], gb = a.st->ring[2 * (size - 1) + 1];
  const float gain = (float)(ga - gb), base = (float)gb;
  const size_t at = (size_t)y * a.pitch + x0;                    // (a multiple of 16, as both planes' bases and PS's)
  if (x0 + 15 < a.w) {
    uint4 v = *reinterpret_cast<const uint4 *>(a.raw + at);
    if (apply) {
      const float4 *ps = reinterpret_cast<const float4 *>(a.PS + at);
      const float4 p0 = ps[0], p1 = ps[1], p2 = ps[2], p3 = ps[3];
      v.x = xk_photo_four(v.x, gain, base, p0); v.y = xk_photo_four(v.y, gain, base, p1);
      v.z = xk_photo_four(v.z, gain, base, p2); v.w = xk_photo_four(v.w, gain, base, p3);
    }
    *reinterpret_cast<uint4 *>(a.out + at) = v;
  } else {
    for (int x = x0; x < a.w; ++x) {                             // the row's end: bytes, never the padding columns
      const unsigned int v = a.raw[at + (x - x0)];
      a.out[at + (x - x0)] = (unsigned char)(apply ? xk_photo_pixel(v, gain, base, a.PS[at + (x - x0)]) : v);
    }
  }
}
