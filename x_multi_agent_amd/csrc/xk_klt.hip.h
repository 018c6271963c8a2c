// xk_klt.hip.h -- pyramidal Lucas-Kanade tracking of the tracker's features, Tracker::featureTracking (gfx950).
//
//   cv::calcOpticalFlowPyrLK(img1, img2, pts1, pts2, status, err, win_size_, max_level_, term_crit_,
//                            cv::OPTFLOW_LK_GET_MIN_EIGENVALS, min_eig_thr_)                        (tracker.cpp:623-655)
//   keep the pairs that were tracked and stayed inside the frame                                      (tracker.cpp:658-686)
//
// The algorithm is this project's own statement of that call, restated in NumPy by tests/klt_np.py.  It follows
// OpenCV step by step with two differences: every quantity OpenCV keeps as an integer stays an EXACT integer -- the pyramid, the
// Scharr derivatives, the fixed-point window samples and also the sums over the window, which OpenCV accumulates in float --
// and everything else is fp64 where OpenCV uses float.  The fp64 part is written without contraction (no fused multiply-add),
// so that a restatement in IEEE arithmetic follows it operation by operation.
//
// Per pushed image, on the handle's stream:
//   xk_klt_scharr    one launch per level: int16 dIx, dIy = [3 10 3] across x [-1 0 1] along, the image mirrored at its edge
//   xk_klt_pyrdown   one launch per level above 0: [1 4 6 4 1]^2, + 128 >> 8, separable through an LDS tile; the source tile is
//                    loaded four bytes at a time where the four lie inside the row, mirrored byte by byte where they do not
// Per frame, one launch pair:
//   xk_klt_track     one WAVEFRONT per feature, XK_KLT_WAVES features per workgroup, no workgroup barrier; all levels of the
//                    feature in this launch.  Lane `lane` owns the window pixels s 64 + lane, s < 16 (31 x 31 = 961 = 15 64 + 1);
//                    their Iw, gx, gy stay in registers across the iterations.  Window sums: int32 per lane (<= 16 terms below
//                    2^27), int64 across the wavefront by a butterfly of cross-lane moves, which leaves the total in every lane;
//                    the 2 x 2 solve and every decision are then redundant and identical in all lanes.
//   xk_klt_compact   one workgroup: the post-filter and the ORDERED compaction of the kept pairs (xk_ransac_compact, as in
//                    xk_fund_mask)
// No atomics, no inline assembly.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "xk_ransac.hip.h"     // the ordered compaction, XkKeptPairs

#define XK_KLT_MAX_LEVELS 5        // levels 0 ... 4
#define XK_KLT_MAX_WIN 31
#define XK_KLT_SLOTS 16            // window pixels per lane
#define XK_KLT_WAVES 4             // features per workgroup of xk_klt_track
#define XK_KLT_PD_TW 64            // output tile of xk_klt_pyrdown
#define XK_KLT_PD_TH 8
#define XK_KLT_PD_ROWS (2 * XK_KLT_PD_TH + 3)
#define XK_KLT_PD_COLS (2 * XK_KLT_PD_TW + 8)   // source columns 2 tx0 - 4 ... 2 tx0 + 131: a multiple of four on both sides

struct XkKltLevel {
  unsigned char *img;              // [h][pitch]
  short *dx, *dy;                  // [h][pitch] each
  int w, h, pitch;                 // pitch in elements, a multiple of 16
};
struct XkKltPyr { XkKltLevel lv[XK_KLT_MAX_LEVELS]; };

// One Lucas-Kanade parameter set: what Tracker::featureTracking switches once the photometric calibration is done (tracker.cpp:641-651).
struct XkKltSet {
  int levels, win_w, win_h;
  double min_eig_thr;
};

struct XkKltArgs {
  XkKltPyr prev, cur;              // both built to the deeper set's levels
  XkKltSet set[2];
  const int *second_on;            // NULL: set[0], the host chose.  Else set[1] where *second_on is not 0 when the kernel runs (the
                                   //   photometric frame: XkPhotoState::done), set[0] where it is 0
  int n, max_iter;
  double eps2;
  const float *pts;                // [n][2] previous points, cv::Point2f
  double *cur_xy;                  // [n][2]
  double *min_eig;                 // [n]
  unsigned char *status;           // [n]
  XkKeptPairs kept;                // res: n_kept
  const int *n_dev;                // NULL: n features.  Else n is the bound the buffers are laid out by, *n_dev the count (xk_dev_count)
};

// reflect-101 (-1 -> 1, n -> n - 2), then clamped: a caller that needs the value stays within one reflection, a tile's unused
// border may ask for anything
__device__ __forceinline__ int xk_klt_mirror(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * n - 2 - i : i;
  return min(max(i, 0), n - 1);
}

__global__ __launch_bounds__(256) void xk_klt_pyrdown(const unsigned char *src, int sw, int sh, int sp, unsigned char *dst, int dw,
                                                      int dh, int dp) {
  __shared__ __attribute__((aligned(16))) unsigned char s_in[XK_KLT_PD_ROWS][XK_KLT_PD_COLS];
  __shared__ unsigned short s_h[XK_KLT_PD_ROWS][XK_KLT_PD_TW];
  const int tx0 = blockIdx.x * XK_KLT_PD_TW, ty0 = blockIdx.y * XK_KLT_PD_TH;
  const int cx0 = 2 * tx0 - 4, cy0 = 2 * ty0 - 2;
  for (int i = threadIdx.x; i < XK_KLT_PD_ROWS * (XK_KLT_PD_COLS / 4); i += 256) {
    const int r = i / (XK_KLT_PD_COLS / 4), g = i - r * (XK_KLT_PD_COLS / 4);
    const unsigned char *row = src + (size_t)xk_klt_mirror(cy0 + r, sh) * sp;
    const int x = cx0 + 4 * g;
    uchar4 v;
    if (x >= 0 && x + 3 < sw) {
      v = *reinterpret_cast<const uchar4 *>(row + x);          // (x, sp and the level's base are multiples of four)
    } else {
      v.x = row[xk_klt_mirror(x, sw)]; v.y = row[xk_klt_mirror(x + 1, sw)];
      v.z = row[xk_klt_mirror(x + 2, sw)]; v.w = row[xk_klt_mirror(x + 3, sw)];
    }
    *reinterpret_cast<uchar4 *>(&s_in[r][4 * g]) = v;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < XK_KLT_PD_ROWS * XK_KLT_PD_TW; i += 256) {
    const int r = i / XK_KLT_PD_TW, c = i - r * XK_KLT_PD_TW;
    const unsigned char *p = &s_in[r][2 * c + 2];               // source column 2 (tx0 + c) - 2
    s_h[r][c] = (unsigned short)(p[0] + 4 * p[1] + 6 * p[2] + 4 * p[3] + p[4]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < XK_KLT_PD_TH * XK_KLT_PD_TW; i += 256) {
    const int r = i / XK_KLT_PD_TW, c = i - r * XK_KLT_PD_TW;
    const int x = tx0 + c, y = ty0 + r;
    if (x < dw && y < dh) {
      const int v = s_h[2 * r][c] + 4 * s_h[2 * r + 1][c] + 6 * s_h[2 * r + 2][c] + 4 * s_h[2 * r + 3][c] + s_h[2 * r + 4][c];
      dst[(size_t)y * dp + x] = (unsigned char)((v + 128) >> 8);
    }
  }
}

__global__ __launch_bounds__(256) void xk_klt_scharr(const unsigned char *img, int w, int h, int p, short *dx, short *dy) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  const int xm = xk_klt_mirror(x - 1, w), xp = xk_klt_mirror(x + 1, w);
  const unsigned char *r0 = img + (size_t)xk_klt_mirror(y - 1, h) * p, *r1 = img + (size_t)y * p,
                      *r2 = img + (size_t)xk_klt_mirror(y + 1, h) * p;
  const int a00 = r0[xm], a01 = r0[x], a02 = r0[xp], a10 = r1[xm], a12 = r1[xp], a20 = r2[xm], a21 = r2[x], a22 = r2[xp];
  dx[(size_t)y * p + x] = (short)(3 * (a02 - a00) + 10 * (a12 - a10) + 3 * (a22 - a20));
  dy[(size_t)y * p + x] = (short)(3 * (a20 - a00) + 10 * (a21 - a01) + 3 * (a22 - a02));
}

// The total over the wavefront in every lane.
__device__ __forceinline__ long long xk_klt_wave_sum(int v32) {
  long long v = (long long)v32;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct XkKltW { int w00, w01, w10, w11; };

__device__ __forceinline__ XkKltW xk_klt_weights(double a, double b) {
  XkKltW w;
  w.w00 = (int)rint((1.0 - a) * (1.0 - b) * 16384.0);
  w.w01 = (int)rint(a * (1.0 - b) * 16384.0);
  w.w10 = (int)rint((1.0 - a) * b * 16384.0);
  w.w11 = 16384 - w.w00 - w.w01 - w.w10;
  return w;
}

// The bounds test of a window's floored corner, taken in fp64 so that it also decides for values no int holds (false for a NaN).
__device__ __forceinline__ bool xk_klt_corner_ok(double fx, double fy, int w, int h, int win_w, int win_h) {
  return fx >= -(double)win_w && fx < (double)w && fy >= -(double)win_h && fy < (double)h;
}

// The four image taps of window pixel (x0, y0) weighed, + 2^8 >> 9: the image scaled by 32.  interior (the same in every lane):
// all taps of the window lie inside the image; otherwise each is mirrored.
__device__ __forceinline__ int xk_klt_image_sample(const unsigned char *img, int w, int h, int pitch, int x0, int y0, bool interior,
                                                   const XkKltW &wt) {
  int v00, v01, v10, v11;
  if (interior) {
    const unsigned char *p = img + y0 * pitch + x0;
    v00 = p[0]; v01 = p[1]; v10 = p[pitch]; v11 = p[pitch + 1];
  } else {
    const int xa = xk_klt_mirror(x0, w), xb = xk_klt_mirror(x0 + 1, w);
    const unsigned char *ra = img + xk_klt_mirror(y0, h) * pitch, *rb = img + xk_klt_mirror(y0 + 1, h) * pitch;
    v00 = ra[xa]; v01 = ra[xb]; v10 = rb[xa]; v11 = rb[xb];
  }
  return (v00 * wt.w00 + v01 * wt.w01 + v10 * wt.w10 + v11 * wt.w11 + (1 << 8)) >> 9;
}

// The same on a derivative plane, + 2^13 >> 14; a tap outside the image is 0.
__device__ __forceinline__ int xk_klt_deriv_sample(const short *d, int w, int h, int pitch, int x0, int y0, bool interior,
                                                   const XkKltW &wt) {
  int v00, v01, v10, v11;
  if (interior) {
    const short *p = d + y0 * pitch + x0;
    v00 = p[0]; v01 = p[1]; v10 = p[pitch]; v11 = p[pitch + 1];
  } else {
    const bool xa = (unsigned)x0 < (unsigned)w, xb = (unsigned)(x0 + 1) < (unsigned)w;
    const bool ya = (unsigned)y0 < (unsigned)h, yb = (unsigned)(y0 + 1) < (unsigned)h;
    v00 = (xa && ya) ? d[y0 * pitch + x0] : 0;
    v01 = (xb && ya) ? d[y0 * pitch + x0 + 1] : 0;
    v10 = (xa && yb) ? d[(y0 + 1) * pitch + x0] : 0;
    v11 = (xb && yb) ? d[(y0 + 1) * pitch + x0 + 1] : 0;
  }
  return (v00 * wt.w00 + v01 * wt.w01 + v10 * wt.w10 + v11 * wt.w11 + (1 << 13)) >> 14;
}

__global__ __launch_bounds__(64 * XK_KLT_WAVES) void xk_klt_track(XkKltArgs a) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * XK_KLT_WAVES + (threadIdx.x >> 6);
  if (f >= xk_dev_count(a.n_dev, a.n)) return;                   // (a whole wavefront; the kernel has no barrier)
  const double px = (double)a.pts[2 * f], py = (double)a.pts[2 * f + 1];
  if (!(isfinite(px) && isfinite(py))) {
    if (lane == 0) { a.cur_xy[2 * f] = px; a.cur_xy[2 * f + 1] = py; a.status[f] = 0; a.min_eig[f] = 0.0; }
    return;
  }
  // One set for the whole feature, read once: the address is the kernel argument's, so the load and the selects below are scalar.
  const bool second = a.second_on && *a.second_on != 0;
  const int levels = second ? a.set[1].levels : a.set[0].levels;
  const int win_w = second ? a.set[1].win_w : a.set[0].win_w, win_h = second ? a.set[1].win_h : a.set[0].win_h, npix = win_w * win_h;
  const double min_eig_thr = second ? a.set[1].min_eig_thr : a.set[0].min_eig_thr;
  const double hx = (double)(win_w - 1) * 0.5, hy = (double)(win_h - 1) * 0.5;
  const double scale20 = 1.0 / 1048576.0;
  int wx[XK_KLT_SLOTS], wy[XK_KLT_SLOTS], Iw[XK_KLT_SLOTS], gx[XK_KLT_SLOTS], gy[XK_KLT_SLOTS];
#pragma unroll
  for (int s = 0; s < XK_KLT_SLOTS; ++s) {
    const int idx = min(s * 64 + lane, npix - 1);
    wy[s] = idx / win_w;
    wx[s] = idx - wy[s] * win_w;
    Iw[s] = 0; gx[s] = 0; gy[s] = 0;
  }
  int status = 1;
  double min_eig_out = 0.0, nx = 0.0, ny = 0.0;
  for (int l = levels; l >= 0; --l) {
    const XkKltLevel P = a.prev.lv[l];
    const unsigned char *J = a.cur.lv[l].img;
    const int W = P.w, H = P.h, pitch = P.pitch;
    const double scale = 1.0 / (double)(1 << l);
    double qx = px * scale, qy = py * scale;
    if (l == levels) { nx = qx; ny = qy; } else { nx = 2.0 * nx; ny = 2.0 * ny; }
    qx -= hx; qy -= hy;
    double fx = floor(qx), fy = floor(qy);
    if (!xk_klt_corner_ok(fx, fy, W, H, win_w, win_h)) {
      if (l == 0) { status = 0; min_eig_out = 0.0; }
      continue;
    }
    int ix = (int)fx, iy = (int)fy;
    XkKltW wt = xk_klt_weights(qx - fx, qy - fy);
    bool interior = ix >= 0 && iy >= 0 && ix + win_w < W && iy + win_h < H;
    int s11 = 0, s12 = 0, s22 = 0;
#pragma unroll
    for (int s = 0; s < XK_KLT_SLOTS; ++s) {
      if (s * 64 < npix) {                                       // (the same in every lane)
        const bool mine = s * 64 + lane < npix;
        const int x0 = ix + wx[s], y0 = iy + wy[s];
        const int vi = xk_klt_image_sample(P.img, W, H, pitch, x0, y0, interior, wt);
        const int vx = xk_klt_deriv_sample(P.dx, W, H, pitch, x0, y0, interior, wt);
        const int vy = xk_klt_deriv_sample(P.dy, W, H, pitch, x0, y0, interior, wt);
        Iw[s] = mine ? vi : 0; gx[s] = mine ? vx : 0; gy[s] = mine ? vy : 0;
        s11 += gx[s] * gx[s]; s12 += gx[s] * gy[s]; s22 += gy[s] * gy[s];
      }
    }
    const double A11 = (double)xk_klt_wave_sum(s11) * scale20, A12 = (double)xk_klt_wave_sum(s12) * scale20,
                 A22 = (double)xk_klt_wave_sum(s22) * scale20;
    const double D = A11 * A22 - A12 * A12;
    const double dA = A11 - A22;
    const double min_eig = (A22 + A11 - sqrt(dA * dA + 4.0 * A12 * A12)) / (double)(2 * win_w * win_h);
    if (l == 0) min_eig_out = min_eig;
    if (min_eig < min_eig_thr || D < 1.1920928955078125e-07) {  // 2^-23, FLT_EPSILON
      if (l == 0) status = 0;
      continue;
    }
    nx -= hx; ny -= hy;
    double pdx = 0.0, pdy = 0.0;
    for (int j = 0; j < a.max_iter; ++j) {
      fx = floor(nx); fy = floor(ny);
      if (!xk_klt_corner_ok(fx, fy, W, H, win_w, win_h)) {
        if (l == 0) status = 0;
        break;
      }
      ix = (int)fx; iy = (int)fy;
      wt = xk_klt_weights(nx - fx, ny - fy);
      interior = ix >= 0 && iy >= 0 && ix + win_w < W && iy + win_h < H;
      int t1 = 0, t2 = 0;
#pragma unroll
      for (int s = 0; s < XK_KLT_SLOTS; ++s) {
        if (s * 64 < npix) {
          const int d = xk_klt_image_sample(J, W, H, pitch, ix + wx[s], iy + wy[s], interior, wt) - Iw[s];
          t1 += d * gx[s]; t2 += d * gy[s];                      // (gx = gy = 0 in a lane past the window's end)
        }
      }
      const double b1 = (double)xk_klt_wave_sum(t1) * scale20, b2 = (double)xk_klt_wave_sum(t2) * scale20;
      const double dx = (A12 * b2 - A22 * b1) / D, dy = (A12 * b1 - A11 * b2) / D;
      nx += dx; ny += dy;
      if (dx * dx + dy * dy <= a.eps2) break;
      if (j > 0 && fabs(dx + pdx) < 0.01 && fabs(dy + pdy) < 0.01) {
        nx -= dx * 0.5; ny -= dy * 0.5;
        break;
      }
      pdx = dx; pdy = dy;
    }
    nx += hx; ny += hy;
  }
  if (lane == 0) { a.cur_xy[2 * f] = nx; a.cur_xy[2 * f + 1] = ny; a.status[f] = (unsigned char)status; a.min_eig[f] = min_eig_out; }
}

__global__ __launch_bounds__(256) void xk_klt_compact(XkKltArgs a) {
  const double xmax = (double)a.cur.lv[0].w - 0.5, ymax = (double)a.cur.lv[0].h - 0.5;
  double x = 0.0, y = 0.0;                     // of this thread's index: loaded by the predicate, written by the writer
  const int kept = xk_ransac_compact(
      xk_dev_count(a.n_dev, a.n),
      [&](int i) {
        x = a.cur_xy[2 * i]; y = a.cur_xy[2 * i + 1];
        return a.status[i] != 0 && x >= -0.5 && y >= -0.5 && x <= xmax && y <= ymax;
      },
      [&](int i, int pos) {
        a.kept.keep_idx[pos] = i;
        a.kept.kept_prev[2 * pos] = (double)a.pts[2 * i]; a.kept.kept_prev[2 * pos + 1] = (double)a.pts[2 * i + 1];
        a.kept.kept_cur[2 * pos] = x; a.kept.kept_cur[2 * pos + 1] = y;
      });
  if (threadIdx.x == 0) a.kept.res[0] = kept;
}
