// xk_orb.hip.h -- rotated-BRIEF (ORB) descriptors of keypoints on level 0 of an image slot (gfx950).
//
//   PlaceRecognition::compute -> cv::ORB::compute(img, keypoints, descriptors)         (place_recognition.cpp:72-94, tracker.cpp:440-444)
//
// The algorithm is this project's own statement of that call, restated in NumPy by tests/orb_np.py.  Every
// quantity is an integer but the one square root and the two divisions of the centroid direction, which are correctly rounded
// fp64 operations on exact operands, so the device and the restatement agree bit for bit.
//
// Per description, on the handle's stream:
//   xk_orb_blur      once per pushed image, before its first description: G = the image under the separable 7-tap kernel
//                    {18, 34, 49, 54, 49, 34, 18} / 256, both passes in one launch.  A 64 x 16 tile with its 3-pixel apron
//                    (reflected at the image's border without repeating the edge pixel) goes to LDS, the horizontal pass leaves
//                    unrounded 16-bit sums in LDS, the vertical pass sums them in 32 bits and rounds once, (s + 32768) >> 16.
//   xk_orb_filter    ONE workgroup: KeyPointsFilter::runByImageBorder (edge <= x < W - edge, edge <= y < H - edge) and the ORDERED
//                    compaction of the kept keypoints (xk_ransac_compact).  It comes before any read of the image: a kept keypoint's
//                    samples lie within 22 pixels of it and edge >= 25, so nothing below needs a bounds test.
//   xk_orb_describe  one wavefront per kept keypoint, a grid-stride loop over them.  Centroid mode: the lanes split the 31 x 31 box
//                    around the keypoint, the pixels of the disc (|u| <= umax[|v|]) add u I and v I, a butterfly leaves both int32
//                    sums in every lane, and (A, B) = rint(16384 m / |m|) comes from __dsqrt_rn and __ddiv_rn.  Then four rounds:
//                    lane l evaluates pair 64 j + l and the 64-bit ballot of sample1 < sample2 IS bytes 8j ... 8j + 7 of the
//                    descriptor (lane l is bit l & 7 of byte l >> 3 of a little-endian word).  Four 8-byte stores per keypoint.
// The samples are read straight from G in global memory: eight byte loads per lane and keypoint out of a 45 x 45 footprint that the
// wavefront has to itself in the L1.  Staging that patch in LDS would move four times as many bytes (2025 against 512) before the
// first comparison; the choice was made by that count and was not measured against the alternative.
// No workgroup waits on another one, no inline assembly, no atomic.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "xk_ransac.hip.h"     // the ordered compaction

#define XK_ORB_TW 64                         // tile of xk_orb_blur
#define XK_ORB_TH 16
#define XK_ORB_ROWS (XK_ORB_TH + 6)
#define XK_ORB_COLS (XK_ORB_TW + 8)          // image columns tx0 - 4 ... tx0 + 67: a multiple of four on both sides
#define XK_ORB_WAVES 4                       // wavefronts (keypoints in flight) per workgroup of xk_orb_describe
#define XK_ORB_MAX_GRID 512                  // workgroups of xk_orb_describe: beyond 2048 keypoints the wavefronts take several
#define XK_ORB_MAX_DESC 32768
#define XK_ORB_HALF 15                       // the pattern and the moments reach 15 pixels

struct XkOrbArgs {
  const unsigned char *img;                  // level 0 of the slot: [h][pitch]
  unsigned char *G;                          // its blur, [h][pitch]
  int w, h, pitch;
  const int *xy;                             // [n][2] as the caller gave them
  int n, edge;
  int centroid, A, B;                        // orientation mode; the fixed direction in Q14
  const signed char *pattern;                // [256][4]: x1 y1 x2 y2
  int *kept_xy;                              // [max_desc][2]: the kept keypoints, in input order
  int *res;                                  // n_kept, 0, 0, 0 | keep_idx [n] | dir [n][2] | moments [n][2] | desc [n][32]
  const int *n_dev;                          // NULL: n keypoints.  Else n is the bound the block is laid out by, *n_dev the count (xk_dev_count)
  const int *pred;                           // NULL: blur.  Else xk_orb_blur returns at once where *pred is 0 (the frame's re-detection)
};
// the result block for n keypoints; desc starts at a multiple of 8 (res itself is 16-byte aligned)
inline __host__ __device__ size_t xk_orb_desc_off(size_t n) { return (sizeof(int) * (4 + 5 * n) + 7) / 8 * 8; }
inline size_t xk_orb_res_bytes(size_t n) { return xk_orb_desc_off(n) + 32 * n; }

// index -k -> k, n - 1 + k -> n - 1 - k; then held inside the image (the tile's columns no output needs)
__device__ __forceinline__ int xk_orb_reflect(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * (n - 1) - i : i;
  return min(max(i, 0), n - 1);
}

__global__ __launch_bounds__(256) void xk_orb_blur(XkOrbArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char s_in[XK_ORB_ROWS][XK_ORB_COLS];
  __shared__ unsigned short s_h[XK_ORB_ROWS][XK_ORB_TW];
  const int w = a.w, h = a.h, pitch = a.pitch;
  if (a.pred && *a.pred == 0) return;                            // (the same in every thread)
  const int tx0 = blockIdx.x * XK_ORB_TW, ty0 = blockIdx.y * XK_ORB_TH;
  const int cx0 = tx0 - 4, cy0 = ty0 - 3;
  for (int i = threadIdx.x; i < XK_ORB_ROWS * (XK_ORB_COLS / 4); i += 256) {
    const int r = i / (XK_ORB_COLS / 4), g = i - r * (XK_ORB_COLS / 4);
    const int x = cx0 + 4 * g;
    const unsigned char *row = a.img + (size_t)xk_orb_reflect(cy0 + r, h) * pitch;
    uchar4 v;
    if (x >= 0 && x + 3 < w) {
      v = *reinterpret_cast<const uchar4 *>(row + x);            // (x, pitch and the slot's base are multiples of four)
    } else {
      v.x = row[xk_orb_reflect(x, w)];
      v.y = row[xk_orb_reflect(x + 1, w)];
      v.z = row[xk_orb_reflect(x + 2, w)];
      v.w = row[xk_orb_reflect(x + 3, w)];
    }
    *reinterpret_cast<uchar4 *>(&s_in[r][4 * g]) = v;
  }
  __syncthreads();
  const int taps[7] = {18, 34, 49, 54, 49, 34, 18};
  for (int i = threadIdx.x; i < XK_ORB_ROWS * XK_ORB_TW; i += 256) {
    const int r = i >> 6, lx = i & 63;
    const unsigned char *p = &s_in[r][lx + 1];                   // image column tx0 + lx - 3
    int s = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) s += taps[k] * (int)p[k];
    s_h[r][lx] = (unsigned short)s;                              // <= 255 * 256
  }
  __syncthreads();
  const int lx = threadIdx.x & 63, x = tx0 + lx;
#pragma unroll
  for (int q = 0; q < XK_ORB_TH / 4; ++q) {
    const int ly = (threadIdx.x >> 6) + 4 * q, y = ty0 + ly;
    if (x >= w || y >= h) continue;
    int s = 32768;
#pragma unroll
    for (int k = 0; k < 7; ++k) s += taps[k] * (int)s_h[ly + k][lx];
    a.G[(size_t)y * pitch + x] = (unsigned char)(s >> 16);
  }
}

__global__ __launch_bounds__(256) void xk_orb_filter(XkOrbArgs a) {
  const int w = a.w, h = a.h, edge = a.edge;
  int x = 0, y = 0;
  const int kept = xk_ransac_compact(
      xk_dev_count(a.n_dev, a.n),
      [&](int i) {
        x = a.xy[2 * i]; y = a.xy[2 * i + 1];
        return x >= edge && x < w - edge && y >= edge && y < h - edge;
      },
      [&](int i, int pos) {
        a.res[4 + pos] = i;
        a.kept_xy[2 * pos] = x; a.kept_xy[2 * pos + 1] = y;
      });
  if (threadIdx.x == 0) a.res[0] = kept;
}

// round half away from zero of v / 16384
__device__ __forceinline__ int xk_orb_r14(int v) {
  const int m = (abs(v) + 8192) >> 14;
  return v < 0 ? -m : m;
}

__global__ __launch_bounds__(64 * XK_ORB_WAVES) void xk_orb_describe(XkOrbArgs a) {
  const int lane = threadIdx.x & 63;
  const int n_kept = a.res[0];                                    // (written by the launch before)
  const int pitch = a.pitch;
  int *dir = a.res + 4 + a.n, *mom = dir + 2 * (size_t)a.n;
  unsigned long long *desc = reinterpret_cast<unsigned long long *>(reinterpret_cast<unsigned char *>(a.res) + xk_orb_desc_off((size_t)a.n));
  for (int k = blockIdx.x * XK_ORB_WAVES + (threadIdx.x >> 6); k < n_kept; k += gridDim.x * XK_ORB_WAVES) {
    const int x = a.kept_xy[2 * k], y = a.kept_xy[2 * k + 1];
    int A = a.A, B = a.B, m10 = 0, m01 = 0;
    if (a.centroid) {
      const int umax[XK_ORB_HALF + 1] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
      const unsigned char *c = a.img + (size_t)y * pitch + x;
      for (int i = lane; i < 31 * 31; i += 64) {
        const int r = i / 31, v = r - XK_ORB_HALF, u = i - 31 * r - XK_ORB_HALF;
        if (abs(u) <= umax[abs(v)]) {
          const int I = c[v * pitch + u];
          m10 += u * I;
          m01 += v * I;
        }
      }
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) {                          // exact in int32: at most 749 pixels of 15 * 255
        m10 += __shfl_xor(m10, s, 64);
        m01 += __shfl_xor(m01, s, 64);
      }
      A = 16384; B = 0;
      if (m10 != 0 || m01 != 0) {
        const double hyp = __dsqrt_rn((double)((long long)m10 * m10 + (long long)m01 * m01));   // (the argument < 2^53)
        A = (int)rint(__ddiv_rn((double)m10 * 16384.0, hyp));
        B = (int)rint(__ddiv_rn((double)m01 * 16384.0, hyp));
      }
    }
    if (lane == 0) {
      dir[2 * k] = A; dir[2 * k + 1] = B;
      mom[2 * k] = m10; mom[2 * k + 1] = m01;
    }
    const unsigned char *g = a.G + (size_t)y * pitch + x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const char4 p = reinterpret_cast<const char4 *>(a.pattern)[64 * j + lane];
      const int s1 = g[xk_orb_r14(p.x * B + p.y * A) * pitch + xk_orb_r14(p.x * A - p.y * B)];
      const int s2 = g[xk_orb_r14(p.z * B + p.w * A) * pitch + xk_orb_r14(p.z * A - p.w * B)];
      const unsigned long long bits = __ballot(s1 < s2);
      if (lane == 0) desc[4 * (size_t)k + j] = bits;
    }
  }
}
