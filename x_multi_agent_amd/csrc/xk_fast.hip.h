// xk_fast.hip.h -- FAST corner detection and the neighbourhood selection of the tracker's new features,
// Tracker::featureDetection (gfx950).
//
//   cv::FAST(img, keypoints, fast_detection_delta_, non_max_supp_)                     (tracker.cpp:441-448)
//   isFeatureInsideBorder, the sort by score                                           (tracker.cpp:459-486, :536-552)
//   computeNeighborhoodMask + appendNonNeighborFeatures                                (tracker.cpp:494-534, :564-590)
//
// The algorithm is this project's own statement of those calls, restated in NumPy by tests/fast_np.py.  Every
// quantity is an integer, so the device and the restatement agree bit for bit.
//
// Per detection, three launches on the handle's stream:
//   xk_fast_score       one thread per pixel, four pixels per thread: a 64 x 16 tile with its 3-pixel halo goes to LDS four bytes
//                       at a time where the four lie inside the row.  Two 16-bit masks (circle pixel brighter than I + t, darker
//                       than I - t) settle the 9-of-16 segment test in a few bit operations; only a pixel that passes computes the
//                       score s = max over the 16 arcs of the arc's smallest |difference|, - 1.  Writes the score image S (0 at
//                       every pixel that is no corner) and zeroes the candidate counter for the next kernel.
//   xk_fast_candidates  one thread per pixel of S: non-maximum suppression against the eight neighbours, the border test, and the
//                       key ((255 - s) << 24) | (y W + x) appended to the key list through ONE atomic counter.  The list's order
//                       is therefore open -- the sort below closes it, the keys being unique -- and a key past the list's capacity
//                       is counted but not stored, so an overflow is reported with the exact count.
//   xk_fast_select      ONE workgroup of 1024: the keys sorted ascending by a bitonic network in LDS (score descending, raster
//                       order within a score), the old features' boxes painted into the blocked mask (bits; atomic OR, which
//                       commutes), then wavefront 0 alone walks the sorted list 64 candidates at a time: every lane tests its
//                       candidate against the mask, and while the ballot of the untested survivors is not empty its lowest lane
//                       accepts, the accepted box is painted for the later chunks, and the lanes within b of it withdraw -- a
//                       compare in registers against the accepted pixel, broadcast by a cross-lane move.  No cap on the rounds: a
//                       chain of N dependent decisions costs N rounds and is exact.
// The blocked mask is W H bits.  It lives in LDS behind the keys when both fit 160 KiB - 512, otherwise in global memory; the
// kernel reaches either through one generic pointer.  In global memory it is written and read by the one workgroup only, and
// after the barrier that ends the sort by wavefront 0 only; see xk_fast_select for why those reads see those writes.
// No workgroup waits on another one, no inline assembly, no atomic whose order could change a result.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define XK_FAST_TW 64                        // tile of xk_fast_score
#define XK_FAST_TH 16
#define XK_FAST_ROWS (XK_FAST_TH + 6)
#define XK_FAST_COLS (XK_FAST_TW + 8)        // image columns tx0 - 4 ... tx0 + 67: a multiple of four on both sides
#define XK_FAST_SEL_T 1024                   // threads of xk_fast_select
#define XK_FAST_MAX_CAND 32768
#define XK_FAST_LDS_MAX (160 * 1024 - 512)

struct XkFastArgs {
  const unsigned char *img;                  // level 0 of the slot: [h][pitch]
  int w, h, pitch;
  unsigned char *S;                          // score image [h][pitch]
  unsigned int *keys;                        // [max_candidates]: as found, then sorted in place
  int *count;                                // candidates found, those past max_candidates included
  unsigned int *mask_g;                      // the blocked mask in global memory, NULL: in LDS behind the keys
  int key_cap;                               // keys the LDS holds: max_candidates rounded up to a power of two, >= 64
  int wpr;                                   // mask words per image row
  const double *old_xy;                      // [n_old][2]
  int n_old;
  int threshold, nms, b, margin, max_candidates, max_matches;
  int *res;                                  // n_found, n_candidates, 0, 0 | xy [max_matches][2] | score [max_matches]
  const int *n_old_dev;                      // NULL: n_old old features.  Else n_old is their bound, *n_old_dev the count (xk_dev_count)
  const int *pred;                           // NULL: run.  Else the three kernels return at once where *pred is 0 (the frame's re-detection)
  const int *alt_on;                         // NULL: `threshold`, by value.  Else alt_threshold where *alt_on is not 0 (the photometric frame:
  int alt_threshold;                         //   fast_detection_delta_photo_ once the calibration is done, tracker.cpp:848)
};

// any nine contiguous bits set in the 16-bit ring m
__device__ __forceinline__ bool xk_fast_arc9(unsigned int m) {
  unsigned int r = m | (m << 16);
  const unsigned int m32 = r;
  r &= r >> 1;                               // 2 in a row
  r &= r >> 2;                               // 4
  r &= r >> 4;                               // 8
  r &= m32 >> 8;                             // 9
  return (r & 0xFFFFu) != 0u;
}

// max over the 16 arcs of the smallest of the arc's nine values
__device__ __forceinline__ int xk_fast_arc_maxmin(const int (&d)[16]) {
  int a[16], b[16], c[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) a[k] = min(d[k], d[(k + 1) & 15]);
#pragma unroll
  for (int k = 0; k < 16; ++k) b[k] = min(a[k], a[(k + 2) & 15]);
#pragma unroll
  for (int k = 0; k < 16; ++k) c[k] = min(b[k], b[(k + 4) & 15]);
  int best = -256;
#pragma unroll
  for (int k = 0; k < 16; ++k) best = max(best, min(c[k], d[(k + 8) & 15]));
  return best;
}

__global__ __launch_bounds__(256) void xk_fast_score(XkFastArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char s_in[XK_FAST_ROWS][XK_FAST_COLS];
  if (a.pred && *a.pred == 0) return;                                               // (the same in every thread)
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *a.count = 0;       // (read by the next launch)
  const int w = a.w, h = a.h, pitch = a.pitch;
  const int tx0 = blockIdx.x * XK_FAST_TW, ty0 = blockIdx.y * XK_FAST_TH;
  const int cx0 = tx0 - 4, cy0 = ty0 - 3;
  for (int i = threadIdx.x; i < XK_FAST_ROWS * (XK_FAST_COLS / 4); i += 256) {
    const int r = i / (XK_FAST_COLS / 4), g = i - r * (XK_FAST_COLS / 4);
    const int y = cy0 + r, x = cx0 + 4 * g;
    uchar4 v = make_uchar4(0, 0, 0, 0);                          // (outside the image: never a pixel anyone scores)
    if (y >= 0 && y < h) {
      const unsigned char *row = a.img + (size_t)y * pitch;
      if (x >= 0 && x + 3 < w) {
        v = *reinterpret_cast<const uchar4 *>(row + x);          // (x, pitch and the slot's base are multiples of four)
      } else {
        if ((unsigned)x < (unsigned)w) v.x = row[x];
        if ((unsigned)(x + 1) < (unsigned)w) v.y = row[x + 1];
        if ((unsigned)(x + 2) < (unsigned)w) v.z = row[x + 2];
        if ((unsigned)(x + 3) < (unsigned)w) v.w = row[x + 3];
      }
    }
    *reinterpret_cast<uchar4 *>(&s_in[r][4 * g]) = v;
  }
  __syncthreads();
  const int cdx[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
  const int cdy[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
  const int lx = threadIdx.x & 63, x = tx0 + lx;
  const int t = (a.alt_on && *a.alt_on != 0) ? a.alt_threshold : a.threshold;
#pragma unroll
  for (int q = 0; q < XK_FAST_TH / 4; ++q) {
    const int ly = (threadIdx.x >> 6) + 4 * q, y = ty0 + ly;
    if (x >= w || y >= h) continue;
    int s = 0;
    if (x >= 3 && x < w - 3 && y >= 3 && y < h - 3) {
      const unsigned char *p = &s_in[ly + 3][lx + 4];
      const int c = p[0];
      int d[16];
      unsigned int brighter = 0u, darker = 0u;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        d[k] = (int)p[cdy[k] * XK_FAST_COLS + cdx[k]] - c;
        brighter |= (d[k] > t ? 1u : 0u) << k;
        darker |= (d[k] < -t ? 1u : 0u) << k;
      }
      if (xk_fast_arc9(brighter) || xk_fast_arc9(darker)) {
        int e[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) e[k] = -d[k];
        s = max(xk_fast_arc_maxmin(d), xk_fast_arc_maxmin(e)) - 1;      // >= t here, <= 254
      }
    }
    a.S[(size_t)y * pitch + x] = (unsigned char)s;
  }
}

__global__ __launch_bounds__(256) void xk_fast_candidates(XkFastArgs a) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int w = a.w, h = a.h, pitch = a.pitch;
  if (a.pred && *a.pred == 0) return;
  if (x < 3 || x >= w - 3 || y < 3 || y >= h - 3) return;         // (S is 0 on the 3-pixel frame; inside it every neighbour exists)
  if (x < a.margin || x > w - a.margin - 1 || y < a.margin || y > h - a.margin - 1) return;
  const unsigned char *p = a.S + (size_t)y * pitch + x;
  const int s = p[0];
  if (s == 0) return;
  if (a.nms) {
    const int m = max(max(max((int)p[-pitch - 1], (int)p[-pitch]), max((int)p[-pitch + 1], (int)p[-1])),
                      max(max((int)p[1], (int)p[pitch - 1]), max((int)p[pitch], (int)p[pitch + 1])));
    if (s <= m) return;
  }
  const int pos = atomicAdd(a.count, 1);                            // (the order of the list is open; xk_fast_select sorts it)
  if (pos < a.max_candidates) a.keys[pos] = ((unsigned int)(255 - s) << 24) | (unsigned int)(y * w + x);
}

// The bits of the box [x0, x1] x [y0, y1] (inside the image) set, one (row, word) per lane and turn: within one call no two lanes
// touch the same word.  ATOMIC: several calls may run at once (the old features' boxes, one per wavefront).
template <bool ATOMIC>
__device__ __forceinline__ void xk_fast_paint(unsigned int *mask, int wpr, int x0, int x1, int y0, int y1, int lane) {
  const int w0 = x0 >> 5, nw = (x1 >> 5) - w0 + 1, items = nw * (y1 - y0 + 1);
  for (int i = lane; i < items; i += 64) {
    const int r = i / nw, wi = w0 + (i - r * nw);
    const int lo = max(x0 - 32 * wi, 0), hi = min(x1 - 32 * wi, 31);
    const unsigned int bits = (0xFFFFFFFFu >> (31 - hi)) & (0xFFFFFFFFu << lo);
    unsigned int *p = mask + (size_t)(y0 + r) * wpr + wi;
    if (ATOMIC) atomicOr(p, bits);
    else *p |= bits;
  }
}

__global__ __launch_bounds__(XK_FAST_SEL_T) void xk_fast_select(XkFastArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned int xk_fast_sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (a.pred && *a.pred == 0) return;                               // (the same in every thread: before any barrier)
  const int n_old = xk_dev_count(a.n_old_dev, a.n_old);
  const int n = *a.count;
  if (n > a.max_candidates) {                                       // reported, nothing selected
    if (tid == 0) { a.res[0] = 0; a.res[1] = n; }
    return;
  }
  int np = 64;
  while (np < n) np <<= 1;                                          // <= key_cap
  unsigned int *keys = xk_fast_sm;
  unsigned int *mask = a.mask_g ? a.mask_g : xk_fast_sm + a.key_cap;   // (a generic pointer: LDS or global memory)
  const int w = a.w, h = a.h, b = a.b, wpr = a.wpr;
  for (int i = tid; i < np; i += XK_FAST_SEL_T) keys[i] = i < n ? a.keys[i] : 0xFFFFFFFFu;
  for (int i = tid; i < wpr * h; i += XK_FAST_SEL_T) mask[i] = 0u;
  __syncthreads();
  // computeNeighborhoodMask: one old feature per wavefront and turn, its box clipped to the image.  The clipping is done in fp64
  // so that it also decides for coordinates no int holds.
  for (int f = wave; f < n_old; f += XK_FAST_SEL_T / 64) {
    const double ox = a.old_xy[2 * f], oy = a.old_xy[2 * f + 1];
    if (!(isfinite(ox) && isfinite(oy))) continue;
    const double rx = round(ox), ry = round(oy);                    // half away from zero
    const double x0 = fmax(rx - (double)b, 0.0), x1 = fmin(rx + (double)b, (double)(w - 1));
    const double y0 = fmax(ry - (double)b, 0.0), y1 = fmin(ry + (double)b, (double)(h - 1));
    if (x0 > x1 || y0 > y1) continue;
    xk_fast_paint<true>(mask, wpr, (int)x0, (int)x1, (int)y0, (int)y1, lane);
  }
  // bitonic sort, ascending; the padding keys 0xFFFFFFFF are larger than every real key (a real key's pixel index is < 2^24)
  for (int k = 2; k <= np; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < np / 2; t += XK_FAST_SEL_T) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        const unsigned int u = keys[i], v = keys[p];
        if ((u > v) == ((i & k) == 0)) { keys[i] = v; keys[p] = u; }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < n; i += XK_FAST_SEL_T) a.keys[i] = keys[i];   // for xk_trk_detect_stage
  if (wave != 0) return;                                            // (no barrier below)
  // appendNonNeighborFeatures.  Wavefront 0 alone reads and writes the mask from here on.  The old boxes were written before
  // the barriers above, which order them at workgroup scope.  A box painted below is read back by this same wavefront in a later
  // chunk, possibly by another lane: in LDS a wavefront's accesses complete in order; in global memory the workgroup-scope
  // fence after each paint keeps the later loads behind the stores, and the whole workgroup shares one compute unit's L1, which
  // the stores write through, so no other cache holds an older copy.
  int *out_xy = a.res + 4, *out_score = a.res + 4 + 2 * a.max_matches;
  int n_acc = 0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    const bool valid = i < n;
    const unsigned int key = valid ? keys[i] : 0u;
    const int pix = (int)(key & 0xFFFFFFu), y = pix / w, x = pix - y * w;
    bool alive = valid && ((mask[(size_t)y * wpr + (x >> 5)] >> (x & 31)) & 1u) == 0u;
    for (;;) {
      const unsigned long long bal = __ballot(alive);
      if (bal == 0ull) break;
      const int l = __ffsll((long long)bal) - 1;
      const int ax = __shfl(x, l, 64), ay = __shfl(y, l, 64);
      if (lane == l && n_acc < a.max_matches) {
        out_xy[2 * n_acc] = x; out_xy[2 * n_acc + 1] = y;
        out_score[n_acc] = 255 - (int)(key >> 24);
      }
      ++n_acc;                                                      // (counted past max_matches: the overflow is reported exactly)
      xk_fast_paint<false>(mask, wpr, max(ax - b, 0), min(ax + b, w - 1), max(ay - b, 0), min(ay + b, h - 1), lane);
      __threadfence_block();                                        // (the next paint and the next chunk read these words)
      alive = alive && !(abs(x - ax) <= b && abs(y - ay) <= b);     // (lane l itself withdraws here)
    }
  }
  if (lane == 0) { a.res[0] = n_acc; a.res[1] = n; }
}
