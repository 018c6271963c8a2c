// xk_frame.hip.h -- the glue of one frame of Tracker::track (tracker.cpp:134-306) on a feature list that stays on the device (gfx950).
//
// The stages of a frame have kernels of their own (xk_klt, xk_fast, xk_orb, xk_fundamental .hip.h).  xk_trk_frame queues them on one
// stream with their counts in device memory (xk_dev_count) and these kernels between them:
//   xk_frame_overflow   one workgroup: Tracker::removeOverflowFeatures (tracker.cpp:592-620) behind the tracking's post-filter.  The
//                       tiles of both features by the fp64 subtraction loops of TiledImage::setTileForFeature (tiled_image.cpp:139-158),
//                       bounded by the tile counts; the histogram of the CURRENT features' tiles in LDS by integer atomics; then the
//                       ordered compaction.  The reference's second loop runs on i - 1 from size - 1 down, so the last pair is never
//                       examined, and it reads counts that stay as counted while pairs are erased: the erase mask is a pure function
//                       of the histogram.  Score, descriptor and origin move with their pair in the compaction's put.  Writes the
//                       re-detection flag (fewer than n_feat_min pairs left, tracker.cpp:204).
//   xk_frame_gate       one workgroup, the re-detection predicate: returns at once where the flag is clear; otherwise takes the
//                       detection's counts, decides the capacity errors and leaves the count the description and the second tracking
//                       run on (0 after an error: they then return past it), and the new features' pixels as the float points the
//                       tracking takes
//   xk_frame_concat     one workgroup: the newly tracked pairs behind the old ones (tracker.cpp:222-227), their score, descriptor,
//                       origin -(k + 1) and the tile the detection gave the previous feature (tracker.cpp:578)
//   xk_frame_pack       the kept pairs of the RANSAC into the result block, and the kept current features into the resident list
//                       (tracker.cpp:299)
//   xk_frame_first      the first frame: the detected features become the resident list
//   xk_frame_trunc      (photometric frame) the kept current points of a tracking truncated to the integer pixels
//                       Tracker::computeIntensity is asked at (tracker.cpp:666), for xk_photo_intensity behind it
// The photometric frame (xk_trk_photo_frame, Tracker::track of a PHOTOMETRIC_CALI build) runs the same kernels with the optional
// pointers of XkFrameArgs set: every pair then carries the intensity of its previous and of its current feature, the resident
// list the intensity of each feature, and the head of the result block the outcome of the frame's calibration.
// No kernel waits on another: every count and flag is a plain load of what an earlier launch on the same stream wrote.  Integer
// atomics on LDS only; no inline assembly.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "xk_orb.hip.h"
#include "xk_photo.hip.h"
#include "xk_ransac.hip.h"

// the frame's counts in device memory, and the head of the result block in the same order
enum {
  XK_FC_TRACKED = 0,     // pairs the tracking's post-filter kept
  XK_FC_LEFT,            // pairs left by the overflow pass
  XK_FC_REDETECT,        // 1: fewer than n_feat_min were left
  XK_FC_CAND,            // candidates of the re-detection (or of the first frame's detection)
  XK_FC_ACCEPTED,        // features it accepted
  XK_FC_NEW_TRACKED,     // of those, tracked into the current image
  XK_FC_TOTAL,           // pairs into the outlier removal
  XK_FC_MATCHES,         // pairs it kept
  XK_FC_WINNER,          // its winning hypothesis, -1: none
  XK_FC_STATUS,          // 0, or an XK_FRAME_E* below
  XK_FC_NEW,             // what the description and the second tracking run on: ACCEPTED, 0 after an error or without a re-detection
  // the photometric frame only, head of the result block only (zero otherwise): the outcome of the frame's calibration
  XK_FC_CAL_KEPT,        // points its tracking between the raw images kept
  XK_FC_ESTIMATED,       // 1: it estimated gains and the ring advanced
  XK_FC_DONE,            // XkPhotoState::done after it
  XK_FC_SUPPORT,         // inliers of the refit
  XK_FC_RING_N,          // the ring's size after it
  XK_FC_N = 16
};
#define XK_FRAME_ECAND 1       // more candidates than max_candidates
#define XK_FRAME_EACCEPTED 2   // more features accepted than max_matches
#define XK_FRAME_EDESC 3       // more keypoints than max_desc
#define XK_FRAME_ETOTAL 4      // old plus new pairs exceed max_matches
#define XK_FRAME_MAX_TILES 4096

struct XkFrameArgs {
  int B;                         // the host's bound on the pairs of this frame: every list below is laid out by it
  int n_res;                     // the resident count, known to the host: the previous frame's matches
  int first;                     // 1: the first frame (xk_frame_gate has no flag to ask)
  int n_feat_min, tiles_h, tiles_w, max_per_tile;
  double tile_w, tile_h, height; // tiled_image.cpp:104-105
  int cap_new;                   // the bound of the re-detection's lists: the detection's packing bound, max_desc with a description
  int max_candidates, max_matches, max_desc;   // max_desc 0: no description
  int *c;                        // [XK_FC_N]
  // the resident list [max_matches]: distorted pixels, their float cast (what the tracking takes), FAST score, descriptor
  double *res_dist;
  float *res_pts;
  int *res_score;
  unsigned char *res_desc;       // [max_matches][32], NULL without a description
  // the frame's pair lists [B]: previous and current distorted pixels (the current list 2 B doubles behind the previous one, as
  // xk_fund_undistort takes them), and what follows each pair
  double *l_prev, *l_cur;
  int *l_score, *l_origin, *l_tiles;   // tiles: previous row, previous column, current row, current column
  unsigned char *l_desc;
  int *tmp_tiles;                // [B][4]: of the pairs before the overflow pass
  XkKeptPairs kept1, kept2, kept3;   // of the tracking, the second tracking, the outlier removal
  const double *und;             // [2 B][2] undistorted pixels of both lists
  int *det_res;                  // the detection's result block (XkFastArgs::res)
  const int *orb_res;            // the description's (XkOrbArgs::res), laid out by cap_new
  float *pts_new;                // [cap_new][2]
  unsigned char *out;            // the result block, xk_frame_out_*
  // The photometric frame; res_int NULL: none of these is read.  fp64 box means as xk_photo_intensity leaves them.
  double *res_int;               // [max_matches] of the resident list
  double *l_iprev, *l_icur;      // [B] of the pair lists: the previous and the current feature's
  const double *val1;            // [n_res] of the tracked current features, by kept1's position
  const double *val_new;         // [cap_new] of the features the detection accepted, by its position
  const double *val2;            // [cap_new] of the newly tracked current features, by kept2's position
  const XkPhotoState *photo_st;  // the calibration's state
  const int *cal_kept;           // the kept count of the calibration's tracking; NULL: the frame ran none (fewer than 4 resident features)
};

// The result block for bound B: head [XK_FC_N] ints | undistorted previous, current, distorted previous, current [B][2] fp64 each |
// score [B] | origin [B] | tiles [B][4] | descriptors [B][32].
inline __host__ __device__ size_t xk_frame_out_xy(size_t B, int which) { return sizeof(int) * XK_FC_N + sizeof(double) * 2 * B * (size_t)which; }
inline __host__ __device__ size_t xk_frame_out_score(size_t B) { return xk_frame_out_xy(B, 4); }
inline __host__ __device__ size_t xk_frame_out_origin(size_t B) { return xk_frame_out_score(B) + sizeof(int) * B; }
inline __host__ __device__ size_t xk_frame_out_tiles(size_t B) { return xk_frame_out_origin(B) + sizeof(int) * B; }
inline __host__ __device__ size_t xk_frame_out_desc(size_t B) { return xk_frame_out_tiles(B) + sizeof(int) * 4 * B; }   // (a multiple of 8)
inline __host__ __device__ size_t xk_frame_out_bytes(size_t B, bool desc) { return xk_frame_out_desc(B) + (desc ? 32 * B : 0); }
// The photometric frame's block: the same, then previous intensities [B] | current intensities [B] | a_rel, b_rel, frame_ab [4], fp64.
inline __host__ __device__ size_t xk_frame_out_int(size_t B, bool desc, int which) { return xk_frame_out_bytes(B, desc) + sizeof(double) * B * (size_t)which; }
inline __host__ __device__ size_t xk_frame_out_cal(size_t B, bool desc) { return xk_frame_out_int(B, desc, 2); }
inline __host__ __device__ size_t xk_frame_photo_out_bytes(size_t B, bool desc) { return xk_frame_out_cal(B, desc) + sizeof(double) * 6; }

// The calibration's outcome into the head of the photometric frame's result block (thread 0 of the packing kernel, after the counts).
__device__ __forceinline__ void xk_frame_cal_head(const XkFrameArgs &a, int *head) {
  const XkPhotoState *st = a.photo_st;
  const int est = a.cal_kept ? st->estimated : 0;                 // (without a calibration the flag is an earlier frame's)
  head[XK_FC_CAL_KEPT] = a.cal_kept ? a.cal_kept[0] : 0;
  head[XK_FC_ESTIMATED] = est;
  head[XK_FC_DONE] = st->done;
  head[XK_FC_SUPPORT] = est ? st->support[0] : 0;
  head[XK_FC_RING_N] = st->ring_n;
}

// TiledImage::setTileForFeature (tiled_image.cpp:139-158): the loops as written, each bounded by its tile count (a feature inside the
// image leaves them earlier).  The body is shared with the track store (xk_track_store.hip.h), which bins the same features.
__device__ __forceinline__ void xk_tile_for_feature(double tile_w, double tile_h, double height, int tiles_h, int tiles_w, double x, double y,
                                                    int *row, int *col) {
#pragma clang fp contract(off)
  double c = x - tile_w - 0.5;
  int cc = 0;
  for (int it = 0; it <= tiles_w && c > 0; ++it) { cc += 1; c -= tile_w; }
  double r = height - y - 0.5;
  int rr = tiles_h - 1;
  for (int it = 0; it <= tiles_h && r > tile_h; ++it) { rr -= 1; r -= tile_h; }
  *row = rr; *col = cc;
}

__device__ __forceinline__ void xk_frame_tile(const XkFrameArgs &a, double x, double y, int *row, int *col) {
  xk_tile_for_feature(a.tile_w, a.tile_h, a.height, a.tiles_h, a.tiles_w, x, y, row, col);
}

// 32 bytes, both 8-byte aligned
__device__ __forceinline__ void xk_frame_copy_desc(unsigned char *dst, const unsigned char *src) {
  const unsigned long long *s = reinterpret_cast<const unsigned long long *>(src);
  unsigned long long *d = reinterpret_cast<unsigned long long *>(dst);
  d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = s[3];
}

__global__ __launch_bounds__(256) void xk_frame_overflow(XkFrameArgs a) {
  extern __shared__ int xk_frame_hist[];                          // [tiles_h][tiles_w]
  const int n_tiles = a.tiles_h * a.tiles_w;
  const int n1 = a.n_res > 0 ? min(max(a.kept1.res[0], 0), a.n_res) : 0;   // (no tracking was launched on an empty list)
  for (int i = threadIdx.x; i < n_tiles; i += 256) xk_frame_hist[i] = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < n1; i += 256) {
    const int k = a.kept1.keep_idx[i];
    int t[4];
    xk_frame_tile(a, a.res_dist[2 * k], a.res_dist[2 * k + 1], &t[0], &t[1]);
    xk_frame_tile(a, a.kept1.kept_cur[2 * i], a.kept1.kept_cur[2 * i + 1], &t[2], &t[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) a.tmp_tiles[4 * i + j] = t[j];
    if (t[2] >= 0 && t[2] < a.tiles_h && t[3] >= 0 && t[3] < a.tiles_w) atomicAdd(&xk_frame_hist[t[2] * a.tiles_w + t[3]], 1);   // (a tile outside the grid is not counted)
  }
  __syncthreads();
  const int left = xk_ransac_compact(
      n1,
      [&](int i) {
        if (i == n1 - 1) return true;                             // the last pair is never examined
        const int r = a.tmp_tiles[4 * i + 2], c = a.tmp_tiles[4 * i + 3];
        const int count = (r >= 0 && r < a.tiles_h && c >= 0 && c < a.tiles_w) ? xk_frame_hist[r * a.tiles_w + c] : 0;
        return count <= a.max_per_tile;
      },
      [&](int i, int pos) {
        const int k = a.kept1.keep_idx[i];
        a.l_prev[2 * pos] = a.res_dist[2 * k]; a.l_prev[2 * pos + 1] = a.res_dist[2 * k + 1];
        a.l_cur[2 * pos] = a.kept1.kept_cur[2 * i]; a.l_cur[2 * pos + 1] = a.kept1.kept_cur[2 * i + 1];
        a.l_score[pos] = a.res_score[k];
        a.l_origin[pos] = k;
#pragma unroll
        for (int j = 0; j < 4; ++j) a.l_tiles[4 * pos + j] = a.tmp_tiles[4 * i + j];
        if (a.l_desc) xk_frame_copy_desc(a.l_desc + 32 * (size_t)pos, a.res_desc + 32 * (size_t)k);
        if (a.res_int) { a.l_iprev[pos] = a.res_int[k]; a.l_icur[pos] = a.val1[i]; }   // getIntensity of both features, tracker.cpp:666
      });
  if (threadIdx.x == 0) {
    for (int j = 0; j < XK_FC_N; ++j) a.c[j] = 0;
    a.c[XK_FC_TRACKED] = n1;
    a.c[XK_FC_LEFT] = left;
    a.c[XK_FC_REDETECT] = left < a.n_feat_min ? 1 : 0;
    a.c[XK_FC_WINNER] = -1;
    a.det_res[0] = 0; a.det_res[1] = 0;                           // (what a skipped detection leaves)
  }
}

__global__ __launch_bounds__(256) void xk_frame_gate(XkFrameArgs a) {
  if (a.first) {
    if (threadIdx.x < XK_FC_N && threadIdx.x != XK_FC_CAND && threadIdx.x != XK_FC_ACCEPTED && threadIdx.x != XK_FC_STATUS &&
        threadIdx.x != XK_FC_NEW)
      a.c[threadIdx.x] = threadIdx.x == XK_FC_WINNER ? -1 : 0;
  } else if (a.c[XK_FC_REDETECT] == 0) {
    return;                                                       // (the counts are zero since xk_frame_overflow)
  }
  const int found = a.det_res[0], cand = a.det_res[1];
  int status = 0;
  if (cand > a.max_candidates) status = XK_FRAME_ECAND;
  else if (found > a.max_matches) status = XK_FRAME_EACCEPTED;
  else if (a.max_desc > 0 && found > a.max_desc) status = XK_FRAME_EDESC;
  else if (found > a.cap_new || found < 0) status = XK_FRAME_EACCEPTED;   // (past the packing bound: cannot happen)
  const int n_new = status == 0 ? found : 0;
  for (int i = threadIdx.x; i < 2 * n_new; i += 256) a.pts_new[i] = (float)a.det_res[4 + i];
  if (threadIdx.x == 0) {
    a.c[XK_FC_CAND] = cand; a.c[XK_FC_ACCEPTED] = found; a.c[XK_FC_STATUS] = status; a.c[XK_FC_NEW] = n_new;
  }
}

__global__ __launch_bounds__(256) void xk_frame_concat(XkFrameArgs a) {
  const int n2 = a.c[XK_FC_LEFT], n_new = a.c[XK_FC_NEW];
  int status = a.c[XK_FC_STATUS];
  const int n3 = n_new > 0 ? min(max(a.kept2.res[0], 0), n_new) : 0;
  if (status == 0 && n2 + n3 > a.B) status = XK_FRAME_ETOTAL;     // (B = min(max_matches, resident + packing bound): past it is past max_matches)
  const int total = status == 0 ? n2 + n3 : 0;
  __syncthreads();                                                // (every thread has read the status thread 0 writes)
  const int *det_xy = a.det_res + 4, *det_score = a.det_res + 4 + 2 * (size_t)a.max_matches;
  const unsigned char *orb_desc = reinterpret_cast<const unsigned char *>(a.orb_res) + xk_orb_desc_off((size_t)a.cap_new);
  if (status == 0) {
    for (int j = threadIdx.x; j < n3; j += 256) {
      const int k = a.kept2.keep_idx[j], pos = n2 + j;
      const double x = (double)det_xy[2 * k], y = (double)det_xy[2 * k + 1];
      a.l_prev[2 * pos] = x; a.l_prev[2 * pos + 1] = y;
      a.l_cur[2 * pos] = a.kept2.kept_cur[2 * j]; a.l_cur[2 * pos + 1] = a.kept2.kept_cur[2 * j + 1];
      a.l_score[pos] = det_score[k];
      a.l_origin[pos] = -(k + 1);
      int row, col;
      xk_frame_tile(a, x, y, &row, &col);                         // tracker.cpp:578; the tracked feature is a new Feature: no tile yet
      a.l_tiles[4 * pos] = row; a.l_tiles[4 * pos + 1] = col; a.l_tiles[4 * pos + 2] = -1; a.l_tiles[4 * pos + 3] = -1;
      if (a.l_desc) xk_frame_copy_desc(a.l_desc + 32 * (size_t)pos, orb_desc + 32 * (size_t)k);   // (every accepted feature is described: margin >= edge)
      if (a.res_int) { a.l_iprev[pos] = a.val_new[k]; a.l_icur[pos] = a.val2[j]; }                // tracker.cpp:461, :666
    }
  }
  if (threadIdx.x == 0) { a.c[XK_FC_NEW_TRACKED] = n3; a.c[XK_FC_TOTAL] = total; a.c[XK_FC_STATUS] = status; }
}

__global__ __launch_bounds__(256) void xk_frame_pack(XkFrameArgs a) {
  const size_t B = (size_t)a.B;
  const int status = a.c[XK_FC_STATUS];
  const int m = status == 0 ? min(max(a.kept3.res[0], 0), min(a.c[XK_FC_TOTAL], a.B)) : 0;
  const int pos = blockIdx.x * 256 + threadIdx.x;
  if (pos == 0) {
    int *head = reinterpret_cast<int *>(a.out);
    for (int j = 0; j < XK_FC_N; ++j) head[j] = a.c[j];
    head[XK_FC_MATCHES] = m;
    head[XK_FC_WINNER] = status == 0 ? a.kept3.res[1] : -1;
    if (a.res_int) {
      xk_frame_cal_head(a, head);
      double *cal = reinterpret_cast<double *>(a.out + xk_frame_out_cal(B, a.l_desc != nullptr));
      const bool est = head[XK_FC_ESTIMATED] != 0;
      cal[0] = est ? a.photo_st->a_rel[0] : 1.0; cal[1] = est ? a.photo_st->b_rel[0] : 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j) cal[2 + j] = est ? a.photo_st->frame_ab[j] : 0.0;
    }
  }
  if (pos >= m) return;
  const int i = a.kept3.keep_idx[pos];
  double *o_up = reinterpret_cast<double *>(a.out + xk_frame_out_xy(B, 0)), *o_uc = reinterpret_cast<double *>(a.out + xk_frame_out_xy(B, 1));
  double *o_dp = reinterpret_cast<double *>(a.out + xk_frame_out_xy(B, 2)), *o_dc = reinterpret_cast<double *>(a.out + xk_frame_out_xy(B, 3));
  int *o_score = reinterpret_cast<int *>(a.out + xk_frame_out_score(B)), *o_origin = reinterpret_cast<int *>(a.out + xk_frame_out_origin(B));
  int *o_tiles = reinterpret_cast<int *>(a.out + xk_frame_out_tiles(B));
  const double cx = a.l_cur[2 * i], cy = a.l_cur[2 * i + 1];
  o_up[2 * pos] = a.und[2 * i]; o_up[2 * pos + 1] = a.und[2 * i + 1];
  o_uc[2 * pos] = a.und[2 * (B + i)]; o_uc[2 * pos + 1] = a.und[2 * (B + i) + 1];
  o_dp[2 * pos] = a.l_prev[2 * i]; o_dp[2 * pos + 1] = a.l_prev[2 * i + 1];
  o_dc[2 * pos] = cx; o_dc[2 * pos + 1] = cy;
  o_score[pos] = a.l_score[i];
  o_origin[pos] = a.l_origin[i];
#pragma unroll
  for (int j = 0; j < 4; ++j) o_tiles[4 * pos + j] = a.l_tiles[4 * i + j];
  // previous_features_ = current_features (tracker.cpp:299)
  a.res_dist[2 * pos] = cx; a.res_dist[2 * pos + 1] = cy;
  a.res_pts[2 * pos] = (float)cx; a.res_pts[2 * pos + 1] = (float)cy;   // Feature::getDistPoint2f, tracker.cpp:629-633
  a.res_score[pos] = a.l_score[i];
  if (a.l_desc) {
    xk_frame_copy_desc(a.out + xk_frame_out_desc(B) + 32 * (size_t)pos, a.l_desc + 32 * (size_t)i);
    xk_frame_copy_desc(a.res_desc + 32 * (size_t)pos, a.l_desc + 32 * (size_t)i);
  }
  if (a.res_int) {
    const double ic = a.l_icur[i];
    reinterpret_cast<double *>(a.out + xk_frame_out_int(B, a.l_desc != nullptr, 0))[pos] = a.l_iprev[i];
    reinterpret_cast<double *>(a.out + xk_frame_out_int(B, a.l_desc != nullptr, 1))[pos] = ic;
    a.res_int[pos] = ic;
  }
}

__global__ __launch_bounds__(256) void xk_frame_first(XkFrameArgs a) {
  const int n = a.c[XK_FC_NEW];
  const int pos = blockIdx.x * 256 + threadIdx.x;
  if (pos == 0) {
    int *head = reinterpret_cast<int *>(a.out);
    for (int j = 0; j < XK_FC_N; ++j) head[j] = a.c[j];
    if (a.res_int) xk_frame_cal_head(a, head);
  }
  if (pos >= n) return;
  const int *det_xy = a.det_res + 4, *det_score = a.det_res + 4 + 2 * (size_t)a.max_matches;
  const int x = det_xy[2 * pos], y = det_xy[2 * pos + 1];
  a.res_dist[2 * pos] = (double)x; a.res_dist[2 * pos + 1] = (double)y;
  a.res_pts[2 * pos] = (float)x; a.res_pts[2 * pos + 1] = (float)y;
  a.res_score[pos] = det_score[pos];
  if (a.res_desc)
    xk_frame_copy_desc(a.res_desc + 32 * (size_t)pos,
                       reinterpret_cast<const unsigned char *>(a.orb_res) + xk_orb_desc_off((size_t)a.cap_new) + 32 * (size_t)pos);
  if (a.res_int) a.res_int[pos] = a.val_new[pos];                 // tracker.cpp:461
}

// static_cast<int> of the kept current points of a tracking (tracker.cpp:666; they lie within [-0.5, W - 0.5] x [-0.5, H - 0.5])
struct XkFrameTruncArgs {
  const double *xy;              // [n][2]
  const int *n_dev;              // where the device holds the count (xk_dev_count)
  int n;                         // its bound
  int *ixy;                      // [n][2]
};

__global__ __launch_bounds__(256) void xk_frame_trunc(XkFrameTruncArgs a) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= xk_dev_count(a.n_dev, a.n)) return;
  const double x = a.xy[2 * j], y = a.xy[2 * j + 1];
  a.ixy[2 * j] = (int)x; a.ixy[2 * j + 1] = (int)y;
}
