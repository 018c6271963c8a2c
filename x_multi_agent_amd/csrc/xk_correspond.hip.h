// xk_correspond.hip.h -- the list work of PlaceRecognition::findCorrespondences (place_recognition.cpp:252-383, the non-GT
// branch) on the device (gfx950), so that xk_pr_find_correspondences is one call: the 2-NN result never leaves the device
// between the matcher and the essential-matrix filter, and the filter's mask never leaves it before the duplicate removal.
//
//   xk_corr_candidates  one workgroup of 256: distance + ratio test (:254-255) over what xk_desc_knn2 left, the ordered
//                       candidate list (query, train), their pixels gathered into the essential filter's two point lists,
//                       the count into device memory (the essential kernels read it through xk_dev_count)
//   xk_corr_finish      one workgroup of 256: the mask applied (:275-281), the duplicate search (:283-296), the erase loop
//                       with its running offset (:297-302) as a rank-select on an alive bit mask, the classification
//                       (:311-383), and the head of the result block
//
// Everything here is integer work: the results are bit-defined.  The erase loop is NOT a de-duplication: erase k removes the
// element at position remove_ids[k] - k of the list as it is THEN, which after earlier erases is no longer the element the
// search found.  The alive mask keeps exactly that meaning: position p of the current list is the p-th set bit.
#pragma once
#include <hip/hip_runtime.h>

#include "xk_ransac.hip.h"

struct XkCorrCandArgs {
  const int *idx, *dist;            // [n_rec][2], xk_desc_knn2's result
  int n_rec;
  double min_distance, ratio_thr;
  const float *rec_xy_in, *cur_xy_in;   // [n_rec][2], [n_cur][2]: the caller's pixels
  float *cur_xy, *rec_xy;           // the essential block's lists, candidate order
  int *cand;                        // [n_rec][2] query, train
  int *count;
};

__global__ __launch_bounds__(256) void xk_corr_candidates(XkCorrCandArgs a) {
  int t = -1;
  const int n = xk_ransac_compact(
      a.n_rec,
      [&](int q) {
        if (a.idx[2 * q + 1] < 0) return false;                // fewer than two neighbours: m[1] does not exist
        const double d0 = (double)a.dist[2 * q], d1 = (double)a.dist[2 * q + 1];
        t = a.idx[2 * q];
        return d0 < a.min_distance && d0 < d1 * a.ratio_thr;
      },
      [&](int q, int pos) {
        a.cand[2 * pos] = q; a.cand[2 * pos + 1] = t;
        a.cur_xy[2 * pos] = a.cur_xy_in[2 * t]; a.cur_xy[2 * pos + 1] = a.cur_xy_in[2 * t + 1];
        a.rec_xy[2 * pos] = a.rec_xy_in[2 * q]; a.rec_xy[2 * pos + 1] = a.rec_xy_in[2 * q + 1];
      });
  if (threadIdx.x == 0) *a.count = n;
}

// The head of the result block, then E [9] doubles, then the lists laid out by the bound n_rec.
struct XkCorrHead { int status, n_candidates, n_inliers, winner, n_good, n_classified, n_remove, pad; };

struct XkCorrFinishArgs {
  int n_rec;                        // the bound
  const int *count;                 // candidates
  const int *cand;                  // [n_rec][2]
  const unsigned char *ess_mask;    // [count], xk_ess_mask's
  const double *ess_E;              // [9]
  const int *ess_res;               // n_inliers, winner
  int n_cur_msckf, n_cur_slam, n_rec_msckf, n_rec_slam;
  // scratch, sized by max_desc
  int *G, *first_j;                 // [n_rec][2], [n_rec]
  unsigned long long *alive;        // [(n_rec + 63) / 64]
  // result block
  XkCorrHead *head;
  double *E;
  int *good, *classified, *remove_ids;   // [n_rec][2], [n_rec][3], [n_rec]
  unsigned char *mask;              // [n_rec]
};

// The index of the r-th set bit of w (r < popcount(w)).
__device__ __forceinline__ int xk_corr_select64(unsigned long long w, int r) {
  int pos = 0;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const int c = __popcll((w >> pos) & ((1ull << s) - 1ull));
    if (r >= c) { r -= c; pos += s; }
  }
  return pos;
}

__device__ __forceinline__ int xk_corr_kind(int q, int t, int cm, int cs, int rm, int rs) {
  if (q < rm) return t >= cs ? 0 : -1;                       // MSCKF_OPP
  if (q < rs) return t >= cs ? 2 : (t >= cm ? 1 : -1);       // SLAM_OPP, SLAM_SLAM
  return t >= cs ? 3 : -1;                                   // OPP_OPP
}

// Between the steps one thread's global stores (G, first_j, remove_ids, alive, good) are another thread's loads, ordered by
// __syncthreads alone: enough for ONE workgroup, whose wavefronts share a compute unit and its L1; not for a grid.
__global__ __launch_bounds__(256) void xk_corr_finish(XkCorrFinishArgs a) {
  __shared__ int2 s_qt[256];
  const int tid = threadIdx.x, lane = tid & 63;
  const int nc = xk_dev_count(a.count, a.n_rec);
  // 1. the mask applied, order kept; the mask itself into the result block, zero up to the bound
  for (int i = tid; i < a.n_rec; i += 256) a.mask[i] = i < nc ? a.ess_mask[i] : 0;
  const int ng = xk_ransac_compact(
      nc, [&](int i) { return a.ess_mask[i] != 0; },
      [&](int i, int pos) { a.G[2 * pos] = a.cand[2 * i]; a.G[2 * pos + 1] = a.cand[2 * i + 1]; });
  __syncthreads();
  // 2. for every i the first j > i with an equal query or train index: tiles of 256 j through LDS, every thread one i
  for (int i0 = 0; i0 < ng; i0 += 256) {
    const int i = i0 + tid;
    const int qi = i < ng ? a.G[2 * i] : -1, ti = i < ng ? a.G[2 * i + 1] : -1;
    int fj = -1;
    for (int j0 = i0; j0 < ng; j0 += 256) {
      __syncthreads();
      s_qt[tid] = j0 + tid < ng ? make_int2(a.G[2 * (j0 + tid)], a.G[2 * (j0 + tid) + 1]) : make_int2(-2, -2);
      __syncthreads();
      // a wavefront walks the tile from its own first i on, every lane the same entry (a broadcast read); no early exit, so
      // that the reads do not wait for the compares: the first match is the smallest
      const int m = min(256, ng - j0);
      int first = 256;
#pragma unroll 8
      for (int jj = max(i0 + (tid & ~63) + 1 - j0, 0); jj < m; ++jj) {
        const int2 e = s_qt[jj];
        const bool hit = ((e.x == qi) | (e.y == ti)) & (j0 + jj > i);   // (no short circuit: no branch per entry)
        first = hit ? min(first, jj) : first;
      }
      if (fj < 0 && first < 256) fj = j0 + first;
    }
    if (i < ng) a.first_j[i] = fj;
  }
  __syncthreads();
  // 3. remove_ids: those j in ascending i
  const int nr = xk_ransac_compact(
      ng, [&](int i) { return a.first_j[i] >= 0; }, [&](int i, int pos) { a.remove_ids[pos] = a.first_j[i]; });
  // 4. the erase loop.  alive bit p of word w: element 64 w + p of G is still in the list.
  const int nw = (ng + 63) / 64;
  for (int w = tid; w < nw; w += 256) a.alive[w] = ng - 64 * w >= 64 ? ~0ull : (1ull << (ng - 64 * w)) - 1ull;
  __syncthreads();
  if (tid < 64) {                                            // one wavefront; lane l owns words l, l + 64, ...
    int len = ng;
    for (int k0 = 0; k0 < nr; k0 += 64) {
      const int mine = k0 + lane < nr ? a.remove_ids[k0 + lane] : 0;
      const int kn = min(64, nr - k0);
      for (int kk = 0; kk < kn; ++kk) {
        int rem = __shfl(mine, kk, 64) - (k0 + kk);          // position in the list as it is now
        if (rem < 0 || rem >= len) continue;                 // (cannot occur: remove_ids[k] comes from an i >= k)
        for (int w0 = 0; w0 < nw; w0 += 64) {
          const int wi = w0 + lane;
          const unsigned long long word = wi < nw ? a.alive[wi] : 0ull;
          const int pc = __popcll(word);
          int incl = pc;
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
          }
          const int total = __shfl(incl, 63, 64);
          if (rem < total) {
            if (rem >= incl - pc && rem < incl) a.alive[wi] = word & ~(1ull << xk_corr_select64(word, rem - (incl - pc)));
            break;
          }
          rem -= total;
        }
        --len;
      }
    }
  }
  __syncthreads();
  // 5. what is left, order kept
  const int n_good = xk_ransac_compact(
      ng, [&](int i) { return ((a.alive[i >> 6] >> (i & 63)) & 1ull) != 0ull; },
      [&](int i, int pos) { a.good[2 * pos] = a.G[2 * i]; a.good[2 * pos + 1] = a.G[2 * i + 1]; });
  __syncthreads();
  // 6. classification: a good match falls in at most one class
  const int cm = a.n_cur_msckf, cs = cm + a.n_cur_slam, rm = a.n_rec_msckf, rs = rm + a.n_rec_slam;
  int kind = -1, q = 0, t = 0;
  const int n_cls = xk_ransac_compact(
      n_good,
      [&](int i) {
        q = a.good[2 * i]; t = a.good[2 * i + 1];
        kind = xk_corr_kind(q, t, cm, cs, rm, rs);
        return kind >= 0;
      },
      [&](int i, int pos) {
        a.classified[3 * pos] = kind;
        a.classified[3 * pos + 1] = t - (kind == 1 ? cm : cs);
        a.classified[3 * pos + 2] = q - (kind == 0 ? 0 : (kind == 3 ? rs : rm));
      });
  // 7. the head
  if (tid < 9) a.E[tid] = a.ess_E[tid];
  if (tid == 0) {
    const int winner = a.ess_res[1];
    const int status = nc == 0 ? 3 : (winner < 0 ? 4 : (n_good == 0 ? 5 : 0));
    XkCorrHead h;
    h.status = status; h.n_candidates = nc; h.n_inliers = a.ess_res[0]; h.winner = winner;
    h.n_good = status == 0 ? n_good : 0; h.n_classified = status == 0 ? n_cls : 0; h.n_remove = nr; h.pad = 0;
    *a.head = h;
  }
}
