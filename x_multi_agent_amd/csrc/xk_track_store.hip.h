// xk_track_store.hip.h -- TrackManager::manageTracks (track_manager.cpp:115-436) on tracks that stay on the device (gfx950, wave64).
//
// The store: max_tracks slots, each a ring of the newest XK_TS_RING observations (undistorted and distorted pixels in fp64, FAST score,
// tile), the track's true length and its id.  The persistent, new persistent and opportunistic lists are index arrays over the slots:
// tracks never move, indices do.  Free slots are a stack.  The id counter lives beside them and survives xk_ts_clear.
//
// One manage call is four launches on one stream.  No kernel waits on another: every count and flag is a plain load of what an earlier
// launch wrote.  Integer atomics on LDS only, no inline assembly, every loop bounded before it starts.
//   xk_ts_associate   one workgroup of 1024.  Tiles of every match (the loops of TiledImage::setTileForFeature, xk_tile_for_feature) and the
//                     refusals, decided before anything changes.  Then the two claims, each as a parallel "first equal" (one wavefront per
//                     item, ballots over the other list) and a check that no two items chose the same partner: if none did, the choices
//                     ARE the sequential scan's (by induction over the list, every earlier item took its own first choice, which is not
//                     this one's).  Otherwise the list is walked in order by the whole workgroup, one item per step, each step the first
//                     unclaimed equal partner by an LDS minimum: the scan itself.  Commit: observations appended to the rings, new
//                     tracks in free slots with ids in match order.
//   xk_ts_candidates  one workgroup of 1024.  The candidates of the baseline batch (dead tracks, then live ones long enough) as CSR offsets
//                     by wavefront scans, their newest <= 64 observations gathered, and the stable sort of the opportunistic list by
//                     true length, descending, as a rank count.
//   xk_ts_baseline    xk_tracks_baseline_body on that batch, the count read from the device: the normalised coordinates go straight
//                     into the result block.
//   xk_ts_walk        one wavefront.  The dead-track pass, the promotion walk (serial by nature: each step reads the tile counts the
//                     previous one changed; the tile counts in LDS, the search for the fullest tile's youngest track and the rescan for
//                     the fullest tile spread over the lanes), the MSCKF-SLAM / standard split, the ordered compactions of all lists,
//                     the freed slots, and the result block.
// bin_track_idx of the reference is, per tile, the positions of its tracks in the joined persistent list in increasing order (persistent
// tracks arrive in list order, promoted ones behind them, and an erase shifts every later position alike), so its back() is the highest
// alive position of that tile and bin_track_idx_per's back() the same track's index before the frame's deletions: the walk keeps one
// tile and one original index per position and marks erased positions; the `idx > gone` shift becomes the final compaction.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "xk_frame.hip.h"
#include "xk_tracks.hip.h"

#define XK_TS_RING 64            // x::TrackManager::kMaxObs
#define XK_TS_THREADS 1024
#define XK_TS_MAX_TILES 4096

// the status of a manage call
#define XK_TS_EOUTSIDE 1         // a match's current feature lies outside the tile grid
#define XK_TS_ECAPACITY 2        // more candidate or live tracks than max_tracks
#define XK_TS_EBOOKKEEPING 3     // "tile bookkeeping out of step": the fullest tile holds no track

// the store's counts
enum { XK_TSH_N_SLAM = 0, XK_TSH_N_NEW, XK_TSH_N_OPP, XK_TSH_FREE_TOP, XK_TSH_N = 4 };

// the call's counts, on the device between its launches
enum {
  XK_TSC_STATUS = 0, XK_TSC_S0, XK_TSC_N0, XK_TSC_O, XK_TSC_KEPT, XK_TSC_LOST, XK_TSC_REM, XK_TSC_DEAD, XK_TSC_STARTED, XK_TSC_CAND,
  XK_TSC_CAND_OBS, XK_TSC_NORM, XK_TSC_N = 16
};

// the head of the result block
enum {
  XK_TSR_STATUS = 0, XK_TSR_N_SLAM, XK_TSR_N_NEW, XK_TSR_N_OPP, XK_TSR_N_LOST, XK_TSR_N_MATCHES, XK_TSR_N_CLAIMED, XK_TSR_N_CAND,
  XK_TSR_N_CAND_OBS, XK_TSR_N_NORM, XK_TSR_NEXT_ID_LO, XK_TSR_NEXT_ID_HI,
  XK_TSR_LIST0,                  // the five measurement lists' lengths: MSCKF, short MSCKF, new standard SLAM, new MSCKF-SLAM, persistent
  XK_TSR_N_PER_OBS = XK_TSR_LIST0 + 5,
  XK_TSR_N = 24
};

struct XkTsArgs {
  // ---- the store ----
  double *obs;                   // [max_tracks][64][4]: undistorted x, y, distorted x, y; observation i of a track at ring position i & 63
  int *score;                    // [max_tracks][64]
  int *tile;                     // [max_tracks][64][2]: row, column
  int *len;                      // [max_tracks] true length
  long long *id;                 // [max_tracks]
  int *slam, *newl, *opp;        // [max_tracks] each: slots in list order
  int *free_;                    // [max_tracks] stack of free slots
  int *hdr;                      // [XK_TSH_N]
  long long *next_id;
  int max_tracks, multi_uav;
  int tiles_h, tiles_w;
  double tile_w, tile_h, height;
  double fx, fy, cx, cy, min_x, min_y;
  // ---- the call ----
  int n;                         // matches
  int n_quats, n_poses_max, n_slam_max, min_track_length, n_opp_ids;
  const double *m_prev, *m_cur, *m_dprev, *m_dcur;   // [n][2] each
  const int *m_score;            // [n]
  const double *quat;            // [n_quats][4]
  const long long *opp_ids;      // [n_opp_ids]
  // ---- scratch ----
  int *c;                        // [XK_TSC_N]
  int *m_tile;                   // [n][4] previous row, column, current row, column
  int *m_bin, *m_owner, *rm, *mo, *newk;   // [n] each
  double *last_xy;               // [max_tracks][2]: the joined persistent list's last features, then the opportunistic list's
  int *pm, *kp, *lost_slot;      // [max_tracks]
  int *o_owner, *o_claimed;      // [max_tracks]
  int *comb, *cbin, *corig, *calive;   // [max_tracks] the joined persistent list of the walk
  int *opp_tmp, *dead, *sorted, *lens, *act;   // [max_tracks]
  int *cand_of;                  // [max_tracks] by slot
  int *cand_slot, *trk_off, *norm_off;   // [max_tracks (+ 1)]
  unsigned char *drop, *flag;    // [max_tracks]
  double *delta;                 // [max_tracks][2]
  double *b_obs;                 // [max_tracks][64][2]
  int *l_msckf, *l_short;        // [max_tracks] candidates
  // ---- the result block ----
  int *head;                     // [XK_TSR_N]
  int *lost;                     // [lost bound]
  int *claimed;                  // [n]
  long long *e_id;               // [entry bound] the five lists behind one another
  int *e_start, *e_len;          // into norm_xy, in observations
  double *norm_xy;               // the batch's normalised coordinates, then the persistent list's
};

// Feature::nearlyEqual (feature.cpp:51-68)
__device__ __forceinline__ bool xk_ts_nearly_equal(double a, double b) {
#pragma clang fp contract(off)
  if (a == b) return true;
  const double tiny = 2.2250738585072014e-308, eps = 2.220446049250313e-16, huge = 1.7976931348623157e308;
  const double abs_a = fabs(a), abs_b = fabs(b), diff = fabs(a - b), sum = abs_a + abs_b;
  if (a == 0.0 || b == 0.0 || sum < tiny) return diff < eps * tiny;
  return diff / (huge < sum ? huge : sum) < eps;                  // std::min(sum, max)
}
__device__ __forceinline__ bool xk_ts_same(double ax, double ay, double bx, double by) { return xk_ts_nearly_equal(ax, bx) && xk_ts_nearly_equal(ay, by); }

// the first i in [first, N) with pred(i), by one wavefront; -1: none
template <class P>
__device__ __forceinline__ int xk_ts_wave_first(int N, int lane, P pred) {
  for (int base = 0; base < N; base += 64) {
    const int i = base + lane;
    const unsigned long long m = __ballot(i < N && pred(i));
    if (m) return base + __ffsll((long long)m) - 1;
  }
  return -1;
}

// ordered compaction by one wavefront: put(i, position) for every i in [0, N) with pred(i); returns their number
template <class P, class W>
__device__ __forceinline__ int xk_ts_wave_compact(int N, int lane, P pred, W put) {
  int run = 0;
  for (int base = 0; base < N; base += 64) {
    const int i = base + lane;
    const bool keep = i < N && pred(i);
    const unsigned long long m = __ballot(keep);
    if (keep) put(i, run + __popcll(m & ((1ull << lane) - 1ull)));
    run += __popcll(m);
  }
  return run;
}

// exclusive prefix sum over a wavefront and its total
__device__ __forceinline__ int xk_ts_wave_excl(int v, int lane, int *total) {
  int s = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(s, d, 64);
    if (lane >= d) s += t;
  }
  *total = __shfl(s, 63, 64);
  return s - v;
}

// one observation behind a track's last one
__device__ __forceinline__ void xk_ts_append(const XkTsArgs &a, int slot, double x, double y, double xd, double yd, int score, int row, int col) {
  const int L = a.len[slot];
  const size_t at = (size_t)slot * XK_TS_RING + (size_t)(L & (XK_TS_RING - 1));
  a.obs[4 * at] = x; a.obs[4 * at + 1] = y; a.obs[4 * at + 2] = xd; a.obs[4 * at + 3] = yd;
  a.score[at] = score;
  a.tile[2 * at] = row; a.tile[2 * at + 1] = col;
  a.len[slot] = L + 1;
}

// the head of a refused call: the status and the store as it stands
__device__ __forceinline__ void xk_ts_refuse(const XkTsArgs &a, int status) {
  for (int j = 0; j < XK_TSR_N; ++j) a.head[j] = 0;
  a.head[XK_TSR_STATUS] = status;
  a.head[XK_TSR_N_SLAM] = a.hdr[XK_TSH_N_SLAM]; a.head[XK_TSR_N_NEW] = a.hdr[XK_TSH_N_NEW]; a.head[XK_TSR_N_OPP] = a.hdr[XK_TSH_N_OPP];
  a.head[XK_TSR_N_MATCHES] = a.n;
  const long long id = *a.next_id;
  a.head[XK_TSR_NEXT_ID_LO] = (int)(unsigned int)(id & 0xffffffffll); a.head[XK_TSR_NEXT_ID_HI] = (int)(id >> 32);
  a.c[XK_TSC_STATUS] = status;
}

// The claims of `n_items` items, in order, on `n_part` partners: item i takes the first partner q in order that no earlier item has
// claimed and for which equal(i, q) holds.  choice[i]: the partner or -1; claimed[q]: 0 or 1 (zero on entry); owner[q]: scratch, -1 on
// entry.  Every thread of the workgroup calls it.
template <class E>
__device__ __forceinline__ void xk_ts_claim(int n_items, int n_part, int *choice, int *owner, int *claimed, int *s_min, E equal) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = wave; i < n_items; i += XK_TS_THREADS / 64) {
    const int q = xk_ts_wave_first(n_part, lane, [&](int p) { return equal(i, p); });
    if (lane == 0) {
      choice[i] = q;
      if (q >= 0) owner[q] = i;                                    // (contested partners: one of the stores stays)
    }
  }
  __syncthreads();
  int contested = 0;
  for (int i = tid; i < n_items; i += XK_TS_THREADS)
    if (choice[i] >= 0 && owner[choice[i]] != i) contested = 1;
  if (!__syncthreads_or(contested)) {
    for (int i = tid; i < n_items; i += XK_TS_THREADS)
      if (choice[i] >= 0) claimed[choice[i]] = 1;
    __syncthreads();
    return;
  }
  for (int i = 0; i < n_items; ++i) {                               // the scan itself, one item per step
    if (tid == 0) *s_min = 0x7fffffff;
    __syncthreads();
    const int hint = choice[i];                                     // its first equal partner, claimed or not: nothing before it is equal
    if (hint >= 0)
      for (int q = hint + tid; q < n_part; q += XK_TS_THREADS)
        if (!claimed[q] && equal(i, q)) {
          atomicMin(s_min, q);
          break;
        }
    __syncthreads();
    if (tid == 0) {
      const int q = *s_min == 0x7fffffff ? -1 : *s_min;
      choice[i] = q;
      if (q >= 0) claimed[q] = 1;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(XK_TS_THREADS) void xk_ts_associate(XkTsArgs a) {
  __shared__ int s_min, s_cnt[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = a.n, S0 = a.hdr[XK_TSH_N_SLAM], N0 = a.hdr[XK_TSH_N_NEW], O = a.hdr[XK_TSH_N_OPP], P = S0 + N0;
  const int free_top = a.hdr[XK_TSH_FREE_TOP];
  const long long next_id = *a.next_id;
  // ---- validate: the tiles of every match, the refusals ----
  int outside = 0;
  for (int i = tid; i < n; i += XK_TS_THREADS) {
    int t[4];
    xk_tile_for_feature(a.tile_w, a.tile_h, a.height, a.tiles_h, a.tiles_w, a.m_dprev[2 * i], a.m_dprev[2 * i + 1], &t[0], &t[1]);
    xk_tile_for_feature(a.tile_w, a.tile_h, a.height, a.tiles_h, a.tiles_w, a.m_dcur[2 * i], a.m_dcur[2 * i + 1], &t[2], &t[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) a.m_tile[4 * i + j] = t[j];
    const bool inside = t[2] >= 0 && t[2] < a.tiles_h && t[3] >= 0 && t[3] < a.tiles_w;
    a.m_bin[i] = inside ? t[2] * a.tiles_w + t[3] : -1;
    if (!inside) outside = 1;
    a.m_owner[i] = -1;
    a.claimed[i] = 0;
  }
  for (int o = tid; o < O; o += XK_TS_THREADS) { a.o_owner[o] = -1; a.o_claimed[o] = 0; }
  int status = __syncthreads_or(outside) ? XK_TS_EOUTSIDE : 0;
  if (status == 0 && (long long)O + (a.min_track_length <= 2 ? n : 0) > (long long)a.max_tracks) status = XK_TS_ECAPACITY;
  if (status != 0) {
    if (tid == 0) xk_ts_refuse(a, status);
    return;
  }
  // ---- the last features of the joined persistent list (the new persistent tracks behind the persistent ones) and of the opportunistic one ----
  for (int p = tid; p < P + O; p += XK_TS_THREADS) {
    const int slot = p < S0 ? a.slam[p] : p < P ? a.newl[p - S0] : a.opp[p - P];
    const size_t at = (size_t)slot * XK_TS_RING + (size_t)((a.len[slot] - 1) & (XK_TS_RING - 1));
    a.last_xy[2 * p] = a.obs[4 * at]; a.last_xy[2 * p + 1] = a.obs[4 * at + 1];
  }
  __syncthreads();
  // ---- 1. persistent tracks claim matches ----
  xk_ts_claim(P, n, a.pm, a.m_owner, a.claimed, &s_min,
              [&](int p, int m) { return xk_ts_same(a.last_xy[2 * p], a.last_xy[2 * p + 1], a.m_prev[2 * m], a.m_prev[2 * m + 1]); });
  if (wave == 0) {
    const int n_rem = xk_ts_wave_compact(n, lane, [&](int m) { return a.claimed[m] == 0; }, [&](int m, int pos) { a.rm[pos] = m; });
    const int n_kept = xk_ts_wave_compact(P, lane, [&](int p) { return a.pm[p] >= 0; }, [&](int p, int pos) { a.kp[pos] = p; });
    const int n_lost = xk_ts_wave_compact(P, lane, [&](int p) { return a.pm[p] < 0; }, [&](int p, int pos) {
      a.lost[pos] = p;                                              // t + lost_per_count: its index before this frame's deletions
      a.lost_slot[pos] = p < S0 ? a.slam[p] : a.newl[p - S0];
    });
    if (lane == 0) { s_cnt[0] = n_rem; s_cnt[1] = n_kept; s_cnt[2] = n_lost; }
  }
  __syncthreads();
  const int n_rem = s_cnt[0], n_kept = s_cnt[1], n_lost = s_cnt[2];
  // ---- 2. the remaining matches claim opportunistic tracks ----
  xk_ts_claim(n_rem, O, a.mo, a.o_owner, a.o_claimed, &s_min, [&](int j, int o) {
    const int m = a.rm[j];
    return xk_ts_same(a.last_xy[2 * (P + o)], a.last_xy[2 * (P + o) + 1], a.m_prev[2 * m], a.m_prev[2 * m + 1]);
  });
  if (wave == 0) {
    const int n_started = xk_ts_wave_compact(n_rem, lane, [&](int j) { return a.mo[j] < 0; }, [&](int j, int pos) { a.newk[j] = pos; });
    const int n_dead = xk_ts_wave_compact(O, lane, [&](int o) { return a.o_claimed[o] == 0; }, [&](int o, int pos) { a.dead[pos] = a.opp[o]; });
    if (lane == 0) { s_cnt[3] = n_started; s_cnt[4] = n_dead; }
  }
  __syncthreads();
  const int n_started = s_cnt[3], n_dead = s_cnt[4];
  if (n_started > free_top) {                                       // (the frame's dead tracks hold their slots until the call ends)
    if (tid == 0) xk_ts_refuse(a, XK_TS_ECAPACITY);
    return;
  }
  // ---- commit ----
  for (int t = tid; t < n_kept; t += XK_TS_THREADS) {
    const int p = a.kp[t], m = a.pm[p];
    const int slot = p < S0 ? a.slam[p] : a.newl[p - S0];
    xk_ts_append(a, slot, a.m_cur[2 * m], a.m_cur[2 * m + 1], a.m_dcur[2 * m], a.m_dcur[2 * m + 1], a.m_score[m], a.m_tile[4 * m + 2], a.m_tile[4 * m + 3]);
    a.comb[t] = slot; a.cbin[t] = a.m_bin[m]; a.corig[t] = p; a.calive[t] = 1;
  }
  for (int j = tid; j < n_rem; j += XK_TS_THREADS) {
    const int m = a.rm[j], o = a.mo[j];
    int slot;
    if (o >= 0) {
      slot = a.opp[o];
    } else {                                                        // ids in match order
      const int k = a.newk[j];
      slot = a.free_[free_top - 1 - k];
      a.id[slot] = next_id + k;
      a.len[slot] = 0;
      xk_ts_append(a, slot, a.m_prev[2 * m], a.m_prev[2 * m + 1], a.m_dprev[2 * m], a.m_dprev[2 * m + 1], a.m_score[m], a.m_tile[4 * m], a.m_tile[4 * m + 1]);
    }
    xk_ts_append(a, slot, a.m_cur[2 * m], a.m_cur[2 * m + 1], a.m_dcur[2 * m], a.m_dcur[2 * m + 1], a.m_score[m], a.m_tile[4 * m + 2], a.m_tile[4 * m + 3]);
    a.opp_tmp[j] = slot;
  }
  if (tid == 0) {
    int *c = a.c;
    c[XK_TSC_STATUS] = 0; c[XK_TSC_S0] = S0; c[XK_TSC_N0] = N0; c[XK_TSC_O] = O; c[XK_TSC_KEPT] = n_kept; c[XK_TSC_LOST] = n_lost;
    c[XK_TSC_REM] = n_rem; c[XK_TSC_DEAD] = n_dead; c[XK_TSC_STARTED] = n_started;
    *a.next_id = next_id + n_started;                               // (every thread read it before the barriers above)
  }
}

__global__ __launch_bounds__(XK_TS_THREADS) void xk_ts_candidates(XkTsArgs a) {
  if (a.c[XK_TSC_STATUS] != 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_dead = a.c[XK_TSC_DEAD], n_opp = a.c[XK_TSC_REM], n_all = n_dead + n_opp;
  __shared__ int s_K;
  if (wave == 0) {
    // dead tracks first (their attitude list without its last entry, single-agent), then the live ones long enough (track_manager.cpp:277-292)
    int K = 0, run_obs = 0, run_norm = 0;
    for (int base = 0; base < n_all; base += 64) {
      const int i = base + lane;
      int is = 0, drop = 0, slot = 0, L = 0;
      if (i < n_all) {
        slot = i < n_dead ? a.dead[i] : a.opp_tmp[i - n_dead];
        L = a.len[slot];
        if (i >= n_dead) {
          is = (L > a.min_track_length - 1 && L >= 2) ? 1 : 0;
        } else if (a.multi_uav) {
          if (L >= 3) {
            const long long id = a.id[slot];
            for (int o = 0; o < a.n_opp_ids; ++o)
              if (a.opp_ids[o] == id) is = 1;
          }
        } else {
          is = L >= 2 ? 1 : 0;
          drop = 1;
        }
      }
      const int nq = a.n_quats - drop;
      const int n_obs = is ? (L < XK_TS_RING ? L : XK_TS_RING) : 0, n_norm = is ? (n_obs < nq ? n_obs : nq) : 0;
      int tk, to, tn;
      const int k = K + xk_ts_wave_excl(is, lane, &tk), oo = run_obs + xk_ts_wave_excl(n_obs, lane, &to), on = run_norm + xk_ts_wave_excl(n_norm, lane, &tn);
      if (i < n_all) a.cand_of[slot] = is ? k : -1;
      if (is) { a.cand_slot[k] = slot; a.drop[k] = (unsigned char)drop; a.trk_off[k] = oo; a.norm_off[k] = on; }
      K += tk; run_obs += to; run_norm += tn;
    }
    if (lane == 0) {
      a.trk_off[K] = run_obs; a.norm_off[K] = run_norm;
      a.c[XK_TSC_CAND] = K; a.c[XK_TSC_CAND_OBS] = run_obs; a.c[XK_TSC_NORM] = run_norm;
      s_K = K;
    }
  }
  for (int j = tid; j < n_opp; j += XK_TS_THREADS) a.lens[j] = a.len[a.opp_tmp[j]];
  __syncthreads();
  const int K = s_K;
  // each candidate's newest <= 64 observations, oldest first
  for (int k = wave; k < K; k += XK_TS_THREADS / 64) {
    const int slot = a.cand_slot[k], L = a.len[slot], cnt = L < XK_TS_RING ? L : XK_TS_RING;
    if (lane < cnt) {
      const size_t at = (size_t)slot * XK_TS_RING + (size_t)((L - cnt + lane) & (XK_TS_RING - 1));
      double *o = a.b_obs + 2 * ((size_t)a.trk_off[k] + lane);
      o[0] = a.obs[4 * at]; o[1] = a.obs[4 * at + 1];
    }
  }
  // std::stable_sort by length, descending: the position of a track is the number of longer ones plus the equally long ones before it
  for (int j = tid; j < n_opp; j += XK_TS_THREADS) {
    const int L = a.lens[j];
    int rank = 0;
    for (int i = 0; i < n_opp; ++i) {
      const int Li = a.lens[i];
      rank += (Li > L || (Li == L && i < j)) ? 1 : 0;
    }
    a.sorted[rank] = a.opp_tmp[j];
  }
}

__global__ __launch_bounds__(64 * XK_TRACKS_WAVES) void xk_ts_baseline(XkTsArgs s) {
  if (s.c[XK_TSC_STATUS] != 0) return;
  XkTracksArgs a{};
  a.quat = s.quat; a.trk_off = s.trk_off; a.norm_off = s.norm_off; a.drop_last = s.drop; a.obs_xy = s.b_obs;
  a.K = 0; a.n_quats = s.n_quats;
  a.fx = s.fx; a.fy = s.fy; a.cx = s.cx; a.cy = s.cy; a.min_x = s.min_x; a.min_y = s.min_y;
  a.norm_xy = s.norm_xy; a.delta_xy = s.delta; a.flag = s.flag;
  xk_tracks_baseline_body(a, s.c[XK_TSC_CAND]);
}

__global__ __launch_bounds__(64) void xk_ts_walk(XkTsArgs a) {
  if (a.c[XK_TSC_STATUS] != 0) return;
  __shared__ int cnt[XK_TS_MAX_TILES];
  __shared__ int s_bmax;
  const int lane = threadIdx.x;
  const int n_bins = a.tiles_h * a.tiles_w;
  const int n_kept = a.c[XK_TSC_KEPT], n_opp = a.c[XK_TSC_REM], n_dead = a.c[XK_TSC_DEAD], n_cand = a.c[XK_TSC_CAND], n_norm = a.c[XK_TSC_NORM];
  int n_lost = a.c[XK_TSC_LOST];
  const int n_lost1 = n_lost;
  for (int b = lane; b < n_bins; b += 64) cnt[b] = 0;
  __syncthreads();
  if (lane == 0) {                                                  // bin_track_idx's sizes and idx_bin_max_per as the persistent tracks arrived
    int bmax = 0;
    for (int t = 0; t < n_kept; ++t) {
      const int b = a.cbin[t];
      cnt[b] += 1;
      if (cnt[b] > cnt[bmax]) bmax = b;
    }
    s_bmax = bmax;
  }
  __syncthreads();
  int bmax = s_bmax;
  // ---- 4. the dead tracks: every candidate with multi_uav (its id was in the list), the ones whose baseline passes otherwise ----
  const int n_short = xk_ts_wave_compact(
      n_dead, lane,
      [&](int i) {
        const int k = a.cand_of[a.dead[i]];
        return k >= 0 && (a.multi_uav || a.flag[k] != 0);
      },
      [&](int i, int pos) { a.l_short[pos] = a.cand_of[a.dead[i]]; });
  // ---- 5. the promotion walk, longest track first: one track per step, every lane with the same scalars ----
  int C = n_kept, total = n_kept, n_msckf = 0, status = 0;
  for (int j = 0; j < n_opp && status == 0; ++j) {
    const int slot = a.sorted[j], L = a.len[slot];
    const size_t at = (size_t)slot * XK_TS_RING + (size_t)((L - 1) & (XK_TS_RING - 1));
    const int b = a.tile[2 * at] * a.tiles_w + a.tile[2 * at + 1];  // (inside the grid: validated)
    int act = 0;                                                    // 0: it waits, 1: promoted, 2: consumed or dropped
    if (L > a.min_track_length - 1) {
      const int cb = cnt[b], cm = cnt[bmax];
      if (total < a.n_slam_max) {
        __syncthreads();
        if (lane == 0) { a.comb[C] = slot; a.cbin[C] = b; a.corig[C] = -1; a.calive[C] = 1; cnt[b] = cb + 1; }
        if (cb + 1 > cm) bmax = b;
        C += 1; total += 1; act = 1;
        __syncthreads();
      } else if (cm > cb + 1) {
        // the youngest track of the fullest tile: its highest alive position
        int gone = -1;
        for (int top = ((C + 63) / 64) * 64; top > 0 && gone < 0; top -= 64) {
          const int p = top - 64 + lane;
          const unsigned long long m = __ballot(p < C && a.calive[p] != 0 && a.cbin[p] == bmax);
          if (m) gone = top - 64 + (63 - __clzll((long long)m));
        }
        if (gone < 0) { status = XK_TS_EBOOKKEEPING; break; }
        const int orig = a.corig[gone];
        __syncthreads();
        if (lane == 0) {
          if (orig >= 0) a.lost[n_lost] = orig;                     // an existing track is reported lost by its index before the deletions;
                                                                    // a new persistent one just disappears
          a.calive[gone] = 0;
          cnt[bmax] = cm - 1;
          a.comb[C] = slot; a.cbin[C] = b; a.corig[C] = -1; a.calive[C] = 1;
        }
        if (orig >= 0) n_lost += 1;
        C += 1; act = 1;
        __syncthreads();
        if (lane == 0) cnt[b] += 1;                                 // (b may be the fullest tile's neighbour, not itself: cm > cb + 1)
        __syncthreads();
        // the rescan with `>` from the tile that was fullest: it stays unless another tile now holds more, then the first such
        int best = -1, best_i = 0x7fffffff;
        for (int i = lane; i < n_bins; i += 64)
          if (cnt[i] > best) { best = cnt[i]; best_i = i; }         // (ascending per lane: the lowest index of the lane's maximum)
        for (int d = 32; d > 0; d >>= 1) {
          const int ob = __shfl_xor(best, d, 64), oi = __shfl_xor(best_i, d, 64);
          if (ob > best || (ob == best && oi < best_i)) { best = ob; best_i = oi; }
        }
        if (best > cnt[bmax]) bmax = best_i;
      } else if (L > a.n_poses_max - 1) {
        const int k = a.cand_of[slot];
        if (a.flag[k] != 0) {
          if (lane == 0) a.l_msckf[n_msckf] = k;
          n_msckf += 1;
        }
        act = 2;
      }
    }
    if (lane == 0) a.act[j] = act;
  }
  __syncthreads();
  if (status != 0) {                                                // (cannot happen: every alive position is counted in its tile)
    if (lane == 0) { a.head[XK_TSR_STATUS] = status; a.c[XK_TSC_STATUS] = status; }
    return;
  }
  // ---- the lists, compacted in order; 6. the new persistent tracks MSCKF-SLAM first ----
  const auto new_flag = [&](int p) { return a.flag[a.cand_of[a.comb[p]]] != 0; };
  const int n_slam = xk_ts_wave_compact(n_kept, lane, [&](int p) { return a.calive[p] != 0; }, [&](int p, int pos) { a.slam[pos] = a.comb[p]; });
  const int n_nm = xk_ts_wave_compact(C - n_kept, lane, [&](int i) { return a.calive[n_kept + i] != 0 && new_flag(n_kept + i); },
                                      [&](int i, int pos) { a.newl[pos] = a.comb[n_kept + i]; });
  const int n_ns = xk_ts_wave_compact(C - n_kept, lane, [&](int i) { return a.calive[n_kept + i] != 0 && !new_flag(n_kept + i); },
                                      [&](int i, int pos) { a.newl[n_nm + pos] = a.comb[n_kept + i]; });
  const int n_left = xk_ts_wave_compact(n_opp, lane, [&](int j) { return a.act[j] == 0; }, [&](int j, int pos) { a.opp[pos] = a.sorted[j]; });
  // ---- the freed slots: lost and evicted persistent tracks, evicted new ones, consumed and dead opportunistic ones ----
  int top = a.hdr[XK_TSH_FREE_TOP] - a.c[XK_TSC_STARTED];
  top += xk_ts_wave_compact(n_lost1, lane, [&](int) { return true; }, [&](int i, int pos) { a.free_[top + pos] = a.lost_slot[i]; });
  top += xk_ts_wave_compact(C, lane, [&](int p) { return a.calive[p] == 0; }, [&](int p, int pos) { a.free_[top + pos] = a.comb[p]; });
  top += xk_ts_wave_compact(n_opp, lane, [&](int j) { return a.act[j] == 2; }, [&](int j, int pos) { a.free_[top + pos] = a.sorted[j]; });
  top += xk_ts_wave_compact(n_dead, lane, [&](int) { return true; }, [&](int i, int pos) { a.free_[top + pos] = a.dead[i]; });
  // ---- the five measurement lists behind one another: candidates point into the batch's normalised coordinates ----
  const auto put_cand = [&](int e, int k) {
    a.e_id[e] = a.id[a.cand_slot[k]]; a.e_start[e] = a.norm_off[k]; a.e_len[e] = a.norm_off[k + 1] - a.norm_off[k];
  };
  int e0 = 0;
  for (int i = lane; i < n_msckf; i += 64) put_cand(e0 + i, a.l_msckf[i]);
  e0 += n_msckf;
  for (int i = lane; i < n_short; i += 64) put_cand(e0 + i, a.l_short[i]);
  e0 += n_short;
  __syncthreads();                                                  // (the new list as this wavefront just wrote it)
  for (int i = lane; i < n_ns; i += 64) put_cand(e0 + i, a.cand_of[a.newl[n_nm + i]]);
  e0 += n_ns;
  for (int i = lane; i < n_nm; i += 64) put_cand(e0 + i, a.cand_of[a.newl[i]]);
  e0 += n_nm;
  // the persistent tracks cropped to n_poses_max (and to the ring), normalised here: two IEEE operations per coordinate
  const int crop = a.n_poses_max < XK_TS_RING ? a.n_poses_max : XK_TS_RING;
  int run = n_norm;
  for (int base = 0; base < n_slam; base += 64) {
    const int t = base + lane;
    int L = 0, slot = 0;
    if (t < n_slam) { slot = a.slam[t]; L = a.len[slot]; }
    const int keep = t < n_slam ? (L < crop ? L : crop) : 0;
    int tot;
    const int start = run + xk_ts_wave_excl(keep, lane, &tot);
    if (t < n_slam) { a.e_id[e0 + t] = a.id[slot]; a.e_start[e0 + t] = start; a.e_len[e0 + t] = keep; }
    run += tot;
  }
  __syncthreads();
  for (int t = 0; t < n_slam; ++t) {
    const int slot = a.slam[t], L = a.len[slot], keep = a.e_len[e0 + t], start = a.e_start[e0 + t];
    for (int i = lane; i < keep; i += 64) {
#pragma clang fp contract(off)
      const size_t at = (size_t)slot * XK_TS_RING + (size_t)((L - keep + i) & (XK_TS_RING - 1));
      a.norm_xy[2 * ((size_t)start + i)] = (a.obs[4 * at] - a.cx) / a.fx;
      a.norm_xy[2 * ((size_t)start + i) + 1] = (a.obs[4 * at + 1] - a.cy) / a.fy;
    }
  }
  if (lane == 0) {
    a.hdr[XK_TSH_N_SLAM] = n_slam; a.hdr[XK_TSH_N_NEW] = n_nm + n_ns; a.hdr[XK_TSH_N_OPP] = n_left; a.hdr[XK_TSH_FREE_TOP] = top;
    int *h = a.head;
    for (int j = 0; j < XK_TSR_N; ++j) h[j] = 0;
    h[XK_TSR_N_SLAM] = n_slam; h[XK_TSR_N_NEW] = n_nm + n_ns; h[XK_TSR_N_OPP] = n_left; h[XK_TSR_N_LOST] = n_lost;
    h[XK_TSR_N_MATCHES] = a.n; h[XK_TSR_N_CLAIMED] = a.n - n_opp; h[XK_TSR_N_CAND] = n_cand; h[XK_TSR_N_CAND_OBS] = a.c[XK_TSC_CAND_OBS];
    h[XK_TSR_N_NORM] = n_norm;
    const long long id = *a.next_id;
    h[XK_TSR_NEXT_ID_LO] = (int)(unsigned int)(id & 0xffffffffll); h[XK_TSR_NEXT_ID_HI] = (int)(id >> 32);
    h[XK_TSR_LIST0] = n_msckf; h[XK_TSR_LIST0 + 1] = n_short; h[XK_TSR_LIST0 + 2] = n_ns; h[XK_TSR_LIST0 + 3] = n_nm; h[XK_TSR_LIST0 + 4] = n_slam;
    h[XK_TSR_N_PER_OBS] = run - n_norm;
  }
}

// ---- the store's own entries ----
// everything free again; the id counter stays (TrackManager::clear)
__global__ __launch_bounds__(256) void xk_ts_clear(XkTsArgs a, int reset_id) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.max_tracks) a.free_[i] = a.max_tracks - 1 - i;
  if (i == 0) {
    a.hdr[XK_TSH_N_SLAM] = 0; a.hdr[XK_TSH_N_NEW] = 0; a.hdr[XK_TSH_N_OPP] = 0; a.hdr[XK_TSH_FREE_TOP] = a.max_tracks;
    if (reset_id) *a.next_id = 1;
  }
}

// erase of list entries: which = 0 the persistent list, 1 the new persistent one; idx ascending, n <= XK_TS_REMOVE_MAX, all below the list's length
#define XK_TS_REMOVE_MAX 32
struct XkTsRemove { int which, n, idx[XK_TS_REMOVE_MAX]; };

__global__ __launch_bounds__(64) void xk_ts_remove(XkTsArgs a, XkTsRemove r) {
  const int lane = threadIdx.x;
  int *list = r.which == 0 ? a.slam : a.newl;
  const int N = a.hdr[r.which == 0 ? XK_TSH_N_SLAM : XK_TSH_N_NEW];
  int top = a.hdr[XK_TSH_FREE_TOP];
  const auto gone = [&](int i) {
    bool g = false;
    for (int j = 0; j < r.n; ++j) g = g || r.idx[j] == i;
    return g;
  };
  // a chunk's reads come before its writes, and every write goes to a position at or below the chunk's first: in place
  int run = 0, freed = 0;
  for (int base = 0; base < N; base += 64) {
    const int i = base + lane;
    const int slot = i < N ? list[i] : 0;
    const bool out = i < N && gone(i), keep = i < N && !out;
    const unsigned long long mk = __ballot(keep), mo = __ballot(out);
    const unsigned long long below = (1ull << lane) - 1ull;
    __syncthreads();
    if (keep) list[run + __popcll(mk & below)] = slot;
    if (out) a.free_[top + freed + __popcll(mo & below)] = slot;
    run += __popcll(mk); freed += __popcll(mo);
    __syncthreads();
  }
  if (lane == 0) { a.hdr[r.which == 0 ? XK_TSH_N_SLAM : XK_TSH_N_NEW] = run; a.hdr[XK_TSH_FREE_TOP] = top + freed; }
}

// One of the store's lists gathered for inspection: which = 0 persistent, 1 new persistent, 2 opportunistic.  One wavefront per track:
// its newest <= 64 observations oldest first, rows past them zero.
struct XkTsListOut {
  int which, n;
  long long *ids;                // [n]
  int *lengths;                  // [n] true lengths
  double *obs;                   // [n][64][4]
  int *score;                    // [n][64]
  int *tiles;                    // [n][64][2]
};

__global__ __launch_bounds__(256) void xk_ts_gather(XkTsArgs a, XkTsListOut o) {
  const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= o.n) return;
  const int slot = (o.which == 0 ? a.slam : o.which == 1 ? a.newl : a.opp)[t];
  const int L = a.len[slot], cnt = L < XK_TS_RING ? L : XK_TS_RING;
  const size_t to = (size_t)t * XK_TS_RING + lane;
  if (lane == 0) { o.ids[t] = a.id[slot]; o.lengths[t] = L; }
  if (lane < cnt) {
    const size_t at = (size_t)slot * XK_TS_RING + (size_t)((L - cnt + lane) & (XK_TS_RING - 1));
#pragma unroll
    for (int j = 0; j < 4; ++j) o.obs[4 * to + j] = a.obs[4 * at + j];
    o.score[to] = a.score[at];
    o.tiles[2 * to] = a.tile[2 * at]; o.tiles[2 * to + 1] = a.tile[2 * at + 1];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) o.obs[4 * to + j] = 0.0;
    o.score[to] = 0;
    o.tiles[2 * to] = 0; o.tiles[2 * to + 1] = 0;
  }
}
